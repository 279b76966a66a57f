// fp32 convolution on split-bf16 matrix instructions ("bf16x3"): mcgmil_conv2d_f32's contract --
// NHWC fp32 in, NHWC fp32 out, packed weights, input BatchNorm (INBN), statistics epilogue (STATS)
// -- with every operand split into two bf16 terms and the GEMM run as three
// v_mfma_f32_16x16x32_bf16 products, hi_w * hi_x + hi_w * lo_x + lo_w * hi_x, accumulated in fp32:
// 3/16 of the matrix-pipe cost of v_mfma_f32_16x16x4_f32 per K. The counterpart of
// torch.set_float32_matmul_precision("high") ("bfloat16_3x") for torch.nn.Conv2d.forward in fp32
// (model.py:166-179, the ResNet feature extractor). Numerics contract: include/mcgmil_features.h.
//
// GEMM view: rows = output channels (the A operand, weights), columns = output pixels (the B
// operand, im2col of x), K = (kh, kw, ci) in steps of 32 input channels of one tap. Both operands
// are k-contiguous rows: 32 consecutive input channels of a tap are 128 contiguous bytes of NHWC
// x, and the weights are packed that way. A workgroup of 4 waves computes 128 x 128 (or 64
// channels x 256 pixels when Cout is an odd multiple of 64), each wave 64 x 64 = 4 x 4 tiles of
// 16 x 16. Per K step a wave issues 48 MFMAs against 16 ds_read_b128.
//
// Packed weights: [K step][hi, lo][Cout][32] bf16, split once by the pack kernel; a tile's rows of
// one step and half are contiguous. Activations are split as they are staged: the next step's
// fp32 values wait in registers while the current step computes (as conv32_kernel), then INBN's
// max(fmaf(x, a, b), lo) is applied (bitwise mcgmil_batchnorm_act's; a thread stages the same 8
// channels of every pixel it owns, so their a_c, b_c travel with the step's loads in 4 registers
// each and take no LDS), then the split, then the store to the other LDS stage.
//
// LDS: two stages of [hi, lo][rows][32 bf16] = 64-byte rows without padding (64 KiB in all for
// the 128 + 128 rows, 80 KiB for the 64 + 256: two workgroups per CU); the 16-byte chunk c of row
// r sits at chunk c ^ (-(r >> 2) & 3). A lane's fragment (k = 8 (lane >> 4) .. + 7 of row lane & 15) is one ds_read_b128. Its 16-lane
// groups are lanes {0-3, 12-15} of chunk c with lanes {4-11} of chunk c ^ 1 (64 banks): rows
// 0-3 / 12-15 / 4-7 / 8-11 of a group land on chunks c ^ {0, 1, 1 ^ 3, 1 ^ 2} = four different
// ones, each on slots (4 r + chunk) mod 16 of its own four rows: conflict-free. The staging
// stores are ds_write_b128 (32 banks, groups of 8 consecutive lanes = 2 rows x 4 chunks, slots
// 4 (r & 1) + chunk): conflict-free too.
//
// No split-K and no atomics: every output element has one writer and a fixed summation order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcgmil.h"
#include "../../include/mcgmil_features.h"
#include "mcgmil_conv_tile_stats.h"
#include "mcgmil_error.h"

namespace {

using mcgmil::f32x4;
using mcgmil::tile_stats;
using mcgmil_detail::fail;
using mcgmil_detail::hip_fail;

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

constexpr int kK = 32;           // K step (input channels of one tap): one 16x16x32 MFMA deep
constexpr int kMaxInBnC = 2048;  // INBN: mcgmil_conv2d_f32's limit on in_channels, kept

struct X3Geom {
    int N, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW;
    long long P;          // N * OH * OW output pixels
    int KS;               // K steps: KH * KW * Cin / 32
    const float* in_ab;   // INBN: [2][Cin] a_c then b_c
    float in_lo;          // INBN: floor after the BatchNorm, 0 (ReLU) or -inf
    float* stats;         // STATS: [pixel tiles][3][Cout] (count, mean, M2)
};

template <int WCO, int WPX>
struct Tile {
    static constexpr int BN_CO = 64 * WCO, BM_PX = 64 * WPX;
    static constexpr int HALF = (BN_CO + BM_PX) * kK;      // bf16 of a stage's hi (or lo) image
    static constexpr int STAGE = 2 * HALF;                 // bf16 per stage
    static_assert(WCO * WPX == 4 && WCO + WPX <= 5, "4 waves, 256 or 320 rows");
};

// v = hi + lo + r with hi = bf16_rne(v), lo = bf16_rne(v - float(hi)) (the subtraction is exact)
__device__ __forceinline__ void split8(const f32x4& v0, const f32x4& v1, u32x4& hi, u32x4& lo) {
    bf16x8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = e < 4 ? v0[e] : v1[e - 4];
        h[e] = (__bf16)v;
        l[e] = (__bf16)(v - (float)h[e]);
    }
    hi = __builtin_bit_cast(u32x4, h);
    lo = __builtin_bit_cast(u32x4, l);
}

// element offset of the 16-byte chunk `chunk` of row `row` in a [rows][32] bf16 image
__device__ __forceinline__ int swz(int row, int chunk) { return row * kK + 8 * (chunk ^ (-(row >> 2) & 3)); }

template <int WCO, int WPX, bool INBN, bool STATS>
__global__ __launch_bounds__(256, 2) void conv32x3_kernel(const X3Geom g, const float* __restrict__ x,
                                                          const __bf16* __restrict__ w, float* __restrict__ y) {
    using T = Tile<WCO, WPX>;
    extern __shared__ __attribute__((aligned(16))) __bf16 smem_x3[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wco = wave % WCO, wpx = wave / WCO;
    const long long px0 = (long long)blockIdx.x * T::BM_PX;
    const int co0 = blockIdx.y * T::BN_CO;

    // Staging map: thread -> 16-byte chunk sch (8 channels) of rows srow + 64 r, of A and of B
    const int srow = tid >> 2, sch = tid & 3;
    // the thread's B pixels: offset of the image in x, and the window's first row and column; a
    // pixel past the last gets a first row no tap brings into the image, so it stages zeros
    long long xoff[WPX];
    int ih0[WPX], iw0[WPX];
    {
        const long long ohw = (long long)g.OH * g.OW;
#pragma unroll
        for (int r = 0; r < WPX; ++r) {
            const long long p = px0 + srow + 64 * r;
            xoff[r] = 0;
            ih0[r] = -(1 << 24);
            iw0[r] = 0;
            if (p < g.P) {
                const int n = (int)(p / ohw);
                const int rem = (int)(p - (long long)n * ohw);
                const int oh = rem / g.OW;
                xoff[r] = (long long)n * g.H * g.W * g.Cin;
                ih0[r] = oh * g.stride - g.pad;
                iw0[r] = (rem - oh * g.OW) * g.stride - g.pad;
            }
        }
    }
    const int cchunks = g.Cin / kK;

    u32x4 ra[WCO][2];     // A: hi and lo chunks
    f32x4 rb[WPX][2];     // B: the chunk's 8 fp32 values
    unsigned bin = 0;     // bit r: the staged B chunk of row r is in-image x (padding stays 0)
    f32x4 na[2], nb[2];   // INBN: a_c, b_c of the staged chunk's 8 channels
    auto load = [&](int ks) {
        // A: packed weights [KS][2][Cout][32], rows co0 + srow + 64 r of this step
        const __bf16* wk = w + ((long long)ks * 2 * g.Cout + co0 + srow) * kK + 8 * sch;
#pragma unroll
        for (int r = 0; r < WCO; ++r) {
            ra[r][0] = *reinterpret_cast<const u32x4*>(wk + (long long)64 * r * kK);
            ra[r][1] = *reinterpret_cast<const u32x4*>(wk + ((long long)g.Cout + 64 * r) * kK);
        }
        // B: x[n, ih, iw, ci .. ci + 7] of the thread's pixels (zero outside the image)
        const int tap = ks / cchunks, ci = (ks - tap * cchunks) * kK + 8 * sch;
        const int kh = tap / g.KW, kw = tap - kh * g.KW;
        bin = 0;
        if constexpr (INBN) {   // one chunk of channels per thread and step: L1/L2 hits, no LDS copy
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                na[h] = *reinterpret_cast<const f32x4*>(g.in_ab + ci + 4 * h);
                nb[h] = *reinterpret_cast<const f32x4*>(g.in_ab + g.Cin + ci + 4 * h);
            }
        }
#pragma unroll
        for (int r = 0; r < WPX; ++r) {
            const int ih = ih0[r] + kh, iw = iw0[r] + kw;
            const bool in = ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
            if (in) {
                const float* src = x + xoff[r] + ((long long)ih * g.W + iw) * g.Cin + ci;
                rb[r][0] = *reinterpret_cast<const f32x4*>(src);
                rb[r][1] = *reinterpret_cast<const f32x4*>(src + 4);
                bin |= 1u << r;
            } else {
                rb[r][0] = rb[r][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    auto store = [&](__bf16* st) {
        __bf16* As = st + swz(srow, sch);                    // rows + 64 r keep the swizzle
        __bf16* Bs = As + T::BN_CO * kK;
#pragma unroll
        for (int r = 0; r < WCO; ++r) {
            *reinterpret_cast<u32x4*>(As + 64 * r * kK) = ra[r][0];
            *reinterpret_cast<u32x4*>(As + 64 * r * kK + T::HALF) = ra[r][1];
        }
#pragma unroll
        for (int r = 0; r < WPX; ++r) {
            if constexpr (INBN) {   // bitwise mcgmil_batchnorm_act's max(fmaf(x, a, b), lo)
                if (bin >> r & 1) {
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int e = 0; e < 4; ++e) rb[r][h][e] = fmaxf(fmaf(rb[r][h][e], na[h][e], nb[h][e]), g.in_lo);
                }
            }
            u32x4 hi, lo;
            split8(rb[r][0], rb[r][1], hi, lo);
            *reinterpret_cast<u32x4*>(Bs + 64 * r * kK) = hi;
            *reinterpret_cast<u32x4*>(Bs + 64 * r * kK + T::HALF) = lo;
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int kl = lane >> 4, cl = lane & 15;
    const int afrag = swz(wco * 64 + cl, kl), bfrag = T::BN_CO * kK + swz(wpx * 64 + cl, kl);
    load(0);
    store(smem_x3);
    __syncthreads();
    for (int ks = 0; ks < g.KS; ++ks) {
        const __bf16* st = smem_x3 + (ks & 1) * T::STAGE;
        if (ks + 1 < g.KS) load(ks + 1);
        bf16x8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ah[i] = *reinterpret_cast<const bf16x8*>(st + afrag + 16 * i * kK);
            al[i] = *reinterpret_cast<const bf16x8*>(st + afrag + 16 * i * kK + T::HALF);
            bh[i] = *reinterpret_cast<const bf16x8*>(st + bfrag + 16 * i * kK);
            bl[i] = *reinterpret_cast<const bf16x8*>(st + bfrag + 16 * i * kK + T::HALF);
        }
        // term by term, so 16 independent MFMAs lie between two on the same accumulator
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
        if (ks + 1 < g.KS) store(smem_x3 + ((ks + 1) & 1) * T::STAGE);
        __syncthreads();
    }

    // D tile (i, j): lane holds channels co0 + wco*64 + 16 i + 4 (lane >> 4) + v of pixel
    // px0 + wpx*64 + 16 j + (lane & 15)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long pp = px0 + wpx * 64 + 16 * j + cl;
        if (pp >= g.P) continue;
        float* yp = y + pp * g.Cout + co0 + wco * 64 + 4 * kl;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(yp + 16 * i) = acc[i][j];
    }
    if constexpr (STATS) {   // the stages are free: the K loop ended with a barrier
        const long long left = g.P - (px0 + wpx * 64);
        tile_stats<T::BN_CO, WPX>(acc, left < 0 ? 0 : (left > 64 ? 64 : (int)left), wco, wpx, lane,
                                  reinterpret_cast<float*>(smem_x3), g.stats, blockIdx.x, g.Cout, co0);
    }
}

// torch layout [Cout, Cin, KH, KW] fp32 -> [KS][2][Cout][32] bf16: K step ks = (kh*KW + kw) *
// (Cin/32) + ci/32, element k = ci % 32; half 0 = hi, half 1 = lo of the split
__global__ void pack_conv32x3_kernel(const float* w, int Cout, int Cin, int KH, int KW, int KS, __bf16* out) {
    const long long total = (long long)KS * Cout * kK;
    const int cchunks = Cin / kK;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % kK);
        const int co = (int)(i / kK % Cout);
        const long long ks = i / kK / Cout;
        const int tap = (int)(ks / cchunks), ci = (int)(ks % cchunks) * kK + k;
        const int kh = tap / KW, kw = tap % KW;
        const float v = w[(((long long)co * Cin + ci) * KH + kh) * KW + kw];
        const __bf16 hi = (__bf16)v;
        out[((ks * 2 + 0) * Cout + co) * kK + k] = hi;
        out[((ks * 2 + 1) * Cout + co) * kK + k] = (__bf16)(v - (float)hi);
    }
}

int validate_x3(const mcgmil_conv_args* a, X3Geom* g) {
    if (!a) return fail(MCGMIL_E_INVALID, "args is NULL");
    if (a->batch < 1 || a->height < 1 || a->width < 1)
        return fail(MCGMIL_E_INVALID, "batch, height and width must be >= 1");
    if (a->in_channels < 1 || a->out_channels < 64 || a->out_channels % 64 != 0)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16x3 convolution: out_channels a multiple of 64");
    if (a->in_channels % kK != 0)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16x3 convolution: in_channels a multiple of 32");
    if (a->kernel_h < 1 || a->kernel_w < 1 || a->kernel_h > 7 || a->kernel_w > 7)
        return fail(MCGMIL_E_UNSUPPORTED, "kernel size must be in 1..7");
    if (a->stride < 1 || a->pad < 0 || a->pad > 64) return fail(MCGMIL_E_INVALID, "stride >= 1 and 0 <= pad <= 64");
    if (a->in_ab && a->in_channels > kMaxInBnC)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16x3 convolution: in_ab needs in_channels <= 2048");
    if (a->in_relu != 0 && a->in_relu != 1) return fail(MCGMIL_E_INVALID, "in_relu must be 0 or 1");
    const long long oh = ((long long)a->height + 2 * a->pad - a->kernel_h) / a->stride + 1;
    const long long ow = ((long long)a->width + 2 * a->pad - a->kernel_w) / a->stride + 1;
    if (oh < 1 || ow < 1) return fail(MCGMIL_E_INVALID, "the kernel does not fit the padded input");
    const long long P = (long long)a->batch * oh * ow;
    if (P >= (1ll << 31) - 256) return fail(MCGMIL_E_UNSUPPORTED, "too many output pixels");
    if (g) {
        g->N = a->batch; g->H = a->height; g->W = a->width; g->Cin = a->in_channels;
        g->Cout = a->out_channels; g->KH = a->kernel_h; g->KW = a->kernel_w;
        g->stride = a->stride; g->pad = a->pad; g->OH = (int)oh; g->OW = (int)ow; g->P = P;
        g->KS = a->kernel_h * a->kernel_w * (a->in_channels / kK);
        g->in_ab = a->in_ab;
        g->in_lo = a->in_relu ? 0.f : -INFINITY;
        g->stats = a->stats;
    }
    return MCGMIL_OK;
}

template <int WCO, int WPX>
long long pixel_tiles(const X3Geom& g) { return (g.P + Tile<WCO, WPX>::BM_PX - 1) / Tile<WCO, WPX>::BM_PX; }

// 128 x 128 tiles when Cout is a multiple of 128, else 64 x 256
bool wide_co(const X3Geom& g) { return g.Cout % 128 == 0; }

template <int WCO, int WPX, bool INBN, bool STATS>
int launch_x3(const X3Geom& g, const float* x, const __bf16* w, float* y, hipStream_t s) {
    using T = Tile<WCO, WPX>;
    constexpr size_t lds = (size_t)2 * T::STAGE * sizeof(__bf16);
    if constexpr (lds > 64 * 1024)   // the 64 x 256 tile: 80 KiB
        if (int rc = mcgmil_detail::raise_lds_limit(reinterpret_cast<const void*>(&conv32x3_kernel<WCO, WPX, INBN, STATS>),
                                                    "conv32x3_kernel LDS limit"))
            return rc;
    dim3 grid((unsigned)pixel_tiles<WCO, WPX>(g), (unsigned)(g.Cout / T::BN_CO));
    hipLaunchKernelGGL((conv32x3_kernel<WCO, WPX, INBN, STATS>), grid, dim3(256), lds, s, g, x, w, y);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCGMIL_OK : hip_fail(e, "conv32x3_kernel launch");
}

template <int WCO, int WPX>
int dispatch_x3(const X3Geom& g, const float* x, const __bf16* w, float* y, hipStream_t s) {
    const bool st = g.stats != nullptr;
    if (g.in_ab)
        return st ? launch_x3<WCO, WPX, true, true>(g, x, w, y, s) : launch_x3<WCO, WPX, true, false>(g, x, w, y, s);
    return st ? launch_x3<WCO, WPX, false, true>(g, x, w, y, s) : launch_x3<WCO, WPX, false, false>(g, x, w, y, s);
}

}  // namespace

extern "C" {

int mcgmil_pack_conv_weights_f32x3(const mcgmil_conv_args* a, const void* weight, void* packed, void* stream) {
    X3Geom g;
    if (int rc = validate_x3(a, &g)) return rc;
    if (!weight || !packed) return fail(MCGMIL_E_INVALID, "NULL weight or packed pointer");
    if (((uintptr_t)weight & 3u) || ((uintptr_t)packed & 15u))
        return fail(MCGMIL_E_ALIGN, "weight must be 4-byte and packed 16-byte aligned");
    const long long total = (long long)g.KS * kK * a->out_channels;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_conv32x3_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const float*>(weight), a->out_channels, a->in_channels, a->kernel_h,
                       a->kernel_w, g.KS, static_cast<__bf16*>(packed));
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCGMIL_OK : hip_fail(e, "pack_conv32x3_kernel launch");
}

int mcgmil_conv_packed_size_f32x3(const mcgmil_conv_args* a, size_t* floats) {
    X3Geom g;
    if (int rc = validate_x3(a, &g)) return rc;
    if (!floats) return fail(MCGMIL_E_INVALID, "floats is NULL");
    *floats = (size_t)g.KS * kK * a->out_channels;   // a hi and a lo bf16 per weight: 4 bytes
    return MCGMIL_OK;
}

int mcgmil_conv_stats_parts_f32x3(const mcgmil_conv_args* a, int32_t* parts) {
    X3Geom g;
    if (int rc = validate_x3(a, &g)) return rc;
    if (!parts) return fail(MCGMIL_E_INVALID, "parts is NULL");
    const long long t = wide_co(g) ? pixel_tiles<2, 2>(g) : pixel_tiles<1, 4>(g);
    if (t > 0x7fffffffll) return fail(MCGMIL_E_UNSUPPORTED, "too many pixel tiles");
    *parts = (int32_t)t;
    return MCGMIL_OK;
}

int mcgmil_conv2d_f32x3(const mcgmil_conv_args* a, void* stream) {
    X3Geom g;
    if (int rc = validate_x3(a, &g)) return rc;
    if (!a->x || !a->w || !a->y) return fail(MCGMIL_E_INVALID, "NULL x, w or y");
    if (((uintptr_t)a->x | (uintptr_t)a->w | (uintptr_t)a->y | (uintptr_t)a->in_ab) & 15u)
        return fail(MCGMIL_E_ALIGN, "x, w, y and in_ab must be 16-byte aligned");
    if ((uintptr_t)a->stats & 3u) return fail(MCGMIL_E_ALIGN, "stats must be 4-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const float* x = static_cast<const float*>(a->x);
    const __bf16* w = static_cast<const __bf16*>(a->w);
    float* y = static_cast<float*>(a->y);
    return wide_co(g) ? dispatch_x3<2, 2>(g, x, w, y, s) : dispatch_x3<1, 4>(g, x, w, y, s);
}

}  // extern "C"
