// bf16x3 weight gradient of the backbone's fp32 block convolutions (include/mcgmil_conv_grad_x3.h):
// the backward of mcgmil_conv2d_f32x3 with respect to its weight, with fp32 x, dY and dW and the
// GEMM on three v_mfma_f32_16x16x32_bf16 products per K. Reference: loss.backward() through
// torch.nn.Conv2d in fp32 (model.py:166-179, the ResNet feature extractor under
// net_utils.train_gacc) at torch.set_float32_matmul_precision("high") ("bfloat16_3x").
//
// The GEMM view, the tiles, the granules and the reduce are those of mcgmil_conv_grad_bf16.hip:
// rows = output channels o (the A operand, dY), columns = (kh, kw, ci) of the weight (the B
// operand, the tap-shifted x), K = output pixels in steps of 32; a workgroup of 4 waves computes a
// 128 x 128 tile (64 x 256 when Cout is not a multiple of 128) of one granule of
// MCGMIL_WGRAD_GRANULE_PIXELS output pixels, each wave a 64 x 64 block; every (tile, granule)
// writes its partial sums to the workspace as [granule][column][o] and wgrad_x3_reduce_kernel adds
// them in granule order. No atomics.
//
// What differs is the operand path. The rows are fp32: a thread's chunk of 8 k-major values is two
// 16-byte global loads, held in registers while the current K step computes. When the step is
// staged every value v is split by the numerics contract of include/mcgmil_features.h, hi =
// bf16_rne(v), lo = bf16_rne(v - float(hi)) (the subtraction is exact), and the 8 hi and the 8 lo
// go with one 16-byte LDS write each into a hi image and a lo image of the operand: a stage is
// [A hi][A lo][B hi][B lo] with the bf16 kernel's [32][BM + 16] and [32][BN + 16] rows, 36,864 B for
// the 128 x 128 tile and 45,056 B for the 64 x 256 one. Zero padding, stride-2 taps, columns past
// kh*kw*Cin and pixels past the granule are zeros written when a row is staged (0 splits into 0, 0).
//
// LDS and occupancy: the 128 x 128 tile keeps two stages (73,728 B), so two workgroups per CU take
// 147,456 of the 163,840 B and a K step costs one barrier. Two stages of the 64 x 256 tile would be
// 90,112 B, one workgroup per CU; it keeps ONE stage (45,056 B, two workgroups per CU) and pays a
// second barrier per K step instead: the next step still waits in registers under the MFMAs, only
// its LDS write is no longer overlapped. The tile serves Cout = 64 and odd multiples of 64 alone.
//
// Fragments are read with ds_read_b64_tr_b16 exactly as the bf16 kernel reads them: per 16-lane
// group a block of 4 k rows x 16 columns comes back column-major; group g takes rows 4g + q and
// 16 + 4g + q (q = 0..3) of both operands, so the two groups of a 32-lane half read 8 rows that are
// consecutive mod 8, and with a row stride of 32 bytes mod 256 (the 16-element pad) those land on 8
// different 32-byte bank slots. Every address is 8-byte aligned and every lane of a reading wave
// supplies one: the `active` skip is wave-uniform, there is no lane-dependent guard around a read.
//
// Per fragment pair three MFMAs into one accumulator, in this order: dy_hi * x_hi, dy_hi * x_lo,
// dy_lo * x_hi. The lo * lo term (below 2^-16 of the product) is dropped. The order is fixed, the
// split is a pure function of the value and the granules do not depend on the device or on
// chunk_pixels, so two calls agree bitwise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcgmil.h"
#include "../../include/mcgmil_conv_grad_x3.h"
#include "mcgmil_error.h"

namespace {

using mcgmil_detail::fail;
using mcgmil_detail::hip_fail;

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) short i16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

constexpr int kK = 32;     // K step (output pixels): one v_mfma_f32_16x16x32_bf16 deep
constexpr int kPad = 16;   // LDS row pad (bf16 elements): 32 bytes, see the bank note above
constexpr int kGranule = MCGMIL_WGRAD_GRANULE_PIXELS;
static_assert(kGranule % kK == 0, "a granule is a whole number of K steps");

struct WGeom {
    int N, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW;
    int Ncols;            // KH * KW * Cin
    long long P;          // N * OH * OW output pixels
};

template <int WCO, int WN>
struct Tile {
    static constexpr int BM = 64 * WCO, BN = 64 * WN;
    static constexpr int AS = BM + kPad, BS = BN + kPad;                     // row strides (bf16)
    static constexpr int AIMG = kK * AS, BIMG = kK * BS;                     // bf16 per hi (or lo) image
    static constexpr int STAGE = 2 * (AIMG + BIMG);                          // bf16 per stage
    static constexpr int STAGES = WCO == 2 ? 2 : 1;                          // see "LDS and occupancy"
    static constexpr size_t LDS = (size_t)STAGES * STAGE * sizeof(__bf16);
    static constexpr int A8 = kK * BM / 8 / 256, B8 = kK * BN / 8 / 256;     // 8-value chunks per thread
    static_assert(A8 >= 1 && B8 >= 1 && 256 % (BN / 8) == 0 && 256 % (BM / 8) == 0, "staging map");
    // an odd number of 32-byte slots per row: 8 consecutive rows hit 8 different slots of the 256
    static_assert((AS * 2) % 64 == 32 && (BS * 2) % 64 == 32, "LDS row stride and the banks");
    static_assert(2 * LDS <= 160 * 1024, "two workgroups per CU");
};

// The 4 x 16 block at p (this lane's row and 4 columns of it), column-major: ds_read_b64_tr_b16.
__device__ __forceinline__ i16x4 read_tr(const __bf16* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)p);
}

// The 8-k operand of this lane: the blocks at p (k rows 4g + q) and 16 rows below (16 + 4g + q).
__device__ __forceinline__ bf16x8 read_frag(const __bf16* p, int stride) {
    const i16x4 lo = read_tr(p), hi = read_tr(p + 16 * stride);
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

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

// The LDS figures DESIGN.md §4 states, held by the compiler (tests/test_conv_grad_x3_codegen.py compiles this file)
static_assert(Tile<2, 2>::STAGE * sizeof(__bf16) == 36864 && Tile<2, 2>::LDS == 73728, "128 x 128: two stages");
static_assert(Tile<1, 4>::STAGE * sizeof(__bf16) == 45056 && Tile<1, 4>::LDS == 45056, "64 x 256: one stage");

// part: [granules of the chunk][Ncols][Cout]. pix0: the chunk's first output pixel (a multiple of
// the granule). tiles = tiles_n * (Cout / BM); blockIdx.x = tile + tiles * (granule in the chunk).
template <int WCO, int WN>
__global__ __launch_bounds__(256, 2) void wgrad_x3_kernel(const WGeom g, const float* __restrict__ x,
                                                          const float* __restrict__ dy, float* __restrict__ part,
                                                          long long pix0, int tiles_n, int tiles) {
    using T = Tile<WCO, WN>;
    extern __shared__ __attribute__((aligned(16))) __bf16 smem_wx3[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wco = wave % WCO, wn = wave / WCO;
    const int tile = blockIdx.x % tiles, gl = blockIdx.x / tiles;
    const int tn = tile % tiles_n, tm = tile / tiles_n;
    const int co0 = tm * T::BM, n0 = tn * T::BN;
    const long long pbeg = pix0 + (long long)gl * kGranule;
    const long long pend = pbeg + kGranule < g.P ? pbeg + kGranule : g.P;
    const int steps = (int)((pend - pbeg + kK - 1) / kK);

    // A staging: chunk ac8 (8 output channels) of row ak + AKSTEP r of the step's 32 dY rows
    const int ak = tid / (T::BM / 8), ac8 = tid % (T::BM / 8);
    constexpr int AKSTEP = 256 / (T::BM / 8);
    // B staging: chunk bc8 (one tap, 8 input channels: the same for every r) of row bk + BKSTEP r
    const int bk = tid / (T::BN / 8), bc8 = tid % (T::BN / 8);
    constexpr int BKSTEP = 256 / (T::BN / 8);
    const int col = n0 + 8 * bc8;
    const bool cvalid = col < g.Ncols;                 // Cin % 8 == 0: a chunk never straddles a tap
    const int tap = cvalid ? col / g.Cin : 0;
    const int ci = cvalid ? col - tap * g.Cin : 0;
    const int kh = tap / g.KW, kw = tap - kh * g.KW;
    const unsigned ohw = (unsigned)(g.OH * g.OW);

    f32x4 ra[T::A8][2], rb[T::B8][2];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    auto load = [&](int ks) {
        const long long ps = pbeg + (long long)ks * kK;
#pragma unroll
        for (int r = 0; r < T::A8; ++r) {
            const long long p = ps + ak + AKSTEP * r;
            const float* src = dy + p * g.Cout + co0 + 8 * ac8;
            ra[r][0] = p < pend ? *reinterpret_cast<const f32x4*>(src) : zero;
            ra[r][1] = p < pend ? *reinterpret_cast<const f32x4*>(src + 4) : zero;
        }
#pragma unroll
        for (int r = 0; r < T::B8; ++r) {
            const long long p = ps + bk + BKSTEP * r;
            bool in = cvalid && p < pend;
            const unsigned pu = in ? (unsigned)p : 0u;      // P < 2^31
            const unsigned n = pu / ohw, rem = pu - n * ohw;
            const unsigned oh = rem / (unsigned)g.OW, ow = rem - oh * (unsigned)g.OW;
            const int ih = (int)oh * g.stride - g.pad + kh, iw = (int)ow * g.stride - g.pad + kw;
            in = in && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
            const float* src = x + (((long long)n * g.H + (in ? ih : 0)) * g.W + (in ? iw : 0)) * g.Cin + ci;
            rb[r][0] = in ? *reinterpret_cast<const f32x4*>(src) : zero;
            rb[r][1] = in ? *reinterpret_cast<const f32x4*>(src + 4) : zero;
        }
    };
    auto store = [&](__bf16* st) {
        __bf16* As = st;
        __bf16* Bs = st + 2 * T::AIMG;
#pragma unroll
        for (int r = 0; r < T::A8; ++r) {
            u32x4 hi, lo;
            split8(ra[r][0], ra[r][1], hi, lo);
            __bf16* d = As + (ak + AKSTEP * r) * T::AS + 8 * ac8;
            *reinterpret_cast<u32x4*>(d) = hi;
            *reinterpret_cast<u32x4*>(d + T::AIMG) = lo;
        }
#pragma unroll
        for (int r = 0; r < T::B8; ++r) {
            u32x4 hi, lo;
            split8(rb[r][0], rb[r][1], hi, lo);
            __bf16* d = Bs + (bk + BKSTEP * r) * T::BS + 8 * bc8;
            *reinterpret_cast<u32x4*>(d) = hi;
            *reinterpret_cast<u32x4*>(d + T::BIMG) = lo;
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // transposed-read address of this lane: group gq = lane >> 4 takes k rows 4 gq + q (first read)
    // and 16 + 4 gq + q (second), lane 4q + p of the group supplies row q, columns 4p .. 4p + 3
    const int kl = lane >> 4, cl = lane & 15;
    const int trow = 4 * kl + (cl >> 2), tcol = 4 * (cl & 3);
    const bool active = n0 + wn * 64 < g.Ncols;    // wave-uniform
    load(0);
    store(smem_wx3);
    __syncthreads();
    for (int ks = 0; ks < steps; ++ks) {
        const __bf16* st = smem_wx3 + (T::STAGES == 2 ? (ks & 1) * T::STAGE : 0);
        const __bf16* As = st + trow * T::AS + wco * 64 + tcol;
        const __bf16* Bs = st + 2 * T::AIMG + trow * T::BS + wn * 64 + tcol;
        if (ks + 1 < steps) load(ks + 1);
        if (active) {
            bf16x8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ah[i] = read_frag(As + 16 * i, T::AS);
                al[i] = read_frag(As + T::AIMG + 16 * i, T::AS);
                bh[i] = read_frag(Bs + 16 * i, T::BS);
                bl[i] = read_frag(Bs + T::BIMG + 16 * i, T::BS);
            }
            // term by term, so 16 independent MFMAs lie between two on the same accumulator
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
            // -DMCGMIL_WX3_HI_ONLY is the ablation of DESIGN.md §4, never the shipped library: python -c "from mcgmil
            // import _build; _build.build(force=True, out='abvar/libmcgmil_wx3_hi_only.so', defines=('MCGMIL_WX3_HI_ONLY',))"
            // gives a build that stops after the hi * hi products, for scripts/bench_conv_grad_x3.py --ablate-lib
#ifndef MCGMIL_WX3_HI_ONLY
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
#endif
        }
        if constexpr (T::STAGES == 1) __syncthreads();   // every wave is done reading the one stage
        if (ks + 1 < steps) store(smem_wx3 + (T::STAGES == 2 ? ((ks + 1) & 1) * T::STAGE : 0));
        __syncthreads();
    }

    // D tile (i, j): lane holds o = co0 + wco*64 + 16 i + 4 (lane >> 4) + v of column
    // n0 + wn*64 + 16 j + (lane & 15)
    float* pg = part + (long long)gl * g.Ncols * g.Cout;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int nn = n0 + wn * 64 + 16 * j + cl;
        if (nn >= g.Ncols) continue;
        float* pp = pg + (long long)nn * g.Cout + co0 + wco * 64 + 4 * kl;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(pp + 16 * i) = acc[i][j];
    }
}

// sum[e] (+)= part[0][e] + part[1][e] + ... in granule order, one element per thread; the last
// chunk writes dW[o][ci][kh][kw] instead of the running sum. e = column * Cout + o. (A private copy
// of the bf16 weight gradient's reduce: the two files share no code on purpose.)
__global__ __launch_bounds__(256) void wgrad_x3_reduce_kernel(const float* __restrict__ part, float* __restrict__ sum,
                                                              float* __restrict__ dw, long long E, int granules,
                                                              int first, int last, int Cout, int Cin, int KH, int KW) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float s = first ? 0.f : sum[e];
    for (int gi = 0; gi < granules; ++gi) s += part[(long long)gi * E + e];
    if (!last) {
        sum[e] = s;
        return;
    }
    const int o = (int)(e % Cout);
    const int c = (int)(e / Cout);
    const int tap = c / Cin, ci = c - tap * Cin;
    const int kh = tap / KW, kw = tap - kh * KW;
    dw[(((long long)o * Cin + ci) * KH + kh) * KW + kw] = s;
}

struct Plan {
    WGeom g;
    long long E;                       // Cout * Ncols
    long long gran_total, gran_chunk;
    int tiles_n, tiles;
    bool wide;                         // 128 x 128 tiles (Cout % 128 == 0), else 64 x 256
    size_t total;                      // workspace bytes
};

int plan_for(const mcgmil_conv_grad_args* a, Plan& pl) {
    if (!a) return fail(MCGMIL_E_INVALID, "args is NULL");
    const mcgmil_conv_args& f = a->fwd;
    if (a->reserved != 0) return fail(MCGMIL_E_INVALID, "reserved must be 0");
    if (a->chunk_pixels < 0) return fail(MCGMIL_E_INVALID, "chunk_pixels must be >= 0");
    if (f.in_ab) return fail(MCGMIL_E_UNSUPPORTED, "bf16x3 weight gradient: in_ab must be NULL (no input BatchNorm)");
    if (f.batch < 1 || f.height < 1 || f.width < 1)
        return fail(MCGMIL_E_INVALID, "batch, height and width must be >= 1");
    if (f.in_channels < 32 || f.in_channels % 32 != 0)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16x3 weight gradient: in_channels a multiple of 32");
    if (f.out_channels < 64 || f.out_channels % 64 != 0)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16x3 weight gradient: out_channels a multiple of 64");
    if (f.kernel_h < 1 || f.kernel_w < 1 || f.kernel_h > 7 || f.kernel_w > 7)
        return fail(MCGMIL_E_UNSUPPORTED, "kernel size must be in 1..7");
    if (f.stride != 1 && f.stride != 2) return fail(MCGMIL_E_UNSUPPORTED, "bf16x3 weight gradient: stride 1 or 2");
    if (f.pad < 0) return fail(MCGMIL_E_INVALID, "pad must be >= 0");
    if (f.pad >= f.kernel_h || f.pad >= f.kernel_w)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16x3 weight gradient: pad must be smaller than the kernel");
    const long long oh = ((long long)f.height + 2ll * f.pad - f.kernel_h) / f.stride + 1;
    const long long ow = ((long long)f.width + 2ll * f.pad - f.kernel_w) / f.stride + 1;
    if ((long long)f.height + 2ll * f.pad < f.kernel_h || (long long)f.width + 2ll * f.pad < f.kernel_w || oh < 1 || ow < 1)
        return fail(MCGMIL_E_INVALID, "the kernel does not fit the padded input");
    long long P = 0, xel = 0, ohw = 0;
    if (__builtin_mul_overflow(oh, ow, &ohw) || ohw >= (1ll << 31) || __builtin_mul_overflow(ohw, (long long)f.batch, &P) ||
        P >= (1ll << 31) - 256)
        return fail(MCGMIL_E_UNSUPPORTED, "too many output pixels (batch * OH * OW must be < 2^31 - 256)");
    if (__builtin_mul_overflow((long long)f.batch * f.height, (long long)f.width * f.in_channels, &xel) ||
        xel >= (1ll << 60) || P * f.out_channels >= (1ll << 60))
        return fail(MCGMIL_E_UNSUPPORTED, "x or dy too large");
    WGeom& g = pl.g;
    g.N = f.batch; g.H = f.height; g.W = f.width; g.Cin = f.in_channels; g.Cout = f.out_channels;
    g.KH = f.kernel_h; g.KW = f.kernel_w; g.stride = f.stride; g.pad = f.pad;
    g.OH = (int)oh; g.OW = (int)ow; g.P = P;
    const long long ncols = (long long)f.kernel_h * f.kernel_w * f.in_channels;
    if (ncols >= (1ll << 30) || ncols * f.out_channels >= (1ll << 34))
        return fail(MCGMIL_E_UNSUPPORTED, "weight too large (out * kh * kw * in must be < 2^34)");
    g.Ncols = (int)ncols;
    pl.E = ncols * f.out_channels;
    pl.wide = f.out_channels % 128 == 0;
    const int BM = pl.wide ? 128 : 64, BN = pl.wide ? 128 : 256;
    pl.tiles_n = (int)((ncols + BN - 1) / BN);
    pl.tiles = pl.tiles_n * (f.out_channels / BM);       // <= E / 2048 < 2^23
    pl.gran_total = (P + kGranule - 1) / kGranule;       // < 2^20
    const long long ebytes = pl.E * 4;                   // a multiple of 8192
    long long gc = a->chunk_pixels ? a->chunk_pixels / kGranule : MCGMIL_WGRAD_DEFAULT_PARTIAL_BYTES / ebytes;
    if (gc < 1) gc = 1;
    if (gc > pl.gran_total) gc = pl.gran_total;
    const long long grid_cap = ((1ll << 31) - 1) / pl.tiles;
    if (gc > grid_cap) gc = grid_cap;
    pl.gran_chunk = gc;
    long long total = 0;
    if (__builtin_mul_overflow(gc + 1, ebytes, &total) || total >= (1ll << 46))
        return fail(MCGMIL_E_UNSUPPORTED, "weight-gradient workspace too large (lower chunk_pixels)");
    pl.total = (size_t)total;
    return MCGMIL_OK;
}

template <int WCO, int WN>
int launch_wgrad(const Plan& pl, const float* x, const float* dy, float* part, long long pix0, long long granules,
                 hipStream_t s) {
    using T = Tile<WCO, WN>;
    if constexpr (T::LDS > 64 * 1024)   // the 128 x 128 tile's two stages: 72 KiB
        if (int rc = mcgmil_detail::raise_lds_limit(reinterpret_cast<const void*>(&wgrad_x3_kernel<WCO, WN>),
                                                    "wgrad_x3_kernel LDS limit"))
            return rc;
    hipLaunchKernelGGL((wgrad_x3_kernel<WCO, WN>), dim3((unsigned)(granules * pl.tiles)), dim3(256), T::LDS, s, pl.g,
                       x, dy, part, pix0, pl.tiles_n, pl.tiles);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCGMIL_OK : hip_fail(e, "wgrad_x3_kernel launch");
}

}  // namespace

extern "C" {

int mcgmil_conv_wgrad_workspace_size_f32x3(const mcgmil_conv_grad_args* a, size_t* bytes) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!bytes) return fail(MCGMIL_E_INVALID, "bytes is NULL");
    *bytes = pl.total;
    return MCGMIL_OK;
}

int mcgmil_conv2d_wgrad_f32x3(const mcgmil_conv_grad_args* a, void* stream) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!a->fwd.x || !a->dy || !a->dw) return fail(MCGMIL_E_INVALID, "NULL x, dy or dw");
    if (((uintptr_t)a->fwd.x | (uintptr_t)a->dy | (uintptr_t)a->dw) & 15u)
        return fail(MCGMIL_E_ALIGN, "x, dy and dw must be 16-byte aligned");
    if (!a->workspace || a->workspace_bytes < pl.total)
        return fail(MCGMIL_E_WORKSPACE, "workspace missing or smaller than mcgmil_conv_wgrad_workspace_size_f32x3()");
    if (((uintptr_t)a->workspace & 255u) != 0) return fail(MCGMIL_E_ALIGN, "workspace must be 256-byte aligned");

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const float* x = static_cast<const float*>(a->fwd.x);
    float* sum = static_cast<float*>(a->workspace);
    float* part = sum + pl.E;
    const unsigned rblocks = (unsigned)((pl.E + 255) / 256);
    for (long long g0 = 0; g0 < pl.gran_total; g0 += pl.gran_chunk) {
        const long long n = pl.gran_total - g0 < pl.gran_chunk ? pl.gran_total - g0 : pl.gran_chunk;
        const long long pix0 = g0 * kGranule;
        if (int rc = pl.wide ? launch_wgrad<2, 2>(pl, x, a->dy, part, pix0, n, s)
                             : launch_wgrad<1, 4>(pl, x, a->dy, part, pix0, n, s))
            return rc;
        hipLaunchKernelGGL(wgrad_x3_reduce_kernel, dim3(rblocks), dim3(256), 0, s, part, sum, a->dw, pl.E, (int)n,
                           (int)(g0 == 0), (int)(g0 + n == pl.gran_total), pl.g.Cout, pl.g.Cin, pl.g.KH, pl.g.KW);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "wgrad_x3_reduce_kernel launch");
    }
    return MCGMIL_OK;
}

}  // extern "C"
