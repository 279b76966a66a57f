// bf16 weight gradient of the backbone's block convolutions (include/mcgmil_conv_grad_bf16.h):
// the backward of mcgmil_conv2d with respect to its weight, on v_mfma_f32_16x16x32_bf16 with bf16
// operands and fp32 accumulation, dW in fp32. Reference: loss.backward() through torch.nn.Conv2d
// under torch.autocast("cuda", torch.bfloat16) (model.py:166-179, the ResNet feature extractor
// under net_utils.train_gacc).
//
// The GEMM view, the tiles, the granules and the reduce are those of mcgmil_conv_grad.hip: rows =
// output channels o (the A operand, dY), columns = (kh, kw, ci) of the weight (the B operand, the
// tap-shifted x), K = output pixels; a workgroup of 4 waves computes a 128 x 128 tile (64 x 256
// when Cout is not a multiple of 128) of one granule of MCGMIL_WGRAD_GRANULE_PIXELS output pixels,
// each wave a 64 x 64 block; every (tile, granule) writes its partial sums to the workspace as
// [granule][column][o] and wgrad_bf16_reduce_kernel adds them in granule order. No atomics.
//
// What differs is the operand path. A K step is 32 output pixels (one MFMA deep). In NHWC a pixel
// of dY is a contiguous row of Cout and one (pixel, tap) of x a contiguous row of Cin, so both
// operands are k-major rows in memory, while the MFMA wants 8 consecutive k per lane: a stage is
// [32][BM + 16] and [32][BN + 16] bf16, filled with 16-byte global loads and 16-byte LDS writes
// (no transposition), and the fragments are read with the gfx950 transposed LDS read
// ds_read_b64_tr_b16: per 16-lane group a block of 4 k rows x 16 columns comes back column-major,
// lane i holding column i of the 4 rows. Two reads make one 8-k operand. Which k rows a lane group
// takes is free as long as A and B agree; group g takes rows 4g + q and 16 + 4g + q (q = 0..3), so
// the two groups of a 32-lane half read 8 rows that are consecutive mod 8, and with a row stride of
// 32 bytes mod 256 (the 16-element pad) those land on 8 different 32-byte bank slots: no conflict.
// Every address is 8-byte aligned and every lane of a reading wave supplies one (the `active` skip
// is wave-uniform; there is no lane-dependent guard around the reads). Zero padding, stride-2 taps,
// columns past kh*kw*Cin and pixels past the granule are zeros written when a row is staged. The
// next K step is loaded into registers while the current one computes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcgmil.h"
#include "../../include/mcgmil_conv_grad_bf16.h"
#include "mcgmil_error.h"

namespace {

using mcgmil_detail::fail;
using mcgmil_detail::hip_fail;

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) short i16x4;
typedef __attribute__((ext_vector_type(8))) short i16x8;
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
    static constexpr int STAGE = kK * (AS + BS);                             // bf16 per stage
    static constexpr int A8 = kK * BM / 8 / 256, B8 = kK * BN / 8 / 256;     // 16-byte chunks per thread
    static_assert(A8 >= 1 && B8 >= 1 && 256 % (BN / 8) == 0 && 256 % (BM / 8) == 0, "staging map");
    // an odd number of 32-byte slots per row: 8 consecutive rows hit 8 different slots of the 256
    static_assert((AS * 2) % 64 == 32 && (BS * 2) % 64 == 32, "LDS row stride and the banks");
};

// The 4 x 16 block at p (this lane's row and 4 columns of it), column-major: ds_read_b64_tr_b16.
__device__ __forceinline__ i16x4 read_tr(const __bf16* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)p);
}

// part: [granules of the chunk][Ncols][Cout]. pix0: the chunk's first output pixel (a multiple of
// the granule). tiles = tiles_n * (Cout / BM); blockIdx.x = tile + tiles * (granule in the chunk).
template <int WCO, int WN>
__global__ __launch_bounds__(256, 2) void wgrad_bf16_kernel(const WGeom g, const __bf16* __restrict__ x,
                                                            const __bf16* __restrict__ dy, float* __restrict__ part,
                                                            long long pix0, int tiles_n, int tiles) {
    using T = Tile<WCO, WN>;
    __shared__ __attribute__((aligned(16))) __bf16 smem[2 * T::STAGE];
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

    u32x4 ra[T::A8], rb[T::B8];
    auto load = [&](int ks) {
        const long long ps = pbeg + (long long)ks * kK;
#pragma unroll
        for (int r = 0; r < T::A8; ++r) {
            const long long p = ps + ak + AKSTEP * r;
            ra[r] = p < pend ? *reinterpret_cast<const u32x4*>(dy + p * g.Cout + co0 + 8 * ac8) : u32x4{0u, 0u, 0u, 0u};
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
            const long long off = (((long long)n * g.H + (in ? ih : 0)) * g.W + (in ? iw : 0)) * g.Cin + ci;
            rb[r] = in ? *reinterpret_cast<const u32x4*>(x + off) : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto store = [&](__bf16* st) {
        __bf16* As = st;
        __bf16* Bs = st + kK * T::AS;
#pragma unroll
        for (int r = 0; r < T::A8; ++r)
            *reinterpret_cast<u32x4*>(As + (ak + AKSTEP * r) * T::AS + 8 * ac8) = ra[r];
#pragma unroll
        for (int r = 0; r < T::B8; ++r)
            *reinterpret_cast<u32x4*>(Bs + (bk + BKSTEP * r) * T::BS + 8 * bc8) = rb[r];
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
    store(smem);
    __syncthreads();
    for (int ks = 0; ks < steps; ++ks) {
        const __bf16* st = smem + (ks & 1) * T::STAGE;
        const __bf16* As = st + trow * T::AS + wco * 64 + tcol;
        const __bf16* Bs = st + kK * T::AS + trow * T::BS + wn * 64 + tcol;
        if (ks + 1 < steps) load(ks + 1);
        if (active) {
            bf16x8 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const i16x4 lo = read_tr(As + 16 * i), hi = read_tr(As + 16 * T::AS + 16 * i);
                a[i] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const i16x4 lo = read_tr(Bs + 16 * j), hi = read_tr(Bs + 16 * T::BS + 16 * j);
                b[j] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (ks + 1 < steps) store(smem + ((ks + 1) & 1) * T::STAGE);
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
// chunk writes dW[o][ci][kh][kw] instead of the running sum. e = column * Cout + o.
__global__ __launch_bounds__(256) void wgrad_bf16_reduce_kernel(const float* __restrict__ part, float* __restrict__ sum,
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

int plan_for(const mcgmil_conv_grad_bf16_args* a, Plan& pl) {
    if (!a) return fail(MCGMIL_E_INVALID, "args is NULL");
    const mcgmil_conv_args& f = a->fwd;
    if (a->reserved != 0) return fail(MCGMIL_E_INVALID, "reserved must be 0");
    if (a->chunk_pixels < 0) return fail(MCGMIL_E_INVALID, "chunk_pixels must be >= 0");
    if (f.in_ab) return fail(MCGMIL_E_UNSUPPORTED, "bf16 weight gradient: in_ab must be NULL (no input BatchNorm)");
    if (f.batch < 1 || f.height < 1 || f.width < 1)
        return fail(MCGMIL_E_INVALID, "batch, height and width must be >= 1");
    if (f.in_channels < 64 || f.in_channels % 64 != 0)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16 weight gradient: in_channels a multiple of 64");
    if (f.out_channels < 64 || f.out_channels % 64 != 0)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16 weight gradient: out_channels a multiple of 64");
    if (f.kernel_h < 1 || f.kernel_w < 1 || f.kernel_h > 7 || f.kernel_w > 7)
        return fail(MCGMIL_E_UNSUPPORTED, "kernel size must be in 1..7");
    if (f.stride != 1 && f.stride != 2) return fail(MCGMIL_E_UNSUPPORTED, "bf16 weight gradient: stride 1 or 2");
    if (f.pad < 0) return fail(MCGMIL_E_INVALID, "pad must be >= 0");
    if (f.pad >= f.kernel_h || f.pad >= f.kernel_w)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16 weight gradient: pad must be smaller than the kernel");
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
    pl.tiles = pl.tiles_n * (f.out_channels / BM);       // <= E / 4096 < 2^22
    pl.gran_total = (P + kGranule - 1) / kGranule;       // < 2^20
    const long long ebytes = pl.E * 4;                   // a multiple of 4096
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
int launch_wgrad(const Plan& pl, const __bf16* x, const __bf16* dy, float* part, long long pix0, long long granules,
                 hipStream_t s) {
    hipLaunchKernelGGL((wgrad_bf16_kernel<WCO, WN>), dim3((unsigned)(granules * pl.tiles)), dim3(256), 0, s, pl.g, x,
                       dy, part, pix0, pl.tiles_n, pl.tiles);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCGMIL_OK : hip_fail(e, "wgrad_bf16_kernel launch");
}

}  // namespace

extern "C" {

size_t mcgmil_conv_grad_bf16_args_size(void) { return sizeof(mcgmil_conv_grad_bf16_args); }

int mcgmil_conv_wgrad_workspace_size_bf16(const mcgmil_conv_grad_bf16_args* a, size_t* bytes) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!bytes) return fail(MCGMIL_E_INVALID, "bytes is NULL");
    *bytes = pl.total;
    return MCGMIL_OK;
}

int mcgmil_conv2d_wgrad_bf16(const mcgmil_conv_grad_bf16_args* a, void* stream) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!a->fwd.x || !a->dy || !a->dw) return fail(MCGMIL_E_INVALID, "NULL x, dy or dw");
    if (((uintptr_t)a->fwd.x | (uintptr_t)a->dy | (uintptr_t)a->dw) & 15u)
        return fail(MCGMIL_E_ALIGN, "x, dy and dw must be 16-byte aligned");
    if (!a->workspace || a->workspace_bytes < pl.total)
        return fail(MCGMIL_E_WORKSPACE, "workspace missing or smaller than mcgmil_conv_wgrad_workspace_size_bf16()");
    if (((uintptr_t)a->workspace & 255u) != 0) return fail(MCGMIL_E_ALIGN, "workspace must be 256-byte aligned");

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const __bf16* x = static_cast<const __bf16*>(a->fwd.x);
    const __bf16* dy = static_cast<const __bf16*>(a->dy);
    float* sum = static_cast<float*>(a->workspace);
    float* part = sum + pl.E;
    const unsigned rblocks = (unsigned)((pl.E + 255) / 256);
    for (long long g0 = 0; g0 < pl.gran_total; g0 += pl.gran_chunk) {
        const long long n = pl.gran_total - g0 < pl.gran_chunk ? pl.gran_total - g0 : pl.gran_chunk;
        const long long pix0 = g0 * kGranule;
        if (int rc = pl.wide ? launch_wgrad<2, 2>(pl, x, dy, part, pix0, n, s)
                             : launch_wgrad<1, 4>(pl, x, dy, part, pix0, n, s))
            return rc;
        hipLaunchKernelGGL(wgrad_bf16_reduce_kernel, dim3(rblocks), dim3(256), 0, s, part, sum, a->dw, pl.E, (int)n,
                           (int)(g0 == 0), (int)(g0 + n == pl.gran_total), pl.g.Cout, pl.g.Cin, pl.g.KH, pl.g.KW);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "wgrad_bf16_reduce_kernel launch");
    }
    return MCGMIL_OK;
}

}  // extern "C"
