// fp32 weight gradient of the backbone's convolutions (include/mcgmil_conv_grad.h): the backward
// of mcgmil_conv2d_f32 with respect to its weight, on v_mfma_f32_16x16x4_f32 with fp32 operands
// and fp32 accumulation. Reference: loss.backward() through torch.nn.Conv2d in fp32
// (model.py:166-179, the ResNet feature extractor under net_utils.train_gacc).
//
// GEMM view: rows = output channels o (the A operand, dY), columns = (kh, kw, ci) of the weight
// (the B operand, the tap-shifted x), K = output pixels. In NHWC one pixel of dY is a contiguous
// row of Cout and one (pixel, tap) of x a contiguous row of Cin, so both operands are k-major
// rows in memory already: a stage is [16][BM + 16] and [16][BN + 16] floats, filled with 16-byte
// loads and 16-byte LDS writes (no transposition), and read with the conflict-free ds_read_b32
// fragment scheme of conv32_kernel (mcgmil_conv32.hip: the 16 lanes of one k read 16 consecutive
// words, the 16-word row pad puts the next k on the next 16 banks). Zero padding, stride-2 taps,
// columns past kh*kw*Cin and pixels past the granule are handled when a row is staged (zeros),
// not in the MFMA loop. The next K step is loaded into registers while the current one computes.
//
// A workgroup of 4 waves computes a 128 x 128 tile (64 x 256 when Cout is not a multiple of 128)
// of one granule of MCGMIL_WGRAD_GRANULE_PIXELS output pixels, each wave a 64 x 64 block (64
// accumulator VGPRs); a wave whose 64 columns all lie past kh*kw*Cin skips its MFMAs (its SIMD
// serves the other workgroups of the CU). The grid is (output tiles) x (granules of the launch
// chunk), tiles fastest, so the workgroups that share a granule's dY and x rows run together.
// Every (tile, granule) writes its partial sums to the workspace as [granule][column][o];
// wgrad_reduce_kernel adds them in granule order to a running sum and, after the last chunk,
// writes dW in torch's [o][ci][kh][kw] layout. No atomics: the summation order is a function of
// the geometry alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcgmil.h"
#include "../../include/mcgmil_conv_grad.h"
#include "mcgmil_error.h"

namespace {

using mcgmil_detail::fail;
using mcgmil_detail::hip_fail;

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int kK = 16;     // K step (output pixels)
constexpr int kPad = 16;   // LDS row pad (words)
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
    static constexpr int AS = BM + kPad, BS = BN + kPad;                     // row strides (floats)
    static constexpr int STAGE = kK * (AS + BS);                             // floats per stage
    static constexpr int A4 = kK * BM / 4 / 256, B4 = kK * BN / 4 / 256;     // float4 per thread
    static_assert(A4 >= 1 && B4 >= 1 && 256 % (BN / 4) == 0 && 256 % (BM / 4) == 0, "staging map");
};

// part: [granules of the chunk][Ncols][Cout]. pix0: the chunk's first output pixel (a multiple of
// the granule). tiles = tiles_n * (Cout / BM); blockIdx.x = tile + tiles * (granule in the chunk).
template <int WCO, int WN>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(const WGeom g, const float* __restrict__ x,
                                                       const float* __restrict__ dy, float* __restrict__ part,
                                                       long long pix0, int tiles_n, int tiles) {
    using T = Tile<WCO, WN>;
    __shared__ __attribute__((aligned(16))) float smem[2 * T::STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wco = wave % WCO, wn = wave / WCO;
    const int tile = blockIdx.x % tiles, gl = blockIdx.x / tiles;
    const int tn = tile % tiles_n, tm = tile / tiles_n;
    const int co0 = tm * T::BM, n0 = tn * T::BN;
    const long long pbeg = pix0 + (long long)gl * kGranule;
    const long long pend = pbeg + kGranule < g.P ? pbeg + kGranule : g.P;
    const int steps = (int)((pend - pbeg + kK - 1) / kK);

    // A staging: float4 ac4 of row ak + (256 / (BM / 4)) r of the step's 16 dY rows
    const int ak = tid / (T::BM / 4), ac4 = tid % (T::BM / 4);
    constexpr int AKSTEP = 256 / (T::BM / 4);
    // B staging: float4 bc4 (one tap, 4 input channels: the same for every r) of row bk + BKSTEP r
    const int bk = tid / (T::BN / 4), bc4 = tid % (T::BN / 4);
    constexpr int BKSTEP = 256 / (T::BN / 4);
    const int col = n0 + 4 * bc4;
    const bool cvalid = col < g.Ncols;
    const int tap = cvalid ? col / g.Cin : 0;
    const int ci = cvalid ? col - tap * g.Cin : 0;
    const int kh = tap / g.KW, kw = tap - kh * g.KW;
    const unsigned ohw = (unsigned)(g.OH * g.OW);

    f32x4 ra[T::A4], rb[T::B4];
    auto load = [&](int ks) {
        const long long ps = pbeg + (long long)ks * kK;
#pragma unroll
        for (int r = 0; r < T::A4; ++r) {
            const long long p = ps + ak + AKSTEP * r;
            ra[r] = p < pend ? *reinterpret_cast<const f32x4*>(dy + p * g.Cout + co0 + 4 * ac4)
                             : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int r = 0; r < T::B4; ++r) {
            const long long p = ps + bk + BKSTEP * r;
            bool in = cvalid && p < pend;
            const unsigned pu = in ? (unsigned)p : 0u;      // P < 2^31
            const unsigned n = pu / ohw, rem = pu - n * ohw;
            const unsigned oh = rem / (unsigned)g.OW, ow = rem - oh * (unsigned)g.OW;
            const int ih = (int)oh * g.stride - g.pad + kh, iw = (int)ow * g.stride - g.pad + kw;
            in = in && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
            const long long off = (((long long)n * g.H + (in ? ih : 0)) * g.W + (in ? iw : 0)) * g.Cin + ci;
            rb[r] = in ? *reinterpret_cast<const f32x4*>(x + off) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store = [&](float* st) {
        float* As = st;
        float* Bs = st + kK * T::AS;
#pragma unroll
        for (int r = 0; r < T::A4; ++r)
            *reinterpret_cast<f32x4*>(As + (ak + AKSTEP * r) * T::AS + 4 * ac4) = ra[r];
#pragma unroll
        for (int r = 0; r < T::B4; ++r)
            *reinterpret_cast<f32x4*>(Bs + (bk + BKSTEP * r) * T::BS + 4 * bc4) = rb[r];
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int kl = lane >> 4, cl = lane & 15;
    const bool active = n0 + wn * 64 < g.Ncols;    // wave-uniform
    load(0);
    store(smem);
    __syncthreads();
    for (int ks = 0; ks < steps; ++ks) {
        const float* st = smem + (ks & 1) * T::STAGE;
        const float* As = st + wco * 64 + cl;
        const float* Bs = st + kK * T::AS + wn * 64 + cl;
        if (ks + 1 < steps) load(ks + 1);
        if (active) {
#pragma unroll
            for (int s = 0; s < kK / 4; ++s) {
                const int k = 4 * s + kl;
                float a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = As[k * T::AS + 16 * i];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = Bs[k * T::BS + 16 * j];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
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
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ sum,
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
    if (f.in_ab) return fail(MCGMIL_E_UNSUPPORTED, "weight gradient: in_ab must be NULL (no input BatchNorm)");
    if (f.batch < 1 || f.height < 1 || f.width < 1)
        return fail(MCGMIL_E_INVALID, "batch, height and width must be >= 1");
    if (f.in_channels < 16 || f.in_channels % 16 != 0)
        return fail(MCGMIL_E_UNSUPPORTED, "weight gradient: in_channels a multiple of 16");
    if (f.out_channels < 64 || f.out_channels % 64 != 0)
        return fail(MCGMIL_E_UNSUPPORTED, "weight gradient: out_channels a multiple of 64");
    if (f.kernel_h < 1 || f.kernel_w < 1 || f.kernel_h > 7 || f.kernel_w > 7)
        return fail(MCGMIL_E_UNSUPPORTED, "kernel size must be in 1..7");
    if (f.stride != 1 && f.stride != 2) return fail(MCGMIL_E_UNSUPPORTED, "weight gradient: stride 1 or 2");
    if (f.pad < 0) return fail(MCGMIL_E_INVALID, "pad must be >= 0");
    if (f.pad >= f.kernel_h || f.pad >= f.kernel_w)
        return fail(MCGMIL_E_UNSUPPORTED, "weight gradient: pad must be smaller than the kernel");
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
int launch_wgrad(const Plan& pl, const float* x, const float* dy, float* part, long long pix0, long long granules,
                 hipStream_t s) {
    hipLaunchKernelGGL((wgrad_kernel<WCO, WN>), dim3((unsigned)(granules * pl.tiles)), dim3(256), 0, s, pl.g, x, dy,
                       part, pix0, pl.tiles_n, pl.tiles);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCGMIL_OK : hip_fail(e, "wgrad_kernel launch");
}

}  // namespace

extern "C" {

size_t mcgmil_conv_grad_args_size(void) { return sizeof(mcgmil_conv_grad_args); }

int mcgmil_conv_wgrad_workspace_size_f32(const mcgmil_conv_grad_args* a, size_t* bytes) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!bytes) return fail(MCGMIL_E_INVALID, "bytes is NULL");
    *bytes = pl.total;
    return MCGMIL_OK;
}

int mcgmil_conv2d_wgrad_f32(const mcgmil_conv_grad_args* a, void* stream) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!a->fwd.x || !a->dy || !a->dw) return fail(MCGMIL_E_INVALID, "NULL x, dy or dw");
    if (((uintptr_t)a->fwd.x | (uintptr_t)a->dy | (uintptr_t)a->dw) & 15u)
        return fail(MCGMIL_E_ALIGN, "x, dy and dw must be 16-byte aligned");
    if (!a->workspace || a->workspace_bytes < pl.total)
        return fail(MCGMIL_E_WORKSPACE, "workspace missing or smaller than mcgmil_conv_wgrad_workspace_size_f32()");
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
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(rblocks), dim3(256), 0, s, part, sum, a->dw, pl.E, (int)n,
                           (int)(g0 == 0), (int)(g0 + n == pl.gran_total), pl.g.Cout, pl.g.Cin, pl.g.KH, pl.g.KW);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "wgrad_reduce_kernel launch");
    }
    return MCGMIL_OK;
}

}  // extern "C"
