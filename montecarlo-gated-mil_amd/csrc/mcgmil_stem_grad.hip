// fp32 weight gradient of a convolution with 1..4 input channels (include/mcgmil_stem_grad.h): the
// backward of mcgmil_conv2d_f32's gather mode with respect to its weight, on
// v_mfma_f32_16x16x4_f32 with fp32 operands and fp32 accumulation. Reference: loss.backward()
// through conv1 = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False) in fp32
// (model.py:166-179, the ResNet feature extractor under net_utils.train_gacc).
//
// GEMM view, as in mcgmil_conv_grad.hip: rows = output channels o (the A operand, dY), columns =
// (kh, kw, ci) of the weight (the B operand, the tap-shifted x), K = output pixels. With so few
// input channels the whole column range (at most 196) is one tile: a workgroup of 4 waves computes
// 64 output channels x all columns of one granule of MCGMIL_WGRAD_GRANULE_PIXELS output pixels,
// each wave 16 output channels x NB blocks of 16 columns (4 NB accumulator VGPRs; NB = 4, 10 or
// 13, the stem's 147 columns take 10). The waves split the output channels, not the pixels, so no
// cross-wave sum exists and the order of every addition is a function of the geometry alone.
//
// A K step is 16 output pixels. dY is staged as in mcgmil_conv_grad.hip (one 16-byte load per
// thread). The B stage [16][16 NB + pad] is gathered: thread t owns pixel t / 16 of the step and
// the columns t % 16 + 16 j, whose (kh, kw) and offset (kh W + kw) Cin + ci inside the window are
// computed once per workgroup, so a step costs one pixel decomposition and NB bounds-checked
// 4-byte loads per thread; the 16 lanes of one pixel read consecutive (kw, ci), which are
// contiguous in NHWC. Zero padding, columns past kh*kw*Cin and pixels past the granule become
// zeros when the stage is filled, not in the MFMA loop. The LDS row strides are an odd number of
// 16-word blocks, so the four k rows of a fragment read (and the four pixel rows of a stage
// write) fall on four different groups of 16 banks. The next K step is loaded into registers
// while the current one computes.
//
// Every (tile, granule) writes its partial sums to the workspace as [granule][column][o];
// stem_wgrad_reduce_kernel adds them in granule order to a running sum and, after the last chunk,
// writes dW in torch's [o][ci][kh][kw] layout. No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcgmil.h"
#include "../../include/mcgmil_stem_grad.h"
#include "mcgmil_error.h"

namespace {

using mcgmil_detail::fail;
using mcgmil_detail::hip_fail;

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int kK = 16;     // K step (output pixels)
constexpr int kBM = 64;    // output channels per workgroup (16 per wave)
constexpr int kGranule = MCGMIL_WGRAD_GRANULE_PIXELS;
static_assert(kGranule % kK == 0, "a granule is a whole number of K steps");

struct SGeom {
    int N, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW;
    int Ncols;            // KH * KW * Cin
    long long P;          // N * OH * OW output pixels
};

template <int NB>
struct STile {
    static constexpr int AS = kBM + 16;                            // 5 blocks of 16 words
    static constexpr int BS = 16 * (NB + (NB % 2 == 0 ? 1 : 2));   // an odd number of blocks
    static constexpr int STAGE = kK * (AS + BS);                   // floats per stage
    static_assert((AS / 16) % 2 == 1 && (BS / 16) % 2 == 1, "row strides: odd multiples of 16 words");
};

// part: [granules of the chunk][Ncols][Cout]. pix0: the chunk's first output pixel (a multiple of
// the granule). tiles = Cout / 64; blockIdx.x = tile + tiles * (granule in the chunk).
template <int NB>
__global__ __launch_bounds__(256, 2) void stem_wgrad_kernel(const SGeom g, const float* __restrict__ x,
                                                            const float* __restrict__ dy, float* __restrict__ part,
                                                            long long pix0, int tiles) {
    using T = STile<NB>;
    __shared__ __attribute__((aligned(16))) float smem[2 * T::STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x % tiles, gl = blockIdx.x / tiles;
    const int co0 = tile * kBM;
    const long long pbeg = pix0 + (long long)gl * kGranule;
    const long long pend = pbeg + kGranule < g.P ? pbeg + kGranule : g.P;
    const int steps = (int)((pend - pbeg + kK - 1) / kK);

    // staging: row sk of the step's 16 pixels; float4 sc of its 64 dY values, columns sc + 16 j of B
    const int sk = tid >> 4, sc = tid & 15;
    // per column: kh | kw << 4 (256: past Ncols) and the offset of (kh, kw, ci) from the window's origin
    int ctap[NB], coff[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int col = sc + 16 * j;
        const bool cvalid = col < g.Ncols;
        const int tap = cvalid ? col / g.Cin : 0;
        const int ci = cvalid ? col - tap * g.Cin : 0;
        const int kh = tap / g.KW, kw = tap - kh * g.KW;
        ctap[j] = cvalid ? (kh | (kw << 4)) : 256;
        coff[j] = (kh * g.W + kw) * g.Cin + ci;
    }
    const unsigned ohw = (unsigned)(g.OH * g.OW);

    f32x4 ra;
    float rb[NB];
    auto load = [&](int ks) {
        const long long p = pbeg + (long long)ks * kK + sk;
        const bool in = p < pend;
        ra = in ? *reinterpret_cast<const f32x4*>(dy + p * g.Cout + co0 + 4 * sc) : f32x4{0.f, 0.f, 0.f, 0.f};
        const unsigned pu = in ? (unsigned)p : 0u;      // P < 2^31
        const unsigned n = pu / ohw, rem = pu - n * ohw;
        const unsigned oh = rem / (unsigned)g.OW, ow = rem - oh * (unsigned)g.OW;
        const int ih0 = (int)oh * g.stride - g.pad, iw0 = (int)ow * g.stride - g.pad;
        // the window's origin; it may lie before x, and is only dereferenced at taps inside the image
        const long long base = (((long long)n * g.H + ih0) * g.W + iw0) * g.Cin;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int kh = ctap[j] & 15, kw = (ctap[j] >> 4) & 15;
            const bool ok = in && ctap[j] < 256 && (unsigned)(ih0 + kh) < (unsigned)g.H &&
                            (unsigned)(iw0 + kw) < (unsigned)g.W;
            rb[j] = ok ? x[base + coff[j]] : 0.f;
        }
    };
    auto store = [&](float* st) {
        *reinterpret_cast<f32x4*>(st + sk * T::AS + 4 * sc) = ra;
        float* Bs = st + kK * T::AS + sk * T::BS + sc;
#pragma unroll
        for (int j = 0; j < NB; ++j) Bs[16 * j] = rb[j];
    };

    f32x4 acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int kl = lane >> 4, cl = lane & 15;
    load(0);
    store(smem);
    __syncthreads();
    for (int ks = 0; ks < steps; ++ks) {
        const float* st = smem + (ks & 1) * T::STAGE;
        const float* As = st + wave * 16 + cl;
        const float* Bs = st + kK * T::AS + cl;
        if (ks + 1 < steps) load(ks + 1);
#pragma unroll
        for (int s = 0; s < kK / 4; ++s) {
            const int k = 4 * s + kl;
            const float a = As[k * T::AS];
            float b[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) b[j] = Bs[k * T::BS + 16 * j];
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[j], acc[j], 0, 0, 0);
        }
        if (ks + 1 < steps) store(smem + ((ks + 1) & 1) * T::STAGE);
        __syncthreads();
    }

    // D block j: lane holds o = co0 + 16 wave + 4 (lane >> 4) + v of column 16 j + (lane & 15)
    float* pg = part + (long long)gl * g.Ncols * g.Cout;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int nn = 16 * j + cl;
        if (nn >= g.Ncols) continue;
        *reinterpret_cast<f32x4*>(pg + (long long)nn * g.Cout + co0 + wave * 16 + 4 * kl) = acc[j];
    }
}

// sum[e] (+)= part[0][e] + part[1][e] + ... in granule order, one element per thread; the last
// chunk writes dW[o][ci][kh][kw] instead of the running sum. e = column * Cout + o.
__global__ __launch_bounds__(256) void stem_wgrad_reduce_kernel(const float* __restrict__ part,
                                                                float* __restrict__ sum, float* __restrict__ dw,
                                                                long long E, int granules, int first, int last,
                                                                int Cout, int Cin, int KH, int KW) {
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
    SGeom g;
    long long E;                       // Cout * Ncols
    long long gran_total, gran_chunk;
    int tiles;                         // Cout / 64
    int nb;                            // column blocks of the kernel variant: 4, 10 or 13
    size_t total;                      // workspace bytes
};

int plan_for(const mcgmil_conv_grad_args* a, Plan& pl) {
    if (!a) return fail(MCGMIL_E_INVALID, "args is NULL");
    const mcgmil_conv_args& f = a->fwd;
    if (a->reserved != 0) return fail(MCGMIL_E_INVALID, "reserved must be 0");
    if (a->chunk_pixels < 0) return fail(MCGMIL_E_INVALID, "chunk_pixels must be >= 0");
    if (f.in_ab) return fail(MCGMIL_E_UNSUPPORTED, "stem weight gradient: in_ab must be NULL (no input BatchNorm)");
    if (f.batch < 1 || f.height < 1 || f.width < 1)
        return fail(MCGMIL_E_INVALID, "batch, height and width must be >= 1");
    if (f.in_channels < 1 || f.in_channels > 4)
        return fail(MCGMIL_E_UNSUPPORTED, "stem weight gradient: in_channels must be in 1..4");
    if (f.out_channels < 64 || f.out_channels % 64 != 0 || f.out_channels > 4096)
        return fail(MCGMIL_E_UNSUPPORTED, "stem weight gradient: out_channels a multiple of 64, at most 4096");
    if (f.kernel_h < 1 || f.kernel_w < 1 || f.kernel_h > 7 || f.kernel_w > 7)
        return fail(MCGMIL_E_UNSUPPORTED, "kernel size must be in 1..7");
    if (f.stride != 1 && f.stride != 2) return fail(MCGMIL_E_UNSUPPORTED, "stem weight gradient: stride 1 or 2");
    if (f.pad < 0) return fail(MCGMIL_E_INVALID, "pad must be >= 0");
    if (f.pad >= f.kernel_h || f.pad >= f.kernel_w)
        return fail(MCGMIL_E_UNSUPPORTED, "stem weight gradient: pad must be smaller than the kernel");
    if (f.height >= (1 << 24) || f.width >= (1 << 24))
        return fail(MCGMIL_E_UNSUPPORTED, "stem weight gradient: height and width must be < 2^24");
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
    SGeom& g = pl.g;
    g.N = f.batch; g.H = f.height; g.W = f.width; g.Cin = f.in_channels; g.Cout = f.out_channels;
    g.KH = f.kernel_h; g.KW = f.kernel_w; g.stride = f.stride; g.pad = f.pad;
    g.OH = (int)oh; g.OW = (int)ow; g.P = P;
    g.Ncols = f.kernel_h * f.kernel_w * f.in_channels;      // <= 196
    pl.E = (long long)g.Ncols * f.out_channels;
    const int nbn = (g.Ncols + 15) / 16;
    pl.nb = nbn <= 4 ? 4 : nbn <= 10 ? 10 : 13;
    pl.tiles = f.out_channels / kBM;                        // <= 64
    pl.gran_total = (P + kGranule - 1) / kGranule;          // < 2^20: the grid stays below 2^26
    const long long ebytes = pl.E * 4;                      // a multiple of 256
    long long gc = a->chunk_pixels ? a->chunk_pixels / kGranule : MCGMIL_WGRAD_DEFAULT_PARTIAL_BYTES / ebytes;
    if (gc < 1) gc = 1;
    if (gc > pl.gran_total) gc = pl.gran_total;
    pl.gran_chunk = gc;
    pl.total = (size_t)((gc + 1) * ebytes);                 // < 2^20 * 2^22
    return MCGMIL_OK;
}

template <int NB>
int launch_wgrad(const Plan& pl, const float* x, const float* dy, float* part, long long pix0, long long granules,
                 hipStream_t s) {
    hipLaunchKernelGGL((stem_wgrad_kernel<NB>), dim3((unsigned)(granules * pl.tiles)), dim3(256), 0, s, pl.g, x, dy,
                       part, pix0, pl.tiles);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCGMIL_OK : hip_fail(e, "stem_wgrad_kernel launch");
}

}  // namespace

extern "C" {

int mcgmil_stem_wgrad_workspace_size_f32(const mcgmil_conv_grad_args* a, size_t* bytes) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!bytes) return fail(MCGMIL_E_INVALID, "bytes is NULL");
    *bytes = pl.total;
    return MCGMIL_OK;
}

int mcgmil_stem_wgrad_f32(const mcgmil_conv_grad_args* a, void* stream) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!a->fwd.x || !a->dy || !a->dw) return fail(MCGMIL_E_INVALID, "NULL x, dy or dw");
    if ((((uintptr_t)a->dy | (uintptr_t)a->dw) & 15u) || ((uintptr_t)a->fwd.x & 3u))
        return fail(MCGMIL_E_ALIGN, "dy and dw must be 16-byte aligned, x 4-byte aligned");
    if (!a->workspace || a->workspace_bytes < pl.total)
        return fail(MCGMIL_E_WORKSPACE, "workspace missing or smaller than mcgmil_stem_wgrad_workspace_size_f32()");
    if (((uintptr_t)a->workspace & 255u) != 0) return fail(MCGMIL_E_ALIGN, "workspace must be 256-byte aligned");

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const float* x = static_cast<const float*>(a->fwd.x);
    float* sum = static_cast<float*>(a->workspace);
    float* part = sum + pl.E;
    const unsigned rblocks = (unsigned)((pl.E + 255) / 256);
    for (long long g0 = 0; g0 < pl.gran_total; g0 += pl.gran_chunk) {
        const long long n = pl.gran_total - g0 < pl.gran_chunk ? pl.gran_total - g0 : pl.gran_chunk;
        const long long pix0 = g0 * kGranule;
        if (int rc = pl.nb == 4    ? launch_wgrad<4>(pl, x, a->dy, part, pix0, n, s)
                     : pl.nb == 10 ? launch_wgrad<10>(pl, x, a->dy, part, pix0, n, s)
                                   : launch_wgrad<13>(pl, x, a->dy, part, pix0, n, s))
            return rc;
        hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3(rblocks), dim3(256), 0, s, part, sum, a->dw, pl.E, (int)n,
                           (int)(g0 == 0), (int)(g0 + n == pl.gran_total), pl.g.Cout, pl.g.Cin, pl.g.KH, pl.g.KW);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "stem_wgrad_reduce_kernel launch");
    }
    return MCGMIL_OK;
}

}  // extern "C"
