// fp32 data gradient of the backbone's convolutions (include/mcgmil_conv_dgrad.h): the backward of
// mcgmil_conv2d_f32 with respect to its input, stride 1 and 2, on v_mfma_f32_16x16x4_f32 with fp32
// operands and fp32 accumulation. Reference: loss.backward() through torch.nn.Conv2d in fp32
// (model.py:166-179, the ResNet feature extractor under net_utils.train_gacc).
//
// Residue classes: input pixel (ih, iw) belongs to class (r_h, r_w) = ((ih + p) mod s, (iw + p) mod s).
// Its rows are ih = a_h + s j_h with a_h = (r_h - p) mod s, j_h = 0 .. Hc - 1 (columns likewise), and
// only the taps kh = r_h + s m_h < KH, kw = r_w + s m_w < KW reach it, from the output pixel
// oh = j_h + c_h - m_h with c_h = (a_h + p - r_h) / s (exact), ow likewise. Inside a class the data
// gradient is therefore a stride-1 implicit GEMM without zero insertion.
//
// GEMM view: rows = input channels (the A operand: the weight image [kh][kw][out][in], so the 16
// out rows of a K step are k-major rows of Cin already), columns = the class's input pixels (the B
// operand: 16 consecutive out channels of dY at (n, oh, ow), one 64-byte row piece, zero when the
// tap's output pixel lies outside dY), K = (tap, out) in steps of 16 out channels of one tap, taps
// in (kh, kw) order. The fragment and LDS scheme is conv32_kernel's (mcgmil_conv32.hip): 4 waves,
// each a 64 x 64 block of 4 x 4 MFMA tiles; tiles of 128 channels x 128 pixels, or 64 x 256 when
// Cin <= 64; two LDS stages of k-major rows with the 16-word pad (every ds_read_b32 conflict-free);
// the next step in registers while the current one computes; one 16-byte store of 4 consecutive
// input channels per lane and tile. Channel rows past Cin (Cin = 16, 32, 48, or the second half of
// a 128-row tile) are staged as zeros and not stored; a wave whose 64 rows all lie past Cin skips
// its MFMAs.
//
// Grid: x = the classes' pixel tiles one class after another, heaviest (most taps) first so the
// short ones fill the tail; y = the channel tile. A workgroup owns pixels of ONE class, so its tap
// list is uniform. A tile of a class without taps stages nothing and stores zeros. Every dx element
// is written exactly once by one lane: no split-K, no atomics, no workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcgmil.h"
#include "../../include/mcgmil_conv_dgrad.h"
#include "mcgmil_error.h"

namespace {

using mcgmil_detail::fail;
using mcgmil_detail::hip_fail;

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int kK = 16;     // K step (output channels of one tap)
constexpr int kPad = 16;   // LDS row pad (words)

struct DGeom {
    int N, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW;
    int ncls;              // stride^2 classes, in grid order
    int res[4];            // r_h | r_w << 4 of the class
    int tile0[5];          // the class's first pixel tile on the grid's x axis; tile0[ncls] = gridDim.x
};

template <int WCI, int WPX>
struct Tile {
    static constexpr int BN_CI = 64 * WCI, BM_PX = 64 * WPX;
    static constexpr int AS = BN_CI + kPad, BS = BM_PX + kPad;              // row strides (floats)
    static constexpr int STAGE = kK * (AS + BS);                             // floats per stage
    static constexpr int A4 = kK * BN_CI / 4 / 256, B4 = kK * BM_PX / 4 / 256;   // float4 per thread
    static_assert(A4 >= 1 && B4 >= 1 && 256 % BM_PX == 0 && 256 % (BN_CI / 4) == 0, "staging map");
};

// One axis of a class: a = first coordinate, cnt = coordinates, c = offset of the output index,
// taps = taps of the axis.
struct Axis {
    int a, cnt, c, taps;
};

__host__ __device__ inline Axis axis_of(int r, int size, int k, int s, int p) {
    Axis x;
    x.a = (r - p) & (s - 1);                       // s is 1 or 2: (r - p) mod s, non-negative
    x.cnt = x.a < size ? (size - x.a + s - 1) / s : 0;
    x.c = (x.a + p - r) / s;                        // exact and >= 0
    x.taps = r < k ? (k - r + s - 1) / s : 0;
    return x;
}

template <int WCI, int WPX>
__global__ __launch_bounds__(256, 2) void dgrad_kernel(const DGeom g, const float* __restrict__ dy,
                                                       const float* __restrict__ wt, float* __restrict__ dx) {
    using T = Tile<WCI, WPX>;
    __shared__ __attribute__((aligned(16))) float smem[2 * T::STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wci = wave % WCI, wpx = wave / WCI;
    const int bx = (int)blockIdx.x;
    const int ci0 = (int)blockIdx.y * T::BN_CI;

    // the workgroup's class (uniform)
    int res = g.res[0], t0 = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
        if (q < g.ncls && bx >= g.tile0[q]) {
            res = g.res[q];
            t0 = g.tile0[q];
        }
    const int s = g.stride, rh = res & 15, rw = res >> 4;
    const Axis ah = axis_of(rh, g.H, g.KH, s, g.pad), aw = axis_of(rw, g.W, g.KW, s, g.pad);
    const int hw = ah.cnt * aw.cnt;                 // > 0: the class has a tile
    const int Pc = g.N * hw;                        // < 2^31 - 256
    const int cch = g.Cout / kK;
    const int KS = ah.taps * aw.taps * cch;
    const int px0 = (bx - t0) * T::BM_PX;

    // B staging: every thread owns pixel tid % BM_PX of the tile and some of its 4 out quads
    const int bpx = tid % T::BM_PX;
    const int bq0 = tid / T::BM_PX;
    constexpr int QSTEP = 256 / T::BM_PX;
    const bool pvalid = px0 + bpx < Pc;
    int n = 0, qh = 0, qw = 0;
    if (pvalid) {
        const int pc = px0 + bpx;
        n = pc / hw;
        const int r = pc - n * hw;
        const int jh = r / aw.cnt;
        qh = jh + ah.c;
        qw = r - jh * aw.cnt + aw.c;
    }
    const float* dyn = dy + (long long)n * g.OH * g.OW * g.Cout;

    f32x4 ra[T::A4], rb[T::B4];
    auto load = [&](int ks) {
        const int tap = ks / cch, co0 = (ks - tap * cch) * kK;
        const int mh = tap / aw.taps, mw = tap - mh * aw.taps;
        const int kh = rh + s * mh, kw = rw + s * mw;
        // A: wt[kh][kw][co0 + k][ci0 ..]: 16 rows of Cin; channels past Cin are zero rows
        const float* wk = wt + ((long long)(kh * g.KW + kw) * g.Cout + co0) * g.Cin + ci0;
#pragma unroll
        for (int r = 0; r < T::A4; ++r) {
            const int f = tid + 256 * r;
            const int k = f / (T::BN_CI / 4), c4 = f % (T::BN_CI / 4);
            ra[r] = ci0 + 4 * c4 < g.Cin ? *reinterpret_cast<const f32x4*>(wk + (long long)k * g.Cin + 4 * c4)
                                         : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // B: dy[n, oh, ow, co0 + 4q .. +3] of this thread's pixel (zero outside dY)
        const int oh = qh - mh, ow = qw - mw;
        const bool in = pvalid && oh >= 0 && oh < g.OH && ow >= 0 && ow < g.OW;
        const float* src = dyn + ((long long)(in ? oh : 0) * g.OW + (in ? ow : 0)) * g.Cout + co0;
#pragma unroll
        for (int r = 0; r < T::B4; ++r) {
            const int q = bq0 + QSTEP * r;
            rb[r] = in ? *reinterpret_cast<const f32x4*>(src + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store = [&](float* st) {
        float* As = st;
        float* Bs = st + kK * T::AS;
#pragma unroll
        for (int r = 0; r < T::A4; ++r) {
            const int f = tid + 256 * r;
            const int k = f / (T::BN_CI / 4), c4 = f % (T::BN_CI / 4);
            *reinterpret_cast<f32x4*>(As + k * T::AS + 4 * c4) = ra[r];
        }
#pragma unroll
        for (int r = 0; r < T::B4; ++r) {
            const int q = bq0 + QSTEP * r;
            Bs[(4 * q + 0) * T::BS + bpx] = rb[r].x;
            Bs[(4 * q + 1) * T::BS + bpx] = rb[r].y;
            Bs[(4 * q + 2) * T::BS + bpx] = rb[r].z;
            Bs[(4 * q + 3) * T::BS + bpx] = rb[r].w;
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int kl = lane >> 4, cl = lane & 15;
    const bool active = ci0 + wci * 64 < g.Cin;    // wave-uniform
    if (KS > 0) {                                   // a class without taps: zeros
        load(0);
        store(smem);
        __syncthreads();
    }
    for (int ks = 0; ks < KS; ++ks) {
        const float* st = smem + (ks & 1) * T::STAGE;
        const float* As = st + wci * 64 + cl;
        const float* Bs = st + kK * T::AS + wpx * 64 + cl;
        if (ks + 1 < KS) load(ks + 1);
        if (active) {
#pragma unroll
            for (int t = 0; t < kK / 4; ++t) {
                const int k = 4 * t + kl;
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
        if (ks + 1 < KS) store(smem + ((ks + 1) & 1) * T::STAGE);
        __syncthreads();
    }

    // D tile (i, j): lane holds channels ci0 + wci*64 + 16 i + 4 (lane >> 4) + v of the class's
    // pixel px0 + wpx*64 + 16 j + (lane & 15)
    const int cbase = ci0 + wci * 64 + 4 * kl;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pc = px0 + wpx * 64 + 16 * j + cl;
        if (pc >= Pc) continue;
        const int nn = pc / hw;
        const int r = pc - nn * hw;
        const int jh = r / aw.cnt, jw = r - jh * aw.cnt;
        const int ih = ah.a + s * jh, iw = aw.a + s * jw;
        float* xp = dx + (((long long)nn * g.H + ih) * g.W + iw) * g.Cin + cbase;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (cbase + 16 * i < g.Cin) *reinterpret_cast<f32x4*>(xp + 16 * i) = acc[i][j];
    }
}

struct Plan {
    DGeom g;
    bool wide;                 // 128 x 128 tiles (Cin > 64), else 64 x 256
    int32_t taps[4];           // per class in (r_h, r_w) row-major order
    int64_t pixels[4], tiles[4];
};

int plan_for(const mcgmil_conv_dgrad_args* a, Plan& pl) {
    if (!a) return fail(MCGMIL_E_INVALID, "args is NULL");
    const mcgmil_conv_args& f = a->fwd;
    if (a->reserved != 0) return fail(MCGMIL_E_INVALID, "reserved must be 0");
    if (f.batch < 1 || f.height < 1 || f.width < 1)
        return fail(MCGMIL_E_INVALID, "batch, height and width must be >= 1");
    if (f.in_channels < 16 || f.in_channels % 16 != 0)
        return fail(MCGMIL_E_UNSUPPORTED, "data gradient: in_channels a multiple of 16");
    if (f.out_channels < 64 || f.out_channels % 64 != 0)
        return fail(MCGMIL_E_UNSUPPORTED, "data gradient: out_channels a multiple of 64");
    if (f.kernel_h < 1 || f.kernel_w < 1 || f.kernel_h > 7 || f.kernel_w > 7)
        return fail(MCGMIL_E_UNSUPPORTED, "kernel size must be in 1..7");
    if (f.stride != 1 && f.stride != 2) return fail(MCGMIL_E_UNSUPPORTED, "data gradient: stride 1 or 2");
    if (f.pad < 0) return fail(MCGMIL_E_INVALID, "pad must be >= 0");
    if (f.pad >= f.kernel_h || f.pad >= f.kernel_w)
        return fail(MCGMIL_E_UNSUPPORTED, "data gradient: pad must be smaller than the kernel");
    if ((long long)f.height + 2ll * f.pad < f.kernel_h || (long long)f.width + 2ll * f.pad < f.kernel_w)
        return fail(MCGMIL_E_INVALID, "the kernel does not fit the padded input");
    const long long oh = ((long long)f.height + 2ll * f.pad - f.kernel_h) / f.stride + 1;
    const long long ow = ((long long)f.width + 2ll * f.pad - f.kernel_w) / f.stride + 1;
    long long xel = 0, yel = 0;
    if (__builtin_mul_overflow((long long)f.batch * f.height, (long long)f.width * f.in_channels, &xel) ||
        xel >= (1ll << 60) || __builtin_mul_overflow((long long)f.batch * oh, ow * f.out_channels, &yel) ||
        yel >= (1ll << 60))
        return fail(MCGMIL_E_UNSUPPORTED, "dx or dy too large");
    const long long wel = (long long)f.out_channels * f.in_channels;     // < 2^62
    if (wel >= (1ll << 34) || wel * f.kernel_h * f.kernel_w >= (1ll << 34))
        return fail(MCGMIL_E_UNSUPPORTED, "weight too large (out * kh * kw * in must be < 2^34)");
    DGeom& g = pl.g;
    g.N = f.batch; g.H = f.height; g.W = f.width; g.Cin = f.in_channels; g.Cout = f.out_channels;
    g.KH = f.kernel_h; g.KW = f.kernel_w; g.stride = f.stride; g.pad = f.pad;
    g.OH = (int)oh; g.OW = (int)ow;
    pl.wide = f.in_channels > 64;
    const int bm = pl.wide ? 128 : 256;
    const int s = f.stride;
    g.ncls = s * s;
    for (int c = 0; c < 4; ++c) {
        pl.taps[c] = 0;
        pl.pixels[c] = pl.tiles[c] = 0;
    }
    for (int c = 0; c < g.ncls; ++c) {
        const Axis ah = axis_of(c / s, g.H, g.KH, s, g.pad), aw = axis_of(c % s, g.W, g.KW, s, g.pad);
        const long long px = (long long)f.batch * ah.cnt * aw.cnt;     // <= xel / 16 < 2^56
        if (px >= (1ll << 31) - 256)
            return fail(MCGMIL_E_UNSUPPORTED, "too many input pixels in a class (must be < 2^31 - 256)");
        pl.taps[c] = ah.taps * aw.taps;
        pl.pixels[c] = px;
        pl.tiles[c] = (px + bm - 1) / bm;
    }
    // grid order: most taps first (stable), so the short classes fill the tail
    int order[4] = {0, 1, 2, 3};
    for (int i = 1; i < g.ncls; ++i)
        for (int j = i; j > 0 && pl.taps[order[j]] > pl.taps[order[j - 1]]; --j) {
            const int t = order[j];
            order[j] = order[j - 1];
            order[j - 1] = t;
        }
    long long t0 = 0;                                                   // < 4 * 2^31 / 128 = 2^26
    for (int q = 0; q < 4; ++q) {
        g.res[q] = 0;
        g.tile0[q] = (int)t0;
        if (q < g.ncls) {
            g.res[q] = (order[q] / s) | ((order[q] % s) << 4);
            t0 += pl.tiles[order[q]];
        }
    }
    g.tile0[4] = (int)t0;
    return MCGMIL_OK;
}

template <int WCI, int WPX>
int launch_dgrad(const Plan& pl, const float* dy, const float* wt, float* dx, hipStream_t s) {
    using T = Tile<WCI, WPX>;
    const DGeom& g = pl.g;
    dim3 grid((unsigned)g.tile0[4], (unsigned)((g.Cin + T::BN_CI - 1) / T::BN_CI));
    hipLaunchKernelGGL((dgrad_kernel<WCI, WPX>), grid, dim3(256), 0, s, g, dy, wt, dx);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCGMIL_OK : hip_fail(e, "dgrad_kernel launch");
}

}  // namespace

extern "C" {

size_t mcgmil_conv_dgrad_args_size(void) { return sizeof(mcgmil_conv_dgrad_args); }

int mcgmil_conv_dgrad_classes(const mcgmil_conv_dgrad_args* a, int32_t taps[4], int64_t pixels[4],
                              int64_t tiles[4]) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!taps || !pixels || !tiles) return fail(MCGMIL_E_INVALID, "taps, pixels or tiles is NULL");
    for (int c = 0; c < 4; ++c) {
        taps[c] = pl.taps[c];
        pixels[c] = pl.pixels[c];
        tiles[c] = pl.tiles[c];
    }
    return MCGMIL_OK;
}

int mcgmil_conv2d_dgrad_f32(const mcgmil_conv_dgrad_args* a, void* stream) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!a->dy || !a->w_t || !a->dx) return fail(MCGMIL_E_INVALID, "NULL dy, w_t or dx");
    if (((uintptr_t)a->dy | (uintptr_t)a->w_t | (uintptr_t)a->dx) & 15u)
        return fail(MCGMIL_E_INVALID, "dy, w_t and dx must be 16-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return pl.wide ? launch_dgrad<2, 2>(pl, a->dy, a->w_t, a->dx, s)
                   : launch_dgrad<1, 4>(pl, a->dy, a->w_t, a->dx, s);
}

}  // extern "C"
