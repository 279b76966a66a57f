// bf16 data gradient of the backbone's convolutions (include/mcgmil_conv_dgrad_bf16.h): the
// backward of mcgmil_conv2d with respect to its input, stride 1 and 2, on v_mfma_f32_16x16x32_bf16
// with bf16 operands, fp32 accumulation and one rounding to nearest-even at the store. Reference:
// loss.backward() through torch.nn.Conv2d under autocast to bf16 (model.py:166-179, the ResNet
// feature extractor under net_utils.train_gacc). The bf16 sibling of mcgmil_conv_dgrad.hip; the
// small host plan (Axis, axis_of, the class order) is that file's, restated.
//
// Residue classes: input pixel (ih, iw) belongs to class (r_h, r_w) = ((ih + p) mod s, (iw + p) mod s).
// Its rows are ih = a_h + s j_h with a_h = (r_h - p) mod s, j_h = 0 .. Hc - 1 (columns likewise), and
// only the taps kh = r_h + s m_h < KH, kw = r_w + s m_w < KW reach it, from the output pixel
// oh = j_h + c_h - m_h with c_h = (a_h + p - r_h) / s (exact), ow likewise. Inside a class the data
// gradient is therefore a stride-1 implicit GEMM without zero insertion.
//
// GEMM view: rows = input channels (the A operand: the weight image [kh][kw][in][out], so a row is
// one input channel's 32 consecutive out values of a tap), columns = the class's input pixels (the
// B operand: the 32 out values of dY at (n, oh, ow), zero when the tap's output pixel lies outside
// dY), K = (tap, out) in steps of 32 out channels of one tap, taps in (kh, kw) order. Both operands
// are k-contiguous rows, in global memory and in LDS alike: a lane's fragment (k = 8 (lane >> 4) ..
// + 7 of row / column lane & 15) is one ds_read_b128, and there are no transposed reads.
//
// LDS: two stages of [rows][32 bf16 + 16 pad] = 96-byte rows; the next step waits in registers
// while the current one computes. With the 96-byte stride the 16-byte slot of (row, chunk) is
// (6 row + chunk) mod 16 for the reads (64 banks): each 16-lane group of ds_read_b128 takes eight
// rows of one chunk and eight of the next, which land on the eight even and the eight odd slots,
// so the reads are conflict-free. The staging stores are ds_write_b128 (32 banks, groups of 8
// consecutive lanes); a group is laid over 4 consecutive rows x 2 adjacent chunks, slots
// (6 row + chunk) mod 8 = {0, 6, 4, 2} + {0, 1}: conflict-free too.
//
// 4 waves, each a 64 x 64 block of 4 x 4 MFMA tiles; tiles of 128 channels x 128 pixels, or
// 64 x 256 when Cin == 64. Grid: x = the classes' pixel tiles one class after another, heaviest
// (most taps) first so the short ones fill the tail; y = the channel tile. A workgroup owns pixels
// of ONE class, so its tap list is uniform. A tile of a class without taps stages nothing and
// stores zeros; a wave whose 64 channel rows lie past Cin (Cin = 64 (2 n + 1), last tile) skips its
// MFMAs and stores. Every dx element is written exactly once by one lane, as one 8-byte store of 4
// consecutive channels: no split-K, no atomics, no workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcgmil.h"
#include "../../include/mcgmil_conv_dgrad_bf16.h"
#include "mcgmil_error.h"

namespace {

using mcgmil_detail::fail;
using mcgmil_detail::hip_fail;

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

constexpr int kK = 32;       // K step (output channels of one tap): one v_mfma_f32_16x16x32_bf16 deep
constexpr int kRow = 48;     // LDS row stride (bf16): 32 + 16 pad = 96 bytes

struct DGeom {
    int N, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW;
    int ncls;              // stride^2 classes, in grid order
    int res[4];            // r_h | r_w << 4 of the class
    int tile0[5];          // the class's first pixel tile on the grid's x axis; tile0[ncls] = gridDim.x
};

template <int WCI, int WPX>
struct Tile {
    static constexpr int BN_CI = 64 * WCI, BM_PX = 64 * WPX;
    static constexpr int STAGE = (BN_CI + BM_PX) * kRow;                     // bf16 per stage
    static_assert(WCI * WPX == 4 && 2 * STAGE * 2 <= 64 * 1024, "4 waves, static LDS");
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
__global__ __launch_bounds__(256, 2) void dgrad_bf16_kernel(const DGeom g, const __bf16* __restrict__ dy,
                                                            const __bf16* __restrict__ wt, __bf16* __restrict__ dx) {
    using T = Tile<WCI, WPX>;
    __shared__ __attribute__((aligned(16))) __bf16 smem[2 * T::STAGE];
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

    // Staging map: thread -> (row srow + 64 r, 16-byte chunk sch) of the A rows and of the B rows.
    // 8 consecutive lanes cover 4 rows x 2 chunks (the ds_write_b128 bank rule above); a wave
    // covers 16 rows x 4 chunks, whole 64-byte row pieces of global memory.
    const int srow = 4 * (tid >> 4) + ((tid >> 1) & 3);
    const int sch = 2 * ((tid >> 3) & 1) + (tid & 1);
    // the thread's B pixels: element offset of image n in dY, and (j_h + c_h, j_w + c_w); a pixel
    // past the class's last gets qh = -8, so every tap's oh is negative and it stages zeros
    int nb[WPX], qh[WPX], qw[WPX];
#pragma unroll
    for (int r = 0; r < WPX; ++r) {
        const int pc = px0 + srow + 64 * r;
        nb[r] = 0;
        qh[r] = -8;
        qw[r] = 0;
        if (pc < Pc) {
            const int n = pc / hw;
            const int rem = pc - n * hw;
            const int jh = rem / aw.cnt;
            nb[r] = n * g.OH * g.OW;
            qh[r] = jh + ah.c;
            qw[r] = rem - jh * aw.cnt + aw.c;
        }
    }

    u32x4 ra[WCI], rb[WPX];
    auto load = [&](int ks) {
        const int tap = ks / cch, co0 = (ks - tap * cch) * kK + 8 * sch;
        const int mh = tap / aw.taps, mw = tap - mh * aw.taps;
        const int kh = rh + s * mh, kw = rw + s * mw;
        // A: wt[kh][kw][ci0 + row][co0 ..]; channel rows past Cin are zero rows
        const __bf16* wk = wt + ((long long)(kh * g.KW + kw) * g.Cin + ci0) * g.Cout + co0;
#pragma unroll
        for (int r = 0; r < WCI; ++r) {
            const int row = srow + 64 * r;
            ra[r] = ci0 + row < g.Cin ? *reinterpret_cast<const u32x4*>(wk + (long long)row * g.Cout)
                                      : u32x4{0u, 0u, 0u, 0u};
        }
        // B: dy[n, oh, ow, co0 ..] of the thread's pixels (zero outside dY); dy is below 2^31 bytes
#pragma unroll
        for (int r = 0; r < WPX; ++r) {
            const int oh = qh[r] - mh, ow = qw[r] - mw;
            const bool in = oh >= 0 && oh < g.OH && ow >= 0 && ow < g.OW;
            rb[r] = in ? *reinterpret_cast<const u32x4*>(dy + (nb[r] + oh * g.OW + ow) * g.Cout + co0)
                       : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto store = [&](__bf16* st) {
        __bf16* As = st + srow * kRow + 8 * sch;
        __bf16* Bs = As + T::BN_CI * kRow;
#pragma unroll
        for (int r = 0; r < WCI; ++r) *reinterpret_cast<u32x4*>(As + 64 * r * kRow) = ra[r];
#pragma unroll
        for (int r = 0; r < WPX; ++r) *reinterpret_cast<u32x4*>(Bs + 64 * r * kRow) = rb[r];
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
        const __bf16* st = smem + (ks & 1) * T::STAGE;
        const __bf16* As = st + (wci * 64 + cl) * kRow + 8 * kl;
        const __bf16* Bs = st + (T::BN_CI + wpx * 64 + cl) * kRow + 8 * kl;
        if (ks + 1 < KS) load(ks + 1);
        if (active) {
            bf16x8 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bf16x8*>(As + 16 * i * kRow);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const bf16x8*>(Bs + 16 * j * kRow);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (ks + 1 < KS) store(smem + ((ks + 1) & 1) * T::STAGE);
        __syncthreads();
    }
    if (!active) return;

    // D tile (i, j): lane holds channels ci0 + wci*64 + 16 i + 4 (lane >> 4) + v of the class's
    // pixel px0 + wpx*64 + 16 j + (lane & 15); dx is below 2^31 bytes
    const int cbase = ci0 + wci * 64 + 4 * kl;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pc = px0 + wpx * 64 + 16 * j + cl;
        if (pc >= Pc) continue;
        const int nn = pc / hw;
        const int r = pc - nn * hw;
        const int jh = r / aw.cnt, jw = r - jh * aw.cnt;
        const int ih = ah.a + s * jh, iw = aw.a + s * jw;
        __bf16* xp = dx + ((nn * g.H + ih) * g.W + iw) * g.Cin + cbase;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bf16x4 o;
#pragma unroll
            for (int v = 0; v < 4; ++v) o[v] = (__bf16)acc[i][j][v];
            *reinterpret_cast<bf16x4*>(xp + 16 * i) = o;
        }
    }
}

struct Plan {
    DGeom g;
    bool wide;                 // 128 x 128 tiles (Cin > 64), else 64 x 256
    int32_t taps[4];           // per class in (r_h, r_w) row-major order
    int64_t pixels[4], tiles[4];
};

int plan_for(const mcgmil_conv_dgrad_bf16_args* a, Plan& pl) {
    if (!a) return fail(MCGMIL_E_INVALID, "args is NULL");
    const mcgmil_conv_args& f = a->fwd;
    if (a->reserved != 0) return fail(MCGMIL_E_INVALID, "reserved must be 0");
    if (f.batch < 1 || f.height < 1 || f.width < 1)
        return fail(MCGMIL_E_INVALID, "batch, height and width must be >= 1");
    if (f.in_channels < 64 || f.in_channels % 64 != 0)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16 data gradient: in_channels a multiple of 64");
    if (f.out_channels < 64 || f.out_channels % 64 != 0)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16 data gradient: out_channels a multiple of 64");
    if (f.kernel_h < 1 || f.kernel_w < 1 || f.kernel_h > 7 || f.kernel_w > 7)
        return fail(MCGMIL_E_UNSUPPORTED, "kernel size must be in 1..7");
    if (f.stride != 1 && f.stride != 2) return fail(MCGMIL_E_UNSUPPORTED, "bf16 data gradient: stride 1 or 2");
    if (f.pad < 0) return fail(MCGMIL_E_INVALID, "pad must be >= 0");
    if (f.pad >= f.kernel_h || f.pad >= f.kernel_w)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16 data gradient: pad must be smaller than the kernel");
    if ((long long)f.height + 2ll * f.pad < f.kernel_h || (long long)f.width + 2ll * f.pad < f.kernel_w)
        return fail(MCGMIL_E_INVALID, "the kernel does not fit the padded input");
    const long long oh = ((long long)f.height + 2ll * f.pad - f.kernel_h) / f.stride + 1;
    const long long ow = ((long long)f.width + 2ll * f.pad - f.kernel_w) / f.stride + 1;
    // the kernel's offsets into dx and dy are 32-bit element offsets
    long long xel = 0, yel = 0;
    if (__builtin_mul_overflow((long long)f.batch * f.height, (long long)f.width * f.in_channels, &xel) ||
        xel >= (1ll << 30) || __builtin_mul_overflow((long long)f.batch * oh, ow * f.out_channels, &yel) ||
        yel >= (1ll << 30))
        return fail(MCGMIL_E_UNSUPPORTED, "bf16 data gradient: dx and dy must be below 2^31 bytes each");
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
        const long long px = (long long)f.batch * ah.cnt * aw.cnt;     // <= xel / 64 < 2^24
        if (px >= (1ll << 31) - 256)                                    // implied by the byte limit above
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
    long long t0 = 0;                                                   // < 4 * 2^24 / 128 + 4
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
int launch_dgrad(const Plan& pl, const __bf16* dy, const __bf16* wt, __bf16* dx, hipStream_t s) {
    using T = Tile<WCI, WPX>;
    const DGeom& g = pl.g;
    dim3 grid((unsigned)g.tile0[4], (unsigned)((g.Cin + T::BN_CI - 1) / T::BN_CI));
    hipLaunchKernelGGL((dgrad_bf16_kernel<WCI, WPX>), grid, dim3(256), 0, s, g, dy, wt, dx);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCGMIL_OK : hip_fail(e, "dgrad_bf16_kernel launch");
}

}  // namespace

extern "C" {

size_t mcgmil_conv_dgrad_bf16_args_size(void) { return sizeof(mcgmil_conv_dgrad_bf16_args); }

int mcgmil_conv_dgrad_classes_bf16(const mcgmil_conv_dgrad_bf16_args* a, int32_t taps[4], int64_t pixels[4],
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

int mcgmil_conv2d_dgrad_bf16(const mcgmil_conv_dgrad_bf16_args* a, void* stream) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!a->dy || !a->w_t || !a->dx) return fail(MCGMIL_E_INVALID, "NULL dy, w_t or dx");
    if (((uintptr_t)a->dy | (uintptr_t)a->w_t | (uintptr_t)a->dx) & 15u)
        return fail(MCGMIL_E_INVALID, "dy, w_t and dx must be 16-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const __bf16* dy = static_cast<const __bf16*>(a->dy);
    const __bf16* wt = static_cast<const __bf16*>(a->w_t);
    __bf16* dx = static_cast<__bf16*>(a->dx);
    return pl.wide ? launch_dgrad<2, 2>(pl, dy, wt, dx, s) : launch_dgrad<1, 4>(pl, dy, wt, dx, s);
}

}  // extern "C"
