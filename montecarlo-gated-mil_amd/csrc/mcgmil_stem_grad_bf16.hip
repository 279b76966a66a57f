// bf16 weight gradient of the stem convolution (include/mcgmil_stem_grad_bf16.h): the backward of
// mcgmil_stem_conv_bf16 / mcgmil_stem_forward's convolution with respect to its weight, on
// v_mfma_f32_16x16x32_bf16 with bf16 operands and fp32 accumulation, dW in fp32. Reference:
// loss.backward() through conv1 = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False) under
// torch.autocast("cuda", torch.bfloat16) (model.py:166-179, the ResNet feature extractor under
// net_utils.train_gacc).
//
// GEMM view: rows = the 64 output channels o (the A operand, dY), columns = (ci, kh, j), j = 0..7
// (the B operand, the tap-shifted x), K = output pixels. The column order is the forward kernel's
// (mcgmil_stem.hip): tap j of pixel ow is input column iw = 2 ow - P + j with P = pad rounded up to
// even, i.e. kernel column kw = j - (P - pad); the taps outside 0..k-1 are dead columns, summed like
// the others and dropped by the reduce kernel (j = 0 for the 7x7 / pad-3 stem). That order is what
// makes the x operand cheap: 2 ow - P is even and so is the width, so the 8 taps of one (pixel, ci,
// kh) are four whole dwords of one NCHW input row, each wholly inside the row or wholly outside it.
// Cin * k * 8 columns (168 for the stem, at most 256) are one tile: a workgroup of 4 waves computes
// 64 output channels x all columns of one granule of MCGMIL_WGRAD_GRANULE_PIXELS output pixels,
// each wave all 64 channels x NBW blocks of 16 columns (NBW = 1..4, the stem's 11 blocks take 3).
// The waves split the columns, not the pixels: no cross-wave sum exists and the order of every
// addition is a function of the geometry alone.
//
// A K step is 32 output pixels (one MFMA deep). Both operands are staged k-major, as in
// mcgmil_conv_grad_bf16.hip: [32][64 + 16] bf16 of dY (a pixel of dY is a contiguous row of 64 in
// NHWC: one 16-byte load per thread) and [32][64 NBW + 16] bf16 of x, where thread t fills the
// 8-column groups (t & 7) + 8 r of pixel t >> 3 with four predicated dword loads and one aligned
// 16-byte LDS write each (8 consecutive lanes write 128 contiguous bytes). Rows outside the image,
// dwords outside the row, groups past Cin * k and pixels past the granule are written as zeros; no
// address is clamped or wrapped, and none outside x is dereferenced. The fragments are read with
// ds_read_b64_tr_b16 under that kernel's rules: every lane address 8-byte aligned, no
// lane-dependent guard around the reads (the `active` skip is wave-uniform), a row stride of 32
// bytes mod 64 so that the 8 k rows of a 32-lane half land on 8 different 32-byte bank slots. The
// next K step is loaded into registers while the current one computes.
//
// Every granule writes its partial sums to the workspace as [granule][column][o];
// stem_wgrad_bf16_reduce_kernel adds them in granule order to a running sum and, after the last
// chunk, writes the live taps to dW in torch's [o][ci][kh][kw] layout. No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcgmil.h"
#include "../../include/mcgmil_stem_grad_bf16.h"
#include "mcgmil_error.h"

namespace {

using mcgmil_detail::fail;
using mcgmil_detail::hip_fail;

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) short i16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

constexpr int kK = 32;     // K step (output pixels): one v_mfma_f32_16x16x32_bf16 deep
constexpr int kBM = 64;    // output channels
constexpr int kPad = 16;   // LDS row pad (bf16 elements): 32 bytes, see the bank note above
constexpr int kGranule = MCGMIL_WGRAD_GRANULE_PIXELS;
static_assert(kGranule % kK == 0, "a granule is a whole number of K steps");

struct SGeom {
    int N, Cin, H, W, OH, OW, k, pad, P;
    int W2;               // dwords per input row: W / 2
    int groups;           // Cin * k: (ci, kh) rows, 8 columns each
    int Ncols;            // 8 * groups
    long long Pix;        // N * OH * OW output pixels
};

template <int NBW>
struct STile {
    static constexpr int BN = 64 * NBW;                         // columns of the stage (4 waves x NBW blocks)
    static constexpr int AS = kBM + kPad, BS = BN + kPad;      // row strides (bf16)
    static constexpr int STAGE = kK * (AS + BS);               // bf16 per stage
    // an odd number of 32-byte slots per row: 8 consecutive rows hit 8 different slots of the 256
    static_assert((AS * 2) % 64 == 32 && (BS * 2) % 64 == 32, "LDS row stride and the banks");
};

// The 4 x 16 block at p (this lane's row and 4 columns of it), column-major: ds_read_b64_tr_b16.
__device__ __forceinline__ i16x4 read_tr(const __bf16* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)p);
}

// part: [granules of the chunk][Ncols][64]. pix0: the chunk's first output pixel (a multiple of the
// granule). blockIdx.x = granule in the chunk. xd: x as dwords (pairs of input columns).
template <int NBW>
__global__ __launch_bounds__(256, 2) void stem_wgrad_bf16_kernel(const SGeom g, const uint32_t* __restrict__ xd,
                                                                 const __bf16* __restrict__ dy,
                                                                 float* __restrict__ part, long long pix0) {
    using T = STile<NBW>;
    __shared__ __attribute__((aligned(16))) __bf16 smem[2 * T::STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gl = blockIdx.x;
    const long long pbeg = pix0 + (long long)gl * kGranule;
    const long long pend = pbeg + kGranule < g.Pix ? pbeg + kGranule : g.Pix;
    const int steps = (int)((pend - pbeg + kK - 1) / kK);

    // staging: row sk of the step's 32 pixels; 16-byte chunk sc of its 64 dY values and the
    // 8-column groups sc + 8 r of x. Per group, fixed for the kernel: kh (far below -H - pad when
    // the group is past Cin * k, so that its row is never inside the image) and the dword offset
    // of (ci, kh) from the window's first row.
    const int sk = tid >> 3, sc = tid & 7;
    int gkh[NBW], goff[NBW];
#pragma unroll
    for (int r = 0; r < NBW; ++r) {
        const int grp = sc + 8 * r;
        const bool gvalid = grp < g.groups;
        const int ci = gvalid ? grp / g.k : 0, kh = gvalid ? grp - ci * g.k : 0;
        gkh[r] = gvalid ? kh : -(1 << 28);
        goff[r] = (ci * g.H + kh) * g.W2;
    }
    const unsigned ohw = (unsigned)(g.OH * g.OW);
    const int P2 = g.P >> 1;

    u32x4 ra, rb[NBW];
    auto load = [&](int ks) {
        const long long p = pbeg + (long long)ks * kK + sk;
        const bool in = p < pend;
        ra = in ? *reinterpret_cast<const u32x4*>(dy + p * kBM + 8 * sc) : u32x4{0u, 0u, 0u, 0u};
        const unsigned pu = in ? (unsigned)p : 0u;      // Pix < 2^31
        const unsigned n = pu / ohw, rem = pu - n * ohw;
        const unsigned oh = rem / (unsigned)g.OW, ow = rem - oh * (unsigned)g.OW;
        const int ih0 = 2 * (int)oh - g.pad, d0 = (int)ow - P2;     // first row, first dword of the window
        // the window's origin in dwords; it may lie before x, and is only dereferenced at rows and
        // dwords inside the image (x < 2 GiB: every offset fits an int)
        const int base = ((int)n * g.Cin * g.H + ih0) * g.W2 + d0;
        bool dok[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) dok[d] = in && (unsigned)(d0 + d) < (unsigned)g.W2;
#pragma unroll
        for (int r = 0; r < NBW; ++r) {
            const bool rok = (unsigned)(ih0 + gkh[r]) < (unsigned)g.H;
            const uint32_t* src = xd + ((long long)base + goff[r]);
            u32x4 v;
            v.x = rok && dok[0] ? src[0] : 0u;
            v.y = rok && dok[1] ? src[1] : 0u;
            v.z = rok && dok[2] ? src[2] : 0u;
            v.w = rok && dok[3] ? src[3] : 0u;
            rb[r] = v;
        }
    };
    auto store = [&](__bf16* st) {
        *reinterpret_cast<u32x4*>(st + sk * T::AS + 8 * sc) = ra;
        __bf16* Bs = st + kK * T::AS + sk * T::BS + 8 * sc;
#pragma unroll
        for (int r = 0; r < NBW; ++r) *reinterpret_cast<u32x4*>(Bs + 64 * r) = rb[r];
    };

    f32x4 acc[4][NBW];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NBW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // transposed-read address of this lane: group kl = lane >> 4 takes k rows 4 kl + q (first read)
    // and 16 + 4 kl + q (second), lane 4q + p of the group supplies row q, columns 4p .. 4p + 3
    const int kl = lane >> 4, cl = lane & 15;
    const int trow = 4 * kl + (cl >> 2), tcol = 4 * (cl & 3);
    const int wcol = wave * 16 * NBW;                   // this wave's first column
    const bool active = wcol < g.Ncols;                 // wave-uniform
    load(0);
    store(smem);
    __syncthreads();
    for (int ks = 0; ks < steps; ++ks) {
        const __bf16* st = smem + (ks & 1) * T::STAGE;
        const __bf16* As = st + trow * T::AS + tcol;
        const __bf16* Bs = st + kK * T::AS + trow * T::BS + wcol + tcol;
        if (ks + 1 < steps) load(ks + 1);
        if (active) {
            bf16x8 a[4], b[NBW];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const i16x4 lo = read_tr(As + 16 * i), hi = read_tr(As + 16 * T::AS + 16 * i);
                a[i] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
            }
#pragma unroll
            for (int j = 0; j < NBW; ++j) {
                const i16x4 lo = read_tr(Bs + 16 * j), hi = read_tr(Bs + 16 * T::BS + 16 * j);
                b[j] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NBW; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (ks + 1 < steps) store(smem + ((ks + 1) & 1) * T::STAGE);
        __syncthreads();
    }

    // D tile (i, j): lane holds o = 16 i + 4 (lane >> 4) + v of column wcol + 16 j + (lane & 15)
    float* pg = part + (long long)gl * g.Ncols * kBM;
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
        const int nn = wcol + 16 * j + cl;
        if (nn >= g.Ncols) continue;
        float* pp = pg + (long long)nn * kBM + 4 * kl;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(pp + 16 * i) = acc[i][j];
    }
}

constexpr int kRE = 32;          // elements per reduce workgroup: one 128-byte line of every partial
constexpr int kRU = 16;          // partials in flight per thread
constexpr int kRB = 8 * kRU;     // partials per batch: 8 threads load for one element

// sum[e] (+)= part[0][e] + part[1][e] + ... in granule order; the last chunk writes
// dW[o][ci][kh][kw] instead of the running sum and drops the dead taps. e = column * 64 + o,
// column = (ci * k + kh) * 8 + j, kw = j - dead. With one tile there are few elements (10,752 for
// the stem) and many granules (9,231 at 1,507 instances), so one thread per element reading its
// partials one after the other is bound by the latency of a few loads in flight. Here a workgroup
// takes 32 elements: all 256 threads fetch a batch of 128 partials of them (16 independent loads
// each) into LDS while the first 32 threads add the previous batch, each its own element, one
// partial after the other -- the order of the additions is the sequential one, whatever the batch.
__global__ __launch_bounds__(256) void stem_wgrad_bf16_reduce_kernel(const float* __restrict__ part,
                                                                     float* __restrict__ sum, float* __restrict__ dw,
                                                                     int E, int granules, int first, int last, int Cin,
                                                                     int k, int dead) {
    __shared__ float buf[kRB][kRE];
    const int tid = threadIdx.x, el = tid & (kRE - 1), slot = tid / kRE;
    const int e = blockIdx.x * kRE + el;                    // E is a multiple of 512: always < E
    const float* src = part + e;
    float v[kRU];
    auto load = [&](int g0) {                               // partials g0 + 8 u + slot
#pragma unroll
        for (int u = 0; u < kRU; ++u) {
            const int gi = g0 + 8 * u + slot;
            v[u] = gi < granules ? src[(long long)gi * E] : 0.f;
        }
    };
    float s = tid < kRE && !first ? sum[e] : 0.f;
    load(0);
    for (int g0 = 0; g0 < granules; g0 += kRB) {
#pragma unroll
        for (int u = 0; u < kRU; ++u) buf[8 * u + slot][el] = v[u];
        __syncthreads();
        if (g0 + kRB < granules) load(g0 + kRB);
        if (tid < kRE) {
            const int n = granules - g0 < kRB ? granules - g0 : kRB;     // never the zeros past the last partial
#pragma unroll 16
            for (int j = 0; j < n; ++j) s += buf[j][el];
        }
        __syncthreads();
    }
    if (tid >= kRE) return;
    if (!last) {
        sum[e] = s;
        return;
    }
    const int o = e % kBM, c = e / kBM;
    const int grp = c >> 3, kw = (c & 7) - dead;
    const int ci = grp / k, kh = grp - ci * k;
    if (kw >= 0 && kw < k) dw[((o * Cin + ci) * k + kh) * k + kw] = s;
}

struct Plan {
    SGeom g;
    int E;                             // 64 * Ncols
    long long gran_total, gran_chunk;
    int nbw;                           // column blocks per wave: 1..4
    size_t total;                      // workspace bytes
};

int plan_for(const mcgmil_stem_grad_bf16_args* a, Plan& pl) {
    if (!a) return fail(MCGMIL_E_INVALID, "args is NULL");
    const mcgmil_stem_args& f = a->fwd;
    if (a->reserved != 0) return fail(MCGMIL_E_INVALID, "reserved must be 0");
    if (a->chunk_pixels < 0) return fail(MCGMIL_E_INVALID, "chunk_pixels must be >= 0");
    if (f.batch < 1 || f.height < 1 || f.width < 1)
        return fail(MCGMIL_E_INVALID, "batch, height and width must be >= 1");
    if (f.in_channels < 1 || f.in_channels > 4)
        return fail(MCGMIL_E_UNSUPPORTED, "bf16 stem weight gradient: in_channels must be in 1..4");
    if (f.out_channels != kBM) return fail(MCGMIL_E_UNSUPPORTED, "bf16 stem weight gradient: 64 output channels");
    if (f.kernel < 1 || f.stride != 2 || f.pad < 0 || f.kernel > 8 - (f.pad & 1))
        return fail(MCGMIL_E_UNSUPPORTED, "bf16 stem weight gradient: stride 2 and kernel + (pad & 1) <= 8");
    if (f.width & 1) return fail(MCGMIL_E_UNSUPPORTED, "bf16 stem weight gradient: an even width");
    const long long oh = ((long long)f.height + 2ll * f.pad - f.kernel) / 2 + 1;
    const long long ow = ((long long)f.width + 2ll * f.pad - f.kernel) / 2 + 1;
    if ((long long)f.height + 2ll * f.pad < f.kernel || (long long)f.width + 2ll * f.pad < f.kernel || oh < 1 || ow < 1)
        return fail(MCGMIL_E_INVALID, "the kernel does not fit the padded input");
    if (ow > 125) return fail(MCGMIL_E_UNSUPPORTED, "bf16 stem weight gradient: OW <= 125");
    long long xel = 0, pix = 0;
    if (__builtin_mul_overflow((long long)f.batch * f.in_channels, (long long)f.height * f.width, &xel) ||
        xel >= (1ll << 30))
        return fail(MCGMIL_E_UNSUPPORTED, "input larger than 2 GiB");
    if (__builtin_mul_overflow((long long)f.batch * oh, ow, &pix) || pix >= (1ll << 31) - 256)
        return fail(MCGMIL_E_UNSUPPORTED, "too many output pixels (batch * OH * OW must be < 2^31 - 256)");
    SGeom& g = pl.g;
    g.N = f.batch; g.Cin = f.in_channels; g.H = f.height; g.W = f.width;
    g.OH = (int)oh; g.OW = (int)ow; g.k = f.kernel; g.pad = f.pad; g.P = f.pad + (f.pad & 1);
    g.W2 = f.width / 2;
    g.groups = f.in_channels * f.kernel;                    // <= 32
    g.Ncols = 8 * g.groups;                                 // <= 256
    g.Pix = pix;
    pl.E = g.Ncols * kBM;                                   // <= 16384
    pl.nbw = (g.Ncols + 63) / 64;                           // ceil(ceil(Ncols / 16) / 4)
    pl.gran_total = (pix + kGranule - 1) / kGranule;        // < 2^20: the grid
    const long long ebytes = (long long)pl.E * 4;           // a multiple of 256
    long long gc = a->chunk_pixels ? a->chunk_pixels / kGranule : MCGMIL_WGRAD_DEFAULT_PARTIAL_BYTES / ebytes;
    if (gc < 1) gc = 1;
    if (gc > pl.gran_total) gc = pl.gran_total;
    pl.gran_chunk = gc;
    pl.total = (size_t)((gc + 1) * ebytes);                 // < 2^21 * 2^16
    return MCGMIL_OK;
}

template <int NBW>
int launch_wgrad(const Plan& pl, const uint32_t* xd, const __bf16* dy, float* part, long long pix0, long long granules,
                 hipStream_t s) {
    hipLaunchKernelGGL((stem_wgrad_bf16_kernel<NBW>), dim3((unsigned)granules), dim3(256), 0, s, pl.g, xd, dy, part,
                       pix0);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCGMIL_OK : hip_fail(e, "stem_wgrad_bf16_kernel launch");
}

}  // namespace

extern "C" {

size_t mcgmil_stem_grad_bf16_args_size(void) { return sizeof(mcgmil_stem_grad_bf16_args); }

int mcgmil_stem_wgrad_workspace_size_bf16(const mcgmil_stem_grad_bf16_args* a, size_t* bytes) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!bytes) return fail(MCGMIL_E_INVALID, "bytes is NULL");
    *bytes = pl.total;
    return MCGMIL_OK;
}

int mcgmil_stem_wgrad_bf16(const mcgmil_stem_grad_bf16_args* a, void* stream) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!a->fwd.x || !a->dy || !a->dw) return fail(MCGMIL_E_INVALID, "NULL x, dy or dw");
    if ((((uintptr_t)a->dy | (uintptr_t)a->dw) & 15u) || ((uintptr_t)a->fwd.x & 3u))
        return fail(MCGMIL_E_ALIGN, "dy and dw must be 16-byte aligned, x 4-byte aligned");
    if (!a->workspace || a->workspace_bytes < pl.total)
        return fail(MCGMIL_E_WORKSPACE, "workspace missing or smaller than mcgmil_stem_wgrad_workspace_size_bf16()");
    if (((uintptr_t)a->workspace & 255u) != 0) return fail(MCGMIL_E_ALIGN, "workspace must be 256-byte aligned");

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t* xd = static_cast<const uint32_t*>(a->fwd.x);
    const __bf16* dy = static_cast<const __bf16*>(a->dy);
    float* sum = static_cast<float*>(a->workspace);
    float* part = sum + pl.E;
    const unsigned rblocks = (unsigned)(pl.E / kRE);        // E = 512 * Cin * k
    for (long long g0 = 0; g0 < pl.gran_total; g0 += pl.gran_chunk) {
        const long long n = pl.gran_total - g0 < pl.gran_chunk ? pl.gran_total - g0 : pl.gran_chunk;
        const long long pix0 = g0 * kGranule;
        if (int rc = pl.nbw == 1   ? launch_wgrad<1>(pl, xd, dy, part, pix0, n, s)
                     : pl.nbw == 2 ? launch_wgrad<2>(pl, xd, dy, part, pix0, n, s)
                     : pl.nbw == 3 ? launch_wgrad<3>(pl, xd, dy, part, pix0, n, s)
                                   : launch_wgrad<4>(pl, xd, dy, part, pix0, n, s))
            return rc;
        hipLaunchKernelGGL(stem_wgrad_bf16_reduce_kernel, dim3(rblocks), dim3(256), 0, s, part, sum, a->dw, pl.E, (int)n,
                           (int)(g0 == 0), (int)(g0 + n == pl.gran_total), pl.g.Cin, pl.g.k, pl.g.P - pl.g.pad);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "stem_wgrad_bf16_reduce_kernel launch");
    }
    return MCGMIL_OK;
}

}  // extern "C"
