// Backward of the fused BatchNorm (+ residual add) (+ ReLU) of the backbone
// (include/mcgmil_bn_grad.h): the gradient of mcgmil_batchnorm_act (mcgmil_bn.hip) in
// batch-statistics mode, fp32. Reference: loss.backward() through relu?(bn(x) [+ residual]) of
// the ResNet blocks (model.py:166-179 under net_utils.train_gacc), where torch runs
// threshold_backward and native_batch_norm_backward.
//
// Channels-last activations are [rows, C] matrices. With xh = (x - mean_c) invstd_c and
// g = dy [y > 0] (dy without ReLU), three launches that mirror the forward's:
//   bn_grad_partial_kernel   each workgroup owns kPartElems / C consecutive rows (a function of
//                            (rows, C) alone): per-thread fp32 sums of g and g xh over its rows,
//                            16-byte loads, one channel group per thread, then an LDS reduction
//                            over the row lanes in lane order -> one [2][C] partial
//   bn_grad_finalize_kernel  fp64 combination of the partials (32 lanes per channel, every 32nd
//                            partial each, then the lanes in order): dbeta, dgamma and
//                            k1 = gamma invstd, k2 = -k1 invstd dgamma / n, k3 = -k1 dbeta / n
//   bn_grad_apply_kernel     dx = k1 g + k2 (x - mean) + k3 and dresidual = g, 16-byte loads and
//                            stores, every element read once and written once
// HBM-bound: x, dy (and y) are read twice, dx (and dresidual) written once. With ReLU and a
// residual the apply pass reads y and dy again rather than a g the partial pass would have
// written to dresidual: the same traffic, and the partial pass stays read-only.
// No floating-point atomics; every sum has one fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <numeric>
#include <string>

#include "../../include/mcgmil.h"
#include "../../include/mcgmil_bn_grad.h"
#include "mcgmil_error.h"

namespace {

using mcgmil_detail::fail;
using mcgmil_detail::hip_fail;

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int kThreads = 256;
constexpr int kMaxC = 2048;           // channel groups of 8 <= threads of a workgroup
constexpr long long kPartElems = MCGMIL_BN_GRAD_PART_ELEMS;
constexpr int kFinCh = 8;             // finalize: channels per workgroup
constexpr int kFinLanes = kThreads / kFinCh;    // finalize: lanes per channel
constexpr long long kMaxElems = 1ll << 46;      // rows * C (64-bit offsets; the grid stays < 2^31)

// The apply pass touches every element exactly once, so it could stream: MCGMIL_BN_GRAD_NT=1 builds
// nontemporal loads and stores there. Plain ones measured faster or equal on the ResNet-18 block
// shapes, whichever of the two builds ran second in the round-robin (layer 1 at 256 instances, whole
// backward: 0.33-0.35 against 0.41-0.44 ms without a residual, 0.31-0.32 against 0.32-0.36 ms with
// one; scripts/bench_norm_grad.py --ab-lib): the partial pass has just read the same
// x, y and dy, and what of them is still in the Infinity Cache serves the plain loads. The partial
// pass reads with plain loads either way.
#ifndef MCGMIL_BN_GRAD_NT
#define MCGMIL_BN_GRAD_NT 0
#endif
#ifndef MCGMIL_BN_GRAD_UNROLL
#define MCGMIL_BN_GRAD_UNROLL 2
#endif
#ifndef MCGMIL_BN_GRAD_MAXBLOCKS
#define MCGMIL_BN_GRAD_MAXBLOCKS 4096
#endif

__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}
__device__ __forceinline__ void load8s(const float* p, float (&v)[8]) {
#if MCGMIL_BN_GRAD_NT
    const f32x4 a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    const f32x4 b = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + 4));
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
#else
    load8(p, v);
#endif
}
__device__ __forceinline__ void store8s(float* p, const float (&v)[8]) {
#if MCGMIL_BN_GRAD_NT
    __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4*>(p));
    __builtin_nontemporal_store(f32x4{v[4], v[5], v[6], v[7]}, reinterpret_cast<f32x4*>(p + 4));
#else
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
#endif
}

// Workgroup b sums rows [b * rpp, (b + 1) * rpp). Thread (rp, cg): channels 8*cg .. 8*cg+7 of
// rows r0 + rp, r0 + rp + RP, ... with RP = 256 / (C / 8) row lanes (threads past RP * C / 8 idle).
template <bool RELU>
__global__ __launch_bounds__(kThreads) void bn_grad_partial_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ y,
                                                                   const float* __restrict__ dy,
                                                                   const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd,
                                                                   long long rows, int C, long long rpp,
                                                                   float* __restrict__ part) {
    __shared__ float red[2][kThreads * 8];
    const int tid = threadIdx.x, CG = C >> 3, RP = kThreads / CG;
    const int cg = tid % CG, rp = tid / CG;
    const long long r0 = (long long)blockIdx.x * rpp;
    const long long r1 = r0 + rpp < rows ? r0 + rpp : rows;
    if (rp < RP) {
        float s[8], sx[8], mu[8], is[8];
        load8(mean + cg * 8, mu);
        load8(invstd + cg * 8, is);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = sx[j] = 0.f;
        auto add = [&](const float (&xv)[8], const float (&yv)[8], const float (&gv)[8]) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float g = RELU ? (yv[j] > 0.f ? gv[j] : 0.f) : gv[j];
                s[j] += g;
                sx[j] = fmaf(g, (xv[j] - mu[j]) * is[j], sx[j]);
            }
        };
        long long r = r0 + rp;
        // two rows in flight per iteration (independent loads); the rows are still added in order
        for (; r + RP < r1; r += 2 * RP) {
            float xa[8], ya[8], ga[8], xb[8], yb[8], gb[8];
            const long long oa = r * C + cg * 8, ob = (r + RP) * C + cg * 8;
            load8(x + oa, xa);
            load8(dy + oa, ga);
            if (RELU) load8(y + oa, ya);
            load8(x + ob, xb);
            load8(dy + ob, gb);
            if (RELU) load8(y + ob, yb);
            add(xa, ya, ga);
            add(xb, yb, gb);
        }
        if (r < r1) {
            float xa[8], ya[8], ga[8];
            const long long oa = r * C + cg * 8;
            load8(x + oa, xa);
            load8(dy + oa, ga);
            if (RELU) load8(y + oa, ya);
            add(xa, ya, ga);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            red[0][rp * C + cg * 8 + j] = s[j];
            red[1][rp * C + cg * 8 + j] = sx[j];
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += kThreads) {
        float S = 0.f, SX = 0.f;
        for (int k = 0; k < RP; ++k) {
            S += red[0][k * C + c];
            SX += red[1][k * C + c];
        }
        part[((size_t)blockIdx.x * 2) * C + c] = S;
        part[((size_t)blockIdx.x * 2 + 1) * C + c] = SX;
    }
}

// One workgroup per 8 channels, 32 lanes per channel each summing every 32nd partial in fp64;
// the 32 lane sums are combined in lane order (deterministic for a given partial count).
// coef: [3][C] k1, k2, k3 of the apply pass.
__global__ __launch_bounds__(kThreads) void bn_grad_finalize_kernel(const float* __restrict__ part, long long parts,
                                                                    long long rows, int C,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ invstd,
                                                                    float* __restrict__ coef, float* dgamma,
                                                                    float* dbeta) {
    __shared__ double red[2][kThreads];
    const int tid = threadIdx.x, lane = tid / kFinCh, cl = tid % kFinCh;
    const int c = blockIdx.x * kFinCh + cl;
    double S = 0.0, SX = 0.0;
    if (c < C) {
        // unrolled so the partial loads are all in flight (same summation order: one chain each)
#pragma unroll 8
        for (long long b = lane; b < parts; b += kFinLanes) {
            S += (double)part[((size_t)b * 2) * C + c];
            SX += (double)part[((size_t)b * 2 + 1) * C + c];
        }
    }
    red[0][tid] = S;
    red[1][tid] = SX;
    __syncthreads();
    if (lane != 0 || c >= C) return;
    S = SX = 0.0;
    for (int k = 0; k < kFinLanes; ++k) {
        S += red[0][k * kFinCh + cl];
        SX += red[1][k * kFinCh + cl];
    }
    if (dbeta) dbeta[c] = (float)S;
    if (dgamma) dgamma[c] = (float)SX;
    const double is = (double)invstd[c], n = (double)rows;
    const double k1 = (gamma ? (double)gamma[c] : 1.0) * is;
    coef[c] = (float)k1;
    coef[C + c] = (float)(-k1 * is * SX / n);
    coef[2 * C + c] = (float)(-k1 * S / n);
}

// Grid-stride over 8-channel vectors; the total thread count is a multiple of C/8, so every
// thread keeps one channel group. U vectors in flight per iteration.
template <bool RELU, bool DX, bool DRES>
__global__ __launch_bounds__(kThreads) void bn_grad_apply_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ y,
                                                                 const float* __restrict__ dy,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ coef,
                                                                 float* __restrict__ dx, float* __restrict__ dres,
                                                                 long long nvec, int C) {
    static_assert(DX || DRES, "nothing to write");
    static_assert(RELU || !DRES, "without ReLU the residual gradient is dy itself");
    const int CG = C >> 3;
    const long long stride = (long long)gridDim.x * kThreads;
    const long long i0 = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int cg = (int)(i0 % CG);
    float k1[8], k2[8], k3[8], mu[8];
    if (DX) {
        load8(coef + cg * 8, k1);
        load8(coef + C + cg * 8, k2);
        load8(coef + 2 * C + cg * 8, k3);
        load8(mean + cg * 8, mu);
    }
    auto one = [&](long long i, const float (&xv)[8], const float (&yv)[8], const float (&gv)[8]) {
        float g[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = RELU ? (yv[j] > 0.f ? gv[j] : 0.f) : gv[j];
        if (DRES) store8s(dres + i * 8, g);
        if (DX) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = fmaf(k1[j], g[j], fmaf(k2[j], xv[j] - mu[j], k3[j]));
            store8s(dx + i * 8, o);
        }
    };
    long long i = i0;
    constexpr int U = MCGMIL_BN_GRAD_UNROLL;
    for (; i + (U - 1) * stride < nvec; i += U * stride) {
        float xv[U][8], yv[U][8], gv[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long o = (i + u * stride) * 8;
            if (DX) load8s(x + o, xv[u]);
            if (RELU) load8s(y + o, yv[u]);
            load8s(dy + o, gv[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) one(i + u * stride, xv[u], yv[u], gv[u]);
    }
    for (; i < nvec; i += stride) {
        float xv[8], yv[8], gv[8];
        if (DX) load8s(x + i * 8, xv);
        if (RELU) load8s(y + i * 8, yv);
        load8s(dy + i * 8, gv);
        one(i, xv, yv, gv);
    }
}

struct Plan {
    long long rpp, parts;
    size_t total;       // workspace bytes
};

// rows, channels and reserved only (what the workspace size depends on)
int plan_for(const mcgmil_bn_grad_args* a, Plan& pl) {
    if (!a) return fail(MCGMIL_E_INVALID, "mcgmil_bn_grad_args is NULL");
    if (a->reserved != 0) return fail(MCGMIL_E_INVALID, "reserved must be 0");
    if (a->channels < 8 || a->channels % 8 || a->channels > kMaxC)
        return fail(MCGMIL_E_UNSUPPORTED, "channels must be a multiple of 8 in [8, 2048], got " +
                                              std::to_string(a->channels));
    if (a->rows < 2) return fail(MCGMIL_E_INVALID, "rows must be >= 2 (batch statistics of one value have no gradient)");
    long long elems = 0;
    if (__builtin_mul_overflow((long long)a->rows, (long long)a->channels, &elems) || elems >= kMaxElems)
        return fail(MCGMIL_E_UNSUPPORTED, "rows * channels must be < 2^46");
    const long long C = a->channels;
    pl.rpp = kPartElems / C;                                   // >= 16
    pl.parts = (a->rows + pl.rpp - 1) / pl.rpp;                // < 2^31: elems < 2^46, rpp * C > 2^14
    pl.total = (size_t)(((4 * C + 2 * C * pl.parts) * (long long)sizeof(float) + 255) & ~255ll);
    return MCGMIL_OK;
}

template <bool RELU, bool DX, bool DRES>
void launch_apply(const mcgmil_bn_grad_args* a, const float* coef, hipStream_t s) {
    const int CG = a->channels / 8;
    const long long nvec = a->rows * CG;
    // blocks: a multiple of CG / gcd(CG, 256) so that every thread keeps its channel group
    const int unit = CG / std::gcd(CG, kThreads);
    long long want = (nvec + 2LL * kThreads - 1) / (2LL * kThreads);
    if (want > MCGMIL_BN_GRAD_MAXBLOCKS) want = MCGMIL_BN_GRAD_MAXBLOCKS;
    const long long blocks = (want + unit - 1) / unit * unit;
    hipLaunchKernelGGL((bn_grad_apply_kernel<RELU, DX, DRES>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a->x,
                       a->y, a->dy, a->mean, coef, a->dx, a->dresidual, nvec, a->channels);
}

}  // namespace

namespace mcgmil_detail {

// bn_grad_finalize_kernel for another backward with the same [parts][2][C] partials and [3][C]
// coefficients (mcgmil_pool_grad.hip); the caller checks hipGetLastError().
void bn_grad_finalize(const float* part, long long parts, long long rows, int C, const float* gamma,
                      const float* invstd, float* coef, float* dgamma, float* dbeta, hipStream_t s) {
    hipLaunchKernelGGL(bn_grad_finalize_kernel, dim3((C + kFinCh - 1) / kFinCh), dim3(kThreads), 0, s, part, parts,
                       rows, C, gamma, invstd, coef, dgamma, dbeta);
}

}  // namespace mcgmil_detail

extern "C" {

size_t mcgmil_bn_grad_args_size(void) { return sizeof(mcgmil_bn_grad_args); }

int mcgmil_bn_grad_workspace_size(const mcgmil_bn_grad_args* a, size_t* bytes) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (!bytes) return fail(MCGMIL_E_INVALID, "bytes is NULL");
    *bytes = pl.total;
    return MCGMIL_OK;
}

int mcgmil_batchnorm_act_backward(const mcgmil_bn_grad_args* a, void* stream) {
    Plan pl;
    if (int rc = plan_for(a, pl)) return rc;
    if (a->relu != 0 && a->relu != 1) return fail(MCGMIL_E_INVALID, "relu must be 0 or 1");
    if (!a->x || !a->dy || !a->mean || !a->invstd) return fail(MCGMIL_E_INVALID, "x, dy, mean and invstd are required");
    if (a->relu && !a->y) return fail(MCGMIL_E_INVALID, "relu needs y (the forward's output)");
    if (!a->dx && !a->dresidual && !a->dgamma && !a->dbeta)
        return fail(MCGMIL_E_INVALID, "no output requested (dx, dresidual, dgamma and dbeta are all NULL)");
    if (a->dresidual && !a->relu)
        return fail(MCGMIL_E_INVALID, "dresidual needs relu (without ReLU the residual's gradient is dy itself)");
    if (((uintptr_t)a->x | (uintptr_t)a->y | (uintptr_t)a->dy | (uintptr_t)a->dx | (uintptr_t)a->dresidual |
         (uintptr_t)a->mean | (uintptr_t)a->invstd) & 15u)
        return fail(MCGMIL_E_ALIGN, "x, y, dy, dx, dresidual, mean and invstd must be 16-byte aligned");
    if (((uintptr_t)a->gamma | (uintptr_t)a->dgamma | (uintptr_t)a->dbeta) & 3u)
        return fail(MCGMIL_E_ALIGN, "gamma, dgamma and dbeta must be 4-byte aligned");
    if (!a->workspace || a->workspace_bytes < pl.total)
        return fail(MCGMIL_E_WORKSPACE, "workspace missing or smaller than mcgmil_bn_grad_workspace_size()");
    if (((uintptr_t)a->workspace & 255u) != 0) return fail(MCGMIL_E_ALIGN, "workspace must be 256-byte aligned");

    hipStream_t s = static_cast<hipStream_t>(stream);
    const int C = a->channels;
    float* coef = static_cast<float*>(a->workspace);    // [3][C] (+ C of padding)
    float* part = coef + 4 * C;                         // [parts][2][C]
    if (a->dx || a->dgamma || a->dbeta) {
        auto k = a->relu ? bn_grad_partial_kernel<true> : bn_grad_partial_kernel<false>;
        hipLaunchKernelGGL(k, dim3((unsigned)pl.parts), dim3(kThreads), 0, s, a->x, a->y, a->dy, a->mean, a->invstd,
                           (long long)a->rows, C, pl.rpp, part);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "bn_grad_partial_kernel launch");
        hipLaunchKernelGGL(bn_grad_finalize_kernel, dim3((C + kFinCh - 1) / kFinCh), dim3(kThreads), 0, s, part,
                           pl.parts, (long long)a->rows, C, a->gamma, a->invstd, coef, a->dgamma, a->dbeta);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "bn_grad_finalize_kernel launch");
    }
    if (a->dx || a->dresidual) {
        if (a->relu) {
            if (a->dx && a->dresidual) launch_apply<true, true, true>(a, coef, s);
            else if (a->dx) launch_apply<true, true, false>(a, coef, s);
            else launch_apply<true, false, true>(a, coef, s);
        } else {
            launch_apply<false, true, false>(a, coef, s);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "bn_grad_apply_kernel launch");
    }
    return MCGMIL_OK;
}

}  // extern "C"
