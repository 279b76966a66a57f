// The partial and apply kernels of the fused BatchNorm (+ residual add) (+ ReLU) backward, templated
// on the element type of x, y, dy, dx and dresidual, with the validation and launch sequence both
// entry points share: mcgmil_bn_grad.hip instantiates them for float (include/mcgmil_bn_grad.h),
// mcgmil_bn_grad_bf16.hip for __bf16 (include/mcgmil_bn_grad_bf16.h). Everything per channel (mean,
// invstd, gamma, the partials, the coefficients, dgamma, dbeta) is fp32 in both.
//
// A thread owns 8 consecutive channels of a row in either type (two 16-byte loads of fp32, one of
// bf16), so the thread-to-element map, the row partition and with them the order of every sum are
// the same: on inputs that are bf16 values, the bf16 instantiation's dgamma and dbeta are bitwise
// the fp32 one's and its dx is the fp32 dx rounded once, to nearest even, at the store.
// bf16 is widened to fp32 exactly (a 16-bit shift); dresidual = g is a widened bf16 value or +0,
// which the store's conversion gives back bit for bit.
#ifndef MCGMIL_BN_GRAD_KERNELS_H_
#define MCGMIL_BN_GRAD_KERNELS_H_

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
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

constexpr int kThreads = 256;
constexpr int kMaxC = 2048;           // channel groups of 8 <= threads of a workgroup
constexpr long long kPartElems = MCGMIL_BN_GRAD_PART_ELEMS;
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
[[maybe_unused]] __device__ __forceinline__ void widen8(const u32x4 u, float (&v)[8]) {
    v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xFFFF0000u);
    v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xFFFF0000u);
    v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xFFFF0000u);
    v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xFFFF0000u);
}
[[maybe_unused]] __device__ __forceinline__ void load8(const __bf16* p, float (&v)[8]) {
    widen8(*reinterpret_cast<const u32x4*>(p), v);
}
[[maybe_unused]] __device__ __forceinline__ void load8s(const float* p, float (&v)[8]) {
#if MCGMIL_BN_GRAD_NT
    const f32x4 a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    const f32x4 b = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + 4));
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
#else
    load8(p, v);
#endif
}
[[maybe_unused]] __device__ __forceinline__ void load8s(const __bf16* p, float (&v)[8]) {
#if MCGMIL_BN_GRAD_NT
    widen8(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)), v);
#else
    load8(p, v);
#endif
}
[[maybe_unused]] __device__ __forceinline__ void store8s(float* p, const float (&v)[8]) {
#if MCGMIL_BN_GRAD_NT
    __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4*>(p));
    __builtin_nontemporal_store(f32x4{v[4], v[5], v[6], v[7]}, reinterpret_cast<f32x4*>(p + 4));
#else
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
#endif
}
[[maybe_unused]] __device__ __forceinline__ void store8s(__bf16* p, const float (&v)[8]) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (__bf16)v[j];             // round to nearest even
#if MCGMIL_BN_GRAD_NT
    __builtin_nontemporal_store(__builtin_bit_cast(u32x4, o), reinterpret_cast<u32x4*>(p));
#else
    *reinterpret_cast<bf16x8*>(p) = o;
#endif
}

// Workgroup b sums rows [b * rpp, (b + 1) * rpp). Thread (rp, cg): channels 8*cg .. 8*cg+7 of
// rows r0 + rp, r0 + rp + RP, ... with RP = 256 / (C / 8) row lanes (threads past RP * C / 8 idle).
template <typename T, bool RELU>
__global__ __launch_bounds__(kThreads) void bn_grad_partial_kernel(const T* __restrict__ x,
                                                                   const T* __restrict__ y,
                                                                   const T* __restrict__ dy,
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

// Grid-stride over 8-channel vectors; the total thread count is a multiple of C/8, so every
// thread keeps one channel group. U vectors in flight per iteration.
template <typename T, bool RELU, bool DX, bool DRES>
__global__ __launch_bounds__(kThreads) void bn_grad_apply_kernel(const T* __restrict__ x,
                                                                 const T* __restrict__ y,
                                                                 const T* __restrict__ dy,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ coef,
                                                                 T* __restrict__ dx, T* __restrict__ dres,
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

// rows, channels and reserved only (what the workspace size depends on). Args is mcgmil_bn_grad_args
// or mcgmil_bn_grad_bf16_args (the same fields; the element pointers differ in type).
template <typename Args>
int plan_for(const Args* a, Plan& pl, const char* args_name) {
    if (!a) return fail(MCGMIL_E_INVALID, std::string(args_name) + " is NULL");
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

template <typename T, bool RELU, bool DX, bool DRES, typename Args>
void launch_apply(const Args* a, const float* coef, hipStream_t s) {
    const int CG = a->channels / 8;
    const long long nvec = a->rows * CG;
    // blocks: a multiple of CG / gcd(CG, 256) so that every thread keeps its channel group
    const int unit = CG / std::gcd(CG, kThreads);
    long long want = (nvec + 2LL * kThreads - 1) / (2LL * kThreads);
    if (want > MCGMIL_BN_GRAD_MAXBLOCKS) want = MCGMIL_BN_GRAD_MAXBLOCKS;
    const long long blocks = (want + unit - 1) / unit * unit;
    hipLaunchKernelGGL((bn_grad_apply_kernel<T, RELU, DX, DRES>), dim3((unsigned)blocks), dim3(kThreads), 0, s,
                       static_cast<const T*>(a->x), static_cast<const T*>(a->y), static_cast<const T*>(a->dy), a->mean,
                       coef, static_cast<T*>(a->dx), static_cast<T*>(a->dresidual), nvec, a->channels);
}

// Every check before any launch, then the three launches. finalize(part, parts, rows, C, gamma,
// invstd, coef, dgamma, dbeta, stream) launches the fp64 combination of the partials.
template <typename T, typename Args, typename Finalize>
int backward(const Args* a, void* stream, const char* args_name, const char* size_name, Finalize finalize) {
    Plan pl;
    if (int rc = plan_for(a, pl, args_name)) return rc;
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
        return fail(MCGMIL_E_WORKSPACE, std::string("workspace missing or smaller than ") + size_name + "()");
    if (((uintptr_t)a->workspace & 255u) != 0) return fail(MCGMIL_E_ALIGN, "workspace must be 256-byte aligned");

    hipStream_t s = static_cast<hipStream_t>(stream);
    const int C = a->channels;
    float* coef = static_cast<float*>(a->workspace);    // [3][C] (+ C of padding)
    float* part = coef + 4 * C;                         // [parts][2][C]
    if (a->dx || a->dgamma || a->dbeta) {
        auto k = a->relu ? bn_grad_partial_kernel<T, true> : bn_grad_partial_kernel<T, false>;
        hipLaunchKernelGGL(k, dim3((unsigned)pl.parts), dim3(kThreads), 0, s, static_cast<const T*>(a->x),
                           static_cast<const T*>(a->y), static_cast<const T*>(a->dy), a->mean, a->invstd,
                           (long long)a->rows, C, pl.rpp, part);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "bn_grad_partial_kernel launch");
        finalize(part, pl.parts, (long long)a->rows, C, a->gamma, a->invstd, coef, a->dgamma, a->dbeta, s);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "bn_grad_finalize_kernel launch");
    }
    if (a->dx || a->dresidual) {
        if (a->relu) {
            if (a->dx && a->dresidual) launch_apply<T, true, true, true>(a, coef, s);
            else if (a->dx) launch_apply<T, true, true, false>(a, coef, s);
            else launch_apply<T, true, false, true>(a, coef, s);
        } else {
            launch_apply<T, false, true, false>(a, coef, s);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "bn_grad_apply_kernel launch");
    }
    return MCGMIL_OK;
}

}  // namespace

#endif /* MCGMIL_BN_GRAD_KERNELS_H_ */
