// The kernels of the stem's fused BatchNorm (+ ReLU) + max-pool training op, templated on the
// element type of z, y, dy and dz, with the plan, the validation and the launch sequences both
// precisions share: mcgmil_pool_grad.hip instantiates them for float (include/mcgmil_pool_grad.h),
// mcgmil_pool_grad_bf16.hip for __bf16 (include/mcgmil_pool_grad_bf16.h). Everything per channel
// (a, b, mean, invstd, gamma, the partials, the coefficients, dgamma, dbeta) is fp32 in both, and
// so are the argmax codes' rule and every sum and product.
//
// A thread owns 8 consecutive channels of a pixel in either type (two 16-byte loads of fp32, one
// of bf16), so the thread-to-element map, the partition and with them the order of every sum are
// the same: on inputs that are bf16 values, the bf16 instantiation's codes, dgamma and dbeta are
// bitwise the fp32 one's, its y is the fp32 y and its dz the fp32 dz, each rounded once, to nearest
// even, at the store. bf16 is widened to fp32 exactly (a 16-bit shift).
//
// Forward: the statistics and finalize launches of mcgmil_batchnorm_act (through
// mcgmil_batchnorm_coefficients, (a_c, b_c) at the workspace start), then
//   bn_pool_argmax_kernel    bn_pool_kernel of mcgmil_bn.hip (same fmaxf chain: same bits) that
//                            also keeps kh * k + kw of the first strict maximum and stores the
//                            8 codes of a (pooled pixel, 8-channel group) as one 8-byte word
// Backward, channels-last z as a [rows = N H W, C] matrix, g gathered per input pixel from dy and
// the codes of its <= 4 covering windows (<= 9 at stride 1), three launches as mcgmil_bn_grad.hip:
//   bn_pool_grad_kernel<false>  each workgroup owns kPartElems / C consecutive input pixels (a
//                               function of (rows, C) alone): per-thread fp32 sums of g and g xh,
//                               then an LDS reduction over the row lanes in lane order
//   bn_grad_finalize_kernel     (mcgmil_bn_grad.hip) fp64 combination of the partials: dbeta,
//                               dgamma, k1 = gamma invstd, k2 = -k1 invstd dgamma / n, k3 = -k1 dbeta / n
//   bn_pool_grad_kernel<true>   the same walk: dz = k1 g + k2 (z - mean) + k3, g gathered again
// HBM-bound: z is read twice and dz written once; dy and the codes (1/4 and, in fp32, 1/16 of z's
// bytes at the stem's 3/2/1 pool; in bf16 the codes are 1/8) are read about 2.25 times per pass,
// mostly from L2 (neighbouring pixels share windows). No floating-point atomics; every sum has one
// fixed order. 64-bit offsets.
#ifndef MCGMIL_POOL_GRAD_KERNELS_H_
#define MCGMIL_POOL_GRAD_KERNELS_H_

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <numeric>
#include <string>
#include <type_traits>

#include "../../include/mcgmil.h"
#include "../../include/mcgmil_pool_grad.h"
#include "mcgmil_error.h"

namespace {

using mcgmil_detail::fail;
using mcgmil_detail::hip_fail;

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

constexpr int kThreads = 256;
constexpr int kMaxC = 2048;           // channel groups of 8 <= threads of a workgroup
constexpr long long kPartElems = MCGMIL_BN_POOL_GRAD_PART_ELEMS;
constexpr long long kMaxElems = 1ll << 46;      // rows * C (64-bit offsets; the grid stays < 2^31)
constexpr unsigned kNone = MCGMIL_POOL_ARGMAX_NONE;

struct Geo {
    int H, W, PH, PW, k, st, pd;
};

__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}
[[maybe_unused]] __device__ __forceinline__ void load8(const __bf16* p, float (&v)[8]) {
    const u32x4 u = *reinterpret_cast<const u32x4*>(p);
    v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xFFFF0000u);
    v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xFFFF0000u);
    v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xFFFF0000u);
    v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xFFFF0000u);
}
[[maybe_unused]] __device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
}
[[maybe_unused]] __device__ __forceinline__ void store8(__bf16* p, const float (&v)[8]) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (__bf16)v[j];             // round to nearest even
    *reinterpret_cast<bf16x8*>(p) = o;
}

// bn_pool_kernel<E, RELU> of mcgmil_bn.hip, thread per (pooled pixel, 8-channel group), plus the
// argmax code: the tap index kh * k + kw is kept where the tap is strictly greater than the
// running maximum (the first maximum wins); the maximum itself goes through the same fmaxf chain.
// Both are taken on the unrounded fp32 value fmaf(z, a, b); y is rounded at the store alone.
template <typename T, bool RELU>
__global__ __launch_bounds__(kThreads) void bn_pool_argmax_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                                  uint8_t* __restrict__ argmax, Geo q,
                                                                  long long nvec, int C,
                                                                  const float* __restrict__ ab) {
    const int CG = C >> 3;
    const long long stride = (long long)gridDim.x * kThreads;
    const long long i0 = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int cg = (int)(i0 % CG);
    float a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        a[j] = ab[cg * 8 + j];
        b[j] = ab[C + cg * 8 + j];
    }
    for (long long i = i0; i < nvec; i += stride) {
        const long long pix = i / CG;
        const int ow = (int)(pix % q.PW);
        const long long t = pix / q.PW;
        const int oh = (int)(t % q.PH);
        const long long n = t / q.PH;
        float m[8];
        unsigned code[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            m[j] = -INFINITY;
            code[j] = kNone;
        }
        const int h0 = oh * q.st - q.pd, w0 = ow * q.st - q.pd;
        for (int kh = 0; kh < q.k; ++kh) {
            const int ih = h0 + kh;
            if (ih < 0 || ih >= q.H) continue;
            const T* row = x + ((n * q.H + ih) * (long long)q.W) * C + cg * 8;
            for (int kw = 0; kw < q.k; ++kw) {
                const int iw = w0 + kw;
                if (iw < 0 || iw >= q.W) continue;
                float v[8];
                load8(row + (long long)iw * C, v);
                const unsigned tap = (unsigned)(kh * q.k + kw);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float t = fmaf(v[j], a[j], b[j]);
                    code[j] = t > m[j] ? tap : code[j];
                    m[j] = fmaxf(m[j], t);
                }
            }
        }
        if (RELU) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                code[j] = m[j] <= 0.f ? kNone : code[j];
                m[j] = fmaxf(m[j], 0.f);
            }
        }
        store8(y + i * 8, m);
        uint2 c;
        c.x = code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24);
        c.y = code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24);
        *reinterpret_cast<uint2*>(argmax + i * 8) = c;
    }
}

// g of input pixel (n, h, w), channels 8 cg .. 8 cg + 7: dy of the pooled outputs whose window
// contains the pixel and whose code names it, added in ascending (ph, pw) order.
template <typename T>
__device__ __forceinline__ void gather(const T* __restrict__ dy, const uint8_t* __restrict__ argmax,
                                       long long n, int h, int w, const Geo& q, int C, int cg, float (&g)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = 0.f;
    const int th = h + q.pd - q.k + 1, tw = w + q.pd - q.k + 1;
    const int ph0 = th <= 0 ? 0 : (int)((unsigned)(th + q.st - 1) / (unsigned)q.st);
    const int pw0 = tw <= 0 ? 0 : (int)((unsigned)(tw + q.st - 1) / (unsigned)q.st);
    int ph1 = (int)((unsigned)(h + q.pd) / (unsigned)q.st), pw1 = (int)((unsigned)(w + q.pd) / (unsigned)q.st);
    ph1 = ph1 < q.PH - 1 ? ph1 : q.PH - 1;
    pw1 = pw1 < q.PW - 1 ? pw1 : q.PW - 1;
    for (int ph = ph0; ph <= ph1; ++ph) {
        const int ch = (h - ph * q.st + q.pd) * q.k;
        const long long prow = (n * q.PH + ph) * (long long)q.PW;
        for (int pw = pw0; pw <= pw1; ++pw) {
            const unsigned want = (unsigned)(ch + (w - pw * q.st + q.pd));
            const long long o = (prow + pw) * C + cg * 8;
            const uint2 c = *reinterpret_cast<const uint2*>(argmax + o);
            float d[8];
            load8(dy + o, d);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned code = ((j < 4 ? c.x : c.y) >> (8 * (j & 3))) & 0xFFu;
                g[j] += code == want ? d[j] : 0.f;
            }
        }
    }
}

// Workgroup b owns input pixels (rows) [b * rpp, (b + 1) * rpp). Thread (rp, cg): channels
// 8*cg .. 8*cg+7 of rows r0 + rp, r0 + rp + RP, ... with RP = 256 / (C / 8) row lanes (threads past
// RP * C / 8 idle).
//   APPLY == false: aux = invstd; out = part (fp32), this workgroup's [2][C] sums of g and g xh
//   APPLY == true:  aux = coef [3][C] (k1, k2, k3); out = dz (T) = k1 g + k2 (z - mean) + k3
template <typename T, bool APPLY>
__global__ __launch_bounds__(kThreads) void bn_pool_grad_kernel(const T* __restrict__ z,
                                                                const uint8_t* __restrict__ argmax,
                                                                const T* __restrict__ dy,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ aux, Geo q,
                                                                long long rows, int C, long long rpp,
                                                                std::conditional_t<APPLY, T, float>* __restrict__ out) {
    const int tid = threadIdx.x, CG = C >> 3, RP = kThreads / CG;
    const int cg = tid % CG, rp = tid / CG;
    const long long r0 = (long long)blockIdx.x * rpp;
    const long long r1 = r0 + rpp < rows ? r0 + rpp : rows;
    const unsigned HW = (unsigned)q.H * (unsigned)q.W;      // < 2^31 (plan_for)
    float s[8], sx[8], mu[8], k1[8], k2[8], k3[8];
    if (rp < RP) {
        load8(mean + cg * 8, mu);
        load8(aux + cg * 8, k1);                            // invstd without APPLY
        if (APPLY) {
            load8(aux + C + cg * 8, k2);
            load8(aux + 2 * C + cg * 8, k3);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = sx[j] = 0.f;
        long long r = r0 + rp;
        long long n = r / HW;
        unsigned pq = (unsigned)(r - n * HW);               // pixel within the image
        for (; r < r1; r += RP) {
            const int h = (int)(pq / (unsigned)q.W), w = (int)(pq % (unsigned)q.W);
            float g[8], zv[8];
            const long long o = r * C + cg * 8;
            load8(z + o, zv);
            gather(dy, argmax, n, h, w, q, C, cg, g);
            if constexpr (APPLY) {
                float d[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) d[j] = fmaf(k1[j], g[j], fmaf(k2[j], zv[j] - mu[j], k3[j]));
                store8(out + o, d);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    s[j] += g[j];
                    sx[j] = fmaf(g[j], (zv[j] - mu[j]) * k1[j], sx[j]);
                }
            }
            pq += (unsigned)RP;
            if (pq >= HW) {
                n += pq / HW;
                pq %= HW;
            }
        }
    }
    if constexpr (!APPLY) {
        __shared__ float red[2][kThreads * 8];
        if (rp < RP) {
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
            out[((size_t)blockIdx.x * 2) * C + c] = S;
            out[((size_t)blockIdx.x * 2 + 1) * C + c] = SX;
        }
    }
}

// k in {2, 3}, 1 <= stride <= k, 0 <= pad <= k / 2
bool pool_supported(int k, int st, int pd) { return (k == 2 || k == 3) && st >= 1 && st <= k && pd >= 0 && 2 * pd <= k; }

// in 64 bits: size + 2 pd can pass 2^31 for a size near INT32_MAX
long long pooled_dim(int size, int k, int st, int pd) { return ((long long)size + 2 * pd - k) / st + 1; }

int unsupported_pool(int k, int st, int pd) {
    return fail(MCGMIL_E_UNSUPPORTED, "pooling needs kernel 2 or 3, 1 <= stride <= kernel and 0 <= pad <= kernel / 2, got " +
                                          std::to_string(k) + " / " + std::to_string(st) + " / " + std::to_string(pd));
}

struct Plan {
    long long rows, rpp, parts;
    Geo q;
    size_t total;       // workspace bytes
};

// the integer fields only (what the workspace size depends on). Args is mcgmil_bn_pool_grad_args
// or mcgmil_bn_pool_grad_bf16_args (the same fields; the element pointers differ in type).
template <typename Args>
int plan_for(const Args* a, Plan& pl, const char* args_name) {
    if (!a) return fail(MCGMIL_E_INVALID, std::string(args_name) + " is NULL");
    if (a->reserved != 0 || a->reserved32 != 0) return fail(MCGMIL_E_INVALID, "reserved and reserved32 must be 0");
    if (a->channels < 8 || a->channels % 8 || a->channels > kMaxC)
        return fail(MCGMIL_E_UNSUPPORTED, "channels must be a multiple of 8 in [8, 2048], got " +
                                              std::to_string(a->channels));
    if (a->batch < 1 || a->height < 1 || a->width < 1) return fail(MCGMIL_E_INVALID, "batch, height and width must be >= 1");
    if ((long long)a->height * a->width >= (1ll << 31))
        return fail(MCGMIL_E_UNSUPPORTED, "height * width must be < 2^31");
    pl.rows = (long long)a->batch * a->height * a->width;    // < 2^62
    if (pl.rows < 2) return fail(MCGMIL_E_INVALID, "batch * height * width must be >= 2 (batch statistics of one value have no gradient)");
    if (pl.rows >= kMaxElems / a->channels) return fail(MCGMIL_E_UNSUPPORTED, "batch * height * width * channels must be < 2^46");
    if (!pool_supported(a->pool_kernel, a->pool_stride, a->pool_pad))
        return unsupported_pool(a->pool_kernel, a->pool_stride, a->pool_pad);
    const long long PH = pooled_dim(a->height, a->pool_kernel, a->pool_stride, a->pool_pad);
    const long long PW = pooled_dim(a->width, a->pool_kernel, a->pool_stride, a->pool_pad);
    if (PH < 1 || PW < 1) return fail(MCGMIL_E_INVALID, "pooling window larger than the padded input");
    if (a->pooled_height != PH || a->pooled_width != PW)
        return fail(MCGMIL_E_INVALID, "pooled_height / pooled_width must be " + std::to_string(PH) + " / " +
                                          std::to_string(PW) + " for this input and pool, got " +
                                          std::to_string(a->pooled_height) + " / " + std::to_string(a->pooled_width));
    pl.q = Geo{a->height, a->width, (int)PH, (int)PW, a->pool_kernel, a->pool_stride, a->pool_pad};
    const long long C = a->channels;
    pl.rpp = kPartElems / C;                                   // >= 16
    pl.parts = (pl.rows + pl.rpp - 1) / pl.rpp;                // < 2^31: rows * C < 2^46, rpp * C > 2^14
    pl.total = (size_t)(((4 * C + 2 * C * pl.parts) * (long long)sizeof(float) + 255) & ~255ll);
    return MCGMIL_OK;
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}

// pool(relu?(bn(z))) with the argmax codes, for a->dtype == want_dtype (T its element type). Every
// check before any launch (mcgmil_batchnorm_coefficients validates the statistics' side first).
template <typename T>
int pool_train(const mcgmil_bn_args* a, uint8_t* argmax, void* stream, int want_dtype, const char* wrong_dtype) {
    if (!a) return fail(MCGMIL_E_INVALID, "mcgmil_bn_args is NULL");
    if (a->dtype != want_dtype) return fail(MCGMIL_E_UNSUPPORTED, wrong_dtype);
    if (a->channels < 8 || a->channels % 8 || a->channels > kMaxC)
        return fail(MCGMIL_E_UNSUPPORTED, "channels must be a multiple of 8 in [8, 2048], got " +
                                              std::to_string(a->channels));
    if (!pool_supported(a->pool_kernel, a->pool_stride, a->pool_pad))
        return unsupported_pool(a->pool_kernel, a->pool_stride, a->pool_pad);
    if (a->rows < 2) return fail(MCGMIL_E_INVALID, "rows must be >= 2 (batch statistics of one value have no gradient)");
    if (a->batch < 1 || a->height < 1 || a->width < 1 || (long long)a->batch * a->height * a->width != a->rows)
        return fail(MCGMIL_E_INVALID, "pooling needs batch * height * width == rows");
    if (a->rows >= kMaxElems / a->channels) return fail(MCGMIL_E_UNSUPPORTED, "rows * channels must be < 2^46");
    if (a->running_mean || a->running_var || a->partials || a->num_partials)
        return fail(MCGMIL_E_INVALID, "the statistics are the batch's own, from a pass over x (no running statistics, no partials)");
    if (a->residual || a->residual_ab) return fail(MCGMIL_E_UNSUPPORTED, "no residual add with pooling");
    if (a->relu != 0 && a->relu != 1) return fail(MCGMIL_E_INVALID, "relu must be 0 or 1");
    if (!a->x || !a->y || !argmax || !a->batch_mean || !a->batch_invstd)
        return fail(MCGMIL_E_INVALID, "x, y, argmax, batch_mean and batch_invstd are required");
    if (((uintptr_t)a->x | (uintptr_t)a->y) & 15u) return fail(MCGMIL_E_ALIGN, "x and y must be 16-byte aligned");
    if ((uintptr_t)argmax & 7u) return fail(MCGMIL_E_ALIGN, "argmax must be 8-byte aligned");
    const long long PH = pooled_dim(a->height, a->pool_kernel, a->pool_stride, a->pool_pad);
    const long long PW = pooled_dim(a->width, a->pool_kernel, a->pool_stride, a->pool_pad);
    if (PH < 1 || PW < 1) return fail(MCGMIL_E_INVALID, "pooling window larger than the padded input");
    if (PH > INT32_MAX || PW > INT32_MAX) return fail(MCGMIL_E_UNSUPPORTED, "the pooled height and width must be < 2^31");
    const Geo q{a->height, a->width, (int)PH, (int)PW, a->pool_kernel, a->pool_stride, a->pool_pad};
    const size_t zb = (size_t)a->rows * a->channels * sizeof(T);
    const size_t codes = (size_t)a->batch * q.PH * q.PW * a->channels;
    if (overlaps(a->y, codes * sizeof(T), a->x, zb) || overlaps(argmax, codes, a->x, zb) ||
        overlaps(argmax, codes, a->y, codes * sizeof(T)))
        return fail(MCGMIL_E_INVALID, "x, y and argmax must not overlap");
    if (!a->workspace) return fail(MCGMIL_E_WORKSPACE, "workspace missing (mcgmil_bn_workspace_size())");
    // the statistics pass and the finalize of mcgmil_batchnorm_act: (a_c, b_c) at the workspace
    // start, the partial sums behind them; it validates the rest (and the workspace's size)
    float* ab = static_cast<float*>(a->workspace);
    if (int rc = mcgmil_batchnorm_coefficients(a, ab, stream)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int C = a->channels;
    const long long nvec = (long long)a->batch * q.PH * q.PW * (C / 8);
    const int unit = (C / 8) / std::gcd(C / 8, kThreads);       // every thread keeps its channel group
    long long want = (nvec + kThreads - 1) / kThreads;
    if (want > 8192) want = 8192;
    const long long blocks = (want + unit - 1) / unit * unit;
    auto k = a->relu ? bn_pool_argmax_kernel<T, true> : bn_pool_argmax_kernel<T, false>;
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kThreads), 0, s, static_cast<const T*>(a->x),
                       static_cast<T*>(a->y), argmax, q, nvec, C, ab);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCGMIL_OK : hip_fail(e, "bn_pool_argmax_kernel launch");
}

// Every check before any launch, then the three launches. finalize(part, parts, rows, C, gamma,
// invstd, coef, dgamma, dbeta, stream) launches the fp64 combination of the partials.
template <typename T, typename Args, typename Finalize>
int pool_backward(const Args* a, void* stream, const char* args_name, const char* size_name, Finalize finalize) {
    Plan pl;
    if (int rc = plan_for(a, pl, args_name)) return rc;
    if (!a->z || !a->argmax || !a->dy || !a->mean || !a->invstd)
        return fail(MCGMIL_E_INVALID, "z, argmax, dy, mean and invstd are required");
    if (!a->dz && !a->dgamma && !a->dbeta)
        return fail(MCGMIL_E_INVALID, "no output requested (dz, dgamma and dbeta are all NULL)");
    if (((uintptr_t)a->z | (uintptr_t)a->dy | (uintptr_t)a->dz | (uintptr_t)a->mean | (uintptr_t)a->invstd) & 15u)
        return fail(MCGMIL_E_ALIGN, "z, dy, dz, mean and invstd must be 16-byte aligned");
    if ((uintptr_t)a->argmax & 7u) return fail(MCGMIL_E_ALIGN, "argmax must be 8-byte aligned");
    if (((uintptr_t)a->gamma | (uintptr_t)a->dgamma | (uintptr_t)a->dbeta) & 3u)
        return fail(MCGMIL_E_ALIGN, "gamma, dgamma and dbeta must be 4-byte aligned");
    const size_t C = (size_t)a->channels, cb = C * sizeof(float);
    const size_t zb = (size_t)pl.rows * C * sizeof(T);
    const size_t codes = (size_t)a->batch * pl.q.PH * pl.q.PW * C;
    const struct { const void* p; size_t n; } in[] = {{a->z, zb}, {a->argmax, codes}, {a->dy, codes * sizeof(T)},
                                                      {a->gamma, cb}, {a->mean, cb}, {a->invstd, cb}},
                                               out[] = {{a->dz, zb}, {a->dgamma, cb}, {a->dbeta, cb}};
    for (const auto& o : out)
        for (const auto& i : in)
            if (overlaps(o.p, o.n, i.p, i.n)) return fail(MCGMIL_E_INVALID, "an output overlaps an input");
    if (overlaps(a->dz, zb, a->dgamma, cb) || overlaps(a->dz, zb, a->dbeta, cb) || overlaps(a->dgamma, cb, a->dbeta, cb))
        return fail(MCGMIL_E_INVALID, "the outputs overlap each other");
    if (!a->workspace || a->workspace_bytes < pl.total)
        return fail(MCGMIL_E_WORKSPACE, std::string("workspace missing or smaller than ") + size_name + "()");
    if (((uintptr_t)a->workspace & 255u) != 0) return fail(MCGMIL_E_ALIGN, "workspace must be 256-byte aligned");

    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ci = a->channels;
    const T* z = static_cast<const T*>(a->z);
    const T* dy = static_cast<const T*>(a->dy);
    float* coef = static_cast<float*>(a->workspace);    // [3][C] (+ C of padding)
    float* part = coef + 4 * Ci;                        // [parts][2][C]
    hipLaunchKernelGGL((bn_pool_grad_kernel<T, false>), dim3((unsigned)pl.parts), dim3(kThreads), 0, s, z, a->argmax, dy,
                       a->mean, a->invstd, pl.q, pl.rows, Ci, pl.rpp, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "bn_pool_grad_kernel (partial sums) launch");
    finalize(part, pl.parts, pl.rows, Ci, a->gamma, a->invstd, coef, a->dgamma, a->dbeta, s);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "bn_grad_finalize_kernel launch");
    if (a->dz) {
        hipLaunchKernelGGL((bn_pool_grad_kernel<T, true>), dim3((unsigned)pl.parts), dim3(kThreads), 0, s, z, a->argmax,
                           dy, a->mean, coef, pl.q, pl.rows, Ci, pl.rpp, static_cast<T*>(a->dz));
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "bn_pool_grad_kernel (apply) launch");
    }
    return MCGMIL_OK;
}

}  // namespace

#endif /* MCGMIL_POOL_GRAD_KERNELS_H_ */
