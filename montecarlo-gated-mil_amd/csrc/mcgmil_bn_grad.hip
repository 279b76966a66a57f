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
#include "mcgmil_bn_grad_kernels.h"     // bn_grad_partial_kernel, bn_grad_apply_kernel, plan_for, backward

namespace {

constexpr int kFinCh = 8;             // finalize: channels per workgroup
constexpr int kFinLanes = kThreads / kFinCh;    // finalize: lanes per channel

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
    if (int rc = plan_for(a, pl, "mcgmil_bn_grad_args")) return rc;
    if (!bytes) return fail(MCGMIL_E_INVALID, "bytes is NULL");
    *bytes = pl.total;
    return MCGMIL_OK;
}

int mcgmil_batchnorm_act_backward(const mcgmil_bn_grad_args* a, void* stream) {
    return backward<float>(a, stream, "mcgmil_bn_grad_args", "mcgmil_bn_grad_workspace_size",
                           mcgmil_detail::bn_grad_finalize);
}

}  // extern "C"
