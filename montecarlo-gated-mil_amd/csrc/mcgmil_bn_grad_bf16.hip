// bf16 backward of the fused BatchNorm (+ residual add) (+ ReLU) of the backbone
// (include/mcgmil_bn_grad_bf16.h): the gradient of mcgmil_batchnorm_act (mcgmil_bn.hip) with
// dtype = MCGMIL_BF16 in batch-statistics mode. Reference: loss.backward() through
// relu?(bn(x) [+ residual]) of the ResNet blocks under torch.autocast(bfloat16), where torch runs
// threshold_backward and native_batch_norm_backward on bf16 tensors.
//
// The kernels are the __bf16 instantiations of mcgmil_bn_grad_kernels.h (the fp32 backward of
// mcgmil_bn_grad.hip instantiates the same templates for float): x, y, dy, dx and dresidual are
// bf16, one 16-byte load or store per 8 channels; mean, invstd, gamma, the partials, the
// coefficients, dgamma and dbeta are fp32. The finalize is mcgmil_bn_grad.hip's own kernel
// (mcgmil_detail::bn_grad_finalize), so this file holds no second one. Same thread-to-element map
// and row partition as fp32: the same summation order, one rounding (to nearest even) at the
// store of dx.
// HBM-bound at half the fp32 backward's bytes: x, dy (and y) are read twice, dx (and dresidual)
// written once. No floating-point atomics; every sum has one fixed order.
#include "../../include/mcgmil_bn_grad_bf16.h"
#include "mcgmil_bn_grad_kernels.h"     // bn_grad_partial_kernel, bn_grad_apply_kernel, plan_for, backward

namespace mcgmil_detail {
// launches bn_grad_finalize_kernel (mcgmil_bn_grad.hip); the caller checks hipGetLastError()
void bn_grad_finalize(const float* part, long long parts, long long rows, int C, const float* gamma,
                      const float* invstd, float* coef, float* dgamma, float* dbeta, hipStream_t s);
}

extern "C" {

size_t mcgmil_bn_grad_bf16_args_size(void) { return sizeof(mcgmil_bn_grad_bf16_args); }

int mcgmil_bn_grad_workspace_size_bf16(const mcgmil_bn_grad_bf16_args* a, size_t* bytes) {
    Plan pl;
    if (int rc = plan_for(a, pl, "mcgmil_bn_grad_bf16_args")) return rc;
    if (!bytes) return fail(MCGMIL_E_INVALID, "bytes is NULL");
    *bytes = pl.total;
    return MCGMIL_OK;
}

int mcgmil_batchnorm_act_backward_bf16(const mcgmil_bn_grad_bf16_args* a, void* stream) {
    return backward<__bf16>(a, stream, "mcgmil_bn_grad_bf16_args", "mcgmil_bn_grad_workspace_size_bf16",
                            mcgmil_detail::bn_grad_finalize);
}

}  // extern "C"
