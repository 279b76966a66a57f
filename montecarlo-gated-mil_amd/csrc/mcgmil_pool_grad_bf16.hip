// bf16 form of the stem's fused BatchNorm (+ ReLU) + max-pool training op
// (include/mcgmil_pool_grad_bf16.h): the forward with the argmax codes on a bf16 activation and the
// backward through pool(relu?(bn(z))) in batch-statistics mode. Reference:
// maxpool(relu(bn1(conv1(x)))) of the torchvision stem under torch.autocast(bfloat16) and
// loss.backward() through it, where torch runs max_pool2d_with_indices_backward,
// threshold_backward and native_batch_norm_backward on bf16 tensors.
//
// The kernels are the __bf16 instantiations of mcgmil_pool_grad_kernels.h (the fp32 op of
// mcgmil_pool_grad.hip instantiates the same templates for float): z, y, dy and dz are bf16, one
// 16-byte load or store per 8 channels; a, b, mean, invstd, gamma, the partials, the coefficients,
// dgamma and dbeta are fp32, and the codes are taken on the unrounded fp32 activated value. The
// finalize is mcgmil_bn_grad.hip's own kernel (mcgmil_detail::bn_grad_finalize). Same
// thread-to-element map and partition as fp32: the same summation order, one rounding (to nearest
// even) at the store of y and of dz.
// HBM-bound at half the fp32 op's activation bytes: z is read twice and dz written once; dy (1/4 of
// z's bytes at the stem's 3/2/1 pool) and the codes (1/8) are read about 2.25 times per pass,
// mostly from L2. No floating-point atomics; every sum has one fixed order. 64-bit offsets.
#include "../../include/mcgmil_pool_grad_bf16.h"
#include "mcgmil_pool_grad_kernels.h"    // bn_pool_argmax_kernel, bn_pool_grad_kernel, plan_for, pool_train, pool_backward

namespace mcgmil_detail {
// launches bn_grad_finalize_kernel (mcgmil_bn_grad.hip); the caller checks hipGetLastError()
void bn_grad_finalize(const float* part, long long parts, long long rows, int C, const float* gamma,
                      const float* invstd, float* coef, float* dgamma, float* dbeta, hipStream_t s);
}

extern "C" {

size_t mcgmil_bn_pool_grad_bf16_args_size(void) { return sizeof(mcgmil_bn_pool_grad_bf16_args); }

int mcgmil_batchnorm_pool_train_bf16(const mcgmil_bn_args* a, uint8_t* argmax, void* stream) {
    return pool_train<__bf16>(a, argmax, stream, MCGMIL_BF16, "mcgmil_batchnorm_pool_train_bf16 is bf16 only");
}

int mcgmil_bn_pool_grad_workspace_size_bf16(const mcgmil_bn_pool_grad_bf16_args* a, size_t* bytes) {
    Plan pl;
    if (int rc = plan_for(a, pl, "mcgmil_bn_pool_grad_bf16_args")) return rc;
    if (!bytes) return fail(MCGMIL_E_INVALID, "bytes is NULL");
    *bytes = pl.total;
    return MCGMIL_OK;
}

int mcgmil_batchnorm_pool_backward_bf16(const mcgmil_bn_pool_grad_bf16_args* a, void* stream) {
    return pool_backward<__bf16>(a, stream, "mcgmil_bn_pool_grad_bf16_args", "mcgmil_bn_pool_grad_workspace_size_bf16",
                                 mcgmil_detail::bn_grad_finalize);
}

}  // extern "C"
