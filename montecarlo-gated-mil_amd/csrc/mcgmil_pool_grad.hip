// The stem's fused BatchNorm (+ ReLU) + max-pool as a training op (include/mcgmil_pool_grad.h):
// a forward that also records which tap of each window won, and the backward through
// pool(relu?(bn(z))) in batch-statistics mode, fp32. Reference: maxpool(relu(bn1(conv1(x)))) of
// the torchvision stem (model.py:166-179 under net_utils.train_gacc) and loss.backward() through
// it, where torch runs max_pool2d_with_indices_backward, threshold_backward and
// native_batch_norm_backward.
//
// The kernels are the float instantiations of mcgmil_pool_grad_kernels.h, which describes them
// (the bf16 op of mcgmil_pool_grad_bf16.hip instantiates the same templates for __bf16). The
// finalize between the two backward passes is mcgmil_bn_grad.hip's kernel
// (mcgmil_detail::bn_grad_finalize).
#include "mcgmil_pool_grad_kernels.h"    // bn_pool_argmax_kernel, bn_pool_grad_kernel, plan_for, pool_train, pool_backward

namespace mcgmil_detail {
// launches bn_grad_finalize_kernel (mcgmil_bn_grad.hip); the caller checks hipGetLastError()
void bn_grad_finalize(const float* part, long long parts, long long rows, int C, const float* gamma,
                      const float* invstd, float* coef, float* dgamma, float* dbeta, hipStream_t s);
}

extern "C" {

size_t mcgmil_bn_pool_grad_args_size(void) { return sizeof(mcgmil_bn_pool_grad_args); }

int mcgmil_batchnorm_pool_train(const mcgmil_bn_args* a, uint8_t* argmax, void* stream) {
    return pool_train<float>(a, argmax, stream, MCGMIL_F32, "mcgmil_batchnorm_pool_train is fp32 only");
}

int mcgmil_bn_pool_grad_workspace_size(const mcgmil_bn_pool_grad_args* a, size_t* bytes) {
    Plan pl;
    if (int rc = plan_for(a, pl, "mcgmil_bn_pool_grad_args")) return rc;
    if (!bytes) return fail(MCGMIL_E_INVALID, "bytes is NULL");
    *bytes = pl.total;
    return MCGMIL_OK;
}

int mcgmil_batchnorm_pool_backward(const mcgmil_bn_pool_grad_args* a, void* stream) {
    return pool_backward<float>(a, stream, "mcgmil_bn_pool_grad_args", "mcgmil_bn_pool_grad_workspace_size",
                                mcgmil_detail::bn_grad_finalize);
}

}  // extern "C"
