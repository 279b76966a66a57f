/*
 * mcgmil_pool_grad_bf16.h -- C ABI of the bf16 form of the stem's fused BatchNorm (+ ReLU) +
 * max-pool training op on the MI355X (gfx950): the forward of include/mcgmil_pool_grad.h on a bf16
 * activation, and its backward. Batch-statistics mode.
 *
 * Reference interface served (the reference trains through torch autograd; there is no FFI):
 *   mcgmil_batchnorm_pool_train_bf16     maxpool(relu(bn1(z))) of torchvision ResNet.forward's stem
 *                                        under torch.autocast(bfloat16), z = conv1(x) in bf16
 *   mcgmil_batchnorm_pool_backward_bf16  loss.backward() through those three layers, where torch runs
 *                                        max_pool2d_with_indices_backward, threshold_backward and
 *                                        native_batch_norm_backward on bf16 tensors, from a saved z, a
 *                                        saved ReLU output of z's size and the pool's int64 indices
 *
 * Layout: channels-last (NHWC) bf16 activations: z and dz are [N, H, W, C], y and dy are
 * [N, PH, PW, C]; the argmax codes are the uint8 [N, PH, PW, C] tensor of mcgmil_pool_grad.h. The
 * domain (C a multiple of 8 and <= 2048, N * H * W >= 2, k in {2, 3}, 1 <= stride <= k,
 * 0 <= pad <= k / 2), the formulas, the validation order (every check before any launch), the
 * error codes and the workspace formula are those of mcgmil_pool_grad.h. Everything per channel is
 * fp32: gamma (the fp32 master parameter), mean and invstd (mcgmil_bn_args.batch_mean /
 * batch_invstd of the forward), and dgamma and dbeta, which can therefore be the .grad of the fp32
 * master parameters without a cast.
 *
 * Arithmetic. bf16 is widened to fp32 exactly. The argmax code is the first strict maximum of the
 * UNROUNDED fp32 activated value fmaf(z, a_c, b_c) over the window's in-image taps in row-major
 * (kh, kw) order, and MCGMIL_POOL_ARGMAX_NONE (255) where that maximum is <= 0 with ReLU: exactly
 * the fp32 kernel's rule. y is that maximum rounded once to bf16, which makes it bitwise
 * mcgmil_batchnorm_act's bf16 output with pooling. Every sum and product of the backward is fp32,
 * with the fp64 finalize of mcgmil_bn_grad.h, in the fp32 kernel's order: the thread-to-element map
 * is the fp32 kernel's (a thread owns 8 channels of an input pixel: one 16-byte load of z, one
 * 16-byte load of dy per covering window, one 8-byte load of codes) and so is the partition
 * (MCGMIL_BN_POOL_GRAD_PART_ELEMS / C pixels per block). dz is rounded to bf16 once, to nearest
 * even, at the store. On the same bf16 values, codes, mean and invstd, dgamma and dbeta are
 * therefore bitwise mcgmil_batchnorm_pool_backward's and dz is its dz rounded to bf16.
 *
 * A difference from torch.autocast. Torch pools the BatchNorm output AFTER rounding it to bf16:
 * where two taps of a window round to the same bf16 value, torch gives the window's gradient to the
 * first of them. This op gives it to the tap whose unrounded fp32 value is larger (to the first of
 * them only where those are equal too). Both are subgradients of the same forward value y; the
 * gradients differ element by element at such windows, so this op is compared against the
 * autograd of the unrounded function on bf16-valued inputs, not against torch's bf16 autograd.
 *
 * Three launches, no floating-point atomics, 64-bit offsets: two calls with the same arguments
 * agree bitwise. Conventions are those of mcgmil.h. This header adds entry points only;
 * MCGMIL_ABI_VERSION is unchanged, and mcgmil_batchnorm_pool_train keeps answering
 * MCGMIL_E_UNSUPPORTED for bf16.
 */
#ifndef MCGMIL_POOL_GRAD_BF16_H_
#define MCGMIL_POOL_GRAD_BF16_H_

#include "mcgmil_pool_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mcgmil_batchnorm_pool_train for dtype == MCGMIL_BF16 (anything else: MCGMIL_E_UNSUPPORTED): a->x
 * and a->y are bf16, a->y is bitwise mcgmil_batchnorm_act's bf16 output with pooling, batch_mean
 * and batch_invstd are fp32, argmax is [N, PH, PW, C] (8-byte aligned). The same rules otherwise:
 * batch statistics from a pass over x, no residual, rows >= 2, a workspace as
 * mcgmil_bn_workspace_size reports. */
int mcgmil_batchnorm_pool_train_bf16(const mcgmil_bn_args* a, uint8_t* argmax, void* stream);

typedef struct mcgmil_bn_pool_grad_bf16_args {
    int32_t batch, height, width;       /* N, H, W of z; N * H * W >= 2 */
    int32_t channels;                   /* C, multiple of 8, <= 2048 */
    int32_t pool_kernel, pool_stride, pool_pad;
    int32_t pooled_height, pooled_width;    /* PH, PW of dy and argmax: must be the pool's */
    int32_t reserved32;                 /* must be 0 */
    const void* z;                      /* bf16 [N, H, W, C] the BatchNorm's input */
    const uint8_t* argmax;              /* [N, PH, PW, C] from mcgmil_batchnorm_pool_train_bf16 */
    const void* dy;                     /* bf16 [N, PH, PW, C] */
    const float* gamma;                 /* [C] BN weight or NULL (1) */
    const float* mean;                  /* [C] mcgmil_bn_args.batch_mean of the forward */
    const float* invstd;                /* [C] mcgmil_bn_args.batch_invstd of the forward */
    /* outputs, each optional (NULL: not computed; at least one is needed), each OVERWRITTEN;
     * none may overlap an input */
    void* dz;                           /* bf16 [N, H, W, C] */
    float* dgamma;                      /* [C] */
    float* dbeta;                       /* [C] */
    void* workspace;                    /* >= mcgmil_bn_pool_grad_workspace_size_bf16() bytes, 256-byte aligned */
    size_t workspace_bytes;
    int64_t reserved;                   /* must be 0 */
} mcgmil_bn_pool_grad_bf16_args;

size_t mcgmil_bn_pool_grad_bf16_args_size(void);    /* sizeof(mcgmil_bn_pool_grad_bf16_args), for binding checks */

/* Bytes of scratch mcgmil_batchnorm_pool_backward_bf16 needs: mcgmil_bn_pool_grad_workspace_size's
 * formula (the partials and coefficients are fp32 here too). Only the integer fields are read. */
int mcgmil_bn_pool_grad_workspace_size_bf16(const mcgmil_bn_pool_grad_bf16_args* a, size_t* bytes);

/* The outputs that are not NULL, from z, argmax, dy, gamma, mean and invstd. z, dy, dz, mean and
 * invstd 16-byte aligned, argmax 8-byte aligned; the overlap checks take z, dy and dz as 2-byte
 * elements. */
int mcgmil_batchnorm_pool_backward_bf16(const mcgmil_bn_pool_grad_bf16_args* a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCGMIL_POOL_GRAD_BF16_H_ */
