/*
 * mcgmil_bn_grad_bf16.h -- C ABI of the bf16 backward pass of the fused BatchNorm (+ residual add)
 * (+ ReLU) of the backbone on the MI355X (gfx950): the gradient of mcgmil_batchnorm_act
 * (include/mcgmil_features.h) with dtype = MCGMIL_BF16 in batch-statistics mode, without pooling.
 *
 * Reference interface served (the reference trains through torch autograd; there is no FFI):
 *   mcgmil_batchnorm_act_backward_bf16  <- loss.backward() through relu?(bn(x) [+ residual]) of
 *                                          the ResNet blocks under torch.autocast(bfloat16), where
 *                                          torch runs threshold_backward and
 *                                          native_batch_norm_backward on bf16 tensors
 *
 * Layout: channels-last (NHWC) activations, i.e. row-major [rows = N*H*W, C] bf16 matrices;
 * C a multiple of 8 and <= 2048, rows >= 2. Everything per channel is fp32: gamma (the fp32 master
 * parameter), mean and invstd (mcgmil_bn_args.batch_mean / batch_invstd of the forward), and dgamma
 * and dbeta, which can therefore be the .grad of the fp32 master parameters without a cast.
 *
 * The formulas are those of include/mcgmil_bn_grad.h. Arithmetic: bf16 is widened to fp32 exactly;
 * every product and sum is fp32 with the fp64 finalize, in the fp32 kernel's order (a thread owns
 * 8 channels of a row there as here, one 16-byte load; the row partition is
 * MCGMIL_BN_GRAD_PART_ELEMS / C rows per block); dx is rounded to bf16 once, to nearest even, at
 * the store; dresidual is dy's own bits where y > 0 and +0 elsewhere. On the same values dgamma and
 * dbeta are therefore bitwise mcgmil_batchnorm_act_backward's, and dx is its dx rounded to bf16.
 *
 * The same three launches, no floating-point atomics, 64-bit offsets, two calls agree bitwise.
 * The domain, the validation order (every check before any launch), the error codes and the
 * workspace formula are those of mcgmil_batchnorm_act_backward. This header adds entry points
 * only; MCGMIL_ABI_VERSION is unchanged.
 */
#ifndef MCGMIL_BN_GRAD_BF16_H_
#define MCGMIL_BN_GRAD_BF16_H_

#include "mcgmil_bn_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcgmil_bn_grad_bf16_args {
    int64_t rows;               /* N * H * W, >= 2 */
    int32_t channels;           /* C, multiple of 8, <= 2048 */
    int32_t relu;               /* 1: the forward ended in max(., 0); needs y */
    const void* x;              /* bf16 [rows, C] the BatchNorm's input */
    const void* y;              /* bf16 [rows, C] the forward's output (mask y > 0); NULL when relu == 0 */
    const void* dy;             /* bf16 [rows, C] */
    const float* gamma;         /* [C] BN weight or NULL (1) */
    const float* mean;          /* [C] mcgmil_bn_args.batch_mean of the forward */
    const float* invstd;        /* [C] mcgmil_bn_args.batch_invstd of the forward */
    /* outputs, each optional (NULL: not computed; at least one is needed), each OVERWRITTEN;
     * none may alias an input */
    void* dx;                   /* bf16 [rows, C] */
    void* dresidual;            /* bf16 [rows, C] = g; with relu == 1 only (without ReLU the residual's
                                   gradient is dy itself: MCGMIL_E_INVALID) */
    float* dgamma;              /* [C] */
    float* dbeta;               /* [C] */
    void* workspace;            /* >= mcgmil_bn_grad_workspace_size_bf16() bytes, 256-byte aligned */
    size_t workspace_bytes;
    int64_t reserved;           /* must be 0 */
} mcgmil_bn_grad_bf16_args;

size_t mcgmil_bn_grad_bf16_args_size(void);     /* sizeof(mcgmil_bn_grad_bf16_args), for binding checks */

/* Bytes of scratch mcgmil_batchnorm_act_backward_bf16 needs: mcgmil_bn_grad_workspace_size's formula
 * (the partials and coefficients are fp32 here too). Only rows, channels and reserved are read. */
int mcgmil_bn_grad_workspace_size_bf16(const mcgmil_bn_grad_bf16_args* a, size_t* bytes);

/* The outputs that are not NULL, from x, y (with relu), dy, gamma, mean and invstd. */
int mcgmil_batchnorm_act_backward_bf16(const mcgmil_bn_grad_bf16_args* a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCGMIL_BN_GRAD_BF16_H_ */
