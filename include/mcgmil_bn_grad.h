/*
 * mcgmil_bn_grad.h -- C ABI of the backward pass of the fused BatchNorm (+ residual add)
 * (+ ReLU) of the backbone on the MI355X (gfx950): the gradient of mcgmil_batchnorm_act
 * (include/mcgmil_features.h) in batch-statistics mode, fp32, without pooling.
 *
 * Reference interface served (the reference trains through torch autograd; there is no FFI):
 *   mcgmil_batchnorm_act_backward  <- loss.backward() through relu?(bn(x) [+ residual]) of the
 *                                     ResNet blocks (torchvision BasicBlock / Bottleneck as built
 *                                     at model.py:166-179; torch runs threshold_backward and
 *                                     native_batch_norm_backward), with the BatchNorm on the
 *                                     bag's own statistics, as net_utils.train_gacc runs it
 *
 * Layout: channels-last (NHWC) activations, i.e. row-major [rows = N*H*W, C] fp32 matrices;
 * C a multiple of 8 and <= 2048, rows >= 2 (as torch's training BatchNorm).
 *
 * With xh = (x - mean_c) * invstd_c, g = dy * [y > 0] (g = dy without ReLU) and n = rows:
 *   dbeta_c     = sum over rows of g
 *   dgamma_c    = sum over rows of g * xh
 *   dx          = gamma_c * invstd_c * (g - dbeta_c / n - xh * dgamma_c / n)
 *   dresidual   = g
 * mean and invstd are what mcgmil_batchnorm_act wrote to batch_mean / batch_invstd; y is its
 * output and is read for the ReLU mask only. The gradients that would flow into mean / invstd as
 * outputs of their own are not part of this formula (they are statistics of x, not parameters).
 *
 * Three launches: per-workgroup fp32 sums of g and g * xh over MCGMIL_BN_GRAD_PART_ELEMS / C
 * consecutive rows; an fp64 combination of those partials in a fixed order, which writes dgamma,
 * dbeta and three per-channel coefficients; and one elementwise pass dx = k1 g + k2 (x - mean)
 * + k3 that reads and writes every element once.
 *
 * Determinism: no floating-point atomics. The row partition is a function of (rows, C) alone
 * (never of the device's CU count) and every sum has one fixed order, so two calls with the same
 * arguments agree bitwise, on any device.
 *
 * Conventions are those of mcgmil.h: device pointers, caller-owned buffers, stream-ordered
 * launches without allocation or host synchronisation, 0 or a negative MCGMIL_E* code with the
 * message in mcgmil_last_error(). This header adds entry points only; MCGMIL_ABI_VERSION is
 * unchanged.
 */
#ifndef MCGMIL_BN_GRAD_H_
#define MCGMIL_BN_GRAD_H_

#include "mcgmil_features.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Elements (rows x C) of one partial-sum block: a block is MCGMIL_BN_GRAD_PART_ELEMS / C
 * consecutive rows (128 KB of x). Fixed: the summation order is tied to it. */
#define MCGMIL_BN_GRAD_PART_ELEMS 32768

typedef struct mcgmil_bn_grad_args {
    int64_t rows;               /* N * H * W, >= 2 */
    int32_t channels;           /* C, multiple of 8, <= 2048 */
    int32_t relu;               /* 1: the forward ended in max(., 0); needs y */
    const float* x;             /* [rows, C] the BatchNorm's input */
    const float* y;             /* [rows, C] the forward's output (mask y > 0); NULL when relu == 0 */
    const float* dy;            /* [rows, C] */
    const float* gamma;         /* [C] BN weight or NULL (1) */
    const float* mean;          /* [C] mcgmil_bn_args.batch_mean of the forward */
    const float* invstd;        /* [C] mcgmil_bn_args.batch_invstd of the forward */
    /* outputs, each optional (NULL: not computed; at least one is needed), each OVERWRITTEN;
     * none may alias an input */
    float* dx;                  /* [rows, C] */
    float* dresidual;           /* [rows, C] = g; with relu == 1 only (without ReLU the residual's
                                   gradient is dy itself: MCGMIL_E_INVALID) */
    float* dgamma;              /* [C] */
    float* dbeta;               /* [C] */
    void* workspace;            /* >= mcgmil_bn_grad_workspace_size() bytes, 256-byte aligned */
    size_t workspace_bytes;
    int64_t reserved;           /* must be 0 */
} mcgmil_bn_grad_args;

size_t mcgmil_bn_grad_args_size(void);      /* sizeof(mcgmil_bn_grad_args), for binding checks */

/* Bytes of scratch mcgmil_batchnorm_act_backward needs: with parts = ceil(rows / (MCGMIL_BN_GRAD_PART_ELEMS / C)),
 * (4 C + 2 C parts) fp32 words (the apply pass's coefficients, then one [2][C] partial per
 * block), rounded up to 256 bytes. Only rows, channels and reserved are read. */
int mcgmil_bn_grad_workspace_size(const mcgmil_bn_grad_args* a, size_t* bytes);

/* The outputs that are not NULL, from x, y (with relu), dy, gamma, mean and invstd. */
int mcgmil_batchnorm_act_backward(const mcgmil_bn_grad_args* a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCGMIL_BN_GRAD_H_ */
