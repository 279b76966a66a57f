/*
 * mcgmil_pool_grad.h -- C ABI of the stem's fused BatchNorm (+ ReLU) + max-pool as a training op
 * on the MI355X (gfx950): a forward that leaves behind what a backward needs, and that backward.
 * fp32, batch-statistics mode.
 *
 * Reference interface served (the reference trains through torch autograd; there is no FFI):
 *   mcgmil_batchnorm_pool_train     maxpool(relu(bn1(z))) of torchvision ResNet.forward's stem
 *                                   (the backbone built at model.py:166-179), z = conv1(x), with the
 *                                   BatchNorm on the bag's own statistics as net_utils.train_gacc
 *                                   runs it: torch's batch_norm, relu and max_pool2d layers
 *   mcgmil_batchnorm_pool_backward  loss.backward() through those three layers (torch runs
 *                                   max_pool2d_with_indices_backward, threshold_backward and
 *                                   native_batch_norm_backward, from a saved z, a saved ReLU output
 *                                   of z's size and the pool's int64 indices)
 *
 * Layout: channels-last (NHWC) fp32 activations: z and dz are [N, H, W, C], y and dy are
 * [N, PH, PW, C] with PH = (H + 2 pad - k) / stride + 1 (likewise PW); C a multiple of 8 and
 * <= 2048, N * H * W >= 2 (as torch's training BatchNorm).
 *
 * Pool geometry: MaxPool2d(k, stride, pad) in floor mode with -inf padding, k in {2, 3},
 * 1 <= stride <= k, 0 <= pad <= k / 2. Anything else is MCGMIL_E_UNSUPPORTED (the caller keeps
 * torch's layers).
 *
 * The argmax code: a uint8 tensor [N, PH, PW, C], one byte per pooled element. Its value is
 * kh * k + kw of the window's maximum of the activated value fmaf(z, a_c, b_c) (a_c, b_c as in
 * include/mcgmil_features.h), the in-image taps scanned in row-major (kh, kw) order with a strict
 * >, so the FIRST maximum wins (torch's max_pool2d rule). With relu the code is
 * MCGMIL_POOL_ARGMAX_NONE (255) where the window maximum is <= 0: the ReLU zeroes that gradient
 * whichever tap torch would name. The backward reads the codes and never recomputes a window, so
 * it needs no (a_c, b_c) and agrees with the forward's choice bit for bit. Behaviour on NaN (or
 * all -inf) inputs is unspecified.
 *
 * Backward, with n = N * H * W and xh = (z - mean_c) * invstd_c:
 *   g[n, h, w, c] = sum of dy[n, ph, pw, c] over the pooled outputs (ph, pw) whose window contains
 *                   (h, w) and whose code names it, i.e. equals
 *                   (h - ph stride + pad) k + (w - pw stride + pad); ph from
 *                   max(0, ceil((h + pad - k + 1) / stride)) to min(PH - 1, floor((h + pad) / stride)),
 *                   likewise pw; the terms are added in ascending (ph, pw) order
 *   dbeta_c  = sum of g
 *   dgamma_c = sum of g * xh
 *   dz       = gamma_c * invstd_c * (g - dbeta_c / n - xh * dgamma_c / n)
 * Gather form: each thread owns one (input pixel, 8-channel group) and looks up its <= 4 covering
 * windows (<= 9 at stride 1); no floating-point atomics. Three launches, as in mcgmil_bn_grad.h:
 * per-workgroup fp32 sums of g and g * xh over MCGMIL_BN_POOL_GRAD_PART_ELEMS / C consecutive input
 * pixels; the fp64 combination of those partials in a fixed order, which writes dgamma, dbeta and
 * the coefficients k1, k2, k3; and an apply pass dz = k1 g + k2 (z - mean) + k3 that derives g
 * again from dy and the codes (the partial pass stays read-only; the alternative, g written to dz
 * by the partial pass and rewritten in place, was not built and not measured).
 *
 * Determinism: the partition is a function of (N * H * W, C) alone, never of the device's CU
 * count, and every sum has one fixed order: two calls with the same arguments agree bitwise.
 *
 * Conventions are those of mcgmil.h: device pointers, caller-owned buffers, stream-ordered
 * launches without allocation or host synchronisation, 0 or a negative MCGMIL_E* code with the
 * message in mcgmil_last_error(). All offsets are 64-bit. This header adds entry points only;
 * MCGMIL_ABI_VERSION is unchanged.
 */
#ifndef MCGMIL_POOL_GRAD_H_
#define MCGMIL_POOL_GRAD_H_

#include "mcgmil_features.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Elements (input pixels x C) of one partial-sum block: a block is
 * MCGMIL_BN_POOL_GRAD_PART_ELEMS / C consecutive input pixels (128 KB of z). Fixed: the summation
 * order is tied to it. */
#define MCGMIL_BN_POOL_GRAD_PART_ELEMS 32768
/* The argmax code of a pooled element whose gradient the ReLU zeroes. */
#define MCGMIL_POOL_ARGMAX_NONE 255

/* pool(relu?(bn(z))) on the batch statistics of z, exactly as mcgmil_batchnorm_act computes it with
 * pooling (a->y is bitwise that function's output), plus the argmax code [N, PH, PW, C] (8-byte
 * aligned). Needs dtype == MCGMIL_F32, batch statistics from a pass over x (no running statistics,
 * no partials), batch_mean and batch_invstd, no residual, rows >= 2, a pool geometry as above and
 * a workspace as mcgmil_bn_workspace_size reports. */
int mcgmil_batchnorm_pool_train(const mcgmil_bn_args* a, uint8_t* argmax, void* stream);

typedef struct mcgmil_bn_pool_grad_args {
    int32_t batch, height, width;       /* N, H, W of z; N * H * W >= 2 */
    int32_t channels;                   /* C, multiple of 8, <= 2048 */
    int32_t pool_kernel, pool_stride, pool_pad;
    int32_t pooled_height, pooled_width;    /* PH, PW of dy and argmax: must be the pool's */
    int32_t reserved32;                 /* must be 0 */
    const float* z;                     /* [N, H, W, C] the BatchNorm's input */
    const uint8_t* argmax;              /* [N, PH, PW, C] from mcgmil_batchnorm_pool_train */
    const float* dy;                    /* [N, PH, PW, C] */
    const float* gamma;                 /* [C] BN weight or NULL (1) */
    const float* mean;                  /* [C] mcgmil_bn_args.batch_mean of the forward */
    const float* invstd;                /* [C] mcgmil_bn_args.batch_invstd of the forward */
    /* outputs, each optional (NULL: not computed; at least one is needed), each OVERWRITTEN;
     * none may overlap an input */
    float* dz;                          /* [N, H, W, C] */
    float* dgamma;                      /* [C] */
    float* dbeta;                       /* [C] */
    void* workspace;                    /* >= mcgmil_bn_pool_grad_workspace_size() bytes, 256-byte aligned */
    size_t workspace_bytes;
    int64_t reserved;                   /* must be 0 */
} mcgmil_bn_pool_grad_args;

size_t mcgmil_bn_pool_grad_args_size(void);     /* sizeof(mcgmil_bn_pool_grad_args), for binding checks */

/* Bytes of scratch mcgmil_batchnorm_pool_backward needs: with rows = N * H * W and
 * parts = ceil(rows / (MCGMIL_BN_POOL_GRAD_PART_ELEMS / C)), (4 C + 2 C parts) fp32 words (the apply
 * pass's coefficients, then one [2][C] partial per block), rounded up to 256 bytes. Only the
 * integer fields are read. */
int mcgmil_bn_pool_grad_workspace_size(const mcgmil_bn_pool_grad_args* a, size_t* bytes);

/* The outputs that are not NULL, from z, argmax, dy, gamma, mean and invstd. z, dy, dz, mean and
 * invstd 16-byte aligned, argmax 8-byte aligned. */
int mcgmil_batchnorm_pool_backward(const mcgmil_bn_pool_grad_args* a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCGMIL_POOL_GRAD_H_ */
