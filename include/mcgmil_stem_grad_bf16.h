/*
 * mcgmil_stem_grad_bf16.h -- C ABI of the bf16 stem convolution for mixed-precision training on
 * the MI355X (gfx950): the raw convolution z = conv1(x) of mcgmil_stem_forward
 * (include/mcgmil_features.h) without its BatchNorm, and the gradient of that convolution with
 * respect to its weight.
 *
 * Reference interface served (the reference trains through torch autograd; there is no FFI):
 *   mcgmil_stem_conv_bf16   <- conv1 = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
 *                              of the ResNet feature extractor (model.py:166-179) under
 *                              torch.autocast("cuda", torch.bfloat16)
 *   mcgmil_stem_wgrad_bf16  <- loss.backward() through that layer
 *
 *   dW[o, ci, kh, kw] = sum over (n, oh, ow) of dY[n, oh, ow, o] * x[n, ci, 2*oh + kh - p, 2*ow + kw - p]
 *
 * with zero padding. x is the NCHW bf16 instance batch the forward read (the layout
 * mcgmil_image_to_bag writes), dY bf16 NHWC. The gradient is a GEMM with M = 64 output channels,
 * N = in_channels * kernel * 8 columns (ci, kh, j) -- the forward kernel's own column order, tap j
 * being kernel column kw = j - (P - pad), P = pad + (pad & 1); the taps outside 0..kernel-1 are
 * dead columns that are computed and dropped -- and K = batch * OH * OW output pixels, on
 * v_mfma_f32_16x16x32_bf16: bf16 operands, whose products are exact in fp32, and fp32
 * accumulation. dW is fp32, so it can be the .grad of an fp32 master weight without a cast. The
 * stem needs no data gradient: the instances do not require grad.
 *
 * Determinism (the contract of mcgmil_conv_grad.h, unchanged): no floating-point atomics. K is cut
 * into granules of MCGMIL_WGRAD_GRANULE_PIXELS consecutive output pixels; each granule writes one
 * partial sum to the workspace (there is one output tile) and a reduce kernel adds the partials in
 * granule order. The waves of a workgroup split the columns, never a granule's pixels, so there is
 * no cross-wave sum. The launcher walks chunks of whole granules, so two calls agree bitwise,
 * whatever chunk_pixels is and whatever device runs them.
 *
 * Supported (the domain of mcgmil_stem_forward): in_channels 1..4, out_channels 64, a square kernel
 * with kernel + (pad & 1) <= 8, stride 2, an even width, OW <= 125, x below 2 GiB; for the
 * gradient also batch * OH * OW < 2^31 - 256, 16-byte aligned dy and dw and a 4-byte aligned x;
 * otherwise MCGMIL_E_UNSUPPORTED, MCGMIL_E_INVALID or MCGMIL_E_ALIGN. Offsets into y and dy are
 * 64-bit: tensors past 2 GiB are fine.
 *
 * Conventions are those of mcgmil.h: device pointers, caller-owned buffers, stream-ordered
 * launches without host synchronisation, 0 or a negative MCGMIL_E* code with the message in
 * mcgmil_last_error(). This header adds entry points only; mcgmil_stem_args and
 * MCGMIL_ABI_VERSION are unchanged.
 */
#ifndef MCGMIL_STEM_GRAD_BF16_H_
#define MCGMIL_STEM_GRAD_BF16_H_

#include "mcgmil_conv_grad.h"
#include "mcgmil_features.h"

#ifdef __cplusplus
extern "C" {
#endif

/* y = conv1(x) alone: the convolution of mcgmil_stem_forward (the same kernel, fp32 accumulation,
 * one rounding to bf16) written to a->y as bf16 NHWC [batch, OH, OW, 64], which may exceed 2^31
 * bytes. No statistics, no BatchNorm pass, no workspace: pool_kernel must be 0 and gamma, beta,
 * running_mean, running_var, batch_mean and batch_invstd NULL; workspace is not read. x is 4-byte
 * and w (mcgmil_pack_stem_weights) and y 16-byte aligned. */
int mcgmil_stem_conv_bf16(const mcgmil_stem_args* a, void* stream);

typedef struct mcgmil_stem_grad_bf16_args {
    mcgmil_stem_args fwd;      /* the forward call's geometry (batch .. pad) and x (bf16 NCHW);
                                  every other field of it is ignored */
    const void* dy;            /* [batch, OH, OW, 64] bf16 NHWC */
    float* dw;                 /* [64, in_channels, kernel, kernel] fp32, torch layout, OVERWRITTEN */
    void* workspace;           /* >= mcgmil_stem_wgrad_workspace_size_bf16() bytes, 256-byte aligned */
    size_t workspace_bytes;
    /* Cap on the output pixels per launch chunk, as in mcgmil_conv_grad_args: a chunk is
     * max(1, chunk_pixels / MCGMIL_WGRAD_GRANULE_PIXELS) granules; 0 = as many granules as keep
     * the partials within MCGMIL_WGRAD_DEFAULT_PARTIAL_BYTES (at least one). */
    int64_t chunk_pixels;
    int64_t reserved;          /* must be 0 */
} mcgmil_stem_grad_bf16_args;

size_t mcgmil_stem_grad_bf16_args_size(void);    /* sizeof(mcgmil_stem_grad_bf16_args), for binding checks */

/* Bytes of scratch mcgmil_stem_wgrad_bf16 needs for this geometry and chunk_pixels: with
 * E = 64 * in_channels * kernel * 8 (the dead taps' columns included), G = ceil(batch * OH * OW /
 * MCGMIL_WGRAD_GRANULE_PIXELS) and g = granules per chunk = min(G, max(1, chunk_pixels ?
 * chunk_pixels / MCGMIL_WGRAD_GRANULE_PIXELS : MCGMIL_WGRAD_DEFAULT_PARTIAL_BYTES / (4 E))),
 * (1 + g) * E fp32 words (the running sum, then one partial per granule of a chunk). */
int mcgmil_stem_wgrad_workspace_size_bf16(const mcgmil_stem_grad_bf16_args* a, size_t* bytes);

/* dw = the weight gradient of the forward call described by a->fwd, given dy. A NULL or short
 * workspace is MCGMIL_E_WORKSPACE. */
int mcgmil_stem_wgrad_bf16(const mcgmil_stem_grad_bf16_args* a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCGMIL_STEM_GRAD_BF16_H_ */
