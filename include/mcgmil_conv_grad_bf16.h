/*
 * mcgmil_conv_grad_bf16.h -- C ABI of the bf16 weight gradient of the backbone's block
 * convolutions on the MI355X (gfx950): the gradient of mcgmil_conv2d (include/mcgmil_features.h)
 * with respect to its weight, for mixed-precision training.
 *
 * Reference interface served (the reference trains through torch autograd; there is no FFI):
 *   mcgmil_conv2d_wgrad_bf16  <- loss.backward() through torch.nn.Conv2d (bias=False, groups=1,
 *                                dilation=1) of the ResNet feature extractor (model.py:166-179)
 *                                under torch.autocast("cuda", torch.bfloat16)
 *
 *   dW[o, kh, kw, i] = sum over (n, oh, ow) of dY[n, oh, ow, o] * x[n, oh*s + kh - p, ow*s + kw - p, i]
 *
 * with zero padding: the GEMM of mcgmil_conv_grad.h (M = out_channels, N = kernel_h * kernel_w *
 * in_channels, K = batch * OH * OW output pixels) on v_mfma_f32_16x16x32_bf16: bf16 operands, whose
 * products are exact in fp32, and fp32 accumulation. dW is fp32, so it can be the .grad of an fp32
 * master weight without a cast. The stride-1 data gradient needs no entry point of its own: it is
 * mcgmil_conv2d of dY with the taps flipped and the channel axes swapped.
 *
 * Determinism: the scheme of mcgmil_conv_grad.h, unchanged. No floating-point atomics. K is cut
 * into granules of MCGMIL_WGRAD_GRANULE_PIXELS consecutive output pixels; each (output tile,
 * granule) writes one partial sum to the workspace and a reduce kernel adds the partials in granule
 * order. The launcher walks chunks of whole granules, so two calls agree bitwise, whatever
 * chunk_pixels is and whatever device runs them.
 *
 * Supported: kernel 1..7 per axis, stride 1 or 2, pad < kernel, in_channels and out_channels
 * multiples of 64 (the domain of mcgmil_conv2d), batch * OH * OW < 2^31 - 256, 16-byte aligned x,
 * dy and dw; otherwise MCGMIL_E_UNSUPPORTED. Offsets into x and dy are 64-bit.
 *
 * Conventions are those of mcgmil.h: device pointers, caller-owned buffers, stream-ordered
 * launches without host synchronisation, 0 or a negative MCGMIL_E* code with the message in
 * mcgmil_last_error(). This header adds entry points only; mcgmil_conv_args, mcgmil_conv_grad.h
 * and MCGMIL_ABI_VERSION are unchanged.
 */
#ifndef MCGMIL_CONV_GRAD_BF16_H_
#define MCGMIL_CONV_GRAD_BF16_H_

#include "mcgmil_conv_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcgmil_conv_grad_bf16_args {
    mcgmil_conv_args fwd;      /* the forward call's geometry and x (bf16 NHWC); w, y, stats,
                                  workspace and flags are ignored; in_ab must be NULL */
    const void* dy;            /* [batch, OH, OW, out_channels] bf16 NHWC */
    float* dw;                 /* [out, in, kh, kw] fp32, torch layout, OVERWRITTEN */
    void* workspace;           /* >= mcgmil_conv_wgrad_workspace_size_bf16() bytes, 256-byte aligned */
    size_t workspace_bytes;
    /* Cap on the output pixels per launch chunk, as in mcgmil_conv_grad_args: a chunk is
     * max(1, chunk_pixels / MCGMIL_WGRAD_GRANULE_PIXELS) granules; 0 = as many granules as keep
     * the partials within MCGMIL_WGRAD_DEFAULT_PARTIAL_BYTES (at least one). */
    int64_t chunk_pixels;
    int64_t reserved;          /* must be 0 */
} mcgmil_conv_grad_bf16_args;

size_t mcgmil_conv_grad_bf16_args_size(void);    /* sizeof(mcgmil_conv_grad_bf16_args), for binding checks */

/* Bytes of scratch mcgmil_conv2d_wgrad_bf16 needs for this geometry and chunk_pixels: with
 * E = out_channels * kernel_h * kernel_w * in_channels and g = granules per chunk,
 * (1 + g) * E fp32 words (the running sum, then one partial per granule of a chunk). */
int mcgmil_conv_wgrad_workspace_size_bf16(const mcgmil_conv_grad_bf16_args* a, size_t* bytes);

/* dw = the weight gradient of the forward call described by a->fwd, given dy. */
int mcgmil_conv2d_wgrad_bf16(const mcgmil_conv_grad_bf16_args* a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCGMIL_CONV_GRAD_BF16_H_ */
