/*
 * mcgmil_conv_grad_x3.h -- C ABI of the bf16x3 weight gradient of the backbone's fp32 block
 * convolutions on the MI355X (gfx950): the gradient of mcgmil_conv2d_f32x3
 * (include/mcgmil_features.h) with respect to its weight, for training with fp32 storage on the
 * bf16 matrix pipe.
 *
 * Reference interface served (the reference trains through torch autograd; there is no FFI):
 *   mcgmil_conv2d_wgrad_f32x3  <- loss.backward() through torch.nn.Conv2d (bias=False, groups=1,
 *                                 dilation=1) of the ResNet feature extractor (model.py:166-179) in
 *                                 fp32, at torch.set_float32_matmul_precision("high")
 *
 *   dW[o, kh, kw, i] = sum over (n, oh, ow) of dY[n, oh, ow, o] * x[n, oh*s + kh - p, ow*s + kw - p, i]
 *
 * with zero padding: the GEMM of mcgmil_conv_grad.h (M = out_channels, N = kernel_h * kernel_w *
 * in_channels, K = batch * OH * OW output pixels) on v_mfma_f32_16x16x32_bf16. x, dY and dW are the
 * fp32 tensors of mcgmil_conv_grad.h, so the struct is mcgmil_conv_grad_args itself. Numerics: the
 * split of include/mcgmil_features.h ("bf16x3"): every operand value v becomes hi = bf16_rne(v) and
 * lo = bf16_rne(v - float(hi)), and every K step adds dy_hi * x_hi, dy_hi * x_lo and dy_lo * x_hi,
 * in that order, into one fp32 accumulator; the lo * lo term is dropped. Each dW element is within
 * 3 * 2^-16 * sum |dY| |x| of the exact sum, plus the fp32 accumulation error. 3/16 of the
 * matrix-pipe work of mcgmil_conv2d_wgrad_f32.
 *
 * Determinism: the scheme of mcgmil_conv_grad.h, unchanged. No floating-point atomics. K is cut
 * into granules of MCGMIL_WGRAD_GRANULE_PIXELS consecutive output pixels; each (output tile,
 * granule) writes one partial sum to the workspace and a reduce kernel adds the partials in granule
 * order. The launcher walks chunks of whole granules, so two calls agree bitwise, whatever
 * chunk_pixels is and whatever device runs them.
 *
 * Supported: kernel 1..7 per axis, stride 1 or 2, pad < kernel, in_channels a multiple of 32 (the
 * domain of mcgmil_conv2d_f32x3), out_channels a multiple of 64, batch * OH * OW < 2^31 - 256,
 * reserved == 0, in_ab == NULL, 16-byte aligned x, dy and dw; otherwise MCGMIL_E_UNSUPPORTED (or
 * MCGMIL_E_INVALID / MCGMIL_E_ALIGN / MCGMIL_E_WORKSPACE as in mcgmil_conv_grad.h). Offsets into x
 * and dy are 64-bit.
 *
 * Conventions are those of mcgmil.h. This header adds two entry points only; mcgmil_conv_args,
 * mcgmil_conv_grad_args and MCGMIL_ABI_VERSION are unchanged.
 */
#ifndef MCGMIL_CONV_GRAD_X3_H_
#define MCGMIL_CONV_GRAD_X3_H_

#include "mcgmil_conv_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch mcgmil_conv2d_wgrad_f32x3 needs for this geometry and chunk_pixels: with
 * E = out_channels * kernel_h * kernel_w * in_channels and g = granules per chunk,
 * (1 + g) * E fp32 words (the running sum, then one partial per granule of a chunk). chunk_pixels
 * means what it means in mcgmil_conv_grad_args. */
int mcgmil_conv_wgrad_workspace_size_f32x3(const mcgmil_conv_grad_args* a, size_t* bytes);

/* dw = the weight gradient of the forward call described by a->fwd, given dy, at bf16x3. */
int mcgmil_conv2d_wgrad_f32x3(const mcgmil_conv_grad_args* a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCGMIL_CONV_GRAD_X3_H_ */
