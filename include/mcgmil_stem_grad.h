/*
 * mcgmil_stem_grad.h -- C ABI of the fp32 weight gradient of a convolution with few input
 * channels on the MI355X (gfx950): the gradient of mcgmil_conv2d_f32's gather mode
 * (include/mcgmil_features.h) with respect to its weight, i.e. of the 7x7 stride-2 stem
 * convolution of the ResNet feature extractor.
 *
 * Reference interface served (the reference trains through torch autograd; there is no FFI):
 *   mcgmil_stem_wgrad_f32  <- loss.backward() through conv1 = torch.nn.Conv2d(3, 64, 7, stride=2,
 *                             padding=3, bias=False) of the ResNet feature extractor
 *                             (model.py:166-179) in fp32, as net_utils.train_gacc runs it
 *
 *   dW[o, ci, kh, kw] = sum over (n, oh, ow) of dY[n, oh, ow, o] * x[n, oh*s + kh - p, ow*s + kw - p, ci]
 *
 * with zero padding: a GEMM with M = out_channels, N = kernel_h * kernel_w * in_channels (at most
 * 196) and K = batch * OH * OW output pixels on v_mfma_f32_16x16x4_f32 (fp32 operands, fp32
 * accumulation). The stem needs no data gradient: the instances do not require grad.
 *
 * Determinism (the contract of mcgmil_conv_grad.h): no floating-point atomics. K is cut into
 * granules of MCGMIL_WGRAD_GRANULE_PIXELS consecutive output pixels; each (output tile, granule)
 * writes one partial sum to the workspace and a reduce kernel adds the partials in granule order.
 * The waves of a workgroup split the output channels, never a granule's pixels, so there is no
 * cross-wave sum. The granule does not depend on the device, and the launcher walks chunks of
 * whole granules, so two calls agree bitwise, whatever chunk_pixels is and whatever device runs
 * them.
 *
 * Supported: in_channels 1..4, out_channels a multiple of 64 (at most 4096), kernel 1..7 per axis
 * (kernel_h and kernel_w may differ), stride 1 or 2, pad < min(kernel_h, kernel_w), height and
 * width < 2^24, batch * OH * OW < 2^31 - 256, in_ab == NULL, reserved == 0, 16-byte aligned dy and dw, 4-byte aligned x; otherwise
 * MCGMIL_E_UNSUPPORTED or MCGMIL_E_INVALID. Offsets into x and dy are 64-bit: tensors past 2 GiB
 * are fine.
 *
 * Conventions are those of mcgmil.h. This header adds entry points only; mcgmil_conv_grad_args
 * and MCGMIL_ABI_VERSION are unchanged.
 */
#ifndef MCGMIL_STEM_GRAD_H_
#define MCGMIL_STEM_GRAD_H_

#include "mcgmil_conv_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch mcgmil_stem_wgrad_f32 needs for this geometry and chunk_pixels: with
 * E = out_channels * kernel_h * kernel_w * in_channels, G = ceil(batch * OH * OW /
 * MCGMIL_WGRAD_GRANULE_PIXELS) and g = granules per chunk = min(G, max(1, chunk_pixels ?
 * chunk_pixels / MCGMIL_WGRAD_GRANULE_PIXELS : MCGMIL_WGRAD_DEFAULT_PARTIAL_BYTES / (4 E))),
 * (1 + g) * E fp32 words (the running sum, then one partial per granule of a chunk). */
int mcgmil_stem_wgrad_workspace_size_f32(const mcgmil_conv_grad_args* a, size_t* bytes);

/* dw = the weight gradient of the forward call described by a->fwd, given dy. The workspace is
 * 256-byte aligned; a NULL or short one is MCGMIL_E_WORKSPACE. */
int mcgmil_stem_wgrad_f32(const mcgmil_conv_grad_args* a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCGMIL_STEM_GRAD_H_ */
