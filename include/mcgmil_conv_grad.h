/*
 * mcgmil_conv_grad.h -- C ABI of the fp32 weight gradient of the backbone's convolutions on the
 * MI355X (gfx950): the gradient of mcgmil_conv2d_f32 (include/mcgmil_features.h) with respect to
 * its weight.
 *
 * Reference interface served (the reference trains through torch autograd; there is no FFI):
 *   mcgmil_conv2d_wgrad_f32  <- loss.backward() through torch.nn.Conv2d (bias=False, groups=1,
 *                               dilation=1) of the ResNet feature extractor (model.py:166-179) in
 *                               fp32, as net_utils.train_gacc runs it on every bag
 *
 *   dW[o, kh, kw, i] = sum over (n, oh, ow) of dY[n, oh, ow, o] * x[n, oh*s + kh - p, ow*s + kw - p, i]
 *
 * with zero padding: a GEMM with M = out_channels, N = kernel_h * kernel_w * in_channels and
 * K = batch * OH * OW output pixels on v_mfma_f32_16x16x4_f32 (fp32 operands, fp32 accumulation).
 * The data gradient has its own entry point in mcgmil_conv_dgrad.h (mcgmil_conv2d_dgrad_f32, stride
 * 1 and 2); for stride 1 it is also mcgmil_conv2d_f32 of dY with the taps flipped and the channel
 * axes swapped.
 *
 * Determinism: no floating-point atomics. K is cut into granules of MCGMIL_WGRAD_GRANULE_PIXELS
 * consecutive output pixels; each (output tile, granule) writes one partial sum to the workspace
 * and a reduce kernel adds the partials in granule order. The granule does not depend on the
 * device, and the launcher walks chunks of whole granules, so two calls agree bitwise, whatever
 * chunk_pixels is and whatever device runs them.
 *
 * Supported: kernel 1..7 per axis, stride 1 or 2, pad < kernel, in_channels a multiple of 16,
 * out_channels a multiple of 64, batch * OH * OW < 2^31 - 256, 16-byte aligned x, dy and dw;
 * otherwise MCGMIL_E_UNSUPPORTED. Offsets into x and dy are 64-bit: tensors past 2 GiB are fine.
 *
 * Conventions are those of mcgmil.h: device pointers, caller-owned buffers, stream-ordered
 * launches without host synchronisation, 0 or a negative MCGMIL_E* code with the message in
 * mcgmil_last_error(). This header adds entry points only; mcgmil_conv_args and
 * MCGMIL_ABI_VERSION are unchanged.
 */
#ifndef MCGMIL_CONV_GRAD_H_
#define MCGMIL_CONV_GRAD_H_

#include "mcgmil_features.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Output pixels per split-K granule of the weight-gradient GEMM. Fixed: the summation order is
 * tied to it, so it must not follow the device (CU count) or the call (chunk_pixels). */
#define MCGMIL_WGRAD_GRANULE_PIXELS 2048
/* Default cap on the bytes of granule partials in the workspace at once (chunk_pixels == 0). */
#define MCGMIL_WGRAD_DEFAULT_PARTIAL_BYTES (128ll << 20)

typedef struct mcgmil_conv_grad_args {
    mcgmil_conv_args fwd;      /* the forward call's geometry and x (fp32 NHWC); w, y, stats,
                                  workspace and flags are ignored; in_ab must be NULL */
    const float* dy;           /* [batch, OH, OW, out_channels] fp32 NHWC */
    float* dw;                 /* [out, in, kh, kw] fp32, torch layout, OVERWRITTEN */
    void* workspace;           /* >= mcgmil_conv_wgrad_workspace_size_f32() bytes, 256-byte aligned */
    size_t workspace_bytes;
    /* Cap on the output pixels per launch chunk. A chunk is max(1, chunk_pixels /
     * MCGMIL_WGRAD_GRANULE_PIXELS) granules; 0 = as many granules as keep the partials within
     * MCGMIL_WGRAD_DEFAULT_PARTIAL_BYTES (at least one). The launcher walks the chunks on the
     * same stream. */
    int64_t chunk_pixels;
    int64_t reserved;          /* must be 0 */
} mcgmil_conv_grad_args;

size_t mcgmil_conv_grad_args_size(void);    /* sizeof(mcgmil_conv_grad_args), for binding checks */

/* Bytes of scratch mcgmil_conv2d_wgrad_f32 needs for this geometry and chunk_pixels: with
 * E = out_channels * kernel_h * kernel_w * in_channels and g = granules per chunk,
 * (1 + g) * E fp32 words (the running sum, then one partial per granule of a chunk). */
int mcgmil_conv_wgrad_workspace_size_f32(const mcgmil_conv_grad_args* a, size_t* bytes);

/* dw = the weight gradient of the forward call described by a->fwd, given dy. */
int mcgmil_conv2d_wgrad_f32(const mcgmil_conv_grad_args* a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCGMIL_CONV_GRAD_H_ */
