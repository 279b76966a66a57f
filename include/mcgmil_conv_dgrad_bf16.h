/*
 * mcgmil_conv_dgrad_bf16.h -- C ABI of the bf16 data gradient of the backbone's convolutions on
 * the MI355X (gfx950): the gradient of mcgmil_conv2d (include/mcgmil_features.h) with respect to
 * its input, for stride 1 and stride 2, as one direct kernel. The bf16 sibling of
 * include/mcgmil_conv_dgrad.h.
 *
 * Reference interface served (the reference trains through torch autograd; there is no FFI):
 *   mcgmil_conv2d_dgrad_bf16 <- loss.backward() through torch.nn.Conv2d (bias=False, groups=1,
 *                               dilation=1) of the ResNet feature extractor (model.py:166-179)
 *                               under torch.autocast("cuda", torch.bfloat16)
 *
 *   dX[n, ih, iw, i] = sum over (kh, kw, o) of dY[n, oh, ow, o] * W[o, i, kh, kw]
 *                      with oh*s + kh - p = ih, ow*s + kw - p = iw, 0 <= oh < OH, 0 <= ow < OW
 *
 * Method: the residue classes of mcgmil_conv_dgrad.h. An input pixel belongs to class
 * (r_h, r_w) = ((ih + p) mod s, (iw + p) mod s); only the taps kh = r_h + s*m_h < KH,
 * kw = r_w + s*m_w < KW reach it, from oh = (ih + p - r_h)/s - m_h and ow likewise, so inside a
 * class the data gradient is a stride-1 implicit GEMM with M = in_channels, N = the class's pixels
 * and K = (taps of the class) * out_channels, here on v_mfma_f32_16x16x32_bf16: bf16 operands,
 * fp32 accumulation, one rounding to nearest-even at the store of dx. There is no zero insertion.
 * A class without taps and input rows or columns past the last window are written as +0.
 *
 * Determinism: every dx element is written exactly once, by one lane; no split-K, no atomics, no
 * workspace. An element's summation order is its class's taps in (kh, kw) order, out ascending
 * within a tap in steps of 32: a function of the geometry alone, not of the grid, the device or
 * the batch. Two calls agree bitwise, and so does an image computed alone against the same image
 * in a batch.
 *
 * Supported: kernel 1..7 per axis (kernel_h != kernel_w allowed), stride 1 or 2, pad < kernel,
 * in_channels and out_channels multiples of 64, fewer than 2^31 - 256 input pixels per class, dx
 * and dy below 2^31 bytes each; otherwise MCGMIL_E_UNSUPPORTED. NULL dy, w_t or dx, one of them
 * not 16-byte aligned, or a non-zero reserved: MCGMIL_E_INVALID. Every check happens before any
 * launch.
 *
 * Conventions are those of mcgmil_conv_grad.h: device pointers, caller-owned buffers,
 * stream-ordered launches without host synchronisation, 0 or a negative MCGMIL_E* code with the
 * message in mcgmil_last_error(). This header adds entry points only; mcgmil_conv_args and
 * MCGMIL_ABI_VERSION are unchanged.
 */
#ifndef MCGMIL_CONV_DGRAD_BF16_H_
#define MCGMIL_CONV_DGRAD_BF16_H_

#include "mcgmil_features.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcgmil_conv_dgrad_bf16_args {
    mcgmil_conv_args fwd;      /* the forward call's geometry; x, w, y, stats, in_ab, workspace
                                  and flags are ignored */
    const void* dy;            /* [batch, OH, OW, out_channels] bf16 NHWC */
    const void* w_t;           /* [kh][kw][in][out] bf16: weight.permute(2, 3, 1, 0), contiguous */
    void* dx;                  /* [batch, H, W, in_channels] bf16 NHWC, OVERWRITTEN, every element */
    int64_t reserved;          /* must be 0 */
} mcgmil_conv_dgrad_bf16_args;

size_t mcgmil_conv_dgrad_bf16_args_size(void);   /* sizeof(mcgmil_conv_dgrad_bf16_args) */

/* Host-only arithmetic of the launch: per residue class, in (r_h, r_w) row-major order, the
 * number of taps, of input pixels, and of pixel tiles (256 pixels when in_channels == 64, else
 * 128) the grid's x axis holds for it. Entries past stride^2 are 0. Pointers are not looked at. */
int mcgmil_conv_dgrad_classes_bf16(const mcgmil_conv_dgrad_bf16_args* a, int32_t taps[4], int64_t pixels[4],
                                   int64_t tiles[4]);

/* dx = the data gradient of the forward call described by a->fwd, given dy and the weight. */
int mcgmil_conv2d_dgrad_bf16(const mcgmil_conv_dgrad_bf16_args* a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCGMIL_CONV_DGRAD_BF16_H_ */
