/*
 * mcgmil_conv_dgrad.h -- C ABI of the fp32 data gradient of the backbone's convolutions on the
 * MI355X (gfx950): the gradient of mcgmil_conv2d_f32 (include/mcgmil_features.h) with respect to
 * its input, for stride 1 and stride 2, as one direct kernel.
 *
 * Reference interface served (the reference trains through torch autograd; there is no FFI):
 *   mcgmil_conv2d_dgrad_f32  <- loss.backward() through torch.nn.Conv2d (bias=False, groups=1,
 *                               dilation=1) of the ResNet feature extractor (model.py:166-179) in
 *                               fp32, as net_utils.train_gacc runs it on every bag
 *
 *   dX[n, ih, iw, i] = sum over (kh, kw, o) of dY[n, oh, ow, o] * W[o, i, kh, kw]
 *                      with oh*s + kh - p = ih, ow*s + kw - p = iw, 0 <= oh < OH, 0 <= ow < OW
 *
 * Method: residue classes. An input pixel belongs to class (r_h, r_w) = ((ih + p) mod s,
 * (iw + p) mod s): one class for stride 1, four for stride 2. Only the taps kh = r_h + s*m_h < KH,
 * kw = r_w + s*m_w < KW reach a pixel of that class, from oh = (ih + p - r_h)/s - m_h and ow
 * likewise, so inside a class the data gradient is a stride-1 implicit GEMM with M = in_channels,
 * N = the class's pixels and K = (taps of the class) * out_channels, on v_mfma_f32_16x16x4_f32
 * (fp32 operands, fp32 accumulation). There is no zero insertion: the classes of a 3x3 stride-2
 * convolution have 4, 2, 2 and 1 taps, 9 in all. A class without taps (three of the four of a
 * 1x1 stride-2 convolution) and input rows or columns past the last window are written as zeros.
 *
 * Determinism: every dx element is written exactly once, by one lane; no split-K, no atomics, no
 * workspace. An element's summation order is its class's taps in (kh, kw) order, out ascending
 * within a tap: a function of the geometry alone, not of the grid, the device or the batch. Two
 * calls agree bitwise, and so does an image computed alone against the same image in a batch.
 *
 * Supported: kernel 1..7 per axis (kernel_h != kernel_w allowed), stride 1 or 2, pad < kernel,
 * in_channels a multiple of 16, out_channels a multiple of 64, fewer than 2^31 - 256 input pixels
 * per class; otherwise MCGMIL_E_UNSUPPORTED. Offsets into dy and dx are 64-bit: tensors past
 * 2 GiB are fine. NULL dy, w_t or dx, one of them not 16-byte aligned, or a non-zero reserved:
 * MCGMIL_E_INVALID. Every check happens before any launch.
 *
 * Conventions are those of mcgmil_conv_grad.h: device pointers, caller-owned buffers,
 * stream-ordered launches without host synchronisation, 0 or a negative MCGMIL_E* code with the
 * message in mcgmil_last_error(). This header adds entry points only; mcgmil_conv_args and
 * MCGMIL_ABI_VERSION are unchanged.
 */
#ifndef MCGMIL_CONV_DGRAD_H_
#define MCGMIL_CONV_DGRAD_H_

#include "mcgmil_features.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcgmil_conv_dgrad_args {
    mcgmil_conv_args fwd;      /* the forward call's geometry; x, w, y, stats, in_ab, workspace
                                  and flags are ignored */
    const float* dy;           /* [batch, OH, OW, out_channels] fp32 NHWC */
    const float* w_t;          /* [kh][kw][out][in] fp32: weight.permute(2, 3, 0, 1), contiguous */
    float* dx;                 /* [batch, H, W, in_channels] fp32 NHWC, OVERWRITTEN, every element */
    int64_t reserved;          /* must be 0 */
} mcgmil_conv_dgrad_args;

size_t mcgmil_conv_dgrad_args_size(void);    /* sizeof(mcgmil_conv_dgrad_args), for binding checks */

/* Host-only arithmetic of the launch: per residue class, in (r_h, r_w) row-major order, the
 * number of taps, of input pixels, and of pixel tiles (256 pixels when in_channels <= 64, else
 * 128) the grid's x axis holds for it. Entries past stride^2 are 0. Pointers are not looked at. */
int mcgmil_conv_dgrad_classes(const mcgmil_conv_dgrad_args* a, int32_t taps[4], int64_t pixels[4],
                              int64_t tiles[4]);

/* dx = the data gradient of the forward call described by a->fwd, given dy and the weight. */
int mcgmil_conv2d_dgrad_f32(const mcgmil_conv_dgrad_args* a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCGMIL_CONV_DGRAD_H_ */
