"""CPU references of the bf16x3 convolution backward (include/mcgmil_conv_grad_x3.h,
features.conv2d_f32x3_wgrad / conv2d_f32x3_dgrad) that the host and GPU tests share: the case
table, the three-term emulation of both gradients with fp64 sums, the fp64 gradients of the unsplit
operands, the magnitudes the split's bound scales with, and a single hi * hi product.

The inputs are unrounded fp32 draws (randn + 0.25 for x, randn for dY, randn / sqrt(fan-in) for the
weight): inputs rounded to bf16 would make every lo term zero and test nothing."""
import functools

import torch
import torch.nn.functional as F

from conv32x3_ref import HI_ONLY_RATIO, SPLIT_BOUND, split  # noqa: F401  (re-exported to the tests)

G = 2048        # MCGMIL_WGRAD_GRANULE_PIXELS (include/mcgmil_conv_grad.h); the tests check it against _lib

CASES = {
    #                 N  Cin  Cout k  s  p  H  W
    "c64_3x3_odd":   (3, 64,  64,  3, 1, 1, 9, 7),      # 189 pixels, no multiple of a K step; the 64 x 256 tile
    "s2_3x3_odd":    (2, 64,  128, 3, 2, 1, 9, 11),     # stride 2, rows and columns past the last window
    "s2_1x1":        (2, 64,  128, 1, 2, 0, 9, 10),     # 64 columns: idle waves of the 128 x 128 tile
    "wide_in_1x1":   (1, 256, 64,  1, 1, 0, 7, 7),      # wide input channels
    "c32_5x5":       (2, 32,  64,  5, 1, 2, 6, 7),      # the domain's minimum Cin; dgrad pads 32 -> 64 filters
    "c192_3x3":      (1, 128, 192, 3, 1, 0, 5, 5),      # Cout no multiple of 128
    "one_pixel":     (1, 64,  64,  3, 1, 1, 1, 1),      # a single output pixel
    # batch * OH * OW = 2 G + G / 2 + 5: three granules, the last one ragged
    "granules":      (1, 32,  64,  3, 1, 1, 1, 2 * G + G // 2 + 5),
}
NAMES = list(CASES)


def wgrad(dy: torch.Tensor, x: torch.Tensor, k: int, stride: int, pad: int, dtype=torch.float64) -> torch.Tensor:
    """dW of F.conv2d(x, W, stride, pad) given dY, by CPU autograd in `dtype`."""
    w = torch.zeros(dy.shape[1], x.shape[1], k, k, dtype=dtype, requires_grad=True)
    F.conv2d(x.to(dtype), w, None, stride, pad).backward(dy.to(dtype))
    return w.grad


def dgrad(dy: torch.Tensor, w: torch.Tensor, x_shape, stride: int, pad: int, dtype=torch.float64) -> torch.Tensor:
    """dX of F.conv2d(x, w, stride, pad) given dY, by CPU autograd in `dtype`."""
    x = torch.zeros(tuple(x_shape), dtype=dtype, requires_grad=True)
    F.conv2d(x, w.to(dtype), None, stride, pad).backward(dy.to(dtype))
    return x.grad


def nrel(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max|got - ref| / max|ref|, the project's error of a tensor (golden_util.nrel)."""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


class Case:
    """Inputs of a case and its references, computed once and left unchanged."""

    def __init__(self, name: str):
        self.name = name
        N, Cin, Cout, k, s, p, H, W = CASES[name]
        self.k, self.stride, self.pad = k, s, p
        gen = torch.Generator().manual_seed(7000 + NAMES.index(name))
        self.x = torch.randn(N, Cin, H, W, generator=gen) + 0.25
        oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        self.dy = torch.randn(N, Cout, oh, ow, generator=gen)
        self.w = torch.randn(Cout, Cin, k, k, generator=gen) / (Cin * k * k) ** 0.5
        g = lambda a, b: wgrad(a, b, k, s, p)                                    # noqa: E731
        (xh, xl), (dh, dl) = split(self.x), split(self.dy)
        self.dw64 = g(self.dy, self.x)                     # fp64 of the unsplit operands
        self.dw_emu = g(dh, xh) + g(dh, xl) + g(dl, xh)    # dy_hi x_hi + dy_hi x_lo + dy_lo x_hi, fp64 sums
        self.dw_hi = g(dh, xh)                             # a single bf16 product
        self.dw_mag = g(self.dy.abs(), self.x.abs())
        # the project's yardstick for a changed summation order: 10 x fp32 CPU autograd's own error
        self.bound_dw = max(10.0 * nrel(wgrad(self.dy, self.x, k, s, p, torch.float32), self.dw64), 1e-6)

    @functools.cached_property
    def dx(self):
        """(fp64 dX, emulation, magnitude) for the data gradient (the stride-1 cases use it)."""
        d = lambda a, b: dgrad(a, b, self.x.shape, self.stride, self.pad)        # noqa: E731
        (wh, wl), (dh, dl) = split(self.w), split(self.dy)
        return d(self.dy, self.w), d(dh, wh) + d(dl, wh) + d(dh, wl), d(self.dy.abs(), self.w.abs())


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return Case(name)
