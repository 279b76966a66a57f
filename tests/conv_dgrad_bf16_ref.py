"""The case table and references the bf16 direct data-gradient tests share
(include/mcgmil_conv_dgrad_bf16.h). A helper module, not a test.

Inputs are drawn in fp32 from a seeded generator and rounded to bf16 first; every reference is
computed from the rounded values, so what is measured is the kernel, not the rounding of its inputs.
References: float64 and fp32 CPU autograd of F.conv2d. The residue-class restatement is
conv_dgrad_ref.dgrad_classes.

Bound of the data gradient, which is rounded to bf16 once: elementwise
|d| <= 2^-7 |ref| + B max|ref| with B = max(10 x nrel(fp32 CPU dx, float64 dx), 1e-6) (2^-8 is
bf16's unit roundoff, doubled for rounding an fp32 sum that itself carries error B; x10 is the
project's factor for a changed summation order). Bound of the weight gradient (fp32):
nrel <= max(10 x nrel(fp32 CPU dw, float64 dw), 1e-6). Every check prints measured / bound before
it asserts."""
import functools

import torch
import torch.nn.functional as F

import golden_util
from conv_dgrad_ref import dgrad_classes, out_size  # noqa: F401  (re-exported for the tests)

BF = torch.bfloat16
CL = torch.channels_last

CASES = {
    #                     N  Cin  Cout k       s  p  H   W
    "s2_3x3_even":       (2, 64,  128, 3,      2, 1, 10, 10),   # classes of 4/2/2/1 taps
    "s2_3x3_odd":        (2, 64,  128, 3,      2, 1, 9,  11),   # unequal class sizes
    "s2_1x1":            (2, 64,  128, 1,      2, 0, 9,  10),   # three classes without taps
    "s2_3x3_p0_tail":    (1, 64,  64,  3,      2, 0, 8,  8),    # row and column past the last window
    "s2_2x2_tail":       (1, 64,  64,  2,      2, 0, 7,  7),    # kernel equal to stride
    "s2_7x7":            (1, 64,  64,  7,      2, 3, 11, 9),    # 16/12/12/9 taps
    "s2_3x5":            (1, 64,  64,  (3, 5), 2, 1, 9,  9),    # non-square kernel
    "s2_k256":           (1, 128, 256, 3,      2, 1, 6,  6),    # eight K steps per tap, wide tile
    "s2_c64_two_tiles":  (3, 64,  128, 3,      2, 1, 20, 22),   # 330 pixels per class: two 256-pixel tiles
    "s2_c192_two_tiles": (3, 192, 64,  3,      2, 1, 20, 22),   # three 128-pixel tiles, half-masked channel tile
    "s1_3x3_odd":        (3, 64,  64,  3,      1, 1, 9,  7),    # stride 1
    "s1_wide_1x1":       (1, 256, 64,  1,      1, 0, 7,  7),    # stride 1, wide input
    "s1_3x5":            (2, 64,  64,  (3, 5), 1, 1, 6,  7),    # stride 1, non-square: the flipped forward refuses it
}
TABLE = list(CASES)


def kernel_hw(k):
    return (k, k) if isinstance(k, int) else tuple(k)


def round_bf16(t):
    return t.to(BF).float()


class Case:
    """bf16-rounded inputs of a case and its float64 / fp32 CPU autograd gradients (computed once;
    never modified)."""

    def __init__(self, name):
        self.name = name
        N, Cin, Cout, k, s, p, H, W = CASES[name]
        kh, kw = kernel_hw(k)
        self.stride, self.pad = s, p
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        self.x = round_bf16(torch.randn(N, Cin, H, W, generator=gen))
        self.w = round_bf16(torch.randn(Cout, Cin, kh, kw, generator=gen) / (Cin * kh * kw) ** 0.5)
        self.dy = round_bf16(torch.randn(N, Cout, out_size(H, kh, s, p), out_size(W, kw, s, p), generator=gen))
        self.dx64, self.dw64 = self._cpu(torch.float64)
        dx32, dw32 = self._cpu(torch.float32)
        self.bound_dx = max(10.0 * golden_util.nrel(dx32.numpy(), self.dx64.numpy()), 1e-6)
        self.bound_dw = max(10.0 * golden_util.nrel(dw32.numpy(), self.dw64.numpy()), 1e-6)

    def _cpu(self, dt):
        x = self.x.to(dt).clone().requires_grad_()
        w = self.w.to(dt).clone().requires_grad_()
        F.conv2d(x, w, None, self.stride, self.pad).backward(self.dy.to(dt))
        return x.grad, w.grad

    def conv(self, dev, dtype=torch.float32):
        from mcgmil import features
        return features._ConvShim(self.w.to(dev, dtype), self.stride, self.pad)

    def gpu(self, dev):
        return (self.x.to(dev, BF).contiguous(memory_format=CL), self.dy.to(dev, BF).contiguous(memory_format=CL))

    def check_dw(self, got):
        err = golden_util.nrel(got.detach().float().cpu().numpy(), self.dw64.numpy())
        print(f"{self.name} dw: {err:.2e} / {self.bound_dw:.2e}")
        assert tuple(got.shape) == tuple(self.dw64.shape)
        assert err <= self.bound_dw, (self.name, err, self.bound_dw)

    def check_dx(self, got):
        assert tuple(got.shape) == tuple(self.dx64.shape) and got.dtype == BF
        check_dx(self.name, got, self.dx64, self.bound_dx)


def check_dx(name, got, ref, bound):
    """|got - ref| <= 2^-7 |ref| + bound max|ref|, elementwise."""
    allowed = 2.0 ** -7 * ref.abs() + bound * ref.abs().max()
    excess = ((got.detach().cpu().double() - ref).abs() / allowed).max().item()
    print(f"{name} dx: max |d| / (2^-7 |ref| + {bound:.2e} max|ref|) = {excess:.3f} / 1")
    assert excess <= 1.0, (name, excess)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
