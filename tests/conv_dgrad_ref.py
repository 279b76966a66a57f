"""The residue-class decomposition of the convolution data gradient
(include/mcgmil_conv_dgrad.h), restated in torch in the dtype of its operands (float64-capable),
and the case table the data-gradient tests share.

An input pixel (ih, iw) belongs to class (r_h, r_w) = ((ih + p) mod s, (iw + p) mod s); only the
taps kh = r_h + s m_h < KH, kw = r_w + s m_w < KW reach it, from oh = (ih + p - r_h) / s - m_h and
ow likewise. `dgrad_classes` walks the classes in (r_h, r_w) row-major order and, inside one, the
taps in (kh, kw) order, as the kernel does."""
import functools

import torch
import torch.nn.functional as F

import golden_util

CASES = {
    #                     N  Cin  Cout k  s  p  H   W
    "s2_3x3_even":       (2, 64,  128, 3, 2, 1, 10, 10),   # classes of 4/2/2/1 taps, 50 pixels each
    "s2_3x3_odd":        (2, 64,  128, 3, 2, 1, 9,  11),   # classes of 40/48/50/60 pixels
    "s2_1x1":            (2, 64,  128, 1, 2, 0, 9,  10),   # three classes without taps
    "s2_7x7_c16":        (1, 16,  64,  7, 2, 3, 11, 9),    # 16/12/12/9 taps, masked channel rows
    "s2_3x3_p0_tail":    (1, 64,  64,  3, 2, 0, 8,  8),    # row and column 7 past the last window
    "s2_2x2_tail":       (1, 64,  64,  2, 2, 0, 7,  7),    # kernel = stride, row / column 6 zeros
    "s2_c64_two_tiles":  (3, 64,  128, 3, 2, 1, 20, 22),   # 330 pixels per class: two 256-pixel tiles
    "s2_c192_two_tiles": (3, 192, 64,  3, 2, 1, 20, 22),   # 128-channel tiles, the second half-masked
    "s1_3x3_odd":        (3, 64,  64,  3, 1, 1, 9,  7),    # stride 1, 189 pixels
    "s1_c48_5x5":        (2, 48,  64,  5, 1, 2, 6,  7),    # stride 1, 25 taps, Cin no multiple of 64
    "s1_wide_1x1":       (1, 256, 64,  1, 1, 0, 7,  7),    # two channel tiles, K = 64
}
TABLE = list(CASES)


def out_size(size, k, s, p):
    return (size + 2 * p - k) // s + 1


def dgrad_classes(dy, w, stride, pad, x_shape):
    """(dx, [(taps, pixels) per class]) of F.conv2d(x, w, None, stride, pad) given dy. dy
    [N, Cout, OH, OW], w [Cout, Cin, KH, KW], x_shape (N, Cin, H, W), NCHW. dx starts as NaN, so
    an element no class writes stays NaN."""
    N, Cin, H, W = x_shape
    Cout, _, KH, KW = w.shape
    OH, OW = dy.shape[2:]
    s, p = stride, pad
    dx = torch.full((N, Cin, H, W), float("nan"), dtype=dy.dtype)
    classes = []
    for rh in range(s):
        for rw in range(s):
            ihs = torch.tensor([i for i in range(H) if (i + p) % s == rh], dtype=torch.long)
            iws = torch.tensor([i for i in range(W) if (i + p) % s == rw], dtype=torch.long)
            taps = [(kh, kw) for kh in range(rh, KH, s) for kw in range(rw, KW, s)]
            classes.append((len(taps), N * len(ihs) * len(iws)))
            if len(ihs) == 0 or len(iws) == 0:
                continue
            acc = torch.zeros(N, Cin, len(ihs), len(iws), dtype=dy.dtype)
            for kh, kw in taps:
                oh = (ihs + p - rh) // s - (kh - rh) // s
                ow = (iws + p - rw) // s - (kw - rw) // s
                okh, okw = (oh >= 0) & (oh < OH), (ow >= 0) & (ow < OW)
                piece = dy[:, :, oh.clamp(0, OH - 1)][:, :, :, ow.clamp(0, OW - 1)]
                piece = piece * (okh.view(-1, 1) & okw.view(1, -1)).to(dy.dtype)
                acc += torch.einsum("nohw,oi->nihw", piece, w[:, :, kh, kw])
            dx[:, :, ihs.view(-1, 1), iws.view(1, -1)] = acc
    return dx, classes


class Case:
    """Inputs of a case and its float64 / fp32 CPU autograd gradients (computed once)."""

    def __init__(self, name):
        self.name = name
        N, Cin, Cout, k, s, p, H, W = CASES[name]
        self.stride, self.pad = s, p
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        self.x = torch.randn(N, Cin, H, W, generator=gen)
        self.w = torch.randn(Cout, Cin, k, k, generator=gen) / (Cin * k * k) ** 0.5
        self.dy = torch.randn(N, Cout, out_size(H, k, s, p), out_size(W, k, s, p), generator=gen)
        self.dx64, self.dw64 = self._cpu(torch.float64)
        dx32, dw32 = self._cpu(torch.float32)
        self.bound_dx = max(10.0 * golden_util.nrel(dx32.numpy(), self.dx64.numpy()), 1e-6)
        self.bound_dw = max(10.0 * golden_util.nrel(dw32.numpy(), self.dw64.numpy()), 1e-6)

    def _cpu(self, dt):
        x = self.x.to(dt).clone().requires_grad_()
        w = self.w.to(dt).clone().requires_grad_()
        F.conv2d(x, w, None, self.stride, self.pad).backward(self.dy.to(dt))
        return x.grad, w.grad

    def check(self, what, got, bound=None):
        want = self.dw64 if what == "dw" else self.dx64
        bound = bound or (self.bound_dw if what == "dw" else self.bound_dx)
        err = golden_util.nrel(got.detach().cpu().numpy(), want.numpy())
        print(f"{self.name} {what}: {err:.2e} / {bound:.2e}")
        assert tuple(got.shape) == tuple(want.shape)
        assert err <= bound, (self.name, what, err, bound)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
