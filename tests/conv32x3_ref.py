"""CPU emulation of the bf16x3 convolution (mcgmil_conv2d_f32x3, include/mcgmil_features.h): the
split of an fp32 value into two bf16 terms and the three-term convolution with fp64 sums, plus
the shapes and bounds the host and GPU tests share."""
import torch
import torch.nn.functional as F

# (N, Cin, H, W, Cout, k, stride, pad): the smallest shapes at which each mechanism of the kernel
# can fail
SHAPES = [
    (7, 32, 3, 5, 64, 1, 1, 0),         # one K step; 105 pixels, less than one tile
    (2, 64, 14, 14, 64, 3, 1, 1),       # the 64-channel tile
    (2, 64, 14, 14, 128, 3, 2, 1),      # stride 2
    (2, 64, 14, 14, 128, 1, 2, 0),
    (5, 64, 9, 11, 192, 3, 1, 1),       # Cout = 128 + 64, 495 pixels
    (1, 96, 8, 13, 128, 7, 3, 3),       # three channel chunks per tap, 7x7 window, stride 3
    (2, 512, 7, 7, 512, 3, 1, 1),       # 144 K steps
    (2, 2048, 5, 3, 512, 1, 1, 0),      # 2,048 channels on either side
    (2, 512, 5, 3, 2048, 1, 1, 0),
    (3, 32, 9, 7, 64, (1, 3), 1, 1),    # non-square windows
    (3, 32, 9, 7, 64, (3, 1), 1, 1),
]

# |x - hi - lo| <= 2^-16 |x| per operand and the dropped lo * lo <= 2^-16 |x w|
SPLIT_BOUND = 3 * 2.0 ** -16
# the emulation's nrel must be at most this fraction of a single hi * hi product's
HI_ONLY_RATIO = 1 / 32


def shape_id(s) -> str:
    return "x".join(str(v).replace(" ", "") for v in s)


def kernel_hw(k):
    return (k, k) if isinstance(k, int) else tuple(k)


def split(v: torch.Tensor):
    """(hi, lo) as fp32 tensors: hi = bf16_rne(v), lo = bf16_rne(v - hi); v fp32."""
    assert v.dtype == torch.float32
    hi = v.bfloat16().float()
    lo = (v - hi).bfloat16().float()
    return hi, lo


def conv64(x: torch.Tensor, w: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    return F.conv2d(x.double(), w.double(), stride=stride, padding=pad)


def conv_x3(x: torch.Tensor, w: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    """hi_w * hi_x + hi_w * lo_x + lo_w * hi_x summed in fp64 (x NCHW fp32, w [out, in, kh, kw] fp32)."""
    xh, xl = split(x)
    wh, wl = split(w)
    return conv64(xh, wh, stride, pad) + conv64(xl, wh, stride, pad) + conv64(xh, wl, stride, pad)


def conv_hi(x: torch.Tensor, w: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    """A single bf16 product, hi_w * hi_x, summed in fp64."""
    return conv64(split(x)[0], split(w)[0], stride, pad)


def nrel(a: torch.Tensor, ref: torch.Tensor) -> float:
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def make_case(shape, seed: int = 0):
    """(x NCHW fp32, w fp32, stride, pad) of a shape: activations like a post-ReLU BatchNorm output
    with an offset, weights with Kaiming scale."""
    N, Cin, H, W, Cout, k, stride, pad = shape
    kh, kw = kernel_hw(k)
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(N, Cin, H, W, generator=g) + 0.25
    w = torch.randn(Cout, Cin, kh, kw, generator=g) * (2.0 / (Cin * kh * kw)) ** 0.5
    return x, w, stride, pad
