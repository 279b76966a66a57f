"""GPU parity of the implicit-GEMM backbone convolution (include/mcgmil_features.h,
mcgmil_conv2d) -- the reference's torchvision BasicBlock / Bottleneck convolutions
(model.py:166-177) as torch.autocast runs them in bf16 on every instance of a bag
(infer.py:191 -> model.py:275-277).

Reference: an fp64 convolution of the same bf16 input and bf16-rounded weight (what autocast
feeds MIOpen). The kernel accumulates in fp32 and rounds once to bf16, so
|y - ref| <= 2^-8 |ref| (half an ulp) + 1e-5 * conv(|x|, |w|) (fp32 summation of up to 4608
terms, a bound far above its typical size).
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (N, Cin, H, W, Cout, k, stride, pad): ResNet-18's block convolutions at small batch, then odd
# sizes (pixel count not a multiple of the 128-pixel tile, 192 output channels -> 64-wide tiles,
# 5x5 / 7x7 windows, stride 3)
SHAPES = [
    (3, 64, 56, 56, 64, 3, 1, 1),
    (2, 64, 56, 56, 128, 3, 2, 1),
    (2, 64, 56, 56, 128, 1, 2, 0),
    (3, 128, 28, 28, 128, 3, 1, 1),
    (2, 256, 14, 14, 512, 3, 2, 1),
    (2, 512, 7, 7, 512, 3, 1, 1),
    (5, 64, 9, 11, 192, 3, 1, 1),
    (2, 128, 10, 10, 64, 5, 1, 2),
    (1, 64, 8, 13, 64, 7, 3, 3),
    # 3x3 / 64 -> 64 halo-tile kernel: tiles spanning several small images, odd widths, a tile
    # crossing image boundaries, and a width whose patch only just fits (62) or does not (70)
    (9, 64, 8, 6, 64, 3, 1, 1),
    (3, 64, 30, 17, 64, 3, 1, 1),
    (2, 64, 20, 62, 64, 3, 1, 1),
    (1, 64, 5, 70, 64, 3, 1, 1),
    # the row-ring 64 -> 64 kernel (conv3x3c64_ring_kernel, W + 2 <= 64 and two tiles' rows <= 16):
    # more than 256 tiles, so a workgroup walks several tiles through the ring, an image boundary
    # every ~4 tiles (20 x 50), and config 5's 56 x 56
    (48, 64, 56, 56, 64, 3, 1, 1),
    (120, 64, 20, 50, 64, 3, 1, 1),
    # 3x3 / stride 1 halo kernel with streamed weights (Cin >= 128): many small images per tile,
    # 3 input-channel chunks, 2 channel tiles, and a row too wide for the patch (generic kernel)
    (4, 128, 25, 20, 128, 3, 1, 1),
    (2, 192, 17, 30, 256, 3, 1, 1),
    (1, 128, 6, 80, 128, 3, 1, 1),
    # 1x1 / stride 2: from 64 input channels the streaming kernel (conv1x1_kernel; odd pixel
    # counts, 192 output channels = 6 waves per pixel stream); from 128 / 256 channels (layer 3's and
    # 4's shapes at odd sizes, a single image) the LDS-DMA tiles (make_plan sends only Cin == 64 to
    # the streaming kernel)
    (3, 128, 13, 11, 256, 1, 2, 0),
    (2, 64, 9, 7, 192, 1, 2, 0),
    (1, 256, 14, 14, 512, 1, 2, 0),
    # 1x1 / stride 1 from 64 channels: one K step per tile (KT == 1), so conv_dma_kernel's stream
    # changes tile at every step (setup(), the issue cursor and the epilogue all fire each step).
    # 134,848 pixels = 527 tiles of 256, 2-3 per workgroup row on 256 CUs, on the 256 x 64, the
    # 256 x 128 and the 256 x 256 tiles (the last one ResNet-50's layer-1 downsample)
    (43, 64, 56, 56, 64, 1, 1, 0),
    (43, 64, 56, 56, 128, 1, 1, 0),
    (43, 64, 56, 56, 256, 1, 1, 0),
    # ResNet-50's bottleneck 1x1 / stride 1 shapes (Cin and Cout up to 2048) at ragged pixel counts
    (3, 256, 9, 7, 64, 1, 1, 0),
    (3, 256, 9, 7, 128, 1, 1, 0),
    (2, 128, 9, 7, 512, 1, 1, 0),
    (2, 512, 9, 7, 128, 1, 1, 0),
    (2, 256, 7, 5, 1024, 1, 1, 0),
    (2, 1024, 7, 5, 256, 1, 1, 0),
    (2, 512, 5, 3, 2048, 1, 1, 0),
    (2, 2048, 5, 3, 512, 1, 1, 0),
    # its stride-2 shapes: the downsamples of layers 3 and 4 and the 3x3 of each stage's first block
    (2, 512, 9, 7, 1024, 1, 2, 0),
    (2, 1024, 6, 5, 2048, 1, 2, 0),
    (2, 128, 13, 11, 128, 3, 2, 1),
    (2, 256, 9, 7, 256, 3, 2, 1),
    (2, 512, 7, 5, 512, 3, 2, 1),
    # 8 channel tiles of 256 with more pixel tiles (35) than workgroup rows (32 on 256 CUs); 8 K
    # steps, too few for a K split of the 3 tiles left
    (180, 512, 7, 7, 2048, 1, 1, 0),
]


def _layer(cin, cout, k, s, p, dev, seed):
    """k: the window, an int or (kh, kw)."""
    kh, kw = (k, k) if isinstance(k, int) else k
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(cin, cout, k, s, p, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5)
    return conv.to(dev).eval()


def _planned(conv, x, flags=0):
    """(statistics rows, K-split workspace bytes) of the launch plan, as the ABI reports them."""
    import ctypes
    from mcgmil import _lib
    from mcgmil.features import _conv_args
    a = _conv_args(conv, x)
    a.flags = flags
    parts, nb = ctypes.c_int32(), ctypes.c_size_t()
    assert _lib.load().mcgmil_conv_stats_parts(ctypes.byref(a), ctypes.byref(parts)) == 0
    assert _lib.load().mcgmil_conv_workspace_size(ctypes.byref(a), ctypes.byref(nb)) == 0
    return parts.value, nb.value


def _expected_plan(conv, x, cus, policy="auto"):
    """What the tile policy is documented to pick (mcgmil_features.h), as far as the
    ABI shows it: (256 x 256 or 512 x 128 tiles?, K split of their last round?). The 256 x 256
    tiles take every layer with Cout % 256 == 0 (under `big512` the 512 x 128 tiles the other
    layers with Cout % 128 == 0) except, under the auto policy, the streaming 1x1 / stride 2 from
    64 channels and, unless `nohalo`, the 3x3 / stride 1 halo kernel with streamed weights
    (Cin >= 128, OW >= 20, a patch of <= 480 pixels); `small` keeps the 256 x 128 tiles. The R
    256 x 256 tiles left after F whole rounds over gb workgroup rows are cut into
    P = min(gb // R, 4) K ranges when F >= 1, P >= 2 and there are >= 4 P K steps."""
    N, Cin, H, W = x.shape
    Cout, (kh, kw), s, p = conv.out_channels, conv.kernel_size, conv.stride[0], conv.padding[0]
    oh, ow = (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1
    wide = Cout % 256 == 0 or (policy == "big512" and Cout % 128 == 0)
    if policy == "small" or not wide:
        return False, False
    if policy == "auto" and (kh, kw, s, p, Cin) == (1, 1, 2, 0, 64):
        return False, False
    if policy != "nohalo" and (kh, kw, s, p) == (3, 3, 1, 1) and Cin >= 128 and ow >= 20:
        rows = (255 + ow - 1) // ow + 1
        imgs = (255 + oh * ow - 1) // (oh * ow) + 1
        if (rows + 2 + 2 * (imgs - 1)) * (W + 2) <= 480:
            return False, False
    if Cout % 256:
        return True, False            # 512 x 128 tiles: no K split
    tiles_m, tiles_n = (N * oh * ow + 255) // 256, Cout // 256
    gb = min(max(cus // tiles_n, 1), tiles_m)
    F_, R = tiles_m // gb, tiles_m % gb
    P = min(gb // R, 4) if R else 0
    return True, F_ >= 1 and P >= 2 and kh * kw * (Cin // 64) >= 4 * P


def _assert_plan(conv, x, policy="auto"):
    """The shape runs the kernel its comment names: no statistics rows exactly on the 256 x 256 and
    512 x 128 tiles, a workspace exactly where the last round of 256 x 256 tiles is split."""
    from mcgmil import _lib
    cus = torch.cuda.get_device_properties(x.device).multi_processor_count
    big, split = _expected_plan(conv, x, cus, policy)
    parts, nb = _planned(conv, x, _lib.CONV_TILE_FLAGS[policy])
    assert (parts == 0) == big, (policy, parts, big)
    assert (nb > 0) == split, (policy, nb, split)


@pytest.mark.parametrize("shape", SHAPES)
def test_conv2d_matches_fp64(cuda, shape):
    from mcgmil.features import conv2d, conv_fusable
    N, Cin, H, W, Cout, k, s, p = shape
    conv = _layer(Cin, Cout, k, s, p, cuda, Cin + Cout + k)
    g = torch.Generator(device=cuda).manual_seed(N * H + W)
    x = torch.randn(N, Cin, H, W, device=cuda, generator=g).relu_().bfloat16()
    x = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert conv_fusable(conv, x)
        y = conv2d(conv, x)
    _assert_plan(conv, x)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    wb = conv.weight.detach().bfloat16().double()
    with torch.no_grad():
        ref = F.conv2d(x.double(), wb, None, s, p)
        mag = F.conv2d(x.double().abs(), wb.abs(), None, s, p)
    assert y.shape == ref.shape
    err = (y.double() - ref).abs()
    assert torch.all(err <= 2.0 ** -8 * ref.abs() + 1e-5 * mag), float((err / (ref.abs() + 1e-30)).max())


# kernels with kernel_h != kernel_w (conv_fusable admits them; ConvGeom keeps KH and KW apart): the
# tap order kt = (kh KW + kw) Cin / 64 + cc, the tap mask's bit kh KW + kw and the packed weight's
# [Cout, KH, KW, Cin] must agree. One padding for both axes, so with pad 1 a 1 x 3 window also reads
# the rows of padding above and below the image. 495-605 pixels: 2-3 tiles, the last one ragged.
NONSQUARE = [(kk, p, c) for kk in ((1, 3), (3, 1), (1, 7)) for p in (0, 1)
             for c in ((64, 64), (64, 192), (128, 128))]


@pytest.mark.parametrize("kk,p,chan", NONSQUARE)
def test_conv2d_nonsquare_window(cuda, kk, p, chan):
    from mcgmil.features import conv2d, conv_fusable
    Cin, Cout = chan
    conv = _layer(Cin, Cout, kk, 1, p, cuda, Cin + Cout + 10 * kk[0] + kk[1])
    g = torch.Generator(device=cuda).manual_seed(Cout + kk[1] + p)
    x = torch.randn(5, Cin, 9, 11, device=cuda, generator=g).relu_().bfloat16()
    x = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert conv_fusable(conv, x)
        y = conv2d(conv, x)
        assert torch.equal(conv2d(conv, x), y)
    _assert_plan(conv, x)
    wb = conv.weight.detach().bfloat16().double()
    with torch.no_grad():
        ref = F.conv2d(x.double(), wb, None, 1, p)
        mag = F.conv2d(x.double().abs(), wb.abs(), None, 1, p)
    assert y.shape == ref.shape
    err = (y.double() - ref).abs()
    assert torch.all(err <= 2.0 ** -8 * ref.abs() + 1e-5 * mag), float((err / (ref.abs() + 1e-30)).max())


TILE_SHAPES = [(3, 64, 56, 56, 64, 3, 1, 1), (3, 128, 28, 28, 128, 3, 1, 1), (2, 256, 14, 14, 512, 3, 2, 1),
               (2, 64, 9, 7, 192, 1, 2, 0),
               # one K step per tile, 2-3 tiles per workgroup row; under `small` the 256-channel one
               # takes the 256 x 128 tiles
               (43, 64, 56, 56, 64, 1, 1, 0), (43, 64, 56, 56, 128, 1, 1, 0), (43, 64, 56, 56, 256, 1, 1, 0)]


@pytest.mark.parametrize("shape", TILE_SHAPES)
def test_conv2d_tile_policy_flags(cuda, shape):
    """mcgmil_conv_args.flags (MCGMIL_CONV_TILE_*: auto, no halo / streaming kernels, 256 x 128 for
    256 x 256 tiles, 512 x 128 on 128-channel layers) selects the kernel without the environment;
    every policy is within the fp64 bound and repeatable."""
    from mcgmil import _lib
    from mcgmil.features import conv2d
    N, Cin, H, W, Cout, k, s, p = shape
    conv = _layer(Cin, Cout, k, s, p, cuda, Cin + 2 * Cout + k)
    g = torch.Generator(device=cuda).manual_seed(N * W + H)
    x = torch.randn(N, Cin, H, W, device=cuda, generator=g).relu_().bfloat16()
    x = x.contiguous(memory_format=torch.channels_last)
    wb = conv.weight.detach().bfloat16().double()
    with torch.no_grad():
        ref = F.conv2d(x.double(), wb, None, s, p)
        mag = F.conv2d(x.double().abs(), wb.abs(), None, s, p)
    for name, flag in _lib.CONV_TILE_FLAGS.items():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            y = conv2d(conv, x, flags=flag)
            y2 = conv2d(conv, x, flags=flag)
        assert torch.equal(y, y2), name
        err = (y.double() - ref).abs()
        assert torch.all(err <= 2.0 ** -8 * ref.abs() + 1e-5 * mag), name
        _assert_plan(conv, x, name)


# 256 x 256 tiles with a short last round (on 256 CUs: 14 x 14 -> 256, 307 tiles over 256 rows, 51
# left in 4 K ranges; 7 x 7 x 512 and its stride-2 producer, 134 tiles over 128 rows, 6 left in 4)
SPLIT_SHAPES = [(400, 256, 14, 14, 256, 3, 1, 1), (700, 512, 7, 7, 512, 3, 1, 1), (700, 256, 14, 14, 512, 3, 2, 1)]
# ResNet-50's layer 4 on 256 CUs: a 1x1 / stride 2 window into 8 channel tiles (35 tiles over 32 rows,
# 3 left in 4 ranges of the 16 K steps: slot (tn R + q) P + pp at tn up to 7), and 1x1 / stride 1
# from 2048 channels (134 tiles over 128 rows, 6 left in 4 ranges of the 32 K steps). These two must
# split on the device the suite runs on: a skip would let them pass without the split.
SPLIT_SHAPES_R50 = [(180, 1024, 14, 14, 2048, 1, 2, 0), (700, 2048, 7, 7, 512, 1, 1, 0)]


@pytest.mark.parametrize("shape", SPLIT_SHAPES + SPLIT_SHAPES_R50)
def test_conv2d_k_split(cuda, shape, monkeypatch):
    """The K split of the last round of 256 x 256 tiles (mcgmil_conv_args.workspace): within the
    fp64 bound and repeatable; the whole tiles bitwise those of the unsplit launch
    (MCGMIL_CONV_SPLIT=0, no workspace), the split tiles at most one bf16 rounding from them."""
    import ctypes
    from mcgmil import _lib
    from mcgmil.features import _conv_args, conv2d
    N, Cin, H, W, Cout, k, s, p = shape
    conv = _layer(Cin, Cout, k, s, p, cuda, Cin + 3 * Cout + k)
    g = torch.Generator(device=cuda).manual_seed(N + H)
    x = torch.randn(N, Cin, H, W, device=cuda, generator=g).relu_().bfloat16()
    x = x.contiguous(memory_format=torch.channels_last)
    nb = ctypes.c_size_t()
    assert _lib.load().mcgmil_conv_workspace_size(ctypes.byref(_conv_args(conv, x)), ctypes.byref(nb)) == 0
    if shape in SPLIT_SHAPES_R50:
        assert nb.value > 0
        _assert_plan(conv, x)
    if nb.value == 0:
        pytest.skip("no K split for this shape at this GPU's CU count")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        monkeypatch.setenv("MCGMIL_CONV_SPLIT", "0")
        y0 = conv2d(conv, x)
        monkeypatch.setenv("MCGMIL_CONV_SPLIT", "1")
        y1 = conv2d(conv, x)
        y2 = conv2d(conv, x)
    assert torch.equal(y1, y2)
    wb = conv.weight.detach().bfloat16().double()
    with torch.no_grad():
        ref = F.conv2d(x.double(), wb, None, s, p)
        mag = F.conv2d(x.double().abs(), wb.abs(), None, s, p)
    err = (y1.double() - ref).abs()
    assert torch.all(err <= 2.0 ** -8 * ref.abs() + 1e-5 * mag)
    # rows (pixels) of the whole tiles: F tiles per workgroup row, tiles_n * rows <= CUs
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    tiles_m, tiles_n = (y0.numel() // Cout + 255) // 256, Cout // 256
    rows = min(max(cus // tiles_n, 1), tiles_m)
    whole = (tiles_m // rows) * rows * 256
    r0 = y0.permute(0, 2, 3, 1).reshape(-1, Cout)
    r1 = y1.permute(0, 2, 3, 1).reshape(-1, Cout)
    assert whole < r0.shape[0]
    assert torch.equal(r0[:whole], r1[:whole])
    a, b = r0[whole:].double(), r1[whole:].double()
    m = mag.permute(0, 2, 3, 1).reshape(-1, Cout)[whole:]
    assert torch.all((a - b).abs() <= 2.0 ** -7 * torch.maximum(a.abs(), b.abs()) + 2e-5 * m)


RING_SHAPES = [(3, 64, 56, 56, 64), (48, 64, 56, 56, 64), (120, 64, 20, 50, 64), (2, 64, 20, 62, 64)]


@pytest.mark.parametrize("shape", RING_SHAPES)
def test_ring_kernel_bitwise_equals_generic(cuda, shape):
    """The 64 -> 64 kernels accumulate each output over the same K steps in the same order (tap-major,
    32 channels per MFMA), so the row-ring kernel (auto) is bitwise the generic LDS-DMA kernel
    (MCGMIL_CONV_TILE_NOHALO), with and without an input BatchNorm."""
    from mcgmil import _lib
    from mcgmil.features import batchnorm_act, batchnorm_coefficients, conv2d
    N, Cin, H, W, Cout = shape
    conv = _layer(Cin, Cout, 3, 1, 1, cuda, 3 * Cin + W)
    bn = _bn64(Cin, cuda, W)
    g = torch.Generator(device=cuda).manual_seed(N + H * W)
    x = (torch.randn(N, Cin, H, W, device=cuda, generator=g) * 1.5 + 0.2).bfloat16()
    x = x.contiguous(memory_format=torch.channels_last)
    nohalo = _lib.CONV_TILE_FLAGS["nohalo"]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = conv2d(conv, x)
        y_ref = conv2d(conv, x, flags=nohalo)
        ab = batchnorm_coefficients(x, bn)
        yb = conv2d(conv, x, in_ab=ab, in_relu=True)
        yb_ref = conv2d(conv, batchnorm_act(x, bn, True), flags=nohalo)
    assert torch.equal(y, y_ref)
    assert torch.equal(yb, yb_ref)


def _ring_shapes(count, seed):
    """Random 64 -> 64 shapes the row-ring kernel takes (W + 2 <= 64, two tiles' padded rows <= 16),
    with more than 256 tiles (several per workgroup) in some."""
    import random
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        W = rng.randint(20, 62)
        H = rng.randint(3, 40)
        rows = (2 * 256 - 1 + W - 1) // W + 1
        imgs = (2 * 256 - 1 + H * W - 1) // (H * W) + 1
        if rows + 2 + 2 * (imgs - 1) > 16:
            continue
        many = len(out) % 2 == 0                     # > 256 tiles: workgroups walk the ring
        N = (257 * 256) // (H * W) + 1 + rng.randint(0, 9) if many else rng.randint(1, 9)
        out.append((N, 64, H, W, 64))
    return out


@pytest.mark.parametrize("shape", _ring_shapes(8, 5))
def test_ring_kernel_random_shapes_bitwise(cuda, shape):
    """Random geometries through the row ring (ragged last tiles, image boundaries inside tiles and
    inside fragments, odd widths): bitwise the generic kernel, with and without the input BN."""
    test_ring_kernel_bitwise_equals_generic(cuda, shape)


def test_conv2d_bf16_weights_and_repack(cuda):
    """A bf16 module runs without autocast; an in-place weight update is picked up (the packed
    weight cache is keyed by the tensor version)."""
    from mcgmil.features import conv2d
    conv = _layer(64, 128, 3, 1, 1, cuda, 3).bfloat16()
    g = torch.Generator(device=cuda).manual_seed(17)
    x = torch.randn(2, 64, 12, 12, device=cuda, generator=g).bfloat16().contiguous(
        memory_format=torch.channels_last)
    with torch.no_grad():
        y1 = conv2d(conv, x)
        ref1 = F.conv2d(x.double(), conv.weight.double(), None, 1, 1)
        conv.weight.mul_(-2.0)
        y2 = conv2d(conv, x)
        y2b = conv2d(conv, x)
    assert torch.all((y1.double() - ref1).abs() <= 2.0 ** -8 * ref1.abs() + 1e-3)
    assert torch.equal(y2, y2b)
    # not bitwise -2 * y1: the MFMA's fp32 accumulation is exact under a power-of-two scale but not
    # sign-symmetric, so a sum next to a bf16 rounding tie can round the other way once negated
    # (measured: 1 element, 1 ulp, in 4 of 300 such layers; scale by +2: 0 of 300;
    # scripts/probe_conv_determinism.py). Stale weights would give y1.
    want = -2.0 * y1.float()
    assert torch.all((y2.float() - want).abs() <= 2.0 ** -7 * want.abs())


def test_conv_fusable_gates(cuda):
    """Where torch's convolution stays: CPU, NCHW, fp32 without autocast, the 3-channel stem,
    grouped / biased / dilated convolutions, autograd."""
    from mcgmil.features import conv_fusable
    conv = _layer(64, 64, 3, 1, 1, cuda, 1)
    x = torch.randn(1, 64, 8, 8, device=cuda).bfloat16().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert conv_fusable(conv, x)
            assert not conv_fusable(conv, x.contiguous())                          # NCHW
            assert not conv_fusable(conv.cpu(), x.cpu())
            conv.to(cuda)
            assert not conv_fusable(_layer(3, 64, 7, 2, 3, cuda, 2),
                                    torch.randn(1, 3, 32, 32, device=cuda).bfloat16()
                                    .contiguous(memory_format=torch.channels_last))
            assert not conv_fusable(nn.Conv2d(64, 64, 3, 1, 1, groups=2, bias=False).to(cuda), x)
            assert not conv_fusable(nn.Conv2d(64, 64, 3, 1, 1, bias=True).to(cuda), x)
            assert not conv_fusable(nn.Conv2d(64, 64, 3, 1, 2, dilation=2, bias=False).to(cuda), x)
        assert not conv_fusable(conv, x.float().contiguous(memory_format=torch.channels_last))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not conv_fusable(conv, x)                      # grad enabled, weight needs grad


def _bn64(C, dev, seed):
    from mcgmil.resnet import deactivate_batchnorm
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g) * 0.5 + 1.0)
        bn.weight[::5] *= -1.0
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    deactivate_batchnorm(bn)
    return bn.to(dev).eval()


# conv + batch-statistics BN (+ residual) + ReLU, the statistics taken from the convolution's
# epilogue: every kernel (halo 3x3 64->64, 256 x 64 and 256 x 128 tiles), ragged pixel counts,
# several channel tiles, and an input offset that makes mean >> std for the statistics
STATS_SHAPES = [
    (3, 64, 56, 56, 64, 3, 1, 1, 0.0),
    (40, 64, 56, 56, 64, 3, 1, 1, 1.0),
    (120, 64, 20, 50, 64, 3, 1, 1, 0.0),
    (9, 64, 8, 6, 64, 3, 1, 1, 0.0),
    (2, 64, 28, 28, 128, 3, 2, 1, 0.0),
    (3, 128, 13, 11, 256, 3, 1, 1, 0.0),
    (2, 256, 7, 7, 512, 1, 2, 0, 0.0),
    (5, 64, 9, 11, 192, 3, 1, 1, 0.0),
    (3, 64, 20, 20, 64, 3, 1, 1, 4.0),
    (2, 128, 10, 10, 128, 3, 1, 1, 4.0),
    (4, 128, 25, 20, 128, 3, 1, 1, 0.0),
    (2, 192, 17, 30, 256, 3, 1, 1, 2.0),
    (3, 128, 13, 11, 256, 1, 2, 0, 2.0),
    (2, 64, 28, 28, 128, 1, 2, 0, 0.0),
    # streaming 1x1 kernel with more pixel streams than fragments: M = 9 pixels (1 fragment), 6
    # channel blocks, the stream count rounded up to 2 -- an empty stream whose statistics rows have
    # count 0 and must merge away in the BN finalize
    (1, 64, 6, 6, 192, 1, 2, 0, 0.0),
    # ResNet-50's bottleneck shapes: 1x1 / stride 1 on the 256 x 64 tiles (4 K steps, a single ragged
    # tile, with and without an input offset), one K step per tile with 2-3 tiles per statistics
    # row on the 256 x 128 tiles, the 256 x 256 tiles that emit no statistics (the BN then makes
    # its own pass, at C = 2048), and a 3x3 / stride 2
    (3, 256, 9, 7, 64, 1, 1, 0, 0.0),
    (3, 256, 9, 7, 64, 1, 1, 0, 2.0),
    (43, 64, 56, 56, 128, 1, 1, 0, 0.0),
    (2, 512, 5, 3, 2048, 1, 1, 0, 0.0),
    (2, 128, 13, 11, 128, 3, 2, 1, 0.0),
]


@pytest.mark.parametrize("shape", STATS_SHAPES)
@pytest.mark.parametrize("residual", [False, True])
def test_conv_bn_act_fused_statistics(cuda, shape, residual):
    """|y - ref| <= |a_c| (2^-8 |conv| + 1e-5 conv(|x|,|w|)) + 2^-8 |y| + 2e-3 |a_c| std_c: the
    convolution's rounding, the fused BN's rounding, and the statistics of rounded values."""
    from mcgmil.features import conv2d, conv_bn_act
    N, Cin, H, W, Cout, k, s, p, off = shape
    conv = _layer(Cin, Cout, k, s, p, cuda, Cin * 3 + Cout + k)
    bn = _bn64(Cout, cuda, Cout + k)
    g = torch.Generator(device=cuda).manual_seed(N * H + W + Cout)
    x = (torch.randn(N, Cin, H, W, device=cuda, generator=g).relu_() + off).bfloat16()
    x = x.contiguous(memory_format=torch.channels_last)
    oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    idt = torch.randn(N, Cout, oh, ow, device=cuda, generator=g).bfloat16().contiguous(
        memory_format=torch.channels_last) if residual else None
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = conv_bn_act(conv, bn, x, True, idt)
        _, part = conv2d(conv, x, stats=True)
    _assert_plan(conv, x)
    if part is not None:            # the 256 x 256 tiles (Cout % 256 == 0) emit none
        assert part.shape[1:] == (3, Cout)
        assert float(part[:, 0, :].sum(0).min()) == N * oh * ow == float(part[:, 0, :].sum(0).max())
    else:
        assert Cout % 256 == 0
    wb = conv.weight.detach().bfloat16().double()
    with torch.no_grad():
        c = F.conv2d(x.double(), wb, None, s, p)
        mag = F.conv2d(x.double().abs(), wb.abs(), None, s, p)
    mean, var = c.mean(dim=(0, 2, 3)), c.var(dim=(0, 2, 3), unbiased=False)
    a = bn.weight.double() / torch.sqrt(var + bn.eps)
    b = bn.bias.double() - mean * a
    ref = c * a[None, :, None, None] + b[None, :, None, None]
    if residual:
        ref = ref + idt.double()
    bound = a.abs()[None, :, None, None] * (2.0 ** -8 * c.abs() + 1e-5 * mag) + 2.0 ** -8 * ref.abs() + \
        (2e-3 * a.abs() * torch.sqrt(var))[None, :, None, None] + 1e-6
    ref = torch.relu(ref)
    err = (y.double() - ref).abs()
    assert torch.all(err <= bound), float((err - bound).max())


@pytest.mark.parametrize("cin,cout,k,s,p", [(128, 256, 3, 1, 1), (64, 128, 1, 2, 0)])
def test_conv_statistics_deterministic(cuda, cin, cout, k, s, p):
    from mcgmil.features import conv2d
    conv = _layer(cin, cout, k, s, p, cuda, 7)
    x = torch.randn(6, cin, 28, 28, device=cuda).relu_().bfloat16().contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y1, p1 = conv2d(conv, x, stats=True)
        y2, p2 = conv2d(conv, x, stats=True)
        y3 = conv2d(conv, x)
    assert torch.equal(y1, y2) and torch.equal(p1, p2) and torch.equal(y1, y3)


# conv(relu?(bn(x))) with the BatchNorm applied to the convolution's input patch (in_ab): both
# halo kernels (64 -> 64 weights in registers; Cin >= 128 streamed weights, 2-3 channel chunks),
# tiles spanning several images, odd widths, ragged pixel counts, and an input offset
INBN_SHAPES = [
    (3, 64, 56, 56, 64),
    (48, 64, 56, 56, 64),
    (120, 64, 20, 50, 64),
    (2, 64, 20, 62, 64),
    (9, 64, 8, 6, 64),
    (3, 64, 30, 17, 64),
    (2, 64, 20, 60, 64),
    (4, 128, 25, 20, 128),
    (2, 192, 17, 30, 256),
    (3, 128, 28, 28, 128),
]


@pytest.mark.parametrize("shape", INBN_SHAPES)
@pytest.mark.parametrize("relu", [True, False])
def test_conv_input_bn_bitwise_equals_unfused(cuda, shape, relu):
    """conv2d(conv, x, in_ab=ab) is bit-identical to conv2d(conv, batchnorm_act(x, bn)): the
    kernel rewrites its LDS patch with the apply pass's own arithmetic, padding left at zero.
    Its BatchNorm statistics of the output match too."""
    from mcgmil.features import batchnorm_act, batchnorm_coefficients, conv2d, conv_input_bn
    N, Cin, H, W, Cout = shape
    conv = _layer(Cin, Cout, 3, 1, 1, cuda, Cin + 2 * Cout)
    bn = _bn64(Cin, cuda, Cin + 5)
    g = torch.Generator(device=cuda).manual_seed(N * H + W + Cin)
    x = (torch.randn(N, Cin, H, W, device=cuda, generator=g) * 2.0 + 0.5).bfloat16()
    x = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert conv_input_bn(conv, x)
        ab = batchnorm_coefficients(x, bn)
        h = batchnorm_act(x, bn, relu)
        y_ref, p_ref = conv2d(conv, h, stats=True)
        y, p = conv2d(conv, x, stats=True, in_ab=ab, in_relu=relu)
        y_nostats = conv2d(conv, x, in_ab=ab, in_relu=relu)     # the kernel without the statistics
    assert torch.equal(y, y_ref)
    assert torch.equal(p, p_ref)
    assert torch.equal(y_nostats, y_ref)
    # and the coefficients are the ones the apply pass used: a, b from the fp64 statistics of x
    xd = x.double()
    mean, var = xd.mean(dim=(0, 2, 3)), xd.var(dim=(0, 2, 3), unbiased=False)
    a = bn.weight.double() / torch.sqrt(var + bn.eps)
    assert torch.allclose(ab[0].double(), a, rtol=1e-5, atol=0)
    assert torch.allclose(ab[1].double(), bn.bias.double() - mean * a, rtol=1e-5, atol=1e-5)


def test_conv_input_bn_support_and_errors(cuda):
    """Only the 3x3 / stride 1 halo kernels take in_ab; elsewhere conv2d refuses it."""
    from mcgmil.features import conv2d, conv_input_bn
    x = torch.randn(2, 64, 28, 28, device=cuda).bfloat16().contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert conv_input_bn(_layer(64, 64, 3, 1, 1, cuda, 1), x)
        assert not conv_input_bn(_layer(64, 128, 3, 2, 1, cuda, 1), x)        # stride 2
        assert not conv_input_bn(_layer(64, 128, 1, 1, 0, cuda, 1), x)        # 1 x 1
        x3 = torch.randn(2, 256, 14, 14, device=cuda).bfloat16().contiguous(memory_format=torch.channels_last)
        assert not conv_input_bn(_layer(256, 256, 3, 1, 1, cuda, 1), x3)      # 14 x 14: 256 x 256 tiles
        # width 62 runs the row ring (which takes in_ab); width 70 does not fit it, and the per-tile
        # patch kernel's two patches then fill the 160-KB LDS, no room for the a, b table
        x62 = torch.randn(2, 64, 20, 62, device=cuda).bfloat16().contiguous(memory_format=torch.channels_last)
        assert conv_input_bn(_layer(64, 64, 3, 1, 1, cuda, 1), x62)
        x70 = torch.randn(1, 64, 20, 70, device=cuda).bfloat16().contiguous(memory_format=torch.channels_last)
        assert not conv_input_bn(_layer(64, 64, 3, 1, 1, cuda, 1), x70)
        ab = torch.zeros(2, 64, device=cuda)
        with pytest.raises(RuntimeError):
            conv2d(_layer(64, 128, 3, 2, 1, cuda, 1), x, in_ab=ab)
        with pytest.raises(ValueError):
            conv2d(_layer(64, 64, 3, 1, 1, cuda, 1), x, in_ab=torch.zeros(2, 32, device=cuda))


def test_backbone_input_bn_bitwise(cuda):
    """ResNet-18 with its blocks' first BN deferred into the halo convolutions gives bit-identical
    features to the materialised form (MCGMIL_FUSE_INPUT_BN=0)."""
    import os
    from mcgmil.resnet import build_backbone, deactivate_batchnorm, Identity
    torch.manual_seed(0)
    net = build_backbone("r18", pretrained=False)
    net.fc = Identity()
    net.apply(deactivate_batchnorm)
    net = net.to(cuda).eval().to(memory_format=torch.channels_last)
    g = torch.Generator(device=cuda).manual_seed(9)
    x = torch.rand(10, 3, 112, 112, device=cuda, generator=g).contiguous(memory_format=torch.channels_last)
    out = {}
    for flag in ("1", "0"):
        os.environ["MCGMIL_FUSE_INPUT_BN"] = flag
        try:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                out[flag] = net(x).float()
        finally:
            os.environ.pop("MCGMIL_FUSE_INPUT_BN", None)
    assert torch.equal(out["1"], out["0"])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_residual_bn_bitwise_equals_unfused(cuda, dtype, C=128):
    """batchnorm_act(y, bn2, relu, residual=r, residual_ab=ab_d) equals normalising r in a pass of
    its own first (the downsample branch), bit for bit."""
    from mcgmil.features import batchnorm_act, batchnorm_coefficients
    bn2, bnd = _bn64(C, cuda, 11), _bn64(C, cuda, 12)
    g = torch.Generator(device=cuda).manual_seed(3)
    y = (torch.randn(5, C, 14, 13, device=cuda, generator=g) * 3 + 1).to(dtype).contiguous(
        memory_format=torch.channels_last)
    r = (torch.randn(5, C, 14, 13, device=cuda, generator=g) * 2 - 1).to(dtype).contiguous(
        memory_format=torch.channels_last)
    with torch.no_grad():
        ab_d = batchnorm_coefficients(r, bnd)
        ref = batchnorm_act(y, bn2, True, residual=batchnorm_act(r, bnd, False))
        out = batchnorm_act(y, bn2, True, residual=r, residual_ab=ab_d)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_residual_bn_bitwise_equals_unfused_c200(cuda, dtype):
    """The same at 200 channels: 25 channel groups do not divide a workgroup's 256 threads, so the
    apply grid is rounded to a multiple of 25 blocks for a thread to keep its a, b and the
    residual's own a, b."""
    test_residual_bn_bitwise_equals_unfused(cuda, dtype, C=200)


def test_backbone_running_statistics_folds_bitwise(cuda):
    """With BatchNorms on running statistics (eval without deactivate_batchnorm), the folds use the
    running coefficients: bit-identical to the materialised form."""
    import os
    from mcgmil.resnet import build_backbone, Identity
    torch.manual_seed(1)
    net = build_backbone("r18", pretrained=False)
    net.fc = Identity()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight[::9] *= -1.0
    net = net.to(cuda).eval().to(memory_format=torch.channels_last)
    g = torch.Generator(device=cuda).manual_seed(4)
    x = torch.rand(6, 3, 112, 112, device=cuda, generator=g).contiguous(memory_format=torch.channels_last)
    out = {}
    for flag in ("1", "0"):
        os.environ["MCGMIL_FUSE_INPUT_BN"] = flag
        try:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                out[flag] = net(x).float()
        finally:
            os.environ.pop("MCGMIL_FUSE_INPUT_BN", None)
    assert torch.equal(out["1"], out["0"])
    assert torch.isfinite(out["1"]).all()
