"""The direct bf16 convolution data gradient on the HIP kernel (include/mcgmil_conv_dgrad_bf16.h,
features.conv2d_bf16_dgrad_direct, the route MCGMIL_CONV_GRAD=direct of torch.ops.mcgmil.conv2d_bf16's
backward and of MultiHeadGatedAttentionMIL.enable_bf16_backbone_training) against float64 CPU
autograd of F.conv2d on the bf16-rounded inputs.

Cases, references and bounds: tests/conv_dgrad_bf16_ref.py. dx, rounded to bf16 once:
|d| <= 2^-7 |ref| + B max|ref| elementwise, B = max(10 x the error of fp32 CPU autograd, 1e-6); dw
(fp32): nrel <= max(10 x the error of fp32 CPU autograd, 1e-6). Every test prints measured / bound
before it asserts."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_dgrad_bf16_ref as ref
import golden_util
from mcgmil import MultiHeadGatedAttentionMIL, _lib, features, library  # noqa: F401
from mcgmil.resnet import deactivate_batchnorm

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
INVALID, UNSUPPORTED = -1, -2                # enum mcgmil_status (include/mcgmil.h)


def dgrad_args(conv, x_shape, dy, wt, dx):
    g = _lib.ConvDgradBf16Args()
    a = g.fwd
    a.batch, a.in_channels, a.height, a.width = x_shape
    a.out_channels, (a.kernel_h, a.kernel_w) = conv.out_channels, conv.kernel_size
    a.stride, a.pad = conv.stride[0], conv.padding[0]
    g.dy, g.w_t, g.dx = (ctypes.c_void_p(t.data_ptr()) if t is not None else None for t in (dy, wt, dx))
    return g


def raw_dgrad(conv, dy, dx):
    """mcgmil_conv2d_dgrad_bf16 into a caller-owned dx (features.conv2d_bf16_dgrad_direct allocates its own)."""
    wt = conv.weight.detach().to(BF).permute(2, 3, 1, 0).contiguous()
    g = dgrad_args(conv, dx.shape, dy, wt, dx)
    _lib.check(_lib.load().mcgmil_conv2d_dgrad_bf16(ctypes.byref(g), None), "dgrad")
    torch.cuda.synchronize()


def direct(c, dev, dy=None, x_shape=None):
    dy = c.gpu(dev)[1] if dy is None else dy
    return features.conv2d_bf16_dgrad_direct(c.conv(dev), dy, c.x.shape if x_shape is None else x_shape)


# ---------------------------------------------------------------- 1. parity, overwrite, repeat
@pytest.mark.parametrize("name", ref.TABLE)
def test_dgrad_parity_overwrite_and_repeat(cuda, name):
    c = ref.case(name)
    x, dy = c.gpu(cuda)
    conv = c.conv(cuda)
    assert features.dgrad_bf16_direct_supported(conv, dy)
    # every 16-bit pattern 0x7fc0: a bf16 NaN
    dx = torch.full(x.shape, float("nan"), device=cuda, dtype=BF).contiguous(memory_format=CL)
    assert bool(torch.isnan(dx).all())
    raw_dgrad(conv, dy, dx)
    assert bool(torch.isfinite(dx).all())                       # NaN preset fully overwritten
    c.check_dx(dx)
    again = features.conv2d_bf16_dgrad_direct(conv, dy, x.shape)
    assert again.shape == x.shape and again.dtype == BF and again.is_contiguous(memory_format=CL)
    assert torch.equal(again, dx)                               # bitwise
    bf16_weight = features.conv2d_bf16_dgrad_direct(c.conv(cuda, BF), dy, x.shape)
    assert torch.equal(bf16_weight, dx)                         # the fp32 master weight is cast, no more


# ---------------------------------------------------------------- 2. exact zeros
def _is_plus_zero(t):
    return not bool(t.view(torch.int16).any())                  # all bits clear: +0, not -0


def test_tapless_classes_are_exact_zeros(cuda):
    c = ref.case("s2_1x1")
    dx = direct(c, cuda).cpu()
    live = dx[:, :, 0::2, 0::2]
    assert bool((live != 0).any())
    off = dx.clone()
    off[:, :, 0::2, 0::2] = 0
    assert _is_plus_zero(off)                                   # classes (0,1), (1,0), (1,1): exactly +0
    assert dx.numel() - live.numel() == 2 * 64 * (90 - 25)      # 72% of dx
    c.check_dx(dx)


@pytest.mark.parametrize("name", ["s2_3x3_p0_tail", "s2_2x2_tail"])
def test_rows_and_columns_past_the_last_window_are_exact_zeros(cuda, name):
    c = ref.case(name)
    dx = direct(c, cuda).cpu()
    assert _is_plus_zero(dx[:, :, -1, :].contiguous()) and _is_plus_zero(dx[:, :, :, -1].contiguous())
    assert bool((dx[:, :, :-1, :-1] != 0).all())
    c.check_dx(dx)


# ---------------------------------------------------------------- 3. one pixel
def test_dgrad_one_pixel(cuda):
    gen = torch.Generator().manual_seed(5)
    w = ref.round_bf16(torch.randn(64, 64, 3, 3, generator=gen) / 24.0)
    dy = ref.round_bf16(torch.randn(1, 64, 1, 1, generator=gen))
    conv = features._ConvShim(w.to(cuda), 2, 1)
    dx = features.conv2d_bf16_dgrad_direct(conv, dy.to(cuda, BF).contiguous(memory_format=CL), (1, 64, 1, 1)).cpu()
    want = (dy.double().view(64, 1) * w[:, :, 1, 1].double()).sum(0)
    want32 = (dy.view(64, 1) * w[:, :, 1, 1]).sum(0).double()
    bound = max(10.0 * golden_util.nrel(want32.numpy(), want.numpy()), 1e-6)
    assert dx.dtype == BF and dx.shape == (1, 64, 1, 1)
    ref.check_dx("one pixel centre tap", dx[0, :, 0, 0], want, bound)


# ---------------------------------------------------------------- 4. batch independence
def test_an_image_alone_is_bitwise_the_image_in_the_batch(cuda):
    c = ref.case("s2_3x3_odd")
    x, dy = c.gpu(cuda)
    dy3 = torch.cat([dy[:1], dy[1:], dy[:1]]).contiguous(memory_format=CL)        # a batch of three
    whole = direct(c, cuda, dy3, (3,) + tuple(x.shape[1:]))
    alone = direct(c, cuda, dy[1:2].contiguous(memory_format=CL), (1,) + tuple(x.shape[1:]))
    assert torch.equal(alone[0], whole[1])
    assert torch.equal(whole[0], whole[2])
    c.check_dx(whole[:2])


# ---------------------------------------------------------------- 5. the op on the direct route
class _AtenSpy:
    """Stands in for torch.ops.aten.convolution_backward and records each call's output mask;
    everything else (.default, ...) is the real packet's."""

    def __init__(self, monkeypatch):
        self.masks = []
        self._real = torch.ops.aten.convolution_backward
        monkeypatch.setattr(torch.ops.aten, "convolution_backward", self)

    def __call__(self, *a, **k):
        self.masks.append(tuple(a[-1]))
        return self._real(*a, **k)

    def __getattr__(self, name):
        return getattr(self._real, name)


@pytest.mark.parametrize("name", ref.TABLE)
def test_op_direct_route(cuda, name, monkeypatch):
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "direct")
    c = ref.case(name)
    x, dy = c.gpu(cuda)
    spy = _AtenSpy(monkeypatch)
    directs = []
    real = features.conv2d_bf16_dgrad_direct
    monkeypatch.setattr(features, "conv2d_bf16_dgrad_direct", lambda *a, **k: directs.append(1) or real(*a, **k))

    def step():
        xx = x.clone().requires_grad_()
        w = c.w.to(cuda).requires_grad_()                        # the fp32 master weight
        y = torch.ops.mcgmil.conv2d_bf16(xx, w, c.stride, c.pad)
        y.backward(dy)
        return xx.grad, w.grad
    dx, dw = step()
    assert dw.dtype == torch.float32 and dw.is_contiguous()
    assert dx.dtype == BF and dx.is_contiguous(memory_format=CL)
    c.check_dw(dw)
    c.check_dx(dx)
    dx2, dw2 = step()
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw)         # a second step: bitwise
    gx, gw = torch.ops.mcgmil.conv2d_bf16_backward(x, c.w.to(cuda), dy, c.stride, c.pad, True, False)
    assert gw.numel() == 0 and torch.equal(gx, dx)
    gx, gw = torch.ops.mcgmil.conv2d_bf16_backward(x, c.w.to(cuda), dy, c.stride, c.pad, False, True)
    assert gx.numel() == 0 and torch.equal(gw, dw)
    assert spy.masks == []                                       # no gradient leaves the project's kernels
    native = features.dgrad_bf16_native(c.conv(cuda), dy)        # stride 1 and square: the flipped forward, as before
    assert len(directs) == (0 if native else 3), (native, directs)


def test_opcheck_on_the_direct_route(cuda, monkeypatch):
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "direct")
    c = ref.case("s2_3x3_even")
    x, dy = c.gpu(cuda)
    w = c.w.to(cuda)
    torch.library.opcheck(torch.ops.mcgmil.conv2d_bf16.default,
                          (x.clone().requires_grad_(), w.clone().requires_grad_(), c.stride, c.pad))
    torch.library.opcheck(torch.ops.mcgmil.conv2d_bf16_backward.default, (x, w, dy, c.stride, c.pad, True, True))


# ---------------------------------------------------------------- 6. the module
def _step(m, x, target, seed, autocast=False):
    """One step's gradients {parameter name: tensor}."""
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", BF, enabled=autocast):
        Y, A, aux = m(x, target, seed=seed)
    (F.cross_entropy(Y.float(), target) + aux.float()).backward()
    return {n: p.grad for n, p in m.named_parameters()}


def _drift(got, want, scale):
    """nrel of a gradient against the fp32 step's. A reference gradient below 1e-6 of the largest
    gradient of the model is the rounding residue of a quantity that is zero in exact arithmetic
    (the bias of an attention score: softmax does not see it), and a ratio of two residues measures
    nothing: such a parameter is measured against the model-wide scale instead."""
    want = want.double().cpu().numpy()
    den = np.abs(want).max()
    if den >= 1e-6 * scale:
        return golden_util.nrel(got.double().cpu().numpy(), want)
    return float(np.abs(got.double().cpu().numpy() - want).max() / scale)


@functools.lru_cache(maxsize=None)
def module_case():
    """The module, one bag, and the yardsticks of tests/test_gpu_conv_grad_bf16.py's
    test_module_train_step, restated: the gradients of the same step in fp32 on the torch layers,
    and those of the user's own autocast over the torch layers."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(7)
    m = MultiHeadGatedAttentionMIL(num_classes=2, backbone="r18", pretrained=False).to(dev)
    m.apply(deactivate_batchnorm)
    m.train().enable_head_training()
    x = torch.rand(1, 6, 3, 96, 96, device=dev)
    target = torch.tensor([1], device=dev)
    seed = 1234
    g32 = _step(copy.deepcopy(m), x, target, seed)
    gac = _step(copy.deepcopy(m), x, target, seed, autocast=True)
    return m, x, target, seed, g32, gac


def test_module_train_step_on_the_direct_route(cuda, monkeypatch):
    m0, x, target, seed, g32, gac = module_case()
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "direct")

    def fresh():
        m = copy.deepcopy(m0)
        m.enable_bf16_backbone_training().enable_bf16_norm_training().enable_bf16_stem_training()
        return m.enable_bf16_stem_conv_training()
    spy = _AtenSpy(monkeypatch)
    directs, flipped = [], []
    real_d, real_f = features.conv2d_bf16_dgrad_direct, features.conv2d_bf16_dgrad
    monkeypatch.setattr(features, "conv2d_bf16_dgrad_direct", lambda *a, **k: directs.append(1) or real_d(*a, **k))
    monkeypatch.setattr(features, "conv2d_bf16_dgrad", lambda *a, **k: flipped.append(1) or real_f(*a, **k))
    grads = _step(fresh(), x, target, seed)
    # layer{2,3,4}.0.conv1 and the three 1x1 downsamples; the 13 stride-1 convolutions as before
    assert (len(directs), len(flipped)) == (6, 13)
    assert spy.masks == []                                       # no gradient leaves the project's kernels
    scale = max(float(g.abs().max()) for g in g32.values())
    rows = []
    for n, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any()), n
        err, yard = _drift(g, g32[n], scale), _drift(gac[n], g32[n], scale)
        bound = 2.0 * yard + 1e-3
        rows.append((n, err, bound))
        print(f"route=direct {n}: {err:.2e} / {bound:.2e} (autocast over the torch layers: {yard:.2e})")
    for n, err, bound in rows:
        assert err <= bound, (n, err, bound)
    # a second step from identical state and seed: every gradient bitwise
    again = _step(fresh(), x, target, seed)
    differ = [n for n in grads if not torch.equal(again[n], grads[n])]
    print(f"route=direct: {len(differ)} of {len(grads)} gradients differ between two steps: {differ}")
    assert differ == []


# ---------------------------------------------------------------- 7. validation
def test_validation(cuda):
    L = _lib.load()
    dy = torch.zeros(1, 64, 4, 4, device=cuda, dtype=BF).contiguous(memory_format=CL)
    wt = torch.zeros(3, 3, 64, 64, device=cuda, dtype=BF)
    dx = torch.full((1, 64, 4, 4), 7.0, device=cuda, dtype=BF).contiguous(memory_format=CL)
    conv = features._ConvShim(torch.zeros(64, 64, 3, 3, device=cuda), 1, 1)

    def args(**kw):
        g = dgrad_args(conv, dx.shape, dy, wt, dx)
        for k, v in kw.items():
            setattr(g.fwd, k, v)
        return g

    def rc_of(g):
        rc = L.mcgmil_conv2d_dgrad_bf16(ctypes.byref(g), None)
        if rc:
            assert len(L.mcgmil_last_error()) > 0
        return rc
    for bad in (dict(stride=3), dict(in_channels=48), dict(in_channels=16), dict(out_channels=32), dict(kernel_h=8),
                dict(kernel_w=8), dict(pad=3), dict(pad=5)):
        assert rc_of(args(**bad)) == UNSUPPORTED, bad
    for field in ("dy", "w_t", "dx"):
        g = args()
        setattr(g, field, None)
        assert rc_of(g) == INVALID, field
        g = args()
        setattr(g, field, ctypes.c_void_p(getattr(g, field) + 4))     # misaligned
        assert rc_of(g) == INVALID, field
    g = args()
    g.reserved = 1
    assert rc_of(g) == INVALID
    for shape in ((1, 64, 5, 4), (2, 64, 4, 4), (1, 128, 4, 4)):      # an x_shape that is not this dy's
        with pytest.raises(ValueError):
            features.conv2d_bf16_dgrad_direct(conv, dy, shape)
    with pytest.raises(ValueError):
        features.conv2d_bf16_dgrad_direct(conv, dy.float(), dx.shape)
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all())                              # nothing was launched
    assert rc_of(args()) == 0
    torch.cuda.synchronize()
    assert _is_plus_zero(dx)                                    # dy = 0: overwritten with zeros
