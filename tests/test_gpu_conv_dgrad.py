"""The direct fp32 convolution data gradient on the HIP kernel (include/mcgmil_conv_dgrad.h,
features.conv2d_f32_dgrad_direct, the route MCGMIL_CONV_GRAD=direct of torch.ops.mcgmil.conv2d_f32's
backward and of MultiHeadGatedAttentionMIL.enable_backbone_training) against float64 CPU autograd
of F.conv2d.

Error of a tensor: max|got - ref| / max|ref| (golden_util.nrel). Bound: 10 x the same error of
fp32 CPU autograd on that case (the project's x10 for a changed summation order),
at least 1e-6. Every test prints measured / bound before it asserts."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_dgrad_ref as ref
import golden_util
from mcgmil import _lib, features, library  # noqa: F401

pytestmark = pytest.mark.gpu

CL = torch.channels_last
INVALID, UNSUPPORTED = -1, -2                # enum mcgmil_status (include/mcgmil.h)


def gpu(c, dev):
    return c.x.to(dev).contiguous(memory_format=CL), c.dy.to(dev).contiguous(memory_format=CL)


def conv_of(c, dev):
    return features._ConvShim(c.w.to(dev), c.stride, c.pad)


def dgrad_args(conv, x_shape, dy, wt, dx):
    g = _lib.ConvDgradArgs()
    a = g.fwd
    a.batch, a.in_channels, a.height, a.width = x_shape
    a.out_channels, (a.kernel_h, a.kernel_w) = conv.out_channels, conv.kernel_size
    a.stride, a.pad = conv.stride[0], conv.padding[0]
    g.dy, g.w_t, g.dx = (ctypes.c_void_p(t.data_ptr()) if t is not None else None for t in (dy, wt, dx))
    return g


def raw_dgrad(conv, dy, dx):
    """mcgmil_conv2d_dgrad_f32 into a caller-owned dx (features.conv2d_f32_dgrad_direct allocates its own)."""
    wt = conv.weight.detach().permute(2, 3, 0, 1).contiguous()
    g = dgrad_args(conv, dx.shape, dy, wt, dx)
    _lib.check(_lib.load().mcgmil_conv2d_dgrad_f32(ctypes.byref(g), None), "dgrad")
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 1. parity, overwrite, repeat
@pytest.mark.parametrize("name", ref.TABLE)
def test_dgrad_parity_overwrite_and_repeat(cuda, name):
    c = ref.case(name)
    x, dy = gpu(c, cuda)
    conv = conv_of(c, cuda)
    assert features.dgrad_direct_supported(conv, dy)
    dx = torch.full(x.shape, float("nan"), device=cuda).contiguous(memory_format=CL)
    raw_dgrad(conv, dy, dx)
    assert bool(torch.isfinite(dx).all())                       # NaN preset fully overwritten
    c.check("dx", dx)
    again = features.conv2d_f32_dgrad_direct(conv, dy, x.shape)
    assert again.shape == x.shape and again.is_contiguous(memory_format=CL)
    assert torch.equal(again, dx)                               # bitwise


# ---------------------------------------------------------------- 2. exact zeros
def test_tapless_classes_are_exact_zeros(cuda):
    c = ref.case("s2_1x1")
    _, dy = gpu(c, cuda)
    dx = features.conv2d_f32_dgrad_direct(conv_of(c, cuda), dy, c.x.shape).cpu()
    live = dx[:, :, 0::2, 0::2]
    assert bool((live != 0).any())
    off = dx.clone()
    off[:, :, 0::2, 0::2] = 0
    assert not bool(off.any())                                  # classes (0,1), (1,0), (1,1): exactly 0
    assert dx.numel() - live.numel() == 2 * 64 * (90 - 25)      # 72% of dx
    c.check("dx", dx)


@pytest.mark.parametrize("name", ["s2_3x3_p0_tail", "s2_2x2_tail"])
def test_rows_and_columns_past_the_last_window_are_exact_zeros(cuda, name):
    c = ref.case(name)
    _, dy = gpu(c, cuda)
    dx = features.conv2d_f32_dgrad_direct(conv_of(c, cuda), dy, c.x.shape).cpu()
    assert not bool(dx[:, :, -1, :].any()) and not bool(dx[:, :, :, -1].any())
    assert bool((dx[:, :, :-1, :-1] != 0).all())
    c.check("dx", dx)


# ---------------------------------------------------------------- 3. one pixel
def test_dgrad_one_pixel(cuda):
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(64, 64, 3, 3, generator=gen) / 24.0
    dy = torch.randn(1, 64, 1, 1, generator=gen)
    conv = features._ConvShim(w.to(cuda), 2, 1)
    dx = features.conv2d_f32_dgrad_direct(conv, dy.to(cuda).contiguous(memory_format=CL), (1, 64, 1, 1)).cpu()
    want = (dy.double().view(64, 1) * w[:, :, 1, 1].double()).sum(0)
    want32 = (dy.view(64, 1) * w[:, :, 1, 1]).sum(0).double()
    bound = max(10.0 * golden_util.nrel(want32.numpy(), want.numpy()), 1e-6)
    err = golden_util.nrel(dx[0, :, 0, 0].numpy(), want.numpy())
    print(f"one pixel centre tap: {err:.2e} / {bound:.2e}")
    assert err <= bound


# ---------------------------------------------------------------- 4. batch independence
def test_an_image_alone_is_bitwise_the_image_in_the_batch(cuda):
    c = ref.case("s2_c64_two_tiles")
    x, dy = gpu(c, cuda)
    conv = conv_of(c, cuda)
    whole = features.conv2d_f32_dgrad_direct(conv, dy, x.shape)
    alone = features.conv2d_f32_dgrad_direct(conv, dy[1:2].contiguous(memory_format=CL), (1,) + tuple(x.shape[1:]))
    assert torch.equal(alone[0], whole[1])


# ---------------------------------------------------------------- 5. offsets past 2^31 bytes
def test_dgrad_offsets_past_2gib(cuda):
    N, C, H = 33, 64, 512
    gen = torch.Generator().manual_seed(11)
    w = torch.randn(C, C, 3, 3, generator=gen) / 24.0
    dyl = torch.randn(1, C, H // 2, H // 2, generator=gen)
    dy = torch.empty(N, C, H // 2, H // 2, device=cuda, memory_format=CL).zero_()
    dy[N - 1:] = dyl.to(cuda)
    conv = features._ConvShim(w.to(cuda), 2, 1)
    dx = features.conv2d_f32_dgrad_direct(conv, dy, (N, C, H, H))
    assert dx.numel() * 4 > 2 ** 31
    assert not bool(dx[:-1].any())                               # every other image: exactly 0
    last = dx[N - 1:].cpu()
    del dx, dy

    def cpu(dt):
        x = torch.zeros(1, C, H, H, dtype=dt, requires_grad=True)
        F.conv2d(x, w.to(dt), None, 2, 1).backward(dyl.to(dt))
        return x.grad
    want = cpu(torch.float64)
    bound = max(10.0 * golden_util.nrel(cpu(torch.float32).numpy(), want.numpy()), 1e-6)
    err = golden_util.nrel(last.numpy(), want.numpy())
    print(f"past 2 GiB dx: {err:.2e} / {bound:.2e}")
    assert err <= bound


# ---------------------------------------------------------------- 6. the op on the new route
def count_calls(monkeypatch):
    calls = {"wgrad": 0, "direct": 0, "dgrad": 0, "aten": 0}
    for key, name in (("wgrad", "conv2d_f32_wgrad"), ("direct", "conv2d_f32_dgrad_direct"),
                      ("dgrad", "conv2d_f32_dgrad"), ("aten", "_aten_conv_backward")):
        def counted(*a, _real=getattr(features, name), _key=key, **k):
            calls[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(features, name, counted)
    return calls


@pytest.mark.parametrize("name", ["s1_3x3_odd", "s2_3x3_even", "s1_c48_5x5"])
def test_autograd_through_the_op_on_the_direct_route(cuda, name, monkeypatch):
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "direct")
    calls = count_calls(monkeypatch)
    c = ref.case(name)
    x, dy = gpu(c, cuda)
    x.requires_grad_()
    w = c.w.to(cuda).requires_grad_()
    y = torch.ops.mcgmil.conv2d_f32(x, w, c.stride, c.pad)
    (y * dy).sum().backward()
    c.check("dw", w.grad)
    c.check("dx", x.grad)
    assert calls == {"wgrad": 1, "direct": 1, "dgrad": 0, "aten": 0}


def test_opcheck_on_the_direct_route(cuda, monkeypatch):
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "direct")
    c = ref.case("s2_3x3_odd")
    x, dy = gpu(c, cuda)
    w = c.w.to(cuda)
    torch.library.opcheck(torch.ops.mcgmil.conv2d_f32.default,
                          (x.clone().requires_grad_(), w.clone().requires_grad_(), c.stride, c.pad))
    torch.library.opcheck(torch.ops.mcgmil.conv2d_f32_backward.default, (x, w, dy, c.stride, c.pad, True, True))


# ---------------------------------------------------------------- 7. the module
def test_module_train_step_on_the_direct_route(cuda, monkeypatch):
    import test_gpu_conv_grad as base
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "direct")
    calls = count_calls(monkeypatch)
    m, x, target, seed, g64, bounds = base.module_case()
    m = copy.deepcopy(m).train().enable_head_training()
    assert m.enable_backbone_training() is m
    routed = []
    real = features.conv2d_f32_op
    monkeypatch.setattr(features, "conv2d_f32_op", lambda layer, t: routed.append(layer) or real(layer, t))
    Y, A, aux = m(x, target, seed=seed)
    (F.cross_entropy(Y, target) + aux).backward()
    assert len(routed) == 19                                    # every convolution but the 3-channel stem
    assert calls == {"wgrad": 19, "direct": 19, "dgrad": 0, "aten": 0}
    for n in base.LAYERS:
        g = m.feature_extractor.get_submodule(n).weight.grad
        err = golden_util.nrel(g.cpu().numpy(), g64[n])
        print(f"route=direct {n}: {err:.2e} / {bounds[n]:.2e}")
        assert bool(torch.isfinite(g).all()) and err <= bounds[n], n


# ---------------------------------------------------------------- 8. validation
def test_validation(cuda):
    L = _lib.load()
    dy = torch.zeros(1, 64, 4, 4, device=cuda).contiguous(memory_format=CL)
    wt = torch.zeros(3, 3, 64, 64, device=cuda)
    dx = torch.full((1, 64, 4, 4), 7.0, device=cuda).contiguous(memory_format=CL)
    conv = features._ConvShim(torch.zeros(64, 64, 3, 3, device=cuda), 1, 1)

    def args(**kw):
        g = dgrad_args(conv, dx.shape, dy, wt, dx)
        for k, v in kw.items():
            setattr(g.fwd, k, v)
        return g

    def rc_of(g):
        rc = L.mcgmil_conv2d_dgrad_f32(ctypes.byref(g), None)
        if rc:
            assert len(L.mcgmil_last_error()) > 0
        return rc
    for bad in (dict(stride=3), dict(in_channels=24), dict(out_channels=32), dict(kernel_h=8), dict(kernel_w=8),
                dict(pad=3), dict(pad=5)):
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
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all())                              # nothing was launched
    assert rc_of(args()) == 0
    torch.cuda.synchronize()
    assert not bool(dx.any())                                   # dy = 0: overwritten with zeros
