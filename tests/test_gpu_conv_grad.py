"""The fp32 convolution backward on the HIP kernels (include/mcgmil_conv_grad.h,
features.conv2d_f32_wgrad / conv2d_f32_dgrad, torch.ops.mcgmil.conv2d_f32 and its backward op,
MultiHeadGatedAttentionMIL.enable_backbone_training) against float64 CPU autograd of F.conv2d.

Error of a tensor: max|got - ref| / max|ref| (golden_util.nrel). Bound: 10 x the same error of
fp32 CPU autograd on that case (the project's x10 for a changed summation order),
at least 1e-6. Every test prints measured / bound before it asserts."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util
import head_grad_ref as ref
from mcgmil import MultiHeadGatedAttentionMIL, _lib, features, library, ops  # noqa: F401

pytestmark = pytest.mark.gpu

G = _lib.WGRAD_GRANULE_PIXELS

CASES = {
    #                   N  Cin  Cout k  s  p  H   W
    "c64_3x3_odd":     (3, 64,  64,  3, 1, 1, 9,  7),     # 189 pixels: no multiple of a K step
    "s2_3x3_even":     (2, 64,  128, 3, 2, 1, 10, 10),
    "s2_3x3_odd":      (2, 64,  128, 3, 2, 1, 9,  11),
    "s2_1x1":          (2, 64,  128, 1, 2, 0, 9,  10),
    "wide_in_1x1":     (1, 256, 64,  1, 1, 0, 7,  7),
    "c48_5x5":         (2, 48,  64,  5, 1, 2, 6,  7),     # Cin a multiple of 16 only, generic taps
    "c192_3x3":        (1, 128, 192, 3, 1, 0, 5,  5),     # Cout no multiple of 128
    # batch * OH * OW = 2 G + G / 2 + 5: three granules, the last one ragged
    "granules":        (1, 64,  64,  3, 1, 1, 1,  2 * G + G // 2 + 5),
}
TABLE = [k for k in CASES if k != "granules"]


class Case:
    """Inputs of a case and its float64 / fp32 CPU autograd gradients (computed once)."""

    def __init__(self, name):
        self.name = name
        N, Cin, Cout, k, s, p, H, W = CASES[name]
        self.stride, self.pad = s, p
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        self.x = torch.randn(N, Cin, H, W, generator=gen)
        self.w = torch.randn(Cout, Cin, k, k, generator=gen) / (Cin * k * k) ** 0.5
        oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        self.dy = torch.randn(N, Cout, oh, ow, generator=gen)
        self.dx64, self.dw64 = self._cpu(torch.float64)
        dx32, dw32 = self._cpu(torch.float32)
        self.bound_dx = max(10.0 * golden_util.nrel(dx32.numpy(), self.dx64.numpy()), 1e-6)
        self.bound_dw = max(10.0 * golden_util.nrel(dw32.numpy(), self.dw64.numpy()), 1e-6)

    def _cpu(self, dt):
        x = self.x.to(dt).clone().requires_grad_()
        w = self.w.to(dt).clone().requires_grad_()
        F.conv2d(x, w, None, self.stride, self.pad).backward(self.dy.to(dt))
        return x.grad, w.grad

    def conv(self, dev):
        return features._ConvShim(self.w.to(dev), self.stride, self.pad)

    def gpu(self, dev):
        cl = torch.channels_last
        return self.x.to(dev).contiguous(memory_format=cl), self.dy.to(dev).contiguous(memory_format=cl)

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


def raw_wgrad(conv, x, dy, dw, chunk_pixels=0):
    """mcgmil_conv2d_wgrad_f32 into a caller-owned dw (features.conv2d_f32_wgrad allocates its own)."""
    L = _lib.load()
    g = _lib.ConvGradArgs()
    a = g.fwd
    a.batch, a.in_channels, a.height, a.width = x.shape
    a.out_channels, (a.kernel_h, a.kernel_w) = conv.out_channels, conv.kernel_size
    a.stride, a.pad = conv.stride[0], conv.padding[0]
    a.x, g.dy, g.dw = (ctypes.c_void_p(t.data_ptr()) for t in (x, dy, dw))
    g.chunk_pixels = chunk_pixels
    n = ctypes.c_size_t()
    _lib.check(L.mcgmil_conv_wgrad_workspace_size_f32(ctypes.byref(g), ctypes.byref(n)), "size")
    ws = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    g.workspace, g.workspace_bytes = ctypes.c_void_p(ws.data_ptr()), n.value
    _lib.check(L.mcgmil_conv2d_wgrad_f32(ctypes.byref(g), None), "wgrad")
    torch.cuda.synchronize()
    return n.value


# ---------------------------------------------------------------- 1. weight gradient
@pytest.mark.parametrize("name", TABLE)
def test_wgrad_parity_overwrite_and_repeat(cuda, name):
    c = case(name)
    x, dy = c.gpu(cuda)
    conv = c.conv(cuda)
    assert features.conv32_trainable(conv, x)
    dw = torch.full(c.w.shape, float("nan"), device=cuda)
    raw_wgrad(conv, x, dy, dw)
    assert bool(torch.isfinite(dw).all())                      # NaN preset fully overwritten
    c.check("dw", dw)
    again = features.conv2d_f32_wgrad(conv, x, dy)
    assert again.is_contiguous() and torch.equal(again, dw)     # bitwise


# ---------------------------------------------------------------- 2. one pixel
def test_wgrad_one_pixel(cuda):
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(1, 64, 1, 1, generator=gen)
    dy = torch.randn(1, 64, 1, 1, generator=gen)
    conv = features._ConvShim(torch.zeros(64, 64, 3, 3, device=cuda), 1, 1)
    dw = features.conv2d_f32_wgrad(conv, x.to(cuda).contiguous(memory_format=torch.channels_last),
                                   dy.to(cuda).contiguous(memory_format=torch.channels_last)).cpu()
    want = dy.double().view(64, 1) * x.double().view(1, 64)
    want32 = (dy.view(64, 1) * x.view(1, 64)).double()
    bound = max(10.0 * golden_util.nrel(want32.numpy(), want.numpy()), 1e-6)
    err = golden_util.nrel(dw[:, :, 1, 1].numpy(), want.numpy())
    print(f"one pixel centre tap: {err:.2e} / {bound:.2e}")
    assert err <= bound
    off = dw.clone()
    off[:, :, 1, 1] = 0
    assert not bool(off.any())                                  # the eight other taps: exactly 0


# ---------------------------------------------------------------- 3. granules
def test_wgrad_granules_and_chunking(cuda):
    c = case("granules")
    x, dy = c.gpu(cuda)
    assert dy.shape[0] * dy.shape[2] * dy.shape[3] == 2 * G + G // 2 + 5
    conv = c.conv(cuda)
    whole = torch.empty(c.w.shape, device=cuda)
    n_whole = raw_wgrad(conv, x, dy, whole)
    c.check("dw", whole)
    chunked = torch.full(c.w.shape, float("nan"), device=cuda)
    n_chunked = raw_wgrad(conv, x, dy, chunked, chunk_pixels=G)     # three one-granule chunks
    assert torch.equal(chunked, whole)
    assert n_chunked < n_whole                                   # the workspace follows chunk_pixels
    assert torch.equal(features.conv2d_f32_wgrad(conv, x, dy, chunk_pixels=2 * G), whole)


# ---------------------------------------------------------------- 4. offsets past 2^31 bytes
def test_wgrad_offsets_past_2gib(cuda):
    N, C, H = 33, 64, 512
    gen = torch.Generator().manual_seed(11)
    xl = torch.randn(1, C, H, H, generator=gen)
    dyl = torch.randn(1, C, H, H, generator=gen)
    cl = torch.channels_last
    x = torch.empty(N, C, H, H, device=cuda, memory_format=cl).zero_()
    dy = torch.empty(N, C, H, H, device=cuda, memory_format=cl).zero_()
    assert x.numel() * 4 > 2 ** 31
    x[N - 1:] = xl.to(cuda)
    dy[N - 1:] = dyl.to(cuda)
    conv = features._ConvShim(torch.zeros(C, C, 1, 1, device=cuda), 1, 0)
    dw = features.conv2d_f32_wgrad(conv, x, dy).cpu()
    del x, dy

    def cpu(dt):
        w = torch.zeros(C, C, 1, 1, dtype=dt, requires_grad=True)
        F.conv2d(xl.to(dt), w).backward(dyl.to(dt))
        return w.grad
    want = cpu(torch.float64)
    bound = max(10.0 * golden_util.nrel(cpu(torch.float32).numpy(), want.numpy()), 1e-6)
    err = golden_util.nrel(dw.numpy(), want.numpy())
    print(f"past 2 GiB dw: {err:.2e} / {bound:.2e}")
    assert err <= bound


# ---------------------------------------------------------------- 5. data gradient
@pytest.mark.parametrize("name", TABLE)
def test_dgrad(cuda, name, monkeypatch):
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "native")
    c = case(name)
    x, dy = c.gpu(cuda)
    conv = c.conv(cuda)
    calls = []
    real = features.conv2d_f32
    monkeypatch.setattr(features, "conv2d_f32", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    dx = features.conv2d_f32_dgrad(conv, dy, x.shape)
    assert len(calls) == (1 if c.stride == 1 else 0)            # native forward kernel / aten fallback
    assert features.dgrad_native(conv) == (c.stride == 1)
    assert dx.is_contiguous(memory_format=torch.channels_last)
    c.check("dx", dx)
    dx2, dw2 = torch.ops.mcgmil.conv2d_f32_backward(x, conv.weight, dy, c.stride, c.pad, False, True)
    assert dx2.numel() == 0
    c.check("dw", dw2)


# ---------------------------------------------------------------- 6. the ops
@pytest.mark.parametrize("route", ["native", "aten"])
@pytest.mark.parametrize("name", ["c64_3x3_odd", "s2_3x3_odd"])
def test_opcheck(cuda, name, route, monkeypatch):
    monkeypatch.setenv("MCGMIL_CONV_GRAD", route)
    c = case(name)
    x, dy = c.gpu(cuda)
    w = c.w.to(cuda)
    torch.library.opcheck(torch.ops.mcgmil.conv2d_f32.default,
                          (x.clone().requires_grad_(), w.clone().requires_grad_(), c.stride, c.pad))
    torch.library.opcheck(torch.ops.mcgmil.conv2d_f32_backward.default, (x, w, dy, c.stride, c.pad, True, True))


@pytest.mark.parametrize("route", ["native", "aten"])
@pytest.mark.parametrize("name", ["c64_3x3_odd", "s2_3x3_even", "c48_5x5"])
def test_autograd_through_the_op(cuda, name, route, monkeypatch):
    """loss.backward() through the op on both backward routes (features.conv_grad_native): the HIP
    kernels, and aten.convolution_backward (the default, measured-fastest one)."""
    monkeypatch.setenv("MCGMIL_CONV_GRAD", route)
    wgrads, dgrads = [], []
    real_w, real_d = features.conv2d_f32_wgrad, features.conv2d_f32_dgrad
    monkeypatch.setattr(features, "conv2d_f32_wgrad", lambda *a, **k: wgrads.append(1) or real_w(*a, **k))
    monkeypatch.setattr(features, "conv2d_f32_dgrad", lambda *a, **k: dgrads.append(1) or real_d(*a, **k))
    c = case(name)
    x, dy = c.gpu(cuda)
    x.requires_grad_()
    w = c.w.to(cuda).requires_grad_()
    y = torch.ops.mcgmil.conv2d_f32(x, w, c.stride, c.pad)
    y64 = F.conv2d(c.x.double(), c.w.double(), None, c.stride, c.pad)
    y32 = F.conv2d(c.x, c.w, None, c.stride, c.pad)
    assert golden_util.nrel(y.detach().cpu().numpy(), y64.numpy()) <= \
        max(10.0 * golden_util.nrel(y32.numpy(), y64.numpy()), 1e-6)
    (y * dy).sum().backward(retain_graph=True)
    c.check("dw", w.grad)
    c.check("dx", x.grad)
    assert len(wgrads) == (1 if route == "native" else 0)
    assert len(dgrads) == (1 if route == "native" and c.stride == 1 else 0)
    # the backward op has no autograd formula: a backward of the backward raises
    w.grad = x.grad = None
    gx, = torch.autograd.grad((y * dy).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


# ---------------------------------------------------------------- 7. the module
LAYERS = ("conv1", "layer1.0.conv1", "layer2.0.conv1", "layer2.0.downsample.0", "layer4.1.conv2")


@functools.lru_cache(maxsize=None)
def module_case():
    """The module, one bag, and the float64 / fp32 CPU gradients of the listed convolutions for
    the step of test_gpu_head_grad.test_sgd_step_through_the_backbone (head restated in torch with
    the kernel's own masks)."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(dev)
    m.train()
    x = torch.rand(1, 3, 3, 64, 64, device=dev)
    target = torch.tensor([1], device=dev)
    seed = 99
    pf, pa = m._dropout_ps()
    offs = ops.bag_offsets_tensor([3], dev)
    keepF = torch.from_numpy(np.unpackbits(ops.feature_keep(offs, 3, 1, 512, pf, seed).cpu().numpy(), axis=1,
                                           bitorder="little").reshape(1, 3, 512))
    keepA = ops.attention_keep(offs, 3, 1, 2, pa, seed).cpu().view(1, 2, 3)

    def grads(mod, xx):
        H = mod.extract_features(xx)[0]
        Y, A = ref.head_forward(H, mod._live_head(), keepF, keepA, pf, pa)
        (F.cross_entropy(Y, target.cpu()) +
         mod.auxiliary_loss.scale * mod.auxiliary_loss(A[:, 1, :], A[:, 0, :], True)).backward()
        return {n: mod.feature_extractor.get_submodule(n).weight.grad.double().numpy() for n in LAYERS}
    g64 = grads(copy.deepcopy(m).double().cpu(), x.double().cpu())
    g32 = grads(copy.deepcopy(m).cpu(), x.cpu())
    bounds = {n: max(10.0 * golden_util.nrel(g32[n], g64[n]), 1e-6) for n in LAYERS}
    return m, x, target, seed, g64, bounds


@pytest.mark.parametrize("native,route", [(True, "native"), (True, None), (False, None)])
def test_module_train_step(cuda, native, route, monkeypatch):
    """One step with the backbone opt-in on the native backward route, on the default route
    (aten.convolution_backward behind the same op) and without the opt-in."""
    if route:
        monkeypatch.setenv("MCGMIL_CONV_GRAD", route)
    else:
        monkeypatch.delenv("MCGMIL_CONV_GRAD", raising=False)
    wgrads = []
    real_w = features.conv2d_f32_wgrad
    monkeypatch.setattr(features, "conv2d_f32_wgrad", lambda *a, **k: wgrads.append(1) or real_w(*a, **k))
    m, x, target, seed, g64, bounds = module_case()
    m = copy.deepcopy(m).train().enable_head_training()
    assert m.enable_backbone_training(native) is m
    routed = []
    real = features.conv2d_f32_op
    monkeypatch.setattr(features, "conv2d_f32_op", lambda layer, t: routed.append(layer) or real(layer, t))
    Y, A, aux = m(x, target, seed=seed)
    (F.cross_entropy(Y, target) + aux).backward()
    assert len(routed) == (19 if native else 0)                 # every convolution but the 3-channel stem
    assert len(wgrads) == (19 if route == "native" else 0)      # ... and their weight gradients on the HIP kernel
    for n in LAYERS:
        g = m.feature_extractor.get_submodule(n).weight.grad
        err = golden_util.nrel(g.cpu().numpy(), g64[n])
        print(f"opt-in={native} route={route} {n}: {err:.2e} / {bounds[n]:.2e}")
        assert bool(torch.isfinite(g).all()) and err <= bounds[n], n
    # the inference predicates still refuse a tensor autograd tracks
    conv = m.feature_extractor.layer1[0].conv1
    t = torch.zeros(1, 64, 4, 4, device=cuda).contiguous(memory_format=torch.channels_last)
    assert features.conv32_trainable(conv, t) and not features.conv32_fusable(conv, t)
    with torch.no_grad():
        assert features.conv32_fusable(conv, t)


# ---------------------------------------------------------------- 8. validation
def test_validation(cuda):
    L = _lib.load()
    x = torch.zeros(1, 64, 4, 4, device=cuda).contiguous(memory_format=torch.channels_last)
    dy = torch.zeros(1, 64, 4, 4, device=cuda).contiguous(memory_format=torch.channels_last)
    dw = torch.zeros(64, 64, 3, 3, device=cuda)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=cuda)

    def args(**kw):
        g = _lib.ConvGradArgs()
        a = g.fwd
        a.batch, a.height, a.width, a.in_channels, a.out_channels = 1, 4, 4, 64, 64
        a.kernel_h = a.kernel_w = 3
        a.stride, a.pad = 1, 1
        a.x, g.dy, g.dw = (ctypes.c_void_p(t.data_ptr()) for t in (x, dy, dw))
        g.workspace, g.workspace_bytes = ctypes.c_void_p(ws.data_ptr()), ws.numel()
        for k, v in kw.items():
            setattr(g.fwd, k, v)
        return g

    def rc_of(g):
        rc = L.mcgmil_conv2d_wgrad_f32(ctypes.byref(g), None)
        if rc:
            assert len(L.mcgmil_last_error()) > 0
        return rc
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4                # enum mcgmil_status (include/mcgmil.h)
    assert rc_of(args()) == 0
    for bad in (dict(in_channels=24), dict(stride=3), dict(pad=3), dict(pad=5),
                dict(in_ab=ctypes.c_void_p(x.data_ptr())), dict(out_channels=96), dict(kernel_h=8)):
        assert rc_of(args(**bad)) in (UNSUPPORTED, INVALID), bad
    g = args()
    g.reserved = 1
    assert rc_of(g) in (UNSUPPORTED, INVALID)
    g = args()
    n = ctypes.c_size_t()
    assert L.mcgmil_conv_wgrad_workspace_size_f32(ctypes.byref(g), ctypes.byref(n)) == 0
    assert n.value == 2 * 64 * 64 * 9 * 4                       # one granule: the running sum + one partial
    g.workspace_bytes = n.value - 1
    assert rc_of(g) == WORKSPACE
    g.workspace, g.workspace_bytes = None, 0
    assert rc_of(g) == WORKSPACE
    torch.cuda.synchronize()
