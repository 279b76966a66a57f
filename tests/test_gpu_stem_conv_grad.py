"""The fp32 weight gradient of the stem convolution on the HIP kernel (include/mcgmil_stem_grad.h,
features.conv2d_f32_stem_wgrad, torch.ops.mcgmil.stem_conv_f32 and its backward op,
MultiHeadGatedAttentionMIL.enable_backbone_training(stem_conv=True)) against float64 CPU autograd
of F.conv2d.

Error of a tensor: max|got - ref| / max|ref| (golden_util.nrel). Bound: 10 x the same error of
fp32 CPU autograd on that case (the project's x10 for a changed summation order),
at least 1e-6. Every test prints measured / bound before it asserts. Outputs and the workspace
handed to the C ABI are pre-filled with NaN, every device call is made twice and compared bitwise,
and no element is excused."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import golden_util
from mcgmil import _lib, features, library  # noqa: F401

pytestmark = pytest.mark.gpu

G = _lib.WGRAD_GRANULE_PIXELS
CL = torch.channels_last

CASES = {
    #            N  Cin H   W    kh kw s  p  Cout
    "tiny":     (1, 3,  7,  7,   7, 7, 2, 3, 64),     # 16 pixels; every window clipped on some side
    "odd":      (2, 3,  13, 11,  7, 7, 2, 3, 64),     # 84 pixels: no multiple of a K step; odd H, W
    "granules": (3, 3,  96, 100, 7, 7, 2, 3, 64),     # 7,200 pixels: 4 granules, the last 1,056
    "c1":       (2, 1,  9,  10,  3, 3, 1, 1, 64),     # one channel; stride 1
    "c4":       (2, 4,  10, 12,  5, 5, 2, 2, 128),    # two output tiles; 16-byte pixels
    "short":    (1, 2,  8,  9,   7, 7, 1, 0, 64),     # 6 pixels: less than one K step
    "widest":   (1, 4,  8,  8,   7, 7, 2, 3, 64),     # 196 columns, the most the entry admits
    "rect":     (1, 3,  9,  12,  3, 7, 2, 1, 64),     # kh != kw
}
PIXELS = {"tiny": 16, "odd": 84, "granules": 7200, "short": 6}


class Case:
    """Inputs of a case and its float64 / fp32 CPU autograd gradients (computed once)."""

    def __init__(self, name):
        self.name = name
        N, Cin, H, W, kh, kw, s, p, Cout = CASES[name]
        self.stride, self.pad = s, p
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        self.x = torch.randn(N, Cin, H, W, generator=gen)
        self.w = torch.randn(Cout, Cin, kh, kw, generator=gen) / (Cin * kh * kw) ** 0.5
        oh, ow = (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1
        self.pixels = N * oh * ow
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
        return self.x.to(dev).contiguous(memory_format=CL), self.dy.to(dev).contiguous(memory_format=CL)

    def check(self, what, got):
        want = self.dw64 if what == "dw" else self.dx64
        bound = self.bound_dw if what == "dw" else self.bound_dx
        err = golden_util.nrel(got.detach().cpu().numpy(), want.numpy())
        print(f"{self.name} {what}: {err:.2e} / {bound:.2e}")
        assert tuple(got.shape) == tuple(want.shape)
        assert bool(torch.isfinite(got).all())
        assert err <= bound, (self.name, what, err, bound)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def raw_wgrad(conv, x, dy, chunk_pixels=0):
    """mcgmil_stem_wgrad_f32 into a NaN-filled dw with a NaN-filled workspace -> (dw, workspace bytes)."""
    L = _lib.load()
    g = _lib.ConvGradArgs()
    a = g.fwd
    a.batch, a.in_channels, a.height, a.width = x.shape
    a.out_channels, (a.kernel_h, a.kernel_w) = conv.out_channels, conv.kernel_size
    a.stride, a.pad = conv.stride[0], conv.padding[0]
    dw = torch.full(tuple(conv.weight.shape), float("nan"), device=x.device)
    a.x, g.dy, g.dw = (ctypes.c_void_p(t.data_ptr()) for t in (x, dy, dw))
    g.chunk_pixels = chunk_pixels
    n = ctypes.c_size_t()
    _lib.check(L.mcgmil_stem_wgrad_workspace_size_f32(ctypes.byref(g), ctypes.byref(n)), "size")
    assert n.value % 4 == 0
    ws = torch.full((n.value // 4,), float("nan"), device=x.device)
    g.workspace, g.workspace_bytes = ctypes.c_void_p(ws.data_ptr()), n.value
    _lib.check(L.mcgmil_stem_wgrad_f32(ctypes.byref(g), None), "stem wgrad")
    torch.cuda.synchronize()
    return dw, n.value


# ---------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("name", list(CASES))
def test_wgrad_parity_overwrite_and_repeat(cuda, name):
    c = case(name)
    if name in PIXELS:
        assert c.pixels == PIXELS[name]
    x, dy = c.gpu(cuda)
    conv = c.conv(cuda)
    assert features.stem_conv_trainable(conv, x) and not features.conv32_trainable(conv, x)
    dw, _ = raw_wgrad(conv, x, dy)
    c.check("dw", dw)                                           # NaN preset fully overwritten
    again, _ = raw_wgrad(conv, x, dy)
    assert torch.equal(again, dw)                               # bitwise
    mine = features.conv2d_f32_stem_wgrad(conv, x, dy)
    assert mine.is_contiguous() and torch.equal(mine, dw)


def test_wgrad_chunking_is_bitwise_invariant(cuda):
    c = case("granules")
    assert c.pixels == 3 * G + 1056
    x, dy = c.gpu(cuda)
    conv = c.conv(cuda)
    E = 64 * 147
    whole, n_whole = raw_wgrad(conv, x, dy)
    c.check("dw", whole)
    assert n_whole == (1 + 4) * E * 4
    for chunk, granules in ((G, 1), (2 * G, 2)):
        for _ in range(2):
            got, n = raw_wgrad(conv, x, dy, chunk_pixels=chunk)
            assert n == (1 + granules) * E * 4                  # the workspace follows chunk_pixels
            assert torch.equal(got, whole), chunk
    assert torch.equal(features.conv2d_f32_stem_wgrad(conv, x, dy, chunk_pixels=2 * G), whole)


def test_byte_offsets_past_2_to_31(cuda):
    """33 images of 3 x 1024^2 in the stem geometry: dy is 33 x 512^2 x 64 fp32 = 2^31 + 2^26 bytes
    and the last image's dy starts exactly at byte 2^31. dy is zero except there and x random only
    there, so dW is that image's weight gradient: wrong 32-bit offsets would read zeros."""
    N, H, Cout = 33, 1024, 64
    gen = torch.Generator().manual_seed(11)
    xl = torch.randn(1, 3, H, H, generator=gen)
    dyl = torch.randn(1, Cout, H // 2, H // 2, generator=gen)
    x = torch.zeros(N, 3, H, H, device=cuda).contiguous(memory_format=CL)
    dy = torch.zeros(N, Cout, H // 2, H // 2, device=cuda).contiguous(memory_format=CL)
    assert dy.numel() * 4 > 2 ** 31 and (N - 1) * dy[0].numel() * 4 >= 2 ** 31
    x[N - 1:] = xl.to(cuda)
    dy[N - 1:] = dyl.to(cuda)
    conv = features._ConvShim(torch.zeros(Cout, 3, 7, 7, device=cuda), 2, 3)
    dw, _ = raw_wgrad(conv, x, dy)
    again, _ = raw_wgrad(conv, x, dy)
    assert torch.equal(again, dw)
    del x, dy

    def cpu(dt):
        w = torch.zeros(Cout, 3, 7, 7, dtype=dt, requires_grad=True)
        F.conv2d(xl.to(dt), w, None, 2, 3).backward(dyl.to(dt))
        return w.grad
    want = cpu(torch.float64)
    bound = max(10.0 * golden_util.nrel(cpu(torch.float32).numpy(), want.numpy()), 1e-6)
    err = golden_util.nrel(dw.cpu().numpy(), want.numpy())
    print(f"past 2^31 bytes dw: {err:.2e} / {bound:.2e}")
    assert bool(torch.isfinite(dw).all()) and err <= bound


def test_validation(cuda):
    L = _lib.load()
    x = torch.zeros(1, 3, 8, 8, device=cuda).contiguous(memory_format=CL)
    dy = torch.zeros(1, 64, 4, 4, device=cuda).contiguous(memory_format=CL)
    dw = torch.zeros(64, 3, 7, 7, device=cuda)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=cuda)

    def args(**kw):
        g = _lib.ConvGradArgs()
        a = g.fwd
        a.batch, a.height, a.width, a.in_channels, a.out_channels = 1, 8, 8, 3, 64
        a.kernel_h = a.kernel_w = 7
        a.stride, a.pad = 2, 3
        a.x, g.dy, g.dw = (ctypes.c_void_p(t.data_ptr()) for t in (x, dy, dw))
        g.workspace, g.workspace_bytes = ctypes.c_void_p(ws.data_ptr()), ws.numel()
        for k, v in kw.items():
            setattr(g.fwd, k, v)
        return g

    def rc_of(g):
        rc = L.mcgmil_stem_wgrad_f32(ctypes.byref(g), None)
        if rc:
            assert len(L.mcgmil_last_error()) > 0
        return rc
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4                # enum mcgmil_status (include/mcgmil.h)
    assert rc_of(args()) == 0
    for bad in (dict(in_channels=0), dict(in_channels=5), dict(in_channels=16), dict(out_channels=96),
                dict(kernel_h=8), dict(stride=3), dict(kernel_h=3, kernel_w=3, pad=3),
                dict(in_ab=ctypes.c_void_p(x.data_ptr()))):
        assert rc_of(args(**bad)) in (UNSUPPORTED, INVALID), bad
    g = args()
    g.reserved = 1
    assert rc_of(g) in (UNSUPPORTED, INVALID)
    g = args()
    n = ctypes.c_size_t()
    assert L.mcgmil_stem_wgrad_workspace_size_f32(ctypes.byref(g), ctypes.byref(n)) == 0
    assert n.value == 2 * 64 * 147 * 4                          # one granule: the running sum + one partial
    g.workspace_bytes = n.value - 1
    assert rc_of(g) == WORKSPACE
    g.workspace, g.workspace_bytes = None, 0
    assert rc_of(g) == WORKSPACE
    torch.cuda.synchronize()
    conv = features._ConvShim(torch.zeros(64, 16, 3, 3, device=cuda), 1, 1)
    x16 = torch.zeros(1, 16, 4, 4, device=cuda).contiguous(memory_format=CL)
    with pytest.raises(ValueError):
        features.conv2d_f32_stem_wgrad(conv, x16, torch.zeros(1, 64, 4, 4, device=cuda))


# ---------------------------------------------------------------- 2. the ops
@pytest.mark.parametrize("name", ["odd", "c4"])
def test_opcheck(cuda, name):
    c = case(name)
    x, dy = c.gpu(cuda)
    w = c.w.to(cuda)
    torch.library.opcheck(torch.ops.mcgmil.stem_conv_f32.default,
                          (x.clone().requires_grad_(), w.clone().requires_grad_(), c.stride, c.pad))
    torch.library.opcheck(torch.ops.mcgmil.stem_conv_f32_backward.default, (x, w, dy, c.stride, c.pad, True, True))
    torch.library.opcheck(torch.ops.mcgmil.stem_conv_f32_backward.default, (x, w, dy, c.stride, c.pad, False, True))


@pytest.mark.parametrize("name", ["odd", "c4"])
def test_forward_is_the_inference_kernel_and_autograd_matches_float64(cuda, name, monkeypatch):
    wgrads = []
    real_w = features.conv2d_f32_stem_wgrad
    monkeypatch.setattr(features, "conv2d_f32_stem_wgrad", lambda *a, **k: wgrads.append(1) or real_w(*a, **k))
    c = case(name)
    x, dy = c.gpu(cuda)
    w = c.w.to(cuda).requires_grad_()
    with torch.no_grad():
        want = features.conv2d_f32(c.conv(cuda), x)
    # the weight alone: no data gradient is computed
    y = torch.ops.mcgmil.stem_conv_f32(x, w, c.stride, c.pad)
    assert y.is_contiguous(memory_format=CL) and torch.equal(y, want)       # bitwise
    (y * dy).sum().backward()
    assert len(wgrads) == 1 and x.grad is None
    c.check("dw", w.grad)
    first = w.grad.clone()
    # x as well
    w.grad = None
    x.requires_grad_()
    y = torch.ops.mcgmil.stem_conv_f32(x, w, c.stride, c.pad)
    assert torch.equal(y, want)
    (y * dy).sum().backward(retain_graph=True)
    assert len(wgrads) == 2 and torch.equal(w.grad, first)
    c.check("dx", x.grad)
    # the backward op has no autograd formula: a backward of the backward raises
    gw, = torch.autograd.grad((y * dy).sum(), w, create_graph=True)
    with pytest.raises(RuntimeError):
        gw.sum().backward()
    with pytest.raises((RuntimeError, ValueError)):
        torch.ops.mcgmil.stem_conv_f32(c.x, c.w, c.stride, c.pad)           # no CPU kernel


# ---------------------------------------------------------------- 3. routing
def _spy(monkeypatch):
    routed = []
    real = features.stem_conv_f32_op
    monkeypatch.setattr(features, "stem_conv_f32_op", lambda layer, t: routed.append(layer) or real(layer, t))
    return routed


def test_run_conv_routes_inside_the_context_only(cuda, monkeypatch):
    routed = _spy(monkeypatch)
    conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False).to(cuda)
    x = torch.randn(2, 3, 16, 16, device=cuda)                              # not channels-last: made so
    assert not features.conv32_trainable(conv1, x.contiguous(memory_format=CL))
    assert features.stem_conv_trainable(conv1, x.contiguous(memory_format=CL))
    y0 = features.run_conv(conv1, x)
    with features.native_conv_training():
        features.run_conv(conv1, x)
    assert not routed
    with features.native_stem_conv_training():
        y1 = features.run_conv(conv1, x)
        assert routed == [conv1]
        with torch.no_grad():
            features.run_conv(conv1, x)
        features.run_conv(nn.Conv2d(3, 64, 7, 2, 3, bias=True).to(cuda), x)  # a bias
        features.run_conv(nn.Conv2d(3, 32, 7, 2, 3, bias=False).to(cuda), x)  # out_channels % 64
        assert len(routed) == 1
    features.run_conv(conv1, x)
    assert len(routed) == 1
    y64 = F.conv2d(x.double().cpu(), conv1.weight.detach().double().cpu(), None, 2, 3)
    y32 = F.conv2d(x.cpu(), conv1.weight.detach().cpu(), None, 2, 3)
    bound = max(10.0 * golden_util.nrel(y32.numpy(), y64.numpy()), 1e-6)
    for name, y in (("torch layer", y0), ("op", y1)):
        err = golden_util.nrel(y.detach().cpu().numpy(), y64.numpy())
        print(f"run_conv {name}: {err:.2e} / {bound:.2e}")
        assert err <= bound
    y1.sum().backward()
    assert conv1.weight.grad is not None and bool(torch.isfinite(conv1.weight.grad).all())


# ---------------------------------------------------------------- 4. the module
PARAMS = ("feature_extractor.conv1.weight", "feature_extractor.layer1.0.conv1.weight", "classifiers.0.weight")


@pytest.mark.parametrize("kw", [dict(stem_conv=True), dict(norm=True, stem=True, stem_conv=True)],
                         ids=["stem_conv", "norm+stem+stem_conv"])
def test_module_train_step_with_the_stem_conv_opt_in(cuda, kw, monkeypatch):
    """The r18 step of test_gpu_stem_grad.module_case (3 instances of 64 x 64, deactivate_batchnorm
    state, MODULE_SEED chosen on the CPU so that no ReLU pre-activation of the float64 backbone is
    within 1e-5 of zero: a changed forward route must not flip a mask)."""
    import test_gpu_bn_grad as TB
    import test_gpu_stem_grad as TS
    m0, x, target, seed, g64, bounds, margin, gap = TS.module_case()
    print(f"float64 backbone: smallest |pre-activation| {margin:.2e}, smallest stem pool top-two gap {gap:.2e}")
    assert margin >= 1e-5 and gap >= 1e-5
    routed = _spy(monkeypatch)
    convs = []
    real = features.conv2d_f32_op
    monkeypatch.setattr(features, "conv2d_f32_op", lambda layer, t: convs.append(layer) or real(layer, t))
    m = copy.deepcopy(m0).train().enable_head_training()
    assert m.enable_backbone_training(**kw) is m
    named = TB._step(m, x, target, seed)
    assert routed == [m.feature_extractor.conv1] and len(convs) == 19
    for n in PARAMS:
        g = named[n].grad
        err = float((g.double().cpu() - g64[n]).abs().max() / g64[n].abs().max())
        print(f"{kw} {n}: {err:.2e} / {bounds[n]:.2e}")
        assert bool(torch.isfinite(g).all()) and err <= bounds[n], n
    # without the keyword, and with the flag off: never routed
    del routed[:], convs[:]
    m = copy.deepcopy(m0).train().enable_head_training().enable_backbone_training(stem_conv=False)
    TB._step(m, x, target, seed)
    assert not routed and len(convs) == 19
    del convs[:]
    m = copy.deepcopy(m0).train().enable_head_training().enable_backbone_training(False, stem_conv=True)
    TB._step(m, x, target, seed)
    assert not routed and not convs                   # the flag off: no convolution on the ops
