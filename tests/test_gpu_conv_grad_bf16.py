"""The bf16 convolution backward on the HIP kernels (include/mcgmil_conv_grad_bf16.h,
features.conv2d_bf16_wgrad / conv2d_bf16_dgrad, torch.ops.mcgmil.conv2d_bf16 and its backward op,
MultiHeadGatedAttentionMIL.enable_bf16_backbone_training) against float64 CPU autograd of F.conv2d.

Inputs are drawn in fp32 from a seeded generator and rounded to bf16 first; every reference is
computed from the rounded values, so what is measured is the kernel, not the rounding of its inputs.

Error of a tensor: max|got - ref| / max|ref| (golden_util.nrel). Bound of the weight gradient: 10 x
the same error of fp32 CPU autograd on that case (the project's x10 for a changed summation order,
DESIGN.md §7), at least 1e-6: products of bf16 operands are exact in fp32, so no bf16 factor is
added. The data gradient is rounded to bf16 once: elementwise |d| <= 2^-7 |ref| + B max|ref| with B
the case's fp32 bound for dx (2^-8 is bf16's unit roundoff, doubled for rounding an fp32 sum that
itself carries error B). Every test prints measured / bound before it asserts."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util
from mcgmil import MultiHeadGatedAttentionMIL, _lib, features, library  # noqa: F401
from mcgmil.resnet import deactivate_batchnorm

pytestmark = pytest.mark.gpu

G = _lib.WGRAD_GRANULE_PIXELS
CL = torch.channels_last
BF = torch.bfloat16

CASES = {
    #                   N  Cin  Cout k  s  p  H   W
    "c64_3x3_odd":     (3, 64,  64,  3, 1, 1, 9,  7),     # 189 pixels: no multiple of a K step; 64 x 256 tile
    "s2_3x3_even":     (2, 64,  128, 3, 2, 1, 10, 10),
    "s2_3x3_odd":      (2, 64,  128, 3, 2, 1, 9,  11),
    "s2_1x1":          (2, 64,  128, 1, 2, 0, 9,  10),    # 64 columns: three waves of the 128 x 128 tile idle
    "wide_in_1x1":     (1, 256, 64,  1, 1, 0, 7,  7),
    "c64_5x5":         (2, 64,  64,  5, 1, 2, 6,  7),     # generic taps
    "c192_3x3":        (1, 128, 192, 3, 1, 0, 5,  5),     # Cout no multiple of 128
    # batch * OH * OW = 2 G + G / 2 + 5: three granules, the last one ragged
    "granules":        (1, 64,  64,  3, 1, 1, 1,  2 * G + G // 2 + 5),
}
TABLE = [k for k in CASES if k != "granules"]


def _round(t):
    return t.to(BF).float()


class Case:
    """bf16-rounded inputs of a case and its float64 / fp32 CPU autograd gradients (computed once)."""

    def __init__(self, name):
        self.name = name
        N, Cin, Cout, k, s, p, H, W = CASES[name]
        self.stride, self.pad = s, p
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        self.x = _round(torch.randn(N, Cin, H, W, generator=gen))
        self.w = _round(torch.randn(Cout, Cin, k, k, generator=gen) / (Cin * k * k) ** 0.5)
        oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        self.dy = _round(torch.randn(N, Cout, oh, ow, generator=gen))
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
        ref = self.dx64
        allowed = 2.0 ** -7 * ref.abs() + self.bound_dx * ref.abs().max()
        excess = ((got.detach().cpu().double() - ref).abs() / allowed).max().item()
        print(f"{self.name} dx: max |d| / (2^-7 |ref| + {self.bound_dx:.2e} max|ref|) = {excess:.3f} / 1")
        assert excess <= 1.0, (self.name, excess)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def raw_wgrad(conv, x, dy, dw, chunk_pixels=0):
    """mcgmil_conv2d_wgrad_bf16 into a caller-owned dw (features.conv2d_bf16_wgrad allocates its own);
    returns the workspace bytes the library asked for."""
    L = _lib.load()
    g = _lib.ConvGradBf16Args()
    a = g.fwd
    a.batch, a.in_channels, a.height, a.width = x.shape
    a.out_channels, (a.kernel_h, a.kernel_w) = conv.out_channels, conv.kernel_size
    a.stride, a.pad = conv.stride[0], conv.padding[0]
    a.x, g.dy, g.dw = (ctypes.c_void_p(t.data_ptr()) for t in (x, dy, dw))
    g.chunk_pixels = chunk_pixels
    n = ctypes.c_size_t()
    _lib.check(L.mcgmil_conv_wgrad_workspace_size_bf16(ctypes.byref(g), ctypes.byref(n)), "size")
    ws = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    g.workspace, g.workspace_bytes = ctypes.c_void_p(ws.data_ptr()), n.value
    _lib.check(L.mcgmil_conv2d_wgrad_bf16(ctypes.byref(g), None), "wgrad")
    torch.cuda.synchronize()
    return n.value


# ---------------------------------------------------------------- 1. weight gradient
@pytest.mark.parametrize("name", TABLE)
def test_wgrad_parity_overwrite_and_repeat(cuda, name):
    c = case(name)
    x, dy = c.gpu(cuda)
    conv = c.conv(cuda)
    assert features.conv_bf16_trainable(conv, x), features.conv_bf16_untrainable_reason(conv, x)
    dw = torch.full(c.w.shape, float("nan"), device=cuda)
    raw_wgrad(conv, x, dy, dw)
    assert bool(torch.isfinite(dw).all())                      # NaN preset fully overwritten
    c.check_dw(dw)
    again = features.conv2d_bf16_wgrad(conv, x, dy)
    assert again.dtype == torch.float32 and again.is_contiguous() and torch.equal(again, dw)     # bitwise


# ---------------------------------------------------------------- 2. one pixel
def test_wgrad_one_pixel(cuda):
    gen = torch.Generator().manual_seed(5)
    x = _round(torch.randn(1, 64, 1, 1, generator=gen))
    dy = _round(torch.randn(1, 64, 1, 1, generator=gen))
    conv = features._ConvShim(torch.zeros(64, 64, 3, 3, device=cuda), 1, 1)
    dw = features.conv2d_bf16_wgrad(conv, x.to(cuda, BF).contiguous(memory_format=CL),
                                    dy.to(cuda, BF).contiguous(memory_format=CL)).cpu()
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
    E4 = c.w.numel() * 4
    whole = torch.full(c.w.shape, float("nan"), device=cuda)
    assert raw_wgrad(conv, x, dy, whole) == (1 + 3) * E4            # one chunk of three granules
    c.check_dw(whole)
    for chunk, granules in ((G, 1), (2 * G, 2), (1, 1)):
        got = torch.full(c.w.shape, float("nan"), device=cuda)
        assert raw_wgrad(conv, x, dy, got, chunk_pixels=chunk) == (1 + granules) * E4, chunk
        assert torch.equal(got, whole), chunk                       # bitwise, whatever the chunking
    assert torch.equal(features.conv2d_bf16_wgrad(conv, x, dy, chunk_pixels=2 * G), whole)


# ---------------------------------------------------------------- 4. stride-1 data gradient
@pytest.mark.parametrize("name", [n for n in TABLE if CASES[n][4] == 1])
def test_dgrad_on_the_flipped_forward_kernel(cuda, name, monkeypatch):
    c = case(name)
    x, dy = c.gpu(cuda)
    conv = c.conv(cuda)
    assert features.dgrad_bf16_native(conv, dy)
    calls = []
    real = features.conv2d_bf16
    monkeypatch.setattr(features, "conv2d_bf16", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    dx = features.conv2d_bf16_dgrad(conv, dy, x)
    assert len(calls) == 1                                       # the bf16 forward kernel
    assert dx.is_contiguous(memory_format=CL)
    c.check_dx(dx)


# ---------------------------------------------------------------- 5. the op on both routes
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


@pytest.mark.parametrize("name", TABLE)
def test_op_native_route(cuda, name, monkeypatch):
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "native")
    c = case(name)
    x, dy = c.gpu(cuda)
    spy = _AtenSpy(monkeypatch)

    def step():
        xx = x.clone().requires_grad_()
        w = c.w.to(cuda).requires_grad_()                        # the fp32 master weight
        y = torch.ops.mcgmil.conv2d_bf16(xx, w, c.stride, c.pad)
        y.backward(dy)
        return y, xx.grad, w.grad
    y, dx, dw = step()
    with torch.no_grad():
        assert torch.equal(y, features.conv2d(c.conv(cuda, BF), x))      # the inference kernel, bitwise
    assert dw.dtype == torch.float32 and dw.is_contiguous()
    assert dx.dtype == BF and dx.is_contiguous(memory_format=CL)
    c.check_dw(dw)
    c.check_dx(dx)
    if c.stride == 1:
        assert spy.masks == []                                   # no gradient leaves the project's kernels
    else:
        assert spy.masks and all(m == (True, False, False) for m in spy.masks), spy.masks
    # repeatable, bitwise -- what the project's kernels compute. A stride-2 dx is aten's (MIOpen's),
    # which was seen to differ in the last bit from one call to the next on an MI355X: it is held
    # to the bound again, not to equality.
    _, dx2, dw2 = step()
    assert torch.equal(dw2, dw)
    gx, gw = torch.ops.mcgmil.conv2d_bf16_backward(x, c.w.to(cuda), dy, c.stride, c.pad, False, True)
    assert gx.numel() == 0 and torch.equal(gw, dw)
    gx, gw = torch.ops.mcgmil.conv2d_bf16_backward(x, c.w.to(cuda, BF), dy, c.stride, c.pad, True, False)
    assert gw.numel() == 0 and gw.dtype == BF
    if c.stride == 1:
        assert torch.equal(dx2, dx) and torch.equal(gx, dx)
    else:
        c.check_dx(dx2)
        c.check_dx(gx)


def test_op_direct_means_native(cuda, monkeypatch):
    c = case("c64_3x3_odd")
    x, dy = c.gpu(cuda)
    w = c.w.to(cuda)
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "native")
    want = torch.ops.mcgmil.conv2d_bf16_backward(x, w, dy, c.stride, c.pad, True, True)
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "direct")
    got = torch.ops.mcgmil.conv2d_bf16_backward(x, w, dy, c.stride, c.pad, True, True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("route", ["aten", None, "bogus"])
@pytest.mark.parametrize("name", ["c64_3x3_odd", "s2_3x3_odd"])
def test_op_aten_route(cuda, name, route, monkeypatch):
    """The default route: the yardstick is aten itself, so only shapes, dtypes, layouts, the calls
    and the forward are asserted."""
    if route:
        monkeypatch.setenv("MCGMIL_CONV_GRAD", route)
    else:
        monkeypatch.delenv("MCGMIL_CONV_GRAD", raising=False)
    c = case(name)
    x, dy = c.gpu(cuda)
    wgrads = []
    real_w = features.conv2d_bf16_wgrad
    monkeypatch.setattr(features, "conv2d_bf16_wgrad", lambda *a, **k: wgrads.append(1) or real_w(*a, **k))
    spy = _AtenSpy(monkeypatch)
    xx = x.clone().requires_grad_()
    w = c.w.to(cuda).requires_grad_()
    y = torch.ops.mcgmil.conv2d_bf16(xx, w, c.stride, c.pad)
    with torch.no_grad():
        assert torch.equal(y, features.conv2d(c.conv(cuda, BF), x))
    assert y.dtype == BF and y.is_contiguous(memory_format=CL)
    y.backward(dy, retain_graph=True)
    assert spy.masks == [(True, True, False)] and wgrads == []
    assert w.grad.dtype == torch.float32 and w.grad.shape == w.shape and w.grad.is_contiguous()
    assert xx.grad.dtype == BF and xx.grad.shape == x.shape and xx.grad.is_contiguous(memory_format=CL)
    # the backward op has no autograd formula: a backward of the backward raises
    gx, = torch.autograd.grad(y, xx, dy, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.float().sum().backward()


# ---------------------------------------------------------------- 6. the module
def _step(m, x, target, seed, autocast=False):
    """One step's gradients {parameter name: fp64 numpy} and (Y, A)."""
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", BF, enabled=autocast):
        Y, A, aux = m(x, target, seed=seed)
    (F.cross_entropy(Y.float(), target) + aux.float()).backward()
    grads = {n: p.grad for n, p in m.named_parameters()}
    return grads, Y.detach(), A.detach()


def _drift(got, ref, scale):
    """nrel of a gradient against the fp32 step's. A reference gradient below 1e-6 of the largest
    gradient of the model is the rounding residue of a quantity that is zero in exact arithmetic
    (the bias of an attention score: softmax does not see it), and a ratio of two residues measures
    nothing: such a parameter is measured against the model-wide scale instead."""
    ref = ref.double().cpu().numpy()
    den = np.abs(ref).max()
    if den >= 1e-6 * scale:
        return golden_util.nrel(got.double().cpu().numpy(), ref)
    return float(np.abs(got.double().cpu().numpy() - ref).max() / scale)


@functools.lru_cache(maxsize=None)
def module_case():
    """The module, one bag, and the yardsticks: the gradients of the same step in fp32 on the torch
    layers, and those of the user's own autocast over the torch layers."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(7)
    m = MultiHeadGatedAttentionMIL(num_classes=2, backbone="r18", pretrained=False).to(dev)
    m.apply(deactivate_batchnorm)
    m.train().enable_head_training()
    x = torch.rand(1, 6, 3, 96, 96, device=dev)
    target = torch.tensor([1], device=dev)
    seed = 1234
    g32, Y32, A32 = _step(copy.deepcopy(m), x, target, seed)
    gac, _, _ = _step(copy.deepcopy(m), x, target, seed, autocast=True)
    return m, x, target, seed, g32, gac, (Y32, A32)


@pytest.mark.parametrize("route", ["native", None])
def test_module_train_step(cuda, route, monkeypatch):
    if route:
        monkeypatch.setenv("MCGMIL_CONV_GRAD", route)
    else:
        monkeypatch.delenv("MCGMIL_CONV_GRAD", raising=False)
    m0, x, target, seed, g32, gac, _ = module_case()
    m = copy.deepcopy(m0)
    assert m.enable_bf16_backbone_training() is m
    routed, wgrads = [], []
    real, real_w = features.conv2d_bf16_op, features.conv2d_bf16_wgrad
    monkeypatch.setattr(features, "conv2d_bf16_op", lambda layer, t: routed.append(layer) or real(layer, t))
    monkeypatch.setattr(features, "conv2d_bf16_wgrad", lambda *a, **k: wgrads.append(1) or real_w(*a, **k))
    grads, _, _ = _step(m, x, target, seed)
    assert len(routed) == 19                                     # every convolution but the 3-channel stem
    assert len(wgrads) == (19 if route == "native" else 0)
    convs = {n + ".weight" for n, mod in m.named_modules() if isinstance(mod, torch.nn.Conv2d)}
    scale = max(float(g.abs().max()) for g in g32.values())
    rows = []
    for n, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any()), n
        if n in convs:
            assert g.dtype == torch.float32, n
        err, yard = _drift(g, g32[n], scale), _drift(gac[n], g32[n], scale)
        bound = 2.0 * yard + 1e-3
        rows.append((n, err, bound))
        print(f"route={route} {n}: {err:.2e} / {bound:.2e} (autocast over the torch layers: {yard:.2e})")
    for n, err, bound in rows:
        assert err <= bound, (n, err, bound)
    worst = max(err / bound for _, err, bound in rows)
    print(f"route={route}: worst drift / bound = {worst:.3f}")


def test_module_flag_off_and_eval_are_unchanged(cuda, monkeypatch):
    """Flag off, eval mode and no_grad: no convolution is routed to the op. In eval mode and under
    no_grad (the project's inference kernels, which repeat bitwise) the outputs are bitwise those of
    a model that never had the flag set. The fp32 training forward on the torch layers does not
    repeat bitwise from one call to the next on an MI355X, flag or no flag (features differ by
    about 4e-6 between two calls of the parent commit's code), so there the flag-off output is held
    to 10 x the difference of two steps of the never-flagged model, at least 1e-6 of max|Y|."""
    m0, x, target, seed, _, _, _ = module_case()
    _, Ya, Aa = _step(copy.deepcopy(m0), x, target, seed)       # a model that never had the flag set
    _, Yb, Ab = _step(copy.deepcopy(m0), x, target, seed)       # ... and its own repeat error
    routed = []
    real = features.conv2d_bf16_op
    monkeypatch.setattr(features, "conv2d_bf16_op", lambda layer, t: routed.append(layer) or real(layer, t))
    m = copy.deepcopy(m0).enable_bf16_backbone_training()
    assert m.enable_bf16_backbone_training(False) is m
    feats = []
    m.feature_extractor.register_forward_hook(lambda mod, a, out: feats.append(out.dtype))
    _, Y, A = _step(m, x, target, seed)                          # flag off again: the fp32 torch layers
    assert routed == [] and feats == [torch.float32]
    for name, got, a, b in (("Y", Y, Ya, Yb), ("A", A, Aa, Ab)):
        bound = max(10.0 * float((a - b).abs().max()), 1e-6 * float(a.abs().max()))
        err = float((got - a).abs().max())
        print(f"flag off, train mode {name}: {err:.2e} / {bound:.2e}")
        assert err <= bound, name
    never = copy.deepcopy(m0).eval()
    flagged = copy.deepcopy(m0).enable_bf16_backbone_training().eval()
    Ye, Ae, _ = never(x, target)
    Yf, Af, _ = flagged(x, target)
    assert routed == [] and torch.equal(Yf, Ye) and torch.equal(Af, Ae)
    with torch.no_grad():                                        # train mode, no graph: the inference path
        Yn, An, _ = flagged(x, target)
        Ym, Am, _ = never(x, target)
    assert routed == [] and torch.equal(Yn, Ym) and torch.equal(An, Am)


# ---------------------------------------------------------------- 7. validation
def test_validation(cuda):
    L = _lib.load()
    x = torch.zeros(1, 64, 4, 4, device=cuda, dtype=BF).contiguous(memory_format=CL)
    dy = torch.zeros(1, 64, 4, 4, device=cuda, dtype=BF).contiguous(memory_format=CL)
    dw = torch.zeros(64, 64, 3, 3, device=cuda)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=cuda)

    def args(**kw):
        g = _lib.ConvGradBf16Args()
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
        rc = L.mcgmil_conv2d_wgrad_bf16(ctypes.byref(g), None)
        if rc:
            assert len(L.mcgmil_last_error()) > 0
        return rc
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4                # enum mcgmil_status (include/mcgmil.h)
    assert rc_of(args()) == 0
    for bad in (dict(in_channels=48), dict(in_channels=16), dict(stride=3), dict(pad=3), dict(pad=5),
                dict(in_ab=ctypes.c_void_p(x.data_ptr())), dict(out_channels=96), dict(kernel_h=8)):
        assert rc_of(args(**bad)) in (UNSUPPORTED, INVALID), bad
    g = args()
    g.reserved = 1
    assert rc_of(g) in (UNSUPPORTED, INVALID)
    g = args()
    n = ctypes.c_size_t()
    assert L.mcgmil_conv_wgrad_workspace_size_bf16(ctypes.byref(g), ctypes.byref(n)) == 0
    assert n.value == 2 * 64 * 64 * 9 * 4                       # one granule: the running sum + one partial
    g.workspace_bytes = n.value - 1
    assert rc_of(g) == WORKSPACE
    g.workspace, g.workspace_bytes = None, 0
    assert rc_of(g) == WORKSPACE
    torch.cuda.synchronize()
