"""fp32 training on split-bf16 MFMA on the GPU (include/mcgmil_conv_grad_x3.h,
features.conv2d_f32x3_wgrad / _dgrad / _backward, torch.ops.mcgmil.conv2d_f32x3,
MultiHeadGatedAttentionMIL.enable_bf16x3_backbone_training).

References (tests/conv_grad_x3_ref.py, tests/test_conv_grad_x3_host.py checks them without a GPU):
the three-term emulation with fp64 sums -- products of bf16 terms are exact in fp32, so the kernel
differs from it by its fp32 accumulation alone: max|d| / max|ref| at most 10 x the same error of
fp32 CPU autograd on the case, at least 1e-6, the project's yardstick for a changed summation order
-- and the fp64 gradient of the unsplit operands, elementwise within the split's derived worst
case 3 * 2^-16 * wgrad(|dY|, |x|) plus that bound * max|ref|. Every test prints measured / bound
before it asserts.

Module step, measured on an MI355X (r18, 3 instances of 64 x 64, norm / stem / stem_conv on; error
of weight.grad against the float64 CPU step, max|d| / max|ref|):

    layer                   bf16x3     bf16 step (1/32 of it is the bound)   exact fp32 opt-in (aten and direct alike)
    conv1                   8.16e-05   6.31e-01                              8.28e-03
    layer1.0.conv1          7.91e-05   6.23e-01                              9.69e-03
    layer2.0.conv1          9.03e-05   5.12e-01                              1.14e-02
    layer2.0.downsample.0   6.66e-05   3.69e-01                              2.27e-02
    layer4.1.conv2          1.39e-04   6.35e-01                              1.79e-05

("fp32 convolution backward on split bf16", has the tables and what the figures of the
exact opt-in mean.)
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_grad_x3_ref as ref
import golden_util
import test_gpu_conv_grad as base
from conv_grad_x3_ref import HI_ONLY_RATIO, SPLIT_BOUND
from mcgmil import _lib, features, library  # noqa: F401
from mcgmil.resnet import deactivate_batchnorm

pytestmark = pytest.mark.gpu

G = _lib.WGRAD_GRANULE_PIXELS
CL = torch.channels_last
TABLE = [n for n in ref.NAMES if n != "granules"]
STRIDE1 = [n for n in TABLE if ref.CASES[n][4] == 1]
STRIDE2 = [n for n in TABLE if ref.CASES[n][4] == 2]


def gpu(c, dev):
    return (c.x.to(dev).contiguous(memory_format=CL), c.dy.to(dev).contiguous(memory_format=CL),
            features._ConvShim(c.w.to(dev), c.stride, c.pad))


def raw_args(conv, x, dy, dw, chunk_pixels=0):
    g = _lib.ConvGradArgs()
    a = g.fwd
    a.batch, a.in_channels, a.height, a.width = x.shape
    a.out_channels, (a.kernel_h, a.kernel_w) = conv.out_channels, conv.kernel_size
    a.stride, a.pad = conv.stride[0], conv.padding[0]
    a.x, g.dy, g.dw = (ctypes.c_void_p(t.data_ptr()) for t in (x, dy, dw))
    g.chunk_pixels = chunk_pixels
    return g


def raw_wgrad(conv, x, dy, dw, chunk_pixels=0):
    """mcgmil_conv2d_wgrad_f32x3 into a caller-owned dw; returns the workspace bytes it asked for."""
    L = _lib.load()
    g = raw_args(conv, x, dy, dw, chunk_pixels)
    n = ctypes.c_size_t()
    _lib.check(L.mcgmil_conv_wgrad_workspace_size_f32x3(ctypes.byref(g), ctypes.byref(n)), "size")
    ws = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    g.workspace, g.workspace_bytes = ctypes.c_void_p(ws.data_ptr()), n.value
    _lib.check(L.mcgmil_conv2d_wgrad_f32x3(ctypes.byref(g), None), "wgrad")
    torch.cuda.synchronize()
    return n.value


def check_dw(c, dw):
    """The three conditions of the weight gradient on a case."""
    got = dw.double().cpu()
    assert tuple(got.shape) == tuple(c.dw64.shape)
    err = ref.nrel(got, c.dw_emu)
    print(f"{c.name} dw vs emulation: {err:.2e} / {c.bound_dw:.2e}")
    assert err <= c.bound_dw
    d = (got - c.dw64).abs()
    lim = SPLIT_BOUND * c.dw_mag + c.bound_dw * float(c.dw64.abs().max())
    print(f"{c.name} dw vs fp64: max excess {float((d - lim).max()):.2e} (max |d| {float(d.max()):.2e})")
    assert bool((d <= lim).all())
    n3, n1 = ref.nrel(got, c.dw64), ref.nrel(c.dw_hi, c.dw64)
    print(f"{c.name} dw vs fp64: {n3:.2e} / {HI_ONLY_RATIO * n1:.2e} (hi * hi only: {n1:.2e})")
    assert n3 <= HI_ONLY_RATIO * n1                       # the lo products are in


# ---------------------------------------------------------------- 1. weight gradient
@pytest.mark.parametrize("name", ref.NAMES)
def test_wgrad_parity_overwrite_and_repeat(cuda, name):
    c = ref.case(name)
    x, dy, conv = gpu(c, cuda)
    assert features.conv32x3_trainable(conv, x)
    dw = torch.full(c.w.shape, float("nan"), device=cuda)
    raw_wgrad(conv, x, dy, dw)
    assert bool(torch.isfinite(dw).all())                      # NaN preset fully overwritten
    check_dw(c, dw)
    again = features.conv2d_f32x3_wgrad(conv, x, dy)
    assert again.is_contiguous() and again.dtype == torch.float32 and torch.equal(again, dw)     # bitwise
    exact = features.conv2d_f32_wgrad(conv, x, dy)
    assert not torch.equal(exact, dw)                          # not the exact kernel under another name


# ---------------------------------------------------------------- 2. one pixel
def test_wgrad_one_pixel(cuda):
    c = ref.case("one_pixel")
    x, dy, conv = gpu(c, cuda)
    dw = features.conv2d_f32x3_wgrad(conv, x, dy).cpu()
    centre, want, mag = dw[:, :, 1, 1].double(), c.dw64[:, :, 1, 1], c.dw_mag[:, :, 1, 1]
    d = (centre - want).abs()
    lim = SPLIT_BOUND * mag + c.bound_dw * float(want.abs().max())
    print(f"one pixel centre tap: max |d| {float(d.max()):.2e}, max excess over the bound {float((d - lim).max()):.2e}")
    assert bool((d <= lim).all())
    off = dw.clone()
    off[:, :, 1, 1] = 0
    assert not bool(off.any())                                  # the eight other taps: exactly 0


# ---------------------------------------------------------------- 3. granules
def test_wgrad_granules_and_chunking(cuda):
    c = ref.case("granules")
    x, dy, conv = gpu(c, cuda)
    assert dy.shape[0] * dy.shape[2] * dy.shape[3] == 2 * G + G // 2 + 5
    E = c.w.numel()
    whole = torch.full(c.w.shape, float("nan"), device=cuda)
    assert raw_wgrad(conv, x, dy, whole) == (1 + 3) * E * 4
    check_dw(c, whole)
    for chunk, granules in ((G, 1), (2 * G, 2), (1, 1)):
        chunked = torch.full(c.w.shape, float("nan"), device=cuda)
        assert raw_wgrad(conv, x, dy, chunked, chunk_pixels=chunk) == (1 + granules) * E * 4, chunk
        assert torch.equal(chunked, whole), chunk               # bitwise, whatever the chunking
    assert torch.equal(features.conv2d_f32x3_wgrad(conv, x, dy, chunk_pixels=2 * G), whole)


# ---------------------------------------------------------------- 4. data gradient
@pytest.mark.parametrize("name", STRIDE1)
def test_dgrad_stride_1_on_the_x3_forward_kernel(cuda, name, monkeypatch):
    c = ref.case(name)
    x, dy, conv = gpu(c, cuda)
    calls = []
    real = features.conv2d_f32
    monkeypatch.setattr(features, "conv2d_f32", lambda *a, **k: calls.append(k) or real(*a, **k))
    dx = features.conv2d_f32x3_dgrad(conv, dy, x.shape)
    assert calls == [{"precision": "bf16x3"}]
    assert dx.shape == x.shape and dx.dtype == torch.float32 and dx.is_contiguous(memory_format=CL)
    dx64, emu, mag = c.dx
    got = dx.double().cpu()
    err = (got - emu).abs()
    lim = 2e-6 * emu.abs() + 1e-5 * mag + 1e-30
    print(f"{name} dx vs emulation: max excess {float((err - lim).max()):.2e}, nrel {ref.nrel(got, emu):.2e}")
    assert bool((err <= lim).all())
    err = (got - dx64).abs()
    lim = 2e-6 * dx64.abs() + (SPLIT_BOUND + 1e-5) * mag + 1e-30
    print(f"{name} dx vs fp64: max excess {float((err - lim).max()):.2e}, nrel {ref.nrel(got, dx64):.2e}")
    assert bool((err <= lim).all())
    assert torch.equal(features.conv2d_f32x3_dgrad(conv, dy, x.shape), dx)


@pytest.mark.parametrize("name", STRIDE2)
def test_dgrad_stride_2_is_the_exact_direct_kernel(cuda, name):
    c = ref.case(name)
    x, dy, conv = gpu(c, cuda)
    dx = features.conv2d_f32x3_dgrad(conv, dy, x.shape)
    assert torch.equal(dx, features.conv2d_f32_dgrad_direct(conv, dy, x.shape))


# ---------------------------------------------------------------- 5. the op
@pytest.mark.parametrize("name", ["c64_3x3_odd", "s2_3x3_odd", "c32_5x5"])
def test_the_op_and_its_autograd(cuda, name, monkeypatch):
    c = ref.case(name)
    x, dy, conv = gpu(c, cuda)
    w = c.w.to(cuda)
    monkeypatch.delenv("MCGMIL_CONV_GRAD", raising=False)
    with torch.no_grad():
        want_y = features.conv2d_f32(conv, x, precision="bf16x3")
        want_dx, want_dw = features.conv2d_f32x3_backward(conv, x, dy)
        exact_y = features.conv2d_f32(conv, x)
    assert not torch.equal(want_y, exact_y)
    for route in (None, "native", "direct"):
        if route:
            monkeypatch.setenv("MCGMIL_CONV_GRAD", route)
        xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = torch.ops.mcgmil.conv2d_f32x3(xr, wr, c.stride, c.pad)
        assert torch.equal(y, want_y) and y.is_contiguous(memory_format=CL), route
        (y * dy).sum().backward()
        assert torch.equal(xr.grad, want_dx) and torch.equal(wr.grad, want_dw), route
    dx, dw = torch.ops.mcgmil.conv2d_f32x3_backward(x, w, dy, c.stride, c.pad, False, True)
    assert dx.numel() == 0 and torch.equal(dw, want_dw)
    dx, dw = torch.ops.mcgmil.conv2d_f32x3_backward(x, w, dy, c.stride, c.pad, True, False)
    assert dw.numel() == 0 and torch.equal(dx, want_dx)
    x16 = torch.zeros(1, 16, 4, 4, device=cuda).contiguous(memory_format=CL)
    with pytest.raises(ValueError, match="conv32x3_trainable"):
        torch.ops.mcgmil.conv2d_f32x3(x16, torch.zeros(64, 16, 3, 3, device=cuda), 1, 1)
    with pytest.raises(ValueError, match="conv32x3_trainable"):
        torch.ops.mcgmil.conv2d_f32x3_backward(x16, torch.zeros(64, 16, 3, 3, device=cuda),
                                               torch.zeros(1, 64, 4, 4, device=cuda), 1, 1, True, True)


def test_opcheck(cuda):
    c = ref.case("s2_3x3_odd")
    x, dy, _ = gpu(c, cuda)
    w = c.w.to(cuda)
    torch.library.opcheck(torch.ops.mcgmil.conv2d_f32x3.default,
                          (x.clone().requires_grad_(), w.clone().requires_grad_(), c.stride, c.pad))
    torch.library.opcheck(torch.ops.mcgmil.conv2d_f32x3_backward.default, (x, w, dy, c.stride, c.pad, True, True))


# ---------------------------------------------------------------- 6. the module
def _step(m, x, target, seed):
    m.zero_grad(set_to_none=True)
    Y, A, aux = m(x, target, seed=seed)
    (F.cross_entropy(Y, target) + aux).backward()
    torch.cuda.synchronize()
    return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}, Y.detach(), A.detach()


def _fresh(m0):
    """A copy of the module whose BatchNorms keep no running statistics (the reference's
    deactivate_batchnorm: the same batch-statistics arithmetic in train mode, and what lets
    norm=True and stem=True take them), so that every backbone layer of the step is one of the
    project's kernels and the step can repeat bitwise."""
    m = copy.deepcopy(m0)
    m.apply(deactivate_batchnorm)
    return m


def _fp32_opt_ins(m):
    return m.train().enable_head_training().enable_backbone_training(norm=True, stem=True, stem_conv=True)


def test_module_step(cuda, monkeypatch):
    """One r18 step of 3 instances of 64 x 64 against test_gpu_conv_grad.py's float64 CPU step."""
    monkeypatch.delenv("MCGMIL_CONV_GRAD", raising=False)
    m0, x, target, seed, g64, _ = base.module_case()
    m = _fp32_opt_ins(_fresh(m0))
    assert m.enable_bf16x3_backbone_training() is m
    routed, exact = [], []
    real, real32 = features.conv2d_f32x3_op, features.conv2d_f32_op
    monkeypatch.setattr(features, "conv2d_f32x3_op", lambda layer, t: routed.append(layer) or real(layer, t))
    monkeypatch.setattr(features, "conv2d_f32_op", lambda layer, t: exact.append(layer) or real32(layer, t))
    g1, Y1, A1 = _step(m, x, target, seed)
    stem = m.feature_extractor.conv1
    assert len(routed) == 19 and len({id(c) for c in routed}) == 19 and exact == []
    assert all(c is not stem for c in routed)                   # every block convolution, not the stem
    g2, Y2, A2 = _step(_fp32_opt_ins(_fresh(m0)).enable_bf16x3_backbone_training(), x, target, seed)   # identical state
    assert torch.equal(Y1, Y2) and torch.equal(A1, A2) and g1.keys() == g2.keys()
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    del routed[:]
    gb, _, _ = _step(_fresh(m0).train().enable_head_training().enable_bf16_backbone_training(), x, target, seed)
    ge, _, _ = _step(_fp32_opt_ins(_fresh(m0)), x, target, seed)
    assert routed == [] and len(exact) == 19
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "direct")            # ... and the same opt-in on the project's own backward
    gd, _, _ = _step(_fp32_opt_ins(_fresh(m0)), x, target, seed)
    rows = []
    for layer in base.LAYERS:
        n = f"feature_extractor.{layer}.weight"
        e3, eb, ee, ed = (golden_util.nrel(g[n].double().cpu().numpy(), g64[layer]) for g in (g1, gb, ge, gd))
        rows.append((layer, e3, eb, ee))
        print(f"{layer}: bf16x3 {e3:.2e} / {eb / 32:.2e} (bf16 step {eb:.2e}; exact fp32 opt-in {ee:.2e}, "
              f"on MCGMIL_CONV_GRAD=direct {ed:.2e})")
    for layer, e3, eb, _ in rows:
        assert e3 <= eb / 32, (layer, e3, eb)


# ---------------------------------------------------------------- 7. off means unchanged
def test_off_means_unchanged(cuda, monkeypatch):
    """Never called, switched off again, eval mode and no_grad: no convolution reaches the op and
    outputs and gradients are bitwise those of a model without the method. The training step is
    compared on MCGMIL_CONV_GRAD=direct, the route on which the fp32 opt-ins repeat bitwise."""
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "direct")
    monkeypatch.delenv("MCGMIL_CONV32_PRECISION", raising=False)
    m0, x, target, seed, _, _ = base.module_case()
    routed = []
    real = features.conv2d_f32x3_op
    monkeypatch.setattr(features, "conv2d_f32x3_op", lambda layer, t: routed.append(layer) or real(layer, t))
    never = _fp32_opt_ins(_fresh(m0))
    gn, Yn, An = _step(never, x, target, seed)
    off = _fp32_opt_ins(_fresh(m0)).enable_bf16x3_backbone_training()
    assert off.enable_bf16x3_backbone_training(False) is off
    go, Yo, Ao = _step(off, x, target, seed)
    assert routed == [] and torch.equal(Yo, Yn) and torch.equal(Ao, An) and go.keys() == gn.keys()
    for n in gn:
        assert torch.equal(go[n], gn[n]), n
    # on, but without enable_backbone_training: not in effect
    alone = _fresh(m0).train().enable_head_training().enable_bf16x3_backbone_training()
    _step(alone, x, target, seed)
    assert routed == []
    # feature_precision = "bf16x3" still routes no training op
    never.feature_precision = "bf16x3"
    packs = []
    realp = features.packed_conv_weight_f32x3
    monkeypatch.setattr(features, "packed_conv_weight_f32x3", lambda conv, t: packs.append(conv) or realp(conv, t))
    gp, Yp, _ = _step(never, x, target, seed)
    assert routed == [] and packs == [] and torch.equal(Yp, Yn)
    never.feature_precision = "fp32"
    # eval mode and no_grad: the inference path, bitwise
    flagged = _fp32_opt_ins(_fresh(m0)).enable_bf16x3_backbone_training()
    plain = _fresh(m0)
    Ye, Ae, _ = plain.eval()(x, target)
    Yf, Af, _ = flagged.eval()(x, target)
    assert routed == [] and torch.equal(Yf, Ye) and torch.equal(Af, Ae)
    with torch.no_grad():                                        # train mode, no graph: the inference path
        torch.manual_seed(5)                                     # the dropout masks' key is drawn from it
        Ym, Am, _ = plain.train()(x, target)
        torch.manual_seed(5)
        Yg, Ag, _ = flagged.train()(x, target)
    assert routed == [] and packs == [] and torch.equal(Yg, Ym) and torch.equal(Ag, Am)


# ---------------------------------------------------------------- 8. validation
def test_validation_leaves_dw_untouched(cuda):
    L = _lib.load()
    x = torch.ones(1, 64, 4, 4, device=cuda).contiguous(memory_format=CL)
    dy = torch.ones(1, 64, 4, 4, device=cuda).contiguous(memory_format=CL)
    dw = torch.full((64, 64, 3, 3), 7.0, device=cuda)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=cuda)
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4                # enum mcgmil_status (include/mcgmil.h)

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
        rc = L.mcgmil_conv2d_wgrad_f32x3(ctypes.byref(g), None)
        torch.cuda.synchronize()
        if rc:
            assert len(L.mcgmil_last_error()) > 0
        return rc
    for bad, code in ((dict(in_channels=48), UNSUPPORTED), (dict(in_channels=16), UNSUPPORTED),
                      (dict(out_channels=96), UNSUPPORTED), (dict(stride=3), UNSUPPORTED), (dict(pad=3), UNSUPPORTED),
                      (dict(pad=5), UNSUPPORTED), (dict(kernel_h=8), UNSUPPORTED),
                      (dict(in_ab=ctypes.c_void_p(x.data_ptr())), UNSUPPORTED), (dict(batch=0), INVALID)):
        assert rc_of(args(**bad)) == code, bad
    g = args()
    g.reserved = 1
    assert rc_of(g) == INVALID
    g = args()
    n = ctypes.c_size_t()
    assert L.mcgmil_conv_wgrad_workspace_size_f32x3(ctypes.byref(g), ctypes.byref(n)) == 0
    assert n.value == 2 * 64 * 64 * 9 * 4                       # one granule: the running sum + one partial
    g.workspace_bytes = n.value - 1
    assert rc_of(g) == WORKSPACE                                # a short workspace
    g.workspace, g.workspace_bytes = None, 0
    assert rc_of(g) == WORKSPACE
    assert bool((dw == 7.0).all())                              # every refusal left dw as it was
    assert rc_of(args()) == 0
    assert not bool((dw == 7.0).any())
