"""Host-side checks of fp32 training on split-bf16 MFMA (include/mcgmil_conv_grad_x3.h,
features.conv2d_f32x3_*, torch.ops.mcgmil.conv2d_f32x3,
MultiHeadGatedAttentionMIL.enable_bf16x3_backbone_training), no kernel launches: the numerics
contract on tests/conv_grad_x3_ref.py's emulation (so the GPU tests' reference and bounds stand
without a GPU), the predicate's verdicts and reasons, where run_conv sends a layer, the opt-in
method, the fake kernels and the bindings."""
import ctypes
import inspect

import pytest
import torch
import torch.nn as nn

import conv_grad_x3_ref as ref
from mcgmil import MultiHeadGatedAttentionMIL, _build, _lib, features, library

CL = torch.channels_last


# ---------------------------------------------------------------------------------- numerics
def test_table_matches_the_library_granule():
    assert ref.G == _lib.WGRAD_GRANULE_PIXELS
    N, _, _, k, s, p, H, W = ref.CASES["granules"]
    assert N * ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1) == 2 * ref.G + ref.G // 2 + 5


@pytest.mark.parametrize("name", ref.NAMES)
def test_emulation_within_the_derived_bound(name):
    c = ref.case(name)
    assert not torch.equal(c.x, c.x.bfloat16().float()) and not torch.equal(c.dy, c.dy.bfloat16().float())
    err = (c.dw_emu - c.dw64).abs()
    worst = float((err / c.dw_mag.clamp_min(1e-300)).max())
    n3, n1 = ref.nrel(c.dw_emu, c.dw64), ref.nrel(c.dw_hi, c.dw64)
    print(f"{name} dw: max err / wgrad(|dy|,|x|) {worst:.2e} / {ref.SPLIT_BOUND:.2e}; "
          f"max|d|/max|ref| bf16x3 {n3:.2e}, hi*hi only {n1:.2e}, ratio {n1 / n3:.0f}")
    assert bool((err <= ref.SPLIT_BOUND * c.dw_mag).all())
    assert n3 <= ref.HI_ONLY_RATIO * n1
    if c.stride == 1:                                  # the same construction for dX
        dx64, emu, mag = c.dx
        err = (emu - dx64).abs()
        print(f"{name} dx: max err / dgrad(|dy|,|w|) {float((err / mag.clamp_min(1e-300)).max()):.2e}")
        assert bool((err <= ref.SPLIT_BOUND * mag).all())


# ---------------------------------------------------------------------------------- predicate
def _conv(cin=64, cout=64, k=3, stride=1, pad=1, **kw):
    return nn.Conv2d(cin, cout, k, stride, pad, **dict(dict(bias=False), **kw))


def _x(c=64, dtype=torch.float32):
    return torch.zeros(2, c, 6, 6, dtype=dtype).contiguous(memory_format=CL)


class _Cuda(torch.Tensor):
    """A CPU tensor that reports is_cuda: the clauses are walked, no GPU is touched."""
    is_cuda = True


def _gx(c=64, dtype=torch.float32):
    return _x(c, dtype).as_subclass(_Cuda)


def test_verdicts_and_reasons(monkeypatch):
    monkeypatch.delenv("MCGMIL_NATIVE_CONV32", raising=False)
    monkeypatch.delenv("MCGMIL_NATIVE_CONV", raising=False)
    why, ok = features.conv32x3_untrainable_reason, features.conv32x3_trainable
    assert why(_conv(), _gx()) is None and ok(_conv(), _gx())
    assert ok(_conv(32), _gx(32)) and ok(_conv(stride=2), _gx()) and ok(_conv(256, 64, 1, 1, 0), _gx(256))
    assert ok(_conv(), _gx().requires_grad_())                                        # says nothing about autograd
    for cin in (16, 48):     # the exact kernels' domain, not this one's
        assert features.conv32_trainable(_conv(cin), _gx(cin)) and not ok(_conv(cin), _gx(cin))
        assert "multiple of 32" in why(_conv(cin), _gx(cin))
    stem = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    assert "multiple of 32" in why(stem, _gx(3)) and not ok(stem, _gx(3))             # the stem
    with monkeypatch.context() as mp:                  # autocast on the GPU, without one
        mp.setattr(torch, "is_autocast_enabled", lambda device="cuda": device == "cuda")
        assert why(_conv(), _gx()) == "autocast is enabled"
        assert not features.conv32_trainable(_conv(), _gx())                          # as conv32_trainable
    assert "must be fp32" in why(_conv().half(), _gx())                               # fp16 weights
    assert "must be fp32" in why(_conv(), _gx(dtype=torch.bfloat16))
    assert "stride" in why(_conv(stride=3), _gx())
    assert "pad" in why(_conv(pad=3), _gx())
    assert "multiple of 64" in why(_conv(cout=96), _gx())
    assert "bias-free" in why(_conv(bias=True), _gx())
    assert "channels-last" in why(_conv(), torch.zeros(2, 64, 6, 6).as_subclass(_Cuda))
    assert "CUDA" in why(_conv(), _x()) and not ok(_conv(), _x())
    assert why(nn.Identity(), _gx()) == "not an nn.Conv2d"
    monkeypatch.setenv("MCGMIL_NATIVE_CONV32", "0")
    assert "switched off" in why(_conv(), _gx())


def test_a_cpu_tensor_is_refused_with_a_reason():
    conv, x, dy = _conv(), _x(), torch.zeros(2, 64, 6, 6)
    with pytest.raises(ValueError, match="CUDA"):
        features.conv2d_f32x3_wgrad(conv, x, dy)
    with pytest.raises(ValueError, match="CUDA"):
        features.conv2d_f32x3_backward(conv, x, dy)
    with pytest.raises(ValueError, match="conv32x3_trainable"):
        torch.ops.mcgmil.conv2d_f32x3(x, conv.weight.detach(), 1, 1)
    with pytest.raises(ValueError, match="conv32x3_trainable"):
        torch.ops.mcgmil.conv2d_f32x3_backward(x, conv.weight.detach(), dy, 1, 1, True, True)


# ---------------------------------------------------------------------------------- routing
def test_run_conv_sends_a_trainable_layer_to_the_op_inside_both_contexts_only(monkeypatch):
    sent = []
    for name in ("conv2d_f32x3_op", "conv2d_f32_op", "conv2d_bf16_op", "stem_conv_f32_op", "torch_conv", "conv2d_f32"):
        monkeypatch.setattr(features, name, lambda layer, t, name=name: sent.append(name) or t)
    conv, conv16, x = _conv(), _conv(16), _gx()

    def route(layer=conv, t=x):
        del sent[:]
        features.run_conv(layer, t)
        return sent

    assert route() == ["torch_conv"]
    with features.native_conv_x3_training():                        # alone: not in effect
        assert route() == ["torch_conv"]
    with features.native_conv_training():
        assert route() == ["conv2d_f32_op"]
        with features.native_conv_x3_training():
            assert route() == ["conv2d_f32x3_op"]
            assert route(conv16, _gx(16)) == ["conv2d_f32_op"]      # outside the x3 domain: the exact op
            with features.native_conv_x3_training(False):
                assert route() == ["conv2d_f32_op"]
            with monkeypatch.context() as mp:                       # the predicate refuses under autocast
                mp.setattr(torch, "is_autocast_enabled", lambda device="cuda": device == "cuda")
                assert route() == ["torch_conv"]
            with torch.no_grad():
                frozen = _conv().requires_grad_(False)
                assert route(frozen) == ["conv2d_f32"]              # nothing to train: the inference kernel
        assert route() == ["conv2d_f32_op"]
    assert route() == ["torch_conv"]
    assert features._native_x3_training is False and features._native_training is False


def test_context_restores_after_an_exception():
    with pytest.raises(KeyError):
        with features.native_conv_x3_training():
            assert features._native_x3_training is True and features._native_training is False
            raise KeyError("x")
    assert features._native_x3_training is False


def test_backward_does_not_read_the_route(monkeypatch):
    """conv2d_f32x3_backward takes both gradients from the x3 functions on every MCGMIL_CONV_GRAD."""
    conv, x, dy = _conv(), _gx(), _gx()
    calls = []
    monkeypatch.setattr(features, "conv2d_f32x3_wgrad", lambda c, a, d: calls.append("w") or "dw")
    monkeypatch.setattr(features, "conv2d_f32x3_dgrad", lambda c, d, s: calls.append("x") or "dx")
    monkeypatch.setattr(features, "_aten_conv_backward", lambda *a: pytest.fail("aten"))
    for value in (None, "aten", "native", "direct"):
        if value is None:
            monkeypatch.delenv("MCGMIL_CONV_GRAD", raising=False)
        else:
            monkeypatch.setenv("MCGMIL_CONV_GRAD", value)
        del calls[:]
        assert features.conv2d_f32x3_backward(conv, x, dy) == ("dx", "dw") and calls == ["w", "x"]
    assert features.conv2d_f32x3_backward(conv, x, dy, need_dx=False) == (None, "dw")
    assert features.conv2d_f32x3_backward(conv, x, dy, need_dw=False) == ("dx", None)


def test_dgrad_takes_the_forward_kernel_for_stride_1_and_the_direct_one_otherwise(monkeypatch):
    seen = []
    monkeypatch.setattr(features, "conv2d_f32", lambda conv, t, **k: seen.append((conv, k)) or
                        torch.zeros(t.shape[0], conv.out_channels, 6, 6).contiguous(memory_format=CL))
    monkeypatch.setattr(features, "conv2d_f32_dgrad_direct", lambda conv, d, s: seen.append("direct") or "dx")
    dy = _gx()
    dx = features.conv2d_f32x3_dgrad(_conv(32, 64), dy, (2, 32, 6, 6))
    (shim, kw), = seen
    assert kw == {"precision": "bf16x3"} and tuple(shim.weight.shape) == (64, 64, 3, 3)   # 32 -> 64 zero filters
    assert shim.padding == (1, 1) and shim.stride == (1, 1) and not bool(shim.weight[32:].any())
    assert tuple(dx.shape) == (2, 32, 6, 6) and dx.is_contiguous(memory_format=CL)
    del seen[:]
    assert features.conv2d_f32x3_dgrad(_conv(stride=2), dy, (2, 64, 11, 11)) == "dx" and seen == ["direct"]
    del seen[:]
    assert features.conv2d_f32x3_dgrad(_conv(k=(1, 3), pad=0), dy, (2, 64, 6, 8)) == "dx" and seen == ["direct"]


# ---------------------------------------------------------------------------------- the model
def test_enable_bf16x3_backbone_training(monkeypatch):
    sig = inspect.signature(MultiHeadGatedAttentionMIL.enable_bf16x3_backbone_training)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("flag", True)]
    m = MultiHeadGatedAttentionMIL(pretrained=False)
    assert m._bf16x3_backbone_training is False                     # off by default
    assert m.enable_bf16x3_backbone_training() is m and m._bf16x3_backbone_training is True
    others = ("_head_training", "_backbone_training", "_norm_training", "_stem_training", "_stem_conv_training",
              "_bf16_backbone_training", "_bf16_norm_training", "_bf16_stem_training", "_bf16_stem_conv_training")
    assert all(getattr(m, n) is False for n in others)              # the other opt-ins are untouched
    assert m.feature_precision == "fp32"                            # ... and so is the inference precision
    m.enable_backbone_training(norm=True, stem=True, stem_conv=True)
    assert m._bf16x3_backbone_training is True
    assert m.enable_bf16x3_backbone_training(False) is m and m._bf16x3_backbone_training is False
    m.enable_bf16x3_backbone_training().enable_backbone_training(False)
    m.train()
    with pytest.raises(NotImplementedError, match="enable_head_training"):       # alone it is not enough
        m(torch.zeros(1, 2, 3, 32, 32))
    # in effect only while head and backbone training are on: what forward() hands the context manager
    seen = []

    class Probe(nn.Module):
        def forward(self, t):
            seen.append((features._native_training, features._native_x3_training))
            raise KeyError("stop")

    m.feature_extractor = Probe()
    m.enable_head_training()
    for backbone, x3, want in ((False, True, (False, False)), (True, False, (True, False)), (True, True, (True, True))):
        m.enable_backbone_training(backbone).enable_bf16x3_backbone_training(x3)
        with pytest.raises(KeyError):
            m(torch.zeros(1, 2, 3, 32, 32))
        assert seen.pop() == want
    assert features._native_x3_training is False


def test_existing_signatures_are_unchanged():
    sig = inspect.signature(MultiHeadGatedAttentionMIL.enable_backbone_training)
    assert [(p.name, p.default, p.kind) for p in list(sig.parameters.values())[1:]] == [
        ("flag", True, inspect.Parameter.POSITIONAL_OR_KEYWORD), ("norm", False, inspect.Parameter.KEYWORD_ONLY),
        ("stem", False, inspect.Parameter.KEYWORD_ONLY), ("stem_conv", False, inspect.Parameter.KEYWORD_ONLY)]


# ---------------------------------------------------------------------------------- the library module
def test_ops_are_registered_outside_all():
    assert library.CONV_X3_OPS == ("conv2d_f32x3", "conv2d_f32x3_backward")
    assert library.__all__ == [
        "mcdo_forward", "mcdo_forward_stats", "mcdo_backward", "conv2d_f32", "conv2d_f32_backward",
        "bn_act_f32", "bn_act_f32_backward", "bn_pool_f32", "bn_pool_f32_backward",
        "stem_conv_f32", "stem_conv_f32_backward", "conv2d_bf16", "conv2d_bf16_backward",
        "bn_act_bf16", "bn_act_bf16_backward", "bn_pool_bf16", "bn_pool_bf16_backward"]
    for name in library.CONV_X3_OPS:
        assert name not in library.__all__ and hasattr(torch.ops.mcgmil, name) and hasattr(library, name)
    fwd, bwd = (str(getattr(torch.ops.mcgmil, n).default._schema) for n in library.CONV_X3_OPS)
    assert fwd == str(torch.ops.mcgmil.conv2d_f32.default._schema).replace("conv2d_f32", "conv2d_f32x3")
    assert bwd == str(torch.ops.mcgmil.conv2d_f32_backward.default._schema).replace("conv2d_f32", "conv2d_f32x3")


@pytest.mark.parametrize("stride,pad,k,cout", [(1, 1, 3, 64), (2, 1, 3, 128), (2, 0, 1, 128), (1, 2, 5, 64)])
def test_fake_kernels_shapes_dtypes_and_channels_last_strides(stride, pad, k, cout):
    x = torch.empty(3, 32, 9, 11, device="meta").contiguous(memory_format=CL)
    w = torch.empty(cout, 32, k, k, device="meta")
    y = torch.ops.mcgmil.conv2d_f32x3(x, w, stride, pad)
    oh, ow = (9 + 2 * pad - k) // stride + 1, (11 + 2 * pad - k) // stride + 1
    assert y.shape == (3, cout, oh, ow) and y.dtype == torch.float32 and y.is_contiguous(memory_format=CL)
    dx, dw = torch.ops.mcgmil.conv2d_f32x3_backward(x, w, y, stride, pad, True, True)
    assert dx.shape == x.shape and dx.dtype == torch.float32 and dx.is_contiguous(memory_format=CL)
    assert dw.shape == w.shape and dw.dtype == torch.float32 and dw.is_contiguous()
    dx, dw = torch.ops.mcgmil.conv2d_f32x3_backward(x, w, y, stride, pad, False, False)
    assert dx.numel() == 0 and dw.numel() == 0


# ---------------------------------------------------------------------------------- the bindings
def test_symbols_are_bound_on_the_fp32_struct():
    assert _lib.CONV_GRAD_X3_EXPORTED == ("mcgmil_conv_wgrad_workspace_size_f32x3", "mcgmil_conv2d_wgrad_f32x3")
    assert _lib.ABI_VERSION == 6                                    # entry points only: no ABI bump
    L = _lib.load()
    pcg = ctypes.POINTER(_lib.ConvGradArgs)
    assert L.mcgmil_abi_version() == 6
    assert L.mcgmil_conv_wgrad_workspace_size_f32x3.argtypes == [pcg, ctypes.POINTER(ctypes.c_size_t)]
    assert L.mcgmil_conv2d_wgrad_f32x3.argtypes == [pcg, ctypes.c_void_p]
    assert "mcgmil_conv_grad_x3.hip" in _build.SOURCES and "mcgmil_conv_grad_x3.hip" in _build.DEPS


def test_wgrad_goes_through_the_shared_helper(monkeypatch):
    seen = []
    monkeypatch.setattr(features, "_wgrad", lambda *a: seen.append(a) or "dw")
    conv, x, dy = _conv(), _gx(), _gx()
    assert features.conv2d_f32x3_wgrad(conv, x, dy, chunk_pixels=4096) == "dw"
    assert seen == [(_lib.ConvGradArgs, torch.float32, "mcgmil_conv_wgrad_workspace_size_f32x3",
                     "mcgmil_conv2d_wgrad_f32x3", conv, x, dy, 4096)]


def test_validation_without_a_launch():
    """The entry points refuse what the header says they refuse before any launch."""
    L = _lib.load()
    INVALID, UNSUPPORTED, ALIGN, WORKSPACE = -1, -2, -3, -4         # enum mcgmil_status (include/mcgmil.h)

    def args(**kw):
        g = _lib.ConvGradArgs()
        a = g.fwd
        a.batch, a.height, a.width, a.in_channels, a.out_channels = 1, 4, 4, 64, 64
        a.kernel_h = a.kernel_w = 3
        a.stride, a.pad = 1, 1
        a.x, g.dy, g.dw = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)
        for k, v in kw.items():
            setattr(g.fwd, k, v)
        return g
    n = ctypes.c_size_t()
    size = L.mcgmil_conv_wgrad_workspace_size_f32x3
    assert size(ctypes.byref(args()), ctypes.byref(n)) == 0
    assert n.value == 2 * 64 * 64 * 9 * 4                           # one granule: the running sum + one partial
    assert size(ctypes.byref(args(in_channels=32)), ctypes.byref(n)) == 0 and n.value == 2 * 64 * 32 * 9 * 4
    g = args(batch=5, height=64, width=64)                          # 20,480 pixels: 10 granules
    for chunk, granules in ((0, 10), (1, 1), (_lib.WGRAD_GRANULE_PIXELS, 1), (3 * _lib.WGRAD_GRANULE_PIXELS + 7, 3)):
        g.chunk_pixels = chunk
        assert size(ctypes.byref(g), ctypes.byref(n)) == 0
        assert n.value == (1 + granules) * 64 * 64 * 9 * 4, chunk
    for bad, code in ((dict(in_channels=48), UNSUPPORTED), (dict(in_channels=16), UNSUPPORTED),
                      (dict(in_channels=3), UNSUPPORTED), (dict(out_channels=96), UNSUPPORTED),
                      (dict(stride=3), UNSUPPORTED), (dict(pad=3), UNSUPPORTED), (dict(kernel_h=8), UNSUPPORTED),
                      (dict(in_ab=ctypes.c_void_p(0x40000)), UNSUPPORTED), (dict(batch=0), INVALID),
                      (dict(pad=-1), INVALID)):
        assert size(ctypes.byref(args(**bad)), ctypes.byref(n)) == code and len(L.mcgmil_last_error()) > 0, bad
    assert b"multiple of 32" in (size(ctypes.byref(args(in_channels=16)), ctypes.byref(n)) and L.mcgmil_last_error())
    g = args()
    g.reserved = 1
    assert L.mcgmil_conv2d_wgrad_f32x3(ctypes.byref(g), None) == INVALID
    g = args()
    g.dw = ctypes.c_void_p(0x30004)
    assert L.mcgmil_conv2d_wgrad_f32x3(ctypes.byref(g), None) == ALIGN
    assert L.mcgmil_conv2d_wgrad_f32x3(ctypes.byref(args()), None) == WORKSPACE   # no workspace: no launch
    assert L.mcgmil_conv2d_wgrad_f32x3(None, None) == INVALID
