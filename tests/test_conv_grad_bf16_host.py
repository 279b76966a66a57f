"""Host-side checks of the bf16 convolution training route (no kernel launches): the predicate and
its reasons, the opt-in method, the context manager, the fake kernels and the bindings."""
import ctypes
import inspect

import pytest
import torch
import torch.nn as nn

from mcgmil import MultiHeadGatedAttentionMIL, _build, _lib, features, library  # noqa: F401

CL = torch.channels_last
BF = torch.bfloat16


def _conv(**kw):
    args = dict(in_channels=64, out_channels=128, kernel_size=3, stride=1, padding=1, bias=False)
    args.update(kw)
    return nn.Conv2d(**args)


def test_a_cpu_tensor_is_refused_with_a_reason():
    conv, x = _conv(), torch.zeros(2, 64, 8, 8, dtype=BF).contiguous(memory_format=CL)
    reason = features.conv_bf16_untrainable_reason(conv, x)
    assert isinstance(reason, str) and "CUDA" in reason
    assert features.conv_bf16_trainable(conv, x) is False
    with pytest.raises(ValueError, match="CUDA"):
        features.conv2d_bf16_wgrad(conv, x, torch.zeros(2, 128, 8, 8, dtype=BF))
    with pytest.raises(ValueError, match="CUDA"):
        features.conv2d_bf16(conv, x)
    with pytest.raises(ValueError, match="CUDA"):
        torch.ops.mcgmil.conv2d_bf16(x, conv.weight.detach(), 1, 1)


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is a CUDA one: the predicate's later clauses without a device."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    is_cuda = property(lambda self: True)


@pytest.mark.parametrize("make,x_shape,word", [
    (lambda: _conv(), (2, 64, 8, 8), None),
    (lambda: _conv().to(BF), (2, 64, 8, 8), None),                       # a bf16 weight as well as the fp32 master
    (lambda: _conv(stride=2), (2, 64, 9, 11), None),
    (lambda: _conv(in_channels=256, out_channels=64, kernel_size=1, padding=0), (1, 256, 7, 7), None),
    (lambda: _conv(kernel_size=(3, 7), padding=2), (2, 64, 8, 8), None),
    (lambda: _conv(in_channels=48), (2, 48, 8, 8), "in_channels"),
    (lambda: _conv(in_channels=16), (2, 16, 8, 8), "in_channels"),
    (lambda: _conv(out_channels=96), (2, 64, 8, 8), "out_channels"),
    (lambda: _conv(bias=True), (2, 64, 8, 8), "bias-free"),
    (lambda: _conv(groups=2), (2, 64, 8, 8), "groups"),
    (lambda: _conv(stride=3), (2, 64, 8, 8), "stride"),
    (lambda: _conv(dilation=2), (2, 64, 8, 8), "dilation"),
    (lambda: _conv(padding=3), (2, 64, 8, 8), "pad"),
    (lambda: _conv(kernel_size=9, padding=4), (2, 64, 16, 16), "kernel"),
    (lambda: _conv(padding=(1, 0)), (2, 64, 8, 8), "padding"),
    (lambda: _conv(padding="same"), (2, 64, 8, 8), "padding"),
    (lambda: _conv(), (2, 128, 8, 8), "channels"),
    (lambda: _conv().double(), (2, 64, 8, 8), "weight"),
    (lambda: nn.Linear(3, 3), (2, 64, 8, 8), "Conv2d"),
])
def test_each_clause(make, x_shape, word):
    conv = make()
    x = _OnGpu(torch.zeros(x_shape, dtype=BF).contiguous(memory_format=CL))
    reason = features.conv_bf16_untrainable_reason(conv, x)
    assert features.conv_bf16_trainable(conv, x) is (reason is None)
    if word is None:
        assert reason is None, reason
    else:
        assert reason is not None and word in reason, reason


def test_dtype_layout_and_switch_clauses(monkeypatch):
    conv = _conv()
    fp32 = _OnGpu(torch.zeros(2, 64, 8, 8).contiguous(memory_format=CL))
    assert "bf16" in features.conv_bf16_untrainable_reason(conv, fp32)           # an fp32 activation
    assert "channels-last" in features.conv_bf16_untrainable_reason(conv, _OnGpu(torch.zeros(2, 64, 8, 8, dtype=BF)))
    assert "4-d" in features.conv_bf16_untrainable_reason(conv, _OnGpu(torch.zeros(64, 8, 8, dtype=BF)))
    x = _OnGpu(torch.zeros(2, 64, 8, 8, dtype=BF).contiguous(memory_format=CL))
    assert features.conv_bf16_trainable(conv, x)
    x.requires_grad_()                                             # says nothing about autograd ...
    with torch.autocast("cpu", BF):                                # ... or autocast
        assert features.conv_bf16_trainable(conv, x)
    monkeypatch.setenv("MCGMIL_NATIVE_CONV32", "0")                # the fp32 switch does not concern it
    assert features.conv_bf16_trainable(conv, x)
    monkeypatch.setenv("MCGMIL_NATIVE_CONV", "0")
    assert "switched off" in features.conv_bf16_untrainable_reason(conv, x)


def test_context_restores_after_an_exception_and_leaves_the_other_opt_ins_alone():
    others = ("_native_training", "_native_norm_training", "_native_stem_training", "_native_stem_conv_training")
    assert features._native_bf16_training is False
    with pytest.raises(KeyError):
        with features.native_conv_bf16_training():
            assert features._native_bf16_training is True
            assert all(getattr(features, n) is False for n in others)
            with features.native_conv_bf16_training(False):
                assert features._native_bf16_training is False
            assert features._native_bf16_training is True
            raise KeyError("x")
    assert features._native_bf16_training is False
    with features.native_conv_bf16_training():
        pass
    assert features._native_bf16_training is False
    assert all(getattr(features, n) is False for n in others)
    with features.native_conv_training(), features.native_norm_training():
        with features.native_conv_bf16_training():
            assert features._native_training is True and features._native_norm_training is True
        assert features._native_training is True and features._native_bf16_training is False


def test_route_is_read_on_every_call(monkeypatch):
    monkeypatch.delenv("MCGMIL_CONV_GRAD", raising=False)
    assert features.conv_grad_route() == "aten" and not features.conv_grad_native()
    for value, native in (("native", True), ("direct", True), ("aten", False), ("bogus", False)):
        monkeypatch.setenv("MCGMIL_CONV_GRAD", value)
        assert features.conv_grad_native() is native
    conv = _conv(stride=2)
    dy = torch.zeros(1, 128, 4, 4, dtype=BF)
    assert not features.dgrad_bf16_native(conv, dy)                # stride 2: aten, dx only
    assert features.dgrad_bf16_native(_conv(), dy)
    assert not features.dgrad_bf16_native(_conv(kernel_size=(3, 5), padding=1), dy)


def test_enable_bf16_backbone_training():
    sig = inspect.signature(MultiHeadGatedAttentionMIL.enable_bf16_backbone_training)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("flag", True)]
    m = MultiHeadGatedAttentionMIL(pretrained=False)
    assert m._bf16_backbone_training is False                      # off by default
    assert m.enable_bf16_backbone_training() is m and m._bf16_backbone_training is True
    assert (m._head_training, m._backbone_training, m._norm_training, m._stem_training, m._stem_conv_training) == \
        (False,) * 5                                               # the other opt-ins are untouched
    m.enable_backbone_training(norm=True)
    assert m._bf16_backbone_training is True                       # ... and do not touch this one
    assert m.enable_bf16_backbone_training(False) is m and m._bf16_backbone_training is False
    m.enable_bf16_backbone_training()
    m.enable_backbone_training(False)
    m.train()
    with pytest.raises(NotImplementedError, match="enable_head_training"):       # alone it is not enough
        m(torch.zeros(1, 2, 3, 32, 32))


def test_enable_backbone_training_signature_is_unchanged():
    sig = inspect.signature(MultiHeadGatedAttentionMIL.enable_backbone_training)
    assert [(p.name, p.default, p.kind) for p in list(sig.parameters.values())[1:]] == [
        ("flag", True, inspect.Parameter.POSITIONAL_OR_KEYWORD), ("norm", False, inspect.Parameter.KEYWORD_ONLY),
        ("stem", False, inspect.Parameter.KEYWORD_ONLY), ("stem_conv", False, inspect.Parameter.KEYWORD_ONLY)]


@pytest.mark.parametrize("wdtype", [torch.float32, BF])
@pytest.mark.parametrize("stride,pad,k,cout", [(1, 1, 3, 64), (2, 1, 3, 128), (2, 0, 1, 128), (1, 2, 5, 64)])
def test_fake_kernels_shapes_dtypes_and_channels_last_strides(stride, pad, k, cout, wdtype):
    x = torch.empty(3, 64, 9, 11, device="meta", dtype=BF).contiguous(memory_format=CL)
    w = torch.empty(cout, 64, k, k, device="meta", dtype=wdtype)
    y = torch.ops.mcgmil.conv2d_bf16(x, w, stride, pad)
    oh, ow = (9 + 2 * pad - k) // stride + 1, (11 + 2 * pad - k) // stride + 1
    assert y.shape == (3, cout, oh, ow) and y.dtype == BF and y.device.type == "meta"
    assert y.is_contiguous(memory_format=CL) and y.stride(1) == 1
    dx, dw = torch.ops.mcgmil.conv2d_bf16_backward(x, w, y, stride, pad, True, True)
    assert dx.shape == x.shape and dx.dtype == BF and dx.is_contiguous(memory_format=CL) and dx.stride(1) == 1
    assert dw.shape == w.shape and dw.dtype == wdtype and dw.is_contiguous()     # the weight's dtype
    dx, dw = torch.ops.mcgmil.conv2d_bf16_backward(x, w, y, stride, pad, False, False)
    assert dx.numel() == 0 and dw.numel() == 0


def test_symbols_and_struct_are_bound():
    assert _lib.CONV_GRAD_BF16_EXPORTED == ("mcgmil_conv_grad_bf16_args_size",
                                            "mcgmil_conv_wgrad_workspace_size_bf16", "mcgmil_conv2d_wgrad_bf16")
    assert _lib.ABI_VERSION == 6                                   # entry points only: no ABI bump
    L = _lib.load()
    pcb = ctypes.POINTER(_lib.ConvGradBf16Args)
    assert L.mcgmil_abi_version() == 6
    assert L.mcgmil_conv_grad_bf16_args_size() == ctypes.sizeof(_lib.ConvGradBf16Args)
    assert ctypes.sizeof(_lib.ConvGradBf16Args) == ctypes.sizeof(_lib.ConvGradArgs)
    assert L.mcgmil_conv_wgrad_workspace_size_bf16.argtypes == [pcb, ctypes.POINTER(ctypes.c_size_t)]
    assert L.mcgmil_conv2d_wgrad_bf16.argtypes == [pcb, ctypes.c_void_p]
    assert "mcgmil_conv_grad_bf16.hip" in _build.SOURCES and "mcgmil_conv_grad_bf16.hip" in _build.DEPS


def test_validation_without_a_launch():
    """The entry points refuse what the header says they refuse before any launch."""
    L = _lib.load()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4                   # enum mcgmil_status (include/mcgmil.h)

    def args(**kw):
        g = _lib.ConvGradBf16Args()
        a = g.fwd
        a.batch, a.height, a.width, a.in_channels, a.out_channels = 1, 4, 4, 64, 64
        a.kernel_h = a.kernel_w = 3
        a.stride, a.pad = 1, 1
        a.x, g.dy, g.dw = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)
        for k, v in kw.items():
            setattr(g.fwd, k, v)
        return g
    n = ctypes.c_size_t()
    assert L.mcgmil_conv_wgrad_workspace_size_bf16(ctypes.byref(args()), ctypes.byref(n)) == 0
    assert n.value == 2 * 64 * 64 * 9 * 4                          # one granule: the running sum + one partial
    g = args(batch=5, height=64, width=64)                         # 20,480 pixels: 10 granules
    for chunk, granules in ((0, 10), (1, 1), (_lib.WGRAD_GRANULE_PIXELS, 1), (3 * _lib.WGRAD_GRANULE_PIXELS + 7, 3)):
        g.chunk_pixels = chunk
        assert L.mcgmil_conv_wgrad_workspace_size_bf16(ctypes.byref(g), ctypes.byref(n)) == 0
        assert n.value == (1 + granules) * 64 * 64 * 9 * 4, chunk
    for bad in (dict(in_channels=48), dict(in_channels=16), dict(out_channels=96), dict(stride=3), dict(pad=3),
                dict(kernel_h=8), dict(in_ab=ctypes.c_void_p(0x40000)), dict(batch=0)):
        rc = L.mcgmil_conv_wgrad_workspace_size_bf16(ctypes.byref(args(**bad)), ctypes.byref(n))
        assert rc in (INVALID, UNSUPPORTED) and len(L.mcgmil_last_error()) > 0, bad
    assert L.mcgmil_conv2d_wgrad_bf16(ctypes.byref(args()), None) == WORKSPACE   # no workspace: no launch
