"""Host-side checks of the stem convolution's training route (no kernel launches): the predicate
and its reasons, the opt-in keyword, the context manager, the fake kernels and the bindings."""
import ctypes
import inspect

import pytest
import torch
import torch.nn as nn

from mcgmil import MultiHeadGatedAttentionMIL, _build, _lib, features, library  # noqa: F401

CL = torch.channels_last


def _stem(**kw):
    args = dict(in_channels=3, out_channels=64, kernel_size=7, stride=2, padding=3, bias=False)
    args.update(kw)
    return nn.Conv2d(**args)


def test_a_cpu_tensor_is_refused_with_a_reason():
    conv, x = _stem(), torch.zeros(2, 3, 16, 16).contiguous(memory_format=CL)
    reason = features.stem_conv_untrainable_reason(conv, x)
    assert isinstance(reason, str) and "CUDA" in reason
    assert features.stem_conv_trainable(conv, x) is False
    with pytest.raises(ValueError):
        features.conv2d_f32_stem_wgrad(conv, x, torch.zeros(2, 64, 8, 8))


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is a CUDA one: the predicate's later clauses without a device."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    is_cuda = property(lambda self: True)


@pytest.mark.parametrize("make,x_shape,word", [
    (lambda: _stem(), (2, 3, 16, 16), None),
    (lambda: _stem(in_channels=1), (2, 1, 16, 16), None),
    (lambda: _stem(in_channels=4, kernel_size=(3, 7), padding=1), (2, 4, 16, 16), None),
    (lambda: _stem(in_channels=5), (2, 5, 16, 16), "in_channels"),
    (lambda: _stem(in_channels=16), (2, 16, 16, 16), "in_channels"),
    (lambda: _stem(out_channels=96), (2, 3, 16, 16), "out_channels"),
    (lambda: _stem(bias=True), (2, 3, 16, 16), "bias-free"),
    (lambda: _stem(in_channels=4, groups=2), (2, 4, 16, 16), "groups"),
    (lambda: _stem(stride=3), (2, 3, 16, 16), "stride"),
    (lambda: _stem(dilation=2), (2, 3, 16, 16), "dilation"),
    (lambda: _stem(kernel_size=3, padding=3), (2, 3, 16, 16), "pad"),
    (lambda: _stem(kernel_size=9, padding=4), (2, 3, 16, 16), "kernel"),
    (lambda: _stem(padding=(3, 2)), (2, 3, 16, 16), "padding"),
    (lambda: _stem(padding="same", stride=1), (2, 3, 16, 16), "padding"),
    (lambda: _stem(), (2, 4, 16, 16), "channels"),
    (lambda: _stem().double(), (2, 3, 16, 16), "fp32"),
    (lambda: nn.Linear(3, 3), (2, 3, 16, 16), "Conv2d"),
])
def test_each_clause(make, x_shape, word):
    conv = make()
    x = _OnGpu(torch.zeros(x_shape).contiguous(memory_format=CL))
    reason = features.stem_conv_untrainable_reason(conv, x)
    assert features.stem_conv_trainable(conv, x) is (reason is None)
    if word is None:
        assert reason is None
    else:
        assert reason is not None and word in reason, reason


def test_layout_dtype_and_switch_clauses(monkeypatch):
    conv = _stem()
    assert "channels-last" in features.stem_conv_untrainable_reason(conv, _OnGpu(torch.zeros(2, 3, 16, 16)))
    assert "fp32" in features.stem_conv_untrainable_reason(
        conv, _OnGpu(torch.zeros(2, 3, 16, 16, dtype=torch.float64).contiguous(memory_format=CL)))
    assert "4-d" in features.stem_conv_untrainable_reason(conv, _OnGpu(torch.zeros(3, 16, 16)))
    x = _OnGpu(torch.zeros(2, 3, 16, 16).contiguous(memory_format=CL))
    assert features.stem_conv_trainable(conv, x)
    monkeypatch.setenv("MCGMIL_NATIVE_CONV32", "0")
    assert "switched off" in features.stem_conv_untrainable_reason(conv, x)


def test_context_restores_after_an_exception():
    assert features._native_stem_conv_training is False
    with pytest.raises(KeyError):
        with features.native_stem_conv_training():
            assert features._native_stem_conv_training is True
            with features.native_stem_conv_training(False):
                assert features._native_stem_conv_training is False
            assert features._native_stem_conv_training is True
            raise KeyError("x")
    assert features._native_stem_conv_training is False
    assert features._native_training is False                     # the other opt-ins are untouched


def test_enable_backbone_training_keyword():
    sig = inspect.signature(MultiHeadGatedAttentionMIL.enable_backbone_training)
    assert [(p.name, p.default, p.kind) for p in list(sig.parameters.values())[1:]] == [
        ("flag", True, inspect.Parameter.POSITIONAL_OR_KEYWORD), ("norm", False, inspect.Parameter.KEYWORD_ONLY),
        ("stem", False, inspect.Parameter.KEYWORD_ONLY), ("stem_conv", False, inspect.Parameter.KEYWORD_ONLY)]
    m = MultiHeadGatedAttentionMIL(pretrained=False)
    assert m._stem_conv_training is False
    assert m.enable_backbone_training() is m
    assert (m._backbone_training, m._norm_training, m._stem_training, m._stem_conv_training) == \
        (True, False, False, False)
    assert m.enable_backbone_training(stem_conv=True) is m
    assert (m._backbone_training, m._norm_training, m._stem_training, m._stem_conv_training) == \
        (True, False, False, True)
    assert m.enable_backbone_training(False, stem_conv=True) is m             # cleared by flag=False
    assert (m._backbone_training, m._stem_conv_training) == (False, False)
    m.enable_backbone_training(norm=True, stem=True, stem_conv=True)
    assert (m._norm_training, m._stem_training, m._stem_conv_training) == (True, True, True)
    m.enable_backbone_training()                                                # and by its default
    assert m._stem_conv_training is False


@pytest.mark.parametrize("stride,pad,k", [(2, 3, 7), (1, 1, 3)])
def test_fake_kernels_shapes_and_channels_last_strides(stride, pad, k):
    x = torch.empty(3, 3, 9, 11, device="meta").contiguous(memory_format=CL)
    w = torch.empty(64, 3, k, k, device="meta")
    y = torch.ops.mcgmil.stem_conv_f32(x, w, stride, pad)
    oh, ow = (9 + 2 * pad - k) // stride + 1, (11 + 2 * pad - k) // stride + 1
    assert y.shape == (3, 64, oh, ow) and y.dtype == torch.float32 and y.device.type == "meta"
    assert y.is_contiguous(memory_format=CL) and y.stride(1) == 1
    dx, dw = torch.ops.mcgmil.stem_conv_f32_backward(x, w, y, stride, pad, True, True)
    assert dx.shape == x.shape and dw.shape == w.shape and dw.is_contiguous()
    dx, dw = torch.ops.mcgmil.stem_conv_f32_backward(x, w, y, stride, pad, False, False)
    assert dx.numel() == 0 and dw.numel() == 0


def test_symbols_are_bound_with_the_existing_struct():
    assert _lib.STEM_GRAD_EXPORTED == ("mcgmil_stem_wgrad_workspace_size_f32", "mcgmil_stem_wgrad_f32")
    L = _lib.load()
    pcg = ctypes.POINTER(_lib.ConvGradArgs)
    assert L.mcgmil_stem_wgrad_workspace_size_f32.argtypes == [pcg, ctypes.POINTER(ctypes.c_size_t)]
    assert L.mcgmil_stem_wgrad_f32.argtypes == [pcg, ctypes.c_void_p]
    assert L.mcgmil_stem_wgrad_f32.restype is ctypes.c_int
    assert L.mcgmil_conv_grad_args_size() == ctypes.sizeof(_lib.ConvGradArgs)
    # the geometry checks run on the host: no device is needed to be refused
    g = _lib.ConvGradArgs()
    a = g.fwd
    a.batch, a.height, a.width, a.in_channels, a.out_channels = 1, 8, 8, 3, 64
    a.kernel_h = a.kernel_w = 7
    a.stride, a.pad = 2, 3
    n = ctypes.c_size_t()
    assert L.mcgmil_stem_wgrad_workspace_size_f32(ctypes.byref(g), ctypes.byref(n)) == 0
    assert n.value == 2 * 64 * 147 * 4
    a.in_channels = 16
    assert L.mcgmil_stem_wgrad_workspace_size_f32(ctypes.byref(g), ctypes.byref(n)) == -2
    assert b"in_channels" in L.mcgmil_last_error()
    a.in_channels, a.batch, a.height, a.width = 3, 1507, 224, 224
    assert L.mcgmil_stem_wgrad_workspace_size_f32(ctypes.byref(g), ctypes.byref(n)) == 0
    E4 = 64 * 147 * 4
    assert n.value == (1 + (128 << 20) // E4) * E4              # the default cap on the partials
