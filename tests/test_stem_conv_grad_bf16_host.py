"""Host-side checks of the bf16 stem convolution's training route (no kernel launches): the
predicate and its reasons, the opt-in method, the context manager, the fake kernels, the schemas,
the bindings, and every validation path and the workspace arithmetic of the three C entry points."""
import ctypes
import inspect
import json
import os

import pytest
import torch
import torch.nn as nn

from conftest import REPO
from mcgmil import MultiHeadGatedAttentionMIL, _build, _lib, features, library  # noqa: F401

CL = torch.channels_last
BF = torch.bfloat16
G = _lib.WGRAD_GRANULE_PIXELS
INVALID, UNSUPPORTED, ALIGN, WORKSPACE = -1, -2, -3, -4       # enum mcgmil_status (include/mcgmil.h)


def _stem(**kw):
    args = dict(in_channels=3, out_channels=64, kernel_size=7, stride=2, padding=3, bias=False)
    args.update(kw)
    return nn.Conv2d(**args)


def test_a_cpu_tensor_is_refused_with_a_reason():
    conv, x = _stem(), torch.zeros(2, 3, 16, 16)
    reason = features.stem_conv_bf16_untrainable_reason(conv, x)
    assert isinstance(reason, str) and "CUDA" in reason
    assert features.stem_conv_bf16_trainable(conv, x) is False
    for call in (lambda: features.stem_conv_bf16(conv, x),
                 lambda: features.stem_conv_bf16_wgrad(conv, x, torch.zeros(2, 64, 8, 8, dtype=BF)),
                 lambda: torch.ops.mcgmil.stem_conv_bf16(x, conv.weight, 2, 3)):
        with pytest.raises(ValueError, match="CUDA"):
            call()


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is a CUDA one: the predicate's later clauses without a device."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    is_cuda = property(lambda self: True)


@pytest.mark.parametrize("make,x_shape,word", [
    (lambda: _stem(), (2, 3, 16, 16), None),
    (lambda: _stem(in_channels=1, kernel_size=5, padding=2), (2, 1, 17, 34), None),
    (lambda: _stem(in_channels=4, kernel_size=8, padding=2), (1, 4, 16, 16), None),
    (lambda: _stem(in_channels=2, kernel_size=6, padding=2).to(BF), (5, 2, 64, 96), None),     # a bf16 weight
    (lambda: _stem(), (1, 3, 224, 250), None),                                                  # OW = 125
    (lambda: _stem(in_channels=5), (2, 5, 16, 16), "in_channels"),
    (lambda: _stem(out_channels=128), (2, 3, 16, 16), "out_channels"),
    (lambda: _stem(bias=True), (2, 3, 16, 16), "bias-free"),
    (lambda: _stem(in_channels=4, groups=2), (2, 4, 16, 16), "groups"),
    (lambda: _stem(padding_mode="reflect"), (2, 3, 16, 16), "zero-padded"),
    (lambda: _stem(stride=1), (2, 3, 16, 16), "stride 2"),
    (lambda: _stem(stride=(2, 1)), (2, 3, 16, 16), "stride 2"),
    (lambda: _stem(dilation=2), (2, 3, 16, 16), "dilation"),
    (lambda: _stem(kernel_size=(7, 5)), (2, 3, 16, 16), "square kernel"),
    (lambda: _stem(padding=(3, 2)), (2, 3, 16, 16), "padding"),
    (lambda: _stem(padding="valid"), (2, 3, 16, 16), "padding"),
    (lambda: _stem(kernel_size=8, padding=3), (2, 3, 16, 16), "at most 8"),
    (lambda: _stem(kernel_size=9, padding=4), (2, 3, 16, 16), "at most 8"),
    (lambda: _stem(), (2, 4, 16, 16), "channels"),
    (lambda: _stem(), (2, 3, 16, 15), "even"),
    (lambda: _stem(padding=0), (2, 3, 4, 16), "fit"),
    (lambda: _stem(), (1, 3, 8, 252), "125"),
    (lambda: _stem(), (0, 3, 16, 16), "non-empty"),
    (lambda: _stem().double(), (2, 3, 16, 16), "weight"),
    (lambda: nn.Linear(3, 3), (2, 3, 16, 16), "Conv2d"),
])
def test_each_clause(make, x_shape, word):
    conv = make()
    x = _OnGpu(torch.zeros(x_shape))
    reason = features.stem_conv_bf16_untrainable_reason(conv, x)
    assert features.stem_conv_bf16_trainable(conv, x) is (reason is None)
    if word is None:
        assert reason is None, reason
    else:
        assert reason is not None and word in reason, reason


def test_dtype_layout_and_size_clauses():
    conv = _stem()
    assert features.stem_conv_bf16_trainable(conv, _OnGpu(torch.zeros(2, 3, 16, 16, dtype=BF)))
    assert features.stem_conv_bf16_trainable(conv, _OnGpu(torch.zeros(2, 3, 16, 16).contiguous(memory_format=CL)))
    assert "fp32 or bf16" in features.stem_conv_bf16_untrainable_reason(
        conv, _OnGpu(torch.zeros(2, 3, 16, 16, dtype=torch.float16)))
    assert "4-d" in features.stem_conv_bf16_untrainable_reason(conv, _OnGpu(torch.zeros(3, 16, 16)))
    # the size clauses, on tensors that own no memory
    big = _OnGpu(torch.empty(1).expand(7134, 3, 224, 224))         # bf16 copy: 2^31 + 249,856 bytes
    assert big.numel() * 2 >= 2 ** 31 and "2 GiB" in features.stem_conv_bf16_untrainable_reason(conv, big)
    below = _OnGpu(torch.empty(1).expand(7133, 3, 224, 224))
    assert features.stem_conv_bf16_trainable(conv, below)
    # says nothing about autograd or autocast
    x = _OnGpu(torch.zeros(2, 3, 16, 16).requires_grad_())
    assert conv.weight.requires_grad and features.stem_conv_bf16_trainable(conv, x)


def test_context_restores_after_an_exception():
    assert features._native_stem_conv_bf16_training is False
    with pytest.raises(KeyError):
        with features.native_stem_conv_bf16_training():
            assert features._native_stem_conv_bf16_training is True
            with features.native_stem_conv_bf16_training(False):
                assert features._native_stem_conv_bf16_training is False
            assert features._native_stem_conv_bf16_training is True
            raise KeyError("x")
    assert features._native_stem_conv_bf16_training is False
    assert features._native_stem_conv_training is False and features._native_bf16_training is False   # untouched


def test_opt_in_method():
    sig = inspect.signature(MultiHeadGatedAttentionMIL.enable_bf16_stem_conv_training)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("flag", True)]
    for name in ("enable_bf16_backbone_training", "enable_bf16_norm_training", "enable_bf16_stem_training"):
        s = inspect.signature(getattr(MultiHeadGatedAttentionMIL, name))         # the existing signatures stay
        assert [(p.name, p.default) for p in list(s.parameters.values())[1:]] == [("flag", True)], name
    m = MultiHeadGatedAttentionMIL(pretrained=False)
    assert m._bf16_stem_conv_training is False
    assert m.enable_bf16_stem_conv_training() is m and m._bf16_stem_conv_training is True
    # a flag of its own: nothing else moves, and without the backbone opt-in it has no effect
    assert (m._bf16_backbone_training, m._bf16_norm_training, m._bf16_stem_training, m._stem_conv_training) == \
        (False, False, False, False)
    assert "_bf16_stem_conv_training" in inspect.getsource(MultiHeadGatedAttentionMIL.forward).split(
        "if self._bf16_backbone_training:")[1].split("else:")[0]
    assert m.enable_bf16_stem_conv_training(False) is m and m._bf16_stem_conv_training is False
    m.enable_bf16_backbone_training().enable_bf16_stem_conv_training()
    assert (m._bf16_backbone_training, m._bf16_stem_conv_training) == (True, True)
    m.enable_bf16_norm_training().enable_bf16_stem_training(False)               # independent of the other opt-ins
    assert m._bf16_stem_conv_training is True
    assert m.enable_bf16_backbone_training(False) is m                           # switched off with the backbone opt-in
    assert (m._bf16_backbone_training, m._bf16_norm_training, m._bf16_stem_training, m._bf16_stem_conv_training) == \
        (False, False, False, False)
    m.enable_bf16_backbone_training()
    assert m._bf16_stem_conv_training is False                                   # and stays off until asked for again


def test_run_stem_does_not_route_on_the_cpu_or_outside_the_context(monkeypatch):
    routed = []
    monkeypatch.setattr(features, "stem_conv_bf16_op", lambda layer, t: routed.append(layer))
    conv, bn, pool = _stem(), nn.BatchNorm2d(64), nn.MaxPool2d(3, 2, 1)
    x = torch.zeros(2, 3, 16, 16)
    with features.native_stem_conv_bf16_training():
        features.run_stem(conv, bn, pool, x)
        features.run_stem(conv, bn, pool, x.to(BF).float())
    features.run_stem(conv, bn, pool, x)
    assert routed == []
    # inside the context, tracked, a bf16 input, the predicate satisfied: routed
    xg = _OnGpu(torch.zeros(2, 3, 16, 16, dtype=BF))
    assert features._stem_conv_bf16_routed(conv, xg) is False
    with features.native_stem_conv_bf16_training():
        assert features._stem_conv_bf16_routed(conv, xg) is True
        assert features._stem_conv_bf16_routed(conv, _OnGpu(torch.zeros(2, 3, 16, 16))) is False      # fp32, no autocast
        with torch.no_grad():
            assert features._stem_conv_bf16_routed(conv, xg) is False
        assert features._stem_conv_bf16_routed(_stem().requires_grad_(False), xg) is False
        assert features._stem_conv_bf16_routed(conv, _OnGpu(torch.zeros(2, 3, 16, 15, dtype=BF))) is False


@pytest.mark.parametrize("shape,k,pad,dtype", [((3, 3, 30, 50), 7, 3, torch.float32), ((2, 1, 17, 34), 5, 2, BF),
                                               ((1, 4, 16, 16), 8, 2, BF)])
def test_fake_kernels_shapes_dtypes_and_layouts(shape, k, pad, dtype):
    x = torch.empty(shape, device="meta", dtype=dtype)                    # NCHW, as the instances come
    w = torch.empty(64, shape[1], k, k, device="meta")
    y = torch.ops.mcgmil.stem_conv_bf16(x, w, 2, pad)
    oh, ow = (shape[2] + 2 * pad - k) // 2 + 1, (shape[3] + 2 * pad - k) // 2 + 1
    assert y.shape == (shape[0], 64, oh, ow) and y.dtype == BF and y.device.type == "meta"
    assert y.is_contiguous(memory_format=CL) and y.stride(1) == 1
    dx, dw = torch.ops.mcgmil.stem_conv_bf16_backward(x, w, y, 2, pad, True, True)
    assert dx.shape == x.shape and dx.dtype == BF and dx.is_contiguous(memory_format=CL)
    assert dw.shape == w.shape and dw.dtype == torch.float32 and dw.is_contiguous()
    _, dwb = torch.ops.mcgmil.stem_conv_bf16_backward(x, w.to(BF), y, 2, pad, False, True)
    assert dwb.dtype == BF                                                # in the weight's dtype
    dx, dw = torch.ops.mcgmil.stem_conv_bf16_backward(x, w, y, 2, pad, False, False)
    assert dx.numel() == 0 and dw.numel() == 0


def test_schemas_and_all():
    assert library.STEM_BF16_OPS == ("stem_conv_bf16", "stem_conv_bf16_backward")
    assert str(torch.ops.mcgmil.stem_conv_bf16.default._schema) == \
        "mcgmil::stem_conv_bf16(Tensor x, Tensor weight, SymInt stride, SymInt pad) -> Tensor"
    assert str(torch.ops.mcgmil.stem_conv_bf16_backward.default._schema) == \
        "mcgmil::stem_conv_bf16_backward(Tensor x, Tensor weight, Tensor dy, SymInt stride, SymInt pad, " \
        "bool need_dx, bool need_dw) -> (Tensor, Tensor)"
    # the sibling's schema, argument for argument
    assert str(torch.ops.mcgmil.stem_conv_bf16.default._schema).replace("bf16", "f32") == \
        str(torch.ops.mcgmil.stem_conv_f32.default._schema)
    # __all__ is what the recorded fixture lists, and the new names are not in it
    with open(os.path.join(REPO, "tests", "fixtures", "features_bindings.json")) as f:
        recorded = json.load(f)["schemas"]
    assert sorted(library.__all__) == sorted(recorded) and len(library.__all__) == 17
    assert not set(library.STEM_BF16_OPS) & set(library.__all__)
    for name in library.STEM_BF16_OPS:
        assert hasattr(library, name) and name in library.__doc__
    # the backward op has no autograd formula
    assert "stem_conv_bf16_backward" in library.__doc__ and "no formula" in library.__doc__


def _grad_args(**kw):
    g = _lib.StemGradBf16Args()
    a = g.fwd
    a.batch, a.in_channels, a.height, a.width, a.out_channels = 4, 3, 224, 224, 64
    a.kernel, a.stride, a.pad = 7, 2, 3
    a.x, g.dy, g.dw = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)   # never dereferenced
    for key, v in kw.items():
        setattr(g if key in ("dy", "dw", "workspace", "workspace_bytes", "reserved", "chunk_pixels") else a, key, v)
    return g


def test_symbols_struct_size_and_abi():
    assert _lib.STEM_GRAD_BF16_EXPORTED == ("mcgmil_stem_conv_bf16", "mcgmil_stem_grad_bf16_args_size",
                                            "mcgmil_stem_wgrad_workspace_size_bf16", "mcgmil_stem_wgrad_bf16")
    assert not set(_lib.STEM_GRAD_BF16_EXPORTED) & set(_lib.EXPORTED)
    L = _lib.load()
    assert _lib.ABI_VERSION == 6 and L.mcgmil_abi_version() == 6
    psg, ps = ctypes.POINTER(_lib.StemGradBf16Args), ctypes.POINTER(_lib.StemArgs)
    assert L.mcgmil_stem_conv_bf16.argtypes == [ps, ctypes.c_void_p] and L.mcgmil_stem_conv_bf16.restype is ctypes.c_int
    assert L.mcgmil_stem_grad_bf16_args_size.restype is ctypes.c_size_t
    assert L.mcgmil_stem_wgrad_workspace_size_bf16.argtypes == [psg, ctypes.POINTER(ctypes.c_size_t)]
    assert L.mcgmil_stem_wgrad_bf16.argtypes == [psg, ctypes.c_void_p] and L.mcgmil_stem_wgrad_bf16.restype is ctypes.c_int
    assert L.mcgmil_stem_grad_bf16_args_size() == ctypes.sizeof(_lib.StemGradBf16Args)
    assert [n for n, _ in _lib.StemGradBf16Args._fields_] == ["fwd", "dy", "dw", "workspace", "workspace_bytes",
                                                              "chunk_pixels", "reserved"]
    assert _lib.StemGradBf16Args.fwd.size == ctypes.sizeof(_lib.StemArgs)
    # declared in the header of its own, in none of the four whose functions must equal EXPORTED
    inc = os.path.join(REPO, "include")
    with open(os.path.join(inc, "mcgmil_stem_grad_bf16.h")) as f:
        own = f.read()
    for name in _lib.STEM_GRAD_BF16_EXPORTED:
        assert name + "(" in own, name
        for h in ("mcgmil.h", "mcgmil_image.h", "mcgmil_features.h", "mcgmil_calib.h"):
            with open(os.path.join(inc, h)) as f:
                assert name not in f.read(), (name, h)
    assert "mcgmil_stem_grad_bf16.hip" in _build.SOURCES and "mcgmil_stem_grad_bf16.hip" in _build.DEPS


def _size(g):
    n = ctypes.c_size_t(12345)
    rc = _lib.load().mcgmil_stem_wgrad_workspace_size_bf16(ctypes.byref(g), ctypes.byref(n))
    assert rc == 0 or (n.value == 12345 and len(_lib.load().mcgmil_last_error()) > 0)
    return rc, n.value


def test_workspace_arithmetic():
    E4 = 64 * 3 * 7 * 8 * 4                                     # E = 64 x 168 columns, the dead tap's included
    pixels = 4 * 112 * 112                                      # 50,176: 24.5 granules
    assert _size(_grad_args()) == (0, (1 + 25) * E4)            # chunk_pixels 0: every granule fits the default cap
    assert _size(_grad_args(chunk_pixels=G)) == (0, (1 + 1) * E4)
    assert _size(_grad_args(chunk_pixels=1)) == (0, (1 + 1) * E4)
    assert _size(_grad_args(chunk_pixels=3 * G + 7)) == (0, (1 + 3) * E4)
    assert _size(_grad_args(chunk_pixels=1 << 40)) == (0, (1 + -(-pixels // G)) * E4)
    assert _size(_grad_args(batch=1507)) == (0, (1 + (128 << 20) // E4) * E4)       # the default cap on the partials
    for cin, k, pad in ((1, 5, 2), (4, 3, 1), (2, 6, 2), (4, 8, 2)):
        g = _grad_args(in_channels=cin, kernel=k, pad=pad, height=16, width=16)
        assert _size(g) == (0, 2 * 64 * cin * k * 8 * 4), (cin, k, pad)


@pytest.mark.parametrize("bad,code,word", [
    (dict(batch=0), INVALID, "batch"), (dict(height=0), INVALID, "height"), (dict(width=0), INVALID, "width"),
    (dict(in_channels=0), UNSUPPORTED, "in_channels"), (dict(in_channels=5), UNSUPPORTED, "in_channels"),
    (dict(out_channels=128), UNSUPPORTED, "64 output"), (dict(stride=1), UNSUPPORTED, "stride 2"),
    (dict(kernel=8), UNSUPPORTED, "kernel"), (dict(kernel=9, pad=4), UNSUPPORTED, "kernel"), (dict(kernel=0), UNSUPPORTED, "kernel"),
    (dict(pad=-1), UNSUPPORTED, "kernel"), (dict(width=223), UNSUPPORTED, "even"), (dict(width=252), UNSUPPORTED, "125"),
    (dict(height=2, width=2, pad=0), INVALID, "fit"), (dict(batch=7134), UNSUPPORTED, "2 GiB"),
    (dict(reserved=1), INVALID, "reserved"), (dict(chunk_pixels=-1), INVALID, "chunk_pixels"),
])
def test_geometry_validation_of_the_gradient_entries(bad, code, word):
    L = _lib.load()
    g = _grad_args(**bad)
    assert _size(g)[0] == code and word.encode() in L.mcgmil_last_error()
    assert L.mcgmil_stem_wgrad_bf16(ctypes.byref(g), None) == code and word.encode() in L.mcgmil_last_error()


def test_pointer_and_workspace_validation_of_the_weight_gradient():
    L = _lib.load()
    run = lambda g: L.mcgmil_stem_wgrad_bf16(ctypes.byref(g), None)  # noqa: E731
    assert L.mcgmil_stem_wgrad_workspace_size_bf16(None, ctypes.byref(ctypes.c_size_t())) == INVALID
    assert L.mcgmil_stem_wgrad_workspace_size_bf16(ctypes.byref(_grad_args()), None) == INVALID
    assert L.mcgmil_stem_wgrad_bf16(None, None) == INVALID
    for key in ("x", "dy", "dw"):
        assert run(_grad_args(**{key: None})) == INVALID and b"NULL" in L.mcgmil_last_error(), key
    for key, v in (("x", 0x10002), ("dy", 0x20008), ("dw", 0x30004)):
        assert run(_grad_args(**{key: ctypes.c_void_p(v)})) == ALIGN, key
    rc, need = _size(_grad_args())
    assert run(_grad_args()) == WORKSPACE                         # a NULL workspace
    assert run(_grad_args(x=ctypes.c_void_p(0x10004))) == WORKSPACE        # a 4-byte aligned x is enough
    assert run(_grad_args(workspace=ctypes.c_void_p(0x100000), workspace_bytes=need - 1)) == WORKSPACE
    assert run(_grad_args(workspace=ctypes.c_void_p(0x100010), workspace_bytes=need)) == ALIGN
    # the forward's other fields are ignored, not validated
    g = _grad_args(flags=0x7fff, pool_kernel=-4, relu=7, gamma=ctypes.c_void_p(0x7), w=ctypes.c_void_p(0x3))
    g.fwd.reserved = 9
    assert _size(g) == (0, need)


def test_validation_of_the_forward_entry():
    L = _lib.load()

    def rc_of(**kw):
        a = _grad_args().fwd
        a.w, a.y = ctypes.c_void_p(0x40000), ctypes.c_void_p(0x50000)
        for key, v in kw.items():
            setattr(a, key, v)
        rc = L.mcgmil_stem_conv_bf16(ctypes.byref(a), None)
        assert rc != 0 and len(L.mcgmil_last_error()) > 0
        return rc
    assert L.mcgmil_stem_conv_bf16(None, None) == INVALID
    p = ctypes.c_void_p(0x60000)
    for bad, code in ((dict(in_channels=5), UNSUPPORTED), (dict(out_channels=128), UNSUPPORTED), (dict(stride=1), UNSUPPORTED),
                      (dict(kernel=8), UNSUPPORTED), (dict(width=223), UNSUPPORTED), (dict(width=252), UNSUPPORTED),
                      (dict(batch=7134), UNSUPPORTED), (dict(batch=0), INVALID), (dict(relu=2), INVALID), (dict(flags=7), INVALID),
                      (dict(reserved=1), INVALID), (dict(pool_kernel=3, pool_stride=2, pool_pad=1), INVALID),
                      (dict(pool_kernel=-1), INVALID), (dict(gamma=p), INVALID), (dict(beta=p), INVALID),
                      (dict(running_mean=p), INVALID), (dict(running_var=p), INVALID), (dict(running_mean=p, running_var=p), INVALID),
                      (dict(batch_mean=p), INVALID), (dict(batch_invstd=p), INVALID),
                      (dict(x=None), INVALID), (dict(w=None), INVALID), (dict(y=None), INVALID),
                      (dict(x=ctypes.c_void_p(0x10002)), ALIGN), (dict(w=ctypes.c_void_p(0x40008)), ALIGN),
                      (dict(y=ctypes.c_void_p(0x50008)), ALIGN)):
        assert rc_of(**bad) == code, bad
    assert b"pool_kernel" in (rc_of(pool_kernel=3, pool_stride=2, pool_pad=1), L.mcgmil_last_error())[1]
    assert b"BatchNorm" in (rc_of(gamma=p), L.mcgmil_last_error())[1]
