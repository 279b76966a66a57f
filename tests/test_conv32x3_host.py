"""Host-side checks of the fp32 convolution on split-bf16 MFMA (mcgmil_conv2d_f32x3, "bf16x3";
include/mcgmil_features.h), no kernel launches: the numerics contract on tests/conv32x3_ref.py's
emulation (so the GPU tests' reference and bounds stand without a GPU), the predicate's refusal
reasons, the precedence of keyword, context manager and environment, model.feature_precision, and
the four entry points' validation through the library."""
import ctypes

import pytest
import torch
import torch.nn as nn

import conv32x3_ref as ref
from mcgmil import _lib, features
from mcgmil.model import MultiHeadGatedAttentionMIL

INVALID, UNSUPPORTED, ALIGN = -1, -2, -3                # enum mcgmil_status (include/mcgmil.h)


# ---------------------------------------------------------------------------------- numerics
def test_split_is_exact_and_small():
    g = torch.Generator().manual_seed(0)
    v = torch.cat([torch.randn(1 << 16, generator=g) * s for s in (1e-20, 1e-3, 1.0, 1e4, 1e30)])
    hi, lo = ref.split(v)
    d = v - hi                                         # fp32 subtraction ...
    assert torch.equal(d.double(), v.double() - hi.double())          # ... is exact
    assert torch.equal(hi, hi.bfloat16().float()) and torch.equal(lo, lo.bfloat16().float())
    assert bool(((v.double() - hi.double() - lo.double()).abs() <= 2.0 ** -16 * v.double().abs()).all())
    assert bool((lo.abs() <= 2.0 ** -8 * v.abs()).all())


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_emulation_within_the_derived_bound(shape):
    x, w, stride, pad = ref.make_case(shape, ref.SHAPES.index(shape))
    ref64 = ref.conv64(x, w, stride, pad)
    mag = ref.conv64(x.abs(), w.abs(), stride, pad)
    emu = ref.conv_x3(x, w, stride, pad)
    err = (emu - ref64).abs()
    worst = float((err / mag.clamp_min(1e-300)).max())
    n3, n1 = ref.nrel(emu, ref64), ref.nrel(ref.conv_hi(x, w, stride, pad), ref64)
    print(f"{ref.shape_id(shape)}: max err / conv(|x|,|w|) {worst:.2e} / {ref.SPLIT_BOUND:.2e}; "
          f"nrel bf16x3 {n3:.2e}, hi*hi only {n1:.2e}, ratio {n1 / n3:.0f}")
    assert bool((err <= ref.SPLIT_BOUND * mag).all())
    assert n3 <= ref.HI_ONLY_RATIO * n1


# ---------------------------------------------------------------------------------- predicate
def _conv(cin=64, cout=64, k=3, **kw):
    return nn.Conv2d(cin, cout, k, 1, 1, **dict(dict(bias=False), **kw)).requires_grad_(False)


def _x(c=64, dtype=torch.float32):
    return torch.zeros(2, c, 6, 6, dtype=dtype).contiguous(memory_format=torch.channels_last)


class _Cuda(torch.Tensor):
    """A CPU tensor that reports is_cuda: the clauses are walked, no GPU is touched."""
    is_cuda = True


def test_refusal_reasons(monkeypatch):
    monkeypatch.delenv("MCGMIL_NATIVE_CONV32", raising=False)
    monkeypatch.delenv("MCGMIL_NATIVE_CONV", raising=False)
    why = features.conv32x3_unfusable_reason
    assert why(_conv(), _x().as_subclass(_Cuda)) is None and features.conv32x3_fusable(_conv(), _x().as_subclass(_Cuda))
    for cin in (16, 48):                                                              # Cin % 32
        assert "multiple of 32" in why(_conv(cin), _x(cin))
    assert "multiple of 32" in why(nn.Conv2d(3, 64, 7, 2, 3, bias=False).requires_grad_(False),
                                   _x(3))                                             # the stem (gather)
    assert "must be fp32" in why(_conv(), _x(dtype=torch.bfloat16))                   # bf16 input
    assert "channels-last" in why(_conv(), torch.zeros(2, 64, 6, 6))                  # NCHW
    assert "bias-free" in why(_conv(bias=True), _x())
    assert "bias-free" in why(_conv(groups=2), _x())
    assert "multiple of 64" in why(_conv(cout=96), _x())
    assert "autograd" in why(_conv().requires_grad_(True), _x())
    with torch.no_grad():
        assert why(_conv().requires_grad_(True), _x()) == "the activation is not a CUDA tensor"
    assert why(_conv(), _x()) == "the activation is not a CUDA tensor"                # the device comes last
    assert not features.conv32x3_fusable(_conv(), _x())
    assert why(nn.Identity(), _x()) == "not an nn.Conv2d"
    monkeypatch.setenv("MCGMIL_NATIVE_CONV32", "0")
    assert "switched off" in why(_conv(), _x().as_subclass(_Cuda))
    # the exact kernel's predicate still asks for the device with the rank
    monkeypatch.delenv("MCGMIL_NATIVE_CONV32")
    assert not features.conv32_fusable(_conv(), _x())
    assert features.conv32_fusable(_conv(), _x().as_subclass(_Cuda))


# ---------------------------------------------------------------------------------- precedence
def test_keyword_over_context_over_environment(monkeypatch):
    """Which entry point conv2d_f32 calls, with the library replaced by a recorder."""
    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append(name) or 0

    monkeypatch.setattr(features._lib, "load", lambda: Lib())
    monkeypatch.setattr(features, "_ptr", lambda t: None)
    monkeypatch.setattr(features, "_stream", lambda dev: None)
    monkeypatch.setattr(features, "packed_conv_weight_f32", lambda conv, x: None)
    monkeypatch.setattr(features, "packed_conv_weight_f32x3", lambda conv, x: None)
    conv, x = _conv(), _x().as_subclass(_Cuda)
    conv16, x16 = _conv(16), _x(16).as_subclass(_Cuda)

    def kernel(*a, **k):
        del calls[:]
        features.conv2d_f32(*a, **k)
        return calls[-1]

    monkeypatch.delenv("MCGMIL_CONV32_PRECISION", raising=False)
    assert features.conv32_precision() == "fp32"
    assert kernel(conv, x) == "mcgmil_conv2d_f32"
    assert kernel(conv, x, precision="bf16x3") == "mcgmil_conv2d_f32x3"
    assert kernel(conv, x, stats=True, precision="bf16x3") == "mcgmil_conv2d_f32x3"
    assert calls == ["mcgmil_conv_stats_parts_f32x3", "mcgmil_conv2d_f32x3"]
    monkeypatch.setenv("MCGMIL_CONV32_PRECISION", "bf16x3")                          # read on every call
    assert features.conv32_precision() == "bf16x3"
    assert kernel(conv, x) == "mcgmil_conv2d_f32x3"
    assert kernel(conv16, x16) == "mcgmil_conv2d_f32"                                # outside the domain: exact
    assert kernel(conv, x, precision="fp32") == "mcgmil_conv2d_f32"                  # keyword over environment
    with features.float32_conv_precision("fp32"):                                    # context over environment
        assert features.conv32_precision() == "fp32"
        assert kernel(conv, x) == "mcgmil_conv2d_f32"
        assert kernel(conv, x, precision="bf16x3") == "mcgmil_conv2d_f32x3"          # keyword over context
        with features.float32_conv_precision("bf16x3"):
            assert kernel(conv, x) == "mcgmil_conv2d_f32x3"
        assert kernel(conv, x) == "mcgmil_conv2d_f32"
    assert kernel(conv, x) == "mcgmil_conv2d_f32x3"
    monkeypatch.setenv("MCGMIL_CONV32_PRECISION", "BF16X3")                          # anything else: fp32
    assert features.conv32_precision() == "fp32" and kernel(conv, x) == "mcgmil_conv2d_f32"
    with features.float32_conv_precision("bf16x3"):
        assert kernel(conv, x) == "mcgmil_conv2d_f32x3"
        assert kernel(conv, x, precision="fp32") == "mcgmil_conv2d_f32"
        with pytest.raises(ValueError, match="multiple of 32"):
            features.conv2d_f32(conv16, x16, precision="bf16x3")
    with pytest.raises(ValueError):
        features.conv2d_f32(conv, x, precision="tf32")
    with pytest.raises(ValueError):
        with features.float32_conv_precision("bf16"):
            pass
    assert features._conv32_precision is None


def test_model_feature_precision_validation():
    m = MultiHeadGatedAttentionMIL(pretrained=False)
    assert m.feature_precision == "fp32"
    m.feature_precision = "bf16x3"
    assert m.feature_precision == "bf16x3"
    for bad in ("bf16", "tf32", None, torch.float32):
        with pytest.raises(ValueError):
            m.feature_precision = bad
    assert m.feature_precision == "bf16x3"
    m.feature_precision = "fp32"
    assert m.feature_precision == "fp32" and m.compute_dtype == torch.float32


def test_extract_features_runs_under_the_matching_context(monkeypatch):
    m = MultiHeadGatedAttentionMIL(pretrained=False)
    seen = []
    monkeypatch.delenv("MCGMIL_CONV32_PRECISION", raising=False)

    class Probe(nn.Module):
        def forward(self, t):
            seen.append(features.conv32_precision())
            return torch.zeros(t.shape[0], 512)

    m.feature_extractor = Probe()
    x = torch.zeros(1, 2, 3, 8, 8)
    m.extract_features(x)
    m.feature_precision = "bf16x3"
    m.extract_features(x)
    m.feature_precision = "fp32"
    monkeypatch.setenv("MCGMIL_CONV32_PRECISION", "bf16x3")                          # "fp32" leaves the ambient setting
    m.extract_features(x)
    assert seen == ["fp32", "bf16x3", "bf16x3"] and features._conv32_precision is None


# ---------------------------------------------------------------------------------- the library
def conv_args(N=2, Cin=64, H=10, W=10, Cout=128, kh=3, kw=3, s=1, p=1):
    a = _lib.ConvArgs()
    a.batch, a.in_channels, a.height, a.width, a.out_channels = N, Cin, H, W, Cout
    a.kernel_h, a.kernel_w, a.stride, a.pad = kh, kw, s, p
    return a


def _sizes(L, a):
    n, parts = ctypes.c_size_t(), ctypes.c_int32()
    return (L.mcgmil_conv_packed_size_f32x3(ctypes.byref(a), ctypes.byref(n)), n.value,
            L.mcgmil_conv_stats_parts_f32x3(ctypes.byref(a), ctypes.byref(parts)), parts.value)


def test_entry_points_sizes_and_abi(hip_lib):
    assert hip_lib.mcgmil_abi_version() == 6
    for f in ("mcgmil_conv2d_f32x3", "mcgmil_pack_conv_weights_f32x3", "mcgmil_conv_packed_size_f32x3",
              "mcgmil_conv_stats_parts_f32x3"):
        assert hasattr(hip_lib, f) and f in _lib.EXPORTED, f
    assert _sizes(hip_lib, conv_args()) == (0, 3 * 3 * 64 * 128, 0, 2)                 # 200 pixels, 128-pixel tiles
    assert _sizes(hip_lib, conv_args(Cout=192)) == (0, 3 * 3 * 64 * 192, 0, 1)         # 256-pixel tiles
    assert _sizes(hip_lib, conv_args(Cin=2048, Cout=2048, kh=1, kw=1, p=0)) == (0, 2048 * 2048, 0, 2)
    f32 = ctypes.c_int32()
    assert hip_lib.mcgmil_conv_stats_parts_f32(ctypes.byref(conv_args()), ctypes.byref(f32)) == 0 and f32.value == 2


def test_entry_points_refuse_what_is_outside_the_domain(hip_lib):
    L = hip_lib
    for change in (dict(Cin=3, kh=7, kw=7, s=2, p=3), dict(Cin=16), dict(Cin=48), dict(Cin=24, kh=1, kw=1),
                   dict(Cout=96), dict(Cout=32), dict(kh=8), dict(kw=8)):
        a = conv_args(**change)
        assert _sizes(L, a)[::2] == (UNSUPPORTED, UNSUPPORTED), change
        assert L.mcgmil_conv2d_f32x3(ctypes.byref(a), None) == UNSUPPORTED, change
        assert L.mcgmil_pack_conv_weights_f32x3(ctypes.byref(a), None, None, None) == UNSUPPORTED, change
        assert len(L.mcgmil_last_error()) > 0
    assert b"multiple of 32" in (L.mcgmil_conv2d_f32x3(ctypes.byref(conv_args(Cin=16)), None) and L.mcgmil_last_error())
    for change in (dict(N=0), dict(s=0), dict(p=-1), dict(H=1, W=1, p=0)):
        a = conv_args(**change)
        assert _sizes(L, a)[::2] == (INVALID, INVALID), change
        assert L.mcgmil_conv2d_f32x3(ctypes.byref(a), None) == INVALID, change
    a = conv_args()
    a.in_relu = 2
    assert L.mcgmil_conv2d_f32x3(ctypes.byref(a), None) == INVALID
    # in_ab past 2,048 input channels, as mcgmil_conv2d_f32
    a = conv_args(Cin=4096, kh=1, kw=1, p=0)
    assert _sizes(L, a)[0] == 0
    a.in_ab = 0x1000
    assert L.mcgmil_conv2d_f32x3(ctypes.byref(a), None) == UNSUPPORTED


def test_entry_points_null_and_misaligned_pointers(hip_lib):
    """Refused before anything is launched: the pointers are never dereferenced."""
    L = hip_lib
    for f in (L.mcgmil_conv_packed_size_f32x3, L.mcgmil_conv_stats_parts_f32x3):
        assert f(None, None) == INVALID
        assert f(ctypes.byref(conv_args()), None) == INVALID
    assert L.mcgmil_conv2d_f32x3(None, None) == INVALID
    assert L.mcgmil_pack_conv_weights_f32x3(None, None, None, None) == INVALID
    a = conv_args()
    assert L.mcgmil_conv2d_f32x3(ctypes.byref(a), None) == INVALID                       # NULL x, w, y
    assert L.mcgmil_pack_conv_weights_f32x3(ctypes.byref(a), None, None, None) == INVALID
    assert L.mcgmil_pack_conv_weights_f32x3(ctypes.byref(a), ctypes.c_void_p(0x1000), None, None) == INVALID
    assert L.mcgmil_pack_conv_weights_f32x3(ctypes.byref(a), ctypes.c_void_p(0x1002), ctypes.c_void_p(0x2000),
                                            None) == ALIGN
    assert L.mcgmil_pack_conv_weights_f32x3(ctypes.byref(a), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2008),
                                            None) == ALIGN
    for field, value in (("x", 0x1004), ("w", 0x2008), ("y", 0x3002), ("stats", 0x4002), ("in_ab", 0x5004)):
        a = conv_args()
        a.x, a.w, a.y = 0x1000, 0x2000, 0x3000
        setattr(a, field, value)
        assert L.mcgmil_conv2d_f32x3(ctypes.byref(a), None) == ALIGN, field
        assert b"aligned" in L.mcgmil_last_error()
