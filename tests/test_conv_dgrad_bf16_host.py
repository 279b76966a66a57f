"""Host-side checks of the bf16 direct convolution data gradient
(include/mcgmil_conv_dgrad_bf16.h; no kernel launches): the residue-class decomposition on the
bf16-rounded inputs against float64 autograd (so the references of the GPU tests stand without a
GPU), the launch arithmetic of mcgmil_conv_dgrad_classes_bf16 against the restatement, the limits,
the validation order, the binding, the predicate and the route table of conv2d_bf16_backward."""
import ctypes

import pytest
import torch

import conv_dgrad_bf16_ref as ref
from mcgmil import _lib, features

INVALID, UNSUPPORTED = -1, -2                # enum mcgmil_status (include/mcgmil.h)


def dgrad_args(N, Cin, Cout, kh, kw, s, p, H, W):
    g = _lib.ConvDgradBf16Args()
    a = g.fwd
    a.batch, a.in_channels, a.out_channels, a.height, a.width = N, Cin, Cout, H, W
    a.kernel_h, a.kernel_w, a.stride, a.pad = kh, kw, s, p
    return g


def classes_of(L, g):
    taps, pixels, tiles = (ctypes.c_int32 * 4)(), (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
    rc = L.mcgmil_conv_dgrad_classes_bf16(ctypes.byref(g), taps, pixels, tiles)
    return rc, list(taps), list(pixels), list(tiles)


def case_args(name):
    N, Cin, Cout, k, s, p, H, W = ref.CASES[name]
    return dgrad_args(N, Cin, Cout, *ref.kernel_hw(k), s, p, H, W)


@pytest.mark.parametrize("name", ref.TABLE)
def test_decomposition_equals_float64_autograd(name):
    c = ref.case(name)
    dx, _ = ref.dgrad_classes(c.dy.double(), c.w.double(), c.stride, c.pad, c.x.shape)
    assert not bool(torch.isnan(dx).any())                       # every element written
    err = float((dx - c.dx64).abs().max())
    print(f"{name}: max|decomposition - autograd| = {err:.2e} / 1e-12")
    assert err <= 1e-12


EXPECTED = {
    "s2_3x3_even": [(4, 50), (2, 50), (2, 50), (1, 50)],
    "s2_1x1": [(1, 50), (0, 50), (0, 40), (0, 40)],
    "s2_7x7": [(16, 20), (12, 25), (12, 24), (9, 30)],
    "s2_3x5": [(6, 16), (4, 20), (3, 20), (2, 25)],
    "s1_3x5": [(15, 84), (0, 0), (0, 0), (0, 0)],
}


@pytest.mark.parametrize("name", ref.TABLE)
def test_classes_agree_with_the_restatement(hip_lib, name):
    N, Cin, Cout, k, s, p, H, W = ref.CASES[name]
    c = ref.case(name)
    _, want = ref.dgrad_classes(c.dy.double(), c.w.double(), s, p, c.x.shape)
    rc, taps, pixels, tiles = classes_of(hip_lib, case_args(name))
    assert rc == 0
    got = list(zip(taps, pixels))
    assert got[:s * s] == want and got[s * s:] == [(0, 0)] * (4 - s * s)
    if name in EXPECTED:
        assert got == EXPECTED[name]
    tile = 256 if Cin == 64 else 128
    assert tiles == [-(-px // tile) for px in pixels]
    assert sum(pixels) == N * H * W


@pytest.mark.parametrize("name,tile,tiles", [("s2_c64_two_tiles", 256, 2), ("s2_c192_two_tiles", 128, 3)])
def test_two_tiles_cases_span_tiles_with_a_ragged_last_one(hip_lib, name, tile, tiles):
    rc, _, pixels, got = classes_of(hip_lib, case_args(name))
    assert rc == 0 and pixels == [330] * 4 and got == [tiles] * 4
    assert 330 % tile != 0 and tiles >= 2                         # the last tile of every class is ragged


def test_limits(hip_lib):
    # 2^31 input pixels in the one class of a stride-1 convolution, and in each of four classes
    assert classes_of(hip_lib, dgrad_args(1 << 11, 64, 64, 1, 1, 1, 0, 1 << 10, 1 << 10))[0] == UNSUPPORTED
    assert len(hip_lib.mcgmil_last_error()) > 0
    assert classes_of(hip_lib, dgrad_args(1 << 13, 64, 64, 3, 3, 2, 1, 1 << 10, 1 << 10))[0] == UNSUPPORTED
    # pixels * channels past 64 bits
    assert classes_of(hip_lib, dgrad_args(0x7fffffff, 0x7fffffc0, 64, 1, 1, 1, 0, 0x7fffffff, 0x7fffffff))[0] == \
        UNSUPPORTED
    # dx of exactly 2^31 bytes (2^24 pixels x 64 channels x 2 bytes); dy is a quarter of it
    assert classes_of(hip_lib, dgrad_args(1 << 4, 64, 64, 3, 3, 2, 1, 1 << 10, 1 << 10))[0] == UNSUPPORTED
    # dy of exactly 2^31 bytes (2^22 pixels x 256 channels x 2 bytes); dx is half of it
    assert classes_of(hip_lib, dgrad_args(1 << 2, 64, 256, 1, 1, 1, 0, 1 << 10, 1 << 10))[0] == UNSUPPORTED
    # just below: one image less than 2^31 bytes of dx ...
    rc, taps, pixels, tiles = classes_of(hip_lib, dgrad_args(15, 64, 64, 3, 3, 2, 1, 1 << 10, 1 << 10))
    assert rc == 0 and pixels == [15 << 18] * 4 and tiles == [15 << 10] * 4 and taps == [4, 2, 2, 1]
    # ... and one row less than 2^31 bytes of dy
    rc, taps, pixels, tiles = classes_of(hip_lib, dgrad_args(1 << 2, 64, 256, 1, 1, 1, 0, (1 << 10) - 1, 1 << 10))
    assert rc == 0 and pixels == [((1 << 10) - 1) << 12, 0, 0, 0] and taps == [1, 0, 0, 0]


def test_validation_order(hip_lib):
    """Each call breaks one more rule than the one before it; the first broken rule answers."""
    ok = dict(N=2, Cin=64, Cout=128, kh=3, kw=3, s=2, p=1, H=10, W=10)
    assert classes_of(hip_lib, dgrad_args(**ok))[0] == 0
    assert hip_lib.mcgmil_conv_dgrad_classes_bf16(None, None, None, None) == INVALID
    assert hip_lib.mcgmil_conv2d_dgrad_bf16(None, None) == INVALID
    # (rule broken, its code, its message), from the one checked last to the one checked first
    rules = [(dict(H=1, W=1, p=0), INVALID, b"does not fit"),
             (dict(p=3), UNSUPPORTED, b"pad must be smaller"),
             (dict(s=3), UNSUPPORTED, b"stride 1 or 2"),
             (dict(Cin=96), UNSUPPORTED, b"in_channels a multiple of 64")]
    for i, (_, code, message) in enumerate(rules):
        bad = dict(ok)
        for change, _, _ in rules[:i + 1]:
            bad.update(change)
        assert classes_of(hip_lib, dgrad_args(**bad))[0] == code, bad
        assert message in hip_lib.mcgmil_last_error(), (bad, hip_lib.mcgmil_last_error())
    bad = dict(ok, H=1, W=1, p=0, s=3, Cin=96)
    g = dgrad_args(**bad)
    g.reserved = 1                                                # reserved answers before the geometry
    assert classes_of(hip_lib, g)[0] == INVALID and b"reserved" in hip_lib.mcgmil_last_error()
    for change in (dict(Cin=48), dict(Cin=16), dict(Cout=96), dict(Cout=32), dict(kh=8), dict(kw=8)):
        assert classes_of(hip_lib, dgrad_args(**dict(ok, **change)))[0] == UNSUPPORTED, change
    assert hip_lib.mcgmil_conv_dgrad_classes_bf16(ctypes.byref(dgrad_args(**ok)), None, None, None) == INVALID
    # without a launch: NULL pointers are refused before anything runs
    assert hip_lib.mcgmil_conv2d_dgrad_bf16(ctypes.byref(dgrad_args(**ok)), None) == INVALID


def test_struct_size_matches_the_binding(hip_lib):
    assert hip_lib.mcgmil_conv_dgrad_bf16_args_size() == ctypes.sizeof(_lib.ConvDgradBf16Args)
    assert _lib.CONV_DGRAD_BF16_EXPORTED == ("mcgmil_conv_dgrad_bf16_args_size", "mcgmil_conv_dgrad_classes_bf16",
                                             "mcgmil_conv2d_dgrad_bf16")
    for f in _lib.CONV_DGRAD_BF16_EXPORTED:
        assert hasattr(hip_lib, f), f


def test_predicate_verdicts_without_a_device():
    conv = features._ConvShim(torch.zeros(64, 64, 3, 3), 2, 1)
    assert not features.dgrad_bf16_direct_supported(conv, torch.zeros(1, 64, 4, 4))                        # fp32, CPU
    assert not features.dgrad_bf16_direct_supported(conv, torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16))  # CPU
    with pytest.raises(ValueError):
        features.conv2d_bf16_dgrad_direct(conv, torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16), (1, 64, 8, 8))


def test_predicate_verdicts_behind_the_device_clause():
    """The clauses behind the device clause, on a CPU tensor that reports is_cuda: no GPU is touched."""
    class Cuda(torch.Tensor):
        is_cuda = True

    def dy(dtype=torch.bfloat16, channels=64):
        return torch.zeros(1, channels, 4, 4, dtype=dtype).as_subclass(Cuda)
    conv = features._ConvShim(torch.zeros(64, 64, 3, 3), 2, 1)
    assert features.dgrad_bf16_direct_supported(conv, dy())
    assert features.dgrad_bf16_direct_supported(features._ConvShim(torch.zeros(64, 64, 3, 5), 1, 1), dy())
    assert features.dgrad_bf16_direct_supported(features._ConvShim(torch.zeros(64, 64, 3, 3, dtype=torch.bfloat16), 2, 1),
                                                dy())
    assert not features.dgrad_bf16_direct_supported(conv, dy(torch.float32))                 # fp32 dy
    assert not features.dgrad_bf16_direct_supported(features._ConvShim(torch.zeros(64, 48, 3, 3), 2, 1), dy())   # Cin 48
    dilated = features._ConvShim(torch.zeros(64, 64, 3, 3), 2, 1)
    dilated.dilation = (2, 2)
    assert not features.dgrad_bf16_direct_supported(dilated, dy())                           # dilation 2
    assert not features.dgrad_bf16_direct_supported(conv, dy(channels=128))                  # not this conv's dY


@pytest.mark.parametrize("route,want", [
    ("direct", {"s1": "dgrad", "s2": "direct", "s1_3x5": "direct"}),
    ("native", {"s1": "dgrad", "s2": "dgrad", "s1_3x5": "dgrad"}),
    ("aten", {"s1": "aten", "s2": "aten", "s1_3x5": "aten"}),
    (None, {"s1": "aten", "s2": "aten", "s1_3x5": "aten"}),
])
def test_route_table(monkeypatch, route, want):
    """Which function conv2d_bf16_backward takes dX from, with the feature functions replaced by
    recorders (nothing runs on a device)."""
    if route is None:
        monkeypatch.delenv("MCGMIL_CONV_GRAD", raising=False)
    else:
        monkeypatch.setenv("MCGMIL_CONV_GRAD", route)
    calls = []
    monkeypatch.setattr(features, "conv_bf16_untrainable_reason", lambda conv, x: None)
    monkeypatch.setattr(features, "conv2d_bf16_wgrad", lambda conv, x, dy: calls.append("wgrad") or torch.zeros(1))
    monkeypatch.setattr(features, "conv2d_bf16_dgrad", lambda conv, dy, x: calls.append("dgrad") or "dgrad")
    monkeypatch.setattr(features, "conv2d_bf16_dgrad_direct",
                        lambda conv, dy, x_shape: calls.append("direct") or "direct")
    monkeypatch.setattr(features, "_aten_conv_backward_bf16",
                        lambda conv, x, dy, need_dx, need_dw: calls.append("aten") or ("aten", None))
    convs = {"s1": features._ConvShim(torch.zeros(64, 64, 3, 3), 1, 1),
             "s2": features._ConvShim(torch.zeros(64, 64, 3, 3), 2, 1),
             "s1_3x5": features._ConvShim(torch.zeros(64, 64, 3, 5), 1, 1)}
    x = torch.zeros(1, 64, 8, 8, dtype=torch.bfloat16)
    for key, conv in convs.items():
        del calls[:]
        dx, dw = features.conv2d_bf16_backward(conv, x, torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16))
        assert dx == want[key], (route, key, calls)
        assert calls == (["aten"] if want[key] == "aten" else ["wgrad", want[key]]), (route, key, calls)
        if route != "direct":
            assert "direct" not in calls
        del calls[:]
        dx, dw = features.conv2d_bf16_backward(conv, x, torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16), need_dx=False)
        assert dx is None or want[key] == "aten"
        assert "direct" not in calls and "dgrad" not in calls
