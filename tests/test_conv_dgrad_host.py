"""Host-side checks of the direct convolution data gradient (include/mcgmil_conv_dgrad.h; no
kernel launches): the residue-class decomposition the kernel rests on against float64 autograd,
the launch arithmetic of mcgmil_conv_dgrad_classes against the restatement, the route switch and
the binding."""
import ctypes

import pytest
import torch

import conv_dgrad_ref as ref
from mcgmil import _lib, features

INVALID, UNSUPPORTED = -1, -2                # enum mcgmil_status (include/mcgmil.h)


def dgrad_args(N, Cin, Cout, kh, kw, s, p, H, W):
    g = _lib.ConvDgradArgs()
    a = g.fwd
    a.batch, a.in_channels, a.out_channels, a.height, a.width = N, Cin, Cout, H, W
    a.kernel_h, a.kernel_w, a.stride, a.pad = kh, kw, s, p
    return g


def classes_of(L, g):
    taps, pixels, tiles = (ctypes.c_int32 * 4)(), (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
    rc = L.mcgmil_conv_dgrad_classes(ctypes.byref(g), taps, pixels, tiles)
    return rc, list(taps), list(pixels), list(tiles)


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
    "s2_7x7_c16": [(16, 20), (12, 25), (12, 24), (9, 30)],
}


@pytest.mark.parametrize("name", ref.TABLE)
def test_classes_agree_with_the_restatement(hip_lib, name):
    N, Cin, Cout, k, s, p, H, W = ref.CASES[name]
    c = ref.case(name)
    _, want = ref.dgrad_classes(c.dy.double(), c.w.double(), s, p, c.x.shape)
    rc, taps, pixels, tiles = classes_of(hip_lib, dgrad_args(N, Cin, Cout, k, k, s, p, H, W))
    assert rc == 0
    got = list(zip(taps, pixels))
    assert got[:s * s] == want and got[s * s:] == [(0, 0)] * (4 - s * s)
    if name in EXPECTED:
        assert got == EXPECTED[name]
    tile = 256 if Cin <= 64 else 128
    assert tiles == [-(-px // tile) for px in pixels]
    assert sum(pixels) == N * H * W


def test_classes_of_a_non_square_kernel(hip_lib):
    rc, taps, pixels, _ = classes_of(hip_lib, dgrad_args(1, 64, 64, 3, 1, 2, 0, 9, 9))
    assert rc == 0 and taps == [2, 0, 1, 0] and pixels == [25, 20, 20, 16]


def test_classes_sizes_past_32_bits_are_unsupported(hip_lib):
    # 2^31 input pixels in the one class of a stride-1 convolution
    rc, *_ = classes_of(hip_lib, dgrad_args(1 << 11, 16, 64, 1, 1, 1, 0, 1 << 10, 1 << 10))
    assert rc == UNSUPPORTED and len(hip_lib.mcgmil_last_error()) > 0
    # 2^31 pixels in each of the four classes of a stride-2 one
    rc, *_ = classes_of(hip_lib, dgrad_args(1 << 13, 16, 64, 3, 3, 2, 1, 1 << 10, 1 << 10))
    assert rc == UNSUPPORTED
    # pixels * channels past 64 bits
    rc, *_ = classes_of(hip_lib, dgrad_args(0x7fffffff, 0x7ffffff0, 64, 1, 1, 1, 0, 0x7fffffff, 0x7fffffff))
    assert rc == UNSUPPORTED
    # just below the limit: four classes of 2^29 pixels
    rc, taps, pixels, tiles = classes_of(hip_lib, dgrad_args(1 << 11, 16, 64, 3, 3, 2, 1, 1 << 10, 1 << 10))
    assert rc == 0 and pixels == [1 << 29] * 4 and tiles == [1 << 21] * 4 and taps == [4, 2, 2, 1]


def test_classes_validation(hip_lib):
    ok = (2, 64, 128, 3, 3, 2, 1, 10, 10)
    assert classes_of(hip_lib, dgrad_args(*ok))[0] == 0
    for i, v in ((5, 3), (1, 24), (2, 32), (3, 8), (6, 3)):       # stride, Cin, Cout, kernel, pad >= kernel
        bad = list(ok)
        bad[i] = v
        assert classes_of(hip_lib, dgrad_args(*bad))[0] == UNSUPPORTED, bad
    g = dgrad_args(*ok)
    g.reserved = 1
    assert classes_of(hip_lib, g)[0] == INVALID
    assert hip_lib.mcgmil_conv_dgrad_classes(None, None, None, None) == INVALID
    assert hip_lib.mcgmil_conv_dgrad_classes(ctypes.byref(dgrad_args(*ok)), None, None, None) == INVALID
    # without a launch: NULL pointers are refused before anything runs
    assert hip_lib.mcgmil_conv2d_dgrad_f32(ctypes.byref(dgrad_args(*ok)), None) == INVALID


def test_struct_size_matches_the_binding(hip_lib):
    assert hip_lib.mcgmil_conv_dgrad_args_size() == ctypes.sizeof(_lib.ConvDgradArgs)
    assert _lib.CONV_DGRAD_EXPORTED == ("mcgmil_conv_dgrad_args_size", "mcgmil_conv_dgrad_classes",
                                        "mcgmil_conv2d_dgrad_f32")
    for f in _lib.CONV_DGRAD_EXPORTED:
        assert hasattr(hip_lib, f), f


@pytest.mark.parametrize("value,route,native", [(None, "aten", False), ("aten", "aten", False),
                                                ("native", "native", True), ("direct", "direct", True),
                                                ("Direct", "aten", False), ("", "aten", False),
                                                ("miopen", "aten", False)])
def test_route_switch(monkeypatch, value, route, native):
    if value is None:
        monkeypatch.delenv("MCGMIL_CONV_GRAD", raising=False)
    else:
        monkeypatch.setenv("MCGMIL_CONV_GRAD", value)
    assert features.conv_grad_route() == route
    assert features.conv_grad_native() is native


def test_dgrad_native_is_unchanged(monkeypatch):
    monkeypatch.setenv("MCGMIL_CONV_GRAD", "direct")
    w = torch.zeros(64, 64, 3, 3)
    assert features.dgrad_native(features._ConvShim(w, 1, 1))
    assert not features.dgrad_native(features._ConvShim(w, 2, 1))
    assert not features.dgrad_native(features._ConvShim(torch.zeros(64, 64, 3, 1), 1, 0))


def test_dgrad_direct_refuses_a_cpu_tensor():
    conv = features._ConvShim(torch.zeros(64, 64, 3, 3), 2, 1)
    dy = torch.zeros(1, 64, 4, 4)
    assert not features.dgrad_direct_supported(conv, dy)
    with pytest.raises(ValueError):
        features.conv2d_f32_dgrad_direct(conv, dy, (1, 64, 8, 8))
