"""Host-side checks of the fused bf16 BatchNorm/add/ReLU training op (no kernel launches): the
binding of include/mcgmil_bn_grad_bf16.h, its workspace arithmetic and the status codes that need no
device, the fake kernels of the two ops, the predicate and the context manager that route
`features.bn_act`, the opt-in on the module, and the build lists."""
import ctypes
import inspect

import pytest
import torch
import torch.nn as nn

from mcgmil import MultiHeadGatedAttentionMIL, _build, _lib, features, library  # noqa: F401
from mcgmil.resnet import deactivate_batchnorm

CL = torch.channels_last
BF = torch.bfloat16
INVALID, UNSUPPORTED, ALIGN, WORKSPACE = -1, -2, -3, -4           # enum mcgmil_status (include/mcgmil.h)


def test_symbols_and_struct_are_bound(hip_lib):
    assert _lib.BN_GRAD_BF16_EXPORTED == ("mcgmil_bn_grad_bf16_args_size", "mcgmil_bn_grad_workspace_size_bf16",
                                          "mcgmil_batchnorm_act_backward_bf16")
    assert _lib.ABI_VERSION == 6 and hip_lib.mcgmil_abi_version() == 6       # entry points only: no ABI bump
    pbb = ctypes.POINTER(_lib.BnGradBf16Args)
    assert hip_lib.mcgmil_bn_grad_bf16_args_size() == ctypes.sizeof(_lib.BnGradBf16Args)
    assert ctypes.sizeof(_lib.BnGradBf16Args) == ctypes.sizeof(_lib.BnGradArgs) == 120
    assert [f[0] for f in _lib.BnGradBf16Args._fields_] == [f[0] for f in _lib.BnGradArgs._fields_]
    assert hip_lib.mcgmil_bn_grad_workspace_size_bf16.argtypes == [pbb, ctypes.POINTER(ctypes.c_size_t)]
    assert hip_lib.mcgmil_batchnorm_act_backward_bf16.argtypes == [pbb, ctypes.c_void_p]
    # the fp32 entry points are still there, unchanged
    assert hip_lib.mcgmil_bn_grad_args_size() == ctypes.sizeof(_lib.BnGradArgs)


def test_sources_and_headers_are_in_the_build():
    assert "mcgmil_bn_grad_bf16.hip" in _build.SOURCES and "mcgmil_bn_grad_bf16.hip" in _build.DEPS
    assert "mcgmil_bn_grad_kernels.h" in _build.DEPS and "mcgmil_bn_grad_kernels.h" not in _build.SOURCES
    assert "mcgmil_bn_grad.hip" in _build.SOURCES
    src = inspect.getsource(_build._stale)
    assert "mcgmil_bn_grad_bf16.h" in src and "mcgmil_bn_grad.h" in src


def _size(L, rows, C, reserved=0, fp32=False):
    a = (_lib.BnGradArgs if fp32 else _lib.BnGradBf16Args)()
    a.rows, a.channels, a.reserved = rows, C, reserved
    n = ctypes.c_size_t(12345)
    f = L.mcgmil_bn_grad_workspace_size if fp32 else L.mcgmil_bn_grad_workspace_size_bf16
    return f(ctypes.byref(a), ctypes.byref(n)), n.value


def test_workspace_arithmetic(hip_lib):
    """(4 C + 2 C parts) fp32 words with parts = ceil(rows / (PART_ELEMS / C)), rounded up to 256
    bytes: the fp32 entry point's formula (the partials and the coefficients are fp32 here too)."""
    PART = _lib.BN_GRAD_PART_ELEMS
    for rows in (2, 3, 189, 512, 513, 5125, 1507 * 56 * 56, 4224 * 64 * 64, 1 << 33):
        for C in (8, 24, 64, 512, 1000, 2048):
            rc, n = _size(hip_lib, rows, C)
            parts = -(-rows // (PART // C))
            assert rc == 0 and n == ((4 * C + 2 * C * parts) * 4 + 255) // 256 * 256, (rows, C)
            assert (rc, n) == _size(hip_lib, rows, C, fp32=True), (rows, C)
    assert _size(hip_lib, 512, 64)[1] == (4 * 64 + 2 * 64 * 1) * 4
    assert _size(hip_lib, 513, 64)[1] == (4 * 64 + 2 * 64 * 2) * 4


def test_status_codes_without_a_launch(hip_lib):
    L = hip_lib
    for rows, C, reserved, want in ((1, 64, 0, INVALID), (0, 64, 0, INVALID), (189, 12, 0, UNSUPPORTED),
                                    (189, 0, 0, UNSUPPORTED), (189, 4096, 0, UNSUPPORTED), (189, 64, 1, INVALID),
                                    (1 << 43, 8, 0, UNSUPPORTED), (2 ** 63 - 1, 2048, 0, UNSUPPORTED)):
        rc, n = _size(L, rows, C, reserved)
        assert rc == want and n == 12345, (rows, C, reserved)      # bytes untouched on error
        assert len(L.mcgmil_last_error()) > 0
    assert L.mcgmil_bn_grad_workspace_size_bf16(None, ctypes.byref(ctypes.c_size_t())) == INVALID
    assert L.mcgmil_batchnorm_act_backward_bf16(None, None) == INVALID

    def args(**kw):                                     # pointers that are never dereferenced on the host
        a = _lib.BnGradBf16Args()
        a.rows, a.channels, a.relu = 189, 64, 1
        a.x, a.y, a.dy, a.gamma, a.mean, a.invstd = 0x10000, 0x20000, 0x30000, 0x40000, 0x41000, 0x42000
        a.dx, a.dresidual, a.dgamma, a.dbeta = 0x50000, 0x60000, 0x70000, 0x71000
        a.workspace, a.workspace_bytes = 0x100000, 1 << 20
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    run = lambda a: L.mcgmil_batchnorm_act_backward_bf16(ctypes.byref(a), None)  # noqa: E731
    # every check comes before any launch, in the fp32 entry point's order
    for bad, want in ((dict(relu=2), INVALID), (dict(x=None), INVALID), (dict(dy=None), INVALID),
                      (dict(mean=None), INVALID), (dict(invstd=None), INVALID), (dict(y=None), INVALID),
                      (dict(dx=None, dresidual=None, dgamma=None, dbeta=None), INVALID),
                      (dict(relu=0, y=None), INVALID),               # dresidual needs relu
                      (dict(x=0x10002), ALIGN), (dict(y=0x20008), ALIGN), (dict(dy=0x3000c), ALIGN),
                      (dict(dx=0x50004), ALIGN), (dict(dresidual=0x60008), ALIGN), (dict(mean=0x41004), ALIGN),
                      (dict(invstd=0x42008), ALIGN), (dict(gamma=0x40002), ALIGN), (dict(dgamma=0x70001), ALIGN),
                      (dict(dbeta=0x71003), ALIGN), (dict(workspace=None), WORKSPACE),
                      (dict(workspace_bytes=_size(L, 189, 64)[1] - 1), WORKSPACE), (dict(workspace=0x100010), ALIGN),
                      (dict(channels=2056), UNSUPPORTED), (dict(rows=1), INVALID), (dict(reserved=-1), INVALID),
                      (dict(x=0x10002, workspace=None), ALIGN)):     # alignment is checked before the workspace
        assert run(args(**bad)) == want, bad
        assert len(L.mcgmil_last_error()) > 0


@pytest.mark.parametrize("relu,res,affine", [(True, True, True), (True, False, True), (False, True, False)])
def test_fake_kernels_shapes_dtypes_and_empty_gradients(relu, res, affine):
    x = torch.empty(3, 64, 9, 7, device="meta", dtype=BF).contiguous(memory_format=CL)
    w = torch.empty(64, device="meta") if affine else None
    y, mean, invstd = torch.ops.mcgmil.bn_act_bf16(x, w, w, x if res else None, 1e-5, relu)
    assert y.shape == x.shape and y.dtype == BF and y.device.type == "meta"
    assert y.is_contiguous(memory_format=CL) and y.stride(1) == 1
    for t in (mean, invstd):
        assert t.shape == (64,) and t.dtype == torch.float32 and t.device.type == "meta"
    dx, dres, dw, db = torch.ops.mcgmil.bn_act_bf16_backward(x, y, y, w, mean, invstd, relu, True, True, True)
    assert dx.shape == x.shape and dx.dtype == BF and dx.is_contiguous(memory_format=CL) and dx.stride(1) == 1
    assert dw.shape == db.shape == (64,) and dw.dtype == db.dtype == torch.float32      # for the fp32 master's .grad
    if relu:
        assert dres.shape == x.shape and dres.dtype == BF and dres.is_contiguous(memory_format=CL)
    else:
        assert dres.numel() == 0               # without ReLU the residual gradient is dy itself
    for flags in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        out = torch.ops.mcgmil.bn_act_bf16_backward(x, y, y, w, mean, invstd, relu, *flags)
        need = (flags[0], flags[1] and relu, flags[2], flags[2])
        assert [t.numel() > 0 for t in out] == list(need), flags


def test_ops_have_no_cpu_kernel():
    x = torch.zeros(2, 8, 2, 2, dtype=BF).contiguous(memory_format=CL)
    v = torch.ones(8)
    with pytest.raises((RuntimeError, ValueError)):
        torch.ops.mcgmil.bn_act_bf16(x, v, v, None, 1e-5, True)
    with pytest.raises((RuntimeError, ValueError)):
        torch.ops.mcgmil.bn_act_bf16_backward(x, x, x, v, v, v, True, True, False, True)
    with pytest.raises(ValueError):
        features.batchnorm_act_stats_bf16(x, v, v, None, 1e-5, True)
    with pytest.raises(ValueError):
        features.batchnorm_act_backward_bf16(x, x, x, v, v, v, True)


def _bn(C=64):
    bn = nn.BatchNorm2d(C)
    deactivate_batchnorm(bn)
    return bn


def test_bn_bf16_trainable_clauses(monkeypatch):
    """Every clause, on CPU tensors: the device is checked last."""
    x = torch.zeros(2, 64, 4, 4, dtype=BF)
    why, ok = features.bn_bf16_untrainable_reason, features.bn_bf16_trainable
    assert not ok(x, _bn()) and why(x, _bn()).startswith("device")                       # a CPU tensor
    assert not ok(x.float(), _bn()) and why(x.float(), _bn()).startswith("dtype")        # fp32: the other op's
    assert why(x.half(), _bn()).startswith("dtype")
    assert why(x, _bn().to(BF)).startswith("dtype")                                      # parameters stay fp32
    noaffine = nn.BatchNorm2d(64, affine=False, track_running_stats=False)
    assert why(x, noaffine).startswith("device")                                         # ... or are absent
    x12 = torch.zeros(2, 12, 4, 4, dtype=BF)
    assert not ok(x12, _bn(12)) and why(x12, _bn(12)).startswith("channels")
    assert why(x, _bn(128)).startswith("channels")
    assert why(torch.zeros(2, 2056, 1, 1, dtype=BF), _bn(2056)).startswith("channels")
    assert why(torch.zeros(1, 64, 1, 1, dtype=BF), _bn()).startswith("rows")
    tracking = nn.BatchNorm2d(64)                       # train mode, tracks running statistics
    assert not ok(x, tracking) and "pending" in why(x, tracking)
    assert "running-statistics mode" in why(x, tracking.eval())
    assert why(x, _bn(), torch.zeros(2, 64, 4, 5, dtype=BF)).startswith("residual")
    assert why(x, _bn(), x.float()).startswith("residual")
    assert why(x, _bn(), x).startswith("device")
    assert why(x, nn.Identity()).startswith("layer") and why(x[0], _bn()).startswith("layer")
    # eval mode without running statistics (deactivate_batchnorm) still normalises with the batch's
    assert why(x, _bn().eval()).startswith("device")
    # no autocast clause: the predicate never asks whether autocast is on
    def asked(*a, **k):
        raise AssertionError("bn_bf16_untrainable_reason consulted autocast")
    monkeypatch.setattr(torch, "is_autocast_enabled", asked)
    assert why(x, _bn()).startswith("device") and why(x.float(), _bn()).startswith("dtype")
    monkeypatch.undo()
    # the fp32 predicate keeps refusing bf16
    assert features.bn_untrainable_reason(x, _bn()).startswith("dtype")


def test_bn_act_keeps_the_torch_layers_on_the_cpu_inside_the_context():
    bn = _bn(8)
    x = torch.randn(2, 8, 3, 3, requires_grad=True)
    want = torch.relu(bn(x) + x)
    with features.native_norm_bf16_training():
        got = features.bn_act(bn, x, True, x)
        xb = x.detach().to(BF).requires_grad_()
        gotb = features.bn_act(bn, xb, True, xb)       # bf16 on the CPU: the device clause declines
    assert torch.equal(got, want) and gotb.dtype == BF


def test_native_norm_bf16_training_context_nests_and_restores():
    assert features._native_norm_bf16_training is False
    with features.native_norm_bf16_training():
        assert features._native_norm_bf16_training is True
        with features.native_norm_bf16_training(False):
            assert features._native_norm_bf16_training is False
        assert features._native_norm_bf16_training is True
        assert features._native_norm_training is False and features._native_bf16_training is False
    assert features._native_norm_bf16_training is False


def test_enable_bf16_norm_training():
    for name in ("enable_bf16_backbone_training", "enable_bf16_norm_training"):
        sig = inspect.signature(getattr(MultiHeadGatedAttentionMIL, name))
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("flag", True)], name
    m = MultiHeadGatedAttentionMIL(pretrained=False)
    assert m._bf16_norm_training is False                              # off by default
    assert m.enable_bf16_backbone_training() is m
    assert m._bf16_backbone_training is True and m._bf16_norm_training is False      # alone: as before
    assert m.enable_bf16_norm_training() is m
    assert m._bf16_backbone_training is True and m._bf16_norm_training is True
    assert (m._head_training, m._backbone_training, m._norm_training, m._stem_training, m._stem_conv_training) == \
        (False,) * 5                                                   # the other opt-ins are untouched
    m.enable_backbone_training(norm=True)
    assert m._bf16_norm_training is True                               # ... and do not touch this one
    assert m.enable_bf16_norm_training(False) is m and m._bf16_norm_training is False
    assert m._bf16_backbone_training is True                           # ... nor does it touch the flag it sits on
    m.enable_bf16_norm_training()
    assert m.enable_bf16_backbone_training(False) is m                 # norm follows the flag
    assert m._bf16_backbone_training is False and m._bf16_norm_training is False
    assert m.enable_bf16_backbone_training() is m and m._bf16_norm_training is False
    m.enable_bf16_norm_training()
    m.enable_backbone_training(False)
    m.train()
    with pytest.raises(NotImplementedError, match="enable_head_training"):       # alone it is not enough
        m(torch.zeros(1, 2, 3, 32, 32))
