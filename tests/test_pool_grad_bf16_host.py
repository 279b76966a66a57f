"""Host-side checks of the bf16 stem BatchNorm / ReLU / max-pool training op (no kernel launches):
the binding of include/mcgmil_pool_grad_bf16.h, its workspace arithmetic and the status codes that
need no device, the fake kernels of the two ops, the predicate and the context manager that route
`features.bn_act`, the opt-in on the module, the build lists, and the references the GPU tests use
(tests/pool_grad_bf16_ref.py)."""
import ctypes
import inspect

import pytest
import torch
import torch.nn as nn

import pool_grad_bf16_ref as PB
from mcgmil import MultiHeadGatedAttentionMIL, _build, _lib, features, library  # noqa: F401
from mcgmil.resnet import deactivate_batchnorm

P, R = PB.P, PB.R
CL = torch.channels_last
BF = torch.bfloat16
INVALID, UNSUPPORTED, ALIGN, WORKSPACE = -1, -2, -3, -4           # enum mcgmil_status (include/mcgmil.h)


def test_symbols_and_struct_are_bound(hip_lib):
    assert _lib.POOL_GRAD_BF16_EXPORTED == ("mcgmil_batchnorm_pool_train_bf16", "mcgmil_bn_pool_grad_bf16_args_size",
                                            "mcgmil_bn_pool_grad_workspace_size_bf16",
                                            "mcgmil_batchnorm_pool_backward_bf16")
    for name in _lib.POOL_GRAD_BF16_EXPORTED:
        assert getattr(hip_lib, name) is not None
    assert _lib.ABI_VERSION == 6 and hip_lib.mcgmil_abi_version() == 6       # entry points only: no ABI bump
    ppb = ctypes.POINTER(_lib.BnPoolGradBf16Args)
    assert hip_lib.mcgmil_bn_pool_grad_bf16_args_size() == ctypes.sizeof(_lib.BnPoolGradBf16Args)
    assert ctypes.sizeof(_lib.BnPoolGradBf16Args) == ctypes.sizeof(_lib.BnPoolGradArgs) == 136
    assert [f[0] for f in _lib.BnPoolGradBf16Args._fields_] == [f[0] for f in _lib.BnPoolGradArgs._fields_]
    assert hip_lib.mcgmil_bn_pool_grad_workspace_size_bf16.argtypes == [ppb, ctypes.POINTER(ctypes.c_size_t)]
    assert hip_lib.mcgmil_batchnorm_pool_backward_bf16.argtypes == [ppb, ctypes.c_void_p]
    assert hip_lib.mcgmil_batchnorm_pool_train_bf16.argtypes == [ctypes.POINTER(_lib.BnArgs), ctypes.c_void_p,
                                                                 ctypes.c_void_p]
    # the fp32 entry points are still there, unchanged
    assert hip_lib.mcgmil_bn_pool_grad_args_size() == ctypes.sizeof(_lib.BnPoolGradArgs)
    assert hip_lib.mcgmil_batchnorm_pool_train.argtypes == hip_lib.mcgmil_batchnorm_pool_train_bf16.argtypes


def test_sources_and_headers_are_in_the_build():
    assert "mcgmil_pool_grad_bf16.hip" in _build.SOURCES and "mcgmil_pool_grad_bf16.hip" in _build.DEPS
    assert "mcgmil_pool_grad_kernels.h" in _build.DEPS and "mcgmil_pool_grad_kernels.h" not in _build.SOURCES
    assert "mcgmil_pool_grad.hip" in _build.SOURCES and "mcgmil_pool_grad.hip" in _build.DEPS
    src = inspect.getsource(_build._stale)
    assert "mcgmil_pool_grad_bf16.h" in src and "mcgmil_pool_grad.h" in src


def _args(shape, pool, fp32=False, **kw):
    a = (_lib.BnPoolGradArgs if fp32 else _lib.BnPoolGradBf16Args)()
    a.batch, a.channels, a.height, a.width = shape
    a.pool_kernel, a.pool_stride, a.pool_pad = pool
    a.pooled_height, a.pooled_width = (P.pooled(s, *pool) for s in shape[2:])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _size(L, shape, pool=(3, 2, 1), fp32=False, **kw):
    a = _args(shape, pool, fp32, **kw)
    n = ctypes.c_size_t(12345)
    f = L.mcgmil_bn_pool_grad_workspace_size if fp32 else L.mcgmil_bn_pool_grad_workspace_size_bf16
    return f(ctypes.byref(a), ctypes.byref(n)), n.value


def test_workspace_arithmetic(hip_lib):
    """(4 C + 2 C parts) fp32 words with parts = ceil(N H W / (PART_ELEMS / C)), rounded up to 256
    bytes: the fp32 entry point's formula (the partials and the coefficients are fp32 here too)."""
    PART = _lib.BN_POOL_GRAD_PART_ELEMS
    assert PART == PB.PART_ELEMS
    for N, H, W in ((1, 2, 1), (3, 9, 7), (1, 23, 23), (2, 16, 16), (64, 112, 112), (1507, 112, 112),
                    (1338, 112, 112), (33, 512, 512), (4096, 1024, 1024)):
        for C in (8, 24, 64, 512, 1000, 2048):
            rc, n = _size(hip_lib, (N, C, H, W))
            parts = -(-(N * H * W) // (PART // C))
            assert rc == 0 and n == ((4 * C + 2 * C * parts) * 4 + 255) // 256 * 256, (N, H, W, C)
            assert (rc, n) == _size(hip_lib, (N, C, H, W), fp32=True), (N, H, W, C)
    assert _size(hip_lib, (1, 64, 256, 2), (2, 2, 0))[1] == (4 * 64 + 2 * 64 * 1) * 4
    assert _size(hip_lib, (1, 64, 513, 2), (2, 2, 0))[1] == (4 * 64 + 2 * 64 * 3) * 4
    assert 4096 * 1024 * 1024 * 64 > 2 ** 32                                  # batch * H * W * C past 2^32


def test_status_codes_without_a_launch(hip_lib):
    L = hip_lib
    shape = (3, 64, 9, 7)
    for kw, pool, want in ((dict(batch=1, height=1, width=1, pooled_height=1, pooled_width=1), (3, 2, 1), INVALID),
                           (dict(batch=0), (3, 2, 1), INVALID), (dict(channels=12), (3, 2, 1), UNSUPPORTED),
                           (dict(channels=0), (3, 2, 1), UNSUPPORTED), (dict(channels=4096), (3, 2, 1), UNSUPPORTED),
                           (dict(reserved=1), (3, 2, 1), INVALID), (dict(reserved32=1), (3, 2, 1), INVALID),
                           (dict(), (4, 2, 1), UNSUPPORTED), (dict(), (3, 2, 2), UNSUPPORTED),
                           (dict(), (2, 3, 0), UNSUPPORTED), (dict(pooled_height=4), (3, 2, 1), INVALID),
                           (dict(batch=1 << 13, height=1 << 15, width=1 << 15, channels=8), (3, 2, 1), UNSUPPORTED),
                           (dict(height=46341, width=46341), (3, 2, 1), UNSUPPORTED)):
        rc, n = _size(L, shape, pool, **kw)
        assert rc == want and n == 12345, (kw, pool)             # bytes untouched on error
        assert rc == _size(L, shape, pool, fp32=True, **kw)[0], (kw, pool)      # the fp32 entry point's codes
        assert len(L.mcgmil_last_error()) > 0
    assert L.mcgmil_bn_pool_grad_workspace_size_bf16(None, ctypes.byref(ctypes.c_size_t())) == INVALID
    assert L.mcgmil_batchnorm_pool_backward_bf16(None, None) == INVALID
    assert L.mcgmil_batchnorm_pool_train_bf16(None, None, None) == INVALID

    def args(**kw):                                     # pointers that are never dereferenced on the host
        a = _args(shape, (3, 2, 1))
        a.z, a.argmax, a.dy, a.gamma, a.mean, a.invstd = 0x100000, 0x200000, 0x300000, 0x400000, 0x410000, 0x420000
        a.dz, a.dgamma, a.dbeta = 0x500000, 0x700000, 0x710000
        a.workspace, a.workspace_bytes = 0x1000000, 1 << 20
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    run = lambda a: L.mcgmil_batchnorm_pool_backward_bf16(ctypes.byref(a), None)  # noqa: E731
    zb = 3 * 9 * 7 * 64 * 2                             # bytes of z and dz: 2-byte elements
    # every check comes before any launch, in the fp32 entry point's order
    for bad, want in ((dict(z=None), INVALID), (dict(argmax=None), INVALID), (dict(dy=None), INVALID),
                      (dict(mean=None), INVALID), (dict(invstd=None), INVALID),
                      (dict(dz=None, dgamma=None, dbeta=None), INVALID),
                      (dict(z=0x100002), ALIGN), (dict(dy=0x300008), ALIGN), (dict(dz=0x500004), ALIGN),
                      (dict(mean=0x410004), ALIGN), (dict(invstd=0x420008), ALIGN), (dict(argmax=0x200004), ALIGN),
                      (dict(gamma=0x400002), ALIGN), (dict(dgamma=0x700001), ALIGN), (dict(dbeta=0x710003), ALIGN),
                      (dict(dz=0x100000), INVALID), (dict(dz=0x100000 + zb - 16), INVALID),
                      (dict(dgamma=0x410000), INVALID), (dict(dbeta=0x700000), INVALID),
                      (dict(dz=0x100000 + zb, workspace=None), WORKSPACE),     # right behind z: 2-byte elements
                      (dict(workspace=None), WORKSPACE),
                      (dict(workspace_bytes=_size(L, shape)[1] - 1), WORKSPACE), (dict(workspace=0x1000010), ALIGN),
                      (dict(channels=2056), UNSUPPORTED), (dict(reserved=-1), INVALID),
                      (dict(z=0x100002, workspace=None), ALIGN)):    # alignment is checked before the workspace
        assert run(args(**bad)) == want, bad
        assert len(L.mcgmil_last_error()) > 0

    def fwd(argmax=0x200000, **kw):
        a = _lib.BnArgs()
        a.rows, a.channels, a.dtype = 189, 64, _lib.MCGMIL_BF16
        a.batch, a.height, a.width = 3, 9, 7
        a.pool_kernel, a.pool_stride, a.pool_pad = 3, 2, 1
        a.x, a.y, a.gamma, a.beta, a.batch_mean, a.batch_invstd = 0x100000, 0x300000, 0x400000, 0x401000, 0x410000, 0x420000
        a.eps, a.relu = 1e-5, 1
        a.workspace, a.workspace_bytes = 0x1000000, 0         # too small on purpose: a complete call would launch
        for k, v in kw.items():
            setattr(a, k, v)
        return a, argmax
    train = lambda a, c: L.mcgmil_batchnorm_pool_train_bf16(ctypes.byref(a), c, None)  # noqa: E731
    for bad, want in ((dict(dtype=_lib.MCGMIL_F32), UNSUPPORTED), (dict(channels=12), UNSUPPORTED),
                      (dict(pool_kernel=4), UNSUPPORTED), (dict(pool_kernel=0), UNSUPPORTED), (dict(pool_pad=2), UNSUPPORTED),
                      (dict(rows=190), INVALID), (dict(running_mean=0x430000, running_var=0x431000), INVALID),
                      (dict(residual=0x600000), UNSUPPORTED), (dict(relu=2), INVALID), (dict(x=None), INVALID),
                      (dict(batch_mean=None), INVALID), (dict(argmax=None), INVALID), (dict(x=0x100002), ALIGN),
                      (dict(argmax=0x200004), ALIGN), (dict(y=0x100000 + zb - 16), INVALID),
                      (dict(y=0x100000 + zb), WORKSPACE), (dict(workspace=None), WORKSPACE), (dict(), WORKSPACE)):
        assert train(*fwd(**bad)) == want, bad
        assert len(L.mcgmil_last_error()) > 0
    # mcgmil_batchnorm_pool_train keeps refusing bf16
    a, c = fwd()
    assert L.mcgmil_batchnorm_pool_train(ctypes.byref(a), c, None) == UNSUPPORTED


@pytest.mark.parametrize("relu,affine,pool", [(True, True, (3, 2, 1)), (False, True, (2, 2, 0)), (True, False, (3, 1, 1)),
                                              (False, False, (2, 1, 1))])
def test_fake_kernels_shapes_dtypes_and_empty_gradients(relu, affine, pool):
    z = torch.empty(3, 64, 9, 7, device="meta", dtype=BF).contiguous(memory_format=CL)
    w = torch.empty(64, device="meta") if affine else None
    y, mean, invstd, code = torch.ops.mcgmil.bn_pool_bf16(z, w, w, 1e-5, relu, *pool)
    shape = (3, 64, P.pooled(9, *pool), P.pooled(7, *pool))
    assert tuple(y.shape) == tuple(code.shape) == shape and y.dtype == BF and code.dtype == torch.uint8
    assert y.device.type == code.device.type == "meta"
    assert y.is_contiguous(memory_format=CL) and y.stride(1) == 1 and code.is_contiguous(memory_format=CL)
    for t in (mean, invstd):
        assert t.shape == (64,) and t.dtype == torch.float32 and t.device.type == "meta"
    dz, dw, db = torch.ops.mcgmil.bn_pool_bf16_backward(z, code, y, w, mean, invstd, *pool, True, True)
    assert dz.shape == z.shape and dz.dtype == BF and dz.is_contiguous(memory_format=CL) and dz.stride(1) == 1
    assert dw.shape == db.shape == (64,) and dw.dtype == db.dtype == torch.float32      # for the fp32 master's .grad
    for flags in ((False, False), (True, False), (False, True)):
        out = torch.ops.mcgmil.bn_pool_bf16_backward(z, code, y, w, mean, invstd, *pool, *flags)
        assert [t.numel() > 0 for t in out] == [flags[0], flags[1], flags[1]], flags
        assert out[0].dtype == BF and out[1].dtype == out[2].dtype == torch.float32


def test_ops_have_no_cpu_kernel():
    z = torch.zeros(2, 8, 4, 4, dtype=BF).contiguous(memory_format=CL)
    y = torch.zeros(2, 8, 2, 2, dtype=BF).contiguous(memory_format=CL)
    code = torch.zeros(2, 8, 2, 2, dtype=torch.uint8).contiguous(memory_format=CL)
    v = torch.ones(8)
    with pytest.raises((RuntimeError, ValueError)):
        torch.ops.mcgmil.bn_pool_bf16(z, v, v, 1e-5, True, 3, 2, 1)
    with pytest.raises((RuntimeError, ValueError)):
        torch.ops.mcgmil.bn_pool_bf16_backward(z, code, y, v, v, v, 3, 2, 1, True, True)
    with pytest.raises(ValueError):
        features.batchnorm_pool_stats_bf16(z, v, v, 1e-5, True, 3, 2, 1)
    with pytest.raises(ValueError):
        features.batchnorm_pool_backward_bf16(z, code, y, v, v, v, 3, 2, 1)


def _bn(C=64):
    bn = nn.BatchNorm2d(C)
    deactivate_batchnorm(bn)
    return bn


def test_bn_pool_bf16_trainable_clauses(monkeypatch):
    """Every clause, on CPU tensors: the pool's first, the device last."""
    x = torch.zeros(2, 64, 8, 8, dtype=BF)
    pool = nn.MaxPool2d(3, 2, 1)
    why, ok = features.bn_pool_bf16_untrainable_reason, features.bn_pool_bf16_trainable
    assert not ok(x, _bn(), pool) and why(x, _bn(), pool).startswith("device")           # a CPU tensor
    # the pool clause of bn_pool_untrainable_reason, with its words
    for bad in (nn.MaxPool2d(5, 2, 2), nn.MaxPool2d(4, 2, 1), nn.MaxPool2d(3, 2, 1, ceil_mode=True),
                nn.MaxPool2d(3, 2, 1, dilation=2), nn.MaxPool2d((3, 2), 2, 1), nn.MaxPool2d(2, 3, 0),
                nn.AvgPool2d(3, 2, 1), nn.Identity(), None):
        assert not ok(x, _bn(), bad) and why(x, _bn(), bad).startswith("pool"), bad
        assert why(x, _bn(), bad) == features.bn_pool_untrainable_reason(x.float(), _bn(), bad), bad
    assert why(x.float(), _bn(), nn.MaxPool2d(5, 2, 2)).startswith("pool")               # the pool comes first
    for good in (nn.MaxPool2d(2), nn.MaxPool2d(2, 1, 1), nn.MaxPool2d(3, 1, 0), nn.MaxPool2d(3, 3, 1)):
        assert why(x, _bn(), good).startswith("device"), good
    small = torch.zeros(2, 64, 1, 1, dtype=BF)
    assert "larger than the padded input" in why(small, _bn(), nn.MaxPool2d(3, 1, 0))
    # the clauses of bn_bf16_untrainable_reason
    assert not ok(x.float(), _bn(), pool) and why(x.float(), _bn(), pool).startswith("dtype")     # fp32: the other op's
    assert why(x.half(), _bn(), pool).startswith("dtype")
    assert why(x, _bn().to(BF), pool).startswith("dtype")                                # parameters stay fp32
    noaffine = nn.BatchNorm2d(64, affine=False, track_running_stats=False)
    assert why(x, noaffine, pool).startswith("device")                                   # ... or are absent
    x12 = torch.zeros(2, 12, 8, 8, dtype=BF)
    assert not ok(x12, _bn(12), pool) and why(x12, _bn(12), pool).startswith("channels")
    assert why(x, _bn(128), pool).startswith("channels")
    assert why(torch.zeros(2, 2056, 2, 2, dtype=BF), _bn(2056), pool).startswith("channels")
    assert why(torch.zeros(1, 64, 1, 1, dtype=BF), _bn(), pool).startswith("rows")
    tracking = nn.BatchNorm2d(64)                       # train mode, tracks running statistics
    assert not ok(x, tracking, pool) and "pending" in why(x, tracking, pool)
    assert "running-statistics mode" in why(x, tracking.eval(), pool)
    assert why(x, nn.Identity(), pool).startswith("layer") and why(x[0], _bn(), pool).startswith("layer")
    assert why(x, _bn().eval(), pool).startswith("device")
    # no autocast clause: the predicate never asks whether autocast is on
    def asked(*a, **k):
        raise AssertionError("bn_pool_bf16_untrainable_reason consulted autocast")
    monkeypatch.setattr(torch, "is_autocast_enabled", asked)
    assert why(x, _bn(), pool).startswith("device") and why(x.float(), _bn(), pool).startswith("dtype")
    monkeypatch.undo()
    # the fp32 predicate keeps refusing bf16
    assert features.bn_pool_untrainable_reason(x, _bn(), pool).startswith("dtype")


def test_bn_act_keeps_the_torch_layers_on_the_cpu_inside_the_context():
    bn = _bn(8)
    pool = nn.MaxPool2d(3, 2, 1)
    x = torch.randn(2, 8, 6, 6, requires_grad=True)
    want = pool(torch.relu(bn(x)))
    with features.native_stem_bf16_training():
        got = features.bn_act(bn, x, True, pool=pool)
        xb = x.detach().to(BF).requires_grad_()
        gotb = features.bn_act(bn, xb, True, pool=pool)    # bf16 on the CPU: the device clause declines
    assert torch.equal(got, want) and gotb.dtype == BF and gotb.shape == want.shape


def test_native_stem_bf16_training_context_nests_and_restores():
    assert features._native_stem_bf16_training is False
    with features.native_stem_bf16_training():
        assert features._native_stem_bf16_training is True
        with features.native_stem_bf16_training(False):
            assert features._native_stem_bf16_training is False
        assert features._native_stem_bf16_training is True
        assert features._native_stem_training is False and features._native_norm_bf16_training is False
        assert features._native_norm_training is False and features._native_bf16_training is False
    assert features._native_stem_bf16_training is False
    with pytest.raises(KeyError):
        with features.native_stem_bf16_training():
            raise KeyError("restored on the way out")
    assert features._native_stem_bf16_training is False


def test_enable_bf16_stem_training():
    for name in ("enable_bf16_backbone_training", "enable_bf16_norm_training", "enable_bf16_stem_training"):
        sig = inspect.signature(getattr(MultiHeadGatedAttentionMIL, name))
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("flag", True)], name
    m = MultiHeadGatedAttentionMIL(pretrained=False)
    assert m._bf16_stem_training is False                              # off by default
    assert m.enable_bf16_backbone_training() is m
    assert m._bf16_backbone_training is True and m._bf16_stem_training is False      # alone: as before
    assert m.enable_bf16_stem_training() is m
    assert m._bf16_backbone_training is True and m._bf16_stem_training is True
    assert m._bf16_norm_training is False                              # it does not depend on the norm opt-in
    assert (m._head_training, m._backbone_training, m._norm_training, m._stem_training, m._stem_conv_training) == \
        (False,) * 5                                                   # the other opt-ins are untouched
    m.enable_backbone_training(stem=True)
    m.enable_bf16_norm_training(False)
    assert m._bf16_stem_training is True                               # ... and do not touch this one
    assert m.enable_bf16_stem_training(False) is m and m._bf16_stem_training is False
    assert m._bf16_backbone_training is True and m._stem_training is True      # ... nor does it touch the others
    m.enable_bf16_stem_training().enable_bf16_norm_training()
    assert m.enable_bf16_backbone_training(False) is m                 # both follow the flag they sit on
    assert m._bf16_backbone_training is False and m._bf16_stem_training is False and m._bf16_norm_training is False
    assert m.enable_bf16_backbone_training() is m and m._bf16_stem_training is False
    m.enable_bf16_stem_training()
    m.enable_backbone_training(False)
    m.train()
    with pytest.raises(NotImplementedError, match="enable_head_training"):       # alone it is not enough
        m(torch.zeros(1, 2, 3, 32, 32))
    assert "native_stem_bf16_training(self._bf16_stem_training)" in inspect.getsource(MultiHeadGatedAttentionMIL.forward)


# ---------------------------------------------------------------- the references of the GPU tests
@pytest.mark.parametrize("name", list(PB.CASES))
def test_reference_margins_and_codes(name):
    """After the rounding of z to bf16 the float64 reference keeps its distance from a flipped argmax
    or ReLU mask: the smallest NON-ZERO top-two gap of any window and the smallest |window maximum|
    are both >= 1e-5 (measured: 7.3e-4 and 1.0e-4 at the least, both on "blocks"). Exact ties, which
    the rounding creates, go to the first tap in the reference and in the kernel alike, and the fp32
    CPU reference names the float64 reference's taps in every case, so the GPU tests ask for the
    float64 codes exactly."""
    c, r64, r32, bounds, fbounds = PB.reference(name)
    assert torch.equal(c["z"], c["z"].to(BF).float()) and torch.equal(c["dy"], c["dy"].to(BF).float())
    assert c["gamma"].dtype == torch.float32
    gap, top = PB.margins(r64["a"], c["pool"])
    print(f"{name}: smallest non-zero top-two gap {gap:.1e}, smallest |window maximum| {top:.1e}")
    assert gap >= 1e-5 and top >= 1e-5
    assert torch.equal(r32["code"], r64["code"])
    first, tied = PB.first_max_codes(r64["a"], c["pool"], c["relu"])
    assert torch.equal(first, r64["code"])                      # max_pool2d gives an exact tie to the first tap
    if name == "ties":
        assert tied >= first.numel() // 4
    assert all(b >= 1e-6 for b in list(bounds.values()) + list(fbounds.values()))
    # the closed form on the reference's codes is the reference's gradient
    f = P.formula(c["z"].double(), r64["code"], c["dy"].double(), c["gamma"].double(), r64["mean"], r64["invstd"],
                  c["pool"])
    err = R.errors(dict(zip(P.GRADS, f)), r64, P.GRADS)
    assert all(e <= 1e-12 for e in err.values()), err


def test_margins_ignore_exact_ties_only():
    a = torch.tensor([[[[1.0, 1.0, 2.0, 1.5], [0.5, 0.25, 0.0, 0.0]]]], dtype=torch.float64)
    assert PB.margins(a, (2, 2, 0)) == (0.5, 1.0)               # the window that ties 1.0 / 1.0 is skipped
    assert P.margins(a, (2, 2, 0))[0] == 0.0                    # the fp32 tests' margin sees the tie
    assert PB.margins(a[..., :2], (2, 2, 0)) == (float("inf"), 1.0)
    b = torch.tensor([[[[1.0, 1.0 - 1e-7], [0.5, 0.25]]]], dtype=torch.float64)
    assert 0 < PB.margins(b, (2, 2, 0))[0] < 1e-5               # a near-tie is not an exact one
    assert PB.bf16_excess(torch.tensor([1.0]).to(BF), torch.tensor([1.0 + 2.0 ** -7]), 0.0) <= 1.0
    assert PB.bf16_excess(torch.tensor([1.0]).to(BF), torch.tensor([1.02]), 0.0) > 1.0
