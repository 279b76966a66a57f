"""The stem's fused BatchNorm / ReLU / max-pool training op on the HIP kernels
(include/mcgmil_pool_grad.h, features.batchnorm_pool_stats / batchnorm_pool_backward,
torch.ops.mcgmil.bn_pool_f32 and its backward op,
MultiHeadGatedAttentionMIL.enable_backbone_training(stem=True)) against float64 autograd of
max_pool2d(relu?(batch_norm(z))).

Error of tensor k: max|got - ref| / max(max|ref_k|, 1e-3 max_j max|ref_j|) over the case's
gradients j (bn_grad_ref.errors). Bound of tensor k: 10 x the same error of fp32 CPU autograd on
that case, at least 1e-6 (bn_grad_ref.bounds). Every test prints measured / bound before it asserts.

Kernel-level tests call the backward with the window codes, mean and invstd of the float64
reference, so no ReLU mask or argmax can differ from the reference's. Tests of the forward assert
first that the float64 reference is not within 1e-5 of a tie or of zero in any window (the seeds
are chosen on the CPU for that) and then excuse no element. Outputs passed through the C ABI are
pre-filled with NaN, and every device call is made twice and compared bitwise."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pool_grad_ref as P
from mcgmil import MultiHeadGatedAttentionMIL, _lib, features, library  # noqa: F401
from mcgmil.resnet import deactivate_batchnorm

pytestmark = pytest.mark.gpu

R = P.R
CL = torch.channels_last
PART = _lib.BN_POOL_GRAD_PART_ELEMS
CASES = P.cases(PART)
FORWARD_CASES = [n for n in CASES if not CASES[n][4]]          # all but the one that ties on purpose
OP_CASES = ("odd", "disjoint", "c2048")
INVALID, UNSUPPORTED, ALIGN, WORKSPACE = -1, -2, -3, -4        # enum mcgmil_status (include/mcgmil.h)
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(inputs, float64 CPU autograd with its window codes, gradient bounds, forward bounds); computed once."""
    shape, pool, relu, seed, integer = CASES[name]
    return _reference(P.make(shape, pool, seed, relu, integer))


def _reference(c):
    r64, r32 = P.autograd(c, torch.float64), P.autograd(c, torch.float32)
    r64["code"] = P.codes(r64["idx"], r64["y"], c["z"].shape[3], c["pool"], c["relu"])
    return c, r64, R.bounds(R.errors(r32, r64, P.GRADS)), R.bounds(R.errors(r32, r64, P.FWD))


def check(label, got, ref, bounds, keys=P.GRADS):
    err = R.errors(got, ref, keys)
    print(label, {k: f"{e:.1e}/{bounds[k]:.1e}" for k, e in err.items()})
    bad = {k: (e, bounds[k]) for k, e in err.items() if not e <= bounds[k]}
    assert not bad, (label, bad)
    for k in err:
        assert bool(torch.isfinite(got[k]).all()), (label, k)


def assert_margins(label, r64, pool):
    gap, top = P.margins(r64["a"], pool)
    print(f"{label}: smallest top-two gap {gap:.1e}, smallest |window maximum| {top:.1e} of the float64 reference")
    assert gap >= 1e-5 and top >= 1e-5


def dev_inputs(c, r64, dev):
    """z, code, dy channels-last and gamma, mean, invstd on the device; code / mean / invstd are the
    float64 reference's (mean and invstd rounded to fp32)."""
    cl = lambda t: t.to(dev).contiguous(memory_format=CL)  # noqa: E731
    v = lambda t: None if t is None else t.float().to(dev)  # noqa: E731
    return cl(c["z"]), cl(r64["code"]), cl(c["dy"]), v(c["gamma"]), v(r64["mean"]), v(r64["invstd"])


def backward_op(z, code, dy, gamma, mean, invstd, pool, need_dz=True, need_dw=True):
    out = torch.ops.mcgmil.bn_pool_f32_backward(z, code, dy, gamma, mean, invstd, *pool, need_dz, need_dw)
    torch.cuda.synchronize()
    return dict(zip(P.GRADS, out))


def grad_args(z, code, dy, gamma, mean, invstd, pool, outs):
    a = _lib.BnPoolGradArgs()
    a.batch, a.channels, a.height, a.width = z.shape
    a.pool_kernel, a.pool_stride, a.pool_pad = pool
    a.pooled_height, a.pooled_width = dy.shape[2:]
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a.z, a.argmax, a.dy, a.gamma, a.mean, a.invstd = p(z), p(code), p(dy), p(gamma), p(mean), p(invstd)
    a.dz, a.dgamma, a.dbeta = (p(outs.get(k)) for k in P.GRADS)
    return a


def capi_backward(z, code, dy, gamma, mean, invstd, pool, outs, ws_bytes=None):
    """mcgmil_batchnorm_pool_backward into the caller's output tensors (None: NULL)."""
    L = _lib.load()
    a = grad_args(z, code, dy, gamma, mean, invstd, pool, outs)
    n = ctypes.c_size_t()
    rc = L.mcgmil_bn_pool_grad_workspace_size(ctypes.byref(a), ctypes.byref(n))
    if rc:
        return rc, 0
    ws = torch.empty(n.value, dtype=torch.uint8, device=z.device)
    a.workspace, a.workspace_bytes = ctypes.c_void_p(ws.data_ptr()), n.value if ws_bytes is None else ws_bytes
    rc = L.mcgmil_batchnorm_pool_backward(ctypes.byref(a), None)
    torch.cuda.synchronize()
    return rc, n.value


def capi_forward(z, gamma, beta, relu, pool, y, mean, invstd, code, **over):
    """mcgmil_batchnorm_pool_train into the caller's tensors; `over` overrides fields of mcgmil_bn_args."""
    L = _lib.load()
    a = _lib.BnArgs()
    N, C, H, W = z.shape
    a.rows, a.channels, a.dtype = N * H * W, C, _lib.MCGMIL_F32
    a.batch, a.height, a.width = N, H, W
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a.x, a.y, a.gamma, a.beta = p(z), p(y), p(gamma), p(beta)
    a.eps, a.relu = P.EPS, int(relu)
    a.batch_mean, a.batch_invstd = p(mean), p(invstd)
    n = ctypes.c_size_t()
    _lib.check(L.mcgmil_bn_workspace_size(ctypes.byref(a), ctypes.byref(n)), "workspace size")   # not the pool's
    a.pool_kernel, a.pool_stride, a.pool_pad = pool
    ws = torch.empty(n.value, dtype=torch.uint8, device=z.device)
    a.workspace, a.workspace_bytes = p(ws), n.value
    for k, v in over.items():
        setattr(a, k, v)
    rc = L.mcgmil_batchnorm_pool_train(ctypes.byref(a), p(code), None)
    torch.cuda.synchronize()
    return rc


def fused_bn(c, dev):
    """An nn.BatchNorm2d on batch statistics with the case's gamma / beta, for features.batchnorm_act."""
    bn = nn.BatchNorm2d(c["z"].shape[1], eps=P.EPS, affine=c["gamma"] is not None).to(dev)
    deactivate_batchnorm(bn)
    if c["gamma"] is not None:
        with torch.no_grad():
            bn.weight.copy_(c["gamma"])
            bn.bias.copy_(c["beta"])
    return bn


# ---------------------------------------------------------------- 1. the backward kernels
@pytest.mark.parametrize("name", list(CASES))
def test_backward_kernels_match_float64(cuda, name):
    c, r64, bounds, _ = reference(name)
    z, code, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    outs = {"dz": torch.full_like(z, NAN), "dgamma": torch.full_like(mean, NAN), "dbeta": torch.full_like(mean, NAN)}
    rc, _ = capi_backward(z, code, dy, gamma, mean, invstd, c["pool"], outs)
    assert rc == 0
    check(f"{name} C ABI", outs, r64, bounds)
    a = backward_op(z, code, dy, gamma, mean, invstd, c["pool"])
    b = backward_op(z, code, dy, gamma, mean, invstd, c["pool"])
    for k in P.GRADS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], outs[k]), k
    assert a["dz"].is_contiguous(memory_format=CL)


def test_partition_has_at_least_four_blocks_with_a_ragged_last_one(cuda):
    N, C, H, W = CASES["blocks"][0]
    rows, rpp = N * H * W, PART // C
    assert C == 64 and rows // rpp >= 4 and rows % rpp != 0
    a = _lib.BnPoolGradArgs()
    a.batch, a.channels, a.height, a.width = N, C, H, W
    a.pool_kernel, a.pool_stride, a.pool_pad = 3, 2, 1
    a.pooled_height, a.pooled_width = P.pooled(H, 3, 2, 1), P.pooled(W, 3, 2, 1)
    n = ctypes.c_size_t()
    assert _lib.load().mcgmil_bn_pool_grad_workspace_size(ctypes.byref(a), ctypes.byref(n)) == 0
    assert n.value == ((4 * C + 2 * C * -(-rows // rpp)) * 4 + 255) // 256 * 256


def test_prepared_channels(cuda):
    """C = 64: channel 5 fully masked (every activation < 0) -> dgamma, dbeta and dz exactly 0;
    channel 9 with a negative gamma; then the whole layer with gamma = NULL."""
    shape, pool, _, _, _ = CASES["odd"]
    c = P.make(shape, pool, 11, True)
    c["gamma"][9] = -1.25
    c["beta"][5] = -50.0
    for label, cc in (("prepared", c), ("no gamma", dict(c, gamma=None, beta=None))):
        _, r64, bounds, _ = _reference(cc)
        r32 = P.autograd(cc, torch.float32)
        z, code, dy, gamma, mean, invstd = dev_inputs(cc, r64, cuda)
        ref = dict(r64)
        if gamma is None:                      # autograd has no dgamma / dbeta without parameters
            f = P.formula(cc["z"].double(), r64["code"], cc["dy"].double(), None, r64["mean"], r64["invstd"], pool)
            ref["dgamma"], ref["dbeta"] = f[1], f[2]
            code32 = P.codes(r32["idx"], r32["y"], shape[3], pool, True)
            e32 = P.formula(cc["z"], code32, cc["dy"], None, r32["mean"], r32["invstd"], pool)
            bounds = R.bounds(R.errors(dict(r32, dgamma=e32[1], dbeta=e32[2]), ref, P.GRADS))
        got = backward_op(z, code, dy, gamma, mean, invstd, pool)
        again = backward_op(z, code, dy, gamma, mean, invstd, pool)
        assert all(torch.equal(got[k], again[k]) for k in P.GRADS)
        check(label, got, ref, bounds)
        if gamma is not None:
            assert float(r64["y"][:, 5].abs().max()) == 0.0 and bool((r64["code"][:, 5] == P.NONE).all())
            assert float(got["dgamma"][5]) == 0.0 and float(got["dbeta"][5]) == 0.0
            assert float(got["dz"][:, 5].abs().max()) == 0.0
            assert float(c["gamma"][9]) < 0 and float(got["dz"][:, 9].abs().max()) > 0.0


def test_each_optional_output_in_turn(cuda):
    c, r64, _, _ = reference("odd")
    z, code, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    full = backward_op(z, code, dy, gamma, mean, invstd, c["pool"])
    for keep in (("dz",), ("dgamma",), ("dbeta",), ("dgamma", "dbeta"), ("dz", "dbeta")):
        outs = {k: torch.full_like(full[k], NAN) for k in keep}
        for _ in range(2):
            rc, _ = capi_backward(z, code, dy, gamma, mean, invstd, c["pool"], outs)
            assert rc == 0, keep
            for k, t in outs.items():
                assert torch.equal(t, full[k]), (keep, k)
    # the op's need_* flags: an empty tensor for what is not needed
    for flags in ((True, False), (False, True)):
        got = backward_op(z, code, dy, gamma, mean, invstd, c["pool"], *flags)
        need = {"dz": flags[0], "dgamma": flags[1], "dbeta": flags[1]}
        for k in P.GRADS:
            assert torch.equal(got[k], full[k]) if need[k] else got[k].numel() == 0, (flags, k)
    assert all(t is None for t in features.batchnorm_pool_backward(z, code, dy, gamma, mean, invstd, *c["pool"],
                                                                   need_dz=False, need_dw=False))


# ---------------------------------------------------------------- 2. the forward
@pytest.mark.parametrize("name", FORWARD_CASES)
def test_forward_is_batchnorm_act_bitwise_and_names_the_reference_argmax(cuda, name):
    c, r64, _, fbounds = reference(name)
    assert_margins(name, r64, c["pool"])
    z = c["z"].to(cuda).contiguous(memory_format=CL)
    gamma, beta = c["gamma"].to(cuda), c["beta"].to(cuda)
    with torch.no_grad():
        want = features.batchnorm_act(z, fused_bn(c, cuda), c["relu"], pool=nn.MaxPool2d(*c["pool"]))
    got = []
    for _ in range(2):
        y, code = torch.full_like(want, NAN), torch.full(want.shape, 77, dtype=torch.uint8, device=cuda).contiguous(memory_format=CL)
        mean, invstd = torch.full_like(gamma, NAN), torch.full_like(gamma, NAN)
        assert capi_forward(z, gamma, beta, c["relu"], c["pool"], y, mean, invstd, code) == 0
        got.append((y, mean, invstd, code))
    for s, t in zip(*got):
        assert torch.equal(s, t)
    y, mean, invstd, code = got[0]
    assert torch.equal(y, want)
    check(f"{name} forward", {"y": y, "mean": mean, "invstd": invstd}, r64, fbounds, P.FWD)
    assert torch.equal(code.cpu(), r64["code"])
    # the python entry point returns the same four tensors
    for s, t in zip(features.batchnorm_pool_stats(z, gamma, beta, P.EPS, c["relu"], *c["pool"]), got[0]):
        assert torch.equal(s, t) and s.shape == t.shape


# ---------------------------------------------------------------- 3. validation
def test_validation(cuda):
    c, r64, _, _ = reference("odd")
    pool = c["pool"]
    z, code, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    L = _lib.load()
    outs = {"dz": torch.empty_like(z)}
    call = lambda **k: capi_backward(**{**dict(z=z, code=code, dy=dy, gamma=gamma, mean=mean, invstd=invstd,  # noqa: E731
                                               pool=pool, outs=outs), **k})[0]
    assert call() == 0
    assert call(z=z[:1, :, :1, :1].contiguous(memory_format=CL), pool=(3, 2, 1),
                dy=dy[:1, :, :1, :1].contiguous(memory_format=CL)) == INVALID          # rows < 2
    assert call(z=z[:, :12].contiguous(memory_format=CL)) == UNSUPPORTED               # C = 12
    a = grad_args(z, code, dy, gamma, mean, invstd, pool, outs)
    a.channels = 4096
    n = ctypes.c_size_t()
    assert L.mcgmil_bn_pool_grad_workspace_size(ctypes.byref(a), ctypes.byref(n)) == UNSUPPORTED
    assert call(pool=(4, 2, 1)) == UNSUPPORTED                                         # k = 4
    assert call(pool=(3, 2, 2)) == UNSUPPORTED                                         # pad > k / 2
    assert call(pool=(2, 3, 0)) == UNSUPPORTED                                         # stride > k
    assert call(outs={"dz": z}) == INVALID                                             # an output aliasing an input
    assert call(outs={"dz": outs["dz"], "dgamma": mean}) == INVALID
    assert call(outs={}) == INVALID                                                    # no output
    assert call(ws_bytes=255) == WORKSPACE                                             # too small a workspace
    assert call(dy=dy[:, :, :-1].contiguous(memory_format=CL)) == INVALID              # not this pool's dy
    assert call(mean=mean[1:]) == ALIGN
    assert len(L.mcgmil_last_error()) > 0
    a = grad_args(z, code, dy, gamma, mean, invstd, pool, outs)
    a.reserved = 1
    assert L.mcgmil_bn_pool_grad_workspace_size(ctypes.byref(a), ctypes.byref(n)) == INVALID
    # the forward
    beta = c["beta"].to(cuda)
    y, cd = torch.empty_like(dy), torch.empty_like(code)
    m, s = torch.empty_like(mean), torch.empty_like(mean)
    fwd = lambda zz=z, pl=pool, yy=y, mm=m, **over: capi_forward(zz, gamma, beta, True, pl, yy, mm, s, cd, **over)  # noqa: E731
    assert fwd() == 0
    assert fwd(pl=(4, 2, 1)) == UNSUPPORTED and fwd(pl=(3, 2, 2)) == UNSUPPORTED
    assert fwd(dtype=_lib.MCGMIL_BF16) == UNSUPPORTED
    assert fwd(mm=None) == INVALID                                                     # batch_mean is required
    assert fwd(running_mean=ctypes.c_void_p(m.data_ptr()), running_var=ctypes.c_void_p(s.data_ptr())) == INVALID
    assert fwd(residual=ctypes.c_void_p(z.data_ptr())) == UNSUPPORTED
    assert fwd(workspace_bytes=255) == WORKSPACE
    assert capi_forward(z, gamma, beta, True, pool, y, m, s, None) == INVALID          # no argmax
    # the python entry points refuse what the kernels do not implement
    with pytest.raises(ValueError):
        features.batchnorm_pool_stats(z, gamma, beta, P.EPS, True, 4, 2, 1)
    with pytest.raises(ValueError):
        features.batchnorm_pool_stats(z.contiguous(), gamma, beta, P.EPS, True, *pool)
    with pytest.raises(ValueError):
        features.batchnorm_pool_backward(z, code, dy[:, :, :-1].contiguous(memory_format=CL), gamma, mean, invstd, *pool)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 4. 64-bit offsets
def test_byte_offsets_past_2_to_31(cuda):
    """33 x 64 x 512 x 512: z is 2.2 GB. The float64 reference (with its window codes) and the fp32
    bound both come from torch autograd on the GPU. The backward runs on the reference's codes; the
    forward's y is compared bitwise with batchnorm_act, and its codes with the reference's on the
    last image, whose z lies wholly past 2^31 bytes, wherever the float64 reference is at least 1e-5
    from a tie and from zero (2e8 windows cannot all keep that margin)."""
    shape, pool = (33, 64, 512, 512), (3, 2, 1)
    g = torch.Generator(device=cuda).manual_seed(7)
    z = (torch.randn(*shape, device=cuda, generator=g) + 0.5).contiguous(memory_format=CL)
    dy = torch.randn(33, 64, 256, 256, device=cuda, generator=g).contiguous(memory_format=CL)
    gamma = 0.5 + torch.rand(64, device=cuda, generator=g)
    beta = torch.zeros_like(gamma)
    assert z.numel() * 4 > 2 ** 31 and z[:32].numel() * 4 >= 2 ** 31
    case = {"z": z, "dy": dy, "gamma": gamma, "beta": beta, "relu": True, "pool": pool}
    r64 = P.autograd(case, torch.float64, cuda)
    code = P.codes(r64.pop("idx"), r64["y"], shape[3], pool, True).contiguous(memory_format=CL)
    a_last = r64.pop("a")[32:].clone()
    del r64["y"]
    r32 = {k: v for k, v in P.autograd(case, torch.float32, cuda).items() if k in P.GRADS}
    bounds = R.bounds(R.errors(r32, r64, P.GRADS))
    del r32
    mean, invstd = r64["mean"].float(), r64["invstd"].float()
    a = backward_op(z, code, dy, gamma, mean, invstd, pool)
    check("2.2 GB", a, r64, bounds)
    del r64
    b = backward_op(z, code, dy, gamma, mean, invstd, pool)
    for k in P.GRADS:
        assert torch.equal(a[k], b[k]), k
    del a, b, dy
    y, _, _, got = features.batchnorm_pool_stats(z, gamma, beta, P.EPS, True, *pool)
    with torch.no_grad():
        want = features.batchnorm_act(z, fused_bn(case, cuda), True, pool=nn.MaxPool2d(*pool))
    assert torch.equal(y, want)
    del y, want
    win = F.unfold(F.pad(a_last, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(1, 64, 9, 256, 256)
    top = win.topk(2, dim=2).values
    safe = ((top[:, :, 0] - top[:, :, 1]) >= 1e-5) & (top[:, :, 0].abs() >= 1e-5)
    print(f"last image: {int(safe.sum())} of {safe.numel()} windows at least 1e-5 from a tie and from zero")
    assert int(safe.sum()) > 0.99 * safe.numel()
    assert torch.equal(got[32:][safe], code[32:][safe])
    del z, code, got, win, top, safe, a_last
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 5. the differentiable op
def test_opcheck(cuda):
    c, r64, _, _ = reference("odd")
    z, code, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    beta = c["beta"].to(cuda)
    rq = lambda t: t.clone().requires_grad_()  # noqa: E731
    torch.library.opcheck(torch.ops.mcgmil.bn_pool_f32.default, (rq(z), rq(gamma), rq(beta), P.EPS, True, 3, 2, 1))
    torch.library.opcheck(torch.ops.mcgmil.bn_pool_f32.default, (rq(z), None, None, P.EPS, False, 2, 2, 0))
    torch.library.opcheck(torch.ops.mcgmil.bn_pool_f32_backward.default,
                          (z, code, dy, gamma, mean, invstd, 3, 2, 1, True, True))
    torch.library.opcheck(torch.ops.mcgmil.bn_pool_f32_backward.default,
                          (z, code, dy, None, mean, invstd, 3, 2, 1, True, False))


@pytest.mark.parametrize("name", OP_CASES)
def test_op_forward_and_autograd_match_float64(cuda, name):
    c, r64, bounds, fbounds = reference(name)
    assert_margins(name, r64, c["pool"])
    rq = lambda t: t.to(cuda).requires_grad_()  # noqa: E731
    z, gamma, beta = rq(c["z"]), rq(c["gamma"]), rq(c["beta"])                # z not channels-last: made so
    y, mean, invstd, code = torch.ops.mcgmil.bn_pool_f32(z, gamma, beta, P.EPS, c["relu"], *c["pool"])
    assert y.shape == r64["y"].shape == code.shape and y.is_contiguous(memory_format=CL)
    assert code.dtype == torch.uint8 and not code.requires_grad and mean.shape == invstd.shape == (z.shape[1],)
    check(f"{name} forward", {"y": y.detach(), "mean": mean.detach(), "invstd": invstd.detach()}, r64, fbounds, P.FWD)
    assert torch.equal(code.cpu(), r64["code"])
    # gradients flowing into mean / invstd are ignored: the loss below uses them on purpose
    (y * c["dy"].to(cuda)).sum().add(mean.sum() + invstd.sum()).backward()
    got = {"dz": z.grad, "dgamma": gamma.grad, "dbeta": beta.grad}
    check(f"{name} autograd", got, r64, bounds)
    # a backward of the backward raises
    z2 = rq(c["z"])
    y2, _, _, code2 = torch.ops.mcgmil.bn_pool_f32(z2, gamma, beta, P.EPS, c["relu"], *c["pool"])
    assert torch.equal(y2, y) and torch.equal(code2, code)
    (dz,) = torch.autograd.grad(y2.sum(), z2, create_graph=True)
    with pytest.raises(RuntimeError):
        dz.sum().backward()
    with pytest.raises((RuntimeError, ValueError)):
        torch.ops.mcgmil.bn_pool_f32(c["z"], None, None, P.EPS, True, *c["pool"])       # no CPU kernel


# ---------------------------------------------------------------- 6. routing and saved state
def _spy(monkeypatch):
    routed = []
    real = features.bn_pool_f32_op
    monkeypatch.setattr(features, "bn_pool_f32_op", lambda bn, *a, **k: routed.append(bn) or real(bn, *a, **k))
    return routed


def test_bn_act_routes_inside_the_context_only(cuda, monkeypatch):
    routed = _spy(monkeypatch)
    bn = nn.BatchNorm2d(64).to(cuda)
    deactivate_batchnorm(bn)
    pool = nn.MaxPool2d(3, 2, 1)
    x = torch.randn(3, 64, 9, 7, device=cuda, requires_grad=True)          # not channels-last: made so
    want = pool(torch.relu(bn(x)))
    assert features.bn_pool_trainable(x, bn, pool)
    y0 = features.bn_act(bn, x, True, pool=pool)
    with features.native_norm_training():
        features.bn_act(bn, x, True, pool=pool)
    assert not routed and torch.equal(y0, want)
    with features.native_stem_training():
        y1 = features.bn_act(bn, x, True, pool=pool)
        assert len(routed) == 1
        with torch.no_grad():
            features.bn_act(bn, x, True, pool=pool)
        features.bn_act(bn, x, True)                                        # no pool
        features.bn_act(bn, x, True, pool=nn.MaxPool2d(5, 2, 2))            # a pool outside the geometry
        features.bn_act(bn, x, True, pool=nn.MaxPool2d(3, 2, 1, ceil_mode=True))
        tracking = nn.BatchNorm2d(64).to(cuda)
        features.bn_act(tracking, x, True, pool=pool)                       # pending running-stat update
        assert len(routed) == 1 and float(tracking.running_mean.abs().max()) > 0
    assert torch.allclose(y1, want, atol=1e-5)
    y1.sum().backward()
    assert x.grad is not None and bn.weight.grad is not None and bool(torch.isfinite(x.grad).all())


def test_saved_state(cuda):
    """What autograd keeps for the stem's BatchNorm / ReLU / pool: z, one byte per pooled element and
    three [C] vectors with the op; z, an activation of z's size and int64 indices on torch's layers."""
    bn = nn.BatchNorm2d(64).to(cuda)
    deactivate_batchnorm(bn)
    pool = nn.MaxPool2d(3, 2, 1)
    z = torch.randn(3, 64, 16, 16, device=cuda).contiguous(memory_format=CL).requires_grad_()

    def saved_bytes(native):
        seen = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: seen.append(t.numel() * t.element_size()) or t,
                                                      lambda t: t), features.native_stem_training(native):
            y = features.bn_act(bn, z, True, pool=pool)
        return sum(seen), y
    op, y = saved_bytes(True)
    torch_layers, _ = saved_bytes(False)
    print(f"saved bytes: op {op}, torch layers {torch_layers}; z {4 * z.numel()}, y {4 * y.numel()}")
    assert op <= 4 * z.numel() + y.numel() + 16 * 64
    assert torch_layers >= 8 * z.numel() + 8 * y.numel()


# ---------------------------------------------------------------- 7. the module
MODULE_SEED = 354
PARAMS = ("feature_extractor.conv1.weight", "feature_extractor.bn1.weight", "feature_extractor.bn1.bias",
          "feature_extractor.layer1.0.conv1.weight", "classifiers.0.weight")


@functools.lru_cache(maxsize=None)
def module_case():
    """The r18 step of test_gpu_bn_grad.module_case (one bag of 3 instances of 64 x 64) with the
    gradients of PARAMS, which include the stem's, and MODULE_SEED: the first seed of 11..400 for
    which both the smallest |pre-activation| of any ReLU and the smallest top-two gap of the stem's
    pool windows are at least 1.2e-5 in the float64 backbone (found on the CPU; the test asserts
    >= 1e-5 for both). Returns module_case's tuple plus that gap."""
    import test_gpu_bn_grad as TB
    saved = TB.MODULE_SEED, TB.PARAMS
    TB.MODULE_SEED, TB.PARAMS = MODULE_SEED, PARAMS
    try:
        m, x, target, seed, g64, bounds, margin = TB.module_case.__wrapped__()
    finally:
        TB.MODULE_SEED, TB.PARAMS = saved
    fe = copy.deepcopy(m.feature_extractor).double().cpu()
    with torch.no_grad():
        a = fe.bn1(fe.conv1(x.double().cpu().view(-1, *x.shape[-3:])))
    return m, x, target, seed, g64, bounds, margin, P.margins(a, (3, 2, 1))[0]


def test_module_train_step_with_the_stem_opt_in(cuda, monkeypatch):
    import test_gpu_bn_grad as TB
    m0, x, target, seed, g64, bounds, margin, gap = module_case()
    routed = _spy(monkeypatch)
    pools = []
    real_pool = F.max_pool2d
    monkeypatch.setattr(F, "max_pool2d", lambda *a, **k: pools.append(1) or real_pool(*a, **k))
    print(f"float64 backbone: smallest |pre-activation| {margin:.2e}, smallest stem pool top-two gap {gap:.2e}")
    assert margin >= 1e-5 and gap >= 1e-5
    m = copy.deepcopy(m0).train().enable_head_training()
    assert m.enable_backbone_training(norm=True, stem=True) is m
    named = TB._step(m, x, target, seed)
    assert routed == [m.feature_extractor.bn1] and not pools
    for n in PARAMS:
        g = named[n].grad
        err = float((g.double().cpu() - g64[n]).abs().max() / g64[n].abs().max())
        print(f"norm=True, stem=True {n}: {err:.2e} / {bounds[n]:.2e}")
        assert bool(torch.isfinite(g).all()) and err <= bounds[n], n
    # stem alone (it does not depend on norm), then without the keyword: never routed
    m = copy.deepcopy(m0).train().enable_head_training().enable_backbone_training(stem=True)
    TB._step(m, x, target, seed)
    assert len(routed) == 2 and not pools
    del routed[:]
    m = copy.deepcopy(m0).train().enable_head_training().enable_backbone_training(norm=True)
    TB._step(m, x, target, seed)
    assert not routed and len(pools) == 1
