"""The fused bf16 BatchNorm/add/ReLU training op on the HIP kernels (include/mcgmil_bn_grad_bf16.h,
features.batchnorm_act_stats_bf16 / batchnorm_act_backward_bf16, torch.ops.mcgmil.bn_act_bf16 and
its backward op, MultiHeadGatedAttentionMIL.enable_bf16_norm_training()) against
float64 autograd of F.batch_norm (+ add, + relu).

Inputs are bn_grad_ref.make(...) with x, dy and the residual rounded to bf16 first (gamma and beta
stay fp32, the master parameters); every reference is computed from the rounded values, so what is
measured is the kernel, not the rounding of its inputs.

fp32 outputs (dgamma, dbeta, mean, invstd): bn_grad_ref.errors against bn_grad_ref.bounds, i.e. 10 x
the error of fp32 CPU autograd on that case, at least 1e-6. bf16 outputs (dx, y): elementwise
|d| <= 2^-7 |ref| + B max|ref| with B the case's fp32 bound for that tensor (the rule of
tests/test_gpu_conv_grad_bf16.py: 2^-8 is bf16's unit roundoff, doubled for rounding an fp32 result
that itself carries error B). Every test prints measured / bound before it asserts.

Kernel-level tests call the backward with y, mean and invstd from the float64 reference (y rounded
to bf16, mean and invstd to fp32), so the ReLU mask is the reference's own."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn as nn

import bn_grad_ref as R
import test_gpu_conv_grad_bf16 as CB        # the module case, its step and its drift rule
from mcgmil import _lib, features, library  # noqa: F401
from mcgmil.resnet import deactivate_batchnorm

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
PART = _lib.BN_GRAD_PART_ELEMS
CASES = {
    #             (N, H, W)     C     relu   residual  seed     (the shapes of tests/test_gpu_bn_grad.py)
    "r2_c8":      ((2, 1, 1),   8,    True,  False,    1),   # the smallest batch torch's training BN accepts
    "r189_c64":   ((3, 9, 7),   64,   True,  True,     1),   # rows no multiple of the 32 row lanes
    "r12_c2048":  ((3, 2, 2),   2048, True,  True,     3),   # one row lane, 256 channel groups
    "r48_c512":   ((3, 4, 4),   512,  False, True,     2),   # the residual gradient is dy
    # rows = 10 blocks of PART / 64 rows + 5: more than three partial blocks, the last one ragged
    "blocks":     ((1, 1, 10 * (PART // 64) + 5), 64, False, False, 5),
    "blocks_relu": ((1, 1, 10 * (PART // 64) + 5), 64, True, True, 6),
}
# seeds whose smallest |pre-activation| in float64 is >= 1e-5 after the rounding of x and the
# residual to bf16, so that no rounding of the forward can flip a ReLU mask (asserted in the test)
OP_SEEDS = {"r189_c64": 1, "r12_c2048": 2, "r48_c512": 2}


def _round(t):
    return None if t is None else t.to(BF).float()


def rounded(c):
    return dict(c, x=_round(c["x"]), dy=_round(c["dy"]), res=_round(c["res"]))


def refs(c):
    """(float64 CPU autograd, gradient bounds, forward bounds) of a case with rounded inputs."""
    r64 = R.autograd(c, torch.float64)
    r32 = R.autograd(c, torch.float32)
    return r64, R.bounds(R.errors(r32, r64)), R.bounds(R.errors(r32, r64, ("y", "mean", "invstd")))


@functools.lru_cache(maxsize=None)
def reference(name, seed=None):
    rs, C, relu, res, s = CASES[name]
    c = rounded(R.make(rs, C, s if seed is None else seed, relu, res))
    return (c,) + refs(c)


def check_f32(label, got, ref, bounds, keys, measure=R.GRADS):
    """The fp32 tensors `keys` against their bounds; the error measure's scale is taken over `measure`,
    the tensors the bounds were computed with."""
    err = {k: e for k, e in R.errors(got, ref, measure).items() if k in keys}
    print(label, {k: f"{e:.1e}/{bounds[k]:.1e}" for k, e in err.items()})
    assert set(err) == set(keys), (label, sorted(err))
    bad = {k: (e, bounds[k]) for k, e in err.items() if not e <= bounds[k]}
    assert not bad, (label, bad)
    for k in err:
        assert got[k].dtype == torch.float32 and bool(torch.isfinite(got[k]).all()), (label, k)


def check_bf16(label, got, ref, B):
    """|got - ref| <= 2^-7 |ref| + B max|ref| for every element."""
    assert got.dtype == BF and tuple(got.shape) == tuple(ref.shape), label
    ref = ref.double()
    allowed = 2.0 ** -7 * ref.abs() + B * ref.abs().max()
    d = (got.detach().cpu().double() - ref).abs()
    excess = float((d / allowed.clamp_min(1e-300)).max()) if float(allowed.max()) > 0 else float(d.max())
    print(f"{label}: max |d| / (2^-7 |ref| + {B:.1e} max|ref|) = {excess:.3f} / 1")
    assert excess <= 1.0, (label, excess)


def dev_inputs(c, r64, dev):
    """x, y, dy bf16 channels-last and gamma, mean, invstd fp32 on the device; y / mean / invstd are
    the float64 reference rounded."""
    cl = lambda t: t.to(dev, BF).contiguous(memory_format=CL)  # noqa: E731
    v = lambda t: None if t is None else t.float().to(dev)  # noqa: E731
    return cl(c["x"]), cl(r64["y"]), cl(c["dy"]), v(c["gamma"]), v(r64["mean"]), v(r64["invstd"])


def backward_op(x, y, dy, gamma, mean, invstd, relu, need_dx=True, need_dres=True, need_dw=True):
    out = torch.ops.mcgmil.bn_act_bf16_backward(x, y, dy, gamma, mean, invstd, relu, need_dx, need_dres, need_dw)
    torch.cuda.synchronize()
    return dict(zip(R.GRADS, out))


def capi_backward(x, y, dy, gamma, mean, invstd, relu, outs):
    """mcgmil_batchnorm_act_backward_bf16 into the caller's output tensors (None: NULL)."""
    L = _lib.load()
    a = _lib.BnGradBf16Args()
    a.rows, a.channels, a.relu = x.numel() // x.shape[1], x.shape[1], int(relu)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a.x, a.y, a.dy, a.gamma, a.mean, a.invstd = p(x), p(y), p(dy), p(gamma), p(mean), p(invstd)
    a.dx, a.dresidual, a.dgamma, a.dbeta = (p(outs.get(k)) for k in R.GRADS)
    n = ctypes.c_size_t()
    _lib.check(L.mcgmil_bn_grad_workspace_size_bf16(ctypes.byref(a), ctypes.byref(n)), "workspace size")
    ws = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    a.workspace, a.workspace_bytes = p(ws), n.value
    rc = L.mcgmil_batchnorm_act_backward_bf16(ctypes.byref(a), None)
    torch.cuda.synchronize()
    return rc, n.value


def check_grads(label, got, r64, bounds, c, dy):
    """dgamma / dbeta against the fp32 bounds, dx by the bf16 rule, dres bitwise dy masked."""
    check_f32(label, got, r64, bounds, ("dgamma", "dbeta"))
    check_bf16(f"{label} dx", got["dx"], r64["dx"], bounds["dx"])
    if c["relu"] and got.get("dres") is not None and got["dres"].numel():
        mask = (r64["y"] > 0).to(dy.device)
        assert torch.equal(got["dres"], torch.where(mask, dy, torch.zeros_like(dy))), label
        assert not bool((got["dres"][~mask].view(torch.int16) != 0).any()), label      # +0, not -0


# ---------------------------------------------------------------- 1. kernel-level parity
@pytest.mark.parametrize("name", list(CASES))
def test_backward_kernels_match_float64(cuda, name):
    c, r64, bounds, _ = reference(name)
    x, y, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    relu = c["relu"]
    nan = float("nan")
    # through the C ABI into NaN-filled outputs: every element is overwritten
    outs = {"dx": torch.full_like(x, nan), "dgamma": torch.full_like(mean, nan), "dbeta": torch.full_like(mean, nan)}
    if relu:
        outs["dres"] = torch.full_like(x, nan)
    rc, _ = capi_backward(x, y if relu else None, dy, gamma, mean, invstd, relu, outs)
    assert rc == 0
    assert all(bool(torch.isfinite(t).all()) for t in outs.values())
    check_grads(f"{name} C ABI", outs, r64, bounds, c, dy)
    # the op, twice: bitwise equal, and bitwise the C ABI call
    a = backward_op(x, y, dy, gamma, mean, invstd, relu)
    b = backward_op(x, y, dy, gamma, mean, invstd, relu)
    for k in R.GRADS:
        assert torch.equal(a[k], b[k]), k
        if k in outs:
            assert torch.equal(a[k], outs[k]), k
    assert a["dx"].dtype == BF and a["dgamma"].dtype == a["dbeta"].dtype == torch.float32
    if relu:
        assert a["dx"].is_contiguous(memory_format=CL) and a["dres"].is_contiguous(memory_format=CL)
    else:
        assert a["dres"].numel() == 0          # without ReLU the residual gradient is dy itself


# ---------------------------------------------------------------- 2. the tie to the fp32 kernel
@pytest.mark.parametrize("name", list(CASES))
def test_bitwise_tie_to_the_fp32_kernel(cuda, name):
    """The same thread-to-element map and summation order: on the same values dgamma and dbeta are
    bitwise the fp32 backward's and dx is its dx rounded to bf16 once. Catches any intermediate
    bf16 rounding, which the elementwise bound is too loose to see."""
    c, r64, _, _ = reference(name)
    x, y, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    relu = c["relu"]
    got = backward_op(x, y, dy, gamma, mean, invstd, relu)
    f = lambda t: t.float().contiguous(memory_format=CL)  # noqa: E731
    want = dict(zip(R.GRADS, torch.ops.mcgmil.bn_act_f32_backward(f(x), f(y), f(dy), gamma, mean, invstd, relu,
                                                                  True, True, True)))
    torch.cuda.synchronize()
    assert torch.equal(got["dgamma"], want["dgamma"]) and torch.equal(got["dbeta"], want["dbeta"])
    assert torch.equal(got["dx"], want["dx"].to(BF))
    if relu:
        assert torch.equal(got["dres"], want["dres"].to(BF)) and torch.equal(got["dres"].float(), want["dres"])


# ---------------------------------------------------------------- 3. special channels, optional outputs
def test_prepared_channels(cuda):
    """C = 64: channel 5 fully masked (every y = 0) -> dgamma, dbeta and dx exactly 0; channel 9 with
    a negative gamma; then the whole layer with gamma = NULL."""
    rs, C = (3, 9, 7), 64
    c = R.make(rs, C, 11, True, True)
    c["gamma"][9] = -1.25
    c["beta"][5] = -50.0                       # pre-activation far below 0 in every row
    c["res"][:, 5] = -c["res"][:, 5].abs()
    c = rounded(c)
    for label, cc in (("prepared", c), ("no gamma", dict(c, gamma=None, beta=None))):
        r64, r32 = R.autograd(cc, torch.float64), R.autograd(cc, torch.float32)
        bounds = R.bounds(R.errors(r32, r64))
        x, y, dy, gamma, mean, invstd = dev_inputs(cc, r64, cuda)
        got = backward_op(x, y, dy, gamma, mean, invstd, True)
        ref = dict(r64)
        if gamma is None:                      # autograd has no dgamma / dbeta without parameters
            f = R.formula(cc["x"].double(), r64["y"], cc["dy"].double(), None, r64["mean"], r64["invstd"], True)
            ref["dgamma"], ref["dbeta"] = f[2], f[3]
            e32 = R.formula(cc["x"], r64["y"].float(), cc["dy"], None, r32["mean"], r32["invstd"], True)
            r32 = dict(r32, dgamma=e32[2], dbeta=e32[3])
            bounds = R.bounds(R.errors(r32, ref))
        check_grads(label, got, ref, bounds, cc, dy)
        if gamma is not None:
            assert float(r64["y"][:, 5].abs().max()) == 0.0
            assert float(got["dgamma"][5]) == 0.0 and float(got["dbeta"][5]) == 0.0
            assert float(got["dx"][:, 5].abs().max()) == 0.0 and float(got["dres"][:, 5].abs().max()) == 0.0
            assert float(c["gamma"][9]) < 0 and float(got["dx"][:, 9].abs().max()) > 0.0


def test_each_optional_output_in_turn(cuda):
    c, r64, _, _ = reference("r189_c64")
    x, y, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    full = backward_op(x, y, dy, gamma, mean, invstd, True)
    for skip in R.GRADS:
        outs = {k: torch.full_like(full[k], float("nan")) for k in R.GRADS if k != skip}
        rc, _ = capi_backward(x, y, dy, gamma, mean, invstd, True, outs)
        assert rc == 0, skip
        for k, t in outs.items():
            assert torch.equal(t, full[k]), (skip, k)
    # the op's need_* flags: an empty tensor for what is not needed
    for flags in ((True, False, False), (False, True, False), (False, False, True), (True, True, False)):
        got = backward_op(x, y, dy, gamma, mean, invstd, True, *flags)
        need = dict(zip(("dx", "dres"), flags[:2]), dgamma=flags[2], dbeta=flags[2])
        for k in R.GRADS:
            assert torch.equal(got[k], full[k]) if need[k] else got[k].numel() == 0, (flags, k)


# ---------------------------------------------------------------- 4. past 2^31 bytes per tensor
def test_byte_offsets_past_2_to_31(cuda):
    """A [1, 64, 64, 64] block repeated 4,224 times along N: 2.2 GB per bf16 tensor, no ReLU, no
    residual. Repetition leaves the per-channel statistics and dx unchanged and multiplies dgamma
    and dbeta by 4,224, so the reference is float64 CPU autograd on the one block."""
    REP, C, H, W = 4224, 64, 64, 64
    c = rounded(R.make((1, H, W), C, 7, False, False))
    r64, bounds, _ = refs(c)
    nhwc = lambda t: t.to(cuda, BF).permute(0, 2, 3, 1).contiguous()  # noqa: E731
    big = lambda t: nhwc(t).expand(REP, H, W, C).contiguous().permute(0, 3, 1, 2)  # noqa: E731
    x, dy = big(c["x"]), big(c["dy"])
    assert x.is_contiguous(memory_format=CL) and x.numel() * 2 > 2 ** 31 and x.numel() > 2 ** 30
    gamma, mean, invstd = c["gamma"].to(cuda), r64["mean"].float().to(cuda), r64["invstd"].float().to(cuda)
    empty = x.new_empty((0,))
    a = backward_op(x, empty, dy, gamma, mean, invstd, False, True, False, True)
    ref = {"dgamma": REP * r64["dgamma"], "dbeta": REP * r64["dbeta"], "dx": r64["dx"]}
    # the scale of the measure: the two sums themselves (4,224 times the block's, far above dx's)
    check_f32("2.2 GB", a, ref, bounds, ("dgamma", "dbeta"), ("dgamma", "dbeta"))
    rdx = r64["dx"].to(cuda)
    allowed = 2.0 ** -7 * rdx.abs() + bounds["dx"] * rdx.abs().max()
    excess = 0.0
    for i in range(0, REP, 264):               # 16 chunks of 264 tiles
        d = (a["dx"][i:i + 264].double() - rdx).abs()
        excess = max(excess, float((d / allowed).max()))
    print(f"2.2 GB dx: max |d| / (2^-7 |ref| + {bounds['dx']:.1e} max|ref|) = {excess:.3f} / 1")
    assert excess <= 1.0
    del d, rdx, allowed
    b = backward_op(x, empty, dy, gamma, mean, invstd, False, True, False, True)
    for k in ("dx", "dgamma", "dbeta"):
        assert torch.equal(a[k], b[k]), k
    del a, b, x, dy
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 5. validation
def test_validation(cuda):
    c, r64, _, _ = reference("r189_c64")
    x, y, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    L = _lib.load()
    outs = {"dx": torch.empty_like(x)}
    assert capi_backward(x, y, dy, gamma, mean, invstd, True, outs)[0] == 0
    INVALID, UNSUPPORTED, ALIGN, WORKSPACE = -1, -2, -3, -4     # enum mcgmil_status (include/mcgmil.h)
    assert capi_backward(x, None, dy, gamma, mean, invstd, True, outs)[0] == INVALID      # relu needs y
    assert capi_backward(x, y, dy, gamma, mean, invstd, True, {})[0] == INVALID           # no output
    assert capi_backward(x, y, dy, gamma, mean, invstd, False, {"dres": outs["dx"]})[0] == INVALID
    assert capi_backward(x, y, dy, gamma, mean[1:], invstd, True, outs)[0] == ALIGN
    assert len(L.mcgmil_last_error()) > 0
    a = _lib.BnGradBf16Args()
    n = ctypes.c_size_t()
    for rows, ch, want in ((1, 64, INVALID), (189, 12, UNSUPPORTED), (189, 4096, UNSUPPORTED)):
        a.rows, a.channels = rows, ch
        assert L.mcgmil_bn_grad_workspace_size_bf16(ctypes.byref(a), ctypes.byref(n)) == want
    a.rows, a.channels, a.reserved = 189, 64, 1
    assert L.mcgmil_bn_grad_workspace_size_bf16(ctypes.byref(a), ctypes.byref(n)) == INVALID
    a.reserved = 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a.x, a.dy, a.mean, a.invstd, a.dx = p(x), p(dy), p(mean), p(invstd), p(outs["dx"])
    assert L.mcgmil_batchnorm_act_backward_bf16(ctypes.byref(a), None) == WORKSPACE
    # the python entry points refuse what the kernels do not implement
    with pytest.raises(ValueError):
        features.batchnorm_act_backward_bf16(x.contiguous(), y, dy, gamma, mean, invstd, True)   # not channels-last
    with pytest.raises(ValueError):
        features.batchnorm_act_backward_bf16(x.float(), y.float(), dy.float(), gamma, mean, invstd, True)
    with pytest.raises(ValueError):
        features.batchnorm_act_stats_bf16(x.float(), gamma, gamma, None, 1e-5, True)
    with pytest.raises(ValueError):
        features.batchnorm_act_stats_bf16(x.contiguous(), gamma, gamma, None, 1e-5, True)
    with pytest.raises(ValueError):
        features.batchnorm_act_stats_bf16(x, gamma.to(BF), gamma, None, 1e-5, True)              # fp32 parameters
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. the differentiable op
def test_opcheck(cuda):
    c, r64, _, _ = reference("r189_c64")
    x, y, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    beta = c["beta"].to(cuda)
    res = c["res"].to(cuda, BF).contiguous(memory_format=CL)
    rq = lambda t: t.clone().requires_grad_()  # noqa: E731
    torch.library.opcheck(torch.ops.mcgmil.bn_act_bf16.default, (rq(x), rq(gamma), rq(beta), rq(res), 1e-5, True))
    torch.library.opcheck(torch.ops.mcgmil.bn_act_bf16.default, (rq(x), None, None, None, 1e-5, False))
    torch.library.opcheck(torch.ops.mcgmil.bn_act_bf16_backward.default,
                          (x, y, dy, gamma, mean, invstd, True, True, True, True))
    torch.library.opcheck(torch.ops.mcgmil.bn_act_bf16_backward.default,
                          (x, x.new_empty((0,)), dy, None, mean, invstd, False, True, False, False))


@pytest.mark.parametrize("name", list(OP_SEEDS))
def test_op_forward_and_autograd_match_float64(cuda, name):
    c, r64, bounds, fbounds = reference(name, OP_SEEDS[name])
    # the seed is chosen so that no pre-activation sits where a rounding could flip the mask
    margin = float(r64["z"].abs().min())
    print(f"{name}: smallest |pre-activation| in float64 {margin:.1e}")
    assert margin >= 1e-5
    rq = lambda t, dt=None: t.to(cuda, dt).requires_grad_()  # noqa: E731
    x, gamma, beta, res = rq(c["x"], BF), rq(c["gamma"]), rq(c["beta"]), rq(c["res"], BF)
    y, mean, invstd = torch.ops.mcgmil.bn_act_bf16(x, gamma, beta, res, R.EPS, c["relu"])
    assert y.shape == x.shape and y.dtype == BF and y.is_contiguous(memory_format=CL)
    assert mean.shape == invstd.shape == (x.shape[1],) and mean.dtype == invstd.dtype == torch.float32
    check_f32(f"{name} forward", {"y": y.detach(), "mean": mean.detach(), "invstd": invstd.detach()}, r64, fbounds,
              ("mean", "invstd"), ("y", "mean", "invstd"))
    check_bf16(f"{name} forward y", y.detach(), r64["y"], fbounds["y"])
    if c["relu"]:
        assert torch.equal(y.detach().cpu() > 0, r64["y"] > 0)
    # gradients flowing into mean / invstd are ignored: the loss below uses them on purpose
    dy = c["dy"].to(cuda, BF)
    (y.float() * dy.float()).sum().add(mean.sum() + invstd.sum()).backward()
    got = {"dx": x.grad, "dres": res.grad, "dgamma": gamma.grad, "dbeta": beta.grad}
    assert x.grad.dtype == res.grad.dtype == BF and gamma.grad.dtype == beta.grad.dtype == torch.float32
    check_grads(f"{name} autograd", got, r64, bounds, c, dy)
    if not c["relu"]:
        assert torch.equal(res.grad, dy)       # without ReLU the residual's gradient is dy itself
    with pytest.raises((RuntimeError, ValueError)):
        torch.ops.mcgmil.bn_act_bf16(c["x"].to(BF), None, None, None, R.EPS, True)       # no CPU kernel


# ---------------------------------------------------------------- 7. routing
def test_bn_act_routes_inside_the_context_only(cuda, monkeypatch):
    routed, routed32 = [], []
    real, real32 = features.bn_act_bf16_op, features.bn_act_f32_op
    monkeypatch.setattr(features, "bn_act_bf16_op", lambda *a, **k: routed.append(1) or real(*a, **k))
    monkeypatch.setattr(features, "bn_act_f32_op", lambda *a, **k: routed32.append(1) or real32(*a, **k))
    bn = nn.BatchNorm2d(64).to(cuda)
    deactivate_batchnorm(bn)
    x = torch.randn(3, 64, 9, 7, device=cuda).to(BF).requires_grad_()      # not channels-last: made so
    want = torch.relu(bn(x) + x)
    assert features.bn_bf16_trainable(x, bn, x)
    y0 = features.bn_act(bn, x, True, x)
    assert not routed and y0.dtype == BF
    with features.native_norm_training():                                  # the fp32 context: not for bf16
        features.bn_act(bn, x, True, x)
    assert not routed and not routed32
    with features.native_norm_bf16_training():
        y1 = features.bn_act(bn, x, True, x)
        assert len(routed) == 1
        with torch.no_grad():
            features.bn_act(bn, x, True, x)
        features.bn_act(bn, x, True, pool=nn.MaxPool2d(3, 2, 1))           # pooling stays on torch
        tracking = nn.BatchNorm2d(64).to(cuda)
        features.bn_act(tracking, x, True)                                  # pending running-stat update
        assert len(routed) == 1 and float(tracking.running_mean.abs().max()) > 0
        x32 = x.detach().float().requires_grad_()
        features.bn_act(bn, x32, True, x32)                                 # an fp32 activation
        assert len(routed) == 1 and not routed32
    with features.native_norm_bf16_training(False):
        features.bn_act(bn, x, True, x)
    assert len(routed) == 1
    # two bf16 roundings of values of order 1 apart at the most
    assert y1.dtype == BF and torch.allclose(y1.float(), want.float(), atol=2.0 ** -6, rtol=2.0 ** -6)
    y1.float().sum().backward()
    assert x.grad is not None and x.grad.dtype == BF and bool(torch.isfinite(x.grad).all())
    assert bn.weight.grad is not None and bn.weight.grad.dtype == torch.float32


# ---------------------------------------------------------------- 8. the module
@pytest.mark.parametrize("route", ["native", None])
def test_module_train_step_with_the_norm_opt_in(cuda, route, monkeypatch):
    if route:
        monkeypatch.setenv("MCGMIL_CONV_GRAD", route)
    else:
        monkeypatch.delenv("MCGMIL_CONV_GRAD", raising=False)
    m0, x, target, seed, g32, gac, _ = CB.module_case()
    routed, backwards = [], []
    real, real_b = features.bn_act_bf16_op, features.batchnorm_act_backward_bf16
    monkeypatch.setattr(features, "bn_act_bf16_op", lambda bn, *a, **k: routed.append(bn) or real(bn, *a, **k))
    monkeypatch.setattr(features, "batchnorm_act_backward_bf16",
                        lambda *a, **k: backwards.append(1) or real_b(*a, **k))
    m = copy.deepcopy(m0)
    assert m.enable_bf16_backbone_training().enable_bf16_norm_training() is m
    grads, _, _ = CB._step(m, x, target, seed)
    assert len(routed) == 19 and len(backwards) == 19       # 16 in blocks, 3 downsample; the stem's stays on torch
    assert len(set(map(id, routed))) == 19 and m.feature_extractor.bn1 not in routed
    scale = max(float(g.abs().max()) for g in g32.values())
    rows = []
    for n, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any()), n
        assert g.dtype == torch.float32, n
        err, yard = CB._drift(g, g32[n], scale), CB._drift(gac[n], g32[n], scale)
        bound = 2.0 * yard + 1e-3
        rows.append((n, err, bound))
        print(f"route={route} norm=True {n}: {err:.2e} / {bound:.2e} (autocast over the torch layers: {yard:.2e})")
    for n, err, bound in rows:
        assert err <= bound, (n, err, bound)
    print(f"route={route} norm=True: worst drift / bound = {max(e / b for _, e, b in rows):.3f}")


def test_module_without_the_keyword_or_the_flag_routes_no_batchnorm(cuda, monkeypatch):
    m0, x, target, seed, _, _, _ = CB.module_case()
    routed, backwards = [], []
    real, real_b = features.bn_act_bf16_op, features.batchnorm_act_backward_bf16
    monkeypatch.setattr(features, "bn_act_bf16_op", lambda bn, *a, **k: routed.append(bn) or real(bn, *a, **k))
    monkeypatch.setattr(features, "batchnorm_act_backward_bf16",
                        lambda *a, **k: backwards.append(1) or real_b(*a, **k))
    off = copy.deepcopy(m0).enable_bf16_backbone_training().enable_bf16_norm_training().enable_bf16_backbone_training(False)
    for mm in (copy.deepcopy(m0).enable_bf16_backbone_training(),
               copy.deepcopy(m0).enable_bf16_backbone_training().enable_bf16_norm_training(False),
               copy.deepcopy(m0).enable_bf16_norm_training(),              # without the flag it sits on: fp32, no BN routed
               off, copy.deepcopy(off).enable_bf16_backbone_training()):
        CB._step(mm, x, target, seed)
        assert routed == [] and backwards == []


def test_module_eval_and_no_grad_are_unchanged(cuda, monkeypatch):
    m0, x, target, seed, _, _, _ = CB.module_case()
    routed = []
    real = features.bn_act_bf16_op
    monkeypatch.setattr(features, "bn_act_bf16_op", lambda bn, *a, **k: routed.append(bn) or real(bn, *a, **k))
    never = copy.deepcopy(m0).eval()
    flagged = copy.deepcopy(m0).enable_bf16_backbone_training().enable_bf16_norm_training().eval()
    Ye, Ae, _ = never(x, target)
    Yf, Af, _ = flagged(x, target)
    assert routed == [] and torch.equal(Yf, Ye) and torch.equal(Af, Ae)
    with torch.no_grad():
        Yn, An, _ = flagged(x, target)
        Ym, Am, _ = never(x, target)
    assert routed == [] and torch.equal(Yn, Ym) and torch.equal(An, Am)
