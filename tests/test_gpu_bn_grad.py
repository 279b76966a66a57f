"""The fused BatchNorm/add/ReLU training op on the HIP kernels (include/mcgmil_bn_grad.h,
features.batchnorm_act_stats / batchnorm_act_backward, torch.ops.mcgmil.bn_act_f32 and its backward
op, MultiHeadGatedAttentionMIL.enable_backbone_training(norm=True)) against float64 autograd of
F.batch_norm (+ add, + relu).

Error of tensor k: max|got - ref| / max(max|ref_k|, 1e-3 max_j max|ref_j|) over the case's
gradients j (bn_grad_ref.errors, the head-gradient tests' measure). Bound of tensor k: 10 x the
same error of fp32 CPU autograd on that case (the project's x10 for a changed summation order), at
least 1e-6. Every test prints measured / bound before it asserts.

Kernel-level tests call bn_act_f32_backward with y, mean and invstd from the float64 reference
rounded to fp32, so the ReLU mask is the reference's own; outputs are pre-filled with NaN through
the C ABI where the test needs to see them overwritten, and every call is made twice and compared
bitwise."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn_grad_ref as R
import head_grad_ref as href
import numpy as np
from mcgmil import MultiHeadGatedAttentionMIL, _lib, features, library, ops  # noqa: F401
from mcgmil.resnet import deactivate_batchnorm

pytestmark = pytest.mark.gpu

CL = torch.channels_last
PART = _lib.BN_GRAD_PART_ELEMS
CASES = {
    #             (N, H, W)     C     relu   residual  seed
    "r2_c8":      ((2, 1, 1),   8,    True,  False,    1),   # the smallest batch torch's training BN accepts
    "r189_c64":   ((3, 9, 7),   64,   True,  True,     1),   # rows no multiple of the 32 row lanes
    "r12_c2048":  ((3, 2, 2),   2048, True,  True,     3),   # one row lane, 256 channel groups
    "r48_c512":   ((3, 4, 4),   512,  False, True,     2),   # the residual gradient is dy
    # rows = 10 blocks of PART / 64 rows + 5: more than three partial blocks, the last one ragged
    "blocks":     ((1, 1, 10 * (PART // 64) + 5), 64, False, False, 5),
    "blocks_relu": ((1, 1, 10 * (PART // 64) + 5), 64, True, True, 6),
}
OP_CASES = ("r189_c64", "r12_c2048", "r48_c512")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(inputs, float64 CPU autograd, per-tensor gradient bounds, forward bounds); computed once."""
    rs, C, relu, res, seed = CASES[name]
    c = R.make(rs, C, seed, relu, res)
    r64 = R.autograd(c, torch.float64)
    r32 = R.autograd(c, torch.float32)
    fwd = ("y", "mean", "invstd")
    return c, r64, R.bounds(R.errors(r32, r64)), R.bounds(R.errors(r32, r64, fwd))


def check(label, got, ref, bounds, keys=R.GRADS):
    err = R.errors(got, ref, keys)
    print(label, {k: f"{e:.1e}/{bounds[k]:.1e}" for k, e in err.items()})
    bad = {k: (e, bounds[k]) for k, e in err.items() if not e <= bounds[k]}
    assert not bad, (label, bad)
    for k in err:
        assert bool(torch.isfinite(got[k]).all()), (label, k)


def dev_inputs(c, r64, dev):
    """x, y, dy channels-last and gamma, mean, invstd on the device; y / mean / invstd are the
    float64 reference rounded to fp32."""
    cl = lambda t: t.float().to(dev).contiguous(memory_format=CL)  # noqa: E731
    v = lambda t: None if t is None else t.float().to(dev)  # noqa: E731
    return cl(c["x"]), cl(r64["y"]), cl(c["dy"]), v(c["gamma"]), v(r64["mean"]), v(r64["invstd"])


def backward_op(x, y, dy, gamma, mean, invstd, relu, need_dx=True, need_dres=True, need_dw=True):
    out = torch.ops.mcgmil.bn_act_f32_backward(x, y, dy, gamma, mean, invstd, relu, need_dx, need_dres, need_dw)
    torch.cuda.synchronize()
    return dict(zip(R.GRADS, out))


def capi_backward(x, y, dy, gamma, mean, invstd, relu, outs):
    """mcgmil_batchnorm_act_backward into the caller's output tensors (None: NULL)."""
    L = _lib.load()
    a = _lib.BnGradArgs()
    a.rows, a.channels, a.relu = x.numel() // x.shape[1], x.shape[1], int(relu)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a.x, a.y, a.dy, a.gamma, a.mean, a.invstd = p(x), p(y), p(dy), p(gamma), p(mean), p(invstd)
    a.dx, a.dresidual, a.dgamma, a.dbeta = (p(outs.get(k)) for k in R.GRADS)
    n = ctypes.c_size_t()
    _lib.check(L.mcgmil_bn_grad_workspace_size(ctypes.byref(a), ctypes.byref(n)), "workspace size")
    ws = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    a.workspace, a.workspace_bytes = p(ws), n.value
    rc = L.mcgmil_batchnorm_act_backward(ctypes.byref(a), None)
    torch.cuda.synchronize()
    return rc, n.value


# ---------------------------------------------------------------- 1. kernel-level parity
@pytest.mark.parametrize("name", list(CASES))
def test_backward_kernels_match_float64(cuda, name):
    c, r64, bounds, _ = reference(name)
    x, y, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    relu = c["relu"]
    # through the C ABI into NaN-filled outputs: every element is overwritten
    outs = {"dx": torch.full_like(x, float("nan")), "dgamma": torch.full_like(mean, float("nan")),
            "dbeta": torch.full_like(mean, float("nan"))}
    if relu:
        outs["dres"] = torch.full_like(x, float("nan"))
    rc, _ = capi_backward(x, y if relu else None, dy, gamma, mean, invstd, relu, outs)
    assert rc == 0
    check(f"{name} C ABI", outs, r64, bounds)
    # the op, twice: bitwise equal, and bitwise the C ABI call
    a = backward_op(x, y, dy, gamma, mean, invstd, relu)
    b = backward_op(x, y, dy, gamma, mean, invstd, relu)
    for k in R.GRADS:
        assert torch.equal(a[k], b[k]), k
        if k in outs:
            assert torch.equal(a[k], outs[k]), k
    if relu:
        assert a["dx"].is_contiguous(memory_format=CL) and a["dres"].is_contiguous(memory_format=CL)
    else:
        assert a["dres"].numel() == 0          # without ReLU the residual gradient is dy itself


def test_partition_has_more_than_three_blocks_with_a_ragged_last_one(cuda):
    rows = CASES["blocks"][0][2]
    rpp = PART // 64
    assert rpp <= 2048 and rows // rpp >= 3 and rows % rpp != 0
    a = _lib.BnGradArgs()
    a.rows, a.channels = rows, 64
    n = ctypes.c_size_t()
    assert _lib.load().mcgmil_bn_grad_workspace_size(ctypes.byref(a), ctypes.byref(n)) == 0
    parts = -(-rows // rpp)
    assert n.value == ((4 * 64 + 2 * 64 * parts) * 4 + 255) // 256 * 256


def test_prepared_channels(cuda):
    """C = 64: channel 5 fully masked (every y = 0) -> dgamma, dbeta and dx exactly 0; channel 9 with
    a negative gamma; then the whole layer with gamma = NULL."""
    rs, C = (3, 9, 7), 64
    c = R.make(rs, C, 11, True, True)
    c["gamma"][9] = -1.25
    c["beta"][5] = -50.0                       # pre-activation far below 0 in every row
    c["res"][:, 5] = -c["res"][:, 5].abs()
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
        check(label, got, ref, bounds)
        if gamma is not None:
            assert float(r64["y"][:, 5].abs().max()) == 0.0
            assert float(got["dgamma"][5]) == 0.0 and float(got["dbeta"][5]) == 0.0
            assert float(got["dx"][:, 5].abs().max()) == 0.0 and float(got["dres"][:, 5].abs().max()) == 0.0
            assert float(c["gamma"][9]) < 0 and float(got["dx"][:, 9].abs().max()) > 0.0


def test_each_optional_output_in_turn(cuda):
    c, r64, bounds, _ = reference("r189_c64")
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


def test_byte_offsets_past_2_to_31(cuda):
    """33 x 64 x 512 x 512: 2.2 GB per tensor, no ReLU, no residual. The float64 reference and the
    fp32 bound both come from torch autograd on the GPU."""
    N, C, H, W = 33, 64, 512, 512
    g = torch.Generator(device=cuda).manual_seed(7)
    x = (torch.randn(N, C, H, W, device=cuda, generator=g) + 0.5).contiguous(memory_format=CL)
    dy = torch.randn(N, C, H, W, device=cuda, generator=g).contiguous(memory_format=CL)
    gamma = 0.5 + torch.rand(C, device=cuda, generator=g)
    assert x.numel() * 4 > 2 ** 31
    case = {"x": x, "dy": dy, "gamma": gamma, "beta": torch.zeros_like(gamma), "res": None, "relu": False}
    r64 = R.autograd(case, torch.float64, cuda)
    r64 = {k: v for k, v in r64.items() if k in ("mean", "invstd", "dx", "dgamma", "dbeta")}
    r32 = {k: v for k, v in R.autograd(case, torch.float32, cuda).items() if k in R.GRADS}
    bounds = R.bounds(R.errors(r32, r64))
    del r32
    mean, invstd = r64["mean"].float(), r64["invstd"].float()
    empty = x.new_empty((0,))
    a = backward_op(x, empty, dy, gamma, mean, invstd, False, True, False, True)
    check("2.2 GB", a, r64, bounds)
    del r64
    b = backward_op(x, empty, dy, gamma, mean, invstd, False, True, False, True)
    for k in ("dx", "dgamma", "dbeta"):
        assert torch.equal(a[k], b[k]), k
    del a, b, x, dy
    torch.cuda.empty_cache()


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
    a = _lib.BnGradArgs()
    n = ctypes.c_size_t()
    for rows, ch, want in ((1, 64, INVALID), (189, 12, UNSUPPORTED), (189, 4096, UNSUPPORTED)):
        a.rows, a.channels = rows, ch
        assert L.mcgmil_bn_grad_workspace_size(ctypes.byref(a), ctypes.byref(n)) == want
    a.rows, a.channels, a.reserved = 189, 64, 1
    assert L.mcgmil_bn_grad_workspace_size(ctypes.byref(a), ctypes.byref(n)) == INVALID
    a.reserved = 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a.x, a.dy, a.mean, a.invstd, a.dx = p(x), p(dy), p(mean), p(invstd), p(outs["dx"])
    assert L.mcgmil_batchnorm_act_backward(ctypes.byref(a), None) == WORKSPACE
    # the python entry points refuse what the kernels do not implement
    with pytest.raises(ValueError):
        features.batchnorm_act_backward(x.contiguous(), y, dy, gamma, mean, invstd, True)
    with pytest.raises(ValueError):
        features.batchnorm_act_stats(x.bfloat16(), gamma, gamma, None, 1e-5, True)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. the differentiable op
def test_opcheck(cuda):
    c, r64, _, _ = reference("r189_c64")
    x, y, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    beta = c["beta"].to(cuda)
    res = c["res"].to(cuda).contiguous(memory_format=CL)
    rq = lambda t: t.clone().requires_grad_()  # noqa: E731
    torch.library.opcheck(torch.ops.mcgmil.bn_act_f32.default, (rq(x), rq(gamma), rq(beta), rq(res), 1e-5, True))
    torch.library.opcheck(torch.ops.mcgmil.bn_act_f32.default, (rq(x), None, None, None, 1e-5, False))
    torch.library.opcheck(torch.ops.mcgmil.bn_act_f32_backward.default,
                          (x, y, dy, gamma, mean, invstd, True, True, True, True))
    torch.library.opcheck(torch.ops.mcgmil.bn_act_f32_backward.default,
                          (x, x.new_empty((0,)), dy, None, mean, invstd, False, True, False, False))


@pytest.mark.parametrize("name", OP_CASES)
def test_op_forward_and_autograd_match_float64(cuda, name):
    c, r64, bounds, fbounds = reference(name)
    # the seed is chosen so that no pre-activation sits where fp32 rounding could flip the mask
    assert float(r64["z"].abs().min()) >= 1e-5
    rq = lambda t: t.to(cuda).requires_grad_()  # noqa: E731
    x, gamma, beta, res = rq(c["x"]), rq(c["gamma"]), rq(c["beta"]), rq(c["res"])
    y, mean, invstd = torch.ops.mcgmil.bn_act_f32(x, gamma, beta, res, R.EPS, c["relu"])
    assert y.shape == x.shape and y.is_contiguous(memory_format=CL) and mean.shape == invstd.shape == (x.shape[1],)
    check(f"{name} forward", {"y": y.detach(), "mean": mean.detach(), "invstd": invstd.detach()}, r64, fbounds,
          ("y", "mean", "invstd"))
    if c["relu"]:
        assert torch.equal(y.detach().cpu() > 0, r64["y"] > 0)
    # gradients flowing into mean / invstd are ignored: the loss below uses them on purpose
    (y * c["dy"].to(cuda)).sum().add(mean.sum() + invstd.sum()).backward()
    got = {"dx": x.grad, "dres": res.grad, "dgamma": gamma.grad, "dbeta": beta.grad}
    check(f"{name} autograd", got, r64, bounds)
    if not c["relu"]:
        assert torch.equal(res.grad.cpu(), c["dy"])
    with pytest.raises((RuntimeError, ValueError)):
        torch.ops.mcgmil.bn_act_f32(c["x"], None, None, None, R.EPS, True)       # no CPU kernel


def test_bn_act_routes_inside_the_context_only(cuda, monkeypatch):
    routed = []
    real = features.bn_act_f32_op
    monkeypatch.setattr(features, "bn_act_f32_op", lambda *a, **k: routed.append(1) or real(*a, **k))
    bn = nn.BatchNorm2d(64).to(cuda)
    deactivate_batchnorm(bn)
    x = torch.randn(3, 64, 9, 7, device=cuda, requires_grad=True)          # not channels-last: made so
    want = torch.relu(bn(x) + x)
    assert features.bn_trainable(x, bn, x)
    y0 = features.bn_act(bn, x, True, x)
    assert not routed and torch.equal(y0, want)
    with features.native_norm_training():
        y1 = features.bn_act(bn, x, True, x)
        assert len(routed) == 1
        with torch.no_grad():
            features.bn_act(bn, x, True, x)
        features.bn_act(bn, x, True, pool=nn.MaxPool2d(3, 2, 1))           # pooling stays on torch
        tracking = nn.BatchNorm2d(64).to(cuda)
        features.bn_act(tracking, x, True)                                  # pending running-stat update
        assert len(routed) == 1 and float(tracking.running_mean.abs().max()) > 0
    assert torch.allclose(y1, want, atol=1e-5)
    y1.sum().backward()
    assert x.grad is not None and bn.weight.grad is not None and bool(torch.isfinite(x.grad).all())


# ---------------------------------------------------------------- 3. the module
MODULE_SEED = 275
PARAMS = ("feature_extractor.conv1.weight", "feature_extractor.layer1.0.conv1.weight",
          "feature_extractor.layer1.0.bn1.weight", "feature_extractor.layer2.0.downsample.1.bias",
          "feature_extractor.layer4.1.bn2.weight", "classifiers.0.weight")


@functools.lru_cache(maxsize=None)
def module_case():
    """The r18 module (BatchNorm on batch statistics, as the reference's scripts set it), one bag of
    3 instances of 64 x 64, and the float64 / fp32 CPU gradients of PARAMS for one train step (the
    step of tests/test_gpu_conv_grad.py::module_case: the head restated in torch with the
    kernel's own masks), plus the smallest |pre-activation| of any ReLU of the float64 backbone.

    MODULE_SEED: a ReLU mask is discontinuous, so a bound made of rounding errors only holds where
    no pre-activation of the float64 reference lies within fp32 noise of zero (the activations of
    two fp32 routes differ by about 1e-6 in the deeper layers). With torch.manual_seed(3), the seed
    of the convolution tests' step, one pre-activation of layer2.0.bn2 is 2e-6: the fused forward
    lands on the other side of zero there and the gradients of every earlier layer move by 1e-2
    (the convolution tests' routes happen to land on float64's side). The seed is the first of
    11..400 whose margin is at least 1.2e-5; the test asserts the margin (>= 1e-5, the margin of
    the op-level cases) before it runs the step."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(MODULE_SEED)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False)
    m.apply(deactivate_batchnorm)
    x = torch.rand(1, 3, 3, 64, 64).to(dev)
    m = m.to(dev).train()
    target = torch.tensor([1], device=dev)
    seed = 99
    pf, pa = m._dropout_ps()
    offs = ops.bag_offsets_tensor([3], dev)
    keepF = torch.from_numpy(np.unpackbits(ops.feature_keep(offs, 3, 1, 512, pf, seed).cpu().numpy(), axis=1,
                                           bitorder="little").reshape(1, 3, 512))
    keepA = ops.attention_keep(offs, 3, 1, 2, pa, seed).cpu().view(1, 2, 3)

    margin = []
    real = features.bn_act

    def spy(bn, xx, relu, residual=None, pool=None):
        if relu and xx.dtype == torch.float64:
            with torch.no_grad():
                margin.append(float((bn(xx) if residual is None else bn(xx) + residual).abs().min()))
        return real(bn, xx, relu, residual, pool)

    def grads(mod, xx):
        features.bn_act = spy
        try:
            H = mod.extract_features(xx)[0]
        finally:
            features.bn_act = real
        Y, A = href.head_forward(H, mod._live_head(), keepF, keepA, pf, pa)
        (F.cross_entropy(Y, target.cpu()) +
         mod.auxiliary_loss.scale * mod.auxiliary_loss(A[:, 1, :], A[:, 0, :], True)).backward()
        named = dict(mod.named_parameters())
        return {n: named[n].grad.double() for n in PARAMS}
    g64 = grads(copy.deepcopy(m).double().cpu(), x.double().cpu())
    g32 = grads(copy.deepcopy(m).cpu(), x.cpu())
    e32 = {n: float((g32[n] - g64[n]).abs().max() / g64[n].abs().max()) for n in PARAMS}
    assert len(margin) == 17                    # the stem's ReLU and two per block
    return m, x, target, seed, g64, R.bounds(e32), min(margin)


def _step(m, x, target, seed):
    Y, A, aux = m(x, target, seed=seed)
    (F.cross_entropy(Y, target) + aux).backward()
    torch.cuda.synchronize()
    return dict(m.named_parameters())


def test_module_train_step_with_the_norm_opt_in(cuda, monkeypatch):
    routed = []
    real = features.bn_act_f32_op
    monkeypatch.setattr(features, "bn_act_f32_op", lambda bn, *a, **k: routed.append(bn) or real(bn, *a, **k))
    m0, x, target, seed, g64, bounds, margin = module_case()
    print(f"smallest |pre-activation| of the float64 backbone: {margin:.2e}")
    assert margin >= 1e-5
    m = copy.deepcopy(m0).train().enable_head_training()
    assert m.enable_backbone_training(norm=True) is m
    named = _step(m, x, target, seed)
    assert len(routed) == 19                    # every BatchNorm of the blocks; the stem's stays on torch
    assert m.feature_extractor.bn1 not in routed
    for n in PARAMS:
        g = named[n].grad
        err = float((g.double().cpu() - g64[n]).abs().max() / g64[n].abs().max())
        print(f"norm=True {n}: {err:.2e} / {bounds[n]:.2e}")
        assert bool(torch.isfinite(g).all()) and err <= bounds[n], n
    # without the keyword nothing is routed
    del routed[:]
    m = copy.deepcopy(m0).train().enable_head_training().enable_backbone_training()
    _step(m, x, target, seed)
    assert not routed


def test_module_keeps_the_torch_path_for_a_bn_that_tracks_running_statistics(cuda, monkeypatch):
    routed = []
    real = features.bn_act_f32_op
    monkeypatch.setattr(features, "bn_act_f32_op", lambda bn, *a, **k: routed.append(bn) or real(bn, *a, **k))
    m0, x, target, seed, _, _, _ = module_case()
    m = copy.deepcopy(m0).train().enable_head_training().enable_backbone_training(norm=True)
    bn = m.feature_extractor.layer1[0].bn1
    bn.track_running_stats = True
    bn.running_mean, bn.running_var = torch.zeros(64, device=cuda), torch.ones(64, device=cuda)
    named = _step(m, x, target, seed)
    assert len(routed) == 18 and bn not in routed
    assert float(bn.running_mean.abs().max()) > 0 and not torch.equal(bn.running_var, torch.ones(64, device=cuda))
    assert all(bool(torch.isfinite(p.grad).all()) for n, p in named.items() if p.grad is not None)
    assert bn.weight.grad is not None
