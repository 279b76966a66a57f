"""The bf16 form of the stem's fused BatchNorm / ReLU / max-pool training op on the HIP kernels
(include/mcgmil_pool_grad_bf16.h, features.batchnorm_pool_stats_bf16 / batchnorm_pool_backward_bf16,
torch.ops.mcgmil.bn_pool_bf16 and its backward op,
MultiHeadGatedAttentionMIL.enable_bf16_stem_training()).

Inputs are pool_grad_ref's cases with z and dy rounded to bf16 first (gamma and beta stay fp32, the
master parameters); every reference is float64 (or, for the bounds, fp32) CPU autograd of the
UNROUNDED max_pool2d(relu?(batch_norm(z))) on the rounded values (pool_grad_bf16_ref). The op is not
compared with torch's bf16 autograd element by element: torch pools the BatchNorm output after
rounding it to bf16 and gives a window whose two largest taps round alike to the first of them; the
op gives it to the tap whose unrounded value is larger. Both are subgradients of the same y.

fp32 outputs (dgamma, dbeta, mean, invstd): bn_grad_ref.errors against bn_grad_ref.bounds, i.e. 10 x
the error of fp32 CPU autograd on that case, at least 1e-6. bf16 outputs (dz, y): elementwise
|d| <= 2^-7 |ref| + B max|ref| with B the case's fp32 bound for that tensor (the rule of
tests/test_gpu_bn_grad_bf16.py). Every test prints measured / bound before it asserts.

Kernel-level tests call the backward with the window codes, mean and invstd of the float64
reference. Tests of the forward assert first that the float64 reference is not within 1e-5 of zero
in any window and that no two largest taps of a window are closer than 1e-5 unless they are equal
(the rounding of z makes exact ties, which the reference and the kernel both give to the first
tap), and then excuse no element: the codes must be the reference's exactly. Outputs passed through
the C ABI are pre-filled with NaN, and every device call is made twice and compared bitwise."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pool_grad_bf16_ref as PB
import test_gpu_conv_grad_bf16 as CB        # the module case, its step and its drift rule
from mcgmil import _lib, features, library  # noqa: F401
from mcgmil.resnet import deactivate_batchnorm

pytestmark = pytest.mark.gpu

P, R = PB.P, PB.R
CL = torch.channels_last
BF = torch.bfloat16
PART = _lib.BN_POOL_GRAD_PART_ELEMS
CASES = PB.CASES
CROSS_CASES = ("blocks", "ties", "c2048")
OP_CASES = ("odd", "clip", "disjoint")
INVALID, UNSUPPORTED, ALIGN, WORKSPACE = -1, -2, -3, -4        # enum mcgmil_status (include/mcgmil.h)
NAN = float("nan")


def reference(name):
    """(inputs, float64 reference with "code", gradient bounds, forward bounds); shared, read-only."""
    c, r64, _, bounds, fbounds = PB.reference(name)
    return c, r64, bounds, fbounds


def check_f32(label, got, ref, bounds, keys, measure):
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
    excess = PB.bf16_excess(got.cpu(), ref, B)
    print(f"{label}: max |d| / (2^-7 |ref| + {B:.1e} max|ref|) = {excess:.3f} / 1")
    assert excess <= 1.0 and bool(torch.isfinite(got.float()).all()), (label, excess)


def check_grads(label, got, ref, bounds):
    check_f32(label, got, ref, bounds, [k for k in ("dgamma", "dbeta") if ref.get(k) is not None], P.GRADS)
    check_bf16(f"{label} dz", got["dz"], ref["dz"], bounds["dz"])


def assert_margins(label, r64, pool):
    gap, top = PB.margins(r64["a"], pool)
    print(f"{label}: smallest non-zero top-two gap {gap:.1e}, smallest |window maximum| {top:.1e} "
          "of the float64 reference")
    assert gap >= 1e-5 and top >= 1e-5


def dev_inputs(c, r64, dev):
    """z, dy bf16 and the codes channels-last, gamma, mean, invstd fp32 on the device; code / mean /
    invstd are the float64 reference's (mean and invstd rounded to fp32)."""
    cl = lambda t, dt=None: t.to(dev, dt).contiguous(memory_format=CL)  # noqa: E731
    v = lambda t: None if t is None else t.float().to(dev)  # noqa: E731
    return cl(c["z"], BF), cl(r64["code"]), cl(c["dy"], BF), v(c["gamma"]), v(r64["mean"]), v(r64["invstd"])


def backward_op(z, code, dy, gamma, mean, invstd, pool, need_dz=True, need_dw=True):
    out = torch.ops.mcgmil.bn_pool_bf16_backward(z, code, dy, gamma, mean, invstd, *pool, need_dz, need_dw)
    torch.cuda.synchronize()
    return dict(zip(P.GRADS, out))


def grad_args(z, code, dy, gamma, mean, invstd, pool, outs, cls=None):
    a = (cls or _lib.BnPoolGradBf16Args)()
    a.batch, a.channels, a.height, a.width = z.shape
    a.pool_kernel, a.pool_stride, a.pool_pad = pool
    a.pooled_height, a.pooled_width = dy.shape[2:]
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a.z, a.argmax, a.dy, a.gamma, a.mean, a.invstd = p(z), p(code), p(dy), p(gamma), p(mean), p(invstd)
    a.dz, a.dgamma, a.dbeta = (p(outs.get(k)) for k in P.GRADS)
    return a


def capi_backward(z, code, dy, gamma, mean, invstd, pool, outs, ws_bytes=None, fp32=False):
    """mcgmil_batchnorm_pool_backward_bf16 (fp32: mcgmil_batchnorm_pool_backward) into the caller's
    output tensors (None: NULL)."""
    L = _lib.load()
    a = grad_args(z, code, dy, gamma, mean, invstd, pool, outs, _lib.BnPoolGradArgs if fp32 else None)
    size = L.mcgmil_bn_pool_grad_workspace_size if fp32 else L.mcgmil_bn_pool_grad_workspace_size_bf16
    run = L.mcgmil_batchnorm_pool_backward if fp32 else L.mcgmil_batchnorm_pool_backward_bf16
    n = ctypes.c_size_t()
    rc = size(ctypes.byref(a), ctypes.byref(n))
    if rc:
        return rc, 0
    ws = torch.empty(n.value, dtype=torch.uint8, device=z.device)
    a.workspace, a.workspace_bytes = ctypes.c_void_p(ws.data_ptr()), n.value if ws_bytes is None else ws_bytes
    rc = run(ctypes.byref(a), None)
    torch.cuda.synchronize()
    return rc, n.value


def capi_forward(z, gamma, beta, relu, pool, y, mean, invstd, code, **over):
    """mcgmil_batchnorm_pool_train_bf16 into the caller's tensors; `over` overrides fields of mcgmil_bn_args."""
    L = _lib.load()
    a = _lib.BnArgs()
    N, C, H, W = z.shape
    a.rows, a.channels, a.dtype = N * H * W, C, _lib.MCGMIL_BF16
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
    rc = L.mcgmil_batchnorm_pool_train_bf16(ctypes.byref(a), p(code), None)
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
    rc, _ = capi_backward(z, code, dy, gamma, mean, invstd, c["pool"], outs)     # overwrites, never accumulates
    assert rc == 0
    check_grads(f"{name} C ABI", outs, r64, bounds)
    a = backward_op(z, code, dy, gamma, mean, invstd, c["pool"])
    b = backward_op(z, code, dy, gamma, mean, invstd, c["pool"])
    for k in P.GRADS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], outs[k]), k
    assert a["dz"].dtype == BF and a["dz"].is_contiguous(memory_format=CL)
    assert a["dgamma"].dtype == a["dbeta"].dtype == torch.float32


# ---------------------------------------------------------------- 2. bitwise against the fp32 kernels
@pytest.mark.parametrize("name", CROSS_CASES)
def test_bitwise_the_fp32_backward_on_the_same_values(cuda, name):
    """Same bf16-valued z and dy, same codes, mean and invstd: the same thread-to-element map,
    partition and summation order, one rounding at the store of dz."""
    c, r64, _, _ = reference(name)
    z, code, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    got = backward_op(z, code, dy, gamma, mean, invstd, c["pool"])
    z32, dy32 = z.float(), dy.float()
    assert z32.is_contiguous(memory_format=CL) and torch.equal(z32.to(BF), z)
    want = {"dz": torch.full_like(z32, NAN), "dgamma": torch.full_like(mean, NAN), "dbeta": torch.full_like(mean, NAN)}
    assert capi_backward(z32, code, dy32, gamma, mean, invstd, c["pool"], want, fp32=True)[0] == 0
    assert torch.equal(got["dgamma"], want["dgamma"]) and torch.equal(got["dbeta"], want["dbeta"])
    assert torch.equal(got["dz"], want["dz"].to(BF))
    assert float(want["dz"].abs().max()) > 0


# ---------------------------------------------------------------- 3. the forward
@pytest.mark.parametrize("name", list(CASES))
def test_forward_is_batchnorm_act_bitwise_and_names_the_reference_argmax(cuda, name):
    c, r64, _, fbounds = reference(name)
    assert_margins(name, r64, c["pool"])
    z = c["z"].to(cuda, BF).contiguous(memory_format=CL)
    gamma, beta = c["gamma"].to(cuda), c["beta"].to(cuda)
    with torch.no_grad():
        want = features.batchnorm_act(z, fused_bn(c, cuda), c["relu"], pool=nn.MaxPool2d(*c["pool"]))
    assert want.dtype == BF
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
    check_f32(f"{name} forward", {"y": y, "mean": mean, "invstd": invstd}, r64, fbounds, ("mean", "invstd"), P.FWD)
    check_bf16(f"{name} forward y", y, r64["y"], fbounds["y"])
    assert torch.equal(code.cpu(), r64["code"])
    # the python entry point returns the same four tensors
    for s, t in zip(features.batchnorm_pool_stats_bf16(z, gamma, beta, P.EPS, c["relu"], *c["pool"]), got[0]):
        assert torch.equal(s, t) and s.shape == t.shape and s.dtype == t.dtype


# ---------------------------------------------------------------- 4. case coverage
def test_partition_has_at_least_four_blocks_with_a_ragged_last_one(cuda):
    N, C, H, W = CASES["blocks"][0]
    rows, rpp = N * H * W, PART // C
    assert C == 64 and rows // rpp >= 4 and rows % rpp != 0
    a = _lib.BnPoolGradBf16Args()
    a.batch, a.channels, a.height, a.width = N, C, H, W
    a.pool_kernel, a.pool_stride, a.pool_pad = 3, 2, 1
    a.pooled_height, a.pooled_width = P.pooled(H, 3, 2, 1), P.pooled(W, 3, 2, 1)
    n = ctypes.c_size_t()
    assert _lib.load().mcgmil_bn_pool_grad_workspace_size_bf16(ctypes.byref(a), ctypes.byref(n)) == 0
    assert n.value == ((4 * C + 2 * C * -(-rows // rpp)) * 4 + 255) // 256 * 256


def test_ties_go_to_the_first_tap(cuda):
    """Integer z: every window has exactly equal taps. The forward names the first of them in
    row-major order, and the backward sends the window's whole gradient there."""
    c, r64, bounds, _ = reference("ties")
    first, tied = PB.first_max_codes(r64["a"], c["pool"], c["relu"])
    print(f"ties: {tied} of {first.numel()} windows have more than one largest tap")
    assert tied >= first.numel() // 4 and torch.equal(first, r64["code"])
    z, _, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    _, _, _, code = features.batchnorm_pool_stats_bf16(z, gamma, c["beta"].to(cuda), P.EPS, True, *c["pool"])
    assert torch.equal(code.cpu(), first)
    check_grads("ties, the forward's own codes", backward_op(z, code, dy, gamma, mean, invstd, c["pool"]), r64, bounds)


def test_prepared_channels(cuda):
    """C = 8 and C = 2048 (the channel minimum and maximum), then C = 64 with channel 5 fully masked
    (every activation < 0) -> dgamma, dbeta and dz exactly 0, channel 9 with a negative gamma, and
    the whole layer with gamma = NULL."""
    assert CASES["clip"][0][1] == 8 and CASES["c2048"][0][1] == 2048      # both run in sections 1 and 3
    shape, pool, _, _, _ = CASES["odd"]
    c = P.make(shape, pool, 11, True)
    c["gamma"][9] = -1.25
    c["beta"][5] = -50.0
    c = PB.rounded(c)
    for label, cc in (("prepared", c), ("no gamma", dict(c, gamma=None, beta=None))):
        _, r64, r32, bounds, _ = PB.reference_of(cc)
        z, code, dy, gamma, mean, invstd = dev_inputs(cc, r64, cuda)
        ref = dict(r64)
        if gamma is None:                      # autograd has no dgamma / dbeta without parameters
            f = P.formula(cc["z"].double(), r64["code"], cc["dy"].double(), None, r64["mean"], r64["invstd"], pool)
            ref["dgamma"], ref["dbeta"] = f[1], f[2]
            e32 = P.formula(cc["z"], r32["code"], cc["dy"], None, r32["mean"], r32["invstd"], pool)
            bounds = R.bounds(R.errors(dict(r32, dgamma=e32[1], dbeta=e32[2]), ref, P.GRADS))
        got = backward_op(z, code, dy, gamma, mean, invstd, pool)
        again = backward_op(z, code, dy, gamma, mean, invstd, pool)
        assert all(torch.equal(got[k], again[k]) for k in P.GRADS)
        check_grads(label, got, ref, bounds)
        if gamma is not None:
            assert float(r64["y"][:, 5].abs().max()) == 0.0 and bool((r64["code"][:, 5] == P.NONE).all())
            assert float(got["dgamma"][5]) == 0.0 and float(got["dbeta"][5]) == 0.0
            assert float(got["dz"][:, 5].float().abs().max()) == 0.0
            assert float(c["gamma"][9]) < 0 and float(got["dz"][:, 9].float().abs().max()) > 0.0


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
    assert all(t is None for t in features.batchnorm_pool_backward_bf16(z, code, dy, gamma, mean, invstd, *c["pool"],
                                                                        need_dz=False, need_dw=False))


# ---------------------------------------------------------------- 5. validation
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
    assert L.mcgmil_bn_pool_grad_workspace_size_bf16(ctypes.byref(a), ctypes.byref(n)) == UNSUPPORTED
    assert call(pool=(4, 2, 1)) == UNSUPPORTED                                         # k = 4
    assert call(pool=(3, 2, 2)) == UNSUPPORTED                                         # pad > k / 2
    assert call(pool=(2, 3, 0)) == UNSUPPORTED                                         # stride > k
    assert call(outs={"dz": z}) == INVALID                                             # an output aliasing an input
    assert call(outs={"dz": outs["dz"], "dgamma": mean}) == INVALID
    assert call(outs={}) == INVALID                                                    # no output
    assert call(ws_bytes=255) == WORKSPACE                                             # too small a workspace
    assert call(dy=dy[:, :, :-1].contiguous(memory_format=CL)) == INVALID              # not this pool's dy
    assert call(mean=mean[1:]) == ALIGN                                                # misaligned mean
    assert len(L.mcgmil_last_error()) > 0
    a = grad_args(z, code, dy, gamma, mean, invstd, pool, outs)
    a.reserved = 1
    assert L.mcgmil_bn_pool_grad_workspace_size_bf16(ctypes.byref(a), ctypes.byref(n)) == INVALID
    # the forward
    beta = c["beta"].to(cuda)
    y, cd = torch.empty_like(dy), torch.empty_like(code)
    m, s = torch.empty_like(mean), torch.empty_like(mean)
    fwd = lambda zz=z, pl=pool, yy=y, mm=m, **over: capi_forward(zz, gamma, beta, True, pl, yy, mm, s, cd, **over)  # noqa: E731
    assert fwd() == 0
    assert fwd(pl=(4, 2, 1)) == UNSUPPORTED and fwd(pl=(3, 2, 2)) == UNSUPPORTED
    assert fwd(dtype=_lib.MCGMIL_F32) == UNSUPPORTED                                   # the fp32 entry point's
    assert fwd(mm=None) == INVALID                                                     # batch_mean is required
    assert fwd(running_mean=ctypes.c_void_p(m.data_ptr()), running_var=ctypes.c_void_p(s.data_ptr())) == INVALID
    assert fwd(residual=ctypes.c_void_p(z.data_ptr())) == UNSUPPORTED
    assert fwd(workspace_bytes=255) == WORKSPACE
    assert capi_forward(z, gamma, beta, True, pool, y, m, s, None) == INVALID          # no argmax
    # the python entry points refuse what the kernels do not implement
    with pytest.raises(ValueError):
        features.batchnorm_pool_stats_bf16(z, gamma, beta, P.EPS, True, 4, 2, 1)
    with pytest.raises(ValueError):
        features.batchnorm_pool_stats_bf16(z.contiguous(), gamma, beta, P.EPS, True, *pool)         # not channels-last
    with pytest.raises(ValueError):
        features.batchnorm_pool_stats_bf16(z.float(), gamma, beta, P.EPS, True, *pool)              # an fp32 z
    with pytest.raises(ValueError):
        features.batchnorm_pool_backward_bf16(z.contiguous(), code, dy, gamma, mean, invstd, *pool)
    with pytest.raises(ValueError):
        features.batchnorm_pool_backward_bf16(z.float(), code, dy.float(), gamma, mean, invstd, *pool)
    with pytest.raises(ValueError):
        features.batchnorm_pool_backward_bf16(z, code, dy[:, :, :-1].contiguous(memory_format=CL), gamma, mean, invstd, *pool)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. 64-bit offsets
def test_byte_offsets_past_2_to_31(cuda):
    """1,340 x 64 x 112 x 112 in bf16: z is 2.15 GB, and the last two images lie wholly past 2^31
    bytes. The float64 reference (with its window codes) and the fp32 bound both come from torch
    autograd on the GPU, on the bf16 values. The backward runs on the reference's codes; the
    forward's y is compared bitwise with batchnorm_act, and its codes with the reference's on the
    last image wherever the float64 reference is at least 1e-5 from zero and its two largest taps
    are equal or at least 1e-5 apart (4e6 windows cannot all keep that margin)."""
    N, pool = 1340, (3, 2, 1)
    shape = (N, 64, 112, 112)
    g = torch.Generator(device=cuda).manual_seed(7)
    z = (torch.randn(*shape, device=cuda, generator=g) + 0.5).to(BF).contiguous(memory_format=CL)
    dy = torch.randn(N, 64, 56, 56, device=cuda, generator=g).to(BF).contiguous(memory_format=CL)
    gamma = 0.5 + torch.rand(64, device=cuda, generator=g)
    beta = torch.zeros_like(gamma)
    assert z.numel() * 2 > 2 ** 31 and z[:N - 2].numel() * 2 >= 2 ** 31
    case = {"z": z, "dy": dy, "gamma": gamma, "beta": beta, "relu": True, "pool": pool}
    r64 = P.autograd(case, torch.float64, cuda)
    code = P.codes(r64.pop("idx"), r64["y"], shape[3], pool, True).contiguous(memory_format=CL)
    a_last = r64.pop("a")[N - 1:].clone()
    del r64["y"]
    r32 = {k: v for k, v in P.autograd(case, torch.float32, cuda).items() if k in P.GRADS}
    bounds = R.bounds(R.errors(r32, r64, P.GRADS))
    del r32
    mean, invstd = r64["mean"].float(), r64["invstd"].float()
    a = backward_op(z, code, dy, gamma, mean, invstd, pool)
    check_f32("2.15 GB", a, r64, bounds, ("dgamma", "dbeta"), P.GRADS)
    rdz = r64["dz"]
    top, B, excess = rdz.abs().max(), bounds["dz"], 0.0
    for i in range(0, N, 134):                 # 10 chunks
        ref = rdz[i:i + 134]
        d = (a["dz"][i:i + 134].double() - ref).abs()
        excess = max(excess, float((d / (2.0 ** -7 * ref.abs() + B * top)).max()))
    print(f"2.15 GB dz: max |d| / (2^-7 |ref| + {B:.1e} max|ref|) = {excess:.3f} / 1")
    assert excess <= 1.0
    del r64, rdz, ref, d
    b = backward_op(z, code, dy, gamma, mean, invstd, pool)
    for k in P.GRADS:
        assert torch.equal(a[k], b[k]), k
    del a, b, dy
    y, _, _, got = features.batchnorm_pool_stats_bf16(z, gamma, beta, P.EPS, True, *pool)
    with torch.no_grad():
        want = features.batchnorm_act(z, fused_bn(case, cuda), True, pool=nn.MaxPool2d(*pool))
    assert torch.equal(y, want)
    del y, want
    win = F.unfold(F.pad(a_last, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(1, 64, 9, 56, 56)
    top = win.topk(2, dim=2).values
    gap = top[:, :, 0] - top[:, :, 1]
    safe = ((gap == 0) | (gap >= 1e-5)) & (top[:, :, 0].abs() >= 1e-5)
    print(f"last image: {int(safe.sum())} of {safe.numel()} windows at least 1e-5 from a near-tie and from zero")
    assert int(safe.sum()) > 0.99 * safe.numel()
    assert torch.equal(got[N - 1:][safe], code[N - 1:][safe])
    del z, code, got, win, top, gap, safe, a_last
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 7. the differentiable op
def test_opcheck(cuda):
    c, r64, _, _ = reference("odd")
    z, code, dy, gamma, mean, invstd = dev_inputs(c, r64, cuda)
    beta = c["beta"].to(cuda)
    rq = lambda t: t.clone().requires_grad_()  # noqa: E731
    torch.library.opcheck(torch.ops.mcgmil.bn_pool_bf16.default, (rq(z), rq(gamma), rq(beta), P.EPS, True, 3, 2, 1))
    torch.library.opcheck(torch.ops.mcgmil.bn_pool_bf16.default, (rq(z), None, None, P.EPS, False, 2, 2, 0))
    torch.library.opcheck(torch.ops.mcgmil.bn_pool_bf16_backward.default,
                          (z, code, dy, gamma, mean, invstd, 3, 2, 1, True, True))
    torch.library.opcheck(torch.ops.mcgmil.bn_pool_bf16_backward.default,
                          (z, code, dy, None, mean, invstd, 3, 2, 1, True, False))


# ---------------------------------------------------------------- 8. the op's forward and autograd
@pytest.mark.parametrize("name", OP_CASES)
def test_op_forward_and_autograd_match_float64(cuda, name):
    c, r64, bounds, fbounds = reference(name)
    assert_margins(name, r64, c["pool"])
    rq = lambda t, dt=None: t.to(cuda, dt).requires_grad_()  # noqa: E731
    z, gamma, beta = rq(c["z"], BF), rq(c["gamma"]), rq(c["beta"])            # z not channels-last: made so
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y, mean, invstd, code = torch.ops.mcgmil.bn_pool_bf16(z, gamma, beta, P.EPS, c["relu"], *c["pool"])
    assert y.shape == r64["y"].shape == code.shape and y.dtype == BF and y.is_contiguous(memory_format=CL)
    assert code.dtype == torch.uint8 and not code.requires_grad and mean.shape == invstd.shape == (z.shape[1],)
    assert mean.dtype == invstd.dtype == torch.float32
    # saved for the backward: z, the codes, mean, invstd and weight -- no activation of z's size, no int64
    kinds = sorted((str(t.dtype), tuple(t.shape)) for t in saved)
    C = z.shape[1]
    assert kinds == sorted([("torch.bfloat16", tuple(z.shape)), ("torch.uint8", tuple(code.shape)),
                            ("torch.float32", (C,)), ("torch.float32", (C,)), ("torch.float32", (C,))]), kinds
    check_f32(f"{name} forward", {"y": y.detach(), "mean": mean.detach(), "invstd": invstd.detach()}, r64, fbounds,
              ("mean", "invstd"), P.FWD)
    check_bf16(f"{name} forward y", y.detach(), r64["y"], fbounds["y"])
    assert torch.equal(code.cpu(), r64["code"])
    # gradients flowing into mean / invstd are ignored: the loss below uses them on purpose
    dy = c["dy"].to(cuda, BF)
    (y.float() * dy.float()).sum().add(mean.sum() + invstd.sum()).backward()
    got = {"dz": z.grad, "dgamma": gamma.grad, "dbeta": beta.grad}
    assert z.grad.dtype == BF and gamma.grad.dtype == beta.grad.dtype == torch.float32
    check_grads(f"{name} autograd", got, r64, bounds)
    # a backward of the backward raises
    z2 = rq(c["z"], BF)
    y2, _, _, code2 = torch.ops.mcgmil.bn_pool_bf16(z2, gamma, beta, P.EPS, c["relu"], *c["pool"])
    assert torch.equal(y2, y) and torch.equal(code2, code)
    (dz,) = torch.autograd.grad(y2.float().sum(), z2, create_graph=True)
    with pytest.raises(RuntimeError):
        dz.float().sum().backward()
    with pytest.raises((RuntimeError, ValueError)):
        torch.ops.mcgmil.bn_pool_bf16(c["z"].to(BF), None, None, P.EPS, True, *c["pool"])       # no CPU kernel


# ---------------------------------------------------------------- 9. routing
def _spies(monkeypatch):
    """Call logs of (bn_pool_bf16_op, batchnorm_pool_backward_bf16, bn_act_bf16_op, bn_pool_f32_op)."""
    logs = {}
    for name in ("bn_pool_bf16_op", "batchnorm_pool_backward_bf16", "bn_act_bf16_op", "bn_pool_f32_op"):
        log, real = logs.setdefault(name, []), getattr(features, name)
        monkeypatch.setattr(features, name, lambda first, *a, _l=log, _r=real, **k: _l.append(first) or _r(first, *a, **k))
    return logs["bn_pool_bf16_op"], logs["batchnorm_pool_backward_bf16"], logs["bn_act_bf16_op"], logs["bn_pool_f32_op"]


def test_bn_act_routes_inside_the_context_only(cuda, monkeypatch):
    routed, _, routed_act, routed32 = _spies(monkeypatch)
    bn = nn.BatchNorm2d(64).to(cuda)
    deactivate_batchnorm(bn)
    pool = nn.MaxPool2d(3, 2, 1)
    x = torch.randn(3, 64, 9, 7, device=cuda).to(BF).requires_grad_()      # not channels-last: made so
    want = pool(torch.relu(bn(x.float())))
    assert features.bn_pool_bf16_trainable(x, bn, pool) and not features.bn_pool_trainable(x, bn, pool)
    y0 = features.bn_act(bn, x, True, pool=pool)
    assert not routed and y0.dtype == BF
    with features.native_stem_training(), features.native_norm_bf16_training(), features.native_norm_training():
        y2 = features.bn_act(bn, x, True, pool=pool)          # the other contexts: a bf16 pool layer stays on torch
    assert not routed and not routed32 and not routed_act and torch.equal(y2, y0)
    with features.native_stem_bf16_training():
        y1 = features.bn_act(bn, x, True, pool=pool)
        assert len(routed) == 1
        with torch.no_grad():
            features.bn_act(bn, x, True, pool=pool)
        features.bn_act(bn, x, True)                                        # no pool
        features.bn_act(bn, x, True, x)                                     # a residual, no pool
        features.bn_act(bn, x, True, pool=nn.MaxPool2d(5, 2, 2))            # a pool outside the geometry
        features.bn_act(bn, x, True, pool=nn.MaxPool2d(3, 2, 1, ceil_mode=True))
        tracking = nn.BatchNorm2d(64).to(cuda)
        features.bn_act(tracking, x, True, pool=pool)                       # pending running-stat update
        assert len(routed) == 1 and float(tracking.running_mean.abs().max()) > 0
        x32 = x.detach().float().requires_grad_()
        features.bn_act(bn, x32, True, pool=pool)                           # an fp32 activation
        assert len(routed) == 1 and not routed32 and not routed_act
    with features.native_stem_bf16_training(False):
        features.bn_act(bn, x, True, pool=pool)
    assert len(routed) == 1
    # one bf16 rounding of values of order 1
    assert y1.dtype == BF and torch.allclose(y1.float(), want, atol=2.0 ** -6, rtol=2.0 ** -6)
    y1.float().sum().backward()
    assert x.grad is not None and x.grad.dtype == BF and bool(torch.isfinite(x.grad.float()).all())
    assert bn.weight.grad is not None and bn.weight.grad.dtype == torch.float32


# ---------------------------------------------------------------- 10. the module
@pytest.mark.parametrize("route", ["native", None])
def test_module_train_step_with_the_stem_opt_in(cuda, route, monkeypatch):
    """The rule of test_gpu_bn_grad_bf16.test_module_train_step_with_the_norm_opt_in: every gradient's
    drift from the fp32 step is <= 2 x the drift of autocast over the torch layers + 1e-3.

    Measured on an MI355X: every gradient but one sits at <= 0.84 of its bound. attention_weights.1.bias
    (one scalar, -0.0388 in fp32) drifts 0.0896 with this opt-in, the same figure in every run and on
    both routes; (e), the norm opt-in alone, drifts 0.0486 there, and (h), the stem opt-in alone,
    0.138. The yardstick is not repeatable: autocast's own step gave 0.029, 0.038, 0.041, 0.042, 0.043,
    0.046 and 0.047 for that scalar over seven runs (aten's bf16 convolution backward is not bitwise
    repeatable), so the bound moved between 0.058 and 0.095. Run alone, this test passed at 0.943 of
    the bound; within the whole suite it FAILED twice, at 1.16 and 1.07 (bounds 0.077 and 0.084). The
    stem's backward does not reach that scalar; only the forward does, and the op's y is the correctly rounded value (bitwise
    mcgmil_batchnorm_act's, as required), where torch's autocast layers differ from it by one bf16 ulp
    in 109,362 of the 221,184 pooled elements of this case. Over eight other random bags the rule
    itself is exceeded by (e) on three, by this opt-in on two and by (h) on three (worst ratios 2.75,
    1.68 and 4.24), so the miss is the yardstick's noise on this one case, not a defect found in the
    op. The bound stays as the rule states it."""
    if route:
        monkeypatch.setenv("MCGMIL_CONV_GRAD", route)
    else:
        monkeypatch.delenv("MCGMIL_CONV_GRAD", raising=False)
    m0, x, target, seed, g32, gac, _ = CB.module_case()
    routed, backwards, routed_act, _ = _spies(monkeypatch)
    pools = []
    real_pool = F.max_pool2d
    monkeypatch.setattr(F, "max_pool2d", lambda *a, **k: pools.append(1) or real_pool(*a, **k))
    m = copy.deepcopy(m0)
    assert m.enable_bf16_backbone_training().enable_bf16_norm_training().enable_bf16_stem_training() is m
    grads, _, _ = CB._step(m, x, target, seed)
    assert routed == [m.feature_extractor.bn1] and len(backwards) == 1 and not pools
    assert len(routed_act) == 19 and len(set(map(id, routed_act))) == 19 and m.feature_extractor.bn1 not in routed_act
    scale = max(float(g.abs().max()) for g in g32.values())
    rows = []
    for n, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any()), n
        assert g.dtype == torch.float32, n
        err, yard = CB._drift(g, g32[n], scale), CB._drift(gac[n], g32[n], scale)
        bound = 2.0 * yard + 1e-3
        rows.append((n, err, bound))
        print(f"route={route} norm+stem {n}: {err:.2e} / {bound:.2e} (autocast over the torch layers: {yard:.2e})")
    for n, err, bound in rows:
        assert err <= bound, (n, err, bound)
    print(f"route={route} norm+stem: worst drift / bound = {max(e / b for _, e, b in rows):.3f}")
    # it depends on neither enable_bf16_norm_training() nor the route: alone, the stem only
    del routed[:], backwards[:], routed_act[:]
    m = copy.deepcopy(m0).enable_bf16_backbone_training().enable_bf16_stem_training()
    CB._step(m, x, target, seed)
    assert routed == [m.feature_extractor.bn1] and len(backwards) == 1 and not routed_act and not pools


def test_module_without_the_flag_routes_no_stem(cuda, monkeypatch):
    m0, x, target, seed, _, _, _ = CB.module_case()
    routed, backwards, _, _ = _spies(monkeypatch)
    off = copy.deepcopy(m0).enable_bf16_backbone_training().enable_bf16_stem_training().enable_bf16_backbone_training(False)
    for mm in (copy.deepcopy(m0).enable_bf16_backbone_training(),                          # without the flag
               copy.deepcopy(m0).enable_bf16_backbone_training().enable_bf16_norm_training(),
               copy.deepcopy(m0).enable_bf16_backbone_training().enable_bf16_stem_training(False),
               copy.deepcopy(m0).enable_bf16_stem_training(),       # the flag without the one it sits on: fp32
               copy.deepcopy(m0).enable_backbone_training(stem=True).enable_bf16_stem_training(),
               off, copy.deepcopy(off).enable_bf16_backbone_training()):
        CB._step(mm, x, target, seed)
        assert routed == [] and backwards == []


def test_module_eval_and_no_grad_are_unchanged(cuda, monkeypatch):
    m0, x, target, seed, _, _, _ = CB.module_case()
    routed, _, _, _ = _spies(monkeypatch)
    never = copy.deepcopy(m0).eval()
    flagged = copy.deepcopy(m0).enable_bf16_backbone_training().enable_bf16_norm_training() \
        .enable_bf16_stem_training().eval()
    Ye, Ae, _ = never(x, target)
    Yf, Af, _ = flagged(x, target)
    assert routed == [] and torch.equal(Yf, Ye) and torch.equal(Af, Ae)
    with torch.no_grad():
        Yn, An, _ = flagged(x, target)
        Ym, Am, _ = never(x, target)
    assert routed == [] and torch.equal(Yn, Ym) and torch.equal(An, Am)
    with torch.no_grad():
        flagged.train()(x, target)              # train mode under no_grad: the inference path
    assert routed == []
