"""The HIP backward pass of the MIL head (include/mcgmil_grad.h, ops.mcdo_backward, the autograd
formula of torch.ops.mcgmil.mcdo_forward, MultiHeadGatedAttentionMIL.enable_head_training)
against the float64 restatement tests/head_grad_ref.py fed the kernel's own masks
(ops.feature_keep / ops.attention_keep).

Error of tensor k: max|got - ref| / max(max|ref_k|, 1e-3 max_j max|ref_j|) over the case's
gradients j. Bound of tensor k: 10 x the same error of the restatement evaluated in fp32 on the
CPU for that case (the project's x10 for a changed summation order), at least 1e-6."""
import copy
import functools

import numpy as np
import pytest
import torch

import golden_util
import head_grad_ref as ref
import head_regimes as hr
from mcgmil import MultiHeadGatedAttentionMIL, _lib, ops, synthetic

pytestmark = pytest.mark.gpu

GRAN = _lib.GRAD_GRANULE_ROWS
TILE = 32                       # rows of a grad_rows_kernel tile at L = 512, D = 128, C = 2
# one bag over three split-K granules, the last one ragged, and a ragged last row tile
N_SPLITK = 2 * GRAN + 2 * TILE + 12

PLAIN = (1, 1, 1)               # torch's default init: gates in their linear part, flat attention
CASES = {
    #           sizes              T  C  D    shared p_f  p_a  t_base bag_ids  (gv, gu, ga)  features
    "n1":      ((1,),              1, 2, 128, False, 0.1, 0.1, 0, None, PLAIN, "relu"),
    "n37":     ((37,),             1, 2, 128, True,  0.1, 0.1, 0, None, PLAIN, "relu"),
    "n130":    ((130,),            2, 3, 64,  False, 0.1, 0.1, 0, None, PLAIN, "relu"),
    "ragged":  ((1, 70, 129, 16),  3, 2, 128, False, 0.1, 0.1, 5, (7, 3, 11, 5), PLAIN, "relu"),
    "p0":      ((70,),             2, 2, 128, False, 0.0, 0.0, 0, None, PLAIN, "relu"),
    "p05":     ((70,),             2, 2, 128, True,  0.5, 0.5, 0, None, PLAIN, "relu"),
    "splitk":  ((N_SPLITK,),       2, 2, 128, False, 0.1, 0.1, 0, None, PLAIN, "relu"),
    # tests/head_regimes.py: peaked attention and gates out of their linear part, where the gate
    # gradients weigh against dwk (float64: max|dWv| 1.5, max|dWu| 0.45 against max|dwk| 3.8 in
    # "trained", 2.9 and 1.1 against 8.5 in "trained_ragged"; 0.03 against 1.07 in the cases above)
    "trained": ((70,),             2, 2, 128, False, 0.1, 0.1, 0, None, hr.REGIMES["trained"], "relu"),
    "trained_ragged": ((1, 70, 129, 16), 3, 2, 128, False, 0.1, 0.1, 5, (7, 3, 11, 5),
                       hr.REGIMES["trained"], "signed_sparse"),
    "saturated_peaked": ((70,),    2, 2, 128, True,  0.1, 0.1, 0, None, hr.REGIMES["saturated_peaked"], "relu"),
}
SEED = 0x1234567890ABCDEF


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(name, dev_index=0):
    """Inputs, the forward call's A and Y, the kernel's masks, and the float64 / fp32 CPU
    reference gradients for loss = sum(Y dY) + sum(A dA): computed once, never modified."""
    sizes, T, C, D, shared, p_f, p_a, t_base, bag_ids, gains, kind = CASES[name]
    dev = torch.device("cuda", dev_index)
    c = Case()
    c.name, c.sizes, c.T, c.C, c.D, c.shared, c.p_f, c.p_a, c.t_base = name, sizes, T, C, D, shared, p_f, p_a, t_base
    L, R, B = 512, sum(sizes), len(sizes)
    c.Hn = np.concatenate([hr.features(kind, 100 + b, n, L) for b, n in enumerate(sizes)])
    sd = hr.scale_state_dict(synthetic.head_state_dict(77, L=L, D=D, C=C, shared=shared), *gains)
    arrays = synthetic.head_arrays(sd, C, shared)
    c.params = [np.ascontiguousarray(arrays[k]) for k in ref.PARAMS]
    c.head = ops.HeadTensors(*[torch.from_numpy(a).to(dev) for a in c.params])
    c.H = torch.from_numpy(c.Hn).to(dev)
    c.offs = ops.bag_offsets_tensor(list(sizes), dev)
    c.bag_ids = None if bag_ids is None else torch.tensor(bag_ids, dtype=torch.int32, device=dev)
    c.kw = dict(p_feat=p_f, p_att=p_a, seed=SEED, t_base=t_base, bag_ids=c.bag_ids)
    fwd = ops.mcdo_forward(c.H, c.offs, c.head, T, **c.kw)
    c.Y, c.A = fwd["Y"], fwd["A"]
    rng = np.random.Generator(np.random.PCG64(5))
    c.dYn = rng.standard_normal((B, T, C)).astype(np.float32)
    c.dAn = rng.standard_normal(T * C * R).astype(np.float32)
    c.dY, c.dA = torch.from_numpy(c.dYn).to(dev), torch.from_numpy(c.dAn).to(dev)
    kf = ops.feature_keep(c.offs, R, T, L, p_f, SEED, t_base=t_base, bag_ids=c.bag_ids).cpu().numpy()
    ka = ops.attention_keep(c.offs, R, T, C, p_a, SEED, t_base=t_base, bag_ids=c.bag_ids).cpu().numpy()
    c.keepF, c.keepA, c.dA_bags, o = [], [], [], 0
    for n in sizes:
        c.keepF.append(np.unpackbits(kf[T * o:T * (o + n)], axis=1, bitorder="little").reshape(T, n, L))
        c.keepA.append(ka[T * C * o:T * C * (o + n)].reshape(T, C, n))
        c.dA_bags.append(c.dAn[T * C * o:T * C * (o + n)].reshape(T, C, n))
        o += n
    return c


@functools.lru_cache(maxsize=None)
def reference(name, with_dA=True):
    """(float64 gradients, per-tensor bounds) of a case."""
    c = case(name)
    args = (c.Hn, c.sizes, c.params, c.keepF, c.keepA, c.p_f, c.p_a, c.dYn, c.dA_bags if with_dA else None)
    g64, Ys, As = ref.batch_grads(*args, torch.float64)
    g32, _, _ = ref.batch_grads(*args, torch.float32)
    bounds = {k: max(10.0 * e, 1e-6) for k, e in ref.grad_errors(g32, g64).items()}
    return g64, bounds, Ys, As


def backward(c, with_dA=True, **kw):
    g = ops.mcdo_backward(c.H, c.offs, c.head, c.T, c.A, c.Y, c.dY, c.dA if with_dA else None, **c.kw, **kw)
    torch.cuda.synchronize()
    return g


def check(label, got, g64, bounds):
    err = ref.grad_errors({k: v.detach().cpu().numpy() for k, v in got.items()}, g64)
    print(label, {k: f"{e:.1e}/{bounds[k]:.1e}" for k, e in err.items()})
    bad = {k: (e, bounds[k]) for k, e in err.items() if not e <= bounds[k]}
    assert not bad, (label, bad)
    return err


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_dA(cuda, name):
    c = case(name)
    g64, bounds, Ys, _ = reference(name)
    # the forward call the gradients belong to is the restatement's
    Yr = np.stack([y.numpy() for y in Ys])
    assert np.max(np.abs(c.Y.cpu().numpy() - Yr)) <= 1e-5 * max(1.0, np.max(np.abs(Yr)))
    pre = {k: torch.full_like(t, float("nan")) for k, t in
           list(zip(ops.GRAD_NAMES, c.head)) + [("dH", c.H)]}
    got = backward(c, out=pre)
    assert all(got[k] is pre[k] for k in pre)          # overwritten, not accumulated
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    check(name, got, g64, bounds)
    # dH is exactly 0 wherever the feature was dropped in every sample: the regenerated mask is
    # the forward's
    o = 0
    for b, n in enumerate(c.sizes):
        never = ~c.keepF[b].astype(bool).any(0)
        assert not got["dH"][o:o + n].cpu().numpy()[never].any()
        o += n
    if c.p_f > 0:
        assert sum(int((~k.astype(bool).any(0)).sum()) for k in c.keepF) > 0
    # bitwise repeatable
    again = backward(c)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_one_instance_bag_gate_gradients_are_exactly_zero(cuda):
    got = backward(case("n1"))
    for k in ("dWv", "dbv", "dWu", "dbu", "dwa", "dba"):
        assert not bool(got[k].any()), k
    assert bool(got["dwk"].any()) and bool(got["dH"].any())


def test_no_dA_no_dH_and_output_subsets(cuda):
    c = case("ragged")
    g64, bounds, _, _ = reference("ragged", with_dA=False)
    full = backward(c, with_dA=False)
    check("ragged dA=None", full, g64, bounds)
    part = backward(c, with_dA=False, need_dH=False, outputs=("dwa", "dWu", "dwk"))
    assert sorted(part) == ["dWu", "dwa", "dwk"]
    assert all(torch.equal(part[k], full[k]) for k in part)
    only_dH = backward(c, with_dA=False, outputs=())
    assert list(only_dH) == ["dH"] and torch.equal(only_dH["dH"], full["dH"])


def test_T3_is_the_sum_of_three_single_sample_calls(cuda):
    c = case("ragged")
    g64, bounds, _, _ = reference("ragged")
    C, T = c.C, c.T
    total = None
    for t in range(T):
        # sample t of every bag: A is per bag [T, C, N_b], Y is [B, T, C]
        At, dAt, o = [], [], 0
        for n in c.sizes:
            blk = slice(T * C * o + t * C * n, T * C * o + (t + 1) * C * n)
            At.append(c.A[blk])
            dAt.append(c.dA[blk])
            o += n
        kw = dict(c.kw, t_base=c.t_base + t)
        g = ops.mcdo_backward(c.H, c.offs, c.head, 1, torch.cat(At), c.Y[:, t:t + 1].contiguous(),
                              c.dY[:, t:t + 1].contiguous(), torch.cat(dAt), **kw)
        total = g if total is None else {k: total[k] + g[k] for k in g}
    torch.cuda.synchronize()
    check("ragged sum of T=1 calls", total, g64, bounds)


def test_forced_chunking_is_bitwise_the_unchunked_result(cuda):
    c = case("splitk")
    assert N_SPLITK > 2 * GRAN and N_SPLITK % GRAN and N_SPLITK % TILE
    whole = backward(c)
    chunked = backward(c, chunk_pairs=c.T * GRAN)           # one granule per launch chunk: three chunks
    assert all(torch.equal(whole[k], chunked[k]) for k in whole)


def test_validation_errors(cuda):
    c = case("n37")
    with pytest.raises(ValueError):
        ops.mcdo_backward(c.H.bfloat16(), c.offs, c.head, c.T, c.A, c.Y, c.dY, None, **c.kw)
    g = _lib.GradArgs()
    g.fwd = ops.make_args(c.H, c.offs, c.head, c.T, c.C, c.head.G, c.D, c.p_f, c.p_a, SEED)
    g.fwd.h_dtype = _lib.MCGMIL_BF16
    n = __import__("ctypes").c_size_t()
    lib = _lib.load()
    assert lib.mcgmil_grad_workspace_size(g, n) == -2                      # MCGMIL_E_UNSUPPORTED
    g.fwd.h_dtype = _lib.MCGMIL_F32
    assert lib.mcgmil_grad_workspace_size(g, n) == 0 and n.value > 0
    g.A, g.Y, g.dY = c.A.data_ptr(), c.Y.data_ptr(), c.dY.data_ptr()
    assert lib.mcgmil_head_backward(g, None) == -4                         # MCGMIL_E_WORKSPACE
    assert b"workspace" in lib.mcgmil_last_error()


# ------------------------------------------------------------------------------------ autograd
def _op_inputs(c, requires_grad=True):
    H = c.H.clone().requires_grad_(requires_grad)
    params = [t.clone().requires_grad_(requires_grad) for t in c.head]
    return H, params


def test_op_autograd_matches_restatement(cuda):
    from mcgmil import library  # noqa: F401
    c = case("p05")
    g64, bounds, _, _ = reference("p05")
    H, params = _op_inputs(c)
    seed = SEED - 2**64 if SEED >= 2**63 else SEED
    Y, A = torch.ops.mcgmil.mcdo_forward(H, c.offs, *params, c.T, c.p_f, c.p_a, seed, 0, c.t_base)
    assert torch.equal(Y, c.Y) and torch.equal(A, c.A)
    loss = (Y * c.dY).sum() + (A * c.dA).sum()
    loss.backward(create_graph=True)
    got = {"dH": H.grad}
    got.update({"d" + k: p.grad for k, p in zip(ref.PARAMS, params)})
    check("op autograd p05", got, g64, bounds)
    # a backward of the backward is not provided
    with pytest.raises(RuntimeError):
        H.grad.sum().backward()


def test_opcheck(cuda):
    from mcgmil import library  # noqa: F401
    c = case("n37")
    H, params = _op_inputs(c)
    fwd_args = (H, c.offs, *params, c.T, c.p_f, c.p_a, 1234, 0, 0)
    torch.library.opcheck(torch.ops.mcgmil.mcdo_forward.default, fwd_args)
    Hn, pn = _op_inputs(c, requires_grad=False)
    out = ops.mcdo_forward(Hn, c.offs, c.head, c.T, p_feat=c.p_f, p_att=c.p_a, seed=1234)
    for dA, need_dH in ((c.dA, True), (None, False)):
        torch.library.opcheck(torch.ops.mcgmil.mcdo_backward.default,
                              (Hn, c.offs, *pn, out["A"], out["Y"], c.dY, dA, c.T, c.p_f, c.p_a, 1234,
                               0, 0, need_dH))


# ------------------------------------------------------------------------------------ module
class _Flatten(torch.nn.Module):
    """Stand-in backbone for fixture inputs: x [N, 512, 1, 1] -> H [N, 512]."""
    fc = None

    def forward(self, x):
        return torch.flatten(x, 1)


def _module_for(c, dev):
    _, sd, _ = c.inputs()
    m = MultiHeadGatedAttentionMIL(num_classes=c.C, pretrained=False, D=c.D, feature_dropout=c.p_f,
                                   attention_dropout=c.p_a, shared_attention=c.shared)
    own = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(v).reshape(own[k].shape) for k, v in sd.items()}, strict=False)
    m.feature_extractor = _Flatten()
    return m.to(dev)


def _module_grads(m, shared):
    lv, lu = m._gate_linears()
    return {"dWv": torch.stack([q.weight.grad for q in lv]), "dbv": torch.stack([q.bias.grad for q in lv]),
            "dWu": torch.stack([q.weight.grad for q in lu]), "dbu": torch.stack([q.bias.grad for q in lu]),
            "dwa": torch.cat([q.weight.grad for q in m.attention_weights]),
            "dba": torch.cat([q.bias.grad for q in m.attention_weights]),
            "dwk": torch.cat([q.weight.grad for q in m.classifiers])}


@pytest.mark.parametrize("name", ["grad_N64_sep_t0", "grad_N37_shared"])
def test_module_training_step_matches_reference_fixture(cuda, name):
    import test_head_grad_ref as cpu
    c = cpu.load(name)
    m = _module_for(c, cuda)
    x = torch.from_numpy(c.inputs()[0]).to(cuda).view(1, c.N, c.L, 1, 1).requires_grad_(True)
    target = torch.tensor([c.target], device=cuda)
    m.train()
    with pytest.raises(NotImplementedError):          # opt-in only
        m(x, target)
    assert m.enable_head_training() is m
    Y, A, aux = m(x, target, seed=c.mask_seed)
    assert Y.shape == (1, c.C) and A.shape == (1, c.C, c.N)
    loss = torch.nn.functional.cross_entropy(Y, target) + aux
    loss.backward()
    got = _module_grads(m, c.shared)
    got["dH"] = x.grad.view(c.N, c.L)
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in got.items()}
    # bounds: the fp32 CPU restatement of this very loss against its float64 run
    g = {}
    for dt in (torch.float64, torch.float32):
        l, _, leaves = cpu.restated_loss(c, dt)
        l.backward()
        g[dt] = {k: t.grad.double().numpy() for k, t in zip(ref.GRADS, leaves)}
    bounds = {k: max(10.0 * e, 1e-6) for k, e in ref.grad_errors(g[torch.float32], g[torch.float64]).items()}
    assert abs(loss.item() - float(c.z["loss"].item())) <= 1e-5
    # against the reference fixture (what it stores of each gradient; same error form) ...
    views = cpu.stored_views(got)
    top = max(float(np.max(np.abs(c.z[k]))) for k in views)
    for k, v in views.items():
        want = c.z[k].astype(np.float64)
        e = float(np.max(np.abs(v - want))) / max(float(np.max(np.abs(want))), 1e-3 * top)
        b = bounds[k.split("_")[0]]
        print(name, k, f"{e:.1e}/{b:.1e}")
        assert e <= b, (k, e, b)
    # ... and against the float64 restatement, every element
    check(name + " module", {k: torch.from_numpy(v) for k, v in got.items()}, g[torch.float64], bounds)
    m.enable_head_training(False)
    with pytest.raises(NotImplementedError):
        m(x, target)


def test_sgd_step_through_the_backbone(cuda):
    torch.manual_seed(3)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(cuda)
    m.train().enable_head_training()
    x = torch.rand(1, 3, 3, 64, 64, device=cuda)
    target = torch.tensor([1], device=cuda)
    seed = 99
    pf, pa = m._dropout_ps()
    offs = ops.bag_offsets_tensor([3], cuda)
    keepF = torch.from_numpy(np.unpackbits(ops.feature_keep(offs, 3, 1, 512, pf, seed).cpu().numpy(), axis=1,
                                           bitorder="little").reshape(1, 3, 512))
    keepA = ops.attention_keep(offs, 3, 1, 2, pa, seed).cpu().view(1, 2, 3)

    def torch_loss(mod, xx, dev):
        """The same step with the head restated in torch (same masks), in mod's dtype."""
        H = mod.extract_features(xx)[0]
        params = mod._live_head()
        Y, A = ref.head_forward(H, params, keepF.to(dev), keepA.to(dev), pf, pa)
        return torch.nn.functional.cross_entropy(Y, target.to(dev)) + \
            mod.auxiliary_loss.scale * mod.auxiliary_loss(A[:, 1, :], A[:, 0, :], True)

    m64 = copy.deepcopy(m).double().cpu()
    m32 = copy.deepcopy(m).cpu()
    torch_loss(m64, x.double().cpu(), "cpu").backward()
    torch_loss(m32, x.cpu(), "cpu").backward()
    g64 = m64.feature_extractor.conv1.weight.grad.numpy()
    g32 = m32.feature_extractor.conv1.weight.grad.double().numpy()
    bound = max(10.0 * golden_util.nrel(g32, g64), 1e-6)

    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    before = m.attention_weights[0].weight.detach().clone()
    Y, A, aux = m(x, target, seed=seed)
    (torch.nn.functional.cross_entropy(Y, target) + aux).backward()
    g = m.feature_extractor.conv1.weight.grad
    assert bool(torch.isfinite(g).all()) and bool(g.any())
    err = golden_util.nrel(g.cpu().numpy(), g64)
    print(f"conv1.weight.grad: {err:.1e} / {bound:.1e}")
    assert err <= bound
    # the cached head tensors follow the optimizer: the next inference sees the new weights
    old_head, _ = m.head_tensors(cuda)
    old_wa = old_head.wa.clone()
    opt.step()
    assert not torch.equal(before, m.attention_weights[0].weight)
    m.eval()
    head, _ = m.head_tensors(cuda)
    assert torch.equal(head.wa[0], m.attention_weights[0].weight[0]) and not torch.equal(head.wa, old_wa)
    with torch.no_grad():
        H = m.extract_features(x)
        Yi, _ = m.mc_inference_features(H, T=1, p_feat=0.0, p_att=0.0)
        ones = torch.ones(1, 3, 512, dtype=torch.uint8), torch.ones(1, 2, 3, dtype=torch.uint8)
        Yr, _ = ref.head_forward(H[0].double().cpu(), [p.detach().double().cpu() for p in m._live_head()],
                                 ones[0], ones[1], 0.0, 0.0)
    assert np.max(np.abs(Yi[0, 0].cpu().numpy() - Yr[0].numpy())) <= 1e-5
