"""The MIL head's kernels where their arithmetic is exercised, not only their shapes
(tests/head_regimes.py): saturated gates, peaked attention, row-strided features, dropout
thresholds next to 0, 0x8000 and 0xFFFF, and Philox counters at the ends of their ranges.

Forward outputs are compared with the float64 oracle (oracle/mcdo_ref.py) on the kernel's own
operands and masks. Errors eA, eY, eL and their bounds are defined in tests/head_regimes.py: 10 x
the float32 CPU oracle's error against float64 for the same case, at least 1e-6, x 10 for bf16.

Measured on an MI355X, test_forward_matches_float64_oracle: per regime and dtype the case closest
to its bound, as error / bound (the largest ratio over the two feature kinds and five heads):

  regime            dtype  eA               eY               eL
  saturated         fp32   1.6e-06/1.1e-05  3.4e-07/1.6e-06  5.0e-06/2.5e-05
  saturated         bf16   4.5e-07/3.9e-05  1.0e-07/1.0e-05  6.7e-07/8.5e-05
  peaked            fp32   1.9e-06/8.8e-06  1.3e-06/6.9e-06  1.4e-05/9.1e-05
  peaked            bf16   2.0e-06/9.4e-05  1.1e-06/5.1e-05  1.1e-05/8.7e-04
  trained           fp32   2.8e-06/1.1e-05  1.7e-06/6.8e-06  1.5e-05/1.1e-04
  trained           bf16   1.2e-06/8.7e-05  5.3e-07/5.3e-05  8.0e-06/6.7e-04
  saturated_peaked  fp32   2.1e-06/1.0e-05  1.2e-06/5.0e-06  3.8e-05/2.1e-04
  saturated_peaked  bf16   6.5e-07/5.0e-05  3.1e-07/2.3e-05  6.1e-06/7.1e-04

The fp32 kernels use at most a quarter of a bound, the bf16 kernels (exact products, fp32
accumulation: as accurate as the fp32 ones, against bounds 10 x as wide) a fiftieth. The softmax
paths: eL 1.2e-05 to 1.6e-05 against 9.2e-05 to 1.2e-04. bag_stats_kernel: A_mean and A_var within
half of their tolerances (the final rounding to fp32), 0 for identical passes; P_mean within 6e-08
of the float64 value.

Before mcgmil.hip zeroed the feature scale at a threshold of 65536, the in-kernel draws of
gate_pipe_kernel (fp32 and bf16), gate_pp_kernel and gate_fused_kernel kept the features whose
draw is 0xFFFF at p_feat = 1 - 2^-24 and scaled them by 2^24, while the replayed masks, the
generic kernel and the backward pass kept none:
test_edge_threshold_draws_equal_replay[1-2^-24-*] and
test_backward_at_the_drop_everything_threshold failed.
"""
import numpy as np
import pytest
import torch

import head_regimes as hr
from mcgmil import ops, synthetic

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def head_on(arrays, dev):
    return ops.HeadTensors(*[torch.from_numpy(np.ascontiguousarray(arrays[k])).to(dev)
                             for k in ops.HeadTensors._fields])


def features_on(ref, dev, dtype):
    return torch.from_numpy(np.concatenate(ref.Hs)).to(dev).to(dtype).contiguous()


def run(ref, dev, dtype, H=None, **kw):
    """ops.mcdo_forward on a head_regimes.reference case, with its masks drawn in the kernel."""
    H = features_on(ref, dev, dtype) if H is None else H
    args = dict(p_feat=ref.p_f, p_att=ref.p_a, seed=ref.seed, bag_id_base=ref.base)
    args.update(kw)
    out = ops.mcdo_forward(H, ops.bag_offsets_tensor(list(ref.sizes), dev), head_on(ref.arrays, dev),
                           ref.T, **args)
    torch.cuda.synchronize()
    return out


def per_bag(out, ref):
    """Y [T, C] and A [T, C, N_b] of every bag, as numpy."""
    Y = out["Y"].cpu().numpy()
    A = ops.split_bags(out["A"].cpu(), ref.sizes, ref.T * ref.C)
    return [Y[b] for b in range(len(ref.sizes))], \
           [A[b].numpy().reshape(ref.T, ref.C, n) for b, n in enumerate(ref.sizes)]


def check_against_oracle(label, out, ref):
    Ys, As = per_bag(out, ref)
    assert all(np.isfinite(y).all() for y in Ys) and all(np.isfinite(a).all() for a in As), label
    e = hr.case_errors(Ys, As, ref)
    print(label, {k: f"{e[k]:.1e}/{ref.bounds[k]:.1e}" for k in ref.bounds})
    assert e["positive"], label
    bad = {k: (e[k], b) for k, b in ref.bounds.items() if not e[k] <= b}
    assert not bad, (label, bad)
    return e


# ------------------------------------------------------------------------------------ forward
CASES = [(name, kind, head, dtype) for name in hr.REGIMES for kind in hr.KINDS for head in hr.HEADS
         for dtype in (F32, BF16)]


def case_id(c):
    name, kind, (L, D, C, shared), dtype = c
    return f"{name}-{kind}-L{L}D{D}C{C}{'sh' if shared else 'sep'}-{'bf16' if dtype == BF16 else 'fp32'}"


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_forward_matches_float64_oracle(cuda, c):
    name, kind, (L, D, C, shared), dtype = c
    ref = hr.reference(name, kind, L, D, C, shared, dtype == BF16)
    check_against_oracle(case_id(c), run(ref, cuda, dtype), ref)


@pytest.mark.parametrize("L,D,C,shared,sizes", hr.SOFTMAX_CASES,
                         ids=["two_classes_in_registers", "per_class_in_registers", "streaming"])
def test_softmax_group_paths_peaked(cuda, L, D, C, shared, sizes):
    ref = hr.reference("peaked", "relu", L, D, C, shared, False, sizes=sizes, T=2)
    assert hr.peak(ref) >= 0.5
    check_against_oracle(f"softmax C={C} N={sizes[0]}", run(ref, cuda, F32), ref)


@pytest.mark.parametrize("L,D,C,shared,sizes", hr.SOFTMAX_CASES,
                         ids=["two_classes_in_registers", "per_class_in_registers", "streaming"])
def test_softmax_group_paths_logits_beyond_exp_range(cuda, L, D, C, shared, sizes):
    ref = hr.reference("peaked", "relu", L, D, C, shared, False, sizes=sizes, T=2, gains=hr.BEYOND_EXP_RANGE)
    assert ref.top_logit >= 100
    check_against_oracle(f"softmax, logits to {ref.top_logit:.0f}, C={C} N={sizes[0]}", run(ref, cuda, F32), ref)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["trained", "saturated_peaked"])
def test_fused_is_bitwise_the_two_kernel_path(cuda, name, dtype):
    from test_gpu_fused import regions
    ref = hr.reference(name, "relu", bf16=dtype == BF16)
    H = features_on(ref, cuda, dtype)
    offs, head = ops.bag_offsets_tensor(list(ref.sizes), cuda), head_on(ref.arrays, cuda)
    assert regions(H, offs, head, ref.T, path="fused") > 0
    assert regions(H, offs, head, ref.T, path="two_kernel") == 0
    fused = run(ref, cuda, dtype, H=H, path="fused", return_stats=True)
    two = run(ref, cuda, dtype, H=H, path="two_kernel", return_stats=True)
    for k in two:
        assert torch.equal(fused[k], two[k]), k
    check_against_oracle(f"fused {name}", fused, ref)


# ------------------------------------------------------------------------------------ statistics
# bag_stats_kernel against float64 numpy statistics of the GPU's own A and Y. A_mean and A_var:
# fp64 sums and one rounding to fp32 (head_regimes.mean_tolerance / var_tolerance, confirmed on
# the CPU by tests/test_head_regimes_host.py). P_mean is the fp64 mean of a per-sample fp32
# softmax over at most 4 classes, p = e / sum(e), e = expf(v - max v): relative to p, the
# argument's rounding costs x e^-x 2^-24 <= 0.37 x 2^-24 and expf 1 ulp = 2^-23, both once for e
# and once through the sum, the sum's 3 additions 3 x 2^-24 and the division 2^-24: 8.8 x 2^-24,
# with p <= 1 and the final rounding to fp32 under 10 x 2^-24 absolute.
P_MEAN_TOL = 10 * 2.0 ** -24


def check_stats(label, out, sizes, T, C):
    Y = out["Y"].cpu().numpy().astype(np.float64)
    A = ops.split_bags(out["A"].cpu(), sizes, T * C)
    Am = ops.split_bags(out["A_mean"].cpu(), sizes, C)
    Av = ops.split_bags(out["A_var"].cpu(), sizes, C)
    worst = dict(mean=0.0, var=0.0)
    for b, n in enumerate(sizes):
        a = A[b].numpy().reshape(T, C, n)
        mean, var = hr.stats_reference(a)
        dm = np.abs(Am[b].numpy().reshape(C, n).astype(np.float64) - mean)
        worst["mean"] = max(worst["mean"], float(np.max(dm / hr.mean_tolerance(mean))))
        assert (dm <= hr.mean_tolerance(mean)).all(), (label, b)
        got = Av[b].numpy().reshape(C, n).astype(np.float64)
        if T == 1:
            assert np.isnan(got).all(), (label, b)
            continue
        assert (got >= 0).all()
        dv = np.abs(got - var)
        tol = hr.var_tolerance(mean, var)
        worst["var"] = max(worst["var"], float(np.max(dv / tol)))
        assert (dv <= tol).all(), (label, b, float(np.max(dv / tol)))
    e = np.exp(Y - Y.max(-1, keepdims=True))
    P = (e / e.sum(-1, keepdims=True)).mean(1)
    dp = float(np.max(np.abs(out["P_mean"].cpu().numpy().astype(np.float64) - P)))
    print(label, f"|dmean|/tol {worst['mean']:.2f} |dvar|/tol {worst['var']:.2f} |dP_mean| {dp:.1e}/{P_MEAN_TOL:.1e}")
    assert dp <= P_MEAN_TOL, (label, dp)


@pytest.mark.parametrize("name", ["peaked", "trained"])
def test_bag_statistics(cuda, name):
    ref = hr.reference(name, "relu")
    out = run(ref, cuda, F32, return_stats=True)
    assert float(out["A"].max()) >= 0.5
    check_stats(name, out, ref.sizes, ref.T, ref.C)
    # T = 7 identical passes and an instance with A near 1: the variance is pure cancellation
    H = features_on(ref, cuda, F32)
    offs, head = ops.bag_offsets_tensor(list(ref.sizes), cuda), head_on(ref.arrays, cuda)
    same = ops.mcdo_forward(H, offs, head, 7, p_feat=0.0, p_att=0.0, seed=ref.seed, return_stats=True)
    A = ops.split_bags(same["A"], ref.sizes, 7 * ref.C)
    for b, n in enumerate(ref.sizes):
        a = A[b].view(7, ref.C, n)
        assert torch.equal(a, a[:1].expand_as(a))
    big = A[-1].view(7, ref.C, -1)[0]
    assert float(big.max()) >= 0.5
    m = same["A_mean"].double()
    assert bool((same["A_var"].double() <= 2.0 ** -45 * m * m + hr.DENORMAL).all())
    check_stats(name + " T=7 p=0", same, ref.sizes, 7, ref.C)
    one = ops.mcdo_forward(H, offs, head, 1, p_feat=ref.p_f, p_att=ref.p_a, seed=ref.seed, return_stats=True)
    assert bool(one["A_var"].isnan().all())
    check_stats(name + " T=1", one, ref.sizes, 1, ref.C)


# ------------------------------------------------------------------------------------ launches
# name -> (L, D, C, shared), dtype, launch flags: one per gate kernel and the fused launch
SEP, SHARED, C4 = (512, 128, 2, False), (512, 128, 2, True), (512, 128, 4, False)
LAUNCHES = {
    "pipe_fp32": (SEP, F32, dict(path="two_kernel")),
    "pipe_bf16": (SEP, BF16, dict(path="two_kernel")),
    "pp": (SHARED, BF16, dict(path="two_kernel", gate="pp")),
    "generic": (C4, F32, dict(path="two_kernel")),
    "fused": (SEP, BF16, dict(path="fused")),
}


def plain_head(shape, dev, seed=21):
    L, D, C, shared = shape
    return head_on(synthetic.head_arrays(synthetic.head_state_dict(seed, L=L, D=D, C=C, shared=shared), C, shared), dev)


def assert_fused_launch(H, offs, head, T, flags):
    from test_gpu_fused import regions
    want_fused = flags.get("path") == "fused"
    assert (regions(H, offs, head, T, **flags) > 0) == want_fused


# ------------------------------------------------------------------------------------ strided H
def strided_views(H):
    """H [R, L] as the left and the right L columns of two NaN-filled [R, L + 8] buffers: a row
    stride of L + 8 elements, 16-byte aligned rows, and padding that poisons whatever reads it."""
    R, L = H.shape
    left = torch.full((R, L + 8), float("nan"), dtype=H.dtype, device=H.device)
    right = left.clone()
    left[:, :L] = H
    right[:, 8:] = H
    views = {"left": left[:, :L], "right": right[:, 8:8 + L]}
    for v in views.values():
        assert v.stride() == (L + 8, 1) and not v.is_contiguous() and torch.equal(v, H)
    return views


@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_forward_row_stride(cuda, launch):
    shape, dtype, flags = LAUNCHES[launch]
    sizes, T = [130, 37, 1, 300], 3
    head = plain_head(shape, cuda)
    H = torch.cat([torch.from_numpy(hr.features("signed_sparse", 40 + b, n)) for b, n in enumerate(sizes)]) \
        .to(cuda).to(dtype).contiguous()
    offs = ops.bag_offsets_tensor(sizes, cuda)
    assert_fused_launch(H, offs, head, T, flags)
    kw = dict(p_feat=0.2, p_att=0.1, seed=77, bag_id_base=3, return_stats=True, **flags)
    want = ops.mcdo_forward(H, offs, head, T, **kw)
    assert bool(torch.isfinite(want["A"]).all()) and bool(torch.isfinite(want["Y"]).all())
    for where, view in strided_views(H).items():
        got = ops.mcdo_forward(view, offs, head, T, **kw)
        for k in want:
            assert torch.equal(got[k], want[k]), (where, k)


def test_backward_row_stride(cuda):
    sizes, T = [1, 70, 129, 16], 3
    ref = hr.reference("trained", "signed_sparse", sizes=tuple(sizes), T=T)
    head = head_on(ref.arrays, cuda)
    H = features_on(ref, cuda, F32)
    offs = ops.bag_offsets_tensor(sizes, cuda)
    kw = dict(p_feat=0.2, p_att=0.1, seed=77, bag_id_base=3)
    fwd = ops.mcdo_forward(H, offs, head, T, **kw)
    g = torch.Generator(device="cpu").manual_seed(9)
    dY = torch.randn(fwd["Y"].shape, generator=g).to(cuda)
    dA = torch.randn(fwd["A"].shape, generator=g).to(cuda)
    want = ops.mcdo_backward(H, offs, head, T, fwd["A"], fwd["Y"], dY, dA, **kw)
    assert sorted(want) == sorted(ops.GRAD_NAMES + ("dH",))
    assert all(bool(torch.isfinite(v).all()) and bool(v.any()) for v in want.values())
    for where, view in strided_views(H).items():
        got = ops.mcdo_backward(view, offs, head, T, fwd["A"], fwd["Y"], dY, dA, **kw)
        assert got["dH"].is_contiguous()
        for k in want:
            assert torch.equal(got[k], want[k]), (where, k)


# ------------------------------------------------------------------------------------ thresholds
ALMOST_ONE, EDGE_P, oracle_masks = hr.ALMOST_ONE, hr.EDGE_P, hr.oracle_masks
EDGE_SIZES, EDGE_T, EDGE_SEED, EDGE_BASE = hr.EDGE_SIZES, hr.EDGE_T, hr.EDGE_SEED, hr.EDGE_BASE


@pytest.mark.parametrize("p", list(EDGE_P.values()), ids=list(EDGE_P))
def test_edge_threshold_masks_match_oracle(cuda, p):
    L, C, R = 512, 2, sum(EDGE_SIZES)
    offs = ops.bag_offsets_tensor(EDGE_SIZES, cuda)
    kf = ops.feature_keep(offs, R, EDGE_T, L, p, EDGE_SEED, bag_id_base=EDGE_BASE).cpu().numpy()
    ka = ops.attention_keep(offs, R, EDGE_T, C, p, EDGE_SEED, bag_id_base=EDGE_BASE).cpu().numpy()
    want_f, want_a = oracle_masks(EDGE_SIZES, EDGE_T, L, C, p, p, EDGE_SEED,
                                  [EDGE_BASE + b for b in range(len(EDGE_SIZES))])
    assert np.array_equal(kf, want_f) and np.array_equal(ka, want_a)


@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("p", list(EDGE_P.values()), ids=list(EDGE_P))
def test_edge_threshold_draws_equal_replay(cuda, p, launch):
    """mcdo_forward drawing its masks in the kernel (the packed 16-bit rule) against the same call
    replaying the masks of feature_keep / attention_keep (the plain u16 >= thr rule)."""
    shape, dtype, flags = LAUNCHES[launch]
    L, D, C, shared = shape
    head = plain_head(shape, cuda)
    R = sum(EDGE_SIZES)
    H = torch.cat([torch.from_numpy(hr.features("signed_sparse", 50 + b, n)) for b, n in enumerate(EDGE_SIZES)]) \
        .to(cuda).to(dtype).contiguous()
    offs = ops.bag_offsets_tensor(EDGE_SIZES, cuda)
    assert_fused_launch(H, offs, head, EDGE_T, flags)
    kw = dict(p_feat=p, p_att=p, seed=EDGE_SEED, bag_id_base=EDGE_BASE, return_stats=True)
    drawn = ops.mcdo_forward(H, offs, head, EDGE_T, **kw, **flags)
    kf = ops.feature_keep(offs, R, EDGE_T, L, p, EDGE_SEED, bag_id_base=EDGE_BASE)
    ka = ops.attention_keep(offs, R, EDGE_T, C, p, EDGE_SEED, bag_id_base=EDGE_BASE)
    replay = ops.mcdo_forward(H, offs, head, EDGE_T, keep_feat=kf, keep_att=ka, **kw,
                              **dict(flags, path="two_kernel"))
    torch.cuda.synchronize()
    for k in replay:
        assert bool(torch.isfinite(replay[k]).all()), k
        assert torch.equal(drawn[k], replay[k]), k
    if p == ALMOST_ONE:                   # everything dropped: zero logits, uniform attention
        assert not bool(drawn["Y"].any())
        A = ops.split_bags(drawn["A"], EDGE_SIZES, EDGE_T * C)
        for a, n in zip(A, EDGE_SIZES):
            assert torch.equal(a, (torch.ones_like(a) / n))


def test_backward_at_the_drop_everything_threshold(cuda):
    """p_feat = 1 - 2^-24 (threshold 65536): no feature survives, so dH and the gate weights'
    gradients are exactly 0, like the forward's Y."""
    sizes, T = EDGE_SIZES, EDGE_T          # enough draws for one equal to 0xFFFF (the host test checks)
    head = plain_head(SEP, cuda)
    H = torch.cat([torch.from_numpy(hr.features("signed_sparse", 50 + b, n)) for b, n in enumerate(sizes)]).to(cuda)
    offs = ops.bag_offsets_tensor(sizes, cuda)
    kw = dict(p_feat=ALMOST_ONE, p_att=0.1, seed=EDGE_SEED, bag_id_base=EDGE_BASE)
    fwd = ops.mcdo_forward(H, offs, head, T, **kw)
    assert not bool(fwd["Y"].any())
    g = torch.Generator(device="cpu").manual_seed(9)
    dY = torch.randn(fwd["Y"].shape, generator=g).to(cuda)
    dA = torch.randn(fwd["A"].shape, generator=g).to(cuda)
    got = ops.mcdo_backward(H, offs, head, T, fwd["A"], fwd["Y"], dY, dA, **kw)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    for k in ("dH", "dWv", "dWu", "dwk"):
        assert not bool(got[k].any()), k


# ------------------------------------------------------------------------------------ counters
COUNTER_CASES = {
    #                  seed          bag_id_base  bag_ids                t_base
    "bag_base_wraps": (0xABCDEF,     0xFFFFFFFE,  None,                  0),
    "bag_id_minus_1": (0xABCDEF,     0,           (7, -1, 0, -2**31),    0),
    "t_base_top":     (0xABCDEF,     3,           None,                  2**31 - 4),
    "seed_all_ones":  (2**64 - 1,    3,           None,                  5),
}


@pytest.mark.parametrize("name", list(COUNTER_CASES))
def test_philox_counter_edges(cuda, name):
    """Masks against the C oracle at the ends of the counters' ranges, and the in-kernel draws of
    gate_pipe_kernel against a replay of them."""
    seed, base, ids, t_base = COUNTER_CASES[name]
    sizes, T, L, C, p_f, p_a = [5, 37, 64, 9], 3, 512, 2, 0.25, 0.3
    R = sum(sizes)
    offs = ops.bag_offsets_tensor(sizes, cuda)
    bag_ids = None if ids is None else torch.tensor(ids, dtype=torch.int32, device=cuda)
    counters = [(base + b) & 0xFFFFFFFF for b in range(4)] if ids is None else [i & 0xFFFFFFFF for i in ids]
    if name == "bag_base_wraps":
        assert counters == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1]
    ctr = dict(bag_id_base=base, t_base=t_base, bag_ids=bag_ids)
    kf = ops.feature_keep(offs, R, T, L, p_f, seed, **ctr)
    ka = ops.attention_keep(offs, R, T, C, p_a, seed, **ctr)
    want_f, want_a = oracle_masks(sizes, T, L, C, p_f, p_a, seed, counters, t0=t_base)
    assert np.array_equal(kf.cpu().numpy(), want_f) and np.array_equal(ka.cpu().numpy(), want_a)
    assert 0.2 < 1 - np.unpackbits(want_f).mean() < 0.3
    head = plain_head(SEP, cuda)
    H = torch.cat([torch.from_numpy(synthetic.bag_features(60 + b, n)) for b, n in enumerate(sizes)]).to(cuda).bfloat16()
    kw = dict(p_feat=p_f, p_att=p_a, seed=seed, path="two_kernel", **ctr)
    drawn = ops.mcdo_forward(H, offs, head, T, **kw)
    replay = ops.mcdo_forward(H, offs, head, T, keep_feat=kf, keep_att=ka, **kw)
    for k in replay:
        assert torch.equal(drawn[k], replay[k]), k
