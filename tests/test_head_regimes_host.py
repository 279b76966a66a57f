"""CPU checks of tests/head_regimes.py: every regime case that tests/test_gpu_head_regimes.py runs
is in the regime its name claims, its bounds come from a float32 run that really differs from
float64, and bag_stats_kernel's formula (restated in numpy) meets the tolerances the GPU test
derives from it."""
import numpy as np
import pytest

import head_regimes as hr
from oracle import philox

CASES = [(name, kind, head, bf16) for name in hr.REGIMES for kind in hr.KINDS for head in hr.HEADS
         for bf16 in (False, True)]


def case_id(c):
    name, kind, (L, D, C, shared), bf16 = c
    return f"{name}-{kind}-L{L}D{D}C{C}{'sh' if shared else 'sep'}-{'bf16' if bf16 else 'fp32'}"


def test_regime_scales_only_the_gate_and_attention_layers():
    from mcgmil import synthetic
    plain = synthetic.head_state_dict(3, C=2, shared=False)
    sd = hr.regime("saturated_peaked", 3)
    gv, gu, ga = hr.REGIMES["saturated_peaked"]
    assert sorted(sd) == sorted(plain)
    for k, v in plain.items():
        g = gv if k.startswith("attention_V") else gu if k.startswith("attention_U") else \
            ga if k.startswith("attention_weights") else 1
        assert sd[k].dtype == np.float32 and np.array_equal(sd[k], v * np.float32(g)), k
    shared = hr.regime("trained", 3, shared=True)
    assert np.array_equal(shared["attention_V.0.bias"], synthetic.head_state_dict(3, shared=True)["attention_V.0.bias"] * 4)


def test_signed_sparse_features():
    from mcgmil import synthetic
    H = hr.features("signed_sparse", 11, 300)
    base = synthetic.bag_features(11, 300)
    assert H.dtype == np.float32 and H.shape == base.shape
    assert np.array_equal(H, hr.features("signed_sparse", 11, 300))
    nz = H != 0
    assert np.array_equal(np.abs(H[nz]), base[nz])
    assert 0.28 <= 1 - nz.mean() <= 0.32
    assert 0.48 <= (H[nz] < 0).mean() <= 0.52
    assert not np.signbit(H[~nz]).any()
    assert np.array_equal(hr.features("relu", 11, 300), base)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_is_in_its_regime(c):
    name, kind, (L, D, C, shared), bf16 = c
    r = hr.reference(name, kind, L, D, C, shared, bf16)
    print(case_id(c), {k: f"{v:.3f}" for k, v in r.shares.items()}, f"peak {hr.peak(r):.3g}",
          {k: f"{r.err32[k]:.1e}" for k in ("eA", "eY", "eL")})
    if name.startswith("saturated"):
        assert all(s >= 0.02 for s in r.shares.values()), r.shares
    if name != "saturated":
        assert hr.peak(r) >= 0.5
    assert r.err32["skipped"] <= 0.01
    assert r.err32["positive"]
    assert r.err32["eL"] > 0                       # the eL bound is not on its floor by accident
    assert all(np.isfinite(v) and v >= hr.BOUND_FLOOR for v in r.bounds.values())
    for Y, A, n in zip(r.Y64, r.A64, r.sizes):
        assert Y.shape == (r.T, C) and A.shape == (r.T, C, n)
        assert np.isfinite(Y).all() and np.allclose(A.sum(-1), 1.0, atol=1e-12)


def test_softmax_path_cases_are_peaked():
    for L, D, C, shared, sizes in hr.SOFTMAX_CASES:
        r = hr.reference("peaked", "relu", L, D, C, shared, False, sizes=sizes, T=2)
        assert hr.peak(r) >= 0.5 and r.err32["eL"] > 0 and r.err32["skipped"] <= 0.01
        assert r.top_logit < 80
        # the same three paths with logits that only a max-subtracting softmax survives in fp32
        r = hr.reference("peaked", "relu", L, D, C, shared, False, sizes=sizes, T=2, gains=hr.BEYOND_EXP_RANGE)
        assert r.top_logit >= 100 and hr.peak(r) >= 0.5 and r.err32["eL"] > 0 and r.err32["positive"]


# ------------------------------------------------------------------------------------ statistics
def _check_stats(A, label):
    mean_k, var_k = hr.stats_kernel_restated(A)
    mean, var = hr.stats_reference(A)
    dm = np.abs(mean_k.astype(np.float64) - mean)
    assert (dm <= hr.mean_tolerance(mean)).all(), label
    if A.shape[0] > 1:
        dv = np.abs(var_k.astype(np.float64) - var)
        tol = hr.var_tolerance(mean, var)
        print(label, f"max dv/tol = {np.max(dv / tol):.3f}")
        assert (dv <= tol).all(), label
    else:
        assert np.isnan(var_k).all()


@pytest.mark.parametrize("name", ["peaked", "trained"])
def test_stats_formula_meets_its_tolerances(name):
    r = hr.reference(name, "relu")
    for A in r.A64:
        _check_stats(A.astype(np.float32), name)
        _check_stats(A[:1].astype(np.float32), name + " T=1")
    # T identical passes with one instance near 1: the variance is pure cancellation
    r0 = hr.reference(name, "relu", sizes=(300,), T=1, p_f=0.0, p_a=0.0)
    A = np.repeat(r0.A64[0].astype(np.float32), 7, axis=0)
    assert A.max() >= 0.5
    mean_k, var_k = hr.stats_kernel_restated(A)
    assert (var_k <= 2.0 ** -45 * mean_k.astype(np.float64) ** 2 + hr.DENORMAL).all()
    _check_stats(A, name + " T=7 identical")
    # T = 64, the largest T of the tolerance, with values that differ in every bit
    rng = np.random.Generator(np.random.PCG64(1))
    A = np.float32(1.0) - rng.random((64, 4096)).astype(np.float32) * np.float32(2.0 ** -12)
    _check_stats(A, "T=64 near 1")


# ------------------------------------------------------------------------------------ thresholds
def test_edge_thresholds_are_what_they_claim():
    """The thresholds sit where the packed keep rule can go wrong, and the draws reach them."""
    thr = {k: philox.drop_threshold(p) for k, p in hr.EDGE_P.items()}
    assert thr == {"1/65536": 1, "0x7FFF/65536": 0x7FFF, "0x8000/65536": 0x8000, "0x8001/65536": 0x8001,
                   "0xFFFF/65536": 0xFFFF, "1-2^-24": 65536}
    assert hr.ALMOST_ONE < 1 and philox.dropout_scale(hr.ALMOST_ONE) == 2.0 ** 24
    counters = [hr.EDGE_BASE + b for b in range(len(hr.EDGE_SIZES))]
    top, _ = hr.oracle_masks(hr.EDGE_SIZES, hr.EDGE_T, 512, 2, 0xFFFF / 65536, 0.0, hr.EDGE_SEED, counters)
    low, _ = hr.oracle_masks(hr.EDGE_SIZES, hr.EDGE_T, 512, 2, 1 / 65536, 0.0, hr.EDGE_SEED, counters)
    none, _ = hr.oracle_masks(hr.EDGE_SIZES, hr.EDGE_T, 512, 2, hr.ALMOST_ONE, 0.0, hr.EDGE_SEED, counters)
    assert top.any()                      # a draw equal to 0xFFFF: kept at thr 0xFFFF ...
    assert not none.any()                 # ... and dropped at thr 65536
    assert (low != 0xFF).any()            # a draw equal to 0: dropped at thr 1
