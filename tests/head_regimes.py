"""Value regimes for the MIL head's tests: the same synthetic heads and bags as everywhere else,
with the gate and attention layers scaled so that the arithmetic leaves the almost-linear,
almost-uniform corner that torch's default init and |N(0, 1)| features stay in.

  regime(name, ...)    a synthetic.head_state_dict with attention_V x gv, attention_U x gu and
                       attention_weights x ga (weights and biases)
  features(kind, ...)  "relu" = synthetic.bag_features, "signed_sparse" = the same values with a
                       seeded random sign and ~30 % of the elements exactly 0
  reference(...)       oracle.mcdo_ref.mc_inference in float64 and in float32 on the same inputs
                       and Philox masks; the float32 run's errors give the bounds

Errors of a case (the largest over its bags):
  eA = max|A - A_ref| / max|A_ref|
  eY = max|Y - Y_ref| / max(1, max|Y_ref|)
  eL = max|ln A - ln A_ref| over the entries with A_ref >= 1e-30: the per-entry relative error
       that eA cannot see once one instance holds nearly all of the attention
Bound of each error: max(10 x the float32 CPU run's error against float64, 1e-6), the rule of
tests/test_gpu_head_grad.py; x 10 again for bf16 operands (the ratio of TOL_BF16_IN to TOL32 in
tests/test_gpu_parity.py), where both CPU runs see the bf16-rounded operands.

Measured on the CPU (float64; one bag of 300, T = 3, separate heads):
  saturated          5-9 % of the tanh arguments beyond +-15, 13-16 % of the sigmoid arguments
                     beyond each of +-88, attention still flat (max 0.009-0.014)
  peaked             gates linear, max A = 0.997, min A = 2e-20
  trained            max A = 0.87-0.999, min A = 3e-25
  saturated_peaked   saturated gates and max A = 0.82, min A = 1e-10
"""
import functools

import numpy as np
import torch

from mcgmil import synthetic
from oracle import mcdo_ref, philox

#                              gv   gu    ga
REGIMES = {"saturated":        (16, 160, 1),
           "peaked":           (1,  1,   60),
           "trained":          (4,  4,   30),
           "saturated_peaked": (16, 160, 8)}
KINDS = ("relu", "signed_sparse")
_SCALED = ("attention_V.", "attention_U.", "attention_weights.")

TANH_LIMIT = 15.0        # the kernel clamps the tanh argument there (tanh is +-1 in fp32)
SIGMOID_LIMIT = 88.0     # e^-y overflows / underflows fp32 beyond it
LOG_FLOOR = 1e-30        # eL skips reference entries below this
BOUND_FLOOR = 1e-6

SIZES = (130, 37, 1, 300)
SEED, BASE = 0x5EED0FF1CE, 5
# (L, D, C, shared) of tests/test_gpu_parity.py SHAPES that select distinct gate kernels
HEADS = [(512, 128, 2, False),   # gate_pipe_kernel
         (512, 128, 2, True),    # gate_pp_kernel in bf16
         (512, 128, 4, False),   # generic kernel, 32 gate tile pairs
         (96, 32, 2, True),      # generic kernel, L % 64 != 0
         (512, 64, 4, False)]    # 32x32x16 kernel in bf16
# (L, D, C, shared, sizes) for softmax_group's three paths: two classes in registers, one class at
# a time in registers, streaming (more than 4096 instances)
SOFTMAX_CASES = [(512, 128, 2, False, (300,)), (512, 64, 3, False, (300,)), (512, 128, 2, False, (4100,))]
# attention_weights x 300: logits beyond 88, where e^logit leaves fp32 and only the subtraction of
# the group's maximum keeps the softmax finite. (The four regimes' logits stay below 30, where a
# softmax without the subtraction is the same function.) Most of A is then below eL's floor, so
# eL covers only the few instances that hold the attention.
BEYOND_EXP_RANGE = (1, 1, 300)


def scale_state_dict(sd, gv=1.0, gu=1.0, ga=1.0):
    out = {}
    for k, v in sd.items():
        g = 1.0
        for prefix, gain in zip(_SCALED, (gv, gu, ga)):
            if k.startswith(prefix):
                g = gain
        out[k] = (v * np.float32(g)).astype(np.float32)
    return out


def regime(name, seed, L=512, D=128, C=2, shared=False):
    """State dict (reference key names) of a synthetic head in the named regime."""
    return scale_state_dict(synthetic.head_state_dict(seed, L=L, D=D, C=C, shared=shared), *REGIMES[name])


def signed_sparse(seed, N, L=512):
    H = synthetic.bag_features(seed, N, L)
    rng = np.random.Generator(np.random.PCG64(seed + 0x51A9))
    negative = rng.integers(0, 2, size=H.shape) == 1
    zero = rng.random(H.shape) < 0.3
    return np.where(zero, np.float32(0), np.where(negative, -H, H)).astype(np.float32)


def features(kind, seed, N, L=512):
    if kind == "relu":
        return synthetic.bag_features(seed, N, L)
    if kind == "signed_sparse":
        return signed_sparse(seed, N, L)
    raise ValueError(kind)


# ------------------------------------------------------------------------------------ errors
def _nrel(got, ref):
    den = float(np.max(np.abs(ref)))
    return float(np.max(np.abs(got - ref))) / (den if den > 0 else 1.0)


def bag_errors(Y, A, Y_ref, A_ref):
    """(eA, eY, eL, skipped entries, all compared entries > 0) of one bag; float64 arrays."""
    Y, A = np.asarray(Y, dtype=np.float64), np.asarray(A, dtype=np.float64)
    eA = _nrel(A, A_ref)
    eY = float(np.max(np.abs(Y - Y_ref))) / max(1.0, float(np.max(np.abs(Y_ref))))
    use = A_ref >= LOG_FLOOR
    positive = bool((A[use] > 0).all())
    with np.errstate(divide="ignore"):
        eL = float(np.max(np.abs(np.log(A[use]) - np.log(A_ref[use])))) if use.any() else 0.0
    return eA, eY, eL, int((~use).sum()), positive


def case_errors(Ys, As, ref):
    """Errors of a whole case: Ys[b] [T, C] and As[b] [T, C, N_b] against ref.Y64 / ref.A64."""
    e = dict(eA=0.0, eY=0.0, eL=0.0)
    skipped, positive = 0, True
    for Y, A, Yr, Ar in zip(Ys, As, ref.Y64, ref.A64):
        eA, eY, eL, sk, pos = bag_errors(Y, A, Yr, Ar)
        e = dict(eA=max(e["eA"], eA), eY=max(e["eY"], eY), eL=max(e["eL"], eL))
        skipped += sk
        positive = positive and pos
    e["skipped"] = skipped / max(1, sum(a.size for a in ref.A64))
    e["positive"] = positive
    return e


# ------------------------------------------------------------------------------------ reference
class Ref:
    pass


def _pre_activations(H, keepF, arrays, p_f):
    """float64 tanh / sigmoid arguments of one bag: two arrays [T, G, N, D]."""
    Hd = H.astype(np.float64)[None] * (keepF * np.float64(np.float32(mcdo_ref.dropout_scale(p_f))))
    x = np.einsum("tnl,gdl->tgnd", Hd, arrays["Wv"].astype(np.float64)) + arrays["bv"][None, :, None, :]
    y = np.einsum("tnl,gdl->tgnd", Hd, arrays["Wu"].astype(np.float64)) + arrays["bu"][None, :, None, :]
    return x, y


@functools.lru_cache(maxsize=None)
def reference(name, kind, L=512, D=128, C=2, shared=False, bf16=False, sizes=SIZES, T=3,
              p_f=0.2, p_a=0.1, seed=SEED, base=BASE, gains=None):
    """One case: a batch of bags through a head in regime `name` (or with the explicit `gains`).
    Computed once per process and never modified.

      .sd, .arrays   the head the kernel gets (fp32, unrounded)
      .Hs            the bags' features as the kernel gets them (bf16 cases: already rounded)
      .Y64 [T, C], .A64 [T, C, N_b] per bag: the float64 oracle on the kernel's operands
      .err32         case_errors of the float32 oracle against them
      .bounds        eA / eY / eL bounds (see the module docstring)
      .shares        fractions of the gate arguments beyond each limit: x_lo, x_hi, y_lo, y_hi
      .top_logit     the largest attention logit (after its dropout) of the case
    """
    r = Ref()
    r.name, r.kind, r.L, r.D, r.C, r.shared, r.bf16 = name, kind, L, D, C, shared, bf16
    r.sizes, r.T, r.p_f, r.p_a, r.seed, r.base = tuple(sizes), T, p_f, p_a, seed, base
    head_seed = L + D + C
    if gains is None:
        r.sd = regime(name, head_seed, L=L, D=D, C=C, shared=shared)
    else:
        r.sd = scale_state_dict(synthetic.head_state_dict(head_seed, L=L, D=D, C=C, shared=shared), *gains)
    r.arrays = synthetic.head_arrays(r.sd, C, shared)
    r.Hs = [features(kind, 300 + b, n, L) for b, n in enumerate(sizes)]
    sd_ref = r.sd
    if bf16:
        r.Hs = [synthetic.bf16_round(h) for h in r.Hs]
        sd_ref = synthetic.round_state_dict_bf16(r.sd)
    arrays_ref = synthetic.head_arrays(sd_ref, C, shared)
    p64 = mcdo_ref.HeadParams(arrays_ref, dtype=torch.float64)
    p32 = mcdo_ref.HeadParams(arrays_ref, dtype=torch.float32)
    r.Y64, r.A64, Y32, A32 = [], [], [], []
    beyond = np.zeros(4)
    total = 0
    r.top_logit = -np.inf
    for b, n in enumerate(sizes):
        kF, kA = mcdo_ref.masks_for_bag(seed, base + b, T, n, L, C, p_f, p_a)
        Y, A = mcdo_ref.mc_inference(r.Hs[b], p64, kF, kA, p_f, p_a)
        r.Y64.append(Y[:, 0].numpy())
        r.A64.append(A[:, 0].numpy())
        Y, A = mcdo_ref.mc_inference(r.Hs[b], p32, kF, kA, p_f, p_a)
        Y32.append(Y[:, 0].numpy())
        A32.append(A[:, 0].numpy())
        x, y = _pre_activations(r.Hs[b], kF, arrays_ref, p_f)
        beyond += [(x < -TANH_LIMIT).sum(), (x > TANH_LIMIT).sum(),
                   (y < -SIGMOID_LIMIT).sum(), (y > SIGMOID_LIMIT).sum()]
        total += x.size
        with np.errstate(over="ignore"):
            gated = np.tanh(x) / (1.0 + np.exp(-y))
        G = gated.shape[1]
        logits = np.stack([gated[:, c if G > 1 else 0] @ arrays_ref["wa"][c].astype(np.float64) + arrays_ref["ba"][c]
                           for c in range(C)], axis=1) * (kA * np.float64(np.float32(mcdo_ref.dropout_scale(p_a))))
        r.top_logit = max(r.top_logit, float(logits.max(-1).max()))
    r.shares = dict(zip(("x_lo", "x_hi", "y_lo", "y_hi"), (beyond / total).tolist()))
    r.err32 = case_errors(Y32, A32, r)
    scale = 10.0 if bf16 else 1.0
    r.bounds = {k: scale * max(10.0 * r.err32[k], BOUND_FLOOR) for k in ("eA", "eY", "eL")}
    return r


def peak(ref, min_rows=100):
    """Largest reference attention weight over the (t, c) groups of the bags of >= min_rows."""
    return max(float(a.max()) for a in ref.A64 if a.shape[-1] >= min_rows)


# ------------------------------------------------------------------------------------ statistics
def stats_kernel_restated(A):
    """bag_stats_kernel's arithmetic on A [T, ...] (fp32 values): fp64 sums over 8 interleaved
    sample groups added in group order, mean = s / T, var = max((ss - s mean) / (T - 1), 0), each
    rounded to fp32 once."""
    A = np.asarray(A, dtype=np.float32).astype(np.float64)
    T = A.shape[0]
    s = np.zeros(A.shape[1:])
    ss = np.zeros(A.shape[1:])
    for g in range(8):
        gs = np.zeros(A.shape[1:])
        gss = np.zeros(A.shape[1:])
        for t in range(g, T, 8):
            gs = gs + A[t]
            gss = gss + A[t] * A[t]
        s, ss = (gs, gss) if g == 0 else (s + gs, ss + gss)
    mean = s / T
    var = np.maximum((ss - s * mean) / (T - 1), 0.0) if T > 1 else np.full(A.shape[1:], np.nan)
    return mean.astype(np.float32), var.astype(np.float32)


def stats_reference(A):
    """float64 mean and unbiased two-pass variance over axis 0 of the fp32 values A."""
    A = np.asarray(A, dtype=np.float32).astype(np.float64)
    mean = A.mean(0)
    var = ((A - mean) ** 2).sum(0) / (A.shape[0] - 1) if A.shape[0] > 1 else np.full(A.shape[1:], np.nan)
    return mean, var


DENORMAL = 2.0 ** -149       # spacing of the fp32 denormals: a result below 2^-126 rounds to within it


def mean_tolerance(mean):
    """fp64 sum, one division, one rounding to fp32."""
    return 2.0 ** -23 * np.abs(mean) + DENORMAL


def var_tolerance(mean, var):
    """The rounding of the result (first term) and the cancellation in ss - s mean, both of about
    T (mean^2 + var): a few fp64 roundings of it, divided by T - 1, for T <= 64 (second term)."""
    return 2.0 ** -23 * var + 2.0 ** -45 * (mean ** 2 + var) + DENORMAL


# ------------------------------------------------------------------------------------ thresholds
# drop probabilities whose 16-bit thresholds sit next to 0, 0x8000 and 0xFFFF, and the batch they
# are tested on: about 5e5 feature draws, so one equal to 0xFFFF occurs with probability > 0.999
ALMOST_ONE = float(np.nextafter(np.float32(1), np.float32(0)))       # the largest float32 below 1
EDGE_P = {"1/65536": 1 / 65536, "0x7FFF/65536": 0x7FFF / 65536, "0x8000/65536": 0x8000 / 65536,
          "0x8001/65536": 0x8001 / 65536, "0xFFFF/65536": 0xFFFF / 65536, "1-2^-24": ALMOST_ONE}
EDGE_SIZES, EDGE_T, EDGE_SEED, EDGE_BASE = [300, 37], 3, 0xC0FFEE, 2


def oracle_masks(sizes, T, L, C, p_f, p_a, seed, counters, t0=0):
    """(packed feature keep bits [T * rows, L / 8], attention keep flags [T * C * rows]) of a
    batch, from the C oracle."""
    kf = [philox.feature_keep_bits(seed, c, T, n, L, p_f, t0).reshape(T * n, L // 8) for c, n in zip(counters, sizes)]
    ka = [philox.attention_keep(seed, c, T, C, n, p_a, t0).astype(np.uint8).reshape(-1) for c, n in zip(counters, sizes)]
    return np.concatenate(kf), np.concatenate(ka)
