"""References for the bf16 form of the stem's fused BatchNorm / ReLU / max-pool training op
(include/mcgmil_pool_grad_bf16.h), shared by tests/test_pool_grad_bf16_host.py and
tests/test_gpu_stem_grad_bf16.py.

The cases are pool_grad_ref.cases() with z and dy rounded to bf16 first (gamma and beta stay fp32,
as the fp32 master parameters do). The references are float64 and fp32 CPU autograd of the
UNROUNDED function max_pool2d(relu?(batch_norm(z))) on those bf16-valued inputs: the op names the
window's largest unrounded value, so it is not compared with torch's bf16 autograd, which pools
the rounded BatchNorm output (include/mcgmil_pool_grad_bf16.h).

Rounding z to bf16 creates exact ties between taps of a window. The reference (max_pool2d) and the
kernel both give an exact tie to the first tap in row-major order, so exact ties are allowed and
margins() looks at the smallest NON-ZERO gap."""
import functools

import torch
import torch.nn.functional as F

import bn_grad_ref as R
import pool_grad_ref as P

BF = torch.bfloat16
EPS = P.EPS
GRADS = P.GRADS
FWD = P.FWD
PART_ELEMS = 32768                  # MCGMIL_BN_POOL_GRAD_PART_ELEMS
CASES = P.cases(PART_ELEMS)


def rounded(case):
    """The case with z and dy rounded to bf16 (kept as fp32 tensors of bf16 values)."""
    return dict(case, z=case["z"].to(BF).float(), dy=case["dy"].to(BF).float())


def make(name):
    shape, pool, relu, seed, integer = CASES[name]
    return rounded(P.make(shape, pool, seed, relu, integer))


def margins(a, pool):
    """(smallest NON-ZERO gap between the two largest values of any window, smallest |window
    maximum|) of the BatchNorm output a [N, C, H, W] under -inf padding. A window with one tap has
    an infinite gap; inf when every gap is an exact tie."""
    k, st, pd = pool
    N, C = a.shape[:2]
    win = F.unfold(F.pad(a, (pd, pd, pd, pd), value=float("-inf")), k, stride=st).view(N, C, k * k, -1)
    top = win.topk(2, dim=2).values
    gap = top[:, :, 0] - top[:, :, 1]
    gap = gap[gap > 0]
    return (float(gap.min()) if gap.numel() else float("inf")), float(top[:, :, 0].abs().min())


def reference_of(c):
    """(case, float64 CPU autograd with its window codes "code", fp32 CPU autograd with "code",
    gradient bounds, forward bounds) of a case whose z and dy are bf16 values."""
    r64, r32 = P.autograd(c, torch.float64), P.autograd(c, torch.float32)
    for r in (r64, r32):
        r["code"] = P.codes(r["idx"], r["y"], c["z"].shape[3], c["pool"], c["relu"])
    return c, r64, r32, R.bounds(R.errors(r32, r64, GRADS)), R.bounds(R.errors(r32, r64, FWD))


@functools.lru_cache(maxsize=None)
def reference(name):
    """reference_of(make(name)); computed once and shared, so treat it as read-only."""
    return reference_of(make(name))


def bf16_excess(got, ref, B):
    """The project's rule for a bf16 tensor against a float64 reference, elementwise
    |d| <= 2^-7 |ref| + B max|ref| (2^-8 is bf16's unit roundoff, doubled for rounding an fp32 result
    that itself carries the error B): the largest |d| / (2^-7 |ref| + B max|ref|), <= 1 within it."""
    ref = ref.double()
    d = (got.detach().to(ref.device).double().reshape(ref.shape) - ref).abs()
    allowed = 2.0 ** -7 * ref.abs() + B * ref.abs().max()
    return float((d / allowed.clamp_min(1e-300)).max()) if float(allowed.max()) > 0 else float(d.max())


def first_max_codes(a, pool, relu):
    """The header's rule restated without max_pool2d: for every window of the BatchNorm output a
    [N, C, H, W] the smallest kh * k + kw among the taps that equal the window's maximum (255 where
    that maximum is <= 0 with ReLU), and the number of windows in which more than one tap does."""
    k, st, pd = pool
    N, C, H, W = a.shape
    PH, PW = P.pooled(H, k, st, pd), P.pooled(W, k, st, pd)
    win = F.unfold(F.pad(a, (pd, pd, pd, pd), value=float("-inf")), k, stride=st).view(N, C, k * k, PH, PW)
    top = win.max(dim=2, keepdim=True).values
    hit = win == top
    tap = torch.arange(k * k).view(1, 1, -1, 1, 1).expand_as(win)
    code = torch.where(hit, tap, torch.full_like(tap, P.NONE)).min(dim=2).values
    if relu:
        code = torch.where(top[:, :, 0] <= 0, torch.full_like(code, P.NONE), code)
    return code.to(torch.uint8), int((hit.sum(2) > 1).sum())
