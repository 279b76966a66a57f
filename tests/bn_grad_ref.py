"""References for the fused BatchNorm/add/ReLU backward (include/mcgmil_bn_grad.h), shared by
tests/test_bn_grad_host.py and tests/test_gpu_bn_grad.py.

autograd(): torch.autograd of F.batch_norm (training mode: batch statistics, biased variance)
(+ residual) (+ relu) in a chosen dtype, on a chosen device. formula(): the header's closed form,
restated. errors(): the head-gradient tests' measure, for tensor k
max|got_k - ref_k| / max(max|ref_k|, 1e-3 max_j max|ref_j|)."""
import torch
import torch.nn.functional as F

EPS = 1e-5
GRADS = ("dx", "dres", "dgamma", "dbeta")


def make(rows_shape, C, seed, relu, residual, gamma=True):
    """Unit-scale fp32 inputs of a case: x [N, C, H, W] with a per-channel offset and scale, gamma of
    both signs, beta, residual, dy. rows_shape = (N, H, W)."""
    N, H, W = rows_shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g) * (0.5 + torch.rand(1, C, 1, 1, generator=g)) + \
        torch.randn(1, C, 1, 1, generator=g)
    case = {"x": x, "relu": relu, "dy": torch.randn(N, C, H, W, generator=g),
            "gamma": (0.5 + torch.rand(C, generator=g)) * (1 - 2 * (torch.rand(C, generator=g) < 0.25).float())
            if gamma else None,
            "beta": 0.5 * torch.randn(C, generator=g) if gamma else None,
            "res": torch.randn(N, C, H, W, generator=g) if residual else None}
    return case


def autograd(case, dtype, device="cpu"):
    """{"y", "z" (the pre-activation), "mean", "invstd", "dx", "dres", "dgamma", "dbeta"} (dres /
    dgamma / dbeta None where the case has no residual / affine parameters)."""
    to = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype)  # noqa: E731
    leaf = lambda t: None if t is None else to(t).clone().requires_grad_()  # noqa: E731
    x, gamma, beta, res = leaf(case["x"]), leaf(case["gamma"]), leaf(case["beta"]), leaf(case["res"])
    z = F.batch_norm(x, None, None, gamma, beta, True, 0.0, EPS)
    if res is not None:
        z = z + res
    y = torch.relu(z) if case["relu"] else z
    y.backward(to(case["dy"]))
    xd = x.detach()
    var = xd.var((0, 2, 3), unbiased=False)
    g = lambda t: None if t is None else t.grad  # noqa: E731
    return {"y": y.detach(), "z": z.detach(), "mean": xd.mean((0, 2, 3)), "invstd": (var + EPS).rsqrt(),
            "dx": x.grad, "dres": g(res), "dgamma": g(gamma), "dbeta": g(beta)}


def formula(x, y, dy, gamma, mean, invstd, relu):
    """(dx, dresidual, dgamma, dbeta) of include/mcgmil_bn_grad.h in the dtype of x ([N, C, H, W])."""
    b = lambda v: v.view(1, -1, 1, 1)  # noqa: E731
    n = x.numel() // x.shape[1]
    xh = (x - b(mean)) * b(invstd)
    g = dy * (y > 0) if relu else dy
    dbeta = g.sum((0, 2, 3))
    dgamma = (g * xh).sum((0, 2, 3))
    gam = torch.ones_like(mean) if gamma is None else gamma
    dx = b(gam * invstd) * (g - b(dbeta) / n - xh * b(dgamma) / n)
    return dx, g, dgamma, dbeta


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def errors(got, ref, keys=GRADS):
    """{k: error of got[k] against ref[k]} over the keys both have (tensors on any device)."""
    keys = [k for k in keys if ref.get(k) is not None and got.get(k) is not None]
    top = max(_amax(ref[k]) for k in keys)
    out = {}
    for k in keys:
        r = ref[k]
        d = _amax(got[k].detach().to(device=r.device, dtype=r.dtype).reshape(r.shape) - r)
        out[k] = d / max(_amax(r), 1e-3 * top)
    return out


def bounds(e32):
    """10 x the fp32 reference's own error, at least 1e-6."""
    return {k: max(10.0 * e, 1e-6) for k, e in e32.items()}
