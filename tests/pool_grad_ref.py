"""References for the stem's fused BatchNorm / ReLU / max-pool training op
(include/mcgmil_pool_grad.h), shared by tests/test_pool_grad_ref.py and
tests/test_gpu_stem_grad.py.

make(): a case's fp32 inputs. autograd(): torch.autograd of
max_pool2d(relu?(batch_norm(z))) (training mode: batch statistics, biased variance) in a chosen
dtype on a chosen device, with the pool's flat indices. codes(): those indices as the header's
window codes kh * k + kw (255 where the ReLU zeroes the gradient). formula(): the header's closed
form in plain torch. margins(): how far the reference is from a flipped argmax or ReLU mask.
The error measure and the bounds are bn_grad_ref.errors / bounds."""
import torch
import torch.nn.functional as F

import bn_grad_ref as R

EPS = R.EPS
NONE = 255
GRADS = ("dz", "dgamma", "dbeta")
FWD = ("y", "mean", "invstd")


def pooled(size, k, st, pd):
    return (size + 2 * pd - k) // st + 1


def make(shape, pool, seed, relu=True, integer=False, gamma=True):
    """Unit-scale fp32 inputs of a case: z [N, C, H, W] by the seed scheme of bn_grad_ref.make
    (per-channel offset and scale, gamma of both signs, beta), dy [N, C, PH, PW]. integer: z of
    small integers 0..3 and gamma = 1 + c / C, beta = 0.5, so that every window has exact ties and
    positive activated values above the mean."""
    N, C, H, W = shape
    k, st, pd = pool
    c = R.make((N, H, W), C, seed, relu, False, gamma)
    g = torch.Generator().manual_seed(seed + 1000)
    case = {"z": c["x"], "gamma": c["gamma"], "beta": c["beta"], "relu": relu, "pool": pool,
            "dy": torch.randn(N, C, pooled(H, k, st, pd), pooled(W, k, st, pd), generator=g)}
    if integer:
        case["z"] = torch.randint(0, 4, (N, C, H, W), generator=g).float()
        case["gamma"] = 1.0 + torch.arange(C).float() / C
        case["beta"] = torch.full((C,), 0.5)
    return case


def autograd(case, dtype, device="cpu"):
    """{"y", "a" (the BatchNorm output, before the ReLU), "idx" (max_pool2d's flat indices), "mean",
    "invstd", "dz", "dgamma", "dbeta"} (dgamma / dbeta None without affine parameters)."""
    to = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype)  # noqa: E731
    leaf = lambda t: None if t is None else to(t).clone().requires_grad_()  # noqa: E731
    z, gamma, beta = leaf(case["z"]), leaf(case["gamma"]), leaf(case["beta"])
    k, st, pd = case["pool"]
    a = F.batch_norm(z, None, None, gamma, beta, True, 0.0, EPS)
    r = torch.relu(a) if case["relu"] else a
    y, idx = F.max_pool2d(r, k, st, pd, return_indices=True)
    y.backward(to(case["dy"]))
    zd = z.detach()
    var = zd.var((0, 2, 3), unbiased=False)
    g = lambda t: None if t is None else t.grad  # noqa: E731
    return {"y": y.detach(), "a": a.detach(), "idx": idx, "mean": zd.mean((0, 2, 3)), "invstd": (var + EPS).rsqrt(),
            "dz": z.grad, "dgamma": g(gamma), "dbeta": g(beta)}


def codes(idx, y, W, pool, relu):
    """torch's flat indices ih * W + iw [N, C, PH, PW] as uint8 window codes kh * k + kw; 255 where
    y == 0 with ReLU (the whole window was <= 0)."""
    k, st, pd = pool
    PH, PW = idx.shape[2:]
    ph = torch.arange(PH, device=idx.device).view(1, 1, PH, 1)
    pw = torch.arange(PW, device=idx.device).view(1, 1, 1, PW)
    kh = idx // W - (ph * st - pd)
    kw = idx % W - (pw * st - pd)
    assert int(kh.min()) >= 0 and int(kh.max()) < k and int(kw.min()) >= 0 and int(kw.max()) < k
    code = kh * k + kw
    if relu:
        code = torch.where(y == 0, torch.full_like(code, NONE), code)
    return code.to(torch.uint8)


def scatter(code, dy, H, W, pool):
    """g [N, C, H, W]: dy of every pooled output added at the input pixel its code names."""
    k, st, pd = pool
    N, C, PH, PW = dy.shape
    g = dy.new_zeros((N, C, max(H + 2 * pd, k + st * (PH - 1)), max(W + 2 * pd, k + st * (PW - 1))))
    for kh in range(k):
        for kw in range(k):
            g[:, :, kh:kh + st * (PH - 1) + 1:st, kw:kw + st * (PW - 1) + 1:st] += dy * (code == kh * k + kw)
    return g[:, :, pd:pd + H, pd:pd + W]


def formula(z, code, dy, gamma, mean, invstd, pool):
    """(dz, dgamma, dbeta) of include/mcgmil_pool_grad.h in the dtype of z ([N, C, H, W])."""
    b = lambda v: v.view(1, -1, 1, 1)  # noqa: E731
    n = z.numel() // z.shape[1]
    xh = (z - b(mean)) * b(invstd)
    g = scatter(code, dy, z.shape[2], z.shape[3], pool)
    dbeta = g.sum((0, 2, 3))
    dgamma = (g * xh).sum((0, 2, 3))
    gam = torch.ones_like(mean) if gamma is None else gamma
    dz = b(gam * invstd) * (g - b(dbeta) / n - xh * b(dgamma) / n)
    return dz, dgamma, dbeta


def margins(a, pool):
    """(smallest gap between the two largest values of any window, smallest |window maximum|) of the
    BatchNorm output a [N, C, H, W] under -inf padding; a window with one tap has an infinite gap."""
    k, st, pd = pool
    N, C = a.shape[:2]
    win = F.unfold(F.pad(a, (pd, pd, pd, pd), value=float("-inf")), k, stride=st).view(N, C, k * k, -1)
    top = win.topk(2, dim=2).values
    return float((top[:, :, 0] - top[:, :, 1]).min()), float(top[:, :, 0].abs().min())


def block_shape(part_elems, C=64):
    """A C-channel [1, C, H, H] shape of at least four partition blocks of part_elems / C input pixels
    with a ragged last one."""
    rpp = part_elems // C
    H = 2
    while H * H < 4 * rpp or H * H % rpp == 0:
        H += 1
    return (1, C, H, H)


def cases(part_elems):
    """name -> ((N, C, H, W), (k, stride, pad), relu, seed, integer). The seeds are chosen on the CPU
    so that the float64 reference's margins() are both >= 1e-5 (except "ties", which ties on
    purpose)."""
    return {
        "clip":       ((2, 8, 5, 6),    (3, 2, 1), True,  1, False),   # windows clipped at both edges, H odd, W even
        "odd":        ((3, 64, 9, 7),   (3, 2, 1), True,  1, False),   # odd H and W
        "one_window": ((1, 64, 2, 2),   (3, 2, 1), True,  1, False),   # one window covers the image
        "disjoint":   ((2, 16, 6, 8),   (2, 2, 0), False, 1, False),   # disjoint windows, no ReLU
        "ties":       ((2, 16, 5, 5),   (3, 1, 1), True,  1, True),    # up to nine windows per pixel, exact ties
        "c2048":      ((3, 2048, 2, 2), (3, 2, 1), True,  1, False),   # the channel maximum
        "blocks":     (block_shape(part_elems), (3, 2, 1), True, 1, False),
    }
