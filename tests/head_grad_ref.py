"""A torch restatement of the MIL head's forward with explicit dropout masks (reference
model.py:211-253 from H on, for T samples of one bag), in whatever dtype its inputs have. Its
autograd gradients are the reference for the HIP backward pass (tests/test_gpu_head_grad.py) and
are themselves pinned to the reference module's (tests/test_head_grad_ref.py)."""
import numpy as np
import torch

from oracle import philox

PARAMS = ("Wv", "bv", "Wu", "bu", "wa", "ba", "wk")
GRADS = ("dH",) + tuple("d" + n for n in PARAMS)


def head_forward(H, params, keepF, keepA, p_f, p_a):
    """H [N, L]; params = (Wv [G,D,L], bv [G,D], Wu, bu, wa [C,D], ba [C], wk [C,L]);
    keepF [T, N, L], keepA [T, C, N] (0/1)  ->  Y [T, C], A [T, C, N]."""
    Wv, bv, Wu, bu, wa, ba, wk = params
    G, C = Wv.shape[0], wa.shape[0]
    dt = H.dtype
    sf = torch.tensor(philox.dropout_scale(p_f), dtype=torch.float32).to(dt)
    sa = torch.tensor(philox.dropout_scale(p_a), dtype=torch.float32).to(dt)
    Hd = H.unsqueeze(0) * (keepF.to(dt) * sf)                                   # [T, N, L]
    V = torch.tanh(torch.einsum("tnl,gdl->tgnd", Hd, Wv) + bv[None, :, None, :])
    U = torch.sigmoid(torch.einsum("tnl,gdl->tgnd", Hd, Wu) + bu[None, :, None, :])
    gate = [c if G > 1 else 0 for c in range(C)]
    s = torch.einsum("tcnd,cd->tcn", (V * U)[:, gate], wa) + ba[None, :, None]
    A = torch.softmax(s * (keepA.to(dt) * sa), dim=-1)                          # [T, C, N]
    Y = (torch.einsum("tcn,tnl->tcl", A, Hd) * wk[None]).sum(-1)                # [T, C]
    return Y, A


def leaf(arrays, dtype):
    return [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in arrays]


def batch_grads(H, sizes, params, keepF_bags, keepA_bags, p_f, p_a, dY, dA_bags, dtype):
    """Gradients of sum(Y * dY) + sum(A * dA) over a batch of bags (rows of H split by `sizes`),
    T samples each: dict of numpy float64 arrays named as GRADS. keepF_bags[b] [T, N_b, L],
    keepA_bags[b] [T, C, N_b]; dY [B, T, C]; dA_bags[b] [T, C, N_b] or None."""
    Ht, = leaf([H], dtype)
    pt = leaf(params, dtype)
    loss, o, Ys, As = 0, 0, [], []
    for b, n in enumerate(sizes):
        Y, A = head_forward(Ht[o:o + n], pt, torch.as_tensor(keepF_bags[b]),
                            torch.as_tensor(keepA_bags[b]), p_f, p_a)
        loss = loss + (Y * torch.as_tensor(dY[b], dtype=dtype)).sum()
        if dA_bags is not None:
            loss = loss + (A * torch.as_tensor(dA_bags[b], dtype=dtype)).sum()
        Ys.append(Y.detach())
        As.append(A.detach())
        o += n
    loss.backward()
    out = {"dH": Ht.grad}
    out.update({"d" + k: t.grad for k, t in zip(PARAMS, pt)})
    out = {k: (torch.zeros_like(t) if v is None else v).double().numpy()
           for (k, v), t in zip(out.items(), [Ht] + pt)}
    return out, Ys, As


def grad_errors(got, ref):
    """Per tensor k: max|got - ref| / max(max|ref_k|, 1e-3 max_j max|ref_j|)."""
    top = max(float(np.max(np.abs(v))) if v.size else 0.0 for v in ref.values())
    err = {}
    for k, r in ref.items():
        if k not in got:
            continue
        den = max(float(np.max(np.abs(r))) if r.size else 0.0, 1e-3 * top)
        g = np.asarray(got[k], dtype=np.float64).reshape(r.shape)
        err[k] = float(np.max(np.abs(g - r)) / den) if r.size and den > 0 else 0.0
    return err
