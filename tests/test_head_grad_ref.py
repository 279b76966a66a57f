"""The float64 restatement of the head (tests/head_grad_ref.py) against the REFERENCE module's own
gradients (tests/golden/grad/*.npz, written by tests/golden/grad/make_golden_grad.py from the
reference in train() mode, loss = cross_entropy(Y, target) + auxiliary loss).

Agreement measured here (nrel = max|got - ref| / max|ref|, the reference being fp32): at most
6.8e-6 over every stored quantity of every fixture (dba of grad_N64_sep_t0, a cancelling sum);
gate-side gradients of the one-instance bag are exactly 0 on both sides. The bound is 10x that."""
import glob
import os

import numpy as np
import pytest
import torch

import golden_util
import head_grad_ref as ref
from mcgmil import AuxiliaryLoss, MultiHeadGatedAttentionMIL

GRAD_DIR = os.path.join(golden_util.GOLDEN, "grad")
NAMES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GRAD_DIR, "*.npz")))
BOUND = 6.8e-5


def load(name):
    c = golden_util.Case(os.path.join("grad", name))
    c.target = int(c.z["target"].item())
    return c


def restated_loss(c, dtype):
    """(loss, Y, leaves H + params) of the restatement for fixture case c."""
    H, _, arrays = c.inputs()
    kF, kA = c.masks()
    Ht, = ref.leaf([H], dtype)
    pt = ref.leaf([arrays[k] for k in ref.PARAMS], dtype)
    Y, A = ref.head_forward(Ht, pt, torch.as_tensor(np.asarray(kF)), torch.as_tensor(np.asarray(kA)),
                            c.p_f, c.p_a)
    aux = AuxiliaryLoss("pairwise", margin=1.0, scale=.5)
    loss = torch.nn.functional.cross_entropy(Y, torch.tensor([c.target])) + \
        aux.scale * aux(A[:, 1, :], A[:, 0, :], c.target == 1)
    return loss, Y, [Ht] + pt


def stored_views(g):
    """The restatement's gradients cut down to what a fixture stores."""
    out = {k: g[k] for k in ("dbv", "dbu", "dwa", "dba", "dwk")}
    out["dH"] = g["dH"][:, ::4]
    for w in ("dWv", "dWu"):
        out[w] = g[w][:, ::8, ::8]
        out[w + "_sum1"] = g[w].sum(1)
        out[w + "_sum2"] = g[w].sum(2)
    return out


def test_fixtures_present():
    assert NAMES == ["grad_N130_C3_D64_sep", "grad_N1_sep", "grad_N37_shared", "grad_N64_sep_t0"]
    for n in NAMES:
        assert os.path.getsize(os.path.join(GRAD_DIR, n + ".npz")) < 256 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_gradients(name):
    c = load(name)
    assert c.T == 1
    loss, Y, leaves = restated_loss(c, torch.float64)
    loss.backward()
    g = {k: t.grad.numpy() for k, t in zip(ref.GRADS, leaves)}
    worst = {"Y": golden_util.nrel(Y.detach().numpy(), c.z["Y"]),
             "loss": golden_util.nrel(loss.item(), c.z["loss"])}
    for k, v in stored_views(g).items():
        want = c.z[k]
        assert v.shape == want.shape, k
        if c.N == 1 and k not in ("dH", "dwk"):
            # one instance: the softmax is constant, nothing flows into the gates
            assert not want.any() and not v.any(), k
        worst[k] = golden_util.nrel(v, want)
    print(name, {k: f"{v:.1e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= BOUND}
    assert not bad, bad


def test_training_forward_on_cpu_tensors_still_raises():
    """Opting in to head training does not add a CPU path."""
    class Flatten(torch.nn.Module):
        def forward(self, x):
            return torch.flatten(x, 1)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False).train()
    m.feature_extractor = Flatten()
    with pytest.raises(NotImplementedError):
        m(torch.rand(1, 4, 512, 1, 1), torch.tensor([1]))
    m.enable_head_training()
    with pytest.raises(RuntimeError, match="HIP device only"):
        m(torch.rand(1, 4, 512, 1, 1), torch.tensor([1]))
