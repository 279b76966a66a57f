"""Generate the gradient fixtures tests/golden/grad/*.npz from the REFERENCE module itself.

Runs only where the read-only reference checkout exists (see tests/golden/make_golden.py, whose
torchvision stand-in, build_reference and ReplayDropout it reuses). The reference module runs in
train() mode on one bag with the build's Philox masks queued (keepF[0] as [N, L], keepA[0, i] as
[1, 1, N], bag counter 0 as the module's forward() draws them); the loss is cross_entropy(Y, target) + auxiliary loss, then backward().

Fixture contents: metadata, target, Y, the loss and the eight gradients in kernel layout. To stay
small, dWv / dWu are stored as [:, ::8, ::8] plus their sums over each of the two axes, dH as
[:, ::4]. Inputs, weights and masks are regenerated from the seeds (tests/golden_util.py). The
archives are written with fixed zip timestamps, so a rerun reproduces them byte for byte.

Usage:  python tests/golden/grad/make_golden_grad.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))

import make_golden as mg  # noqa: E402  (also puts the repository and the package on sys.path)
from make_golden import philox, synthetic  # noqa: E402


def save_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())


def run_case(name, *, N, target, C=2, shared=False, p_f=0.1, p_a=0.1, D=128, L=512, h_seed, w_seed,
             mask_seed, bag_ctr=0):
    H = synthetic.bag_features(h_seed, N, L)
    sd = synthetic.head_state_dict(w_seed, L=L, D=D, C=C, shared=shared)
    m = mg.build_reference(C, shared, sd, p_f, p_a, D=D)
    m.train()
    x = torch.from_numpy(H).view(1, N, L, 1, 1).requires_grad_(True)
    keepF = torch.from_numpy(philox.feature_keep(mask_seed, bag_ctr, 1, N, L, p_f))
    keepA = torch.from_numpy(philox.attention_keep(mask_seed, bag_ctr, 1, C, N, p_a))
    m.feature_dropout.queue = [keepF[0]]
    for i in range(C):
        m.attention_dropouts[i].queue = [keepA[0, i].view(1, 1, N)]
    t = torch.tensor([target])
    Y, A, aux = m(x, t)
    loss = torch.nn.functional.cross_entropy(Y, t) + aux
    loss.backward()
    G = 1 if shared else C
    lv = [m.attention_V[0]] if shared else [m.attention_V[g][0] for g in range(G)]
    lu = [m.attention_U[0]] if shared else [m.attention_U[g][0] for g in range(G)]
    dWv = torch.stack([q.weight.grad for q in lv]).numpy()
    dWu = torch.stack([q.weight.grad for q in lu]).numpy()
    meta = dict(N=N, T=1, C=C, L=L, D=D, shared=int(shared), p_f=p_f, p_a=p_a, h_seed=h_seed,
                w_seed=w_seed, mask_seed=mask_seed, bag_ctr=bag_ctr, bf16=0)
    out = {k: np.asarray(v) for k, v in meta.items()}
    out.update(
        target=np.asarray(target), Y=Y.detach().numpy(), loss=loss.detach().numpy(),
        dH=x.grad.view(N, L).numpy()[:, ::4],
        dWv=dWv[:, ::8, ::8], dWv_sum1=dWv.sum(1), dWv_sum2=dWv.sum(2),
        dWu=dWu[:, ::8, ::8], dWu_sum1=dWu.sum(1), dWu_sum2=dWu.sum(2),
        dbv=torch.stack([q.bias.grad for q in lv]).numpy(),
        dbu=torch.stack([q.bias.grad for q in lu]).numpy(),
        dwa=torch.cat([q.weight.grad for q in m.attention_weights]).numpy(),
        dba=torch.cat([q.bias.grad for q in m.attention_weights]).numpy(),
        dwk=torch.cat([q.weight.grad for q in m.classifiers]).numpy())
    path = os.path.join(OUT, name + ".npz")
    save_npz(path, out)
    print(f"{name}: loss {float(loss.detach()):.6f} -> {os.path.getsize(path)} B")


def main():
    if not os.path.isdir(mg.REF):
        raise SystemExit("make_golden_grad.py needs the reference checkout")
    mg._install_torchvision_standin()
    torch.set_num_threads(8)
    torch.use_deterministic_algorithms(True)
    run_case("grad_N1_sep", N=1, target=1, h_seed=60, w_seed=61, mask_seed=62)
    run_case("grad_N37_shared", N=37, target=1, shared=True, h_seed=63, w_seed=64, mask_seed=65)
    run_case("grad_N64_sep_t0", N=64, target=0, h_seed=66, w_seed=67, mask_seed=68)
    run_case("grad_N130_C3_D64_sep", N=130, target=1, C=3, D=64, h_seed=69, w_seed=70, mask_seed=71)


if __name__ == "__main__":
    main()
