"""Time one training step of the MIL head (forward + backward from H on) on the HIP op against
PyTorch-ROCm autograd over the fp32 torch restatement, in the same process on the same GPU.

Shapes (L = 512, D = 128, C = 2, p_feat = p_att = 0.1):
  a_sep / a_shared  the reference's training step: one bag of 1,507 instances, T = 1
  b                 net_utils.train_gacc's accumulation as one call: 16 bags of 1,507, T = 1
  c                 4 bags of 1,507, T = 8
Each step is timed with HIP events (warm-up, then >= 20 timed steps, median); the HIP step is also
split into its forward and backward halves and, with torch.profiler, into kernels. Peak memory is
torch.cuda.max_memory_allocated over a step, above what is allocated before it.

Prints one JSON line.  Usage: python scripts/bench_head_grad.py [--steps 30] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-gated-mil_amd"))

from mcgmil import library, ops, synthetic  # noqa: E402,F401

L, D, C, N = 512, 128, 2, 1507
SHAPES = {"a_sep": (1, 1, False), "a_shared": (1, 1, True), "b": (16, 1, False), "c": (4, 8, False)}


def torch_head(H, params, T, pf, pa):
    """The head in torch ops (reference model.py:211-253 for T samples of B bags), fp32."""
    Wv, bv, Wu, bu, wa, ba, wk = params
    B, n, _ = H.shape
    Hd = F.dropout(H.unsqueeze(1).expand(B, T, n, L), pf)
    Ys, As = [], []
    for c in range(C):
        g = c if Wv.shape[0] > 1 else 0
        s = (torch.tanh(F.linear(Hd, Wv[g], bv[g])) * torch.sigmoid(F.linear(Hd, Wu[g], bu[g]))) @ wa[c] + ba[c]
        A = torch.softmax(F.dropout(s, pa), dim=-1)                       # [B, T, n]
        Ys.append((A.unsqueeze(-2) @ Hd).squeeze(-2) @ wk[c])             # [B, T]
        As.append(A)
    return torch.stack(Ys, -1), torch.stack(As, 2)                        # [B, T, C], [B, T, C, n]


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), torch.cuda.max_memory_allocated() - base


def kernel_times(step):
    """Mean device time per step of each kernel (microseconds), by name, largest first."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                step()
            torch.cuda.synchronize()
        rows = [(e.key.split("(")[0][:60], getattr(e, "device_time_total", 0.0) / 5) for e in prof.key_averages()]
        return {k: round(v, 1) for k, v in sorted(rows, key=lambda r: -r[1])[:8] if v > 0}
    except Exception as e:     # the profiler is optional: the step times above do not depend on it
        return {"unavailable": repr(e)[:80]}


def bench(name, steps, warmup, dev):
    B, T, shared = SHAPES[name]
    sd = synthetic.head_state_dict(3, L=L, D=D, C=C, shared=shared)
    arrays = synthetic.head_arrays(sd, C, shared)
    params = [torch.from_numpy(arrays[k].copy()).to(dev).requires_grad_(True) for k in ops.HeadTensors._fields]
    H = torch.from_numpy(synthetic.bag_features(4, B * N, L)).to(dev).requires_grad_(True)
    offs = ops.uniform_offsets(N, B, dev)
    dY = torch.randn(B, T, C, device=dev)
    dA = torch.randn(T * C * B * N, device=dev)
    seed = [0]

    def clear():
        for t in [H] + params:
            t.grad = None

    def hip_step():
        clear()
        seed[0] += 1
        Y, A = torch.ops.mcgmil.mcdo_forward(H, offs, *params, T, 0.1, 0.1, seed[0], 0, 0)
        ((Y * dY).sum() + (A * dA).sum()).backward()

    def torch_step():
        clear()
        Y, A = torch_head(H.view(B, N, L), params, T, 0.1, 0.1)
        ((Y * dY).sum() + (A * dA.view(B, T, C, N)).sum()).backward()

    hip_ms, hip_mem = timed(hip_step, steps, warmup)
    torch_ms, torch_mem = timed(torch_step, steps, warmup)
    # the HIP step's halves, by themselves
    head = ops.HeadTensors(*[p.detach() for p in params])
    Hn = H.detach()
    fwd = ops.mcdo_forward(Hn, offs, head, T, p_feat=0.1, p_att=0.1, seed=1)
    kw = dict(p_feat=0.1, p_att=0.1, seed=1)
    fwd_ms, _ = timed(lambda: ops.mcdo_forward(Hn, offs, head, T, **kw), steps, warmup)
    bwd_ms, _ = timed(lambda: ops.mcdo_backward(Hn, offs, head, T, fwd["A"], fwd["Y"], dY, dA, **kw), steps, warmup)
    bwd_nodh_ms, _ = timed(lambda: ops.mcdo_backward(Hn, offs, head, T, fwd["A"], fwd["Y"], dY, dA, need_dH=False, **kw),
                           steps, warmup)
    return {"B": B, "T": T, "N": N, "shared": shared, "hip_ms": round(hip_ms, 4), "torch_ms": round(torch_ms, 4),
            "speedup": round(torch_ms / hip_ms, 3), "hip_peak_mib": round(hip_mem / 2**20, 1),
            "torch_peak_mib": round(torch_mem / 2**20, 1), "hip_fwd_ms": round(fwd_ms, 4),
            "hip_bwd_ms": round(bwd_ms, 4), "hip_bwd_no_dH_ms": round(bwd_nodh_ms, 4),
            "hip_kernels_us": kernel_times(hip_step)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps must be >= 20")
    dev = torch.device("cuda", 0)
    out = {"bench": "head_grad", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "L": L, "D": D, "C": C}
    for name in a.shapes.split(","):
        out[name] = bench(name, a.steps, a.warmup, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
