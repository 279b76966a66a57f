"""Time the fused BatchNorm/add/ReLU training op (torch.ops.mcgmil.bn_act_f32: the fused HIP
forward and the HIP backward of include/mcgmil_bn_grad.h) against the torch layers on the same
tensors, in one process on one GPU.

Per BatchNorm shape of the ResNet-18 blocks at --instances (default 64 and 256) instances of
224 x 224, forward + backward of relu(bn(x) + r) and of relu(bn(x)), x / r / the BN parameters
requiring gradients: "op" (features.bn_act inside native_norm_training()) against "torch"
(bn(x), + r, torch.relu), interleaved call by call. Each call is timed with HIP events: warm-up,
then --steps timed calls, median and min-max. The op "wins" ("loses") when the medians differ by
more than the larger of the two min-max spreads, else it "ties".
The two new kernels' achieved bandwidth comes from two calls of the C ABI on the same tensors: one
that asks for dgamma / dbeta only (bn_grad_partial_kernel + the small finalize: reads x, dy and,
with ReLU, y) and the full call; the apply pass (reads the same, writes dx and, with a residual,
dresidual) is the difference. With --ab-lib PATH (a build of the library with other compile
switches, e.g. -DMCGMIL_BN_GRAD_NT=0) the full call of that build is timed in the same round-robin.

Then a whole training step, forward() + backward() of MultiHeadGatedAttentionMIL (r18, BatchNorm
on batch statistics as the reference's scripts set it, head training on) on one bag of --bags
instances, interleaved: "off" (torch layers), "on" (enable_backbone_training(): the baseline) and
"norm" (enable_backbone_training(norm=True)), with the peak memory of a step above what is
allocated before it.

Prints the tables (markdown) on stderr and one JSON line on stdout.
Usage: python scripts/bench_norm_grad.py [--steps 10] [--warmup 3] [--instances 64,256]
                                         [--bags 64,256,1507] [--no-shapes] [--ab-lib PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-gated-mil_amd"))

from mcgmil import MultiHeadGatedAttentionMIL, _lib, features, library  # noqa: E402,F401
from mcgmil.resnet import deactivate_batchnorm  # noqa: E402

# (name, C, H = W of the BatchNorm's input at 224 x 224 instances, with residual / without in r18)
R18 = [("layer1", 64, 56, 4, 4), ("layer2", 128, 28, 4, 5), ("layer3", 256, 14, 4, 5), ("layer4", 512, 7, 4, 5)]


def interleaved(fns, steps, warmup):
    """{name: (median, min, max) ms} of the calls in fns, run round-robin."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(steps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def capi_backward(L, x, y, dy, gamma, mean, invstd, relu, outs, ws):
    a = _lib.BnGradArgs()
    a.rows, a.channels, a.relu = x.numel() // x.shape[1], x.shape[1], int(relu)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a.x, a.y, a.dy, a.gamma, a.mean, a.invstd = p(x), p(y), p(dy), p(gamma), p(mean), p(invstd)
    a.dx, a.dresidual, a.dgamma, a.dbeta = (p(outs.get(k)) for k in ("dx", "dres", "dgamma", "dbeta"))
    a.workspace, a.workspace_bytes = p(ws), ws.numel()
    rc = L.mcgmil_batchnorm_act_backward(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc:
        raise RuntimeError(f"mcgmil_batchnorm_act_backward failed ({rc}): {L.mcgmil_last_error().decode()}")


def verdict(a, b):
    """"wins" / "loses" / "ties" of a against b, (median, min, max) each."""
    spread = max(a[2] - a[1], b[2] - b[1])
    return "wins" if b[0] - a[0] > spread else "loses" if a[0] - b[0] > spread else "ties"


def bench_shape(shape, n, res, steps, warmup, dev, ab):
    name, C, hw, _, _ = shape
    cl = torch.channels_last
    bn = nn.BatchNorm2d(C).to(dev)
    deactivate_batchnorm(bn)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    x = torch.randn(n, C, hw, hw, device=dev).contiguous(memory_format=cl).requires_grad_()
    r = torch.randn(n, C, hw, hw, device=dev).contiguous(memory_format=cl).requires_grad_() if res else None
    dy = torch.randn(n, C, hw, hw, device=dev).contiguous(memory_format=cl)

    def fwd_bwd(native):
        for t in (x, r, bn.weight, bn.bias):
            if t is not None:
                t.grad = None
        with features.native_norm_training(native):
            features.bn_act(bn, x, True, r).backward(dy)
    with torch.no_grad():
        y, mean, invstd = features.batchnorm_act_stats(x.detach(), bn.weight.detach(), bn.bias.detach(),
                                                       None if r is None else r.detach(), bn.eps, True)
    L = _lib.load()
    a = _lib.BnGradArgs()
    a.rows, a.channels = x.numel() // C, C
    nbytes = ctypes.c_size_t()
    _lib.check(L.mcgmil_bn_grad_workspace_size(ctypes.byref(a), ctypes.byref(nbytes)), "mcgmil_bn_grad_workspace_size")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    full = {"dx": torch.empty_like(y), "dgamma": torch.empty_like(mean), "dbeta": torch.empty_like(mean)}
    if res:
        full["dres"] = torch.empty_like(y)
    stats = {"dgamma": full["dgamma"], "dbeta": full["dbeta"]}
    args = (x.detach(), y, dy, bn.weight.detach(), mean, invstd, True)
    fns = {"op": lambda: fwd_bwd(True), "torch": lambda: fwd_bwd(False),
           "bwd_full": lambda: capi_backward(L, *args, full, ws), "bwd_stats": lambda: capi_backward(L, *args, stats, ws)}
    if ab is not None:
        fns["bwd_full_ab"] = lambda: capi_backward(ab, *args, full, ws)
    t = interleaved(fns, steps, warmup)
    unit = x.numel() * 4
    apply_ms = t["bwd_full"][0] - t["bwd_stats"][0]
    rnd = lambda v: [round(c, 4) for c in v]  # noqa: E731
    out = {"shape": name, "C": C, "hw": hw, "n": n, "residual": bool(res), "op_ms": rnd(t["op"]), "torch_ms": rnd(t["torch"]),
           "ratio": round(t["torch"][0] / t["op"][0], 3), "op": verdict(t["op"], t["torch"]),
           "bwd_full_ms": rnd(t["bwd_full"]), "bwd_stats_ms": rnd(t["bwd_stats"]),
           "partial_tbs": round(3 * unit / t["bwd_stats"][0] / 1e9, 2),
           "apply_tbs": round((3 + (2 if res else 1)) * unit / apply_ms / 1e9, 2) if apply_ms > 0 else None}
    if ab is not None:
        out["bwd_full_ab_ms"] = rnd(t["bwd_full_ab"])
        out["ab"] = verdict(t["bwd_full"], t["bwd_full_ab"])
    return out


def train_step(n, steps, warmup, dev):
    torch.manual_seed(0)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(dev)
    m.apply(deactivate_batchnorm)
    m.train().enable_head_training()
    x = torch.rand(1, n, 3, 224, 224, device=dev)
    target = torch.tensor([1], device=dev)

    def step(flag, norm=False):
        m.enable_backbone_training(flag, norm=norm)
        m.zero_grad(set_to_none=True)
        Y, A, aux = m(x, target, seed=7)
        (F.cross_entropy(Y, target) + aux).backward()
    out = {"instances": n}
    variants = {"off": lambda: step(False), "on": lambda: step(True), "norm": lambda: step(True, True)}
    t = interleaved(variants, steps, warmup)
    for key, f in variants.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        out[key + "_ms"] = [round(c, 3) for c in t[key]]
        out[key + "_peak_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
    out["speedup_norm_vs_on"] = round(t["on"][0] / t["norm"][0], 3)
    out["norm_vs_on"] = verdict(t["norm"], t["on"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--instances", default="64,256")
    ap.add_argument("--bags", default="64,256,1507")
    ap.add_argument("--no-shapes", action="store_true", help="only the training step")
    ap.add_argument("--ab-lib", default=None, help="a second build of the library for the backward A/B")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ab = _lib.bind(a.ab_lib) if a.ab_lib else None
    out = {"bench": "norm_grad", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "ab_lib": os.path.basename(a.ab_lib) if a.ab_lib else None, "shapes": [], "train_step": []}
    f = lambda v: f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    print("| shape | n | residual | op fwd+bwd ms (min-max) | torch layers | torch / op | op | backward ms | "
          "stats-only ms | partial TB/s | apply TB/s |" + (" A/B build backward ms | default vs A/B |" if ab else ""),
          file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|---|---|" + ("---|---|" if ab else ""), file=sys.stderr)
    for n in [] if a.no_shapes else [int(v) for v in a.instances.split(",") if v]:
        for shape in R18:
            for res in (True, False):
                r = bench_shape(shape, n, res, a.steps, a.warmup, dev, ab)
                out["shapes"].append(r)
                print(f"| {r['shape']} {r['C']} x {r['hw']}^2 | {n} | {'yes' if res else 'no'} | {f(r['op_ms'])} | "
                      f"{f(r['torch_ms'])} | {r['ratio']:.2f} | {r['op']} | {f(r['bwd_full_ms'])} | {f(r['bwd_stats_ms'])} | "
                      f"{r['partial_tbs']} | {r['apply_tbs']} |" +
                      (f" {f(r['bwd_full_ab_ms'])} | {r['ab']} |" if ab else ""), file=sys.stderr, flush=True)
    print("| instances | off ms (min-max) | on | norm | on / norm | norm vs on | peak MiB off / on / norm |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|", file=sys.stderr)
    for n in [int(v) for v in a.bags.split(",") if v]:
        r = train_step(n, a.steps, a.warmup, dev)
        out["train_step"].append(r)
        print(f"| {n} | {f(r['off_ms'])} | {f(r['on_ms'])} | {f(r['norm_ms'])} | {r['speedup_norm_vs_on']:.3f} | "
              f"{r['norm_vs_on']} | {r['off_peak_mib']} / {r['on_peak_mib']} / {r['norm_peak_mib']} |",
              file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
