"""Time the stem's fused BatchNorm/ReLU/max-pool training op (torch.ops.mcgmil.bn_pool_f32: the
fused HIP forward that records the pool's argmax codes and the HIP backward of
include/mcgmil_pool_grad.h) against the torch layers on the same tensors, in one process on one GPU.

(a) Forward + backward of maxpool(relu(bn(z))) on the stem activation [n, 64, 112, 112] at
--instances (default 64 and 256), z and the BN parameters requiring gradients: "op"
(features.bn_act inside native_stem_training()) against "torch" (batch_norm, relu, max_pool2d
under autograd), interleaved call by call. Each call is timed with HIP events: warm-up, then
--steps timed calls, median and min-max. The op "wins" ("loses") when the medians differ by more
than the larger of the two min-max spreads, else it "ties". The forward and the two backward passes
are also timed alone through the python entry points / the C ABI (a call that asks for dgamma /
dbeta only runs the partial-sum pass and the small finalize; the apply pass is the difference to
the full call), with the bytes of z that each moves per second, and the bytes autograd saves for
either route.

(b) A whole training step, forward() + backward() of MultiHeadGatedAttentionMIL (r18, BatchNorm on
batch statistics as the reference's scripts set it, head training on) on one bag of --bags
instances, interleaved: "norm" (enable_backbone_training(norm=True): the baseline) and "stem"
(enable_backbone_training(norm=True, stem=True)), with the peak memory of a step above what is
allocated before it.

Prints the tables (markdown) on stderr and one JSON line on stdout.
Usage: python scripts/bench_stem_grad.py [--steps 10] [--warmup 3] [--instances 64,256]
                                         [--bags 64,256,1507] [--no-shapes]
"""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-gated-mil_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_norm_grad import interleaved, verdict  # noqa: E402
from mcgmil import MultiHeadGatedAttentionMIL, _lib, features, library  # noqa: E402,F401
from mcgmil.resnet import deactivate_batchnorm  # noqa: E402

POOL = (3, 2, 1)


def capi_backward(L, z, code, dy, gamma, mean, invstd, outs, ws):
    a = _lib.BnPoolGradArgs()
    a.batch, a.channels, a.height, a.width = z.shape
    a.pool_kernel, a.pool_stride, a.pool_pad = POOL
    a.pooled_height, a.pooled_width = dy.shape[2:]
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a.z, a.argmax, a.dy, a.gamma, a.mean, a.invstd = p(z), p(code), p(dy), p(gamma), p(mean), p(invstd)
    a.dz, a.dgamma, a.dbeta = (p(outs.get(k)) for k in ("dz", "dgamma", "dbeta"))
    a.workspace, a.workspace_bytes = p(ws), ws.numel()
    rc = L.mcgmil_batchnorm_pool_backward(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc:
        raise RuntimeError(f"mcgmil_batchnorm_pool_backward failed ({rc}): {L.mcgmil_last_error().decode()}")


def bench_shape(n, hw, steps, warmup, dev):
    C, cl = 64, torch.channels_last
    bn = nn.BatchNorm2d(C).to(dev)
    deactivate_batchnorm(bn)
    pool = nn.MaxPool2d(*POOL)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    z = torch.randn(n, C, hw, hw, device=dev).contiguous(memory_format=cl).requires_grad_()
    ph = (hw + 2 * POOL[2] - POOL[0]) // POOL[1] + 1
    dy = torch.randn(n, C, ph, ph, device=dev).contiguous(memory_format=cl)

    def fwd_bwd(native):
        for t in (z, bn.weight, bn.bias):
            t.grad = None
        with features.native_stem_training(native):
            features.bn_act(bn, z, True, pool=pool).backward(dy)

    def saved(native):
        seen = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: seen.append(t.numel() * t.element_size()) or t,
                                                      lambda t: t), features.native_stem_training(native):
            features.bn_act(bn, z, True, pool=pool)
        return sum(seen)
    w, b = bn.weight.detach(), bn.bias.detach()
    with torch.no_grad():
        y, mean, invstd, code = features.batchnorm_pool_stats(z.detach(), w, b, bn.eps, True, *POOL)
    L = _lib.load()
    a = _lib.BnPoolGradArgs()
    a.batch, a.channels, a.height, a.width = z.shape
    a.pool_kernel, a.pool_stride, a.pool_pad = POOL
    a.pooled_height, a.pooled_width = ph, ph
    nbytes = ctypes.c_size_t()
    _lib.check(L.mcgmil_bn_pool_grad_workspace_size(ctypes.byref(a), ctypes.byref(nbytes)),
               "mcgmil_bn_pool_grad_workspace_size")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    full = {"dz": torch.empty_like(z), "dgamma": torch.empty_like(mean), "dbeta": torch.empty_like(mean)}
    stats = {"dgamma": full["dgamma"], "dbeta": full["dbeta"]}
    args = (z.detach(), code, dy, w, mean, invstd)
    fns = {"op": lambda: fwd_bwd(True), "torch": lambda: fwd_bwd(False),
           "fwd": lambda: features.batchnorm_pool_stats(z.detach(), w, b, bn.eps, True, *POOL),
           "bwd_full": lambda: capi_backward(L, *args, full, ws), "bwd_stats": lambda: capi_backward(L, *args, stats, ws)}
    t = interleaved(fns, steps, warmup)
    unit = z.numel() * 4
    apply_ms = t["bwd_full"][0] - t["bwd_stats"][0]
    rnd = lambda v: [round(c, 4) for c in v]  # noqa: E731
    return {"n": n, "C": C, "hw": hw, "op_ms": rnd(t["op"]), "torch_ms": rnd(t["torch"]),
            "ratio": round(t["torch"][0] / t["op"][0], 3), "op": verdict(t["op"], t["torch"]),
            "fwd_ms": rnd(t["fwd"]), "bwd_full_ms": rnd(t["bwd_full"]), "bwd_stats_ms": rnd(t["bwd_stats"]),
            # bytes of z (and dz) alone, per second: the forward reads z twice, the partial pass once,
            # the apply pass reads z and writes dz
            "fwd_z_tbs": round(2 * unit / t["fwd"][0] / 1e9, 2), "partial_z_tbs": round(unit / t["bwd_stats"][0] / 1e9, 2),
            "apply_z_tbs": round(2 * unit / apply_ms / 1e9, 2) if apply_ms > 0 else None,
            "saved_op_mib": round(saved(True) / 2**20, 1), "saved_torch_mib": round(saved(False) / 2**20, 1)}


def train_step(n, steps, warmup, dev):
    torch.manual_seed(0)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(dev)
    m.apply(deactivate_batchnorm)
    m.train().enable_head_training()
    x = torch.rand(1, n, 3, 224, 224, device=dev)
    target = torch.tensor([1], device=dev)

    def step(stem):
        m.enable_backbone_training(True, norm=True, stem=stem)
        m.zero_grad(set_to_none=True)
        Y, A, aux = m(x, target, seed=7)
        (F.cross_entropy(Y, target) + aux).backward()
    out = {"instances": n}
    variants = {"norm": lambda: step(False), "stem": lambda: step(True)}
    t = interleaved(variants, steps, warmup)
    for key, f in variants.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        out[key + "_ms"] = [round(c, 3) for c in t[key]]
        out[key + "_peak_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
    out["speedup_stem_vs_norm"] = round(t["norm"][0] / t["stem"][0], 3)
    out["stem_vs_norm"] = verdict(t["stem"], t["norm"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--instances", default="64,256")
    ap.add_argument("--bags", default="64,256,1507")
    ap.add_argument("--hw", type=int, default=112, help="H = W of the stem activation (112 at 224 x 224 instances)")
    ap.add_argument("--no-shapes", action="store_true", help="only the training step")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"bench": "stem_grad", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "shapes": [], "train_step": []}
    f = lambda v: f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    print("| n | op fwd+bwd ms (min-max) | torch layers | torch / op | op | forward ms | backward ms | stats-only ms | "
          "forward / partial / apply TB/s of z | saved MiB op / torch |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|---|", file=sys.stderr)
    for n in [] if a.no_shapes else [int(v) for v in a.instances.split(",") if v]:
        r = bench_shape(n, a.hw, a.steps, a.warmup, dev)
        out["shapes"].append(r)
        print(f"| {n} | {f(r['op_ms'])} | {f(r['torch_ms'])} | {r['ratio']:.2f} | {r['op']} | {f(r['fwd_ms'])} | "
              f"{f(r['bwd_full_ms'])} | {f(r['bwd_stats_ms'])} | {r['fwd_z_tbs']} / {r['partial_z_tbs']} / {r['apply_z_tbs']} | "
              f"{r['saved_op_mib']} / {r['saved_torch_mib']} |", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print("| instances | norm ms (min-max) | norm + stem | norm / stem | stem vs norm | peak MiB norm / stem |", file=sys.stderr)
    print("|---|---|---|---|---|---|", file=sys.stderr)
    for n in [int(v) for v in a.bags.split(",") if v]:
        r = train_step(n, a.steps, a.warmup, dev)
        out["train_step"].append(r)
        print(f"| {n} | {f(r['norm_ms'])} | {f(r['stem_ms'])} | {r['speedup_stem_vs_norm']:.3f} | {r['stem_vs_norm']} | "
              f"{r['norm_peak_mib']} / {r['stem_peak_mib']} |", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
