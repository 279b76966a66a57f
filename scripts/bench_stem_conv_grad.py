"""Time the stem convolution's training op (torch.ops.mcgmil.stem_conv_f32: the gather-mode fp32
HIP forward and the HIP weight gradient of include/mcgmil_stem_grad.h) against the torch layer on
the same tensors, in one process on one GPU.

(a) Forward + backward of conv1 = Conv2d(3, 64, 7, stride 2, pad 3) on --instances (default 64, 256
and 1507) instances of 3 x 224 x 224, the weight requiring a gradient and the instances not: "op"
(features.run_conv inside native_stem_conv_training()) against "torch" (features.torch_conv under
autograd: MIOpen in batch chunks below 2^31 bytes and a torch.cat), interleaved call by call. Each
call is timed with HIP events: warm-up, then --steps timed calls, median and min-max. The op "wins"
("loses") when the medians differ by more than the larger of the two min-max spreads, else it
"ties". The backward is also timed alone both ways (features.conv2d_f32_stem_wgrad against
aten.convolution_backward in the same chunks), with the kernel's achieved TF/s (2 * 64 * 147 *
pixels) and GB/s (dY and x read once).

(b) A whole training step, forward() + backward() of MultiHeadGatedAttentionMIL (r18, BatchNorm on
batch statistics as the reference's scripts set it, head training on) on one bag of --bags
instances, interleaved: "base" (enable_backbone_training(norm=True, stem=True)) and "stem_conv"
(the same with stem_conv=True), with the peak memory of a step above what is allocated before it.

Prints the tables (markdown) on stderr and one JSON line on stdout.
Usage: python scripts/bench_stem_conv_grad.py [--steps 10] [--warmup 3] [--instances 64,256,1507]
                                              [--bags 64,256,1507] [--no-shapes]
"""
import argparse
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
from mcgmil import MultiHeadGatedAttentionMIL, features, library  # noqa: E402,F401
from mcgmil.resnet import deactivate_batchnorm  # noqa: E402


def bench_layer(n, hw, steps, warmup, dev):
    cl = torch.channels_last
    torch.manual_seed(0)
    conv = nn.Conv2d(3, 64, 7, 2, 3, bias=False).to(dev)
    x = torch.randn(n, 3, hw, hw, device=dev).contiguous(memory_format=cl)
    oh = (hw + 6 - 7) // 2 + 1
    dy = torch.randn(n, 64, oh, oh, device=dev).contiguous(memory_format=cl)

    def fwd_bwd(native):
        conv.weight.grad = None
        with features.native_stem_conv_training(native):
            features.run_conv(conv, x).backward(dy)
    fns = {"op": lambda: fwd_bwd(True), "torch": lambda: fwd_bwd(False),
           "bwd_op": lambda: features.conv2d_f32_stem_wgrad(conv, x, dy),
           "bwd_torch": lambda: features._aten_conv_backward(conv, x, dy, False, True)}
    t = interleaved(fns, steps, warmup)
    pixels = n * oh * oh
    flop, nbytes = 2.0 * 64 * 147 * pixels, 4.0 * (dy.numel() + x.numel())
    rnd = lambda v: [round(c, 4) for c in v]  # noqa: E731
    return {"n": n, "hw": hw, "op_ms": rnd(t["op"]), "torch_ms": rnd(t["torch"]),
            "ratio": round(t["torch"][0] / t["op"][0], 3), "op": verdict(t["op"], t["torch"]),
            "bwd_op_ms": rnd(t["bwd_op"]), "bwd_torch_ms": rnd(t["bwd_torch"]),
            "bwd_ratio": round(t["bwd_torch"][0] / t["bwd_op"][0], 3), "bwd_op": verdict(t["bwd_op"], t["bwd_torch"]),
            "wgrad_tflops": round(flop / t["bwd_op"][0] / 1e9, 2), "wgrad_gbs": round(nbytes / t["bwd_op"][0] / 1e6, 1)}


def train_step(n, steps, warmup, dev):
    torch.manual_seed(0)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(dev)
    m.apply(deactivate_batchnorm)
    m.train().enable_head_training()
    x = torch.rand(1, n, 3, 224, 224, device=dev)
    target = torch.tensor([1], device=dev)

    def step(stem_conv):
        m.enable_backbone_training(True, norm=True, stem=True, stem_conv=stem_conv)
        m.zero_grad(set_to_none=True)
        Y, A, aux = m(x, target, seed=7)
        (F.cross_entropy(Y, target) + aux).backward()
    out = {"instances": n}
    variants = {"base": lambda: step(False), "stem_conv": lambda: step(True)}
    t = interleaved(variants, steps, warmup)
    for key, f in variants.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        out[key + "_ms"] = [round(c, 3) for c in t[key]]
        out[key + "_peak_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
    out["speedup_stem_conv_vs_base"] = round(t["base"][0] / t["stem_conv"][0], 3)
    out["stem_conv_vs_base"] = verdict(t["stem_conv"], t["base"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--instances", default="64,256,1507")
    ap.add_argument("--bags", default="64,256,1507")
    ap.add_argument("--hw", type=int, default=224, help="H = W of an instance")
    ap.add_argument("--no-shapes", action="store_true", help="only the training step")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"bench": "stem_conv_grad", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "layer": [], "train_step": []}
    f = lambda v: f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    print("| n | op fwd+bwd ms (min-max) | torch layer | torch / op | op | wgrad ms | aten backward ms | aten / wgrad | "
          "wgrad | wgrad TF/s | wgrad GB/s |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|---|---|", file=sys.stderr)
    for n in [] if a.no_shapes else [int(v) for v in a.instances.split(",") if v]:
        r = bench_layer(n, a.hw, a.steps, a.warmup, dev)
        out["layer"].append(r)
        print(f"| {n} | {f(r['op_ms'])} | {f(r['torch_ms'])} | {r['ratio']:.2f} | {r['op']} | {f(r['bwd_op_ms'])} | "
              f"{f(r['bwd_torch_ms'])} | {r['bwd_ratio']:.2f} | {r['bwd_op']} | {r['wgrad_tflops']} | {r['wgrad_gbs']} |",
              file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print("| instances | base ms (min-max) | base + stem_conv | base / stem_conv | stem_conv vs base | "
          "peak MiB base / stem_conv |", file=sys.stderr)
    print("|---|---|---|---|---|---|", file=sys.stderr)
    for n in [int(v) for v in a.bags.split(",") if v]:
        r = train_step(n, a.steps, a.warmup, dev)
        out["train_step"].append(r)
        print(f"| {n} | {f(r['base_ms'])} | {f(r['stem_conv_ms'])} | {r['speedup_stem_conv_vs_base']:.3f} | "
              f"{r['stem_conv_vs_base']} | {r['base_peak_mib']} / {r['stem_conv_peak_mib']} |", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
