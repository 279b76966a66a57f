"""Time the direct bf16 convolution data gradient (features.conv2d_bf16_dgrad_direct,
include/mcgmil_conv_dgrad_bf16.h) against aten.convolution_backward on bf16 tensors (MIOpen) and,
for stride 1, against the flipped-forward route (features.conv2d_bf16_dgrad), in one process on one
GPU. The protocol of scripts/bench_conv_dgrad.py: HIP events, --warmup warm-up calls then --steps
timed calls per entry, variants interleaved call by call, median (min-max), instances of 224 x 224.

Per convolution shape of ResNet-18 (and, with --r50, the bottleneck shapes of ResNet-50) at
--instances instances: the direct kernel including the torch cast and permute of the fp32 master
weight, aten's bf16 data gradient (output_mask [True, False, False]) on the weight cast as autocast
casts it, for stride 1 the flipped-forward route, and the direct kernel's TF/s. "wins" / "loses"
only when the medians differ by more than the larger of the two min-max spreads, else "ties".

Then a whole training step, forward() + backward() of MultiHeadGatedAttentionMIL (r18, BatchNorm
on batch statistics as the reference's scripts set it, head training on) on one bag of --bags
instances on the backward routes MCGMIL_CONV_GRAD=native and direct, interleaved, in two
configurations: "d" enable_bf16_backbone_training() alone, "i" all four bf16 opt-ins
(+ enable_bf16_norm_training, enable_bf16_stem_training, enable_bf16_stem_conv_training). Per
route: step time, the peak memory of a step above what is allocated before it, and whether two
consecutive steps from identical state give bitwise-equal .grad on every parameter (reported, not
asserted).

Prints the per-shape table (markdown) on stderr and one JSON line on stdout.
Usage: python scripts/bench_conv_dgrad_bf16.py [--steps 10] [--warmup 3] [--instances 64,256,1507]
                                               [--bags 64,256,1507] [--r50] [--no-shapes]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-gated-mil_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_backbone_grad import R18, R50, interleaved  # noqa: E402
from bench_conv_dgrad import verdict  # noqa: E402
from mcgmil import MultiHeadGatedAttentionMIL, features, library  # noqa: E402,F401
from mcgmil.resnet import deactivate_batchnorm  # noqa: E402

ROUTES = ("native", "direct")
BF = torch.bfloat16


def bench_shape(shape, n, steps, warmup, dev):
    name, cin, cout, k, s, p, hw, count = shape
    cl = torch.channels_last
    x = torch.empty(n, cin, hw, hw, device=dev, dtype=BF).contiguous(memory_format=cl)
    conv = features._ConvShim(torch.randn(cout, cin, k, k, device=dev) / (cin * k * k) ** 0.5, s, p)   # fp32 master
    oh = (hw + 2 * p - k) // s + 1
    dy = torch.randn(n, cout, oh, oh, device=dev).to(BF).contiguous(memory_format=cl)

    def aten():
        w = conv.weight.detach().to(BF)
        return torch.ops.aten.convolution_backward(dy, x, w, None, [s, s], [p, p], [1, 1], False, [0, 0], 1,
                                                   [True, False, False])
    if x.numel() * 2 >= 2 ** 31 or not features.dgrad_bf16_direct_supported(conv, dy):   # dX or dY of 2 GiB or more
        return {"shape": name, "n": n, "count": count, "stride": s, "direct_ms": None}
    fns = {"direct": lambda: features.conv2d_bf16_dgrad_direct(conv, dy, x.shape), "aten": aten}
    if features.dgrad_bf16_native(conv, dy):
        fns["flipped"] = lambda: features.conv2d_bf16_dgrad(conv, dy, x)
    t = interleaved(fns, steps, warmup)
    flops = 2.0 * n * oh * oh * cout * cin * k * k
    r = lambda v: [round(c, 4) for c in v]  # noqa: E731
    flipped = t.get("flipped")
    return {"shape": name, "n": n, "count": count, "stride": s, "direct_ms": r(t["direct"]), "aten_ms": r(t["aten"]),
            "flipped_ms": r(flipped) if flipped else None,
            "direct_tflops": round(flops / t["direct"][0] / 1e9, 1), "vs_aten": verdict(t["direct"], t["aten"]),
            "vs_flipped": verdict(t["direct"], flipped) if flipped else None}


def train_step(config, n, steps, warmup, dev):
    torch.manual_seed(0)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(dev)
    m.apply(deactivate_batchnorm)          # BatchNorm on batch statistics, as the reference's scripts set it
    m.train().enable_head_training().enable_bf16_backbone_training()
    if config == "i":
        m.enable_bf16_norm_training().enable_bf16_stem_training().enable_bf16_stem_conv_training()
    x = torch.rand(1, n, 3, 224, 224, device=dev)
    target = torch.tensor([1], device=dev)

    def step(route):
        os.environ["MCGMIL_CONV_GRAD"] = route
        m.zero_grad(set_to_none=True)
        Y, A, aux = m(x, target, seed=7)
        (F.cross_entropy(Y.float(), target) + aux.float()).backward()

    def grads():
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    out = {"config": config, "instances": n}
    variants = {route: (lambda route=route: step(route)) for route in ROUTES}
    t = interleaved(variants, steps, warmup)
    for route, f in variants.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        out[route + "_ms"] = [round(c, 3) for c in t[route]]
        out[route + "_peak_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
        first = grads()
        f()                                  # the parameters did not move: identical state
        second = grads()
        differ = sorted(k for k in first if not torch.equal(first[k], second[k]))
        out[route + "_grads_bitwise_equal"] = not differ and first.keys() == second.keys()
        out[route + "_grads_differing"] = len(differ)
        del first, second
    out["direct_vs_native"] = verdict(t["direct"], t["native"])
    os.environ.pop("MCGMIL_CONV_GRAD", None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--instances", default="64,256,1507")
    ap.add_argument("--bags", default="64,256,1507")
    ap.add_argument("--configs", default="d,i")
    ap.add_argument("--r50", action="store_true")
    ap.add_argument("--no-shapes", action="store_true", help="only the training step")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"bench": "conv_dgrad_bf16", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "shapes": [], "train_step": []}
    print("| shape | n | direct ms (min-max) | aten dgrad | flipped forward | TF/s | vs aten | vs flipped |",
          file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|", file=sys.stderr)
    f = lambda v: "-" if v is None else f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    for n in [] if a.no_shapes else [int(v) for v in a.instances.split(",") if v]:
        for shape in R18 + (R50 if a.r50 else []):
            r = bench_shape(shape, n, a.steps, a.warmup, dev)
            out["shapes"].append(r)
            if r["direct_ms"] is None:
                print(f"| {r['shape']} | {n} | outside the kernel's domain: dX or dY of 2 GiB or more |", file=sys.stderr)
                continue
            print(f"| {r['shape']} | {n} | {f(r['direct_ms'])} | {f(r['aten_ms'])} | {f(r['flipped_ms'])} | "
                  f"{r['direct_tflops']} | {r['vs_aten']} | {r['vs_flipped'] or '-'} |", file=sys.stderr, flush=True)
    for config in [c for c in a.configs.split(",") if c]:
        for n in [int(v) for v in a.bags.split(",") if v]:
            out["train_step"].append(train_step(config, n, a.steps, a.warmup, dev))
            print(out["train_step"][-1], file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
