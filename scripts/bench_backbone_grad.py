"""Time the fp32 convolution backward of the backbone on the HIP kernels against
aten.convolution_backward (MIOpen) on the same tensors, in one process on one GPU.

Per convolution shape of ResNet-18 (and, with --r50, the bottleneck shapes of ResNet-50) at
--instances (default 64 and 256) instances of 224 x 224: the native weight gradient
(features.conv2d_f32_wgrad) and data gradient (features.conv2d_f32_dgrad; stride 2 has no native
one and is marked "aten") against aten.convolution_backward with the matching output_mask,
interleaved call by call. Each call is timed with HIP events: warm-up, then --steps timed calls,
median and min-max. A shape "loses" when the native median (wgrad + dgrad) exceeds aten's by more
than the larger of the two min-max spreads.

Then a whole training step, forward() + backward() of MultiHeadGatedAttentionMIL (r18, head
training on) on one bag of --bags instances, interleaved: "off" (every convolution on the torch
layers), "on" (enable_backbone_training(): the HIP forward, the default backward route) and
"on_native_bwd" (the same with MCGMIL_CONV_GRAD=native: the HIP backward kernels), with the peak
memory of a step above what is allocated before it.

Prints the per-shape table (markdown) on stderr and one JSON line on stdout.
Usage: python scripts/bench_backbone_grad.py [--steps 10] [--warmup 3] [--instances 64,256]
                                             [--bags 64,256] [--r50] [--no-shapes]
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

from mcgmil import MultiHeadGatedAttentionMIL, features, library  # noqa: E402,F401

# (name, Cin, Cout, kernel, stride, pad, input H = W at 224 x 224 instances, count in the network)
R18 = [
    ("l1 3x3",       64,  64,  3, 1, 1, 56, 4),
    ("l2.0 3x3/2",   64,  128, 3, 2, 1, 56, 1),
    ("l2.0 down/2",  64,  128, 1, 2, 0, 56, 1),
    ("l2 3x3",       128, 128, 3, 1, 1, 28, 3),
    ("l3.0 3x3/2",   128, 256, 3, 2, 1, 28, 1),
    ("l3.0 down/2",  128, 256, 1, 2, 0, 28, 1),
    ("l3 3x3",       256, 256, 3, 1, 1, 14, 3),
    ("l4.0 3x3/2",   256, 512, 3, 2, 1, 14, 1),
    ("l4.0 down/2",  256, 512, 1, 2, 0, 14, 1),
    ("l4 3x3",       512, 512, 3, 1, 1, 7,  3),
]
R50 = [
    ("r50 l1 1x1 64-64",     64,   64,   1, 1, 0, 56, 1),
    ("r50 l1 1x1 64-256",    64,   256,  1, 1, 0, 56, 4),
    ("r50 l1 1x1 256-64",    256,  64,   1, 1, 0, 56, 2),
    ("r50 l2 1x1 256-128",   256,  128,  1, 1, 0, 56, 1),
    ("r50 l2 3x3/2 128",     128,  128,  3, 2, 1, 56, 1),
    ("r50 l2 1x1 128-512",   128,  512,  1, 1, 0, 28, 4),
    ("r50 l2 down/2",        256,  512,  1, 2, 0, 56, 1),
    ("r50 l2 1x1 512-128",   512,  128,  1, 1, 0, 28, 3),
    ("r50 l3 1x1 512-256",   512,  256,  1, 1, 0, 28, 1),
    ("r50 l3 3x3/2 256",     256,  256,  3, 2, 1, 28, 1),
    ("r50 l3 1x1 256-1024",  256,  1024, 1, 1, 0, 14, 6),
    ("r50 l3 down/2",        512,  1024, 1, 2, 0, 28, 1),
    ("r50 l3 1x1 1024-256",  1024, 256,  1, 1, 0, 14, 5),
    ("r50 l4 1x1 1024-512",  1024, 512,  1, 1, 0, 14, 1),
    ("r50 l4 3x3/2 512",     512,  512,  3, 2, 1, 14, 1),
    ("r50 l4 1x1 512-2048",  512,  2048, 1, 1, 0, 7,  3),
    ("r50 l4 down/2",        1024, 2048, 1, 2, 0, 14, 1),
    ("r50 l4 1x1 2048-512",  2048, 512,  1, 1, 0, 7,  2),
]


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


def bench_shape(shape, n, steps, warmup, dev):
    name, cin, cout, k, s, p, hw, count = shape
    cl = torch.channels_last
    x = torch.randn(n, cin, hw, hw, device=dev).contiguous(memory_format=cl)
    conv = features._ConvShim(torch.randn(cout, cin, k, k, device=dev) / (cin * k * k) ** 0.5, s, p)
    w = conv.weight.detach()
    oh = (hw + 2 * p - k) // s + 1
    dy = torch.randn(n, cout, oh, oh, device=dev).contiguous(memory_format=cl)
    native_d = features.dgrad_native(conv)

    def aten(mask):
        return torch.ops.aten.convolution_backward(dy, x, w, None, [s, s], [p, p], [1, 1], False, [0, 0], 1, mask)
    fns = {"wgrad": lambda: features.conv2d_f32_wgrad(conv, x, dy),
           "aten_wgrad": lambda: aten([False, True, False]),
           "aten_dgrad": lambda: aten([True, False, False]),
           "aten_both": lambda: aten([True, True, False])}
    if native_d:
        fns["dgrad"] = lambda: features.conv2d_f32_dgrad(conv, dy, x.shape, x)
    t = interleaved(fns, steps, warmup)
    d = t["dgrad"] if native_d else t["aten_dgrad"]
    native = t["wgrad"][0] + d[0]
    ref = min(t["aten_both"][0], t["aten_wgrad"][0] + t["aten_dgrad"][0])
    spread = max(t["wgrad"][2] - t["wgrad"][1] + d[2] - d[1], t["aten_both"][2] - t["aten_both"][1])
    flops = 2.0 * n * oh * oh * cout * cin * k * k
    r = lambda v: [round(c, 4) for c in v]  # noqa: E731
    return {"shape": name, "n": n, "count": count, "wgrad_ms": r(t["wgrad"]), "aten_wgrad_ms": r(t["aten_wgrad"]),
            "dgrad_ms": r(t["dgrad"]) if native_d else "aten", "aten_dgrad_ms": r(t["aten_dgrad"]),
            "aten_both_ms": r(t["aten_both"]), "native_ms": round(native, 4), "aten_ms": round(ref, 4),
            "spread_ms": round(spread, 4), "wgrad_tflops": round(flops / t["wgrad"][0] / 1e9, 1),
            "loses": bool(native - ref > spread)}


def train_step(n, steps, warmup, dev):
    torch.manual_seed(0)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(dev)
    m.train().enable_head_training()
    x = torch.rand(1, n, 3, 224, 224, device=dev)
    target = torch.tensor([1], device=dev)

    def step(native, route="aten"):
        os.environ["MCGMIL_CONV_GRAD"] = route
        m.enable_backbone_training(native)
        m.zero_grad(set_to_none=True)
        Y, A, aux = m(x, target, seed=7)
        (F.cross_entropy(Y, target) + aux).backward()
    out = {"instances": n}
    variants = {"off": lambda: step(False), "on": lambda: step(True), "on_native_bwd": lambda: step(True, "native")}
    t = interleaved(variants, steps, warmup)
    for key, f in variants.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        out[key + "_ms"] = [round(c, 3) for c in t[key]]
        out[key + "_peak_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
    os.environ.pop("MCGMIL_CONV_GRAD", None)
    out["speedup"] = round(t["off"][0] / t["on"][0], 3)
    out["speedup_native_bwd"] = round(t["off"][0] / t["on_native_bwd"][0], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--instances", default="64,256")
    ap.add_argument("--bags", default="64,256")
    ap.add_argument("--r50", action="store_true")
    ap.add_argument("--no-shapes", action="store_true", help="only the training step")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"bench": "backbone_grad", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "shapes": [], "train_step": []}
    print("| shape | n | wgrad ms (min-max) | aten wgrad | dgrad | aten dgrad | native | aten | spread | TF/s |",
          file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|---|", file=sys.stderr)
    for n in [] if a.no_shapes else [int(v) for v in a.instances.split(",") if v]:
        for shape in R18 + (R50 if a.r50 else []):
            r = bench_shape(shape, n, a.steps, a.warmup, dev)
            out["shapes"].append(r)
            f = lambda v: v if isinstance(v, str) else f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
            print(f"| {r['shape']} | {n} | {f(r['wgrad_ms'])} | {f(r['aten_wgrad_ms'])} | {f(r['dgrad_ms'])} | "
                  f"{f(r['aten_dgrad_ms'])} | {r['native_ms']:.3f} | {r['aten_ms']:.3f}{' LOSES' if r['loses'] else ''} | "
                  f"{r['spread_ms']:.3f} | {r['wgrad_tflops']} |", file=sys.stderr, flush=True)
    for n in [int(v) for v in a.bags.split(",") if v]:
        out["train_step"].append(train_step(n, a.steps, a.warmup, dev))
        print(out["train_step"][-1], file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
