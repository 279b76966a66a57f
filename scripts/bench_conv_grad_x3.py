"""Time fp32 training on split-bf16 MFMA (bf16x3): the bf16x3 weight gradient
(features.conv2d_f32x3_wgrad, include/mcgmil_conv_grad_x3.h) against the fp32 HIP weight gradient
(features.conv2d_f32_wgrad) and aten's (MIOpen), and the bf16x3 flipped-forward data gradient
(features.conv2d_f32x3_dgrad, stride 1) against aten's, on the same tensors, in one process on one
GPU.

Per convolution shape class of ResNet-18 and (with --r50) ResNet-50 at --instances instances of
224 x 224, interleaved call by call, each call timed with HIP events: warm-up, then --steps timed
calls, median (min-max). An entry "wins" or "loses" against another only when the medians differ by
more than the larger min-max spread of the two sides; otherwise it "ties".

Then the r18 training step of one bag of --bags instances with enable_backbone_training(norm=True,
stem=True, stem_conv=True), interleaved: (a) "aten": the default backward route, (b) "direct":
MCGMIL_CONV_GRAD=direct, (c) "x3": enable_bf16x3_backbone_training(); with the peak memory of a
step above what is allocated before it, and whether two steps from identical state give
bitwise-equal gradients on every parameter.

--ablate-lib PATH: a build of the library with -DMCGMIL_WX3_HI_ONLY (the weight-gradient kernel
issues the hi * hi MFMA only: a third of the matrix work, the same loads, splits, LDS traffic and
barriers); its weight gradient is timed beside the full one ("x3_hi_only") to tell the matrix pipe
from the operand path.

Prints the tables (markdown) on stderr and one JSON line on stdout (--out FILE writes it as well).
Usage: python scripts/bench_conv_grad_x3.py [--steps 10] [--warmup 3] [--instances 64,256,1507]
                                            [--bags 64,256,1507] [--r50] [--no-shapes] [--out FILE]
"""
import argparse
import copy
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-gated-mil_amd"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from bench_backbone_grad import R18, R50, interleaved  # noqa: E402
from mcgmil import MultiHeadGatedAttentionMIL, _lib, features, library  # noqa: E402,F401
from mcgmil.resnet import deactivate_batchnorm  # noqa: E402


def verdict(a, b):
    """a against b, (median, min, max) each: "wins", "loses" or "ties" by the project's convention."""
    spread = max(a[2] - a[1], b[2] - b[1])
    if abs(a[0] - b[0]) <= spread:
        return "ties"
    return "wins" if a[0] < b[0] else "loses"


def ablated_wgrad(path):
    """features.conv2d_f32x3_wgrad on another build of the library."""
    L = _lib.bind(path)

    def wgrad(conv, x, dy):
        g = _lib.ConvGradArgs()
        g.fwd = features._conv_args(conv, x)
        a = g.fwd
        dw = torch.empty((a.out_channels, a.in_channels, a.kernel_h, a.kernel_w), device=x.device)
        a.x, g.dy, g.dw = features._ptr(x), features._ptr(dy), features._ptr(dw)
        features._workspace(L.mcgmil_conv_wgrad_workspace_size_f32x3, "size", g, x.device)
        rc = L.mcgmil_conv2d_wgrad_f32x3(ctypes.byref(g), features._stream(x.device))
        assert rc == 0, L.mcgmil_last_error()
        return dw
    return wgrad


def bench_shape(shape, n, steps, warmup, dev, ablated):
    name, cin, cout, k, s, p, hw, count = shape
    cl = torch.channels_last
    x = (torch.randn(n, cin, hw, hw, device=dev) + 0.25).contiguous(memory_format=cl)
    conv = features._ConvShim(torch.randn(cout, cin, k, k, device=dev) / (cin * k * k) ** 0.5, s, p)
    oh = (hw + 2 * p - k) // s + 1
    dy = torch.randn(n, cout, oh, oh, device=dev).contiguous(memory_format=cl)
    fns = {"x3_wgrad": lambda: features.conv2d_f32x3_wgrad(conv, x, dy),
           "f32_wgrad": lambda: features.conv2d_f32_wgrad(conv, x, dy),
           "aten_wgrad": lambda: features._aten_conv_backward(conv, x, dy, False, True)}
    if s == 1:
        fns["x3_dgrad"] = lambda: features.conv2d_f32x3_dgrad(conv, dy, x.shape)
        fns["aten_dgrad"] = lambda: features._aten_conv_backward(conv, x, dy, True, False)
    if ablated is not None:
        fns["x3_hi_only"] = lambda: ablated(conv, x, dy)
    t = interleaved(fns, steps, warmup)
    flops = 2.0 * n * oh * oh * cout * cin * k * k
    out = {"shape": name, "n": n, "count": count}
    out.update({key + "_ms": [round(c, 4) for c in v] for key, v in t.items()})
    out["x3_wgrad_tflops"] = round(flops / t["x3_wgrad"][0] / 1e9, 1)
    out["f32_wgrad_tflops"] = round(flops / t["f32_wgrad"][0] / 1e9, 1)
    out["x3_vs_f32"] = verdict(t["x3_wgrad"], t["f32_wgrad"])
    out["x3_vs_aten"] = verdict(t["x3_wgrad"], t["aten_wgrad"])
    out["x3_dgrad_vs_aten"] = verdict(t["x3_dgrad"], t["aten_dgrad"]) if s == 1 else "direct fp32 kernel"
    return out


def train_step(n, steps, warmup, dev):
    torch.manual_seed(0)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(dev)
    m.apply(deactivate_batchnorm)         # batch statistics without running ones: norm and stem take the layers
    m.train().enable_head_training().enable_backbone_training(norm=True, stem=True, stem_conv=True)
    twins = [copy.deepcopy(m), copy.deepcopy(m)]     # identical state, for the repeat check at the end
    x = torch.rand(1, n, 3, 224, 224, device=dev)
    target = torch.tensor([1], device=dev)

    def step(x3, route, model=m):
        os.environ["MCGMIL_CONV_GRAD"] = route
        model.enable_bf16x3_backbone_training(x3)
        model.zero_grad(set_to_none=True)
        Y, A, aux = model(x, target, seed=7)
        (F.cross_entropy(Y, target) + aux).backward()
    variants = {"aten": lambda: step(False, "aten"), "direct": lambda: step(False, "direct"),
                "x3": lambda: step(True, "aten")}
    t = interleaved(variants, steps, warmup)
    out = {"instances": n}
    for key, f in variants.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        out[key + "_ms"] = [round(c, 3) for c in t[key]]
        out[key + "_peak_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
    grads = []
    for twin in twins:                    # two steps from identical state
        step(True, "aten", twin)
        torch.cuda.synchronize()
        grads.append({k: p.grad.clone() for k, p in twin.named_parameters() if p.grad is not None})
    out["x3_bitwise_repeat"] = grads[0].keys() == grads[1].keys() and \
        all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])
    os.environ.pop("MCGMIL_CONV_GRAD", None)
    out["x3_vs_aten"] = verdict(t["x3"], t["aten"])
    out["x3_vs_direct"] = verdict(t["x3"], t["direct"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--instances", default="64,256,1507")
    ap.add_argument("--bags", default="64,256,1507")
    ap.add_argument("--r50", action="store_true")
    ap.add_argument("--no-shapes", action="store_true", help="only the training step")
    ap.add_argument("--ablate-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ablated = ablated_wgrad(a.ablate_lib) if a.ablate_lib else None
    out = {"bench": "conv_grad_x3", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "shapes": [], "train_step": []}
    f = lambda v: "-" if v is None else f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    print("| shape | n | x3 wgrad ms (min-max) | fp32 HIP wgrad | aten wgrad | x3 TF/s | vs fp32 HIP | vs aten | "
          "x3 dgrad | aten dgrad | vs aten | x3 hi-only |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|---|---|---|", file=sys.stderr)
    for n in [] if a.no_shapes else [int(v) for v in a.instances.split(",") if v]:
        for shape in R18 + (R50 if a.r50 else []):
            r = bench_shape(shape, n, a.steps, a.warmup, dev, ablated)
            out["shapes"].append(r)
            print(f"| {r['shape']} | {n} | {f(r['x3_wgrad_ms'])} | {f(r['f32_wgrad_ms'])} | {f(r['aten_wgrad_ms'])} | "
                  f"{r['x3_wgrad_tflops']} | {r['x3_vs_f32']} | {r['x3_vs_aten']} | {f(r.get('x3_dgrad_ms'))} | "
                  f"{f(r.get('aten_dgrad_ms'))} | {r['x3_dgrad_vs_aten']} | {f(r.get('x3_hi_only_ms'))} |",
                  file=sys.stderr, flush=True)
    for n in [int(v) for v in a.bags.split(",") if v]:
        out["train_step"].append(train_step(n, a.steps, a.warmup, dev))
        print(out["train_step"][-1], file=sys.stderr, flush=True)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
