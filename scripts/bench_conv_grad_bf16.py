"""Time the bf16 convolution backward of the backbone on the HIP kernels against
aten.convolution_backward (MIOpen) in bf16 and against the fp32 HIP weight gradient, in one process
on one GPU.

Per block-convolution shape class of ResNet-18 at --instances (default 64, 256 and 1,507) instances
of 224 x 224, interleaved call by call on the same values: the bf16 HIP weight gradient
(features.conv2d_bf16_wgrad), aten's bf16 weight gradient, the fp32 HIP weight gradient
(features.conv2d_f32_wgrad, on the same values in fp32) with ms and TF/s each, and for stride 1 the
data gradient on the flipped bf16 forward kernel (features.conv2d_bf16_dgrad) against aten's bf16
one (stride 2 has no native one and is marked "aten"). Each call is timed with HIP events:
--warmup calls, then --steps timed ones, median and min-max. A shape "loses" when the bf16 HIP weight
gradient's median exceeds aten's by more than the larger of the two min-max spreads.

Then a whole training step, forward() + backward() of MultiHeadGatedAttentionMIL (r18, head
training on, batch-statistics BatchNorm) on one bag of --bags instances, interleaved, with the
peak memory of a step above what is allocated before it:
  a  fp32, enable_backbone_training() (the fp32 HIP forward, the default backward route)
  b  the user's own torch.autocast("cuda", torch.bfloat16) over the torch layers
  c  enable_bf16_backbone_training() on the aten route
  d  enable_bf16_backbone_training() with MCGMIL_CONV_GRAD=native

Prints the per-shape table (markdown) on stderr and one JSON line on stdout.
Usage: python scripts/bench_conv_grad_bf16.py [--steps 30] [--warmup 5] [--instances 64,256,1507]
                                               [--bags 64,256,1507] [--no-shapes]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-gated-mil_amd"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from bench_backbone_grad import R18, interleaved  # noqa: E402
from mcgmil import MultiHeadGatedAttentionMIL, features, library  # noqa: E402,F401
from mcgmil.resnet import deactivate_batchnorm  # noqa: E402

BF = torch.bfloat16


def bench_shape(shape, n, steps, warmup, dev):
    name, cin, cout, k, s, p, hw, count = shape
    cl = torch.channels_last
    x32 = torch.randn(n, cin, hw, hw, device=dev).to(BF).float().contiguous(memory_format=cl)
    w32 = (torch.randn(cout, cin, k, k, device=dev) / (cin * k * k) ** 0.5).to(BF).float()
    oh = (hw + 2 * p - k) // s + 1
    dy32 = torch.randn(n, cout, oh, oh, device=dev).to(BF).float().contiguous(memory_format=cl)
    x, dy, w = x32.to(BF), dy32.to(BF), w32.to(BF)
    conv, conv32 = features._ConvShim(w32, s, p), features._ConvShim(w32, s, p)
    native_d = features.dgrad_bf16_native(conv, dy)

    def aten(mask):
        return torch.ops.aten.convolution_backward(dy, x, w, None, [s, s], [p, p], [1, 1], False, [0, 0], 1, mask)
    fns = {"wgrad": lambda: features.conv2d_bf16_wgrad(conv, x, dy),
           "aten_wgrad": lambda: aten([False, True, False]),
           "f32_wgrad": lambda: features.conv2d_f32_wgrad(conv32, x32, dy32),
           "aten_dgrad": lambda: aten([True, False, False])}
    if native_d:
        fns["dgrad"] = lambda: features.conv2d_bf16_dgrad(conv, dy, x)
    t = interleaved(fns, steps, warmup)
    spread = max(t["wgrad"][2] - t["wgrad"][1], t["aten_wgrad"][2] - t["aten_wgrad"][1])
    flops = 2.0 * n * oh * oh * cout * cin * k * k
    r = lambda v: [round(c, 4) for c in v]  # noqa: E731
    tf = lambda key: round(flops / t[key][0] / 1e9, 1)  # noqa: E731
    return {"shape": name, "n": n, "count": count, "wgrad_ms": r(t["wgrad"]), "aten_wgrad_ms": r(t["aten_wgrad"]),
            "f32_wgrad_ms": r(t["f32_wgrad"]), "wgrad_tflops": tf("wgrad"), "aten_wgrad_tflops": tf("aten_wgrad"),
            "f32_wgrad_tflops": tf("f32_wgrad"), "dgrad_ms": r(t["dgrad"]) if native_d else "aten",
            "aten_dgrad_ms": r(t["aten_dgrad"]), "wgrad_vs_aten": round(t["wgrad"][0] / t["aten_wgrad"][0], 3),
            "wgrad_vs_f32": round(t["wgrad"][0] / t["f32_wgrad"][0], 3),
            "dgrad_vs_aten": round(t["dgrad"][0] / t["aten_dgrad"][0], 3) if native_d else None,
            "loses": bool(t["wgrad"][0] - t["aten_wgrad"][0] > spread)}


def train_step(n, steps, warmup, dev):
    torch.manual_seed(0)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(dev)
    m.apply(deactivate_batchnorm)
    m.train().enable_head_training()
    x = torch.rand(1, n, 3, 224, 224, device=dev)
    target = torch.tensor([1], device=dev)

    def step(fp32_native=False, bf16=False, autocast=False, route="aten"):
        os.environ["MCGMIL_CONV_GRAD"] = route
        m.enable_backbone_training(fp32_native)
        m.enable_bf16_backbone_training(bf16)
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", BF, enabled=autocast):
            Y, A, aux = m(x, target, seed=7)
        (F.cross_entropy(Y.float(), target) + aux.float()).backward()
    variants = {"a_fp32_optin": lambda: step(fp32_native=True),
                "b_user_autocast": lambda: step(autocast=True),
                "c_bf16_optin_aten": lambda: step(bf16=True),
                "d_bf16_optin_native": lambda: step(bf16=True, route="native")}
    out = {"instances": n}
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
    m.enable_backbone_training(False)
    m.enable_bf16_backbone_training(False)
    out["fastest"] = min(variants, key=lambda key: t[key][0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--instances", default="64,256,1507")
    ap.add_argument("--bags", default="64,256,1507")
    ap.add_argument("--no-shapes", action="store_true", help="only the training step")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"bench": "conv_grad_bf16", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "shapes": [], "train_step": []}
    print("| shape | n | bf16 wgrad ms (min-max) | TF/s | aten bf16 wgrad | TF/s | fp32 wgrad | TF/s | "
          "flipped-forward dgrad | aten bf16 dgrad |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|---|", file=sys.stderr)
    for n in [] if a.no_shapes else [int(v) for v in a.instances.split(",") if v]:
        for shape in R18:
            r = bench_shape(shape, n, a.steps, a.warmup, dev)
            out["shapes"].append(r)
            f = lambda v: v if isinstance(v, str) else f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
            print(f"| {r['shape']} | {n} | {f(r['wgrad_ms'])} | {r['wgrad_tflops']} | "
                  f"{f(r['aten_wgrad_ms'])}{' LOSES' if r['loses'] else ''} | {r['aten_wgrad_tflops']} | "
                  f"{f(r['f32_wgrad_ms'])} | {r['f32_wgrad_tflops']} | {f(r['dgrad_ms'])} | {f(r['aten_dgrad_ms'])} |",
                  file=sys.stderr, flush=True)
    for n in [int(v) for v in a.bags.split(",") if v]:
        out["train_step"].append(train_step(n, a.steps, a.warmup, dev))
        print(out["train_step"][-1], file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
