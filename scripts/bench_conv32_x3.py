"""Time and measure the fp32 convolution on split-bf16 MFMA (features.conv2d_f32(precision="bf16x3"),
mcgmil_conv2d_f32x3) in one process on one GPU. The protocol of scripts/bench_conv_dgrad.py: HIP
events, --warmup warm-up calls then --steps timed calls per entry, variants interleaved call by
call, median (min-max), instances of 224 x 224.

(a) Per block-convolution shape of ResNet-18 and (with --r50) ResNet-50 at --instances instances:
    the exact fp32 kernel, bf16x3, MIOpen's fp32 convolution (the torch layer) and, for scale, the
    bf16 MFMA kernel on bf16 activations. TF/s on the fp32-equivalent flop 2 N OH OW Cout Cin k^2
    and GB/s on x + y + w read or written once. bf16x3 "wins" / "loses" against the exact kernel
    only when the medians differ by more than the larger of the two min-max spreads, else "ties".
(b) extract_features of one fp32 bag of --bag instances with model.feature_precision "fp32" and
    "bf16x3", interleaved.
(c) On config 5's image and seed (bench_cfg5.py) the nrel max|a - ref| / max|ref| of features, Y,
    A_mean, A_var and prob_mean of the bf16x3 pipeline and of the bf16 pipeline, each against the
    exact fp32 pipeline.

Prints the per-shape table (markdown) on stderr and one JSON line on stdout.
Usage: python scripts/bench_conv32_x3.py [--steps 10] [--warmup 3] [--instances 64,256,1507] [--r50]
                                         [--bag 1507] [--no-shapes] [--no-features] [--no-drift]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-gated-mil_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench_backbone_grad import R18, R50, interleaved  # noqa: E402
from bench_conv_dgrad import verdict  # noqa: E402
from mcgmil import MultiHeadGatedAttentionMIL, features  # noqa: E402
from mcgmil.resnet import deactivate_batchnorm  # noqa: E402

BF = torch.bfloat16


def bench_shape(shape, n, steps, warmup, dev):
    name, cin, cout, k, s, p, hw, count = shape
    cl = torch.channels_last
    oh = (hw + 2 * p - k) // s + 1
    if 4 * n * max(cin * hw * hw, cout * oh * oh) >= 2 ** 31:      # MIOpen's fp32 limit (features.torch_conv)
        return {"shape": name, "n": n, "count": count, "x3_ms": None}
    x = torch.randn(n, cin, hw, hw, device=dev).contiguous(memory_format=cl)
    conv = features._ConvShim(torch.randn(cout, cin, k, k, device=dev) / (cin * k * k) ** 0.5, s, p)
    conv.requires_grad_(False)
    fns = {"exact": lambda: features.conv2d_f32(conv, x, precision="fp32"),
           "x3": lambda: features.conv2d_f32(conv, x, precision="bf16x3"),
           "miopen": lambda: conv(x)}
    if cin % 64 == 0:
        xb = x.to(BF)
        convb = features._ConvShim(conv.weight.detach().to(BF), s, p).requires_grad_(False)
        fns["bf16"] = lambda: features.conv2d(convb, xb)
    with torch.no_grad():
        t = interleaved(fns, steps, warmup)
    flops = 2.0 * n * oh * oh * cout * cin * k * k
    gbytes = 4.0 * (x.numel() + n * oh * oh * cout + conv.weight.numel()) / 1e9
    r = lambda v: [round(c, 4) for c in v]  # noqa: E731
    out = {"shape": name, "n": n, "count": count}
    for key in fns:
        out[key + "_ms"] = r(t[key])
    out.update({"exact_tflops": round(flops / t["exact"][0] / 1e9, 1), "x3_tflops": round(flops / t["x3"][0] / 1e9, 1),
                "x3_gbs": round(gbytes / t["x3"][0] * 1e3), "exact_gbs": round(gbytes / t["exact"][0] * 1e3),
                "x3_speedup": round(t["exact"][0] / t["x3"][0], 2),
                "vs_exact": verdict(t["x3"], t["exact"]), "vs_miopen": verdict(t["x3"], t["miopen"])})
    return out


def _model(dev):
    torch.manual_seed(0)
    m = MultiHeadGatedAttentionMIL(pretrained=False, shared_attention=False)
    m.apply(deactivate_batchnorm)
    m.to(dev).eval()
    m.feature_extractor.to(memory_format=torch.channels_last)
    return m


def bench_features(n, steps, warmup, dev):
    m = _model(dev)
    x = torch.rand(1, n, 3, 224, 224, device=dev)

    def run(precision):
        m.feature_precision = precision
        return m.extract_features(x)
    with torch.no_grad():
        t = interleaved({"fp32": lambda: run("fp32"), "bf16x3": lambda: run("bf16x3")}, steps, warmup)
        a, b = run("fp32").double(), run("bf16x3").double()
    m.feature_precision = "fp32"
    return {"instances": n, "fp32_ms": [round(c, 3) for c in t["fp32"]], "bf16x3_ms": [round(c, 3) for c in t["bf16x3"]],
            "speedup": round(t["fp32"][0] / t["bf16x3"][0], 2), "verdict": verdict(t["bf16x3"], t["fp32"]),
            "features_nrel": float((b - a).abs().max() / a.abs().max())}


def drift(dev):
    import bench_cfg5 as C5
    from mcgmil.infer import mc_predict_image
    from mcgmil.patcher import ImagePatcher
    m = _model(dev)
    patcher = ImagePatcher(patch_size=C5.PS, overlap=C5.OVERLAP, empty_thresh=C5.THRESH)
    patcher.get_tiles(C5.H_IMG, C5.W_IMG)
    img = C5.synthetic_mammogram(dev, seed=5)
    keys = ("features", "Y", "A_mean", "A_var", "prob_mean")

    def run(mode):
        m.compute_dtype = BF if mode == "bf16" else torch.float32
        m.feature_precision = "bf16x3" if mode == "bf16x3" else "fp32"
        o = mc_predict_image(m, patcher, img, T=100, seed=6, features_dtype=BF if mode == "bf16" else None)
        torch.cuda.synchronize()
        return {k: o[k].double().cpu() for k in keys}, len(o["tiles_indices"])
    ref, k = run("fp32")
    out = {"instances": k}
    for mode in ("bf16x3", "bf16", "fp32"):        # the last: the exact pipeline against itself
        o, _ = run(mode)
        out[mode] = {key: float((o[key] - ref[key]).abs().max() / ref[key].abs().max()) for key in keys}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--instances", default="64,256,1507")
    ap.add_argument("--bag", type=int, default=1507)
    ap.add_argument("--r50", action="store_true")
    ap.add_argument("--no-shapes", action="store_true")
    ap.add_argument("--no-features", action="store_true")
    ap.add_argument("--no-drift", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"bench": "conv32_x3", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "shapes": [], "extract_features": None, "cfg5_nrel_vs_fp32": None}
    print("| shape | n | exact fp32 ms (min-max) | bf16x3 | MIOpen fp32 | bf16 kernel | bf16x3 TF/s | GB/s | "
          "x exact | vs exact | vs MIOpen |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|---|---|", file=sys.stderr)
    f = lambda v: "-" if v is None else f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    for n in [] if a.no_shapes else [int(v) for v in a.instances.split(",") if v]:
        for shape in R18 + (R50 if a.r50 else []):
            r = bench_shape(shape, n, a.steps, a.warmup, dev)
            out["shapes"].append(r)
            if r.get("x3_ms") is None:
                print(f"| {r['shape']} | {n} | not timed: x or y of 2 GiB or more (MIOpen's limit) |", file=sys.stderr)
                continue
            print(f"| {r['shape']} | {n} | {f(r['exact_ms'])} | {f(r['x3_ms'])} | {f(r['miopen_ms'])} | "
                  f"{f(r.get('bf16_ms'))} | {r['x3_tflops']} | {r['x3_gbs']} | {r['x3_speedup']} | {r['vs_exact']} | "
                  f"{r['vs_miopen']} |", file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    if not a.no_features:
        out["extract_features"] = bench_features(a.bag, a.steps, a.warmup, dev)
        print(out["extract_features"], file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    if not a.no_drift:
        out["cfg5_nrel_vs_fp32"] = drift(dev)
        print(out["cfg5_nrel_vs_fp32"], file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
