"""Time the bf16 stem convolution's training op (torch.ops.mcgmil.stem_conv_bf16: the inference
stem's MFMA kernel without its BatchNorm as the forward, the bf16 HIP weight gradient of
include/mcgmil_stem_grad_bf16.h as the backward) against the route it replaces, in one process on
one GPU.

(a) The layer, conv1 = Conv2d(3, 64, 7, stride 2, pad 3) on --instances (default 64, 256 and 1,507)
instances of 3 x 224 x 224, the fp32 NCHW instances as the model has them, the fp32 master weight
requiring a gradient, under torch.autocast("cuda", torch.bfloat16) -- forward + backward:
  op          torch.ops.mcgmil.stem_conv_bf16
  torch       what features.run_stem did before: the channels-last copy of x, then
              features.torch_conv (batch chunks sized by 4-byte elements, MIOpen per chunk,
              torch.cat) and aten.convolution_backward through autograd
  torch_conv  features.torch_conv alone, on an x that is channels-last already
and the weight gradient alone, on bf16 tensors that exist already:
  wgrad       mcgmil_stem_wgrad_bf16 through the C ABI (workspace and dw allocated once)
  aten_wgrad  aten.convolution_backward with mask (False, True, False), split along the batch
              below 2^31 bytes as features._aten_conv_backward splits it
interleaved call by call. Each call is timed with HIP events: --warmup calls, then --steps timed
ones, median and min-max. A variant "wins" ("loses") when the medians differ by more than the larger
of the two min-max spreads, else it "ties". The weight gradient's achieved bandwidth counts dY and
the bf16 x read once, its rate 2 * 64 * Cin * k^2 flop per output pixel (the live taps).

(b) A whole training step, forward() + backward() of MultiHeadGatedAttentionMIL (r18, head training
on, batch-statistics BatchNorm, MCGMIL_CONV_GRAD=native) on one bag of --bags instances,
interleaved, with the peak memory of a step above what is allocated before it:
  g  enable_bf16_backbone_training() + enable_bf16_norm_training() + enable_bf16_stem_training()
  i  g + enable_bf16_stem_conv_training()

Prints the tables (markdown) on stderr and one JSON line on stdout. Fails without a GPU.
Usage: python scripts/bench_stem_conv_grad_bf16.py [--steps 20] [--warmup 5] [--instances 64,256,1507]
                                                    [--bags 64,256,1507] [--no-shapes] [--no-steps]
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
sys.path.insert(0, os.path.join(REPO, "scripts"))

from bench_norm_grad import interleaved, verdict  # noqa: E402
from mcgmil import MultiHeadGatedAttentionMIL, _lib, features, library  # noqa: E402,F401
from mcgmil.resnet import deactivate_batchnorm  # noqa: E402

BF = torch.bfloat16
CL = torch.channels_last
CIN, HW, K, PAD = 3, 224, 7, 3


def bench_layer(n, steps, warmup, dev):
    torch.manual_seed(0)
    conv = nn.Conv2d(CIN, 64, K, stride=2, padding=PAD, bias=False).to(dev)
    x = torch.rand(n, CIN, HW, HW, device=dev)                      # the instances: fp32 NCHW
    x_cl = x.contiguous(memory_format=CL)
    oh = (HW + 2 * PAD - K) // 2 + 1
    dy = torch.randn(n, oh, oh, 64, device=dev).to(BF).permute(0, 3, 1, 2)      # bf16 channels-last

    def op():
        conv.weight.grad = None
        with torch.autocast("cuda", BF):
            y = features.stem_conv_bf16_op(conv, x)
        y.backward(dy)

    def torch_route(copy):
        conv.weight.grad = None
        with torch.autocast("cuda", BF):
            y = features.torch_conv(conv, x.contiguous(memory_format=CL) if copy else x_cl)
        y.backward(dy)

    # the weight gradient alone, through the C ABI
    L = _lib.load()
    xb = x.to(BF).contiguous()
    xb_cl = xb.contiguous(memory_format=CL)
    g = _lib.StemGradBf16Args()
    a = g.fwd
    a.batch, a.in_channels, a.height, a.width = xb.shape
    a.out_channels, a.kernel, a.stride, a.pad = 64, K, 2, PAD
    nbytes = ctypes.c_size_t()
    _lib.check(L.mcgmil_stem_wgrad_workspace_size_bf16(ctypes.byref(g), ctypes.byref(nbytes)),
               "mcgmil_stem_wgrad_workspace_size_bf16")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    dw = torch.empty(64, CIN, K, K, device=dev)
    a.x, g.dy, g.dw = (ctypes.c_void_p(t.data_ptr()) for t in (xb, dy, dw))
    g.workspace, g.workspace_bytes = ctypes.c_void_p(ws.data_ptr()), nbytes.value

    def wgrad():
        _lib.check(L.mcgmil_stem_wgrad_bf16(ctypes.byref(g), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "mcgmil_stem_wgrad_bf16")
    shim = features._ConvShim(conv.weight.detach(), 2, PAD)
    fns = {"op": op, "torch": lambda: torch_route(True), "torch_conv": lambda: torch_route(False), "wgrad": wgrad,
           "aten_wgrad": lambda: features._aten_conv_backward_bf16(shim, xb_cl, dy, False, True)}
    t = interleaved(fns, steps, warmup)
    pixels = n * oh * oh
    nbytes_algo = dy.numel() * 2 + xb.numel() * 2
    flop = 2 * 64 * CIN * K * K * pixels
    rnd = lambda v: [round(c, 4) for c in v]  # noqa: E731
    out = {"n": n, "pixels": pixels}
    for key in fns:
        out[key + "_ms"] = rnd(t[key])
    out.update(op_vs_torch=verdict(t["op"], t["torch"]), op_vs_torch_conv=verdict(t["op"], t["torch_conv"]),
               wgrad_vs_aten=verdict(t["wgrad"], t["aten_wgrad"]), torch_over_op=round(t["torch"][0] / t["op"][0], 3),
               aten_over_wgrad=round(t["aten_wgrad"][0] / t["wgrad"][0], 3),
               wgrad_algo_mb=round(nbytes_algo / 1e6, 1), wgrad_gbs=round(nbytes_algo / t["wgrad"][0] / 1e6, 1),
               wgrad_tfs=round(flop / t["wgrad"][0] / 1e9, 2))
    return out


VARIANTS = {"g_norm_stem": dict(stem_conv=False), "i_norm_stem_conv1": dict(stem_conv=True)}


def train_step(n, steps, warmup, dev):
    torch.manual_seed(0)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(dev)
    m.apply(deactivate_batchnorm)
    m.train().enable_head_training()
    x = torch.rand(1, n, 3, 224, 224, device=dev)
    target = torch.tensor([1], device=dev)
    os.environ["MCGMIL_CONV_GRAD"] = "native"

    def step(stem_conv):
        m.enable_bf16_backbone_training().enable_bf16_norm_training().enable_bf16_stem_training()
        m.enable_bf16_stem_conv_training(stem_conv)
        m.zero_grad(set_to_none=True)
        Y, A, aux = m(x, target, seed=7)
        (F.cross_entropy(Y.float(), target) + aux.float()).backward()
    variants = {k: (lambda kw=kw: step(**kw)) for k, kw in VARIANTS.items()}
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
    m.enable_bf16_backbone_training(False)
    out["i_vs_g"] = verdict(t["i_norm_stem_conv1"], t["g_norm_stem"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--instances", default="64,256,1507")
    ap.add_argument("--bags", default="64,256,1507")
    ap.add_argument("--no-shapes", action="store_true", help="only the training step")
    ap.add_argument("--no-steps", action="store_true", help="only the per-layer table")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_stem_conv_grad_bf16.py needs a GPU")
    dev = torch.device("cuda", 0)
    out = {"bench": "stem_conv_grad_bf16", "device": torch.cuda.get_device_name(0), "steps": a.steps,
           "warmup": a.warmup, "layer": [], "train_step": []}
    f = lambda v: f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    print("| n | op fwd+bwd ms (min-max) | torch (copy + torch_conv) | torch_conv alone | torch / op | op vs torch | "
          "wgrad ms | aten wgrad ms | aten / wgrad | wgrad vs aten | MB | GB/s | TF/s |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|", file=sys.stderr)
    for n in [] if a.no_shapes else [int(v) for v in a.instances.split(",") if v]:
        r = bench_layer(n, a.steps, a.warmup, dev)
        out["layer"].append(r)
        print(f"| {n} | {f(r['op_ms'])} | {f(r['torch_ms'])} | {f(r['torch_conv_ms'])} | {r['torch_over_op']:.2f} | "
              f"{r['op_vs_torch']} | {f(r['wgrad_ms'])} | {f(r['aten_wgrad_ms'])} | {r['aten_over_wgrad']:.2f} | "
              f"{r['wgrad_vs_aten']} | {r['wgrad_algo_mb']} | {r['wgrad_gbs']} | {r['wgrad_tfs']} |",
              file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print("| instances | g = bf16 backbone + norm + stem ms (min-max) | i = g + stem conv | i vs g | peak MiB g / i |",
          file=sys.stderr)
    print("|---|---|---|---|---|", file=sys.stderr)
    for n in [] if a.no_steps else [int(v) for v in a.bags.split(",") if v]:
        r = train_step(n, a.steps, a.warmup, dev)
        out["train_step"].append(r)
        print(f"| {n} | " + " | ".join(f(r[k + "_ms"]) for k in VARIANTS) + f" | {r['i_vs_g']} | " +
              " / ".join(str(r[k + "_peak_mib"]) for k in VARIANTS) + " |", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
