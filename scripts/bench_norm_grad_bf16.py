"""Time the fused bf16 BatchNorm/add/ReLU training op (torch.ops.mcgmil.bn_act_bf16: the fused HIP
forward in bf16 and the HIP backward of include/mcgmil_bn_grad_bf16.h) against the torch layers
under autocast on the same tensors, in one process on one GPU.

Per BatchNorm shape of the ResNet-18 blocks at --instances (default 64, 256 and 1,507) instances of
224 x 224, in the three forms the blocks use -- relu(bn(x) + r) (bn2), relu(bn(x)) (bn1) and bn(x)
(downsample) -- forward + backward with x / r bf16 and the fp32 BN parameters requiring gradients:
"op" (features.bn_act inside native_norm_bf16_training()) against "torch" (bn(x), + r, torch.relu
under torch.autocast("cuda", torch.bfloat16)), interleaved call by call. Each call is timed with HIP
events: --warmup calls, then --steps timed ones, median and min-max. The op "wins" ("loses") when
the medians differ by more than the larger of the two min-max spreads, else it "ties".
The backward's achieved bandwidth is its algorithmic bytes (x and dy read once, y read once with
ReLU; dx written once, dresidual written once with ReLU and a residual; 2 bytes each) over the
median of the C ABI call on the same tensors; the kernels read x, dy and y twice, so the traffic
they cause is higher than that.

Then a whole training step, forward() + backward() of MultiHeadGatedAttentionMIL (r18, head
training on, batch-statistics BatchNorm) on one bag of --bags instances, interleaved, with the peak
memory of a step above what is allocated before it:
  b  the user's own torch.autocast("cuda", torch.bfloat16) over the torch layers
  c  enable_bf16_backbone_training() on the aten route
  d  enable_bf16_backbone_training() with MCGMIL_CONV_GRAD=native
  e  d + enable_bf16_norm_training()
  f  c + enable_bf16_norm_training()

Prints the tables (markdown) on stderr and one JSON line on stdout.
Usage: python scripts/bench_norm_grad_bf16.py [--steps 20] [--warmup 5] [--instances 64,256,1507]
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

from bench_norm_grad import R18, interleaved, verdict  # noqa: E402
from mcgmil import MultiHeadGatedAttentionMIL, _lib, features, library  # noqa: E402,F401
from mcgmil.resnet import deactivate_batchnorm  # noqa: E402

BF = torch.bfloat16
FORMS = (("add+relu", True, True), ("relu", False, True), ("plain", False, False))     # (name, residual, relu)


def capi_backward(L, x, y, dy, gamma, mean, invstd, relu, outs, ws):
    a = _lib.BnGradBf16Args()
    a.rows, a.channels, a.relu = x.numel() // x.shape[1], x.shape[1], int(relu)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a.x, a.y, a.dy, a.gamma, a.mean, a.invstd = p(x), p(y if relu else None), p(dy), p(gamma), p(mean), p(invstd)
    a.dx, a.dresidual, a.dgamma, a.dbeta = (p(outs.get(k)) for k in ("dx", "dres", "dgamma", "dbeta"))
    a.workspace, a.workspace_bytes = p(ws), ws.numel()
    rc = L.mcgmil_batchnorm_act_backward_bf16(ctypes.byref(a),
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc:
        raise RuntimeError(f"mcgmil_batchnorm_act_backward_bf16 failed ({rc}): {L.mcgmil_last_error().decode()}")


def bench_shape(shape, n, form, steps, warmup, dev):
    name, C, hw, _, _ = shape
    fname, res, relu = form
    cl = torch.channels_last
    bn = nn.BatchNorm2d(C).to(dev)
    deactivate_batchnorm(bn)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    new = lambda: torch.randn(n, C, hw, hw, device=dev).to(BF).contiguous(memory_format=cl)  # noqa: E731
    x = new().requires_grad_()
    r = new().requires_grad_() if res else None
    dy = new()

    def fwd_bwd(native):
        for t in (x, r, bn.weight, bn.bias):
            if t is not None:
                t.grad = None
        with torch.autocast("cuda", BF), features.native_norm_bf16_training(native):
            features.bn_act(bn, x, relu, r).backward(dy)
    with torch.no_grad():
        y, mean, invstd = features.batchnorm_act_stats_bf16(x.detach(), bn.weight.detach(), bn.bias.detach(),
                                                            None if r is None else r.detach(), bn.eps, relu)
    L = _lib.load()
    a = _lib.BnGradBf16Args()
    a.rows, a.channels = x.numel() // C, C
    nbytes = ctypes.c_size_t()
    _lib.check(L.mcgmil_bn_grad_workspace_size_bf16(ctypes.byref(a), ctypes.byref(nbytes)),
               "mcgmil_bn_grad_workspace_size_bf16")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    full = {"dx": torch.empty_like(y), "dgamma": torch.empty_like(mean), "dbeta": torch.empty_like(mean)}
    if res and relu:
        full["dres"] = torch.empty_like(y)
    args = (x.detach(), y, dy, bn.weight.detach(), mean, invstd, relu)
    fns = {"op": lambda: fwd_bwd(True), "torch": lambda: fwd_bwd(False),
           "bwd": lambda: capi_backward(L, *args, full, ws)}
    t = interleaved(fns, steps, warmup)
    algo = (3 + int(relu) + int(res and relu)) * x.numel() * 2          # bytes
    rnd = lambda v: [round(c, 4) for c in v]  # noqa: E731
    return {"shape": name, "C": C, "hw": hw, "n": n, "form": fname, "op_ms": rnd(t["op"]), "torch_ms": rnd(t["torch"]),
            "ratio": round(t["torch"][0] / t["op"][0], 3), "op": verdict(t["op"], t["torch"]),
            "bwd_ms": rnd(t["bwd"]), "bwd_algo_mb": round(algo / 1e6, 1),
            "bwd_gbs": round(algo / t["bwd"][0] / 1e6, 1)}


VARIANTS = {"b_user_autocast": dict(autocast=True),
            "c_bf16_optin_aten": dict(bf16=True),
            "d_bf16_optin_native": dict(bf16=True, route="native"),
            "e_native_norm": dict(bf16=True, route="native", norm=True),
            "f_aten_norm": dict(bf16=True, norm=True)}


def train_step(n, steps, warmup, dev):
    torch.manual_seed(0)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(dev)
    m.apply(deactivate_batchnorm)
    m.train().enable_head_training()
    x = torch.rand(1, n, 3, 224, 224, device=dev)
    target = torch.tensor([1], device=dev)

    def step(bf16=False, autocast=False, route="aten", norm=False):
        os.environ["MCGMIL_CONV_GRAD"] = route
        m.enable_bf16_backbone_training(bf16).enable_bf16_norm_training(bf16 and norm)
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", BF, enabled=autocast):
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
    out["fastest"] = min(variants, key=lambda key: t[key][0])
    out["e_vs_d"] = verdict(t["e_native_norm"], t["d_bf16_optin_native"])
    out["f_vs_c"] = verdict(t["f_aten_norm"], t["c_bf16_optin_aten"])
    out["e_vs_b"] = verdict(t["e_native_norm"], t["b_user_autocast"])
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
    dev = torch.device("cuda", 0)
    out = {"bench": "norm_grad_bf16", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "shapes": [], "train_step": []}
    f = lambda v: f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    print("| shape | n | form | op fwd+bwd ms (min-max) | torch autocast layers | torch / op | op | backward ms | "
          "algorithmic MB | GB/s |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|---|", file=sys.stderr)
    for n in [] if a.no_shapes else [int(v) for v in a.instances.split(",") if v]:
        for shape in R18:
            for form in FORMS:
                r = bench_shape(shape, n, form, a.steps, a.warmup, dev)
                out["shapes"].append(r)
                print(f"| {r['shape']} {r['C']} x {r['hw']}^2 | {n} | {r['form']} | {f(r['op_ms'])} | {f(r['torch_ms'])} | "
                      f"{r['ratio']:.2f} | {r['op']} | {f(r['bwd_ms'])} | {r['bwd_algo_mb']} | {r['bwd_gbs']} |",
                      file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    print("| instances | b autocast ms (min-max) | c opt-in aten | d opt-in native | e = d + norm | f = c + norm | "
          "fastest | e vs d | f vs c | e vs b | peak MiB b / c / d / e / f |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|---|---|", file=sys.stderr)
    for n in [] if a.no_steps else [int(v) for v in a.bags.split(",") if v]:
        r = train_step(n, a.steps, a.warmup, dev)
        out["train_step"].append(r)
        print(f"| {n} | " + " | ".join(f(r[k + "_ms"]) for k in VARIANTS) + f" | {r['fastest'][0]} | {r['e_vs_d']} | "
              f"{r['f_vs_c']} | {r['e_vs_b']} | " + " / ".join(str(r[k + "_peak_mib"]) for k in VARIANTS) + " |",
              file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
