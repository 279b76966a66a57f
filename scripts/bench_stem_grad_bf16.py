"""Time the fused bf16 stem BatchNorm/ReLU/max-pool training op (torch.ops.mcgmil.bn_pool_bf16: the
fused HIP forward in bf16 that records the pool's argmax codes, and the HIP backward of
include/mcgmil_pool_grad_bf16.h) against the torch layers under autocast on the same tensors, in one
process on one GPU.

The stem's layers, maxpool(relu(bn1(z))) on z = 64 x 112 x 112 per instance with the 3 / 2 / 1
pool, at --instances (default 64, 256 and 1,507) instances -- forward + backward with z bf16 and the
fp32 BN parameters requiring gradients: "op" (features.bn_act inside native_stem_bf16_training())
against "torch" (bn(z), torch.relu, max_pool2d under torch.autocast("cuda", torch.bfloat16)),
interleaved call by call. Each call is timed with HIP events: --warmup calls, then --steps timed
ones, median and min-max. The op "wins" ("loses") when the medians differ by more than the larger
of the two min-max spreads, else it "ties". The bytes autograd saves for the backward are counted
with saved_tensors_hooks on one call of each.
The backward's achieved bandwidth is its algorithmic bytes (z read once and dz written once, 2 bytes
each; dy read once, 2 bytes, and the codes once, 1 byte, per pooled element) over the median of the
C ABI call on the same tensors; the kernels read z twice and dy and the codes about 2.25 times per
pass, so the traffic they cause is higher than that.

Then a whole training step, forward() + backward() of MultiHeadGatedAttentionMIL (r18, head
training on, batch-statistics BatchNorm) on one bag of --bags instances, interleaved, with the peak
memory of a step above what is allocated before it:
  b  the user's own torch.autocast("cuda", torch.bfloat16) over the torch layers
  d  enable_bf16_backbone_training() with MCGMIL_CONV_GRAD=native
  e  d + enable_bf16_norm_training()
  g  e + enable_bf16_stem_training()
  h  d + enable_bf16_stem_training()

Prints the tables (markdown) on stderr and one JSON line on stdout.
Usage: python scripts/bench_stem_grad_bf16.py [--steps 20] [--warmup 5] [--instances 64,256,1507]
                                               [--bags 64,256,1507] [--no-shapes] [--no-steps]
"""
import argparse
import contextlib
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
STEM = ("stem", 64, 112, (3, 2, 1))         # name, C, H = W of z, the pool


def capi_backward(L, z, code, dy, gamma, mean, invstd, pool, outs, ws):
    a = _lib.BnPoolGradBf16Args()
    a.batch, a.channels, a.height, a.width = z.shape
    a.pool_kernel, a.pool_stride, a.pool_pad = pool
    a.pooled_height, a.pooled_width = dy.shape[2:]
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a.z, a.argmax, a.dy, a.gamma, a.mean, a.invstd = p(z), p(code), p(dy), p(gamma), p(mean), p(invstd)
    a.dz, a.dgamma, a.dbeta = (p(outs.get(k)) for k in ("dz", "dgamma", "dbeta"))
    a.workspace, a.workspace_bytes = p(ws), ws.numel()
    rc = L.mcgmil_batchnorm_pool_backward_bf16(ctypes.byref(a),
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc:
        raise RuntimeError(f"mcgmil_batchnorm_pool_backward_bf16 failed ({rc}): {L.mcgmil_last_error().decode()}")


def bench_shape(n, steps, warmup, dev):
    name, C, hw, pool_p = STEM
    cl = torch.channels_last
    bn = nn.BatchNorm2d(C).to(dev)
    deactivate_batchnorm(bn)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    pool = nn.MaxPool2d(*pool_p)
    z = torch.randn(n, C, hw, hw, device=dev).to(BF).contiguous(memory_format=cl).requires_grad_()
    with torch.no_grad():
        y, mean, invstd, code = features.batchnorm_pool_stats_bf16(z.detach(), bn.weight.detach(), bn.bias.detach(),
                                                                   bn.eps, True, *pool_p)
    dy = torch.randn(y.shape, device=dev).to(BF).contiguous(memory_format=cl)

    def fwd_bwd(native, seen=None):
        for t in (z, bn.weight, bn.bias):
            t.grad = None
        hooks = contextlib.nullcontext() if seen is None else torch.autograd.graph.saved_tensors_hooks(
            lambda t: seen.append(t.numel() * t.element_size()) or t, lambda t: t)
        with torch.autocast("cuda", BF), features.native_stem_bf16_training(native), hooks:
            out = features.bn_act(bn, z, True, pool=pool)
        out.backward(dy)
    saved = {}
    for key, native in (("op", True), ("torch", False)):
        seen = []
        fwd_bwd(native, seen)
        saved[key] = sum(seen)
    L = _lib.load()
    a = _lib.BnPoolGradBf16Args()
    a.batch, a.channels, a.height, a.width = z.shape
    a.pool_kernel, a.pool_stride, a.pool_pad = pool_p
    a.pooled_height, a.pooled_width = y.shape[2:]
    nbytes = ctypes.c_size_t()
    _lib.check(L.mcgmil_bn_pool_grad_workspace_size_bf16(ctypes.byref(a), ctypes.byref(nbytes)),
               "mcgmil_bn_pool_grad_workspace_size_bf16")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    full = {"dz": torch.empty_like(z.detach()), "dgamma": torch.empty_like(mean), "dbeta": torch.empty_like(mean)}
    args = (z.detach(), code, dy, bn.weight.detach(), mean, invstd, pool_p)
    fns = {"op": lambda: fwd_bwd(True), "torch": lambda: fwd_bwd(False),
           "bwd": lambda: capi_backward(L, *args, full, ws)}
    t = interleaved(fns, steps, warmup)
    algo = 2 * z.numel() * 2 + y.numel() * (2 + 1)          # bytes
    rnd = lambda v: [round(c, 4) for c in v]  # noqa: E731
    return {"shape": name, "C": C, "hw": hw, "n": n, "op_ms": rnd(t["op"]), "torch_ms": rnd(t["torch"]),
            "ratio": round(t["torch"][0] / t["op"][0], 3), "op": verdict(t["op"], t["torch"]),
            "bwd_ms": rnd(t["bwd"]), "bwd_algo_mb": round(algo / 1e6, 1), "bwd_gbs": round(algo / t["bwd"][0] / 1e6, 1),
            "saved_op_mb": round(saved["op"] / 1e6, 1), "saved_torch_mb": round(saved["torch"] / 1e6, 1)}


VARIANTS = {"b_user_autocast": dict(autocast=True),
            "d_bf16_optin_native": dict(bf16=True, route="native"),
            "e_native_norm": dict(bf16=True, route="native", norm=True),
            "g_native_norm_stem": dict(bf16=True, route="native", norm=True, stem=True),
            "h_native_stem": dict(bf16=True, route="native", stem=True)}


def train_step(n, steps, warmup, dev):
    torch.manual_seed(0)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(dev)
    m.apply(deactivate_batchnorm)
    m.train().enable_head_training()
    x = torch.rand(1, n, 3, 224, 224, device=dev)
    target = torch.tensor([1], device=dev)

    def step(bf16=False, autocast=False, route="aten", norm=False, stem=False):
        os.environ["MCGMIL_CONV_GRAD"] = route
        m.enable_bf16_backbone_training(bf16).enable_bf16_norm_training(bf16 and norm)
        m.enable_bf16_stem_training(bf16 and stem)
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
    out["g_vs_e"] = verdict(t["g_native_norm_stem"], t["e_native_norm"])
    out["h_vs_d"] = verdict(t["h_native_stem"], t["d_bf16_optin_native"])
    out["g_vs_b"] = verdict(t["g_native_norm_stem"], t["b_user_autocast"])
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
    out = {"bench": "stem_grad_bf16", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "shapes": [], "train_step": []}
    f = lambda v: f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    print("| shape | n | op fwd+bwd ms (min-max) | torch autocast layers | torch / op | op | backward ms | "
          "algorithmic MB | GB/s | saved MB op / torch |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|---|", file=sys.stderr)
    for n in [] if a.no_shapes else [int(v) for v in a.instances.split(",") if v]:
        r = bench_shape(n, a.steps, a.warmup, dev)
        out["shapes"].append(r)
        print(f"| {r['shape']} {r['C']} x {r['hw']}^2 | {n} | {f(r['op_ms'])} | {f(r['torch_ms'])} | "
              f"{r['ratio']:.2f} | {r['op']} | {f(r['bwd_ms'])} | {r['bwd_algo_mb']} | {r['bwd_gbs']} | "
              f"{r['saved_op_mb']} / {r['saved_torch_mb']} |", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print("| instances | b autocast ms (min-max) | d opt-in native | e = d + norm | g = e + stem | h = d + stem | "
          "fastest | g vs e | h vs d | g vs b | peak MiB b / d / e / g / h |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|---|---|", file=sys.stderr)
    for n in [] if a.no_steps else [int(v) for v in a.bags.split(",") if v]:
        r = train_step(n, a.steps, a.warmup, dev)
        out["train_step"].append(r)
        print(f"| {n} | " + " | ".join(f(r[k + "_ms"]) for k in VARIANTS) + f" | {r['fastest'][0]} | {r['g_vs_e']} | "
              f"{r['h_vs_d']} | {r['g_vs_b']} | " + " / ".join(str(r[k + "_peak_mib"]) for k in VARIANTS) + " |",
              file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
