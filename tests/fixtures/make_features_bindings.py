"""What mcgmil.features hands to the C ABI, recorded on the CPU (no library, no device), and the
generator of tests/fixtures/features_bindings.json:

    python tests/fixtures/make_features_bindings.py            # writes the fixture (HEAD's hash in it)

`record()` runs every wrapper of features.py that calls the library with `features._lib.load`
replaced by a stub and `torch.cuda.current_stream` by a dummy. The inputs are `OnGpu` tensors: CPU
tensors whose is_cuda is True, each filled with a constant of its own. For every library call the
stub records the entry point, every non-zero scalar field of the args struct (nested `fwd`
included), and for every non-NULL pointer field "ws" (the workspace), "out" (an output field) or
the first 4 bytes behind it. Size queries get WS_BYTES / PARTS through their out-parameter; a
launch gets a 4-byte constant of the field's own (`mark`) written through every output pointer, so
that the caller can tell which field each returned tensor came from: a swapped pointer shows.
It also records the verdict (and reason) of every predicate over a table of layers, activations,
env switches, autocast and requires_grad, and the schema of every torch.ops.mcgmil op.

The fixture is generated once, from the commit BEFORE a change to the bindings, and committed with
the change; tests/test_features_bindings_host.py compares record() of the tree with it.
"""
import contextlib
import ctypes
import json
import os
import struct
import subprocess
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, os.path.join(REPO, "montecarlo-gated-mil_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from mcgmil import features, library  # noqa: E402,F401

FIXTURE = os.path.join(HERE, "features_bindings.json")
CL, F32, BF = torch.channels_last, torch.float32, torch.bfloat16
WS_BYTES, PARTS, STREAM = 512, 3, 0x5EED00
OUTPUT_FIELDS = ("y", "dx", "dw", "dz", "dresidual", "dgamma", "dbeta", "stats", "batch_mean", "batch_invstd")
# the arguments after the args struct and before the stream: (name, "in" | "int" | "out")
TRAILING = {
    "mcgmil_pack_conv_weights": (("weight", "in"), ("weight_dtype", "int"), ("packed", "out")),
    "mcgmil_pack_conv_weights_f32": (("weight", "in"), ("packed", "out")),
    "mcgmil_pack_stem_weights": (("weight", "in"), ("weight_dtype", "int"), ("packed", "out")),
    "mcgmil_batchnorm_coefficients": (("ab", "out"),),
    "mcgmil_batchnorm_pool_train": (("argmax", "out"),),
    "mcgmil_batchnorm_pool_train_bf16": (("argmax", "out"),),
}


def mark(field: str) -> bytes:
    """The 4 bytes the stub writes through the output pointer `field`."""
    return struct.pack("<I", zlib.crc32(field.encode()) | 0x01010101)


MARKS = {mark(f): f for f in OUTPUT_FIELDS + ("argmax", "ab", "packed")}


class OnGpu(torch.Tensor):
    """A CPU tensor that says it is a CUDA one: past the predicates without a device."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    is_cuda = property(lambda self: True)


def _peek(ptr) -> str:
    return ctypes.string_at(ptr, 4).hex()


def came_from(t):
    """The output field a returned tensor was written through (None for None, "?" for neither)."""
    if t is None or t.numel() == 0:
        return None if t is None else "empty"
    return MARKS.get(ctypes.string_at(t.data_ptr(), 4), "?")


class Stub:
    """Stands in for the loaded library: every attribute is a recording entry point."""

    def __init__(self, ws_bytes=WS_BYTES, parts=PARTS, keep=True):
        self.ws_bytes, self.parts, self.keep, self.calls = ws_bytes, parts, keep, []

    def __getattr__(self, name):
        def entry(*args):
            return self._call(name, args)
        self.__dict__[name] = entry
        return entry

    def _call(self, name, args):
        objs = [getattr(a, "_obj", a) for a in args]              # byref(x) -> x
        query = False
        for o in objs[1:]:
            if isinstance(o, ctypes.c_size_t):
                o.value, query = self.ws_bytes, True
            elif isinstance(o, ctypes.c_int32):
                o.value, query = self.parts, True
        rec = {"fn": name}
        if self.keep:
            self._struct(objs[0], rec, "", write=not query)
        if not query:                                             # a launch: ..., stream
            last = objs[-1]
            rec["stream"] = isinstance(last, ctypes.c_void_p) and last.value == STREAM
            for (arg, kind), o in zip(TRAILING.get(name, ()), objs[1:-1]):
                v = o.value if isinstance(o, ctypes.c_void_p) else o
                if kind == "int":
                    rec[arg] = int(v)
                elif v and kind == "in":
                    rec[arg] = _peek(v)
                elif v:
                    rec[arg] = "out"
                    ctypes.memmove(v, mark(arg), 4)
            if len(objs) - 2 != len(TRAILING.get(name, ())):
                rec["unexpected_args"] = len(objs)
        if self.keep:
            self.calls.append(rec)
        return 0

    def _struct(self, s, rec, prefix, write):
        outs = []
        for fname, ftype in s._fields_:
            v, key = getattr(s, fname), prefix + fname
            if isinstance(v, ctypes.Structure):
                self._struct(v, rec, key + ".", write)
            elif ftype is ctypes.c_void_p:
                if v:
                    rec[key] = "ws" if fname == "workspace" else "out" if fname in OUTPUT_FIELDS else _peek(v)
                    if write and fname in OUTPUT_FIELDS:
                        outs.append((v, fname))
            elif v:
                rec[key] = v
        for v, fname in outs:                                     # after every input has been read
            ctypes.memmove(v, mark(fname), 4)


class _Stream:
    cuda_stream = STREAM


@contextlib.contextmanager
def stubbed(stub):
    load, stream = features._lib.load, torch.cuda.current_stream
    features._lib.load, torch.cuda.current_stream = (lambda: stub), (lambda *a, **k: _Stream)
    try:
        yield stub
    finally:
        features._lib.load, torch.cuda.current_stream = load, stream


@contextlib.contextmanager
def env(**kw):
    before = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@contextlib.contextmanager
def cuda_autocast_bf16():
    """torch.is_autocast_enabled("cuda") without a device (torch.autocast would switch itself off)."""
    on, dt = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    torch.set_autocast_enabled("cuda", True)
    torch.set_autocast_dtype("cuda", BF)
    try:
        yield
    finally:
        torch.set_autocast_enabled("cuda", on)
        torch.set_autocast_dtype("cuda", dt)


# ---------------------------------------------------------------- inputs, each with its own constant
def full(shape, dtype, value, cl=True, gpu=True):
    t = torch.full(shape, float(value), dtype=dtype)
    if cl and t.dim() == 4:
        t = t.contiguous(memory_format=CL)
    return OnGpu(t) if gpu else t


def conv(cin, cout, k=3, stride=1, pad=1, dtype=F32):
    c = nn.Conv2d(cin, cout, k, stride, pad, bias=False).to(dtype)
    with torch.no_grad():
        c.weight.fill_(2.0)
    return c


def bnorm(C, mode="batch", affine=True):
    """mode "batch": no running statistics (the reference's deactivate_batchnorm); "running": eval."""
    bn = nn.BatchNorm2d(C, affine=affine, track_running_stats=mode == "running")
    with torch.no_grad():
        if affine:
            bn.weight.fill_(5.0), bn.bias.fill_(6.0)
        if mode == "running":
            bn.running_mean.fill_(7.0), bn.running_var.fill_(8.0)
    return bn.eval() if mode == "running" else bn


def vec(C, value):
    return torch.full((C,), float(value))


def oh(h, k, s, p):
    return (h + 2 * p - k) // s + 1


H, W = 9, 7


def _conv_cases():
    f = features
    x64 = lambda: full((2, 64, H, W), BF, 1)          # noqa: E731
    x16 = lambda: full((2, 16, H, W), F32, 1)         # noqa: E731
    ab = lambda C: torch.full((2, C), 4.0)            # noqa: E731
    c = {}
    c["packed_conv_weight/f32w"] = lambda: (f.packed_conv_weight(conv(64, 64), x64()),)
    c["packed_conv_weight/bf16w"] = lambda: (f.packed_conv_weight(conv(64, 64, dtype=BF), x64()),)
    c["packed_conv_weight/f64w"] = lambda: (f.packed_conv_weight(conv(64, 64).double(), x64()),)

    def cached():
        cv = conv(64, 64)
        return f.packed_conv_weight(cv, x64()), f.packed_conv_weight(cv, x64())
    c["packed_conv_weight/cached"] = cached
    c["packed_conv_weight_f32"] = lambda: (f.packed_conv_weight_f32(conv(16, 64), x16()),)
    c["conv_input_bn"] = lambda: (None,) if f.conv_input_bn(conv(64, 64, dtype=BF), x64()) else ()
    b64 = lambda **kw: conv(64, 64, dtype=BF, **kw)   # noqa: E731
    c["conv2d"] = lambda: (f.conv2d(b64(), x64()),)
    c["conv2d/stats"] = lambda: f.conv2d(b64(), x64(), stats=True)
    c["conv2d/in_ab"] = lambda: (f.conv2d(b64(), x64(), in_ab=ab(64)),)
    c["conv2d/in_ab_norelu_stats"] = lambda: f.conv2d(b64(), x64(), True, ab(64), False)
    c["conv2d/flags"] = lambda: (f.conv2d(b64(), x64(), flags=2),)
    c["conv2d/stride2"] = lambda: (f.conv2d(b64(stride=2), x64()),)
    c["conv2d/1x1_128"] = lambda: (f.conv2d(conv(64, 128, 1, 2, 0, BF), x64()),)
    c["conv2d_f32"] = lambda: (f.conv2d_f32(conv(16, 64), x16()),)
    c["conv2d_f32/stats"] = lambda: f.conv2d_f32(conv(16, 64), x16(), stats=True)
    c["conv2d_f32/in_ab"] = lambda: (f.conv2d_f32(conv(16, 64), x16(), in_ab=ab(16)),)
    c["conv2d_f32/in_ab_norelu_stats"] = lambda: f.conv2d_f32(conv(16, 64), x16(), True, ab(16), False)
    c["conv2d_f32/stride2"] = lambda: (f.conv2d_f32(conv(16, 64, stride=2), x16()),)
    c["conv2d_f32/stem"] = lambda: (f.conv2d_f32(conv(3, 64, 7, 2, 3), full((2, 3, H, W), F32, 1)),)
    c["conv2d_bf16"] = lambda: (f.conv2d_bf16(conv(64, 64), x64()),)
    for s in (1, 2):
        dy = lambda s=s, dt=F32, cl=True: full((2, 64, oh(H, 3, s, 1), oh(W, 3, s, 1)), dt, 3, cl=cl, gpu=False)  # noqa: E731
        c[f"conv2d_f32_wgrad/s{s}"] = lambda s=s, dy=dy: (f.conv2d_f32_wgrad(conv(16, 64, stride=s), x16(), dy()),)
        c[f"conv2d_bf16_wgrad/s{s}"] = lambda s=s, dy=dy: (f.conv2d_bf16_wgrad(conv(64, 64, stride=s), x64(), dy(dt=BF)),)
        c[f"conv2d_f32_dgrad_direct/s{s}"] = lambda s=s, dy=dy: (
            f.conv2d_f32_dgrad_direct(conv(16, 64, stride=s), OnGpu(dy()), (2, 16, H, W)),)
    c["conv2d_f32_wgrad/chunk_nhwc_dy"] = lambda: (
        f.conv2d_f32_wgrad(conv(16, 64), x16(), full((2, 64, H, W), F32, 3, cl=False, gpu=False), chunk_pixels=4096),)
    c["conv2d_bf16_wgrad/chunk"] = lambda: (
        f.conv2d_bf16_wgrad(conv(64, 64), x64(), full((2, 64, H, W), BF, 3, gpu=False), 2048),)
    for s, k, p in ((2, 7, 3), (1, 3, 1)):
        c[f"conv2d_f32_stem_wgrad/s{s}"] = lambda s=s, k=k, p=p: (f.conv2d_f32_stem_wgrad(
            conv(3, 64, k, s, p), full((2, 3, H, W), F32, 1),
            full((2, 64, oh(H, k, s, p), oh(W, k, s, p)), F32, 3, gpu=False), 4096 * (s - 1)),)
    c["conv2d_f32_dgrad/native16"] = lambda: (
        f.conv2d_f32_dgrad(conv(16, 64), full((2, 64, H, W), F32, 3), (2, 16, H, W)),)
    c["conv2d_f32_dgrad/native64_5x5"] = lambda: (
        f.conv2d_f32_dgrad(conv(64, 64, 5, 1, 1), full((2, 64, H - 2, W - 2), F32, 3), (2, 64, H, W)),)
    c["conv2d_bf16_dgrad/native"] = lambda: (
        f.conv2d_bf16_dgrad(conv(64, 64), full((2, 64, H, W), BF, 3), x64()),)
    return c


def _bn_cases():
    f = features
    x = {F32: lambda: full((2, 8, H, W), F32, 1), BF: lambda: full((2, 64, H, W), BF, 1)}
    C = {F32: 8, BF: 64}
    c = {}
    for dt, tag in ((F32, "f32"), (BF, "bf16")):
        n = C[dt]
        like = lambda v, dt=dt, n=n: full((2, n, H, W), dt, v)                      # noqa: E731
        part = lambda n=n: torch.full((4, 3, n), 9.0)                                 # noqa: E731
        c[f"batchnorm_act/{tag}/relu"] = lambda dt=dt, n=n: (f.batchnorm_act(x[dt](), bnorm(n), True),)
        c[f"batchnorm_act/{tag}/norelu_residual"] = lambda dt=dt, n=n, like=like: (
            f.batchnorm_act(x[dt](), bnorm(n), False, like(10)),)
        c[f"batchnorm_act/{tag}/residual_ab_partials"] = lambda dt=dt, n=n, like=like, part=part: (
            f.batchnorm_act(x[dt](), bnorm(n), True, like(10), partials=part(), residual_ab=torch.full((2, n), 11.0)),)
        c[f"batchnorm_act/{tag}/pool"] = lambda dt=dt, n=n: (
            f.batchnorm_act(x[dt](), bnorm(n), True, pool=nn.MaxPool2d(3, 2, 1)),)
        c[f"batchnorm_act/{tag}/pool2_partials"] = lambda dt=dt, n=n, part=part: (
            f.batchnorm_act(x[dt](), bnorm(n), False, pool=nn.MaxPool2d(2), partials=part()),)
        c[f"batchnorm_act/{tag}/running"] = lambda dt=dt, n=n, part=part: (
            f.batchnorm_act(x[dt](), bnorm(n, "running"), True, partials=part()),)
        c[f"batchnorm_act/{tag}/no_affine"] = lambda dt=dt, n=n: (f.batchnorm_act(x[dt](), bnorm(n, affine=False), True),)
        c[f"batchnorm_coefficients/{tag}"] = lambda dt=dt, n=n: (f.batchnorm_coefficients(x[dt](), bnorm(n)),)
        c[f"batchnorm_coefficients/{tag}/partials"] = lambda dt=dt, n=n, part=part: (
            f.batchnorm_coefficients(x[dt](), bnorm(n), part()),)
        c[f"batchnorm_coefficients/{tag}/running"] = lambda dt=dt, n=n, part=part: (
            f.batchnorm_coefficients(x[dt](), bnorm(n, "running"), part()),)
        sfx = "" if dt is F32 else "_bf16"
        stats, back = getattr(f, "batchnorm_act_stats" + sfx), getattr(f, "batchnorm_act_backward" + sfx)
        pstats, pback = getattr(f, "batchnorm_pool_stats" + sfx), getattr(f, "batchnorm_pool_backward" + sfx)
        g, b, m, i = (lambda n=n, v=v: vec(n, v) for v in (5, 6, 12, 13))
        c[f"batchnorm_act_stats/{tag}/relu"] = lambda dt=dt, s=stats, g=g, b=b: s(x[dt](), g(), b(), None, 1e-5, True)
        c[f"batchnorm_act_stats/{tag}/norelu_residual"] = lambda dt=dt, s=stats, g=g, b=b, like=like: (
            s(x[dt](), g(), b(), like(10), 1e-3, False))
        c[f"batchnorm_act_stats/{tag}/no_affine"] = lambda dt=dt, s=stats: s(x[dt](), None, None, None, 1e-5, True)
        for name, kw in (("all", dict(need_dres=True)), ("default", {}), ("no_dx", dict(need_dx=False)),
                         ("no_dw", dict(need_dw=False)), ("none", dict(need_dx=False, need_dw=False))):
            c[f"batchnorm_act_backward/{tag}/relu_{name}"] = lambda dt=dt, back=back, like=like, g=g, m=m, i=i, kw=kw: (
                back(x[dt](), like(14), like(3), g(), m(), i(), True, **kw))
        c[f"batchnorm_act_backward/{tag}/norelu_dres_asked"] = lambda dt=dt, back=back, like=like, g=g, m=m, i=i: (
            back(x[dt](), None, like(3), g(), m(), i(), False, need_dres=True))
        c[f"batchnorm_act_backward/{tag}/norelu_y_no_affine"] = lambda dt=dt, back=back, like=like, m=m, i=i: (
            back(x[dt](), like(14), like(3), None, m(), i(), False))
        for k, s, p in ((3, 2, 1), (2, 2, 0)):
            geo = f"k{k}s{s}p{p}"
            pooled = lambda dtp, v, n=n, k=k, s=s, p=p: full((2, n, oh(H, k, s, p), oh(W, k, s, p)), dtp, v)  # noqa: E731
            c[f"batchnorm_pool_stats/{tag}/{geo}"] = lambda dt=dt, ps=pstats, g=g, b=b, k=k, s=s, p=p: (
                ps(x[dt](), g(), b(), 1e-5, k == 3, k, s, p))
            for name, kw in (("default", {}), ("no_dz", dict(need_dz=False)), ("no_dw", dict(need_dw=False)),
                             ("none", dict(need_dz=False, need_dw=False))):
                if k == 2 and name != "default":
                    continue
                c[f"batchnorm_pool_backward/{tag}/{geo}_{name}"] = \
                    lambda dt=dt, pb=pback, pooled=pooled, g=g, m=m, i=i, k=k, s=s, p=p, kw=kw: (
                        pb(x[dt](), pooled(torch.uint8, 15), pooled(dt, 3), g(), m(), i(), k, s, p, **kw))
        c[f"batchnorm_pool_stats/{tag}/no_affine"] = lambda dt=dt, ps=pstats: ps(x[dt](), None, None, 1e-5, True, 3, 2, 1)
    return c


def _stem_cases():
    f = features
    xs = lambda dt=BF: full((2, 3, 10, 8), dt, 1, cl=False)     # noqa: E731
    st = lambda dt=F32: conv(3, 64, 7, 2, 3, dt)                # noqa: E731
    c = {}
    c["packed_stem_weight/f32w"] = lambda: (f.packed_stem_weight(st(), xs()),)
    c["packed_stem_weight/bf16w"] = lambda: (f.packed_stem_weight(st(BF), xs()),)
    c["packed_stem_weight/f64w"] = lambda: (f.packed_stem_weight(st().double(), xs()),)
    c["stem/pool"] = lambda: (f.stem(st(), bnorm(64), True, nn.MaxPool2d(3, 2, 1), xs()),)
    c["stem/nopool_norelu_flags"] = lambda: (f.stem(st(), bnorm(64), False, None, xs(), flags=1),)
    c["stem/running_f32x_bf16w"] = lambda: (f.stem(st(BF), bnorm(64, "running"), True, nn.MaxPool2d(2), xs(F32)),)
    c["stem/no_affine"] = lambda: (f.stem(st(), bnorm(64, affine=False), True, None, xs()),)
    return c


def wrapper_cases():
    """name -> a call that builds fresh inputs, runs one wrapper and returns its tensors as a tuple."""
    return {**_conv_cases(), **_bn_cases(), **_stem_cases()}


def _flat(out):
    return [out] if out is None or isinstance(out, torch.Tensor) else list(out)


def record_wrappers():
    got = {}
    with torch.no_grad():
        for name, call in wrapper_cases().items():
            with stubbed(Stub()) as stub:
                out = call()
            got[name] = {"calls": stub.calls, "returns": [came_from(t) for t in _flat(out)]}
        # sizes of zero: conv2d allocates no workspace and no statistics, the others an empty workspace
        for name in ("conv2d/stats", "batchnorm_act/f32/relu", "batchnorm_coefficients/f32", "conv2d_f32_wgrad/s1",
                     "batchnorm_act_backward/f32/relu_default", "batchnorm_pool_backward/f32/k3s2p1_default"):
            with stubbed(Stub(ws_bytes=0, parts=0)) as stub:
                out = wrapper_cases()[name]()
            got[name + "@zero"] = {"calls": stub.calls, "returns": [came_from(t) for t in _flat(out)]}
        with env(MCGMIL_CONV_SPLIT="0"), stubbed(Stub()) as stub:
            out = wrapper_cases()["conv2d/stats"]()
        got["conv2d/stats@nosplit"] = {"calls": stub.calls, "returns": [came_from(t) for t in _flat(out)]}
    return got


# ---------------------------------------------------------------- predicates
def _stem_layer(**kw):
    args = dict(in_channels=3, out_channels=64, kernel_size=7, stride=2, padding=3, bias=False)
    args.update(kw)
    return nn.Conv2d(**args)


def _block_layer(**kw):
    args = dict(in_channels=64, out_channels=128, kernel_size=3, stride=1, padding=1, bias=False)
    args.update(kw)
    return nn.Conv2d(**args)


# the tables of test_stem_conv_grad_host.test_each_clause and test_conv_grad_bf16_host.test_each_clause
CONV_LAYERS = [
    (lambda: _stem_layer(), (2, 3, 16, 16)),
    (lambda: _stem_layer(in_channels=1), (2, 1, 16, 16)),
    (lambda: _stem_layer(in_channels=4, kernel_size=(3, 7), padding=1), (2, 4, 16, 16)),
    (lambda: _stem_layer(in_channels=5), (2, 5, 16, 16)),
    (lambda: _stem_layer(in_channels=16), (2, 16, 16, 16)),
    (lambda: _stem_layer(out_channels=96), (2, 3, 16, 16)),
    (lambda: _stem_layer(bias=True), (2, 3, 16, 16)),
    (lambda: _stem_layer(in_channels=4, groups=2), (2, 4, 16, 16)),
    (lambda: _stem_layer(stride=3), (2, 3, 16, 16)),
    (lambda: _stem_layer(dilation=2), (2, 3, 16, 16)),
    (lambda: _stem_layer(kernel_size=3, padding=3), (2, 3, 16, 16)),
    (lambda: _stem_layer(kernel_size=9, padding=4), (2, 3, 16, 16)),
    (lambda: _stem_layer(padding=(3, 2)), (2, 3, 16, 16)),
    (lambda: _stem_layer(padding="same", stride=1), (2, 3, 16, 16)),
    (lambda: _stem_layer(), (2, 4, 16, 16)),
    (lambda: _stem_layer().double(), (2, 3, 16, 16)),
    (lambda: nn.Linear(3, 3), (2, 3, 16, 16)),
    (lambda: _block_layer(), (2, 64, 8, 8)),
    (lambda: _block_layer().to(BF), (2, 64, 8, 8)),
    (lambda: _block_layer(stride=2), (2, 64, 9, 11)),
    (lambda: _block_layer(in_channels=256, out_channels=64, kernel_size=1, padding=0), (1, 256, 7, 7)),
    (lambda: _block_layer(kernel_size=(3, 7), padding=2), (2, 64, 8, 8)),
    (lambda: _block_layer(in_channels=48), (2, 48, 8, 8)),
    (lambda: _block_layer(in_channels=16), (2, 16, 8, 8)),
    (lambda: _block_layer(out_channels=96), (2, 64, 8, 8)),
    (lambda: _block_layer(bias=True), (2, 64, 8, 8)),
    (lambda: _block_layer(groups=2), (2, 64, 8, 8)),
    (lambda: _block_layer(stride=3), (2, 64, 8, 8)),
    (lambda: _block_layer(dilation=2), (2, 64, 8, 8)),
    (lambda: _block_layer(padding=3), (2, 64, 8, 8)),
    (lambda: _block_layer(kernel_size=9, padding=4), (2, 64, 16, 16)),
    (lambda: _block_layer(padding=(1, 0)), (2, 64, 8, 8)),
    (lambda: _block_layer(padding="same"), (2, 64, 8, 8)),
    (lambda: _block_layer(), (2, 128, 8, 8)),
    (lambda: _block_layer().double(), (2, 64, 8, 8)),
    (lambda: nn.Linear(3, 3), (2, 64, 8, 8)),
    # beyond those tables: the stem's other domain (kh * kw * in <= 1024), a 1x1 on one pixel, out_channels > 4096
    (lambda: _stem_layer(in_channels=24, kernel_size=7), (2, 24, 16, 16)),
    (lambda: _block_layer(kernel_size=3, padding=0), (2, 64, 2, 2)),
    (lambda: _stem_layer(out_channels=4160), (1, 3, 8, 8)),
]
# activations beyond the zeros(x_shape) of the tables, for the first stem and the first block layer
ODD_X = {
    "nchw": lambda s, dt: OnGpu(torch.zeros(s, dtype=dt)),
    "3d": lambda s, dt: OnGpu(torch.zeros(s[1:], dtype=dt)),
    "f64": lambda s, dt: OnGpu(torch.zeros(s, dtype=torch.float64).contiguous(memory_format=CL)),
    "empty": lambda s, dt: OnGpu(torch.zeros((0,) + tuple(s[1:]), dtype=dt).contiguous(memory_format=CL)),
    "cpu": lambda s, dt: torch.zeros(s, dtype=dt).contiguous(memory_format=CL),
    # the size clauses, on meta tensors: 2^31 bytes of bf16, H > 16383, 2^31 output pixels
    "2gib": lambda s, dt: OnGpu(torch.empty((4, s[1], 2048, 2 ** 22 // s[1]), dtype=dt, device="meta")
                                .contiguous(memory_format=CL)),
    "tall": lambda s, dt: OnGpu(torch.empty((1, s[1], 16384, 8), dtype=dt, device="meta").contiguous(memory_format=CL)),
    "pixels": lambda s, dt: OnGpu(torch.empty((2, s[1], 32768, 32768), dtype=dt, device="meta")
                                  .contiguous(memory_format=CL)),
}
MODES = {
    "default": contextlib.nullcontext,
    "MCGMIL_NATIVE_CONV=0": lambda: env(MCGMIL_NATIVE_CONV="0"),
    "MCGMIL_NATIVE_CONV32=0": lambda: env(MCGMIL_NATIVE_CONV32="0"),
    "MCGMIL_FUSED_BN=0": lambda: env(MCGMIL_FUSED_BN="0"),
    "MCGMIL_NATIVE_STEM=0": lambda: env(MCGMIL_NATIVE_STEM="0"),
    "cpu_autocast": lambda: torch.autocast("cpu", BF),
    "cuda_autocast": cuda_autocast_bf16,
    "requires_grad": contextlib.nullcontext,
}
CONV_PREDICATES = ("conv_fusable", "conv32_fusable", "conv32_trainable", "stem_conv_untrainable_reason",
                   "stem_conv_trainable", "conv_bf16_untrainable_reason", "conv_bf16_trainable",
                   "dgrad_direct_supported(dy)", "dgrad_direct_supported(x)", "conv_input_bn", "conv32_input_bn")


def _conv_verdicts(layer, x):
    f = features
    out = [f.conv_fusable(layer, x), f.conv32_fusable(layer, x), f.conv32_trainable(layer, x),
           f.stem_conv_untrainable_reason(layer, x), f.stem_conv_trainable(layer, x),
           f.conv_bf16_untrainable_reason(layer, x), f.conv_bf16_trainable(layer, x)]
    dy = x
    if isinstance(layer, nn.Conv2d) and x.dim() == 4 and x.device.type != "meta":
        dy = type(x)(torch.zeros((x.shape[0], layer.out_channels, 5, 5), dtype=x.dtype).contiguous(memory_format=CL)) \
            if isinstance(x, OnGpu) else torch.zeros((x.shape[0], layer.out_channels, 5, 5), dtype=x.dtype)
        if x.requires_grad:
            dy.requires_grad_()
    out += [f.dgrad_direct_supported(layer, dy), f.dgrad_direct_supported(layer, x)]
    with stubbed(Stub(keep=False)):
        out += [f.conv_input_bn(layer, x) if f.conv_fusable(layer, x) else None, f.conv32_input_bn(layer, x)]
    return out


def _bn_layers():
    tracking = lambda C: nn.BatchNorm2d(C)                                          # noqa: E731
    return {
        "batch": lambda C: bnorm(C), "batch_eval": lambda C: bnorm(C).eval(), "running": lambda C: bnorm(C, "running"),
        "tracking_train": tracking, "no_affine": lambda C: bnorm(C, affine=False), "wrong_C": lambda C: bnorm(2 * C),
        "bf16_params": lambda C: bnorm(C).to(BF), "identity": lambda C: nn.Identity(),
    }


BN_X = {
    "c8": lambda dt: OnGpu(torch.zeros((2, 8, 6, 6), dtype=dt).contiguous(memory_format=CL)),
    "c64": lambda dt: OnGpu(torch.zeros((2, 64, 6, 6), dtype=dt).contiguous(memory_format=CL)),
    "c12": lambda dt: OnGpu(torch.zeros((2, 12, 6, 6), dtype=dt).contiguous(memory_format=CL)),
    "c2056": lambda dt: OnGpu(torch.zeros((2, 2056, 1, 1), dtype=dt).contiguous(memory_format=CL)),
    "one_row": lambda dt: OnGpu(torch.zeros((1, 8, 1, 1), dtype=dt).contiguous(memory_format=CL)),
    "nchw": lambda dt: OnGpu(torch.zeros((2, 8, 6, 6), dtype=dt)),
    "3d": lambda dt: OnGpu(torch.zeros((8, 6, 6), dtype=dt)),
    "empty": lambda dt: OnGpu(torch.zeros((0, 8, 6, 6), dtype=dt).contiguous(memory_format=CL)),
    "cpu": lambda dt: torch.zeros((2, 8, 6, 6), dtype=dt).contiguous(memory_format=CL),
    "tiny_hw": lambda dt: OnGpu(torch.zeros((2, 8, 1, 1), dtype=dt).contiguous(memory_format=CL)),
}
BN_RESIDUALS = {
    "none": lambda x: None, "same": lambda x: torch.zeros_like(x), "other_dtype": lambda x: torch.zeros_like(x).double(),
    "other_shape": lambda x: torch.zeros_like(x)[..., :-1] if x.dim() == 4 else torch.zeros_like(x),
    "nchw": lambda x: OnGpu(torch.zeros(x.shape, dtype=x.dtype)),
}
POOLS = {"3/2/1": lambda: nn.MaxPool2d(3, 2, 1), "2": lambda: nn.MaxPool2d(2), "5/2/2": lambda: nn.MaxPool2d(5, 2, 2),
         "ceil": lambda: nn.MaxPool2d(3, 2, 1, ceil_mode=True), "dilated": lambda: nn.MaxPool2d(3, 2, 1, dilation=2),
         "oblong": lambda: nn.MaxPool2d((3, 2), 2, 1), "2/3/0": lambda: nn.MaxPool2d(2, 3, 0),
         "3/1/0": lambda: nn.MaxPool2d(3, 1, 0),
         "avg": lambda: nn.AvgPool2d(3, 2, 1), "none": lambda: None}
BN_PREDICATES = ("fusable", "bn_untrainable_reason", "bn_trainable", "bn_bf16_untrainable_reason", "bn_bf16_trainable")
BN_POOL_PREDICATES = ("bn_pool_untrainable_reason", "bn_pool_trainable", "bn_pool_bf16_untrainable_reason",
                      "bn_pool_bf16_trainable", "_pool_params")
DTYPES = {"f32": F32, "bf16": BF}


def record_predicates():
    """{"reasons": [...], "conv": {...}, "bn": {...}, "bn_pool": {...}, "stem": {...}}: every verdict
    as true / false / null or, for a reason, its index in "reasons". Keys are "mode|case..."."""
    reasons = []

    def enc(v):
        if isinstance(v, str):
            if v not in reasons:
                reasons.append(v)
            return reasons.index(v)
        return None if v is None else list(v) if isinstance(v, tuple) else bool(v)
    f = features
    got = {"conv": {}, "bn": {}, "bn_pool": {}, "stem": {}}
    for mode, ctx in MODES.items():
        grad = mode == "requires_grad"
        with ctx():
            for i, (make, shape) in enumerate(CONV_LAYERS):
                for dn, dt in DTYPES.items():
                    x = OnGpu(torch.zeros(shape, dtype=dt).contiguous(memory_format=CL))
                    layer = make()
                    if grad:
                        x.requires_grad_()
                    else:
                        layer.requires_grad_(False)
                    got["conv"][f"{mode}|{i}|{dn}"] = [enc(v) for v in _conv_verdicts(layer, x)]
                    if grad:                                      # ... and the weight alone
                        got["conv"][f"weight_grad|{i}|{dn}"] = [enc(v) for v in _conv_verdicts(layer, x.detach())]
            for i in (0, 17):
                make, shape = CONV_LAYERS[i]
                for dn, dt in DTYPES.items():
                    for xn, mk in ODD_X.items():
                        if mode == "default" or xn in ("nchw", "cpu"):
                            layer = make().requires_grad_(False)
                            got["conv"][f"{mode}|{i}|{dn}|{xn}"] = [enc(v) for v in _conv_verdicts(layer, mk(shape, dt))]
            for dn, dt in DTYPES.items():
                for xn, mk in BN_X.items():
                    for bn_name, mkbn in _bn_layers().items():
                        for rn, mkres in BN_RESIDUALS.items():
                            if rn != "none" and (bn_name != "batch" or xn not in ("c8", "cpu")):
                                continue
                            x = mk(dt)
                            bn = mkbn(x.shape[1] if x.dim() == 4 else 8)
                            if grad:
                                x.requires_grad_()
                            else:
                                bn.requires_grad_(False)
                            res = mkres(x.detach())
                            v = [f.fusable(x, bn, res) if isinstance(bn, nn.BatchNorm2d) else None,
                                 f.bn_untrainable_reason(x, bn, res), f.bn_trainable(x, bn, res),
                                 f.bn_bf16_untrainable_reason(x, bn, res), f.bn_bf16_trainable(x, bn, res)]
                            got["bn"][f"{mode}|{dn}|{xn}|{bn_name}|{rn}"] = [enc(u) for u in v]
                for xn in ("c8", "tiny_hw", "3d", "cpu", "c12"):
                    for bn_name in ("batch", "tracking_train", "identity"):
                        for pn, mkpool in POOLS.items():
                            if bn_name != "batch" and pn != "3/2/1":
                                continue
                            x = BN_X[xn](dt)
                            bn = _bn_layers()[bn_name](x.shape[1] if x.dim() == 4 else 8).requires_grad_(False)
                            pool = mkpool()
                            v = [f.bn_pool_untrainable_reason(x, bn, pool), f.bn_pool_trainable(x, bn, pool),
                                 f.bn_pool_bf16_untrainable_reason(x, bn, pool), f.bn_pool_bf16_trainable(x, bn, pool),
                                 f._pool_params(pool)]
                            got["bn_pool"][f"{mode}|{dn}|{xn}|{bn_name}|{pn}"] = [enc(u) for u in v]
            for i, (make, shape) in enumerate(CONV_LAYERS[:17]):
                for dn, dt in DTYPES.items():
                    for wn, wdt in DTYPES.items():
                        for bn_name in ("batch", "tracking_train", "running", "wrong_C", "identity"):
                            for pn in ("3/2/1", "none", "ceil"):
                                if (bn_name != "batch" or pn != "3/2/1" or wn != "f32") and i != 0:
                                    continue
                                layer, bn = make(), _bn_layers()[bn_name](64)
                                if wn == "bf16" and not any(p.dtype == torch.float64 for p in layer.parameters()):
                                    layer = layer.to(wdt)
                                x = OnGpu(torch.zeros(shape, dtype=dt))
                                if grad:
                                    x.requires_grad_()
                                else:
                                    layer.requires_grad_(False), bn.requires_grad_(False)
                                got["stem"][f"{mode}|{i}|{dn}|{wn}|{bn_name}|{pn}"] = \
                                    enc(f.stem_fusable(layer, bn, POOLS[pn](), x))
            for xn, x in (("odd_w", OnGpu(torch.zeros((2, 3, 16, 15), dtype=BF))),
                          ("wide", OnGpu(torch.zeros((1, 3, 8, 252), dtype=BF))),
                          ("empty", OnGpu(torch.zeros((0, 3, 16, 16), dtype=BF))),
                          ("cpu", torch.zeros((2, 3, 16, 16), dtype=BF))):
                got["stem"][f"{mode}|{xn}"] = enc(f.stem_fusable(_stem_layer().requires_grad_(False),
                                                                 bnorm(64).requires_grad_(False), None, x))
    for table in got.values():          # a row of another mode is kept only where it differs from "default"
        for key in [k for k in table if not k.startswith("default|")]:
            if table.get("default|" + key.split("|", 1)[1], table) == table[key]:
                del table[key]
    got["reasons"] = reasons
    return got


OPS = ("mcdo_forward", "mcdo_forward_stats", "mcdo_backward", "conv2d_f32", "conv2d_f32_backward",
       "bn_act_f32", "bn_act_f32_backward", "bn_pool_f32", "bn_pool_f32_backward",
       "stem_conv_f32", "stem_conv_f32_backward", "conv2d_bf16", "conv2d_bf16_backward",
       "bn_act_bf16", "bn_act_bf16_backward", "bn_pool_bf16", "bn_pool_bf16_backward")


def record_schemas():
    return {name: str(getattr(torch.ops.mcgmil, name).default._schema) for name in OPS}


def record():
    return {"wrappers": record_wrappers(), "predicates": record_predicates(), "schemas": record_schemas()}


def dumps(doc) -> str:
    """One line per wrapper case, predicate table and schema: small, and a diff names the case."""
    one = lambda v: json.dumps(v, separators=(",", ":"))       # noqa: E731
    lines = ["{", f' "generated_from": {one(doc["generated_from"])},', ' "wrappers": {']
    lines += [",\n".join(f"  {one(k)}: {one(v)}" for k, v in doc["wrappers"].items()), " },", ' "predicates": {']
    pred = doc["predicates"]
    lines.append(",\n".join(f"  {one(k)}: {one(pred[k])}" for k in pred))
    lines += [" },", ' "schemas": {', ",\n".join(f"  {one(k)}: {one(v)}" for k, v in doc["schemas"].items()), " }", "}"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    def git(*a):
        return subprocess.run(("git", "-C", REPO) + a, check=True, capture_output=True, text=True).stdout.strip()
    dirty = git("status", "--porcelain", "--", "montecarlo-gated-mil_amd/mcgmil")
    if dirty:
        sys.exit("the package differs from HEAD: the fixture records a commit\n" + dirty)
    doc = {"generated_from": {"commit": git("rev-parse", "HEAD"), "subject": git("log", "-1", "--format=%s")}}
    doc.update(record())
    with open(FIXTURE, "w") as fh:
        fh.write(dumps(doc))
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes from {doc['generated_from']['commit']}")
