"""The channels-last backbone's layers on the GPU (include/mcgmil_features.h): fused BatchNorm +
residual add + ReLU (mcgmil_batchnorm_act) and the implicit-GEMM convolution (mcgmil_conv2d).

The reference runs its ResNet's BatchNorm2d layers on the statistics of the bag itself
(infer.py:105-109 deactivate_batchnorm: running stats None, so torch.nn.functional.batch_norm
normalises with the batch mean and biased variance in eval mode too). `batchnorm_act` computes
exactly that layer -- plus the residual add and ReLU that follow it in BasicBlock / Bottleneck --
in three HBM-bound HIP kernels instead of MIOpen's training-mode BN and PyTorch's separate add and
clamp kernels. Layers that keep running statistics (no deactivate_batchnorm, eval mode) are
normalised with them.

`fusable` tells the backbone when the fused path applies: a CUDA(HIP) channels-last bf16/fp32
activation with C % 8 == 0 and C <= 2048, no autograd, and no running-statistics update pending
(a BN in training mode that tracks running stats keeps the torch path, which updates them).
MCGMIL_FUSED_BN=0 switches the backbone back to the torch layers (A/B timing and parity tests).

`conv2d` runs a 3x3 / 1x1 torch.nn.Conv2d of the blocks (bias-free, groups 1, dilation 1, zero
padding, 64k input and output channels) on a channels-last bf16 activation as one MFMA
implicit-GEMM kernel -- the arithmetic of torch.autocast's bf16 convolution (bf16 operands, fp32
accumulation, one rounding) without MIOpen's per-convolution output fill. `conv_fusable` says when
it applies. MCGMIL_NATIVE_CONV=0 switches it off.

`stem` runs the torchvision stem maxpool(relu(bn1(conv1(x)))) (7x7/2 convolution of the 3-channel
instances) as one library call (mcgmil_stem_forward): an MFMA implicit GEMM straight from the NCHW
bf16 instances the patcher writes, with the BatchNorm statistics accumulated in its epilogue, then
the fused normalise + ReLU + max-pool pass. `stem_fusable` says when it applies (else the torch
layers run); MCGMIL_NATIVE_STEM=0 switches it off.

Training (opt-in, MultiHeadGatedAttentionMIL.enable_backbone_training): inside
`native_conv_training()` `run_conv` sends a `conv32_trainable` convolution that autograd tracks to
torch.ops.mcgmil.conv2d_f32 (mcgmil.library). `conv2d_f32_wgrad` is the HIP weight gradient
(include/mcgmil_conv_grad.h), `conv2d_f32_dgrad` the data gradient (the forward kernel on the
flipped weight for stride 1), `conv2d_f32_dgrad_direct` the direct data-gradient kernel for stride 1
and 2 (include/mcgmil_conv_dgrad.h), `conv2d_f32_backward` the op's backward on the route
`conv_grad_route()` names (MCGMIL_CONV_GRAD=native or direct; default aten.convolution_backward).
Inside `native_norm_training()` (enable_backbone_training(norm=True)) `bn_act` sends a pool-free
`bn_trainable` BatchNorm (+ residual add) (+ ReLU) that autograd tracks to
torch.ops.mcgmil.bn_act_f32: `batchnorm_act_stats` is its forward (mcgmil_batchnorm_act, which also
returns the batch mean and 1 / sqrt(var + eps)), `batchnorm_act_backward` its HIP backward
(include/mcgmil_bn_grad.h).
Inside `native_stem_training()` (enable_backbone_training(stem=True)) `bn_act` sends the stem's
`bn_pool_trainable` BatchNorm + ReLU + max-pool that autograd tracks to
torch.ops.mcgmil.bn_pool_f32: `batchnorm_pool_stats` is its forward (mcgmil_batchnorm_pool_train:
batchnorm_act's pooled output bit for bit, plus one byte per pooled element that names the
window's winning tap), `batchnorm_pool_backward` its HIP backward (include/mcgmil_pool_grad.h).
Inside `native_stem_conv_training()` (enable_backbone_training(stem_conv=True)) `run_conv` sends a
`stem_conv_trainable` convolution (1..4 input channels: the 7x7 stem) that autograd tracks to
torch.ops.mcgmil.stem_conv_f32: `conv2d_f32` in its gather mode is the forward,
`conv2d_f32_stem_wgrad` the HIP weight gradient (include/mcgmil_stem_grad.h).
Mixed precision (opt-in, MultiHeadGatedAttentionMIL.enable_bf16_backbone_training): inside
`native_conv_bf16_training()` `run_conv` sends a `conv_bf16_trainable` convolution that autograd
tracks (a bf16 activation, as the blocks see it under torch.autocast) to
torch.ops.mcgmil.conv2d_bf16: `conv2d_bf16` is the forward (the bf16 MFMA kernel of `conv2d`),
`conv2d_bf16_wgrad` the bf16 HIP weight gradient with fp32 output
(include/mcgmil_conv_grad_bf16.h), `conv2d_bf16_dgrad` the data gradient (the forward kernel on the
flipped weight for stride 1, else aten), `conv2d_bf16_dgrad_direct` the direct bf16 data-gradient
kernel for stride 1 and 2 (include/mcgmil_conv_dgrad_bf16.h), `conv2d_bf16_backward` the op's
backward on the route MCGMIL_CONV_GRAD names (native: the HIP kernels, aten for the stride-2 data
gradient; direct: the direct kernel in aten's place; default aten.convolution_backward).
Inside `native_norm_bf16_training()` (enable_bf16_norm_training()) `bn_act` sends a
pool-free `bn_bf16_trainable` BatchNorm (+ residual add) (+ ReLU) that autograd tracks to
torch.ops.mcgmil.bn_act_bf16: `batchnorm_act_stats_bf16` is its forward (mcgmil_batchnorm_act in
bf16), `batchnorm_act_backward_bf16` its HIP backward (include/mcgmil_bn_grad_bf16.h).
Inside `native_stem_bf16_training()` (enable_bf16_stem_training()) `bn_act` sends the stem's
`bn_pool_bf16_trainable` BatchNorm + ReLU + max-pool that autograd tracks (a bf16 activation) to
torch.ops.mcgmil.bn_pool_bf16: `batchnorm_pool_stats_bf16` is its forward
(mcgmil_batchnorm_pool_train_bf16: batchnorm_act's pooled bf16 output bit for bit, plus the argmax
codes taken on the unrounded fp32 value), `batchnorm_pool_backward_bf16` its HIP backward
(include/mcgmil_pool_grad_bf16.h).
Inside `native_stem_conv_bf16_training()` (enable_bf16_stem_conv_training()) `run_stem` sends a
`stem_conv_bf16_trainable` convolution that autograd tracks (the 7x7 stem under bf16 autocast) to
torch.ops.mcgmil.stem_conv_bf16: `stem_conv_bf16` is its forward (mcgmil_stem_conv_bf16: the
inference stem's MFMA kernel straight from the NCHW instances, without the BatchNorm),
`stem_conv_bf16_wgrad` the bf16 HIP weight gradient with fp32 output
(include/mcgmil_stem_grad_bf16.h).

Precision of the fp32 convolutions: `conv2d_f32(..., precision=)` / `float32_conv_precision()` /
MCGMIL_CONV32_PRECISION send a `conv32x3_fusable` convolution (in_channels a multiple of 32: every
block convolution) to mcgmil_conv2d_f32x3, the split-bf16 kernel with fp32 storage (three bf16 MFMA
products per K, "bf16x3"); the stem, other layers and every differentiable op but conv2d_f32x3 stay exact fp32.
Training at that precision (opt-in, MultiHeadGatedAttentionMIL.enable_bf16x3_backbone_training):
inside `native_conv_training()` and `native_conv_x3_training()` `run_conv` sends a
`conv32x3_trainable` convolution that autograd tracks (conv32_trainable with in_channels a multiple
of 32: every block convolution, not the stem) to torch.ops.mcgmil.conv2d_f32x3: `conv2d_f32x3` is
the forward (mcgmil_conv2d_f32x3), `conv2d_f32x3_wgrad` the bf16x3 HIP weight gradient
(include/mcgmil_conv_grad_x3.h), `conv2d_f32x3_dgrad` the data gradient (the bf16x3 forward kernel
on the flipped weight for stride 1, else the exact fp32 direct kernel), `conv2d_f32x3_backward` the
op's backward, which does not read MCGMIL_CONV_GRAD: no gradient leaves the project's kernels.

How the bindings are laid out: every operation is bound once, with the dtype as a parameter, and
the public fp32 / bf16 names are thin wrappers over it. `_ptr`, `_stream` and `_workspace` do the
marshalling; `_conv_args` fills mcgmil_conv_args (also as the `fwd` of the gradient structs) and
`_bn_args` mcgmil_bn_args; `_conv_refusal` is the one walk over the clauses of the native
convolutions' domains (the six conv predicates differ in its keywords alone), `_bn_refusal` and
`_bn_pool_refusal` the same for the BatchNorm training ops; `_wgrad`, `_bn_stats`,
`_bn_act_backward` and `_bn_pool_backward` are the shared bodies, `_TWIN` what differs between an
fp32 op and its bf16 twin. tests/test_features_bindings_host.py pins what reaches the C ABI.
"""
import contextlib
import ctypes
import os
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib

_DT = {torch.float32: _lib.MCGMIL_F32, torch.bfloat16: _lib.MCGMIL_BF16}
_CL = torch.channels_last


# ---------------------------------------------------------------- marshalling
def _ptr(t: Optional[torch.Tensor]) -> Optional[ctypes.c_void_p]:
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(dev) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _workspace(size_fn, what: str, args, dev, optional: bool = False) -> None:
    """Ask size_fn (the entry point named `what`) for the bytes `args` needs and point
    args.workspace at that many from the caching allocator. The tensor lives as long as `args`:
    until after the launches, and its memory is freed stream-ordered. optional: a size of 0 leaves
    args.workspace NULL."""
    n = ctypes.c_size_t()
    _lib.check(size_fn(ctypes.byref(args), ctypes.byref(n)), what)
    if n.value or not optional:
        args._workspace_tensor = ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
        args.workspace, args.workspace_bytes = ctypes.c_void_p(ws.data_ptr()), n.value


def _square(v):
    return v if isinstance(v, int) else (v[0] if len(set(v)) == 1 else None)


def _out_hw(H: int, W: int, kh: int, kw: int, stride: int, pad: int):
    """The output extent of a convolution or pooling window."""
    return (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1


def _use_batch(bn: nn.BatchNorm2d) -> bool:
    return bn.training or bn.running_mean is None or bn.running_var is None


# what differs between an fp32 training op and its bf16 twin: the suffix of the wrapper's and the
# entry points' names, the word for the dtype, the args structs of the two backwards
class _Twin(NamedTuple):
    suffix: str
    word: str
    bn_grad_args: type
    bn_pool_grad_args: type


_TWIN = {torch.float32: _Twin("", "fp32", _lib.BnGradArgs, _lib.BnPoolGradArgs),
         torch.bfloat16: _Twin("_bf16", "bf16", _lib.BnGradBf16Args, _lib.BnPoolGradBf16Args)}


def enabled() -> bool:
    return os.environ.get("MCGMIL_FUSED_BN", "1") != "0"


def fusable(x: torch.Tensor, bn: nn.BatchNorm2d, residual: Optional[torch.Tensor] = None) -> bool:
    if not (enabled() and x.is_cuda and x.dim() == 4 and x.dtype in _DT):
        return False
    C = x.shape[1]
    if C % 8 or C > 2048 or C != bn.num_features or x.numel() == 0:
        return False
    if not x.is_contiguous(memory_format=torch.channels_last):
        return False
    if residual is not None and (residual.shape != x.shape or residual.dtype != x.dtype or
                                 not residual.is_contiguous(memory_format=torch.channels_last)):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in bn.parameters())):
        return False
    if bn.training and bn.track_running_stats and bn.running_mean is not None:
        return False                       # torch would update the running statistics
    return True


def conv_enabled() -> bool:
    return os.environ.get("MCGMIL_NATIVE_CONV", "1") != "0"


def conv32_enabled() -> bool:
    """MCGMIL_NATIVE_CONV32=0 keeps fp32 convolutions on the torch layers (MIOpen)."""
    return os.environ.get("MCGMIL_NATIVE_CONV32", "1") != "0" and conv_enabled()


# ---------------------------------------------------------------- the native convolutions' domains
def _conv_refusal(conv: nn.Module, t: torch.Tensor, *, fp32: bool, weights: Optional[tuple], autocast: str,
                  in_channels: str, strides: Optional[tuple] = (1, 2), pad_below_kernel: bool = True,
                  out_max: Optional[int] = None, of_dy: bool = False, nonempty: bool = True,
                  channels_last: bool = True, pixels: Optional[str] = "positive", below_2gib: bool = False,
                  max_hw: Optional[int] = None, autograd: bool = False, device_last: bool = False) -> Optional[str]:
    """Why `conv` on the activation `t` is outside a native convolution's domain: the first clause
    that fails, or None. Every predicate below is this walk with its own keywords:
      fp32          an fp32 activation behind MCGMIL_NATIVE_CONV32, else a bf16 one behind MCGMIL_NATIVE_CONV
      weights       the weight dtypes taken (None: any)
      autocast      "refuse" it, "ignore" it (never asked), or "bf16": autocast to bf16 stands in for a bf16 weight
      in_channels   "64" / "16": a multiple of it, "1..4", or "16 or gather": % 16 or kh * kw * in <= 1024
      strides       the square strides taken (None: any)
      out_max       the largest out_channels (None: no limit); always a multiple of 64
      of_dy         t is dY, [batch, out_channels, OH, OW], not x
      pixels        "positive": 1 <= OH, OW and batch * OH * OW < 2^31 - 256; "any": the product alone; None
      below_2gib, max_hw   the bf16 kernels' limits on t: numel * 2 < 2^31, height and width <= max_hw
      autograd      refuse what autograd tracks (the inference predicates)
      device_last   ask for a CUDA activation after every other clause, not with the rank"""
    if not (conv32_enabled() if fp32 else conv_enabled()):
        return "the native fp32 convolutions are switched off (MCGMIL_NATIVE_CONV32 / MCGMIL_NATIVE_CONV)" if fp32 \
            else "the native convolutions are switched off (MCGMIL_NATIVE_CONV)"
    if not isinstance(conv, nn.Conv2d):
        return "not an nn.Conv2d"
    if not ((t.is_cuda or device_last) and t.dim() == 4):
        return "the activation is not a 4-d CUDA tensor"
    if fp32:
        if t.dtype != torch.float32 or (weights is not None and conv.weight.dtype not in weights):
            return "the activation and the weight must be fp32"
    else:
        if t.dtype != torch.bfloat16:
            return "the activation must be bf16"
        if conv.weight.dtype not in weights and not (
                autocast == "bf16" and torch.is_autocast_enabled("cuda") and
                torch.get_autocast_dtype("cuda") == torch.bfloat16):
            return "the weight must be fp32 or bf16"
    if autocast == "refuse" and torch.is_autocast_enabled("cuda"):
        return "autocast is enabled"
    if conv.groups != 1 or conv.bias is not None or conv.padding_mode != "zeros":
        return "only a bias-free groups=1 zero-padded convolution"
    stride = _square(conv.stride)
    if _square(conv.dilation) != 1 or (stride is None if strides is None else stride not in strides) or \
            not isinstance(conv.padding, tuple) or _square(conv.padding) is None:
        return "dilation 1, a square stride of 1 or 2 and a square integer padding"
    kh, kw = conv.kernel_size
    pad = conv.padding[0]
    if not (1 <= kh <= 7 and 1 <= kw <= 7) or (pad_below_kernel and pad >= min(kh, kw)):
        return "kernel 1..7 per axis and pad < min(kh, kw)"
    cin = conv.in_channels
    if in_channels == "1..4":
        if not 1 <= cin <= 4:
            return "in_channels must be in 1..4"
    elif in_channels == "16 or gather":
        if cin % 16 and kh * kw * cin > 1024:
            return "in_channels must be a multiple of 16, or kh * kw * in_channels at most 1024"
    elif cin % int(in_channels):
        return f"in_channels must be a multiple of {in_channels}"
    if conv.out_channels % 64 or (out_max is not None and conv.out_channels > out_max):
        return "out_channels must be a multiple of 64" + ("" if out_max is None else f" (at most {out_max})")
    if t.shape[1] != (conv.out_channels if of_dy else cin):
        return "the activation's channels are not the convolution's in_channels"
    if (nonempty and t.numel() == 0) or (channels_last and not t.is_contiguous(memory_format=_CL)):
        return "the activation must be non-empty and channels-last"
    if pixels is not None:
        oh, ow = _out_hw(t.shape[2], t.shape[3], kh, kw, stride, pad)
        if (pixels == "positive" and (oh < 1 or ow < 1)) or t.shape[0] * oh * ow >= 2 ** 31 - 256:
            return "batch * OH * OW must be in 1 .. 2^31 - 257"
    if (below_2gib and t.numel() * 2 >= 2 ** 31) or (max_hw is not None and max(t.shape[2], t.shape[3]) > max_hw):
        return "the activation must be smaller than 2 GiB, height and width at most 16383"
    if autograd and torch.is_grad_enabled() and (t.requires_grad or conv.weight.requires_grad):
        return "autograd tracks the activation or the weight"
    if not t.is_cuda:
        return "the activation is not a CUDA tensor"
    return None


_CONV_FUSABLE = dict(fp32=False, weights=(torch.bfloat16,), autocast="bf16", in_channels="64", strides=None,
                     pad_below_kernel=False, nonempty=False, pixels=None, below_2gib=True, autograd=True)
_CONV32_FUSABLE = dict(fp32=True, weights=None, autocast="refuse", in_channels="16 or gather", strides=None,
                       pad_below_kernel=False, nonempty=False, pixels="any", autograd=True)
_CONV32X3_FUSABLE = dict(_CONV32_FUSABLE, in_channels="32", device_last=True)
_CONV32_TRAINABLE = dict(fp32=True, weights=(torch.float32,), autocast="refuse", in_channels="16")
_CONV32X3_TRAINABLE = dict(_CONV32_TRAINABLE, in_channels="32")
_STEM_CONV_TRAINABLE = dict(fp32=True, weights=(torch.float32,), autocast="refuse", in_channels="1..4", out_max=4096)
_CONV_BF16_TRAINABLE = dict(fp32=False, weights=(torch.float32, torch.bfloat16), autocast="ignore", in_channels="64",
                            below_2gib=True, max_hw=16383)
_DGRAD_DIRECT = dict(fp32=True, weights=(torch.float32,), autocast="refuse", in_channels="16", of_dy=True,
                     channels_last=False, pixels=None)
_DGRAD_BF16_DIRECT = dict(fp32=False, weights=(torch.float32, torch.bfloat16), autocast="ignore", in_channels="64",
                          of_dy=True, channels_last=False, pixels=None, below_2gib=True)


def conv_fusable(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    """A CUDA channels-last activation that torch would convolve in bf16 (bf16 input, or autocast
    to bf16), with a convolution the kernel implements, and no autograd."""
    return _conv_refusal(conv, x, **_CONV_FUSABLE) is None


def _conv_args(conv: nn.Conv2d, x) -> "_lib.ConvArgs":
    """mcgmil_conv_args with the geometry of conv on x (a tensor, or the shape of one)."""
    a = _lib.ConvArgs()
    a.batch, _, a.height, a.width = x.shape if isinstance(x, torch.Tensor) else (int(v) for v in x)
    a.in_channels, a.out_channels = conv.in_channels, conv.out_channels
    a.kernel_h, a.kernel_w = conv.kernel_size
    a.stride, a.pad = _square(conv.stride), _square(conv.padding)
    return a


def _conv_out_shape(a: "_lib.ConvArgs") -> tuple:
    return (a.batch, a.out_channels) + _out_hw(a.height, a.width, a.kernel_h, a.kernel_w, a.stride, a.pad)


def _set_in_ab(a: "_lib.ConvArgs", in_ab: Optional[torch.Tensor], in_relu: bool, dev) -> None:
    if in_ab is not None:
        if in_ab.shape != (2, a.in_channels) or in_ab.dtype != torch.float32 or \
                in_ab.device != dev or not in_ab.is_contiguous():
            raise ValueError("in_ab must be a contiguous fp32 [2, in_channels] tensor on x's device")
        a.in_ab, a.in_relu = _ptr(in_ab), int(bool(in_relu))


def packed_conv_weight(conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """The weight as bf16 [out, kh, kw, in] (torch's autocast cast, then channels-last), cached on
    the module until the weight changes."""
    w = conv.weight.detach()
    key = (w.data_ptr(), w._version, w.dtype, x.device)
    cached = getattr(conv, "_mcgmil_packed", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    L = _lib.load()
    if w.device != x.device or w.dtype not in (torch.float32, torch.bfloat16):
        w = w.to(device=x.device, dtype=torch.float32)
    w = w.contiguous()
    packed = torch.empty(w.numel(), dtype=torch.bfloat16, device=x.device)
    _lib.check(L.mcgmil_pack_conv_weights(ctypes.byref(_conv_args(conv, x)), _ptr(w), _DT[w.dtype], _ptr(packed),
                                          _stream(x.device)), "mcgmil_pack_conv_weights")
    conv._mcgmil_packed = (key, packed)
    return packed


def fold_enabled() -> bool:
    """MCGMIL_FUSE_INPUT_BN=0 materialises every BatchNorm output (no DeferredBN)."""
    return os.environ.get("MCGMIL_FUSE_INPUT_BN", "1") != "0"


def conv_input_bn(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    """Whether conv2d(conv, x, in_ab=...) can apply an input BatchNorm inside the convolution
    (mcgmil_conv_input_bn: the 3x3 / stride 1 halo kernels); False with MCGMIL_FUSE_INPUT_BN=0."""
    if not fold_enabled():
        return False
    L = _lib.load()
    ok = ctypes.c_int32()
    _lib.check(L.mcgmil_conv_input_bn(ctypes.byref(_conv_args(conv, x)), ctypes.byref(ok)), "mcgmil_conv_input_bn")
    return bool(ok.value)


def split_enabled() -> bool:
    """MCGMIL_CONV_SPLIT=0: no K split of the last pixel tiles (mcgmil_conv_args.workspace NULL)."""
    return os.environ.get("MCGMIL_CONV_SPLIT", "1") != "0"


def conv2d(conv: nn.Conv2d, x: torch.Tensor, stats: bool = False,
           in_ab: Optional[torch.Tensor] = None, in_relu: bool = True, flags: int = 0):
    """conv(x) for a channels-last bf16 activation (see conv_fusable) on the MFMA kernel; returns a
    channels-last bf16 tensor, or with stats=True (y, partials): the BatchNorm statistics of y
    as [parts, 3, Cout] (count, mean, M2) blocks for batchnorm_act(..., partials=...), or None
    where the layer's kernel emits none (256 x 256 tiles). With in_ab ([2, Cin] fp32 from
    batchnorm_coefficients) the convolution reads relu?(bn(x)) instead of x (conv_input_bn).
    flags: mcgmil_conv_args.flags (the tile policy, MCGMIL_CONV_TILE_*; 0 = auto).
    Layers whose plan takes a K split of its last tiles get their workspace from the caching
    allocator (mcgmil_conv_workspace_size); MCGMIL_CONV_SPLIT=0 runs them on whole tiles."""
    if not conv_fusable(conv, x):
        raise ValueError("conv2d needs a CUDA channels-last bf16 activation, a bias-free groups=1 "
                         "convolution with 64k channels and no autograd (see conv_fusable)")
    return _conv2d(conv, x, stats, in_ab, in_relu, flags)


def _conv2d(conv: nn.Conv2d, x: torch.Tensor, stats: bool = False,
            in_ab: Optional[torch.Tensor] = None, in_relu: bool = True, flags: int = 0):
    """conv2d without its predicate: for callers that have checked the domain themselves (conv2d
    after conv_fusable, conv2d_bf16 after conv_bf16_trainable)."""
    L = _lib.load()
    dev = x.device
    a = _conv_args(conv, x)
    a.flags = int(flags)
    _set_in_ab(a, in_ab, in_relu, dev)
    y = torch.empty(_conv_out_shape(a), dtype=torch.bfloat16, device=dev, memory_format=_CL)
    w = packed_conv_weight(conv, x)
    a.x, a.w, a.y = _ptr(x), _ptr(w), _ptr(y)
    if split_enabled():
        _workspace(L.mcgmil_conv_workspace_size, "mcgmil_conv_workspace_size", a, dev, optional=True)
    part = None
    if stats:
        n = ctypes.c_int32()
        _lib.check(L.mcgmil_conv_stats_parts(ctypes.byref(a), ctypes.byref(n)), "mcgmil_conv_stats_parts")
        if n.value > 0:          # 0: this layer's kernel emits no statistics
            part = torch.empty((n.value, 3, a.out_channels), dtype=torch.float32, device=dev)
            a.stats = _ptr(part)
    _lib.check(L.mcgmil_conv2d(ctypes.byref(a), _stream(dev)), "mcgmil_conv2d")
    return (y, part) if stats else y


def conv32_fusable(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    """A CUDA channels-last fp32 activation (no autocast) and a convolution the fp32 kernel
    implements (mcgmil_conv2d_f32: out_channels % 64, kernel <= 7, and in_channels % 16 or
    kh * kw * in_channels <= 1024 -- the 3-channel stem), no autograd."""
    return _conv_refusal(conv, x, **_CONV32_FUSABLE) is None


def packed_conv_weight_f32(conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """The fp32 weight in mcgmil_conv2d_f32's packed layout, cached on the module until it changes."""
    w = conv.weight.detach()
    key = (w.data_ptr(), w._version, w.dtype, x.device, "f32")
    cached = getattr(conv, "_mcgmil_packed32", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    L = _lib.load()
    w32 = w.to(device=x.device, dtype=torch.float32).contiguous()
    a = _conv_args(conv, x)
    n = ctypes.c_size_t()
    _lib.check(L.mcgmil_conv_packed_size_f32(ctypes.byref(a), ctypes.byref(n)), "mcgmil_conv_packed_size_f32")
    packed = torch.empty(n.value, dtype=torch.float32, device=x.device)
    _lib.check(L.mcgmil_pack_conv_weights_f32(ctypes.byref(a), _ptr(w32), _ptr(packed), _stream(x.device)),
               "mcgmil_pack_conv_weights_f32")
    conv._mcgmil_packed32 = (key, packed)
    return packed


def conv32_input_bn(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    """Whether conv2d_f32(conv, x, in_ab=...) can apply an input BatchNorm (in_channels a multiple
    of 16, <= 2048: every fp32 kernel but the gather mode); False with MCGMIL_FUSE_INPUT_BN=0."""
    return fold_enabled() and conv32_fusable(conv, x) and conv.in_channels % 16 == 0 and \
        conv.in_channels <= 2048


# ---------------------------------------------------------------- fp32 convolutions on split bf16 (bf16x3)
_PRECISIONS = ("fp32", "bf16x3")
_conv32_precision: Optional[str] = None      # float32_conv_precision's setting (None: the environment's)


def conv32_precision() -> str:
    """The ambient precision of the fp32 convolutions: what float32_conv_precision set, else
    MCGMIL_CONV32_PRECISION (read on every call): "bf16x3", or "fp32" for anything else."""
    if _conv32_precision is not None:
        return _conv32_precision
    return "bf16x3" if os.environ.get("MCGMIL_CONV32_PRECISION", "fp32") == "bf16x3" else "fp32"


def _check_precision(precision: str) -> str:
    if precision not in _PRECISIONS:
        raise ValueError(f"precision must be one of {_PRECISIONS}, not {precision!r}")
    return precision


@contextlib.contextmanager
def float32_conv_precision(precision: str):
    """Inside this context conv2d_f32 (and with it run_conv, conv_bn_act and the stem fallback)
    runs every `conv32x3_fusable` convolution at `precision`: "fp32" (mcgmil_conv2d_f32, exact fp32
    MFMA) or "bf16x3" (mcgmil_conv2d_f32x3: fp32 storage, three bf16 MFMA products per K, about
    15x fp32's distance from the exact sum; include/mcgmil_features.h). Takes precedence over
    MCGMIL_CONV32_PRECISION; conv2d_f32's own keyword takes precedence over both. The counterpart
    of torch.set_float32_matmul_precision for the backbone's convolutions. Inference only: the
    differentiable ops stay exact fp32."""
    global _conv32_precision
    before, _conv32_precision = _conv32_precision, _check_precision(precision)
    try:
        yield
    finally:
        _conv32_precision = before


def conv32x3_unfusable_reason(conv: nn.Module, x: torch.Tensor) -> Optional[str]:
    """Why conv on x is outside the bf16x3 kernel's domain (mcgmil_conv2d_f32x3), or None when it is
    inside: conv32_fusable's clauses with in_channels a multiple of 32 -- so not the 3-channel stem
    (the gather mode) nor 16 or 48 input channels. The device is asked for last."""
    return _conv_refusal(conv, x, **_CONV32X3_FUSABLE)


def conv32x3_fusable(conv: nn.Module, x: torch.Tensor) -> bool:
    """conv32x3_unfusable_reason(conv, x) is None."""
    return conv32x3_unfusable_reason(conv, x) is None


def packed_conv_weight_f32x3(conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """The fp32 weight split into bf16 hi and lo terms in mcgmil_conv2d_f32x3's packed layout,
    cached on the module until it changes."""
    w = conv.weight.detach()
    key = (w.data_ptr(), w._version, w.dtype, x.device, "f32x3")
    cached = getattr(conv, "_mcgmil_packed32x3", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    L = _lib.load()
    w32 = w.to(device=x.device, dtype=torch.float32).contiguous()
    a = _conv_args(conv, x)
    n = ctypes.c_size_t()
    _lib.check(L.mcgmil_conv_packed_size_f32x3(ctypes.byref(a), ctypes.byref(n)), "mcgmil_conv_packed_size_f32x3")
    packed = torch.empty(2 * n.value, dtype=torch.bfloat16, device=x.device)
    _lib.check(L.mcgmil_pack_conv_weights_f32x3(ctypes.byref(a), _ptr(w32), _ptr(packed), _stream(x.device)),
               "mcgmil_pack_conv_weights_f32x3")
    conv._mcgmil_packed32x3 = (key, packed)
    return packed


def conv2d_f32(conv: nn.Conv2d, x: torch.Tensor, stats: bool = False,
               in_ab: Optional[torch.Tensor] = None, in_relu: bool = True, precision: Optional[str] = None):
    """conv(x) in fp32 on the MFMA kernel (fp32 operands and accumulation) for a channels-last fp32
    activation (see conv32_fusable); returns a channels-last fp32 tensor, or with stats=True
    (y, partials): the BatchNorm statistics of y as [pixel tiles, 3, Cout] (count, mean, M2)
    blocks for batchnorm_act(..., partials=...). With in_ab ([2, Cin] fp32 from
    batchnorm_coefficients) the convolution reads relu?(bn(x)) instead of x (conv32_input_bn).
    precision: "fp32" (that kernel), "bf16x3" (the split-bf16 kernel mcgmil_conv2d_f32x3, same
    interface; raises outside conv32x3_fusable) or None: the ambient setting conv32_precision(),
    under which bf16x3 takes the `conv32x3_fusable` convolutions and leaves the others exact."""
    if not conv32_fusable(conv, x):
        raise ValueError("conv2d_f32 needs a CUDA channels-last fp32 activation and a bias-free groups=1 "
                         "convolution with out_channels % 64 == 0 (conv32_fusable)")
    if precision is None:
        x3 = conv32_precision() == "bf16x3" and conv32x3_fusable(conv, x)
    else:
        x3 = _check_precision(precision) == "bf16x3"
        if x3 and not conv32x3_fusable(conv, x):
            raise ValueError(f"conv2d_f32(precision=\"bf16x3\"): {conv32x3_unfusable_reason(conv, x)} "
                             "(see conv32x3_fusable)")
    sfx = "_f32x3" if x3 else "_f32"
    L = _lib.load()
    dev = x.device
    a = _conv_args(conv, x)
    _set_in_ab(a, in_ab, in_relu, dev)
    y = torch.empty(_conv_out_shape(a), dtype=torch.float32, device=dev, memory_format=_CL)
    w = packed_conv_weight_f32x3(conv, x) if x3 else packed_conv_weight_f32(conv, x)
    a.x, a.w, a.y = _ptr(x), _ptr(w), _ptr(y)
    part = None
    if stats:
        n = ctypes.c_int32()
        _lib.check(getattr(L, "mcgmil_conv_stats_parts" + sfx)(ctypes.byref(a), ctypes.byref(n)),
                   "mcgmil_conv_stats_parts" + sfx)
        part = torch.empty((n.value, 3, a.out_channels), dtype=torch.float32, device=dev)
        a.stats = _ptr(part)
    _lib.check(getattr(L, "mcgmil_conv2d" + sfx)(ctypes.byref(a), _stream(dev)), "mcgmil_conv2d" + sfx)
    return (y, part) if stats else y


# ---------------------------------------------------------------- fp32 convolution backward
_native_training = False


@contextlib.contextmanager
def native_conv_training(flag: bool = True):
    """Inside this context `run_conv` sends every `conv32_trainable` convolution that autograd
    tracks to the differentiable op torch.ops.mcgmil.conv2d_f32 (forward and backward on the HIP
    kernels). Off outside it: the opt-in of MultiHeadGatedAttentionMIL.enable_backbone_training."""
    global _native_training
    before, _native_training = _native_training, bool(flag)
    try:
        yield
    finally:
        _native_training = before


def conv32_trainable(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    """A convolution whose forward AND weight gradient run on the fp32 HIP kernels
    (include/mcgmil_conv_grad.h): a CUDA channels-last fp32 activation without autocast, a
    bias-free groups=1 dilation-1 zero-padded convolution with kernel 1..7, stride 1 or 2,
    pad < kernel, in_channels % 16 == 0 and out_channels % 64 == 0. Says nothing about autograd:
    that is what the kernels are for."""
    return _conv_refusal(conv, x, **_CONV32_TRAINABLE) is None


class _ConvShim(nn.Conv2d):
    """The nn.Conv2d view of a bare (weight, stride, pad) triple, without nn.Conv2d's parameter
    initialisation: what the fp32 entry points below take. The weight is shared, not copied."""

    def __init__(self, weight: torch.Tensor, stride: int, pad: int):
        nn.Module.__init__(self)
        self.out_channels, self.in_channels = weight.shape[:2]
        self.kernel_size = tuple(weight.shape[2:])
        self.stride, self.padding, self.dilation = (stride, stride), (pad, pad), (1, 1)
        self.transposed, self.output_padding, self.groups = False, (0, 0), 1
        self.padding_mode = "zeros"
        self.weight = nn.Parameter(weight.detach(), requires_grad=False)
        self.register_parameter("bias", None)


def flipped_weight(weight: torch.Tensor) -> torch.Tensor:
    """W'[i, o, kh, kw] = W[o, i, KH-1-kh, KW-1-kw]: with it the data gradient of a stride-1
    convolution is the forward convolution dX = conv2d(dY, W', stride 1, pad k - 1 - p)."""
    return weight.flip(2, 3).transpose(0, 1).contiguous()


def _wgrad(args_type, dy_dtype: torch.dtype, size_name: str, launch_name: str,
           conv: nn.Conv2d, x: torch.Tensor, dy: torch.Tensor, chunk_pixels: int) -> torch.Tensor:
    """The three weight gradients after their predicates: dW [out, in, kh, kw] fp32 from x and dY."""
    L = _lib.load()
    dev = x.device
    g = args_type()
    g.fwd = _conv_args(conv, x)
    a = g.fwd
    if dy.shape != _conv_out_shape(a) or dy.dtype != dy_dtype or dy.device != dev:
        raise ValueError(f"dy must be {_TWIN[dy_dtype].word} {_conv_out_shape(a)} on x's device")
    dy = dy.contiguous(memory_format=_CL)
    dw = torch.empty((a.out_channels, a.in_channels, a.kernel_h, a.kernel_w), dtype=torch.float32, device=dev)
    a.x, g.dy, g.dw = _ptr(x), _ptr(dy), _ptr(dw)
    g.chunk_pixels = int(chunk_pixels)
    _workspace(getattr(L, size_name), size_name, g, dev)
    _lib.check(getattr(L, launch_name)(ctypes.byref(g), _stream(dev)), launch_name)
    return dw


def conv2d_f32_wgrad(conv: nn.Conv2d, x: torch.Tensor, dy: torch.Tensor, chunk_pixels: int = 0) -> torch.Tensor:
    """dW [out, in, kh, kw] fp32 of conv(x) given dY, on the HIP weight-gradient kernel
    (mcgmil_conv2d_wgrad_f32; see conv32_trainable). chunk_pixels caps the output pixels per
    launch chunk (0: the library's default); the result does not depend on it, bitwise."""
    if not conv32_trainable(conv, x):
        raise ValueError("conv2d_f32_wgrad needs a CUDA channels-last fp32 activation and a convolution "
                         "the weight-gradient kernel implements (see conv32_trainable)")
    return _wgrad(_lib.ConvGradArgs, torch.float32, "mcgmil_conv_wgrad_workspace_size_f32", "mcgmil_conv2d_wgrad_f32",
                  conv, x, dy, chunk_pixels)


def dgrad_native(conv: nn.Conv2d) -> bool:
    """Whether conv2d_f32_dgrad runs this convolution's data gradient on the forward HIP kernel:
    stride 1 and a square kernel (one pad k - 1 - p for both axes). Stride 2 takes
    aten.convolution_backward: there is no native strided data gradient yet."""
    return _square(conv.stride) == 1 and conv.kernel_size[0] == conv.kernel_size[1]


def conv2d_f32_dgrad(conv: nn.Conv2d, dy: torch.Tensor, x_shape, x: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dX (channels-last fp32, shape x_shape) of conv(x) given dY. Stride 1: mcgmil_conv2d_f32 of
    dY with the flipped, channel-swapped weight (flipped_weight), pad k - 1 - p; an in_channels
    that is no multiple of 64 is padded with zero filters to the next one and cut off again.
    Otherwise (dgrad_native False) aten.convolution_backward with output_mask (True, False,
    False); x, when given, is passed to it as the input (only its shape and layout matter) and
    the call is split along the batch below 2^31 bytes."""
    dy = dy.contiguous(memory_format=torch.channels_last)
    s, p = _square(conv.stride), _square(conv.padding)
    if dgrad_native(conv):
        w = flipped_weight(conv.weight.detach())                      # [in, out, kh, kw]
        cin = conv.in_channels
        if cin % 64:
            w = torch.cat([w, w.new_zeros((-cin % 64,) + tuple(w.shape[1:]))])
        with torch.no_grad():
            dx = conv2d_f32(_ConvShim(w, 1, conv.kernel_size[0] - 1 - p), dy, precision="fp32")
        if dx.shape[1] != cin:
            dx = dx[:, :cin].contiguous(memory_format=torch.channels_last)
        if tuple(dx.shape) != tuple(x_shape):
            raise ValueError(f"x_shape {tuple(x_shape)} does not belong to this convolution and dy {tuple(dx.shape)}")
        return dx
    if x is not None:
        return _aten_conv_backward(conv, x, dy, True, False)[0]
    like = dy.new_empty(1).expand(tuple(x_shape))
    dx = torch.ops.aten.convolution_backward(dy, like, conv.weight.detach(), None, [s, s], [p, p], [1, 1], False,
                                             [0, 0], 1, [True, False, False])[0]
    return dx.contiguous(memory_format=torch.channels_last)


def conv_grad_route() -> str:
    """Which backward torch.ops.mcgmil.conv2d_f32 takes, from MCGMIL_CONV_GRAD: "aten" (the
    default, also for an unset or unknown value): aten.convolution_backward (MIOpen) for both
    gradients; "native": the HIP weight gradient and, for stride 1, the forward kernel on the
    flipped weight as data gradient (stride 2: aten); "direct": the HIP weight gradient and the
    direct HIP data gradient (conv2d_f32_dgrad_direct, include/mcgmil_conv_dgrad.h) for stride 1
    and stride 2 alike -- no gradient of the convolution leaves the project's kernels. The forward
    stays on the HIP kernel on every route."""
    route = os.environ.get("MCGMIL_CONV_GRAD", "aten")
    return route if route in ("native", "direct") else "aten"


def conv_grad_native() -> bool:
    """Whether the weight gradient of torch.ops.mcgmil.conv2d_f32 comes from the HIP kernel:
    MCGMIL_CONV_GRAD=native (with, for stride 1, the forward kernel as data gradient) or =direct
    (with the direct data-gradient kernel; conv_grad_route). Default ("aten"):
    aten.convolution_backward (MIOpen) for both -- the measured-fastest for every ResNet-18 / -50
    shape class at 64 and 256 instances ("Backbone convolution backward"); the
    forward stays on the HIP kernel either way. Tensors of 2^31 bytes or more always take the
    native kernels where there is one (64-bit offsets)."""
    return conv_grad_route() in ("native", "direct")


def dgrad_direct_supported(conv: nn.Conv2d, dy: torch.Tensor) -> bool:
    """Whether conv2d_f32_dgrad_direct implements this convolution's data gradient for dy: a CUDA
    fp32 dy [batch, out_channels, OH, OW] without autocast, and a bias-free groups=1 dilation-1
    zero-padded convolution with kernel 1..7 per axis, stride 1 or 2, pad < kernel,
    in_channels % 16 == 0 and out_channels % 64 == 0 (include/mcgmil_conv_dgrad.h)."""
    return _conv_refusal(conv, dy, **_DGRAD_DIRECT) is None


def conv2d_f32_dgrad_direct(conv: nn.Conv2d, dy: torch.Tensor, x_shape) -> torch.Tensor:
    """dX (channels-last fp32, shape x_shape) of conv(x) given dY on the direct HIP data-gradient
    kernel mcgmil_conv2d_dgrad_f32, stride 1 and 2: the residue classes of the input pixels, each
    a stride-1 implicit GEMM over its own taps (include/mcgmil_conv_dgrad.h). The weight goes in
    as one weight.permute(2, 3, 0, 1).contiguous(); every element of dX is written exactly once,
    so two calls agree bitwise. Raises for anything dgrad_direct_supported refuses."""
    if not dgrad_direct_supported(conv, dy):
        raise ValueError("conv2d_f32_dgrad_direct needs a CUDA fp32 dy and a convolution the data-gradient "
                         "kernel implements (see dgrad_direct_supported)")
    L = _lib.load()
    g = _lib.ConvDgradArgs()
    g.fwd = _conv_args(conv, x_shape)
    if int(x_shape[1]) != conv.in_channels or tuple(dy.shape) != _conv_out_shape(g.fwd):
        raise ValueError(f"x_shape {tuple(x_shape)} does not belong to this convolution and dy {tuple(dy.shape)}")
    dy = dy.contiguous(memory_format=_CL)
    wt = conv.weight.detach().permute(2, 3, 0, 1).contiguous()           # [kh][kw][out][in]
    dev = dy.device
    dx = torch.empty(tuple(x_shape), dtype=torch.float32, device=dev, memory_format=_CL)
    g.dy, g.w_t, g.dx = _ptr(dy), _ptr(wt), _ptr(dx)
    _lib.check(L.mcgmil_conv2d_dgrad_f32(ctypes.byref(g), _stream(dev)), "mcgmil_conv2d_dgrad_f32")
    return dx


def _aten_conv_backward(conv: nn.Conv2d, x: torch.Tensor, dy: torch.Tensor, need_dx: bool, need_dw: bool):
    """(dx, dw) from aten.convolution_backward, split along the batch so that no call's x or dy
    reaches 2^31 bytes (see torch_conv); the pieces' dw are added in batch order."""
    s, p = _square(conv.stride), _square(conv.padding)
    w = conv.weight.detach()
    n = max(1, ((1 << 31) - 1) // (4 * max(x[0].numel(), dy[0].numel())))
    dxs, dw = [], None
    for i in range(0, x.shape[0], n):
        gx, gw, _ = torch.ops.aten.convolution_backward(dy[i:i + n], x[i:i + n], w, None, [s, s], [p, p], [1, 1],
                                                        False, [0, 0], 1, [need_dx, need_dw, False])
        if need_dx:
            dxs.append(gx)
        if need_dw:
            dw = gw if dw is None else dw + gw
    dx = None
    if need_dx:
        dx = (dxs[0] if len(dxs) == 1 else torch.cat(dxs)).contiguous(memory_format=torch.channels_last)
    return dx, dw.contiguous() if need_dw else None


def conv2d_f32_backward(conv: nn.Conv2d, x: torch.Tensor, dy: torch.Tensor, need_dx: bool = True,
                        need_dw: bool = True):
    """(dX or None, dW or None) of conv(x) given dY for a `conv32_trainable` convolution, on the
    route conv_grad_route() names: the backward of torch.ops.mcgmil.conv2d_f32."""
    if not conv32_trainable(conv, x):
        raise ValueError("conv2d_f32_backward needs a convolution and activation as conv32_trainable")
    dy = dy.contiguous(memory_format=torch.channels_last)
    if conv_grad_route() == "direct":       # both gradients on the HIP kernels, whatever the size
        dw = conv2d_f32_wgrad(conv, x, dy) if need_dw else None
        dx = conv2d_f32_dgrad_direct(conv, dy, x.shape) if need_dx else None
        return dx, dw
    big = 4 * max(x.numel(), dy.numel()) >= 2 ** 31
    if not (conv_grad_native() or big):
        return _aten_conv_backward(conv, x, dy, need_dx, need_dw)
    dw = conv2d_f32_wgrad(conv, x, dy) if need_dw else None
    dx = None
    if need_dx:
        dx = conv2d_f32_dgrad(conv, dy, x.shape, x) if dgrad_native(conv) else \
            _aten_conv_backward(conv, x, dy, True, False)[0]
    return dx, dw


def _conv_op(name: str, layer: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    from . import library  # noqa: F401  (registers torch.ops.mcgmil.*)
    return getattr(torch.ops.mcgmil, name)(x, layer.weight, _square(layer.stride), _square(layer.padding))


def conv2d_f32_op(layer: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """layer(x) through the differentiable op torch.ops.mcgmil.conv2d_f32 (mcgmil.library)."""
    return _conv_op("conv2d_f32", layer, x)


# ---------------------------------------------------------------- fp32 convolution backward on split bf16 (bf16x3)
_native_x3_training = False


@contextlib.contextmanager
def native_conv_x3_training(flag: bool = True):
    """Inside this context AND native_conv_training() `run_conv` sends every `conv32x3_trainable`
    convolution that autograd tracks to the differentiable op torch.ops.mcgmil.conv2d_f32x3 instead
    of torch.ops.mcgmil.conv2d_f32: fp32 storage, forward and both gradients on the project's
    kernels, the GEMMs of the forward, the weight gradient and the stride-1 data gradient at bf16x3.
    Off outside it: the opt-in of MultiHeadGatedAttentionMIL.enable_bf16x3_backbone_training."""
    global _native_x3_training
    before, _native_x3_training = _native_x3_training, bool(flag)
    try:
        yield
    finally:
        _native_x3_training = before


def conv32x3_untrainable_reason(conv: nn.Module, x: torch.Tensor) -> Optional[str]:
    """Why conv on x is not a convolution whose forward AND weight gradient run on the bf16x3 HIP
    kernels (mcgmil_conv2d_f32x3, include/mcgmil_conv_grad_x3.h), or None when it is:
    conv32_trainable's clauses with in_channels a multiple of 32 in place of 16 -- every block
    convolution of ResNet-18 / -34 / -50, not the 3-channel stem. Refuses under autocast, as
    conv32_trainable does. Says nothing about autograd."""
    return _conv_refusal(conv, x, **_CONV32X3_TRAINABLE)


def conv32x3_trainable(conv: nn.Module, x: torch.Tensor) -> bool:
    """conv32x3_untrainable_reason(conv, x) is None."""
    return conv32x3_untrainable_reason(conv, x) is None


def conv2d_f32x3(conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """conv(x) on the bf16x3 kernel: conv2d_f32(conv, x, precision="bf16x3"), whatever the ambient
    precision is. The forward of torch.ops.mcgmil.conv2d_f32x3."""
    return conv2d_f32(conv, x, precision="bf16x3")


def conv2d_f32x3_wgrad(conv: nn.Conv2d, x: torch.Tensor, dy: torch.Tensor, chunk_pixels: int = 0) -> torch.Tensor:
    """dW [out, in, kh, kw] fp32 of conv(x) given dY (both fp32), on the bf16x3 HIP weight-gradient
    kernel (mcgmil_conv2d_wgrad_f32x3; see conv32x3_trainable): operands split into bf16 hi and lo
    terms as they are staged, dy_hi x_hi + dy_hi x_lo + dy_lo x_hi into fp32. chunk_pixels caps the
    output pixels per launch chunk (0: the library's default); the result does not depend on it,
    bitwise."""
    reason = conv32x3_untrainable_reason(conv, x)
    if reason is not None:
        raise ValueError(f"conv2d_f32x3_wgrad: {reason} (see conv32x3_trainable)")
    return _wgrad(_lib.ConvGradArgs, torch.float32, "mcgmil_conv_wgrad_workspace_size_f32x3",
                  "mcgmil_conv2d_wgrad_f32x3", conv, x, dy, chunk_pixels)


def conv2d_f32x3_dgrad(conv: nn.Conv2d, dy: torch.Tensor, x_shape) -> torch.Tensor:
    """dX (channels-last fp32, shape x_shape) of conv(x) given dY. Stride 1 and a square kernel
    (dgrad_native): mcgmil_conv2d_f32x3 of dY with the flipped, channel-swapped weight
    (flipped_weight), pad k - 1 - p; an in_channels that is no multiple of 64 is padded with zero
    filters to the next one and cut off again, as conv2d_f32_dgrad does. Otherwise (stride 2, a
    non-square kernel) conv2d_f32_dgrad_direct, the exact fp32 kernel: there is no bf16x3 strided
    data gradient."""
    dy = dy.contiguous(memory_format=_CL)
    if not dgrad_native(conv):
        return conv2d_f32_dgrad_direct(conv, dy, x_shape)
    w = flipped_weight(conv.weight.detach())                      # [in, out, kh, kw]
    cin = conv.in_channels
    if cin % 64:
        w = torch.cat([w, w.new_zeros((-cin % 64,) + tuple(w.shape[1:]))])
    with torch.no_grad():
        dx = conv2d_f32x3(_ConvShim(w, 1, conv.kernel_size[0] - 1 - _square(conv.padding)), dy)
    if dx.shape[1] != cin:
        dx = dx[:, :cin].contiguous(memory_format=_CL)
    if tuple(dx.shape) != tuple(x_shape):
        raise ValueError(f"x_shape {tuple(x_shape)} does not belong to this convolution and dy {tuple(dx.shape)}")
    return dx


def conv2d_f32x3_backward(conv: nn.Conv2d, x: torch.Tensor, dy: torch.Tensor, need_dx: bool = True,
                          need_dw: bool = True):
    """(dX or None, dW or None) of conv(x) given dY for a `conv32x3_trainable` convolution: the
    backward of torch.ops.mcgmil.conv2d_f32x3, conv2d_f32x3_dgrad and conv2d_f32x3_wgrad. It does
    not read MCGMIL_CONV_GRAD: the opt-in is itself the choice of the project's kernels, so no
    gradient of the convolution leaves them and both repeat bitwise."""
    reason = conv32x3_untrainable_reason(conv, x)
    if reason is not None:
        raise ValueError(f"conv2d_f32x3_backward: {reason} (see conv32x3_trainable)")
    dy = dy.contiguous(memory_format=_CL)
    dw = conv2d_f32x3_wgrad(conv, x, dy) if need_dw else None
    dx = conv2d_f32x3_dgrad(conv, dy, x.shape) if need_dx else None
    return dx, dw


def conv2d_f32x3_op(layer: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """layer(x) through the differentiable op torch.ops.mcgmil.conv2d_f32x3 (mcgmil.library)."""
    return _conv_op("conv2d_f32x3", layer, x)


# ---------------------------------------------------------------- fp32 stem convolution backward
_native_stem_conv_training = False


@contextlib.contextmanager
def native_stem_conv_training(flag: bool = True):
    """Inside this context `run_conv` sends a `stem_conv_trainable` convolution that autograd
    tracks (the 7x7 stem, 3 input channels) to the differentiable op torch.ops.mcgmil.stem_conv_f32:
    the gather-mode forward kernel and the HIP weight gradient of include/mcgmil_stem_grad.h. Off
    outside it: the opt-in of MultiHeadGatedAttentionMIL.enable_backbone_training(stem_conv=True)."""
    global _native_stem_conv_training
    before, _native_stem_conv_training = _native_stem_conv_training, bool(flag)
    try:
        yield
    finally:
        _native_stem_conv_training = before


def stem_conv_untrainable_reason(conv: nn.Conv2d, x: torch.Tensor) -> Optional[str]:
    """Why conv on x is not a convolution whose forward AND weight gradient run on the fp32 HIP
    kernels for few input channels (include/mcgmil_stem_grad.h), or None when it is. The conditions
    are those of conv32_trainable with 1 <= in_channels <= 4 in place of in_channels % 16 == 0."""
    return _conv_refusal(conv, x, **_STEM_CONV_TRAINABLE)


def stem_conv_trainable(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    """stem_conv_untrainable_reason(conv, x) is None. Says nothing about autograd."""
    return stem_conv_untrainable_reason(conv, x) is None


def conv2d_f32_stem_wgrad(conv: nn.Conv2d, x: torch.Tensor, dy: torch.Tensor, chunk_pixels: int = 0) -> torch.Tensor:
    """dW [out, in, kh, kw] fp32 of conv(x) given dY for a `stem_conv_trainable` convolution, on the
    HIP kernel mcgmil_stem_wgrad_f32: the sibling of conv2d_f32_wgrad for 1..4 input channels.
    chunk_pixels as there; the result does not depend on it, bitwise."""
    reason = stem_conv_untrainable_reason(conv, x)
    if reason is not None:
        raise ValueError(f"conv2d_f32_stem_wgrad: {reason} (see stem_conv_trainable)")
    return _wgrad(_lib.ConvGradArgs, torch.float32, "mcgmil_stem_wgrad_workspace_size_f32", "mcgmil_stem_wgrad_f32",
                  conv, x, dy, chunk_pixels)


def stem_conv_f32_op(layer: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """layer(x) through the differentiable op torch.ops.mcgmil.stem_conv_f32 (mcgmil.library)."""
    return _conv_op("stem_conv_f32", layer, x)


# ---------------------------------------------------------------- bf16 convolution backward
_native_bf16_training = False


@contextlib.contextmanager
def native_conv_bf16_training(flag: bool = True):
    """Inside this context `run_conv` sends every `conv_bf16_trainable` convolution that autograd
    tracks (a bf16 activation: the blocks under torch.autocast("cuda", torch.bfloat16)) to the
    differentiable op torch.ops.mcgmil.conv2d_bf16: the bf16 MFMA forward kernel and, on the native
    route, the bf16 HIP weight gradient of include/mcgmil_conv_grad_bf16.h. Off outside it: the
    opt-in of MultiHeadGatedAttentionMIL.enable_bf16_backbone_training."""
    global _native_bf16_training
    before, _native_bf16_training = _native_bf16_training, bool(flag)
    try:
        yield
    finally:
        _native_bf16_training = before


def conv_bf16_untrainable_reason(conv: nn.Conv2d, x: torch.Tensor) -> Optional[str]:
    """Why conv on x is not a convolution whose forward AND weight gradient run on the bf16 HIP
    kernels (mcgmil_conv2d, include/mcgmil_conv_grad_bf16.h), or None when it is: a CUDA
    channels-last bf16 activation below 2 GiB, an fp32 (master) or bf16 weight, a bias-free groups=1
    dilation-1 zero-padded convolution with kernel 1..7, stride 1 or 2, pad < kernel and
    in_channels and out_channels multiples of 64. Says nothing about autograd or autocast."""
    return _conv_refusal(conv, x, **_CONV_BF16_TRAINABLE)


def conv_bf16_trainable(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    """conv_bf16_untrainable_reason(conv, x) is None. Says nothing about autograd."""
    return conv_bf16_untrainable_reason(conv, x) is None


def conv2d_bf16(conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """conv(x) on the bf16 MFMA kernel for a `conv_bf16_trainable` convolution: what conv2d gives,
    bit for bit, without conv2d's autocast and autograd clauses (the weight, fp32 master or bf16,
    goes through mcgmil_pack_conv_weights). The forward of torch.ops.mcgmil.conv2d_bf16."""
    reason = conv_bf16_untrainable_reason(conv, x)
    if reason is not None:
        raise ValueError(f"conv2d_bf16: {reason} (see conv_bf16_trainable)")
    return _conv2d(conv, x)


def conv2d_bf16_wgrad(conv: nn.Conv2d, x: torch.Tensor, dy: torch.Tensor, chunk_pixels: int = 0) -> torch.Tensor:
    """dW [out, in, kh, kw] fp32 of conv(x) given dY (both bf16), on the bf16 HIP weight-gradient
    kernel (mcgmil_conv2d_wgrad_bf16; see conv_bf16_trainable): bf16 operands, fp32 accumulation.
    chunk_pixels caps the output pixels per launch chunk (0: the library's default); the result
    does not depend on it, bitwise."""
    reason = conv_bf16_untrainable_reason(conv, x)
    if reason is not None:
        raise ValueError(f"conv2d_bf16_wgrad: {reason} (see conv_bf16_trainable)")
    return _wgrad(_lib.ConvGradBf16Args, torch.bfloat16, "mcgmil_conv_wgrad_workspace_size_bf16",
                  "mcgmil_conv2d_wgrad_bf16", conv, x, dy, chunk_pixels)


def dgrad_bf16_native(conv: nn.Conv2d, dy: torch.Tensor) -> bool:
    """Whether conv2d_bf16_dgrad runs this convolution's data gradient on the bf16 forward kernel:
    stride 1, a square kernel (one pad k - 1 - p for both axes) and a dY below 2 GiB (the forward
    kernel's input limit). Otherwise conv2d_bf16_dgrad takes aten.convolution_backward; the bf16
    direct kernel for stride 2 and non-square kernels is conv2d_bf16_dgrad_direct, which
    conv2d_bf16_backward calls on the "direct" route."""
    return _square(conv.stride) == 1 and conv.kernel_size[0] == conv.kernel_size[1] and dy.numel() * 2 < 2 ** 31


def _aten_conv_backward_bf16(conv: nn.Conv2d, x: torch.Tensor, dy: torch.Tensor, need_dx: bool, need_dw: bool):
    """(dx, dw) from aten.convolution_backward on bf16 tensors (the weight cast as autocast casts
    it); dw comes back in conv.weight's dtype."""
    w = conv.weight.detach()
    dx, dw = _aten_conv_backward(_ConvShim(w.to(torch.bfloat16), _square(conv.stride), _square(conv.padding)),
                                 x, dy, need_dx, need_dw)
    return dx, dw.to(w.dtype) if need_dw else None


def conv2d_bf16_dgrad(conv: nn.Conv2d, dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """dX (channels-last bf16, x's shape) of conv(x) given dY. When dgrad_bf16_native: the bf16
    forward kernel (mcgmil_conv2d) of dY with the flipped, channel-swapped weight
    (flipped_weight), pad k - 1 - p -- fp32 accumulation and one rounding to bf16. Otherwise
    aten.convolution_backward with output mask (True, False, False)."""
    dy = dy.contiguous(memory_format=torch.channels_last)
    if not dgrad_bf16_native(conv, dy):
        return _aten_conv_backward_bf16(conv, x, dy, True, False)[0]
    shim = _ConvShim(flipped_weight(conv.weight.detach()), 1, conv.kernel_size[0] - 1 - _square(conv.padding))
    dx = conv2d_bf16(shim, dy)
    if tuple(dx.shape) != tuple(x.shape):
        raise ValueError(f"x {tuple(x.shape)} does not belong to this convolution and dy {tuple(dy.shape)}")
    return dx


def dgrad_bf16_direct_supported(conv: nn.Conv2d, dy: torch.Tensor) -> bool:
    """Whether conv2d_bf16_dgrad_direct implements this convolution's data gradient for dy: a CUDA
    bf16 dy [batch, out_channels, OH, OW] below 2 GiB, an fp32 (master) or bf16 weight, and a
    bias-free groups=1 dilation-1 zero-padded convolution with kernel 1..7 per axis, stride 1 or 2,
    pad < kernel and in_channels and out_channels multiples of 64
    (include/mcgmil_conv_dgrad_bf16.h). A `conv_bf16_trainable` convolution is one unless its dY
    reaches 2 GiB, which the forward allows while x stays below it."""
    return _conv_refusal(conv, dy, **_DGRAD_BF16_DIRECT) is None


def conv2d_bf16_dgrad_direct(conv: nn.Conv2d, dy: torch.Tensor, x_shape) -> torch.Tensor:
    """dX (channels-last bf16, shape x_shape) of conv(x) given dY on the direct bf16 HIP
    data-gradient kernel mcgmil_conv2d_dgrad_bf16, stride 1 and 2, square kernel or not: the
    residue classes of the input pixels, each a stride-1 implicit GEMM over its own taps on the
    bf16 MFMA with fp32 accumulation and one rounding (include/mcgmil_conv_dgrad_bf16.h). The
    weight goes in as one weight.to(bfloat16).permute(2, 3, 1, 0).contiguous(); every element of dX
    is written exactly once, so two calls agree bitwise. Raises for anything
    dgrad_bf16_direct_supported refuses."""
    reason = _conv_refusal(conv, dy, **_DGRAD_BF16_DIRECT)
    if reason is not None:
        raise ValueError(f"conv2d_bf16_dgrad_direct: {reason} (dY; see dgrad_bf16_direct_supported)")
    L = _lib.load()
    g = _lib.ConvDgradBf16Args()
    g.fwd = _conv_args(conv, x_shape)
    if int(x_shape[1]) != conv.in_channels or tuple(dy.shape) != _conv_out_shape(g.fwd):
        raise ValueError(f"x_shape {tuple(x_shape)} does not belong to this convolution and dy {tuple(dy.shape)}")
    dy = dy.contiguous(memory_format=_CL)
    wt = conv.weight.detach().to(torch.bfloat16).permute(2, 3, 1, 0).contiguous()     # [kh][kw][in][out]
    dev = dy.device
    dx = torch.empty(tuple(x_shape), dtype=torch.bfloat16, device=dev, memory_format=_CL)
    g.dy, g.w_t, g.dx = _ptr(dy), _ptr(wt), _ptr(dx)
    _lib.check(L.mcgmil_conv2d_dgrad_bf16(ctypes.byref(g), _stream(dev)), "mcgmil_conv2d_dgrad_bf16")
    return dx


def conv2d_bf16_backward(conv: nn.Conv2d, x: torch.Tensor, dy: torch.Tensor, need_dx: bool = True,
                         need_dw: bool = True):
    """(dX bf16 or None, dW in the weight's dtype or None) of conv(x) given dY for a
    `conv_bf16_trainable` convolution: the backward of torch.ops.mcgmil.conv2d_bf16, on the route
    MCGMIL_CONV_GRAD names (conv_grad_route, read on every call). "aten" (the default):
    aten.convolution_backward on bf16 tensors for both gradients. "native": the bf16 HIP weight
    gradient (conv2d_bf16_wgrad; fp32, so an fp32 master weight gets it unrounded) and
    conv2d_bf16_dgrad (stride 1 and a square kernel: the forward kernel on the flipped weight;
    else aten, dx only). "direct": as "native" where dgrad_bf16_native holds, and everywhere else
    (stride 2, a non-square kernel) the direct bf16 HIP data gradient conv2d_bf16_dgrad_direct
    (include/mcgmil_conv_dgrad_bf16.h) -- no gradient of the convolution leaves the project's
    kernels, and both repeat bitwise. A dY of 2 GiB or more (the forward takes it while x is below
    2 GiB) is outside both data-gradient kernels: "native" sends it to aten, "direct" raises."""
    reason = conv_bf16_untrainable_reason(conv, x)
    if reason is not None:
        raise ValueError(f"conv2d_bf16_backward: {reason} (see conv_bf16_trainable)")
    dy = dy.contiguous(memory_format=torch.channels_last)
    route = conv_grad_route()
    if route == "aten":
        return _aten_conv_backward_bf16(conv, x, dy, need_dx, need_dw)
    dw = conv2d_bf16_wgrad(conv, x, dy).to(conv.weight.dtype) if need_dw else None
    dx = None
    if need_dx:
        dx = conv2d_bf16_dgrad_direct(conv, dy, x.shape) if route == "direct" and not dgrad_bf16_native(conv, dy) \
            else conv2d_bf16_dgrad(conv, dy, x)
    return dx, dw


def conv2d_bf16_op(layer: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """layer(x) through the differentiable op torch.ops.mcgmil.conv2d_bf16 (mcgmil.library)."""
    return _conv_op("conv2d_bf16", layer, x)


def _native_conv(conv: nn.Module, x: torch.Tensor) -> Optional[str]:
    """"bf16" (conv2d), "f32" (conv2d_f32) or None (the torch layer) for conv on x."""
    if isinstance(conv, nn.Conv2d):
        if conv_fusable(conv, x):
            return "bf16"
        if conv32_fusable(conv, x):
            return "f32"
    return None


def _takes_input_bn(conv: nn.Module, x: torch.Tensor) -> bool:
    kind = _native_conv(conv, x)
    return (kind == "bf16" and conv_input_bn(conv, x)) or (kind == "f32" and conv32_input_bn(conv, x))


def torch_conv(layer: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """The torch layer, with fp32 convolutions on the GPU split along the batch so that no call's
    input or output reaches 2^31 bytes (MCGMIL_FP32_CONV_CHUNK=0: unsplit). On some MI355X boxes
    the unsplit fp32 stem convolution of a config-5 bag (1,507 instances: a 4.85 GB output) came
    back wrong from MIOpen -- features nrel 1.68 against the CPU, with this build's kernels off --
    while other boxes matched the CPU to 2e-6 (scripts/probe_cfg5_drift.py)."""
    if not (isinstance(layer, nn.Conv2d) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and x.shape[0] > 1 and os.environ.get("MCGMIL_FP32_CONV_CHUNK", "1") != "0"):
        return layer(x)
    oh = (x.shape[2] + 2 * layer.padding[0] - layer.dilation[0] * (layer.kernel_size[0] - 1) - 1) \
        // layer.stride[0] + 1
    ow = (x.shape[3] + 2 * layer.padding[1] - layer.dilation[1] * (layer.kernel_size[1] - 1) - 1) \
        // layer.stride[1] + 1
    per = 4 * max(x[0].numel(), layer.out_channels * oh * ow)
    n = max(1, ((1 << 31) - 1) // per)
    if n >= x.shape[0]:
        return layer(x)
    mf = torch.channels_last if x.is_contiguous(memory_format=torch.channels_last) else torch.contiguous_format
    return torch.cat([layer(x[i:i + n]) for i in range(0, x.shape[0], n)]).contiguous(memory_format=mf)


def run_conv(layer: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """The backbone's convolution: the bf16 MFMA kernel when `conv_fusable`, the fp32 one when
    `conv32_fusable` (at the ambient conv32_precision()), else the torch layer. Inside native_conv_training() a convolution under
    autograd that is `conv32_trainable` goes to the differentiable op instead of the torch layer
    (the activation is made channels-last first if it is not: once, after the stem). Inside
    native_stem_conv_training() the same holds for a `stem_conv_trainable` convolution (1..4 input
    channels: the stem) and torch.ops.mcgmil.stem_conv_f32, and inside native_conv_bf16_training()
    for a `conv_bf16_trainable` convolution (a bf16 activation) and torch.ops.mcgmil.conv2d_bf16.
    Inside native_conv_training() and native_conv_x3_training() a `conv32x3_trainable` convolution
    goes to torch.ops.mcgmil.conv2d_f32x3 in conv2d_f32's place."""
    if (_native_training or _native_stem_conv_training or _native_bf16_training) and isinstance(layer, nn.Conv2d) and \
            torch.is_grad_enabled() and (x.requires_grad or layer.weight.requires_grad) and x.is_cuda and x.dim() == 4:
        xc = x.contiguous(memory_format=torch.channels_last)
        if _native_bf16_training and conv_bf16_trainable(layer, xc):
            return conv2d_bf16_op(layer, xc)
        if _native_training and _native_x3_training and conv32x3_trainable(layer, xc):
            return conv2d_f32x3_op(layer, xc)
        if _native_training and conv32_trainable(layer, xc):
            return conv2d_f32_op(layer, xc)
        if _native_stem_conv_training and stem_conv_trainable(layer, xc):
            return stem_conv_f32_op(layer, xc)
    if isinstance(layer, nn.Conv2d) and conv_fusable(layer, x):
        return conv2d(layer, x)
    if isinstance(layer, nn.Conv2d) and conv32_fusable(layer, x):
        return conv2d_f32(layer, x)
    return torch_conv(layer, x)


# ---------------------------------------------------------------- fused BatchNorm (+ add) (+ ReLU) (+ pool)
def _f32(t: Optional[torch.Tensor], dev) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = t.detach()
    if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
        t = t.to(device=dev, dtype=torch.float32).contiguous()
    return t


def _pool_params(pool) -> Optional[tuple]:
    """(k, stride, pad) of a plain square nn.MaxPool2d the kernel can fuse, else None."""
    if not isinstance(pool, nn.MaxPool2d) or pool.ceil_mode or pool.return_indices:
        return None
    k, st = _square(pool.kernel_size), _square(pool.stride if pool.stride is not None else pool.kernel_size)
    pd, dil = _square(pool.padding), _square(pool.dilation)
    if None in (k, st, pd, dil) or dil != 1 or k < 1 or st < 1 or pd < 0 or 2 * pd > k:
        return None
    return k, st, pd


def _bn_tensors(bn: nn.BatchNorm2d, dev):
    """(uses batch statistics, gamma, beta, running mean, running var) of a layer as the kernels
    take them: fp32 on dev, None where the layer has none or normalises with the batch's."""
    use_batch = _use_batch(bn)
    return (use_batch, _f32(bn.weight, dev) if bn.affine else None, _f32(bn.bias, dev) if bn.affine else None,
            None if use_batch else _f32(bn.running_mean, dev), None if use_batch else _f32(bn.running_var, dev))


def _bn_args(x: torch.Tensor, gamma, beta, eps: float, relu: bool = False, rmean=None, rvar=None) -> "_lib.BnArgs":
    """mcgmil_bn_args for the channels-last [N, C, H, W] activation x and its layer's tensors."""
    N, C, H, W = x.shape
    a = _lib.BnArgs()
    a.rows, a.channels, a.dtype = N * H * W, C, _DT[x.dtype]
    a.batch, a.height, a.width = N, H, W
    a.x = _ptr(x)
    a.gamma, a.beta, a.running_mean, a.running_var = _ptr(gamma), _ptr(beta), _ptr(rmean), _ptr(rvar)
    a.eps, a.relu = float(eps), int(bool(relu))
    return a


def _set_partials(a: "_lib.BnArgs", partials: torch.Tensor, dev) -> None:
    if partials.dim() != 3 or partials.shape[1:] != (3, a.channels) or not partials.is_contiguous() or \
            partials.dtype != torch.float32 or partials.device != dev:
        raise ValueError("partials must be a contiguous fp32 [parts, 3, C] tensor on x's device")
    a.partials, a.num_partials = _ptr(partials), partials.shape[0]


def batchnorm_act(x: torch.Tensor, bn: nn.BatchNorm2d, relu: bool,
                  residual: Optional[torch.Tensor] = None,
                  pool: Optional[nn.MaxPool2d] = None,
                  partials: Optional[torch.Tensor] = None,
                  residual_ab: Optional[torch.Tensor] = None) -> torch.Tensor:
    """relu?(bn(x) [+ residual]) for a channels-last [N, C, H, W] activation (see fusable), or
    pool(relu?(bn(x))) with a fusable max-pool (the ResNet stem) without materialising the
    activation. `partials` ([parts, 3, C] from conv2d(..., stats=True)) supplies the batch
    statistics of x, so x is read once. `residual_ab` ([2, C] from batchnorm_coefficients) is the
    residual's own BatchNorm, applied on the fly (bit-identical to normalising it first)."""
    if not fusable(x, bn, residual):
        raise ValueError("batchnorm_act needs a CUDA channels-last bf16/fp32 activation with "
                         "C % 8 == 0, C <= 2048 and no autograd (see mcgmil.features.fusable)")
    pp = None
    if pool is not None:
        pp = _pool_params(pool)
        if pp is None or residual is not None:
            raise ValueError("only a square nn.MaxPool2d (dilation 1, floor mode), without a "
                             "residual, is fused")
    L = _lib.load()
    dev = x.device
    use_batch, gamma, beta, rmean, rvar = _bn_tensors(bn, dev)
    a = _bn_args(x, gamma, beta, bn.eps, relu, rmean, rvar)
    N, C, H, W = a.batch, a.channels, a.height, a.width
    if pp is None:
        y = torch.empty_like(x, memory_format=torch.channels_last)
    else:
        k, st, pd = pp
        y = torch.empty((N, C) + _out_hw(H, W, k, k, st, pd), dtype=x.dtype, device=dev, memory_format=_CL)
        a.pool_kernel, a.pool_stride, a.pool_pad = k, st, pd
    a.y, a.residual = _ptr(y), _ptr(residual)
    if residual_ab is not None:
        if residual is None or residual_ab.shape != (2, C) or residual_ab.dtype != torch.float32 or \
                residual_ab.device != dev or not residual_ab.is_contiguous():
            raise ValueError("residual_ab needs a residual and a contiguous fp32 [2, C] tensor on x's device")
        a.residual_ab = _ptr(residual_ab)
    if partials is not None and use_batch:
        _set_partials(a, partials, dev)
    _workspace(L.mcgmil_bn_workspace_size, "mcgmil_bn_workspace_size", a, dev)
    _lib.check(L.mcgmil_batchnorm_act(ctypes.byref(a), _stream(dev)), "mcgmil_batchnorm_act")
    return y


def batchnorm_coefficients(x: torch.Tensor, bn: nn.BatchNorm2d,
                           partials: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The [2, C] fp32 (a_c, b_c) that batchnorm_act(x, bn, ...) would apply
    (mcgmil_batchnorm_coefficients), for a consumer that applies them itself (conv2d's in_ab)."""
    if not fusable(x, bn, None):
        raise ValueError("batchnorm_coefficients needs what batchnorm_act needs (see fusable)")
    L = _lib.load()
    dev = x.device
    use_batch, gamma, beta, rmean, rvar = _bn_tensors(bn, dev)
    a = _bn_args(x, gamma, beta, bn.eps, False, rmean, rvar)
    if partials is not None and use_batch:
        _set_partials(a, partials, dev)
    if use_batch:     # the statistics pass, or more than 1024 partials combined in chunks first
        a.y = a.x
        _workspace(L.mcgmil_bn_workspace_size, "mcgmil_bn_workspace_size", a, dev)
    ab = torch.empty((2, a.channels), dtype=torch.float32, device=dev)
    _lib.check(L.mcgmil_batchnorm_coefficients(ctypes.byref(a), _ptr(ab), _stream(dev)), "mcgmil_batchnorm_coefficients")
    return ab


# ---------------------------------------------------------------- fused BatchNorm backward
_native_norm_training = False


@contextlib.contextmanager
def native_norm_training(flag: bool = True):
    """Inside this context `bn_act` sends every pool-free `bn_trainable` BatchNorm (+ residual add)
    (+ ReLU) that autograd tracks to the differentiable op torch.ops.mcgmil.bn_act_f32 (the fused
    HIP forward and its HIP backward, include/mcgmil_bn_grad.h). Off outside it: the opt-in of
    MultiHeadGatedAttentionMIL.enable_backbone_training(norm=True)."""
    global _native_norm_training
    before, _native_norm_training = _native_norm_training, bool(flag)
    try:
        yield
    finally:
        _native_norm_training = before


def _bn_refusal(x: torch.Tensor, bn: nn.Module, residual: Optional[torch.Tensor], dtype: torch.dtype) -> Optional[str]:
    """Why (x, bn, residual) is outside the fused BatchNorm training op of `dtype`, or None. The
    fp32 op refuses autocast; the bf16 one takes what autocast gives it and never asks."""
    if not isinstance(bn, nn.BatchNorm2d) or x.dim() != 4:
        return "layer: an nn.BatchNorm2d on a 4-D activation"
    if x.dtype != dtype or any(p is not None and p.dtype != torch.float32 for p in (bn.weight, bn.bias)):
        return "dtype: fp32 only" if dtype == torch.float32 else "dtype: a bf16 activation with fp32 parameters"
    C = x.shape[1]
    if C % 8 or C > 2048 or C != bn.num_features:
        return "channels: C % 8 == 0, C <= 2048, C == bn.num_features"
    if x.numel() < 2 * C:
        return "rows: at least 2 values per channel"
    if not _use_batch(bn):
        return "statistics: running-statistics mode"
    if bn.training and bn.track_running_stats and bn.running_mean is not None:
        return "statistics: a running-statistics update is pending"     # torch would update them
    if residual is not None and (residual.shape != x.shape or residual.dtype != x.dtype or
                                 residual.device != x.device):
        return "residual: x's shape, dtype and device"
    if not x.is_cuda or any(p is not None and p.device != x.device for p in (bn.weight, bn.bias)):
        return "device: a CUDA activation with the parameters on its device"
    if dtype == torch.float32 and torch.is_autocast_enabled("cuda"):
        return "autocast"
    return None


def bn_untrainable_reason(x: torch.Tensor, bn: nn.Module, residual: Optional[torch.Tensor] = None) -> Optional[str]:
    """Why `bn_trainable` refuses (x, bn, residual), or None when it holds. The device is checked
    last, so the other clauses can be seen on a machine without a GPU."""
    return _bn_refusal(x, bn, residual, torch.float32)


def bn_trainable(x: torch.Tensor, bn: nn.BatchNorm2d, residual: Optional[torch.Tensor] = None) -> bool:
    """A BatchNorm (+ residual add) (+ ReLU) whose forward AND backward run on the fused fp32 HIP
    kernels: a CUDA fp32 4-D activation without autocast, C % 8 == 0, C <= 2048,
    C == bn.num_features, at least 2 values per channel, a BN that normalises with batch
    statistics and has no running-statistics update pending (a BN in train mode that tracks
    running statistics keeps the torch path, which updates them, exactly as in `fusable`), and a
    residual, if any, of x's shape and dtype. Says nothing about autograd or the memory layout
    (`bn_act` makes the activation channels-last first). `bn_untrainable_reason` names the clause
    that fails."""
    return bn_untrainable_reason(x, bn, residual) is None


def _check_rows_c(name: str, dtype: torch.dtype, x: torch.Tensor, **like) -> None:
    if not (x.is_cuda and x.dim() == 4 and x.dtype == dtype and x.shape[1] % 8 == 0 and
            x.shape[1] <= 2048 and x.numel() >= 2 * x.shape[1] and
            x.is_contiguous(memory_format=torch.channels_last)):
        raise ValueError(f"{name} needs a CUDA channels-last {_TWIN[dtype].word} [N, C, H, W] activation with "
                         "C % 8 == 0, C <= 2048 and at least 2 values per channel")
    for n, t in like.items():
        if t is not None and (t.shape != x.shape or t.dtype != x.dtype or t.device != x.device or
                              not t.is_contiguous(memory_format=torch.channels_last)):
            raise ValueError(f"{name}: {n} must be channels-last with x's shape, dtype and device")


def _check_per_channel(name: str, C: int, dev, **vecs) -> None:
    for n, t in vecs.items():
        if t is not None and (t.shape != (C,) or t.dtype != torch.float32 or t.device != dev or
                              not t.is_contiguous()):
            raise ValueError(f"{name}: {n} must be a contiguous fp32 [{C}] tensor on x's device")


def _pool_grad_geometry(k: int, stride: int, pad: int) -> bool:
    """The pool geometry of include/mcgmil_pool_grad.h: k in {2, 3}, 1 <= stride <= k, 0 <= pad <= k / 2."""
    return k in (2, 3) and 1 <= stride <= k and 0 <= pad and 2 * pad <= k


def _bn_stats(dtype: torch.dtype, base: str, x: torch.Tensor, weight: Optional[torch.Tensor],
              bias: Optional[torch.Tensor], residual: Optional[torch.Tensor], eps: float, relu: bool,
              pool: Optional[tuple] = None):
    """The forward of the four BatchNorm training ops, `base` + the dtype's suffix: (y, mean, invstd)
    from mcgmil_batchnorm_act with batch_mean / batch_invstd requested, or with pool = (k, stride,
    pad) (y, mean, invstd, argmax) from mcgmil_batchnorm_pool_train[_bf16]."""
    twin = _TWIN[dtype]
    name = base + twin.suffix
    _check_rows_c(name, dtype, x, residual=residual)
    if pool is not None and not _pool_grad_geometry(*pool):
        raise ValueError(f"{name} needs a pool with kernel 2 or 3, 1 <= stride <= kernel and "
                         "0 <= pad <= kernel / 2")
    L = _lib.load()
    dev = x.device
    a = _bn_args(x, weight, bias, eps, relu)
    N, C, H, W = shape = a.batch, a.channels, a.height, a.width
    if pool is not None:
        k, stride, pad = pool
        shape = (N, C) + _out_hw(H, W, k, k, stride, pad)
        if shape[2] < 1 or shape[3] < 1:
            raise ValueError(f"{name}: the pooling window is larger than the padded input")
    _check_per_channel(name, C, dev, weight=weight, bias=bias)
    y = torch.empty(shape, dtype=dtype, device=dev, memory_format=_CL)
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    invstd = torch.empty(C, dtype=torch.float32, device=dev)
    a.y, a.residual = _ptr(y), _ptr(residual)
    a.batch_mean, a.batch_invstd = _ptr(mean), _ptr(invstd)
    if pool is None:
        _workspace(L.mcgmil_bn_workspace_size, "mcgmil_bn_workspace_size", a, dev)
        _lib.check(L.mcgmil_batchnorm_act(ctypes.byref(a), _stream(dev)), "mcgmil_batchnorm_act")
        return y, mean, invstd
    a.pool_kernel, a.pool_stride, a.pool_pad = pool
    argmax = torch.empty(shape, dtype=torch.uint8, device=dev, memory_format=_CL)
    _workspace(L.mcgmil_bn_workspace_size, "mcgmil_bn_workspace_size", a, dev)
    launch = "mcgmil_batchnorm_pool_train" + twin.suffix
    _lib.check(getattr(L, launch)(ctypes.byref(a), _ptr(argmax), _stream(dev)), launch)
    return y, mean, invstd, argmax


def _bn_act_backward(dtype: torch.dtype, x, y, dy, weight, mean, invstd, relu, need_dx, need_dres, need_dw):
    """batchnorm_act_backward and batchnorm_act_backward_bf16."""
    twin = _TWIN[dtype]
    name = "batchnorm_act_backward" + twin.suffix
    _check_rows_c(name, dtype, x, y=y if relu else None, dy=dy)
    if relu and y is None:
        raise ValueError(f"{name}: relu needs y (the forward's output)")
    need_dres = bool(need_dres and relu)
    if not (need_dx or need_dres or need_dw):
        return None, None, None, None
    L = _lib.load()
    dev = x.device
    N, C, H, W = x.shape
    _check_per_channel(name, C, dev, weight=weight, mean=mean, invstd=invstd)
    dx = torch.empty_like(x, memory_format=torch.channels_last) if need_dx else None
    dres = torch.empty_like(x, memory_format=torch.channels_last) if need_dres else None
    dw = torch.empty(C, dtype=torch.float32, device=dev) if need_dw else None
    db = torch.empty(C, dtype=torch.float32, device=dev) if need_dw else None
    a = twin.bn_grad_args()
    a.rows, a.channels, a.relu = N * H * W, C, int(bool(relu))
    a.x, a.y, a.dy = _ptr(x), _ptr(y if relu else None), _ptr(dy)
    a.gamma, a.mean, a.invstd = _ptr(weight), _ptr(mean), _ptr(invstd)
    a.dx, a.dresidual, a.dgamma, a.dbeta = _ptr(dx), _ptr(dres), _ptr(dw), _ptr(db)
    size, launch = "mcgmil_bn_grad_workspace_size" + twin.suffix, "mcgmil_batchnorm_act_backward" + twin.suffix
    _workspace(getattr(L, size), size, a, dev)
    _lib.check(getattr(L, launch)(ctypes.byref(a), _stream(dev)), launch)
    return dx, dres, dw, db


def _bn_act_op(op: str, bn: nn.BatchNorm2d, x: torch.Tensor, relu: bool, residual: Optional[torch.Tensor]):
    from . import library  # noqa: F401  (registers torch.ops.mcgmil.*)
    x = x.contiguous(memory_format=torch.channels_last)
    if residual is not None:
        residual = residual.contiguous(memory_format=torch.channels_last)
    return getattr(torch.ops.mcgmil, op)(x, bn.weight, bn.bias, residual, float(bn.eps), bool(relu))[0]


def batchnorm_act_stats(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                        residual: Optional[torch.Tensor], eps: float, relu: bool):
    """(y, mean [C], invstd [C]) of relu?(batch_norm(x) [+ residual]) on the batch statistics of x
    (fp32, channels-last): mcgmil_batchnorm_act with batch_mean / batch_invstd requested and the
    statistics from its own pass over x. What the backward (batchnorm_act_backward) needs."""
    return _bn_stats(torch.float32, "batchnorm_act_stats", x, weight, bias, residual, eps, relu)


def batchnorm_act_backward(x: torch.Tensor, y: Optional[torch.Tensor], dy: torch.Tensor,
                           weight: Optional[torch.Tensor], mean: torch.Tensor, invstd: torch.Tensor,
                           relu: bool, need_dx: bool = True, need_dres: bool = False, need_dw: bool = True):
    """(dx, dresidual, dweight, dbias), None where not needed, of batchnorm_act_stats given dy
    (mcgmil_batchnorm_act_backward, include/mcgmil_bn_grad.h). y is the forward's output, read for
    the ReLU mask only (None without ReLU). dresidual exists with ReLU only: without it the
    residual's gradient is dy itself and the caller passes dy on."""
    return _bn_act_backward(torch.float32, x, y, dy, weight, mean, invstd, relu, need_dx, need_dres, need_dw)


def bn_act_f32_op(bn: nn.BatchNorm2d, x: torch.Tensor, relu: bool,
                  residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """relu?(bn(x) [+ residual]) through the differentiable op torch.ops.mcgmil.bn_act_f32
    (mcgmil.library); the activation and the residual are made channels-last first if they are not."""
    return _bn_act_op("bn_act_f32", bn, x, relu, residual)


# ---------------------------------------------------------------- fused bf16 BatchNorm backward
_native_norm_bf16_training = False


@contextlib.contextmanager
def native_norm_bf16_training(flag: bool = True):
    """Inside this context `bn_act` sends every pool-free `bn_bf16_trainable` BatchNorm (+ residual
    add) (+ ReLU) that autograd tracks (a bf16 activation: the blocks under
    torch.autocast("cuda", torch.bfloat16)) to the differentiable op torch.ops.mcgmil.bn_act_bf16
    (the fused HIP forward in bf16 and the HIP backward of include/mcgmil_bn_grad_bf16.h). Off
    outside it: the opt-in of MultiHeadGatedAttentionMIL.enable_bf16_norm_training()."""
    global _native_norm_bf16_training
    before, _native_norm_bf16_training = _native_norm_bf16_training, bool(flag)
    try:
        yield
    finally:
        _native_norm_bf16_training = before


def bn_bf16_untrainable_reason(x: torch.Tensor, bn: nn.Module, residual: Optional[torch.Tensor] = None) -> Optional[str]:
    """Why `bn_bf16_trainable` refuses (x, bn, residual), or None when it holds: the clauses of
    `bn_untrainable_reason` with a bf16 activation and residual, fp32 (master) parameters or none,
    and no autocast clause (the op takes what autocast gives it). The device is checked last, so
    the other clauses can be seen on a machine without a GPU."""
    return _bn_refusal(x, bn, residual, torch.bfloat16)


def bn_bf16_trainable(x: torch.Tensor, bn: nn.BatchNorm2d, residual: Optional[torch.Tensor] = None) -> bool:
    """A BatchNorm (+ residual add) (+ ReLU) whose forward AND backward run on the fused bf16 HIP
    kernels: `bn_trainable` for a CUDA bf16 4-D activation (and residual) with fp32 parameters,
    under autocast or not. `bn_bf16_untrainable_reason` names the clause that fails."""
    return bn_bf16_untrainable_reason(x, bn, residual) is None


def batchnorm_act_stats_bf16(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                             residual: Optional[torch.Tensor], eps: float, relu: bool):
    """(y bf16, mean [C] fp32, invstd [C] fp32) of relu?(batch_norm(x) [+ residual]) on the batch
    statistics of x (bf16, channels-last; weight and bias fp32): mcgmil_batchnorm_act with
    MCGMIL_BF16, batch_mean / batch_invstd requested and the statistics from its own pass over x.
    What the backward (batchnorm_act_backward_bf16) needs."""
    return _bn_stats(torch.bfloat16, "batchnorm_act_stats", x, weight, bias, residual, eps, relu)


def batchnorm_act_backward_bf16(x: torch.Tensor, y: Optional[torch.Tensor], dy: torch.Tensor,
                                weight: Optional[torch.Tensor], mean: torch.Tensor, invstd: torch.Tensor,
                                relu: bool, need_dx: bool = True, need_dres: bool = False, need_dw: bool = True):
    """(dx bf16, dresidual bf16, dweight fp32, dbias fp32), None where not needed, of
    batchnorm_act_stats_bf16 given dy (mcgmil_batchnorm_act_backward_bf16,
    include/mcgmil_bn_grad_bf16.h). y is the forward's output, read for the ReLU mask only (None
    without ReLU). dresidual exists with ReLU only: without it the residual's gradient is dy itself
    and the caller passes dy on."""
    return _bn_act_backward(torch.bfloat16, x, y, dy, weight, mean, invstd, relu, need_dx, need_dres, need_dw)


def bn_act_bf16_op(bn: nn.BatchNorm2d, x: torch.Tensor, relu: bool,
                   residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """relu?(bn(x) [+ residual]) through the differentiable op torch.ops.mcgmil.bn_act_bf16
    (mcgmil.library); the activation and the residual are made channels-last first if they are not."""
    return _bn_act_op("bn_act_bf16", bn, x, relu, residual)


# ---------------------------------------------------------------- fused stem BatchNorm / pool backward
_native_stem_training = False


@contextlib.contextmanager
def native_stem_training(flag: bool = True):
    """Inside this context `bn_act` sends a `bn_pool_trainable` BatchNorm (+ ReLU) + max-pool that
    autograd tracks (the ResNet stem's bn1 / relu / maxpool) to the differentiable op
    torch.ops.mcgmil.bn_pool_f32 (the fused HIP forward that also records the pool's argmax codes,
    and the HIP backward of include/mcgmil_pool_grad.h). Off outside it: the opt-in of
    MultiHeadGatedAttentionMIL.enable_backbone_training(stem=True)."""
    global _native_stem_training
    before, _native_stem_training = _native_stem_training, bool(flag)
    try:
        yield
    finally:
        _native_stem_training = before


def _bn_pool_refusal(x: torch.Tensor, bn: nn.Module, pool: nn.Module, dtype: torch.dtype) -> Optional[str]:
    """The pool's clauses, then those of `_bn_refusal` (the device last)."""
    pp = _pool_params(pool)
    if pp is None or not _pool_grad_geometry(*pp):
        return "pool: a square floor-mode nn.MaxPool2d, dilation 1, kernel 2 or 3, 1 <= stride <= kernel, pad <= kernel / 2"
    if x.dim() == 4 and min(_out_hw(x.shape[2], x.shape[3], pp[0], pp[0], pp[1], pp[2])) < 1:
        return "pool: the window is larger than the padded input"
    return _bn_refusal(x, bn, None, dtype)


def bn_pool_untrainable_reason(x: torch.Tensor, bn: nn.Module, pool: nn.Module) -> Optional[str]:
    """Why `bn_pool_trainable` refuses (x, bn, pool), or None when it holds: the pool's clause, then
    those of `bn_untrainable_reason` (the device last)."""
    return _bn_pool_refusal(x, bn, pool, torch.float32)


def bn_pool_trainable(x: torch.Tensor, bn: nn.BatchNorm2d, pool: nn.Module) -> bool:
    """A BatchNorm (+ ReLU) + max-pool whose forward AND backward run on the fused fp32 HIP kernels
    of include/mcgmil_pool_grad.h: `bn_trainable(x, bn)` and a plain square nn.MaxPool2d
    (`_pool_params`) with kernel 2 or 3, 1 <= stride <= kernel and pad <= kernel / 2.
    `bn_pool_untrainable_reason` names the clause that fails."""
    return bn_pool_untrainable_reason(x, bn, pool) is None


def _bn_pool_backward(dtype: torch.dtype, z, argmax, dy, weight, mean, invstd, k, stride, pad, need_dz, need_dw):
    """batchnorm_pool_backward and batchnorm_pool_backward_bf16."""
    twin = _TWIN[dtype]
    name = "batchnorm_pool_backward" + twin.suffix
    _check_rows_c(name, dtype, z)
    if not _pool_grad_geometry(k, stride, pad):
        raise ValueError(f"{name} needs a pool with kernel 2 or 3, 1 <= stride <= kernel and "
                         "0 <= pad <= kernel / 2")
    dev = z.device
    N, C, H, W = z.shape
    PH, PW = _out_hw(H, W, k, k, stride, pad)
    for n, t, dt in (("argmax", argmax, torch.uint8), ("dy", dy, dtype)):
        if tuple(t.shape) != (N, C, PH, PW) or t.dtype != dt or t.device != dev or \
                not t.is_contiguous(memory_format=torch.channels_last):
            raise ValueError(f"{name}: {n} must be a channels-last {dt} {(N, C, PH, PW)} "
                             "tensor on z's device")
    if not (need_dz or need_dw):
        return None, None, None
    L = _lib.load()
    _check_per_channel(name, C, dev, weight=weight, mean=mean, invstd=invstd)
    dz = torch.empty_like(z, memory_format=torch.channels_last) if need_dz else None
    dw = torch.empty(C, dtype=torch.float32, device=dev) if need_dw else None
    db = torch.empty(C, dtype=torch.float32, device=dev) if need_dw else None
    a = twin.bn_pool_grad_args()
    a.batch, a.height, a.width, a.channels = N, H, W, C
    a.pool_kernel, a.pool_stride, a.pool_pad = k, stride, pad
    a.pooled_height, a.pooled_width = PH, PW
    a.z, a.argmax, a.dy = _ptr(z), _ptr(argmax), _ptr(dy)
    a.gamma, a.mean, a.invstd = _ptr(weight), _ptr(mean), _ptr(invstd)
    a.dz, a.dgamma, a.dbeta = _ptr(dz), _ptr(dw), _ptr(db)
    size, launch = "mcgmil_bn_pool_grad_workspace_size" + twin.suffix, "mcgmil_batchnorm_pool_backward" + twin.suffix
    _workspace(getattr(L, size), size, a, dev)
    _lib.check(getattr(L, launch)(ctypes.byref(a), _stream(dev)), launch)
    return dz, dw, db


def _bn_pool_op(op: str, bn: nn.BatchNorm2d, x: torch.Tensor, relu: bool, pool: nn.MaxPool2d) -> torch.Tensor:
    from . import library  # noqa: F401  (registers torch.ops.mcgmil.*)
    k, stride, pad = _pool_params(pool)
    x = x.contiguous(memory_format=torch.channels_last)
    return getattr(torch.ops.mcgmil, op)(x, bn.weight, bn.bias, float(bn.eps), bool(relu), k, stride, pad)[0]


def batchnorm_pool_stats(z: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                         eps: float, relu: bool, k: int, stride: int, pad: int):
    """(y, mean [C], invstd [C], argmax) of max_pool2d(relu?(batch_norm(z)), k, stride, pad) on the
    batch statistics of z (fp32, channels-last): mcgmil_batchnorm_pool_train. y is bitwise
    batchnorm_act(..., pool=...); argmax is a channels-last uint8 [N, C, PH, PW] tensor of window
    codes kh * k + kw (255: the ReLU zeroes that gradient). What batchnorm_pool_backward needs."""
    return _bn_stats(torch.float32, "batchnorm_pool_stats", z, weight, bias, None, eps, relu, (k, stride, pad))


def batchnorm_pool_backward(z: torch.Tensor, argmax: torch.Tensor, dy: torch.Tensor,
                            weight: Optional[torch.Tensor], mean: torch.Tensor, invstd: torch.Tensor,
                            k: int, stride: int, pad: int, need_dz: bool = True, need_dw: bool = True):
    """(dz, dweight, dbias), None where not needed, of batchnorm_pool_stats given dy
    (mcgmil_batchnorm_pool_backward, include/mcgmil_pool_grad.h). argmax holds the forward's window
    codes; dy is channels-last [N, C, PH, PW]."""
    return _bn_pool_backward(torch.float32, z, argmax, dy, weight, mean, invstd, k, stride, pad, need_dz, need_dw)


def bn_pool_f32_op(bn: nn.BatchNorm2d, x: torch.Tensor, relu: bool, pool: nn.MaxPool2d) -> torch.Tensor:
    """pool(relu?(bn(x))) through the differentiable op torch.ops.mcgmil.bn_pool_f32
    (mcgmil.library); the activation is made channels-last first if it is not."""
    return _bn_pool_op("bn_pool_f32", bn, x, relu, pool)


# ---------------------------------------------------------------- fused bf16 stem BatchNorm / pool backward
_native_stem_bf16_training = False


@contextlib.contextmanager
def native_stem_bf16_training(flag: bool = True):
    """Inside this context `bn_act` sends a `bn_pool_bf16_trainable` BatchNorm (+ ReLU) + max-pool
    that autograd tracks (a bf16 activation: the ResNet stem's bn1 / relu / maxpool under
    torch.autocast("cuda", torch.bfloat16)) to the differentiable op torch.ops.mcgmil.bn_pool_bf16
    (the fused bf16 HIP forward that also records the pool's argmax codes, and the HIP backward of
    include/mcgmil_pool_grad_bf16.h). Off outside it: the opt-in of
    MultiHeadGatedAttentionMIL.enable_bf16_stem_training()."""
    global _native_stem_bf16_training
    before, _native_stem_bf16_training = _native_stem_bf16_training, bool(flag)
    try:
        yield
    finally:
        _native_stem_bf16_training = before


def bn_pool_bf16_untrainable_reason(x: torch.Tensor, bn: nn.Module, pool: nn.Module) -> Optional[str]:
    """Why `bn_pool_bf16_trainable` refuses (x, bn, pool), or None when it holds: the pool's clause
    of `bn_pool_untrainable_reason`, then the clauses of `bn_bf16_untrainable_reason` (the device
    last)."""
    return _bn_pool_refusal(x, bn, pool, torch.bfloat16)


def bn_pool_bf16_trainable(x: torch.Tensor, bn: nn.BatchNorm2d, pool: nn.Module) -> bool:
    """A BatchNorm (+ ReLU) + max-pool whose forward AND backward run on the fused bf16 HIP kernels
    of include/mcgmil_pool_grad_bf16.h: `bn_bf16_trainable(x, bn)` and the pool of
    `bn_pool_trainable`. `bn_pool_bf16_untrainable_reason` names the clause that fails."""
    return bn_pool_bf16_untrainable_reason(x, bn, pool) is None


def batchnorm_pool_stats_bf16(z: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                              eps: float, relu: bool, k: int, stride: int, pad: int):
    """(y bf16, mean [C] fp32, invstd [C] fp32, argmax) of max_pool2d(relu?(batch_norm(z)), k, stride,
    pad) on the batch statistics of z (bf16, channels-last; weight and bias fp32):
    mcgmil_batchnorm_pool_train_bf16. y is bitwise batchnorm_act(..., pool=...) on the bf16 z; argmax
    is a channels-last uint8 [N, C, PH, PW] tensor of window codes kh * k + kw taken on the unrounded
    fp32 activated value (255: the ReLU zeroes that gradient). What batchnorm_pool_backward_bf16
    needs."""
    return _bn_stats(torch.bfloat16, "batchnorm_pool_stats", z, weight, bias, None, eps, relu, (k, stride, pad))


def batchnorm_pool_backward_bf16(z: torch.Tensor, argmax: torch.Tensor, dy: torch.Tensor,
                                 weight: Optional[torch.Tensor], mean: torch.Tensor, invstd: torch.Tensor,
                                 k: int, stride: int, pad: int, need_dz: bool = True, need_dw: bool = True):
    """(dz bf16, dweight fp32, dbias fp32), None where not needed, of batchnorm_pool_stats_bf16 given
    dy (mcgmil_batchnorm_pool_backward_bf16, include/mcgmil_pool_grad_bf16.h). argmax holds the
    forward's window codes; dy is channels-last bf16 [N, C, PH, PW]."""
    return _bn_pool_backward(torch.bfloat16, z, argmax, dy, weight, mean, invstd, k, stride, pad, need_dz, need_dw)


def bn_pool_bf16_op(bn: nn.BatchNorm2d, x: torch.Tensor, relu: bool, pool: nn.MaxPool2d) -> torch.Tensor:
    """pool(relu?(bn(x))) through the differentiable op torch.ops.mcgmil.bn_pool_bf16
    (mcgmil.library); the activation is made channels-last first if it is not."""
    return _bn_pool_op("bn_pool_bf16", bn, x, relu, pool)


def bn_act(bn: nn.BatchNorm2d, x: torch.Tensor, relu: bool,
           residual: Optional[torch.Tensor] = None, pool: Optional[nn.Module] = None) -> torch.Tensor:
    """The backbone's `pool?(relu?(bn(x) [+ residual]))`: fused on the GPU when `fusable`, else
    the torch layers (CPU, autograd, training with running-stat updates, odd layouts). Inside
    native_norm_training() a pool-free `bn_trainable` layer under autograd goes to the
    differentiable fused op instead of the torch layers; inside native_stem_training() a
    residual-free `bn_pool_trainable` layer with a pool does; inside native_norm_bf16_training()
    a pool-free `bn_bf16_trainable` layer (a bf16 activation) goes to the bf16 fused op; inside
    native_stem_bf16_training() a residual-free `bn_pool_bf16_trainable` layer with a pool (a bf16
    activation) goes to the bf16 fused pool op."""
    tracked = torch.is_grad_enabled() and isinstance(bn, nn.BatchNorm2d) and \
        (x.requires_grad or any(p.requires_grad for p in bn.parameters()))
    if _native_stem_training and pool is not None and residual is None and tracked and bn_pool_trainable(x, bn, pool):
        return bn_pool_f32_op(bn, x, relu, pool)
    if _native_norm_training and pool is None and tracked and bn_trainable(x, bn, residual):
        return bn_act_f32_op(bn, x, relu, residual)
    if _native_norm_bf16_training and pool is None and tracked and bn_bf16_trainable(x, bn, residual):
        return bn_act_bf16_op(bn, x, relu, residual)
    if _native_stem_bf16_training and pool is not None and residual is None and tracked and \
            bn_pool_bf16_trainable(x, bn, pool):
        return bn_pool_bf16_op(bn, x, relu, pool)
    if fusable(x, bn, residual):
        if pool is None or (residual is None and _pool_params(pool) is not None):
            return batchnorm_act(x, bn, relu, residual, pool)
        return pool(batchnorm_act(x, bn, relu, residual))
    y = bn(x)
    if residual is not None:
        y = y + residual
    y = torch.relu(y) if relu else y
    return y if pool is None else pool(y)


def stem_enabled() -> bool:
    return os.environ.get("MCGMIL_NATIVE_STEM", "1") != "0"


def stem_fusable(conv: nn.Module, bn: nn.Module, pool: Optional[nn.Module], x: torch.Tensor) -> bool:
    """A CUDA [N, C<=4, H, W] activation that torch would convolve in bf16, a bias-free
    Conv2d(C, 64, k, stride 2) with k + (pad & 1) <= 8 and OW <= 125, a BatchNorm2d(64) the fused
    BN handles (see fusable), and a plain max-pool (or none); no autograd."""
    if not (stem_enabled() and isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d)):
        return False
    if not (x.is_cuda and x.dim() == 4 and x.dtype in _DT and x.numel() > 0):
        return False
    if conv.groups != 1 or conv.bias is not None or conv.padding_mode != "zeros":
        return False
    if _square(conv.dilation) != 1 or _square(conv.stride) != 2 or not isinstance(conv.padding, tuple) \
            or _square(conv.padding) is None or _square(conv.kernel_size) is None:
        return False
    k, pad = conv.kernel_size[0], conv.padding[0]
    N, C, H, W = x.shape
    if C != conv.in_channels or not 1 <= C <= 4 or conv.out_channels != 64 or bn.num_features != 64:
        return False
    if k + (pad & 1) > 8 or W % 2 or H + 2 * pad < k or W + 2 * pad < k or (W + 2 * pad - k) // 2 + 1 > 125:
        return False
    if pool is not None and _pool_params(pool) is None:
        return False
    bf16 = x.dtype == torch.bfloat16 or conv.weight.dtype == torch.bfloat16 or \
        (torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16)
    if not bf16:
        return False
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in conv.parameters())
                                    or any(p.requires_grad for p in bn.parameters())):
        return False
    if bn.training and bn.track_running_stats and bn.running_mean is not None:
        return False
    return True


def _stem_args(conv: nn.Conv2d, x: torch.Tensor) -> "_lib.StemArgs":
    a = _lib.StemArgs()
    a.batch, a.in_channels, a.height, a.width = x.shape
    a.out_channels, a.kernel = conv.out_channels, conv.kernel_size[0]
    a.stride, a.pad = conv.stride[0], conv.padding[0]
    return a


def packed_stem_weight(conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """The stem weight in the kernel's MFMA fragment order (bf16), cached on the module and keyed
    by the weight's version."""
    w = conv.weight.detach()
    key = (w.data_ptr(), w._version, w.dtype, x.device)
    cached = getattr(conv, "_mcgmil_stem_packed", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    L = _lib.load()
    a = _stem_args(conv, x)
    n = ctypes.c_size_t()
    _lib.check(L.mcgmil_stem_packed_size(ctypes.byref(a), ctypes.byref(n)), "mcgmil_stem_packed_size")
    wc = w.to(device=x.device).contiguous()
    if wc.dtype not in _DT:
        wc = wc.float()
    packed = torch.empty(n.value, dtype=torch.uint8, device=x.device)
    _lib.check(L.mcgmil_pack_stem_weights(ctypes.byref(a), _ptr(wc), _DT[wc.dtype], _ptr(packed), _stream(x.device)),
               "mcgmil_pack_stem_weights")
    conv._mcgmil_stem_packed = (key, packed)
    return packed


def stem(conv: nn.Conv2d, bn: nn.BatchNorm2d, relu: bool, pool: Optional[nn.MaxPool2d],
         x: torch.Tensor, flags: int = 0) -> torch.Tensor:
    """pool?(relu?(bn(conv(x)))) of NCHW instances (see stem_fusable) -> channels-last bf16.
    flags: mcgmil_stem_args.flags (MCGMIL_STEM_POOL_UNSPLIT: one pooling pass; 0 = the split)."""
    if not stem_fusable(conv, bn, pool, x):
        raise ValueError("stem needs a CUDA [N, C<=4, H, W] bf16 (or autocast) input, a bias-free "
                         "stride-2 Conv2d(C, 64) with k + (pad & 1) <= 8 and OW <= 125, a "
                         "BatchNorm2d(64) and a square max-pool, without autograd (see stem_fusable)")
    L = _lib.load()
    dev = x.device
    xb = x.to(torch.bfloat16).contiguous()
    a = _stem_args(conv, xb)
    N, _, H, W = xb.shape
    PH, PW = _out_hw(H, W, a.kernel, a.kernel, 2, a.pad)
    if pool is not None:
        k, st, pd = _pool_params(pool)
        a.pool_kernel, a.pool_stride, a.pool_pad = k, st, pd
        PH, PW = _out_hw(PH, PW, k, k, st, pd)
    _, gamma, beta, rmean, rvar = _bn_tensors(bn, dev)
    w = packed_stem_weight(conv, xb)
    y = torch.empty((N, 64, PH, PW), dtype=torch.bfloat16, device=dev, memory_format=torch.channels_last)
    a.x, a.w, a.y = _ptr(xb), _ptr(w), _ptr(y)
    a.gamma, a.beta, a.running_mean, a.running_var = _ptr(gamma), _ptr(beta), _ptr(rmean), _ptr(rvar)
    a.eps, a.relu = float(bn.eps), int(bool(relu))
    a.flags = int(flags)
    _workspace(L.mcgmil_stem_workspace_size, "mcgmil_stem_workspace_size", a, dev)
    _lib.check(L.mcgmil_stem_forward(ctypes.byref(a), _stream(dev)), "mcgmil_stem_forward")
    return y


# ---------------------------------------------------------------- bf16 stem convolution backward
_native_stem_conv_bf16_training = False


@contextlib.contextmanager
def native_stem_conv_bf16_training(flag: bool = True):
    """Inside this context `run_stem` sends a `stem_conv_bf16_trainable` convolution that autograd
    tracks and torch would run in bf16 (a bf16 input, or torch.autocast("cuda", torch.bfloat16): the
    7x7 stem of the NCHW instances) to the differentiable op torch.ops.mcgmil.stem_conv_bf16: the
    bf16 MFMA forward kernel of the inference stem without its BatchNorm, and the bf16 HIP weight
    gradient of include/mcgmil_stem_grad_bf16.h. Off outside it: the opt-in of
    MultiHeadGatedAttentionMIL.enable_bf16_stem_conv_training()."""
    global _native_stem_conv_bf16_training
    before, _native_stem_conv_bf16_training = _native_stem_conv_bf16_training, bool(flag)
    try:
        yield
    finally:
        _native_stem_conv_bf16_training = before


def stem_conv_bf16_untrainable_reason(conv: nn.Module, x: torch.Tensor) -> Optional[str]:
    """Why conv on x is not a convolution whose forward AND weight gradient run on the bf16 stem
    kernels (mcgmil_stem_conv_bf16, mcgmil_stem_wgrad_bf16; include/mcgmil_stem_grad_bf16.h), or
    None when it is: a CUDA [N, 1..4, H, W] fp32 or bf16 activation (any layout: it is cast to
    bf16 NCHW) whose bf16 copy stays below 2 GiB, an fp32 (master) or bf16 weight, a bias-free
    groups=1 dilation-1 zero-padded Conv2d(C, 64, k, stride 2) with a square kernel and padding,
    k + (pad & 1) <= 8, an even width, OW <= 125 and batch * OH * OW < 2^31 - 256. Says nothing
    about autograd or autocast."""
    if not isinstance(conv, nn.Conv2d):
        return "not an nn.Conv2d"
    if not (x.is_cuda and x.dim() == 4):
        return "the activation is not a 4-d CUDA tensor"
    if x.dtype not in _DT:
        return "the activation must be fp32 or bf16"
    if conv.weight.dtype not in _DT:
        return "the weight must be fp32 or bf16"
    if conv.groups != 1 or conv.bias is not None or conv.padding_mode != "zeros":
        return "only a bias-free groups=1 zero-padded convolution"
    if _square(conv.dilation) != 1 or _square(conv.stride) != 2 or not isinstance(conv.padding, tuple) or \
            _square(conv.padding) is None or _square(conv.kernel_size) is None:
        return "dilation 1, stride 2, a square kernel and a square integer padding"
    k, pad = conv.kernel_size[0], conv.padding[0]
    if k + (pad & 1) > 8:
        return "kernel + (pad & 1) must be at most 8"
    if not 1 <= conv.in_channels <= 4:
        return "in_channels must be in 1..4"
    if conv.out_channels != 64:
        return "out_channels must be 64"
    N, C, H, W = x.shape
    if C != conv.in_channels:
        return "the activation's channels are not the convolution's in_channels"
    if x.numel() == 0:
        return "the activation must be non-empty"
    if W % 2:
        return "the width must be even"
    if H + 2 * pad < k or W + 2 * pad < k:
        return "the kernel does not fit the padded input"
    oh, ow = _out_hw(H, W, k, k, 2, pad)
    if ow > 125:
        return "the output width must be at most 125"
    if x.numel() * 2 >= 2 ** 31:
        return "the bf16 activation must be smaller than 2 GiB"
    if N * oh * ow >= 2 ** 31 - 256:
        return "batch * OH * OW must be below 2^31 - 256"
    return None


def stem_conv_bf16_trainable(conv: nn.Module, x: torch.Tensor) -> bool:
    """stem_conv_bf16_untrainable_reason(conv, x) is None. Says nothing about autograd."""
    return stem_conv_bf16_untrainable_reason(conv, x) is None


def _stem_bf16_input(name: str, conv: nn.Module, x: torch.Tensor) -> torch.Tensor:
    reason = stem_conv_bf16_untrainable_reason(conv, x)
    if reason is not None:
        raise ValueError(f"{name}: {reason} (see stem_conv_bf16_trainable)")
    return x.detach().to(torch.bfloat16).contiguous()      # as features.stem casts it


def stem_conv_bf16(conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """z = conv(x) (channels-last bf16 [N, 64, OH, OW]) for a `stem_conv_bf16_trainable`
    convolution: the stem kernel of `stem` without its BatchNorm (mcgmil_stem_conv_bf16; bf16
    operands, fp32 accumulation, one rounding). x is cast to bf16 NCHW as `stem` casts it; z may
    exceed 2 GiB. The forward of torch.ops.mcgmil.stem_conv_bf16."""
    xb = _stem_bf16_input("stem_conv_bf16", conv, x)
    L = _lib.load()
    dev = xb.device
    a = _stem_args(conv, xb)
    OH, OW = _out_hw(xb.shape[2], xb.shape[3], a.kernel, a.kernel, 2, a.pad)
    w = packed_stem_weight(conv, xb)
    z = torch.empty((xb.shape[0], 64, OH, OW), dtype=torch.bfloat16, device=dev, memory_format=_CL)
    a.x, a.w, a.y = _ptr(xb), _ptr(w), _ptr(z)
    _lib.check(L.mcgmil_stem_conv_bf16(ctypes.byref(a), _stream(dev)), "mcgmil_stem_conv_bf16")
    return z


def stem_conv_bf16_wgrad(conv: nn.Conv2d, x: torch.Tensor, dy: torch.Tensor, chunk_pixels: int = 0) -> torch.Tensor:
    """dW [64, in, k, k] fp32 of conv(x) given dY (bf16 [N, 64, OH, OW]) for a
    `stem_conv_bf16_trainable` convolution, on the bf16 HIP kernel mcgmil_stem_wgrad_bf16: x cast
    to bf16 NCHW as the forward read it, bf16 operands, fp32 accumulation. chunk_pixels caps the
    output pixels per launch chunk (0: the library's default); the result does not depend on it,
    bitwise."""
    xb = _stem_bf16_input("stem_conv_bf16_wgrad", conv, x)
    L = _lib.load()
    dev = xb.device
    g = _lib.StemGradBf16Args()
    g.fwd = _stem_args(conv, xb)
    a = g.fwd
    shape = (a.batch, 64) + _out_hw(a.height, a.width, a.kernel, a.kernel, 2, a.pad)
    if tuple(dy.shape) != shape or dy.dtype != torch.bfloat16 or dy.device != dev:
        raise ValueError(f"dy must be bf16 {shape} on x's device")
    dy = dy.contiguous(memory_format=_CL)
    dw = torch.empty((64, a.in_channels, a.kernel, a.kernel), dtype=torch.float32, device=dev)
    a.x, g.dy, g.dw = _ptr(xb), _ptr(dy), _ptr(dw)
    g.chunk_pixels = int(chunk_pixels)
    _workspace(L.mcgmil_stem_wgrad_workspace_size_bf16, "mcgmil_stem_wgrad_workspace_size_bf16", g, dev)
    _lib.check(L.mcgmil_stem_wgrad_bf16(ctypes.byref(g), _stream(dev)), "mcgmil_stem_wgrad_bf16")
    return dw


def stem_conv_bf16_op(layer: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """layer(x) through the differentiable op torch.ops.mcgmil.stem_conv_bf16 (mcgmil.library)."""
    return _conv_op("stem_conv_bf16", layer, x)


def _stem_conv_bf16_routed(conv: nn.Module, x: torch.Tensor) -> bool:
    if not (_native_stem_conv_bf16_training and isinstance(conv, nn.Conv2d) and torch.is_grad_enabled()
            and (conv.weight.requires_grad or x.requires_grad)):
        return False
    bf16 = x.dtype == torch.bfloat16 or \
        (torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16)
    return bf16 and stem_conv_bf16_trainable(conv, x)


def run_stem(conv: nn.Module, bn: nn.Module, pool: Optional[nn.Module], x: torch.Tensor) -> torch.Tensor:
    """The backbone's stem: the fused kernel when `stem_fusable`, else conv + bn_act (on the GPU
    with a channels-last activation, so the blocks after it stay on the fused path). Inside
    native_stem_conv_bf16_training() a `stem_conv_bf16_trainable` convolution that autograd tracks
    and torch would run in bf16 goes to torch.ops.mcgmil.stem_conv_bf16, straight from the NCHW
    input, and bn_act takes the rest of the stem."""
    if stem_fusable(conv, bn, pool, x):
        return stem(conv, bn, True, pool, x)
    if _stem_conv_bf16_routed(conv, x):
        return bn_act(bn, stem_conv_bf16_op(conv, x), True, pool=pool)
    if x.is_cuda and x.dim() == 4:
        x = x.contiguous(memory_format=torch.channels_last)
    if isinstance(conv, nn.Conv2d) and conv32_fusable(conv, x) and isinstance(bn, nn.BatchNorm2d) \
            and _use_batch(bn):
        y, part = conv2d_f32(conv, x, stats=True)    # statistics from the convolution's epilogue
        if fusable(y, bn) and (pool is None or _pool_params(pool) is not None):
            return batchnorm_act(y, bn, True, pool=pool, partials=part)
        return bn_act(bn, y, True, pool=pool)
    return bn_act(bn, run_conv(conv, x), True, pool=pool)


class DeferredBN(NamedTuple):
    """relu?(bn(y)) left unapplied: the next convolution applies it to its input (conv2d's
    in_ab), so the activation is neither written nor read a second time."""
    y: torch.Tensor
    ab: torch.Tensor                    # [2, C] fp32 (a_c, b_c) from batchnorm_coefficients
    relu: bool
    bn: nn.BatchNorm2d
    partials: Optional[torch.Tensor]    # the statistics ab came from (None: running statistics)

    def materialise(self) -> torch.Tensor:
        return batchnorm_act(self.y, self.bn, self.relu, partials=self.partials)


def conv_bn_act(conv: nn.Module, bn: nn.Module, x, relu: bool, residual=None,
                consumer: Optional[nn.Module] = None, as_residual: bool = False):
    """The blocks' `relu?(bn(conv(x)) [+ residual])`: on the GPU the MFMA convolution (bf16 or
    fp32) also emits the BatchNorm batch statistics of its output (when the BN normalises with
    them), and the fused BN consumes them -- the activation is written once and read once. Else
    run_conv + bn_act.
    x may be a DeferredBN (its BN runs inside this convolution). With `consumer` (the convolution
    that reads the result) and no residual, the result may come back as a DeferredBN when that
    convolution can apply the BN itself (conv_input_bn); pass it on to conv_bn_act. With
    as_residual (the downsample branch) a ReLU-free result may come back as a DeferredBN too; pass
    it as conv_bn_act's residual, whose fused BN applies it while adding."""
    res_ab, res_deferred = None, None
    if isinstance(residual, DeferredBN):
        if residual.relu:
            residual = residual.materialise()
        else:
            res_deferred, residual, res_ab = residual, residual.y, residual.ab
    kw = {}
    if isinstance(x, DeferredBN):
        if _takes_input_bn(conv, x.y):
            kw = {"in_ab": x.ab, "in_relu": x.relu}
            x = x.y
        else:
            x = x.materialise()
    kind = _native_conv(conv, x)
    if kind is not None:
        native = conv2d if kind == "bf16" else conv2d_f32
        if isinstance(bn, nn.BatchNorm2d) and _use_batch(bn):
            y, part = native(conv, x, stats=True, **kw)
        else:
            y, part = native(conv, x, **kw), None
        if not (isinstance(bn, nn.BatchNorm2d) and fusable(y, bn, residual)):
            return bn_act(bn, y, relu, res_deferred.materialise() if res_deferred else residual)
        if residual is None and ((isinstance(consumer, nn.Conv2d) and _takes_input_bn(consumer, y))
                                 or (as_residual and not relu and fold_enabled())):
            return DeferredBN(y, batchnorm_coefficients(y, bn, part), relu, bn, part)
        return batchnorm_act(y, bn, relu, residual, partials=part, residual_ab=res_ab)
    return bn_act(bn, run_conv(conv, x), relu, res_deferred.materialise() if res_deferred else residual)
