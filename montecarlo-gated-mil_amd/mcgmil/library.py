"""torch.library registration of the MCDO head ("register it with
torch.library.custom_op so it composes with torch.compile / autograd-free inference").

    torch.ops.mcgmil.mcdo_forward(H, bag_offsets, Wv, bv, Wu, bu, wa, ba, wk, T, p_feat, p_att,
                                  seed, bag_id_base=0, t_base=0) -> (Y [B, T, C], A [T*C*R])
    torch.ops.mcgmil.mcdo_forward_stats(...same...) -> (Y, A_mean [C*R], A_var [C*R], P_mean [B, C])
    torch.ops.mcgmil.mcdo_backward(H, bag_offsets, Wv, ..., wk, A, Y, dY, dA, T, p_feat, p_att, seed,
                                   bag_id_base=0, t_base=0, need_dH=True)
                                  -> (dH [R, L] or [0, L], dWv, dbv, dWu, dbu, dwa, dba, dwk)

    torch.ops.mcgmil.conv2d_f32(x, weight, stride, pad) -> y
    torch.ops.mcgmil.conv2d_f32_backward(x, weight, dy, stride, pad, need_dx, need_dw) -> (dx, dw)

    torch.ops.mcgmil.bn_act_f32(x, weight?, bias?, residual?, eps, relu) -> (y, mean, invstd)
    torch.ops.mcgmil.bn_act_f32_backward(x, y, dy, weight?, mean, invstd, relu, need_dx, need_dres,
                                         need_dw) -> (dx, dres, dweight, dbias)

    torch.ops.mcgmil.bn_pool_f32(z, weight?, bias?, eps, relu, k, stride, pad) -> (y, mean, invstd, argmax)
    torch.ops.mcgmil.bn_pool_f32_backward(z, argmax, dy, weight?, mean, invstd, k, stride, pad, need_dz,
                                          need_dw) -> (dz, dweight, dbias)

    torch.ops.mcgmil.stem_conv_f32(x, weight, stride, pad) -> y
    torch.ops.mcgmil.stem_conv_f32_backward(x, weight, dy, stride, pad, need_dx, need_dw) -> (dx, dw)

    torch.ops.mcgmil.conv2d_bf16(x, weight, stride, pad) -> y
    torch.ops.mcgmil.conv2d_bf16_backward(x, weight, dy, stride, pad, need_dx, need_dw) -> (dx, dw)

    torch.ops.mcgmil.bn_act_bf16(x, weight?, bias?, residual?, eps, relu) -> (y, mean, invstd)
    torch.ops.mcgmil.bn_act_bf16_backward(x, y, dy, weight?, mean, invstd, relu, need_dx, need_dres,
                                          need_dw) -> (dx, dres, dweight, dbias)

    torch.ops.mcgmil.bn_pool_bf16(z, weight?, bias?, eps, relu, k, stride, pad) -> (y, mean, invstd, argmax)
    torch.ops.mcgmil.bn_pool_bf16_backward(z, argmax, dy, weight?, mean, invstd, k, stride, pad, need_dz,
                                           need_dw) -> (dz, dweight, dbias)

    torch.ops.mcgmil.stem_conv_bf16(x, weight, stride, pad) -> y
    torch.ops.mcgmil.stem_conv_bf16_backward(x, weight, dy, stride, pad, need_dx, need_dw) -> (dx, dw)

    torch.ops.mcgmil.conv2d_f32x3(x, weight, stride, pad) -> y
    torch.ops.mcgmil.conv2d_f32x3_backward(x, weight, dy, stride, pad, need_dx, need_dw) -> (dx, dw)

mcdo_forward is differentiable in H and the seven parameter tensors: its autograd formula
(register_autograd, the only autograd mechanism of the package) calls mcdo_backward, which draws
the dropout masks again from the seed instead of saving them. mcdo_backward itself has no
autograd formula, so a backward of the backward raises. conv2d_f32 is the backbone's fp32
convolution (features.conv2d_f32: x fp32 NCHW-shaped, channels-last in memory; weight
[out, in, kh, kw]) made differentiable in x and weight the same way: its formula calls
conv2d_f32_backward (features.conv2d_f32_backward: the HIP weight gradient and the forward kernel
as data gradient with MCGMIL_CONV_GRAD=native, the HIP weight gradient and the direct HIP data
gradient of include/mcgmil_conv_dgrad.h with MCGMIL_CONV_GRAD=direct, else
aten.convolution_backward -- the measured-fastest today), which has none itself. A gradient that is not needed comes
back as an empty tensor.

bn_act_f32 is the blocks' relu?(batch_norm(x) [+ residual]) on the batch statistics of x (fp32,
x NCHW-shaped and channels-last in memory, made so if it is not): the fused forward
features.batchnorm_act_stats, which also returns the per-channel mean and 1 / sqrt(var + eps) it
used. It is differentiable in x, weight, bias and residual; its formula saves x, weight, mean,
invstd (and y for the ReLU mask) and calls bn_act_f32_backward (features.batchnorm_act_backward,
include/mcgmil_bn_grad.h), which has no formula itself. mean and invstd are returned for that
backward: gradients flowing into them are ignored (they are not differentiable outputs). Without
ReLU the residual's gradient is dy itself: bn_act_f32_backward then returns an empty dres and the
formula passes dy on.

bn_pool_f32 is the stem's max_pool2d(relu?(batch_norm(z)), k, stride, pad) on the batch statistics
of z (fp32, channels-last; k in {2, 3}, 1 <= stride <= k, pad <= k / 2): the fused forward
features.batchnorm_pool_stats, which also returns mean, 1 / sqrt(var + eps) and one uint8 per
pooled element that names the window's winning tap (255: the ReLU zeroes that gradient). It is
differentiable in z, weight and bias; its formula saves only z, argmax, mean, invstd and weight
(neither the activation nor y, nor int64 indices) and calls bn_pool_f32_backward
(features.batchnorm_pool_backward, include/mcgmil_pool_grad.h), which has no formula itself.
Gradients flowing into mean, invstd and argmax are ignored.

stem_conv_f32 is the convolution with 1..4 input channels (features.stem_conv_trainable: the 7x7
stride-2 stem): its forward is features.conv2d_f32 in the gather mode, bitwise what the inference
path gives; its formula calls stem_conv_f32_backward, whose dW always comes from the HIP kernel of
include/mcgmil_stem_grad.h (features.conv2d_f32_stem_wgrad) and whose dX, only when asked for (the
model never does), from aten.convolution_backward. stem_conv_f32_backward has no formula itself.

conv2d_bf16 is the block convolution in mixed precision (features.conv_bf16_trainable: x bf16
NCHW-shaped, channels-last in memory; weight [out, in, kh, kw], the fp32 master or bf16; in and out
channels multiples of 64): its forward is the bf16 MFMA kernel of features.conv2d, bit for bit; its
formula calls conv2d_bf16_backward (features.conv2d_bf16_backward), which has none itself. With
MCGMIL_CONV_GRAD=native the weight gradient is the bf16 HIP kernel of
include/mcgmil_conv_grad_bf16.h (bf16 operands, fp32 accumulation, fp32 dW) and the stride-1 data
gradient the forward kernel on the flipped weight (stride 2: aten, dx only); =direct is native
with the direct bf16 HIP data gradient of include/mcgmil_conv_dgrad_bf16.h wherever native takes
aten (stride 2, a non-square kernel), so no gradient leaves the project's kernels; else
aten.convolution_backward on bf16 tensors. dw comes back in the weight's dtype and contiguous, dx bf16 channels-last.

bn_act_bf16 is bn_act_f32 in mixed precision: x, residual and y bf16, weight and bias the fp32
master parameters, mean and invstd fp32 (features.batchnorm_act_stats_bf16: mcgmil_batchnorm_act
with MCGMIL_BF16). Its formula saves the same tensors and calls bn_act_bf16_backward
(features.batchnorm_act_backward_bf16, include/mcgmil_bn_grad_bf16.h), which has no formula itself:
dx and dres come back bf16, dweight and dbias fp32. Without ReLU the residual's gradient is dy
itself; gradients flowing into mean and invstd are ignored.

bn_pool_bf16 is bn_pool_f32 in mixed precision: z and y bf16, weight and bias the fp32 master
parameters, mean and invstd fp32 (features.batchnorm_pool_stats_bf16:
mcgmil_batchnorm_pool_train_bf16). The codes name the largest UNROUNDED fp32 value of the window
(where two taps round to the same bf16 value torch's autocast layers name the first of them
instead; both are subgradients of the same y). Its formula saves the same tensors, z, argmax, mean,
invstd and weight alone, and calls bn_pool_bf16_backward (features.batchnorm_pool_backward_bf16,
include/mcgmil_pool_grad_bf16.h), which has no formula itself: dz comes back bf16, dweight and
dbias fp32.

stem_conv_bf16 is the stem convolution in mixed precision (features.stem_conv_bf16_trainable: x
[N, 1..4, H, W] fp32 or bf16 in ANY layout -- it is cast to bf16 NCHW, the layout the stem kernel
reads; weight [64, in, k, k], the fp32 master or bf16; stride 2): its forward is the inference
stem's bf16 MFMA kernel without the BatchNorm (features.stem_conv_bf16), y bf16 channels-last; its
formula saves x and weight (x as it came in: the cast is made again in the backward instead of
keeping a bf16 copy alive through the step) and calls stem_conv_bf16_backward, which has no formula
itself. dw always comes from the bf16 HIP kernel of include/mcgmil_stem_grad_bf16.h
(features.stem_conv_bf16_wgrad; MCGMIL_CONV_GRAD does not matter) and comes back in the weight's
dtype, so the fp32 master gets it unrounded; dx, only when asked for (the model never does), from
aten.convolution_backward on bf16 tensors, bf16 channels-last. The two names are listed in
STEM_BF16_OPS, not in __all__.

conv2d_f32x3 is the block convolution with fp32 storage on the bf16 matrix pipe
(features.conv32x3_trainable: conv2d_f32's domain with in_channels a multiple of 32; x and weight
fp32): its forward is features.conv2d_f32x3 (mcgmil_conv2d_f32x3, three bf16 MFMA products per K),
bit for bit what features.conv2d_f32(..., precision="bf16x3") gives; its formula calls
conv2d_f32x3_backward (features.conv2d_f32x3_backward), which has none itself: dw from the bf16x3 HIP
weight gradient of include/mcgmil_conv_grad_x3.h, dx from the bf16x3 forward kernel on the flipped
weight for stride 1 and from the exact fp32 direct kernel of include/mcgmil_conv_dgrad.h for
stride 2. MCGMIL_CONV_GRAD does not matter: no gradient leaves the project's kernels and both repeat
bitwise. The two names are listed in CONV_X3_OPS, not in __all__.

Same semantics as `mcgmil.ops.mcdo_forward` (reference model.py:256-328 for every bag of the
batch, bags as CSR row ranges of H). The ops are opaque to a graph capture: the fake (meta)
implementations below only derive output shapes, and the real ones run the gfx950 kernels
through the C ABI. There is no CPU kernel: called with CPU tensors they raise. `seed` is the
64-bit Philox key as a signed int64 (the schema's int); it is reinterpreted as unsigned.

Each family of backbone ops (the convolutions, bn_act, bn_pool) is written once, as a function
that defines and registers an op, its fake, its backward op, that one's fake and the autograd
formula for one dtype; what differs between the members is its arguments. The `features` functions
are named, not passed, and looked up on every call.
"""
from typing import Callable, Optional, Tuple

import torch

from . import features, ops

__all__ = ["mcdo_forward", "mcdo_forward_stats", "mcdo_backward", "conv2d_f32", "conv2d_f32_backward",
           "bn_act_f32", "bn_act_f32_backward", "bn_pool_f32", "bn_pool_f32_backward",
           "stem_conv_f32", "stem_conv_f32_backward", "conv2d_bf16", "conv2d_bf16_backward",
           "bn_act_bf16", "bn_act_bf16_backward", "bn_pool_bf16", "bn_pool_bf16_backward"]


def _head(Wv, bv, Wu, bu, wa, ba, wk) -> ops.HeadTensors:
    return ops.HeadTensors(Wv, bv, Wu, bu, wa, ba, wk)


@torch.library.custom_op("mcgmil::mcdo_forward", mutates_args=())
def mcdo_forward(H: torch.Tensor, bag_offsets: torch.Tensor, Wv: torch.Tensor, bv: torch.Tensor,
                 Wu: torch.Tensor, bu: torch.Tensor, wa: torch.Tensor, ba: torch.Tensor,
                 wk: torch.Tensor, T: int, p_feat: float, p_att: float, seed: int,
                 bag_id_base: int = 0, t_base: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    out = ops.mcdo_forward(H, bag_offsets, _head(Wv, bv, Wu, bu, wa, ba, wk), T, p_feat=p_feat,
                           p_att=p_att, seed=seed & 0xFFFFFFFFFFFFFFFF, bag_id_base=bag_id_base,
                           t_base=t_base)
    return out["Y"], out["A"]


@mcdo_forward.register_fake
def _mcdo_forward_fake(H, bag_offsets, Wv, bv, Wu, bu, wa, ba, wk, T, p_feat, p_att, seed,
                       bag_id_base=0, t_base=0):
    B, C, R = bag_offsets.shape[0] - 1, wa.shape[0], H.shape[0]
    return (H.new_empty((B, T, C), dtype=torch.float32),
            H.new_empty((T * C * R,), dtype=torch.float32))


@torch.library.custom_op("mcgmil::mcdo_backward", mutates_args=())
def mcdo_backward(H: torch.Tensor, bag_offsets: torch.Tensor, Wv: torch.Tensor, bv: torch.Tensor,
                  Wu: torch.Tensor, bu: torch.Tensor, wa: torch.Tensor, ba: torch.Tensor,
                  wk: torch.Tensor, A: torch.Tensor, Y: torch.Tensor, dY: torch.Tensor,
                  dA: Optional[torch.Tensor], T: int, p_feat: float, p_att: float, seed: int,
                  bag_id_base: int = 0, t_base: int = 0, need_dH: bool = True
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                             torch.Tensor, torch.Tensor, torch.Tensor]:
    g = ops.mcdo_backward(H, bag_offsets, _head(Wv, bv, Wu, bu, wa, ba, wk), T, A, Y, dY, dA,
                          p_feat=p_feat, p_att=p_att, seed=seed & 0xFFFFFFFFFFFFFFFF,
                          bag_id_base=bag_id_base, t_base=t_base, need_dH=need_dH)
    dH = g["dH"] if need_dH else H.new_empty((0, H.shape[1]), dtype=torch.float32)
    return (dH,) + tuple(g[n] for n in ops.GRAD_NAMES)


@mcdo_backward.register_fake
def _mcdo_backward_fake(H, bag_offsets, Wv, bv, Wu, bu, wa, ba, wk, A, Y, dY, dA, T, p_feat, p_att,
                        seed, bag_id_base=0, t_base=0, need_dH=True):
    f = torch.float32
    dH = H.new_empty(H.shape if need_dH else (0, H.shape[1]), dtype=f)
    return (dH,) + tuple(p.new_empty(p.shape, dtype=f) for p in (Wv, bv, Wu, bu, wa, ba, wk))


def _setup_context(ctx, inputs, output):
    H, bag_offsets, Wv, bv, Wu, bu, wa, ba, wk, T, p_feat, p_att, seed, bag_id_base, t_base = inputs
    Y, A = output
    ctx.save_for_backward(H, bag_offsets, Wv, bv, Wu, bu, wa, ba, wk, A, Y)
    ctx.scalars = (T, p_feat, p_att, seed, bag_id_base, t_base)
    ctx.set_materialize_grads(False)


def _backward(ctx, dY, dA):
    H, bag_offsets, Wv, bv, Wu, bu, wa, ba, wk, A, Y = ctx.saved_tensors
    T, p_feat, p_att, seed, bag_id_base, t_base = ctx.scalars
    dY = torch.zeros_like(Y) if dY is None else dY.contiguous()
    dA = None if dA is None else dA.contiguous()
    g = torch.ops.mcgmil.mcdo_backward(H, bag_offsets, Wv, bv, Wu, bu, wa, ba, wk, A, Y, dY, dA, T,
                                       p_feat, p_att, seed, bag_id_base, t_base,
                                       bool(ctx.needs_input_grad[0]))
    need = ctx.needs_input_grad
    grads = [g[0] if need[0] else None, None] + [g[i + 1] if need[i + 2] else None for i in range(7)]
    return tuple(grads) + (None,) * 6


mcdo_forward.register_autograd(_backward, setup_context=_setup_context)


@torch.library.custom_op("mcgmil::mcdo_forward_stats", mutates_args=())
def mcdo_forward_stats(H: torch.Tensor, bag_offsets: torch.Tensor, Wv: torch.Tensor,
                       bv: torch.Tensor, Wu: torch.Tensor, bu: torch.Tensor, wa: torch.Tensor,
                       ba: torch.Tensor, wk: torch.Tensor, T: int, p_feat: float, p_att: float,
                       seed: int, bag_id_base: int = 0, t_base: int = 0
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    out = ops.mcdo_forward(H, bag_offsets, _head(Wv, bv, Wu, bu, wa, ba, wk), T, p_feat=p_feat,
                           p_att=p_att, seed=seed & 0xFFFFFFFFFFFFFFFF, bag_id_base=bag_id_base,
                           t_base=t_base, return_attention=False, return_stats=True)
    return out["Y"], out["A_mean"], out["A_var"], out["P_mean"]


@mcdo_forward_stats.register_fake
def _mcdo_forward_stats_fake(H, bag_offsets, Wv, bv, Wu, bu, wa, ba, wk, T, p_feat, p_att, seed,
                             bag_id_base=0, t_base=0):
    B, C, R = bag_offsets.shape[0] - 1, wa.shape[0], H.shape[0]
    f = torch.float32
    return (H.new_empty((B, T, C), dtype=f), H.new_empty((C * R,), dtype=f),
            H.new_empty((C * R,), dtype=f), H.new_empty((B, C), dtype=f))


# ---------------------------------------------------------------- the backbone's training ops
_CL = torch.channels_last


def _channels_last(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous(memory_format=_CL)


def _plain(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.detach().contiguous()


def _or_empty(t: Optional[torch.Tensor], like: torch.Tensor) -> torch.Tensor:
    """A gradient that was not needed comes back as an empty tensor of `like`'s dtype and device."""
    return like.new_empty((0,)) if t is None else t


def _empty_cl(shape, dtype, like: torch.Tensor, need: bool = True) -> torch.Tensor:
    return torch.empty(shape, dtype=dtype, device=like.device, memory_format=_CL) if need else like.new_empty((0,))


def _conv_family(name: str, dtype: torch.dtype, refusal: Callable, forward: str, backward: Callable,
                 cast_dy: bool, dw_dtype: Optional[torch.dtype], nchw_x: bool = False):
    """Register mcgmil::<name> and mcgmil::<name>_backward, a convolution's op of `dtype`.
    refusal(shim, x): why the op does not take them (the ValueError's text), or None; forward: the
    name of the features function; backward(shim, x, dy, need_dx, need_dw) -> (dx | None, dw | None);
    cast_dy: dy is cast to `dtype` first; dw_dtype: the fake dw's dtype (None: the weight's);
    nchw_x: x goes to the features functions in the layout it has (the stem reads NCHW) instead
    of channels-last."""
    def shim(x, weight, stride, pad):
        x = x.detach() if nchw_x else _channels_last(x)
        conv = features._ConvShim(weight, stride, pad)
        why = refusal(conv, x)
        if why is not None:
            raise ValueError(why)
        return conv, x

    @torch.library.custom_op(f"mcgmil::{name}", mutates_args=())
    def op(x: torch.Tensor, weight: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
        # the ambient precision never reaches an op: each forward names its own (conv2d_f32x3's keyword
        # asks for bf16x3 and takes precedence; every other op stays exact fp32)
        with torch.no_grad(), features.float32_conv_precision("fp32"):
            conv, xc = shim(x, weight, stride, pad)
            return getattr(features, forward)(conv, xc)

    @op.register_fake
    def _(x, weight, stride, pad):
        oh, ow = ((x.shape[i] + 2 * pad - weight.shape[i]) // stride + 1 for i in (2, 3))
        return _empty_cl((x.shape[0], weight.shape[0], oh, ow), dtype, x)

    @torch.library.custom_op(f"mcgmil::{name}_backward", mutates_args=())
    def op_backward(x: torch.Tensor, weight: torch.Tensor, dy: torch.Tensor, stride: int, pad: int,
                    need_dx: bool, need_dw: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        with torch.no_grad(), features.float32_conv_precision("fp32"):
            conv, xc = shim(x, weight, stride, pad)
            dy = dy.detach()
            dx, dw = backward(conv, xc, dy.to(dtype) if cast_dy else dy, need_dx, need_dw)
        return _or_empty(dx if need_dx else None, x), _or_empty(dw if need_dw else None, weight)

    @op_backward.register_fake
    def _(x, weight, dy, stride, pad, need_dx, need_dw):
        dw = weight.new_empty(weight.shape, dtype=dw_dtype) if need_dw else weight.new_empty((0,))
        return _empty_cl(x.shape, dtype, x, need_dx), dw

    def setup_context(ctx, inputs, output):
        x, weight, stride, pad = inputs
        ctx.save_for_backward(x, weight)
        ctx.geometry = (stride, pad)

    def formula(ctx, dy):
        x, weight = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx, dw = getattr(torch.ops.mcgmil, name + "_backward")(x, weight, dy, *ctx.geometry, need_dx, need_dw)
        return dx if need_dx else None, dw if need_dw else None, None, None

    op.register_autograd(formula, setup_context=setup_context)
    return op, op_backward


def _conv32_refusal(conv, x):
    if not features.conv32_trainable(conv, x):
        return ("mcgmil::conv2d_f32 needs a CUDA fp32 activation and weight with kernel 1..7, "
                "stride 1 or 2, pad < kernel, in_channels % 16 == 0 and out_channels % 64 == 0 "
                "(features.conv32_trainable)")


def _named_refusal(name: str, reason: str, trainable: str) -> Callable:
    def refusal(conv, x):
        why = getattr(features, reason)(conv, x)
        return None if why is None else f"mcgmil::{name}: {why} (features.{trainable})"
    return refusal


def _stem_conv_grads(conv, x, dy, need_dx, need_dw):
    dy = dy.contiguous(memory_format=_CL)
    dw = features.conv2d_f32_stem_wgrad(conv, x, dy) if need_dw else None
    # no native data gradient: the model never asks for one (the instances do not require grad)
    dx = features._aten_conv_backward(conv, x, dy, True, False)[0] if need_dx else None
    return dx, dw


conv2d_f32, conv2d_f32_backward = _conv_family(
    "conv2d_f32", torch.float32, _conv32_refusal, "conv2d_f32",
    lambda *a: features.conv2d_f32_backward(*a), cast_dy=False, dw_dtype=torch.float32)
stem_conv_f32, stem_conv_f32_backward = _conv_family(
    "stem_conv_f32", torch.float32, _named_refusal("stem_conv_f32", "stem_conv_untrainable_reason", "stem_conv_trainable"),
    "conv2d_f32", _stem_conv_grads, cast_dy=False, dw_dtype=torch.float32)
conv2d_bf16, conv2d_bf16_backward = _conv_family(
    "conv2d_bf16", torch.bfloat16, _named_refusal("conv2d_bf16", "conv_bf16_untrainable_reason", "conv_bf16_trainable"),
    "conv2d_bf16", lambda *a: features.conv2d_bf16_backward(*a), cast_dy=True, dw_dtype=None)


def _stem_conv_bf16_grads(conv, x, dy, need_dx, need_dw):
    dy = dy.contiguous(memory_format=_CL)
    dw = features.stem_conv_bf16_wgrad(conv, x, dy).to(conv.weight.dtype) if need_dw else None
    dx = None
    if need_dx:     # no native data gradient: the model never asks for one (the instances do not require grad)
        dx = features._aten_conv_backward_bf16(conv, x.to(torch.bfloat16).contiguous(memory_format=_CL), dy, True, False)[0]
    return dx, dw


# The bf16 stem convolution's ops. They are not in __all__: tests/fixtures/features_bindings.json
# records __all__ as the op list of the merged fp32 / bf16 twins, and this op has no fp32 twin of
# the same shape (stem_conv_f32 reads channels-last fp32, this one NCHW).
STEM_BF16_OPS = ("stem_conv_bf16", "stem_conv_bf16_backward")
stem_conv_bf16, stem_conv_bf16_backward = _conv_family(
    "stem_conv_bf16", torch.bfloat16,
    _named_refusal("stem_conv_bf16", "stem_conv_bf16_untrainable_reason", "stem_conv_bf16_trainable"),
    "stem_conv_bf16", _stem_conv_bf16_grads, cast_dy=True, dw_dtype=None, nchw_x=True)


# The bf16x3 convolution's ops. Not in __all__ either: tests/fixtures/features_bindings.json records
# __all__ and every schema of the merged twins.
CONV_X3_OPS = ("conv2d_f32x3", "conv2d_f32x3_backward")
conv2d_f32x3, conv2d_f32x3_backward = _conv_family(
    "conv2d_f32x3", torch.float32, _named_refusal("conv2d_f32x3", "conv32x3_untrainable_reason", "conv32x3_trainable"),
    "conv2d_f32x3", lambda *a: features.conv2d_f32x3_backward(*a), cast_dy=False, dw_dtype=torch.float32)


def _bn_act_family(name: str, dtype: torch.dtype, forward: str, backward: str, mixed: bool):
    """Register mcgmil::<name> and mcgmil::<name>_backward, the fused BatchNorm (+ add) (+ ReLU)
    of `dtype`. forward, backward: the names of the features functions; mixed: the bf16 twin,
    whose dy is cast to `dtype` first and whose placeholders for dweight and dbias (fp32) take
    their dtype from mean; those for dx and dres, and all of the fp32 op's, take it from x."""
    @torch.library.custom_op(f"mcgmil::{name}", mutates_args=())
    def op(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
           residual: Optional[torch.Tensor], eps: float, relu: bool
           ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        with torch.no_grad():
            return getattr(features, forward)(_channels_last(x), _plain(weight), _plain(bias),
                                              None if residual is None else _channels_last(residual), eps, relu)

    @op.register_fake
    def _(x, weight, bias, residual, eps, relu):
        return (_empty_cl(x.shape, dtype, x), x.new_empty((x.shape[1],), dtype=torch.float32),
                x.new_empty((x.shape[1],), dtype=torch.float32))

    @torch.library.custom_op(f"mcgmil::{name}_backward", mutates_args=())
    def op_backward(x: torch.Tensor, y: torch.Tensor, dy: torch.Tensor, weight: Optional[torch.Tensor],
                    mean: torch.Tensor, invstd: torch.Tensor, relu: bool, need_dx: bool, need_dres: bool,
                    need_dw: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        with torch.no_grad():
            dx, dres, dw, db = getattr(features, backward)(
                _channels_last(x), _channels_last(y) if relu else None, _channels_last(dy.to(dtype) if mixed else dy),
                _plain(weight), _plain(mean), _plain(invstd), relu, need_dx, need_dres, need_dw)
        return _or_empty(dx, x), _or_empty(dres, x), _or_empty(dw, mean if mixed else x), _or_empty(db, mean if mixed else x)

    @op_backward.register_fake
    def _(x, y, dy, weight, mean, invstd, relu, need_dx, need_dres, need_dw):
        vec = lambda: (mean if mixed else x).new_empty((x.shape[1],) if need_dw else (0,), dtype=torch.float32)  # noqa: E731
        return _empty_cl(x.shape, dtype, x, need_dx), _empty_cl(x.shape, dtype, x, need_dres and relu), vec(), vec()

    def setup_context(ctx, inputs, output):
        x, weight, bias, residual, eps, relu = inputs
        y, mean, invstd = output
        ctx.relu, ctx.has_weight = relu, weight is not None
        # y is needed for the ReLU mask only
        ctx.save_for_backward(x, mean, invstd, *((weight,) if weight is not None else ()), *((y,) if relu else ()))
        ctx.set_materialize_grads(False)

    def formula(ctx, dy, dmean, dinvstd):
        # dmean / dinvstd: mean and invstd are by-products for the backward, not differentiable outputs
        if dy is None:
            return (None,) * 6
        x, mean, invstd, *rest = ctx.saved_tensors
        weight = rest.pop(0) if ctx.has_weight else None
        y = rest.pop(0) if ctx.relu else x.new_empty((0,))
        need = ctx.needs_input_grad
        need_dx, need_dw, need_dres = need[0], need[1] or need[2], need[3]
        dx, dres, dw, db = getattr(torch.ops.mcgmil, name + "_backward")(
            x, y, dy, weight, mean, invstd, ctx.relu, need_dx, need_dres and ctx.relu, need_dw)
        if need_dres and not ctx.relu:
            dres = dy
        return (dx if need_dx else None, dw if need[1] else None, db if need[2] else None,
                dres if need_dres else None, None, None)

    op.register_autograd(formula, setup_context=setup_context)
    return op, op_backward


bn_act_f32, bn_act_f32_backward = _bn_act_family(
    "bn_act_f32", torch.float32, "batchnorm_act_stats", "batchnorm_act_backward", mixed=False)
bn_act_bf16, bn_act_bf16_backward = _bn_act_family(
    "bn_act_bf16", torch.bfloat16, "batchnorm_act_stats_bf16", "batchnorm_act_backward_bf16", mixed=True)


def _bn_pool_family(name: str, dtype: torch.dtype, forward: str, backward: str, mixed: bool):
    """Register mcgmil::<name> and mcgmil::<name>_backward, the stem's fused BatchNorm (+ ReLU) +
    max-pool of `dtype`; the arguments as _bn_act_family's. The placeholder for dz takes its dtype
    from z."""
    @torch.library.custom_op(f"mcgmil::{name}", mutates_args=())
    def op(z: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float,
           relu: bool, k: int, stride: int, pad: int
           ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        with torch.no_grad():
            return getattr(features, forward)(_channels_last(z), _plain(weight), _plain(bias), eps, relu, k, stride, pad)

    @op.register_fake
    def _(z, weight, bias, eps, relu, k, stride, pad):
        shape = (z.shape[0], z.shape[1], (z.shape[2] + 2 * pad - k) // stride + 1, (z.shape[3] + 2 * pad - k) // stride + 1)
        return (_empty_cl(shape, dtype, z), z.new_empty((z.shape[1],), dtype=torch.float32),
                z.new_empty((z.shape[1],), dtype=torch.float32), _empty_cl(shape, torch.uint8, z))

    @torch.library.custom_op(f"mcgmil::{name}_backward", mutates_args=())
    def op_backward(z: torch.Tensor, argmax: torch.Tensor, dy: torch.Tensor, weight: Optional[torch.Tensor],
                    mean: torch.Tensor, invstd: torch.Tensor, k: int, stride: int, pad: int, need_dz: bool,
                    need_dw: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        with torch.no_grad():
            dz, dw, db = getattr(features, backward)(
                _channels_last(z), _channels_last(argmax), _channels_last(dy.to(dtype) if mixed else dy),
                _plain(weight), _plain(mean), _plain(invstd), k, stride, pad, need_dz, need_dw)
        return _or_empty(dz, z), _or_empty(dw, mean if mixed else z), _or_empty(db, mean if mixed else z)

    @op_backward.register_fake
    def _(z, argmax, dy, weight, mean, invstd, k, stride, pad, need_dz, need_dw):
        vec = lambda: (mean if mixed else z).new_empty((z.shape[1],) if need_dw else (0,), dtype=torch.float32)  # noqa: E731
        return _empty_cl(z.shape, dtype, z, need_dz), vec(), vec()

    def setup_context(ctx, inputs, output):
        z, weight, bias, eps, relu, k, stride, pad = inputs
        y, mean, invstd, argmax = output
        ctx.geometry, ctx.has_weight = (k, stride, pad), weight is not None
        # neither y nor the activation: the codes say where each pooled gradient goes
        ctx.save_for_backward(z, argmax, mean, invstd, *((weight,) if weight is not None else ()))
        ctx.set_materialize_grads(False)

    def formula(ctx, dy, dmean, dinvstd, dargmax):
        # dmean / dinvstd / dargmax: by-products for the backward, not differentiable outputs
        if dy is None:
            return (None,) * 8
        z, argmax, mean, invstd, *rest = ctx.saved_tensors
        weight = rest[0] if ctx.has_weight else None
        need = ctx.needs_input_grad
        need_dz, need_dw = need[0], need[1] or need[2]
        dz, dw, db = getattr(torch.ops.mcgmil, name + "_backward")(z, argmax, dy, weight, mean, invstd, *ctx.geometry,
                                                                  need_dz, need_dw)
        return (dz if need_dz else None, dw if need[1] else None, db if need[2] else None) + (None,) * 5

    op.register_autograd(formula, setup_context=setup_context)
    return op, op_backward


bn_pool_f32, bn_pool_f32_backward = _bn_pool_family(
    "bn_pool_f32", torch.float32, "batchnorm_pool_stats", "batchnorm_pool_backward", mixed=False)
bn_pool_bf16, bn_pool_bf16_backward = _bn_pool_family(
    "bn_pool_bf16", torch.bfloat16, "batchnorm_pool_stats_bf16", "batchnorm_pool_backward_bf16", mixed=True)
