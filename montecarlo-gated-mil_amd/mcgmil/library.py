"""torch.library registration of the MCDO head ("register it with
torch.library.custom_op so it composes with torch.compile / autograd-free inference").

    torch.ops.mcgmil.mcdo_forward(H, bag_offsets, Wv, bv, Wu, bu, wa, ba, wk, T, p_feat, p_att,
                                  seed, bag_id_base=0, t_base=0) -> (Y [B, T, C], A [T*C*R])
    torch.ops.mcgmil.mcdo_forward_stats(...same...) -> (Y, A_mean [C*R], A_var [C*R], P_mean [B, C])
    torch.ops.mcgmil.mcdo_backward(H, bag_offsets, Wv, ..., wk, A, Y, dY, dA, T, p_feat, p_att, seed,
                                   bag_id_base=0, t_base=0, need_dH=True)
                                  -> (dH [R, L] or [0, L], dWv, dbv, dWu, dbu, dwa, dba, dwk)

mcdo_forward is differentiable in H and the seven parameter tensors: its autograd formula
(register_autograd, the only autograd mechanism of the package) calls mcdo_backward, which draws
the dropout masks again from the seed instead of saving them. mcdo_backward itself has no
autograd formula, so a backward of the backward raises.

Same semantics as `mcgmil.ops.mcdo_forward` (reference model.py:256-328 for every bag of the
batch, bags as CSR row ranges of H). The ops are opaque to a graph capture: the fake (meta)
implementations below only derive output shapes, and the real ones run the gfx950 kernels
through the C ABI. There is no CPU kernel: called with CPU tensors they raise. `seed` is the
64-bit Philox key as a signed int64 (the schema's int); it is reinterpreted as unsigned.
"""
from typing import Optional, Tuple

import torch

from . import ops

__all__ = ["mcdo_forward", "mcdo_forward_stats", "mcdo_backward"]


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
