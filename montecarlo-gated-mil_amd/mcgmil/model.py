"""Drop-in MultiHeadGatedAttentionMIL whose MCDO inference path runs on the gfx950 kernels.

Mirrors the reference module xkuubix/MonteCarlo-Gated-MIL model.py:134-401:
  - same constructor keywords and defaults (model.py:135-145),
  - same submodule / parameter names and shapes, so reference checkpoints load with
    load_state_dict(strict=True) (model.py:165-209),
  - same methods and return shapes: forward (211-253), mc_inference (256-328),
    mc_inference_serial (330-401).
What differs, by design:
  - the dropout masks come from the MI355X Philox stream (oracle/philox_oracle.c documents it)
    instead of torch's global RNG; `seed=None` draws the Philox key from torch's default CPU
    generator, so torch.manual_seed(...) still makes a run reproducible (infer.py:137-145);
  - mc_inference and mc_inference_serial give identical samples for the same seed (the
    reference's two methods consume its RNG in different orders);
  - the head runs only on a HIP device. Training (net_utils.py train_gacc, main.py,
    cross_validation.py) is opt-in: after enable_head_training(), forward() in train mode runs the
    backbone under torch autograd and the head through the differentiable op
    torch.ops.mcgmil.mcdo_forward, whose HIP backward (include/mcgmil_grad.h) draws the dropout
    masks again instead of storing them. enable_backbone_training() on top of it moves the
    backbone's block convolutions from the torch layers to the differentiable fp32 HIP op
    (torch.ops.mcgmil.conv2d_f32; include/mcgmil_conv_grad.h is its native backward), and with
    norm=True the blocks' BatchNorm / residual add / ReLU to the fused HIP op
    (torch.ops.mcgmil.bn_act_f32; include/mcgmil_bn_grad.h is its backward), and with stem=True
    the stem's BatchNorm / ReLU / max-pool to torch.ops.mcgmil.bn_pool_f32
    (include/mcgmil_pool_grad.h), and with stem_conv=True the 7x7 stem convolution to
    torch.ops.mcgmil.stem_conv_f32 (include/mcgmil_stem_grad.h is its weight gradient).
    enable_bf16x3_backbone_training() on top of enable_backbone_training() sends the block
    convolutions to torch.ops.mcgmil.conv2d_f32x3 instead: fp32 storage, the GEMMs on three bf16 MFMA
    products per K (include/mcgmil_conv_grad_x3.h is its weight gradient). Without the opt-in, forward() in train mode raises instead of
    silently running elsewhere.
Extra entries: mc_inference_features(H, T, seed, ...) starts at the kernel boundary (features);
forward_features(H, T, seed) is its differentiable form.
"""
import contextlib

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import features, ops
from .resnet import Identity, build_backbone

__all__ = ["MultiHeadGatedAttentionMIL", "AuxiliaryLoss"]


class AuxiliaryLoss(nn.Module):
    """Attention-head separation regulariser (reference model.py:405-438; training only)."""

    def __init__(self, loss_type="pairwise", margin=1.0, scale=1.0):
        super().__init__()
        self.loss_type = loss_type
        self.margin = margin
        self.scale = scale

    def forward(self, pos_attention, neg_attention, is_positive):
        if self.loss_type == "pairwise":
            d = F.pairwise_distance(pos_attention, neg_attention, p=2)
            return torch.mean((self.margin - d).clamp(min=0)) if is_positive else torch.mean(d)
        if self.loss_type == "cosine":
            cs = F.cosine_similarity(pos_attention, neg_attention, dim=1)
            return torch.mean(cs) if is_positive else torch.mean(1 - cs)
        raise ValueError(f"Unknown loss type: {self.loss_type}")


def _walk(root, path):
    """root._modules[path[0]]._modules[path[1]]... (KeyError if a link is gone)."""
    m = root
    for k in path:
        m = m._modules[k]
    return m


def _draw_seed() -> int:
    # key for the Philox stream, taken from torch's default CPU generator
    return int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())


class MultiHeadGatedAttentionMIL(nn.Module):
    def __init__(self, num_classes=2, backbone="r18", pretrained=True, L=512, D=128,
                 feature_dropout=0.1, attention_dropout=0.1, shared_attention=True,
                 neptune_run=None):
        super().__init__()
        self.auxiliary_loss = AuxiliaryLoss(loss_type="pairwise", margin=1.0, scale=.5)
        self.fold_idx = None
        self.neptune_run = neptune_run if neptune_run else None
        self.L = L
        self.D = D
        self.num_classes = num_classes
        self.shared_attention = shared_attention
        # reference model.py:166-177: without `pretrained` the reference always builds r18
        self.feature_extractor = build_backbone(backbone if pretrained else "r18", pretrained)
        self.feature_extractor.fc = Identity()
        if shared_attention:
            self.attention_V = nn.Sequential(nn.Linear(L, D), nn.Tanh())
            self.attention_U = nn.Sequential(nn.Linear(L, D), nn.Sigmoid())
        else:
            self.attention_V = nn.ModuleList([nn.Sequential(nn.Linear(L, D), nn.Tanh())
                                              for _ in range(num_classes)])
            self.attention_U = nn.ModuleList([nn.Sequential(nn.Linear(L, D), nn.Sigmoid())
                                              for _ in range(num_classes)])
        self.attention_weights = nn.ModuleList([nn.Linear(D, 1) for _ in range(num_classes)])
        self.classifiers = nn.ModuleList([nn.Linear(L, 1, bias=False) for _ in range(num_classes)])
        self.feature_dropout = nn.Dropout(feature_dropout)
        self.attention_dropouts = nn.ModuleList([nn.Dropout(attention_dropout)
                                                 for _ in range(num_classes)])
        # GEMM operand precision of the kernel: float32 (reference numerics) or bfloat16
        self.compute_dtype = torch.float32
        # precision of the backbone's fp32 block convolutions: "fp32" (reference numerics) or "bf16x3"
        self._feature_precision = "fp32"
        self._head_cache = None
        self._head_training = False
        self._backbone_training = False
        self._norm_training = False
        self._stem_training = False
        self._stem_conv_training = False
        self._bf16x3_backbone_training = False
        self._bf16_backbone_training = False
        self._bf16_norm_training = False
        self._bf16_stem_training = False
        self._bf16_stem_conv_training = False

    # ------------------------------------------------------------------ parameters
    def _gate_linears(self):
        if self.shared_attention:
            return [self.attention_V[0]], [self.attention_U[0]]
        return [m[0] for m in self.attention_V], [m[0] for m in self.attention_U]

    def _head_slots(self):
        """(module, parameter name) of every head parameter, in kernel order."""
        lv, lu = self._gate_linears()
        slots = [(m, n) for m in lv + lu for n in ("weight", "bias")]
        slots += [(m, n) for m in self.attention_weights for n in ("weight", "bias")]
        slots += [(m, "weight") for m in self.classifiers]
        return slots

    def _head_params(self):
        """The head's parameters in kernel order. The list is cached (the per-bag caller of
        infer.py:187-191 would otherwise walk nn.Module attribute lookups on every call) and
        revalidated on every call by identity, with plain dict lookups: every module on the path
        from self to each parameter's owner, and the Parameter object in its owner's _parameters.
        So replacing a Linear inside a container, assigning a new Parameter, or
        load_state_dict(..., assign=True) all miss the cache; the cache holds the objects it
        compares against, so an id cannot be reused while it is alive."""
        hit = self.__dict__.get("_head_param_cache")
        if hit is not None and self.shared_attention == hit[0]:
            chains, slots, params = hit[1:]
            try:
                ok = all(_walk(self, path) is m for path, m in chains) and \
                    all(m._parameters.get(n) is p for (m, n), p in zip(slots, params))
            except KeyError:
                ok = False
            if ok:
                return params
        slots = self._head_slots()
        params = [m._parameters[n] for m, n in slots]
        names = {id(m): name for name, m in self.named_modules()}
        owners = {id(m): m for m, _ in slots}
        chains = [(tuple(names[i].split(".")), m) for i, m in owners.items()]
        self.__dict__["_head_param_cache"] = (self.shared_attention, chains, slots, params)
        return params

    def head_tensors(self, device) -> ops.HeadTensors:
        """The head parameters stacked for the kernel (cached until a parameter changes)."""
        params = self._head_params()
        key = (str(device), self.compute_dtype,
               tuple((p.data_ptr(), p._version) for p in params))
        if self._head_cache is not None and self._head_cache[0] == key:
            return self._head_cache[1], self._head_cache[2]
        lv, lu = self._gate_linears()
        with torch.no_grad():
            f32 = dict(device=device, dtype=torch.float32)
            head = ops.HeadTensors(
                Wv=torch.stack([m.weight for m in lv]).to(**f32).contiguous(),
                bv=torch.stack([m.bias for m in lv]).to(**f32).contiguous(),
                Wu=torch.stack([m.weight for m in lu]).to(**f32).contiguous(),
                bu=torch.stack([m.bias for m in lu]).to(**f32).contiguous(),
                wa=torch.cat([m.weight for m in self.attention_weights]).to(**f32).contiguous(),
                ba=torch.cat([m.bias for m in self.attention_weights]).to(**f32).contiguous(),
                wk=torch.cat([m.weight for m in self.classifiers]).to(**f32).contiguous())
            packed = ops.packed_weights(head, self.compute_dtype)
        self._head_cache = (key, head, packed)
        return head, packed

    def _dropout_ps(self):
        """Active dropout probabilities: a layer applies dropout iff it is in train mode."""
        pf = self.feature_dropout.p if self.feature_dropout.training else 0.0
        pas = {d.p if d.training else 0.0 for d in self.attention_dropouts}
        if len(pas) != 1:
            raise NotImplementedError("per-class attention dropout rates / modes must agree")
        return pf, pas.pop()

    def _check_device(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("the MI355X MCDO head runs on a HIP device only "
                               f"(got device={device}); there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return device

    def _offsets(self, n, bs, device):
        """CSR offsets of bs bags of n instances, made on the device once per shape (infer.py:187-191
        calls mc_inference once per bag: no per-call host->device copy or allocation)."""
        key = (str(device), n, bs)
        cache = self.__dict__.setdefault("_offs_cache", {})
        t = cache.get(key)
        if t is None:
            if len(cache) > 64:
                cache.clear()
            t = cache[key] = ops.uniform_offsets(n, bs, device) if n > 0 else \
                ops.bag_offsets_tensor([0] * bs, device)
        return t

    # ------------------------------------------------------------------ kernel boundary
    @property
    def feature_precision(self) -> str:
        """How extract_features runs the backbone's fp32 block convolutions on fp32 instances:
        "fp32" (the default: exact fp32 MFMA, the reference precision) or "bf16x3" (fp32 storage,
        three bf16 MFMA products per K; features.float32_conv_precision). The stem, the head
        (compute_dtype) and every differentiable op are not affected. With "fp32" the ambient
        setting (MCGMIL_CONV32_PRECISION) is left as it is."""
        return self._feature_precision

    @feature_precision.setter
    def feature_precision(self, value: str) -> None:
        self._feature_precision = features._check_precision(value)

    def extract_features(self, x):
        """x [bs, n, 3, h, w] -> H [bs, n, L] (reference model.py:275-277)."""
        bs, n = x.shape[:2]
        ctx = features.float32_conv_precision("bf16x3") if self._feature_precision == "bf16x3" \
            else contextlib.nullcontext()
        with ctx:
            H = self.feature_extractor(x.view(-1, *x.shape[-3:]))
        return H.view(bs, n, -1)

    @torch.no_grad()
    def mc_inference_features(self, H, T=30, seed=None, *, p_feat=None, p_att=None,
                              return_stats=False, bag_id_base=0, t_base=0):
        """MCDO over extracted features: H [n, L] or [bs, n, L] -> (Y [T, bs, C], A [T, bs, C, n])
        plus, with return_stats, a dict of A_mean/A_var [bs, C, n] and P_mean [bs, C]."""
        if H.dim() == 2:
            H = H.unsqueeze(0)
        device = self._check_device(H.device)
        bs, n, L = H.shape
        if seed is None:
            seed = _draw_seed()
        pf = self.feature_dropout.p if p_feat is None else p_feat
        pa = self.attention_dropouts[0].p if p_att is None else p_att
        head, packed = self.head_tensors(device)
        Hc = H.reshape(bs * n, L).to(self.compute_dtype).contiguous()
        offs = self._offsets(n, bs, device)
        out = ops.mcdo_forward(Hc, offs, head, T, p_feat=pf, p_att=pa, seed=seed,
                               bag_id_base=bag_id_base, t_base=t_base, packed=packed,
                               return_attention=True, return_stats=return_stats)
        C = self.num_classes
        Y = out["Y"].permute(1, 0, 2)                                   # [T, bs, C]
        A = out["A"].view(bs, T, C, n).permute(1, 0, 2, 3)              # [T, bs, C, n]
        if not return_stats:
            return Y, A
        stats = {"A_mean": out["A_mean"].view(bs, C, n), "A_var": out["A_var"].view(bs, C, n),
                 "P_mean": out["P_mean"]}
        return Y, A, stats

    # ------------------------------------------------------------------ training (opt-in)
    def enable_head_training(self, flag=True):
        """Let forward() in train mode build an autograd graph: backbone under torch autograd, head
        through the differentiable HIP op (fp32). Off by default; returns self."""
        self._head_training = bool(flag)
        return self

    def enable_backbone_training(self, flag=True, *, norm=False, stem=False, stem_conv=False):
        """With enable_head_training(): forward() in train mode runs the backbone's block
        convolutions (every features.conv32_trainable one: all but the 3-channel stem) through
        the differentiable op torch.ops.mcgmil.conv2d_f32 instead of the torch layer: the fp32
        MFMA forward kernel, and for the backward the route features.conv_grad_route() names
        (MCGMIL_CONV_GRAD=native: the HIP weight gradient and the forward kernel again as the
        stride-1 data gradient; MCGMIL_CONV_GRAD=direct: the HIP weight gradient and the direct
        HIP data gradient of include/mcgmil_conv_dgrad.h for stride 1 and 2, so that no gradient
        of these convolutions leaves the project's kernels; default: aten.convolution_backward,
        whose step measured fastest). The stem, BatchNorm, ReLU, the pools and the
        residual add stay on the torch layers, unless norm=True: then every pool-free
        features.bn_trainable BatchNorm of the blocks (fp32, batch statistics, no running-statistics
        update pending), with the residual add and ReLU that follow it, runs through the
        differentiable op torch.ops.mcgmil.bn_act_f32 as well: the fused HIP forward and the HIP
        backward of include/mcgmil_bn_grad.h instead of torch's batch_norm / add / relu kernels and
        their backward (timings in DESIGN.md §4). The stem (conv1 / bn1 / relu / maxpool) stays on
        torch, unless stem=True: then the stem's BatchNorm / ReLU / max-pool, when
        features.bn_pool_trainable, run through the differentiable op torch.ops.mcgmil.bn_pool_f32:
        the fused HIP forward, which keeps one byte per pooled element instead of the ReLU output
        and the pool's int64 indices, and the HIP backward of include/mcgmil_pool_grad.h (timings
        in DESIGN.md §4). stem does not depend on norm; it only needs the flag itself. The 7x7
        convolution stays on the torch layer (features.conv32_trainable refuses 3 input
        channels), unless stem_conv=True: then it runs, when features.stem_conv_trainable, through
        the differentiable op torch.ops.mcgmil.stem_conv_f32: the gather-mode fp32 HIP forward
        kernel the inference path uses, and the HIP weight gradient of include/mcgmil_stem_grad.h
        (no data gradient: the instances do not require grad), instead of MIOpen in batch chunks
        and a torch.cat (timings in DESIGN.md §4). stem_conv depends on neither norm nor stem; it
        only needs the flag itself. Off by default, norm, stem and stem_conv off by default;
        returns self."""
        self._backbone_training = bool(flag)
        self._norm_training = bool(flag) and bool(norm)
        self._stem_training = bool(flag) and bool(stem)
        self._stem_conv_training = bool(flag) and bool(stem_conv)
        return self

    def enable_bf16x3_backbone_training(self, flag=True):
        """On top of enable_head_training() and enable_backbone_training(), and in effect only while
        both are on: forward() in train mode sends the block convolutions (every
        features.conv32x3_trainable one: conv32_trainable with in_channels a multiple of 32, all 19
        of ResNet-18 but the 3-channel stem) through the differentiable op
        torch.ops.mcgmil.conv2d_f32x3 instead of torch.ops.mcgmil.conv2d_f32. Activations, weights
        and gradients stay fp32 -- no autocast, no bf16 tensors -- and the GEMMs of the forward, the
        weight gradient (include/mcgmil_conv_grad_x3.h) and the stride-1 data gradient run as three
        bf16 MFMA products per K ("bf16x3", the precision of feature_precision = "bf16x3"); the
        stride-2 data gradient is the exact fp32 direct kernel of include/mcgmil_conv_dgrad.h.
        MCGMIL_CONV_GRAD is not read: no gradient of a routed convolution leaves the project's
        kernels, and the step repeats bitwise. It composes with enable_backbone_training's norm,
        stem and stem_conv keywords (fp32-storage ops all); under enable_bf16_backbone_training()
        the predicate refuses (autocast) and the bf16 ops run. feature_precision stays
        inference-only; eval mode, no_grad and the default are unchanged. A method of its own, so
        that the existing signatures stay. Off by default; returns self (timings and parity in
        DESIGN.md §4)."""
        self._bf16x3_backbone_training = bool(flag)
        return self

    def enable_bf16_backbone_training(self, flag=True):
        """With enable_head_training(): forward() in train mode runs the backbone in mixed
        precision, under torch.autocast("cuda", torch.bfloat16), and sends the block convolutions
        (every features.conv_bf16_trainable one: all 19 of ResNet-18 but the 3-channel stem)
        through the differentiable op torch.ops.mcgmil.conv2d_bf16 instead of the torch layer: the
        bf16 MFMA forward kernel of the inference path, and for the backward the route
        MCGMIL_CONV_GRAD names (native or direct: the bf16 HIP weight gradient of
        include/mcgmil_conv_grad_bf16.h, written in fp32 into the fp32 master weight's .grad, and
        the forward kernel again as the stride-1 data gradient; the stride-2 data gradient is
        aten's on native and the direct bf16 HIP kernel of include/mcgmil_conv_dgrad_bf16.h on
        direct, so that on direct no gradient of a routed convolution leaves the project's kernels
        and the step repeats bitwise; default: aten.convolution_backward on bf16 tensors). The fp32 opt-ins of enable_backbone_training decline under autocast layer
        by layer, so the stem convolution, BatchNorm, ReLU and the pools are the torch layers under
        autocast, unless enable_bf16_norm_training() (the blocks' BatchNorms),
        enable_bf16_stem_training() (the stem's bn1 / relu / maxpool) or
        enable_bf16_stem_conv_training() (the stem convolution) is on as well. The head stays
        fp32. Eval mode, no_grad and the default are unchanged. Off by default; switching it off
        switches enable_bf16_norm_training, enable_bf16_stem_training and
        enable_bf16_stem_conv_training off too; returns self."""
        self._bf16_backbone_training = bool(flag)
        if not flag:
            self._bf16_norm_training = False
            self._bf16_stem_training = False
            self._bf16_stem_conv_training = False
        return self

    def enable_bf16_norm_training(self, flag=True):
        """On top of enable_bf16_backbone_training(), and in effect only while that is on: forward()
        in train mode additionally sends every pool-free features.bn_bf16_trainable BatchNorm of
        the blocks (a bf16 activation, fp32 parameters, batch statistics, no running-statistics
        update pending: the 19 of ResNet-18, 16 in blocks and 3 downsample), with the residual add
        and ReLU that follow it, through the differentiable op torch.ops.mcgmil.bn_act_bf16: the
        fused bf16 HIP forward and the HIP backward of include/mcgmil_bn_grad_bf16.h instead of
        torch's batch_norm / add / relu kernels and their backward (timings in DESIGN.md §4). It
        does not depend on MCGMIL_CONV_GRAD. The stem's bn1 / relu / maxpool (unless
        enable_bf16_stem_training() is on), the stem convolution (unless
        enable_bf16_stem_conv_training() is on) and the head stay as they are. A
        method of its own, so that enable_bf16_backbone_training keeps its signature. Off by
        default; enable_bf16_backbone_training(False) switches it off; returns self."""
        self._bf16_norm_training = bool(flag)
        return self

    def enable_bf16_stem_training(self, flag=True):
        """On top of enable_bf16_backbone_training(), and in effect only while that is on: forward()
        in train mode additionally sends the stem's bn1 / relu / maxpool, when
        features.bn_pool_bf16_trainable (a bf16 activation, fp32 parameters, batch statistics, no
        running-statistics update pending, a 2- or 3-wide pool), through the differentiable op
        torch.ops.mcgmil.bn_pool_bf16: the fused bf16 HIP forward, which keeps one byte per pooled
        element instead of a full-size bf16 BatchNorm/ReLU output and the pool's int64 indices, and
        the HIP backward of include/mcgmil_pool_grad_bf16.h, instead of torch's batch_norm / relu /
        max_pool2d kernels under autocast and their backward (timings in DESIGN.md §4). Where two
        taps of a window round to the same bf16 value the gradient goes to the one whose unrounded
        value is larger, not to the first as under torch (include/mcgmil_pool_grad_bf16.h). It
        depends on neither enable_bf16_norm_training() nor MCGMIL_CONV_GRAD. The stem convolution
        stays the torch layer under autocast (unless enable_bf16_stem_conv_training() is on). A method
        of its own, so that the existing signatures
        stay. Off by default; enable_bf16_backbone_training(False) switches it off; returns self."""
        self._bf16_stem_training = bool(flag)
        return self

    def enable_bf16_stem_conv_training(self, flag=True):
        """On top of enable_bf16_backbone_training(), and in effect only while that is on: forward()
        in train mode additionally sends the stem convolution conv1, when
        features.stem_conv_bf16_trainable (the NCHW instances with 1..4 channels, a bias-free
        stride-2 Conv2d(C, 64, k) with k + (pad & 1) <= 8, an even width, OW <= 125), through the
        differentiable op torch.ops.mcgmil.stem_conv_bf16: the inference stem's bf16 MFMA kernel
        straight from the NCHW instances (no channels-last copy of x, no batch chunks, no
        torch.cat of the output) and the bf16 HIP weight gradient of
        include/mcgmil_stem_grad_bf16.h, written in fp32 into the fp32 master weight's .grad and
        bitwise repeatable, instead of the torch layer under autocast and
        aten.convolution_backward (timings in DESIGN.md §4). It depends on neither
        enable_bf16_norm_training() nor enable_bf16_stem_training() nor MCGMIL_CONV_GRAD. A method
        of its own, so that the existing signatures stay. Off by default;
        enable_bf16_backbone_training(False) switches it off; returns self."""
        self._bf16_stem_conv_training = bool(flag)
        return self

    def _live_head(self):
        """The head parameters stacked for the kernel WITH their autograd history."""
        lv, lu = self._gate_linears()
        return (torch.stack([m.weight for m in lv]), torch.stack([m.bias for m in lv]),
                torch.stack([m.weight for m in lu]), torch.stack([m.bias for m in lu]),
                torch.cat([m.weight for m in self.attention_weights]),
                torch.cat([m.bias for m in self.attention_weights]),
                torch.cat([m.weight for m in self.classifiers]))

    def forward_features(self, H, T=1, seed=None, *, p_feat=None, p_att=None, bag_id_base=0,
                         t_base=0):
        """mc_inference_features with a graph: H [n, L] or [bs, n, L] -> (Y [T, bs, C],
        A [T, bs, C, n]), differentiable in H and the head parameters (fp32 only). The dropout
        rates default to the active ones (_dropout_ps)."""
        from . import library  # noqa: F401  (registers torch.ops.mcgmil.*)
        if H.dim() == 2:
            H = H.unsqueeze(0)
        device = self._check_device(H.device)
        if self.compute_dtype != torch.float32:
            raise NotImplementedError("the head's backward pass is built for compute_dtype=float32 only")
        bs, n, L = H.shape
        if seed is None:
            seed = _draw_seed()
        seed &= 2**64 - 1
        if seed >= 2**63:                    # the op's schema takes the key as a signed int64
            seed -= 2**64
        pf, pa = self._dropout_ps()
        pf = pf if p_feat is None else p_feat
        pa = pa if p_att is None else p_att
        params = [p.to(device=device, dtype=torch.float32).contiguous() for p in self._live_head()]
        Hc = H.reshape(bs * n, L).to(torch.float32).contiguous()
        Y, A = torch.ops.mcgmil.mcdo_forward(Hc, self._offsets(n, bs, device), *params, T, float(pf),
                                             float(pa), seed, bag_id_base, t_base)
        C = self.num_classes
        return Y.permute(1, 0, 2), A.view(bs, T, C, n).permute(1, 0, 2, 3)

    # ------------------------------------------------------------------ reference API
    def forward(self, x, targets=None, *, seed=None):
        """reference model.py:211-253. Returns (Y [bs, C], A_all [bs, C, n], aux_loss | None).
        Dropout is applied by the layers that are in train mode (eval(): none). In train mode
        with gradients enabled it needs enable_head_training(); `seed` is then the Philox key of
        the step's dropout masks (None: drawn from torch's default CPU generator)."""
        if torch.is_grad_enabled() and self.training and any(p.requires_grad
                                                            for p in self.parameters()):
            if not self._head_training:
                raise NotImplementedError("training is out of scope for the MI355X MCDO build; "
                                          "call forward() in eval mode or under torch.no_grad() "
                                          "(or opt in with enable_head_training())")
            with features.native_conv_training(self._backbone_training), \
                    features.native_conv_x3_training(self._backbone_training and self._bf16x3_backbone_training), \
                    features.native_norm_training(self._norm_training), \
                    features.native_stem_training(self._stem_training), \
                    features.native_stem_conv_training(self._stem_conv_training):
                if self._bf16_backbone_training:
                    with torch.autocast("cuda", torch.bfloat16), features.native_conv_bf16_training(), \
                            features.native_norm_bf16_training(self._bf16_norm_training), \
                            features.native_stem_bf16_training(self._bf16_stem_training), \
                            features.native_stem_conv_bf16_training(self._bf16_stem_conv_training):
                        H = self.extract_features(x)
                else:
                    H = self.extract_features(x)
            Y, A = self.forward_features(H, T=1, seed=seed)
            Y, A = Y[0], A[0]
            aux = None
            if targets is not None:
                is_positive = targets.item() == 1
                aux = self.auxiliary_loss.scale * self.auxiliary_loss(A[:, 1, :], A[:, 0, :],
                                                                      is_positive)
            return Y, A, aux
        with torch.no_grad():
            H = self.extract_features(x)
            pf, pa = self._dropout_ps()
            Y, A = self.mc_inference_features(H, T=1, p_feat=pf, p_att=pa)
        Y, A = Y[0], A[0]
        aux = None
        if targets is not None:
            is_positive = targets.item() == 1
            aux = self.auxiliary_loss.scale * self.auxiliary_loss(A[:, 1, :], A[:, 0, :],
                                                                  is_positive)
        return Y, A, aux

    def _enable_mc_dropout(self, device):
        # reference model.py:263-271 (the dropout layers stay in train mode afterwards)
        self.eval()
        self.to(device)

        def enable_dropout(m):
            if isinstance(m, nn.Dropout):
                m.train()
        self.apply(enable_dropout)

    @torch.no_grad()
    def mc_inference(self, input_tensor, N=30, device="cuda", targets=None, *, seed=None,
                     return_losses=False):
        """reference model.py:256-328: (Y [N, bs, C], A [N, bs, C, n]) for N MC samples.
        return_losses=True returns the 3-tuple (Y, A, losses) the reference's callers unpack
        (infer.py:191, net_utils.py:126,205)."""
        device = self._check_device(device)
        self._enable_mc_dropout(device)
        x = input_tensor.to(device)
        H = self.extract_features(x)
        pf, pa = self._dropout_ps()
        Y, A = self.mc_inference_features(H, T=N, seed=seed, p_feat=pf, p_att=pa)
        if not return_losses:
            return Y, A
        losses = None
        if targets is not None:
            is_positive = targets.item() == 1
            s = self.auxiliary_loss.scale
            losses = [s * self.auxiliary_loss(A[i, :, 1, :], A[i, :, 0, :], is_positive)
                      for i in range(N)]
        return Y, A, losses

    @torch.no_grad()
    def mc_inference_serial(self, input_tensor, N=30, device="cuda", *, seed=None):
        """reference model.py:330-401: one kernel launch per sample (sample counter t_base=t);
        same values as mc_inference with the same seed."""
        device = self._check_device(device)
        self._enable_mc_dropout(device)
        x = input_tensor.to(device)
        H = self.extract_features(x)
        pf, pa = self._dropout_ps()
        if seed is None:
            seed = _draw_seed()
        Ys, As = [], []
        for t in range(N):
            Y, A = self.mc_inference_features(H, T=1, seed=seed, p_feat=pf, p_att=pa, t_base=t)
            Ys.append(Y[0])
            As.append(A[0])
        return torch.stack(Ys), torch.stack(As)
