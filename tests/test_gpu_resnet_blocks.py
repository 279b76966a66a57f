"""GPU parity of the ResNet blocks and of the whole ResNet-34 / ResNet-50 backbones on the native
kernels (mcgmil/resnet.py through features.conv_bn_act) -- the reference's torchvision
BasicBlock / Bottleneck (model.py:166-177) with every BatchNorm on the bag's batch statistics
(infer.py:105-109).

Bottleneck.forward routes a 1x1 convolution's DeferredBN into a 3x3 halo convolution, a 3x3's into a
1x1 that cannot take it (materialise()), and a stride-1 or stride-2 downsample's into the residual
add at 256-2048 channels; ResNet-18's BasicBlocks reach none of that.

Reference: the same modules in fp64 (a deep copy, .double()): double tensors are refused by every
native gate, so it runs on torch's own layers. nrel = max|y - ref| / max|ref|.

  fp32         nrel(native) <= max(10 x nrel(torch fp32 layers), 1e-6): the rule for a changed
               summation order; the bound comes from the torch layers, measured in the
               same test, never from the native result.
  bf16         nrel(native) <= 1.25 x nrel(torch bf16-autocast layers) + 1e-3 (the ResNet-18
               criterion of test_gpu_features.py).
  fold         MCGMIL_FUSE_INPUT_BN=1 and 0 give the same bits, in both precisions.

Every comparison with the torch layers also asserts that the native path ran: its output differs
from theirs in at least one bit.
"""
import copy
import os

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

_TORCH_LAYERS = {"MCGMIL_FUSED_BN": "0", "MCGMIL_NATIVE_CONV": "0", "MCGMIL_NATIVE_STEM": "0"}


def _run(net, x, dtype, env=None):
    """net(x) under no_grad, in fp32 / fp64 as given or under bf16 autocast, with the environment
    switches in env set for the call and popped after it."""
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        with torch.no_grad():
            if dtype == torch.bfloat16:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y = net(x).float()
            else:
                y = net(x)
        torch.cuda.synchronize()
        return y
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)


def _nrel(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def _check_fp32(label, native, torch_layers, ref):
    assert not torch.equal(native, torch_layers), f"{label}: the native fp32 path did not run"
    n_native, n_torch = _nrel(native, ref), _nrel(torch_layers, ref)
    bound = max(10.0 * n_torch, 1e-6)
    print(f"{label} fp32 vs fp64: native nrel {n_native:.3e}, torch layers {n_torch:.3e}, bound {bound:.3e}")
    assert torch.isfinite(native).all()
    assert n_native <= bound, (n_native, n_torch, bound)


def _check_bf16(label, native, torch_layers, ref):
    assert not torch.equal(native, torch_layers), f"{label}: the native bf16 path did not run"
    d_native, d_torch = _nrel(native, ref), _nrel(torch_layers, ref)
    bound = 1.25 * d_torch + 1e-3
    print(f"{label} bf16 vs fp64: native nrel {d_native:.3e}, torch layers {d_torch:.3e}, bound {bound:.3e}")
    assert torch.isfinite(native).all()
    assert d_native <= bound, (d_native, d_torch, bound)


def _check_fold(label, net, x, dtype):
    out = {flag: _run(net, x, dtype, {"MCGMIL_FUSE_INPUT_BN": flag}) for flag in ("1", "0")}
    same = torch.equal(out["1"], out["0"])
    print(f"{label} {str(dtype).split('.')[-1]} fold on / off bitwise equal: {same}")
    assert same
    assert torch.isfinite(out["1"]).all()
    return out["1"]


# ---------------------------------------------------------------------------------- blocks
# (block, inplanes, planes, stride, downsample)
BLOCKS = {
    "bottleneck_64_64_down": ("Bottleneck", 64, 64, 1, True),          # layer 1's first: 64 -> 256, stride-1 downsample
    "bottleneck_256_64": ("Bottleneck", 256, 64, 1, False),            # layer 1's others: the identity is x
    "bottleneck_256_128_s2_down": ("Bottleneck", 256, 128, 2, True),   # layer 2's first
    "bottleneck_1024_512_s2_down": ("Bottleneck", 1024, 512, 2, True),  # layer 4's first: residual_ab at 2048
    "basic_64_128_s2_down": ("BasicBlock", 64, 128, 2, True),
}
_cases = {}


def _case(name, dev):
    """(block, x fp32 of bf16-representable values, fp64 output of the block), built once."""
    if name in _cases:
        return _cases[name]
    from mcgmil import resnet
    kind, inplanes, planes, stride, down = BLOCKS[name]
    cls = getattr(resnet, kind)
    seed = sum(map(ord, name))
    torch.manual_seed(seed)
    d = None
    if down:
        d = nn.Sequential(nn.Conv2d(inplanes, planes * cls.expansion, 1, stride, bias=False),
                          nn.BatchNorm2d(planes * cls.expansion))
    blk = cls(inplanes, planes, stride, d)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.randn(m.num_features, generator=g) * 0.5 + 1.0)
                m.weight[::5] *= -1.0
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.3)
    blk.apply(resnet.deactivate_batchnorm)
    blk = blk.to(dev).eval().to(memory_format=torch.channels_last)
    # bf16-representable inputs: the fp32, bf16 and fp64 runs all read the same values
    x = torch.randn(6, inplanes, 12, 10, generator=g).bfloat16().float().to(dev)
    x = x.contiguous(memory_format=torch.channels_last)
    ref = _run(copy.deepcopy(blk).double(), x.double(), torch.float64)
    assert ref.dtype == torch.float64 and torch.isfinite(ref).all()
    _cases[name] = (blk, x, ref)
    return _cases[name]


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_fp32_matches_fp64(cuda, name):
    blk, x, ref = _case(name, cuda)
    _check_fp32(name, _run(blk, x, torch.float32), _run(blk, x, torch.float32, _TORCH_LAYERS), ref)


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_bf16_drift(cuda, name):
    blk, x, ref = _case(name, cuda)
    xb = x.bfloat16()
    _check_bf16(name, _run(blk, xb, torch.bfloat16), _run(blk, xb, torch.bfloat16, _TORCH_LAYERS), ref)


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_input_bn_fold_bitwise(cuda, name):
    blk, x, _ = _case(name, cuda)
    y32 = _check_fold(name, blk, x, torch.float32)
    y16 = _check_fold(name, blk, x.bfloat16(), torch.bfloat16)
    # the folded runs are the native ones
    assert torch.equal(y32, _run(blk, x, torch.float32))
    assert torch.equal(y16, _run(blk, x.bfloat16(), torch.bfloat16))


# ---------------------------------------------------------------------------------- backbones
_nets = {}


def _backbone(arch, dev):
    """(net with batch-statistics BatchNorms, the ResNet-18 test's input, fp64 features), built once."""
    if arch in _nets:
        return _nets[arch]
    from mcgmil.resnet import build_backbone, deactivate_batchnorm, Identity
    torch.manual_seed(0)
    net = build_backbone(arch, pretrained=False)
    net.fc = Identity()
    net.apply(deactivate_batchnorm)
    net = net.to(dev).eval().to(memory_format=torch.channels_last)
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.rand(12, 3, 96, 96, device=dev, generator=g)
    x = ((x - 0.45) / 0.25).contiguous(memory_format=torch.channels_last)
    ref = _run(copy.deepcopy(net).double(), x.double(), torch.float64)
    assert ref.dtype == torch.float64 and torch.isfinite(ref).all()
    _nets[arch] = (net, x, ref)
    return _nets[arch]


@pytest.mark.parametrize("arch", ["r34", "r50"])
def test_backbone_fp32_matches_fp64(cuda, arch):
    net, x, ref = _backbone(arch, cuda)
    _check_fp32(arch, _run(net, x, torch.float32), _run(net, x, torch.float32, _TORCH_LAYERS), ref)


@pytest.mark.parametrize("arch", ["r34", "r50"])
def test_backbone_bf16_drift(cuda, arch):
    net, x, ref = _backbone(arch, cuda)
    _check_bf16(arch, _run(net, x, torch.bfloat16), _run(net, x, torch.bfloat16, _TORCH_LAYERS), ref)


@pytest.mark.parametrize("arch", ["r34", "r50"])
def test_backbone_input_bn_fold_bitwise(cuda, arch):
    net, x, _ = _backbone(arch, cuda)
    for dtype in (torch.float32, torch.bfloat16):
        y = _check_fold(arch, net, x, dtype)
        assert not torch.equal(y, _run(net, x, dtype, _TORCH_LAYERS)), "the native path did not run"


@pytest.mark.parametrize("arch", ["r34", "r50"])
def test_backbone_running_statistics_fold_bitwise(cuda, arch):
    """BatchNorms on running statistics (eval without deactivate_batchnorm): the folds use the
    running coefficients, bit-identical to the materialised form."""
    from mcgmil.resnet import build_backbone, Identity
    torch.manual_seed(1)
    net = build_backbone(arch, pretrained=False)
    net.fc = Identity()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight[::9] *= -1.0
    net = net.to(cuda).eval().to(memory_format=torch.channels_last)
    g = torch.Generator(device=cuda).manual_seed(4)
    x = torch.rand(6, 3, 112, 112, device=cuda, generator=g).contiguous(memory_format=torch.channels_last)
    for dtype in (torch.float32, torch.bfloat16):
        y = _check_fold(arch + " running statistics", net, x, dtype)
        assert not torch.equal(y, _run(net, x, dtype, _TORCH_LAYERS)), "the native path did not run"
