"""GPU tests of the fp32 convolution on split-bf16 MFMA (include/mcgmil_features.h,
mcgmil_conv2d_f32x3: "bf16x3") -- the reference's fp32 ResNet convolutions (model.py:166-177) with
fp32 storage and three bf16 products per K, opt-in through conv2d_f32(precision=),
features.float32_conv_precision, MCGMIL_CONV32_PRECISION and model.feature_precision.

References: tests/conv32x3_ref.py's three-term emulation with fp64 sums (products of bf16 terms
are exact in fp32, so the kernel differs from it by its fp32 accumulation alone:
test_gpu_conv32.py's bound 2e-6 |ref| + 1e-5 conv(|x|, |w|)), and the fp64 convolution of the
unsplit operands (the same bound plus the split's derived worst case 3 * 2^-16 conv(|x|, |w|)).
The bf16 MFMA kernel (features.conv2d on x.bfloat16()) and the bf16 native backbone give the scale:
bf16x3's nrel must be at most 1/32 of theirs (measured >= 330x per layer in the emulation)."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conv32x3_ref import HI_ONLY_RATIO, SHAPES, SPLIT_BOUND, conv64, conv_x3, make_case, nrel, shape_id

pytestmark = pytest.mark.gpu

_cases = {}


def _layer(w, stride, pad, dev):
    conv = nn.Conv2d(w.shape[1], w.shape[0], tuple(w.shape[2:]), stride, pad, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    return conv.to(dev).eval()


def _case(shape, dev):
    """(conv, x channels-last on the device, emulation, fp64 reference, conv(|x|, |w|)), built once
    per shape and left unchanged."""
    if shape not in _cases:
        x, w, stride, pad = make_case(shape, SHAPES.index(shape) if shape in SHAPES else 99)
        _cases[shape] = (_layer(w, stride, pad, dev), x.to(dev).contiguous(memory_format=torch.channels_last),
                         conv_x3(x, w, stride, pad), conv64(x, w, stride, pad), conv64(x.abs(), w.abs(), stride, pad))
    return _cases[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_matches_emulation_and_fp64(cuda, shape):
    from mcgmil.features import conv2d, conv2d_f32, conv32x3_fusable, conv_fusable
    conv, x, emu, ref, mag = _case(shape, cuda)
    with torch.no_grad():
        assert conv32x3_fusable(conv, x)
        y = conv2d_f32(conv, x, precision="bf16x3")
        y2 = conv2d_f32(conv, x, precision="bf16x3")
        exact = conv2d_f32(conv, x)
        torch.cuda.synchronize()
    assert y.dtype == torch.float32 and y.is_contiguous(memory_format=torch.channels_last)
    assert y.shape == ref.shape
    yd = y.double().cpu()
    # the sharp one: a missing, doubled or mis-indexed term or tap is far outside fp32 accumulation
    err = (yd - emu).abs()
    worst = float((err - 2e-6 * emu.abs() - 1e-5 * mag).max())
    print(f"{shape_id(shape)}: vs emulation max excess {worst:.3e}, nrel {nrel(yd, emu):.3e}")
    assert bool((err <= 2e-6 * emu.abs() + 1e-5 * mag + 1e-30).all()), worst
    err = (yd - ref).abs()
    worst = float((err - 2e-6 * ref.abs() - (SPLIT_BOUND + 1e-5) * mag).max())
    n3 = nrel(yd, ref)
    print(f"{shape_id(shape)}: vs fp64 max excess {worst:.3e}, nrel {n3:.3e}, exact kernel {nrel(exact.cpu(), ref):.3e}")
    assert bool((err <= 2e-6 * ref.abs() + (SPLIT_BOUND + 1e-5) * mag + 1e-30).all()), worst
    # the path ran, and a second launch gives the same bits
    assert not torch.equal(y, exact)
    assert torch.equal(y, y2)
    if conv.in_channels % 64 == 0:       # the bf16 MFMA kernel's domain
        xb = x.bfloat16()
        with torch.no_grad():
            assert conv_fusable(conv.bfloat16(), xb)
            nb = nrel(conv2d(conv.bfloat16(), xb).float().cpu(), ref)
        conv.float()
        print(f"{shape_id(shape)}: bf16 kernel nrel {nb:.3e}, ratio {nb / n3:.0f}")
        assert n3 <= HI_ONLY_RATIO * nb, (n3, nb)


def test_keyword_context_and_environment_reach_the_kernel(cuda, monkeypatch):
    from mcgmil import features
    conv, x, *_ = _case(SHAPES[1], cuda)
    monkeypatch.delenv("MCGMIL_CONV32_PRECISION", raising=False)
    with torch.no_grad():
        exact = features.conv2d_f32(conv, x)
        y = features.conv2d_f32(conv, x, precision="bf16x3")
        assert not torch.equal(y, exact)
        assert torch.equal(features.run_conv(conv, x), exact)
        with features.float32_conv_precision("bf16x3"):
            assert torch.equal(features.conv2d_f32(conv, x), y)
            assert torch.equal(features.run_conv(conv, x), y)
            assert torch.equal(features.conv2d_f32(conv, x, precision="fp32"), exact)
        monkeypatch.setenv("MCGMIL_CONV32_PRECISION", "bf16x3")
        assert torch.equal(features.run_conv(conv, x), y)
        with features.float32_conv_precision("fp32"):
            assert torch.equal(features.run_conv(conv, x), exact)
        monkeypatch.setenv("MCGMIL_CONV32_PRECISION", "tf32")        # anything else: fp32
        assert torch.equal(features.run_conv(conv, x), exact)


def test_layers_outside_the_domain_keep_the_exact_kernel(cuda, monkeypatch):
    """Cin = 16 and the 3-channel stem under the ambient setting: bitwise the exact kernel; the
    keyword raises for them."""
    from mcgmil import features
    monkeypatch.delenv("MCGMIL_CONV32_PRECISION", raising=False)
    for shape in ((2, 16, 10, 10, 64, 5, 1, 2), (3, 3, 64, 52, 64, 7, 2, 3)):
        conv, x, *_ = _case(shape, cuda)
        with torch.no_grad():
            assert features.conv32_fusable(conv, x) and not features.conv32x3_fusable(conv, x)
            exact = features.conv2d_f32(conv, x)
            with features.float32_conv_precision("bf16x3"):
                assert torch.equal(features.conv2d_f32(conv, x), exact)
                assert torch.equal(features.run_conv(conv, x), exact)
            with pytest.raises(ValueError, match="multiple of 32"):
                features.conv2d_f32(conv, x, precision="bf16x3")
    conv, x, *_ = _case(SHAPES[1], cuda)
    with torch.no_grad(), pytest.raises(ValueError, match="precision"):
        features.conv2d_f32(conv, x, precision="bf16")


def _combine(part):
    """fp64 Chan combination of [parts, 3, C] (count, mean, M2) blocks -> (count, mean, var)."""
    p = part.double()
    n, m, M2 = p[:, 0], p[:, 1], p[:, 2]
    N = n.sum(0)
    mean = (n * m).sum(0) / N
    var = (M2 + n * (m - mean) ** 2).sum(0) / N
    return N, mean, var


# both tile shapes, a 9-pixel layer (three of the tile's four waves have no pixel), ragged last
# tiles (1,200 = 4 x 256 + 176 and 126 = 128 - 2 pixels), a 1x1 stride-2 downsample
STATS_SHAPES = [
    (1, 64, 3, 3, 64, 3, 1, 1),
    (3, 64, 20, 20, 64, 3, 1, 1),
    (2, 64, 17, 13, 128, 3, 2, 1),
    (3, 128, 9, 9, 256, 1, 2, 0),
]


@pytest.mark.parametrize("shape", STATS_SHAPES, ids=shape_id)
def test_stats(cuda, shape):
    """The epilogue's (count, mean, M2) blocks combine to the fp64 mean / variance of the kernel's
    own outputs, over every output pixel; y is unchanged by computing them."""
    from mcgmil.features import conv2d_f32
    conv, x, *_ = _case(shape, cuda)
    Cout = conv.out_channels
    with torch.no_grad():
        y, part = conv2d_f32(conv, x, stats=True, precision="bf16x3")
        torch.cuda.synchronize()
        assert torch.equal(y, conv2d_f32(conv, x, precision="bf16x3"))
    cnt, mean, var = _combine(part)
    yd = y.double().permute(0, 2, 3, 1).reshape(-1, Cout)
    assert bool((cnt == yd.shape[0]).all())
    rmean, rvar = yd.mean(0), yd.var(0, unbiased=False)
    scale = rvar.sqrt() + rmean.abs()
    e_mean, e_var = float(((mean - rmean).abs() / scale).max()), float(((var - rvar).abs() / rvar).max())
    print(f"{shape_id(shape)}: {part.shape[0]} parts, mean err {e_mean:.3e}, var err {e_var:.3e}")
    assert e_mean <= 1e-6
    assert e_var <= 1e-5


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", [(3, 64, 15, 11, 64, 3, 1, 1), (2, 128, 9, 9, 256, 3, 2, 1),
                                   (2, 64, 12, 12, 128, 1, 2, 0), (2, 2048, 5, 3, 512, 1, 1, 0),
                                   (3, 256, 9, 7, 64, 1, 1, 0)], ids=shape_id)
def test_input_bn_bitwise(cuda, shape, relu):
    """conv(relu?(bn(x))) with the BatchNorm applied while staging (in_ab), before the split, is
    bit-identical to mcgmil_batchnorm_act followed by the plain bf16x3 convolution; padding stays
    zero."""
    from mcgmil.features import batchnorm_act, batchnorm_coefficients, conv2d_f32, conv32_input_bn
    conv, x, *_ = _case(shape, cuda)
    Cin = conv.in_channels
    x = (x * 3 + 1).contiguous(memory_format=torch.channels_last)
    g = torch.Generator(device=cuda).manual_seed(Cin)
    bn = nn.BatchNorm2d(Cin).to(cuda)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(Cin, device=cuda, generator=g))
        bn.bias.copy_(torch.randn(Cin, device=cuda, generator=g))
    bn.eval()
    bn.running_mean, bn.running_var = None, None          # batch statistics, as the reference
    bn.track_running_stats = False
    with torch.no_grad():
        assert conv32_input_bn(conv, x)
        ab = batchnorm_coefficients(x, bn)
        y_in = conv2d_f32(conv, x, in_ab=ab, in_relu=relu, precision="bf16x3")
        xb = batchnorm_act(x, bn, relu)
        y_ref = conv2d_f32(conv, xb, precision="bf16x3")
        torch.cuda.synchronize()
        assert not torch.equal(y_ref, conv2d_f32(conv, xb))
    assert torch.equal(y_in, y_ref)


# ---------------------------------------------------------------------------------- backbone
def _run(net, x, dtype=torch.float32, env=None, monkeypatch=None):
    with monkeypatch.context() as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        with torch.no_grad():
            if dtype == torch.bfloat16:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y = net(x).float()
            else:
                y = net(x)
        torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("arch", ["r18", "r50"])
def test_backbone(cuda, arch, monkeypatch):
    """Batch statistics, test_gpu_resnet_blocks.py's 12 x 3 x 96 x 96 input, no-grad."""
    from mcgmil.resnet import build_backbone, deactivate_batchnorm, Identity
    monkeypatch.delenv("MCGMIL_CONV32_PRECISION", raising=False)
    torch.manual_seed(0)
    net = build_backbone(arch, pretrained=False)
    net.fc = Identity()
    net.apply(deactivate_batchnorm)
    net = net.to(cuda).eval().to(memory_format=torch.channels_last)
    g = torch.Generator(device=cuda).manual_seed(5)
    x = torch.rand(12, 3, 96, 96, device=cuda, generator=g)
    x = ((x - 0.45) / 0.25).contiguous(memory_format=torch.channels_last)
    ref = _run(copy.deepcopy(net).double(), x.double(), monkeypatch=monkeypatch)
    assert ref.dtype == torch.float64 and torch.isfinite(ref).all()
    stems = []
    hook = net.layer1.register_forward_pre_hook(lambda m, inp: stems.append(inp[0].clone()))
    x3 = {"MCGMIL_CONV32_PRECISION": "bf16x3"}
    exact = _run(net, x, monkeypatch=monkeypatch)
    fold = _run(net, x, env=dict(x3, MCGMIL_FUSE_INPUT_BN="1"), monkeypatch=monkeypatch)
    nofold = _run(net, x, env=dict(x3, MCGMIL_FUSE_INPUT_BN="0"), monkeypatch=monkeypatch)
    hook.remove()
    bf16 = _run(net, x, torch.bfloat16, monkeypatch=monkeypatch)
    assert torch.isfinite(fold).all()
    assert torch.equal(fold, nofold)
    assert not torch.equal(fold, exact)
    assert torch.equal(stems[0], stems[1]) and torch.equal(stems[0], stems[2])
    n32, n3, nb = nrel(exact, ref), nrel(fold, ref), nrel(bf16, ref)
    print(f"{arch} features nrel vs fp64: fp32 {n32:.3e}, bf16x3 {n3:.3e}, bf16 {nb:.3e}, bf16/bf16x3 {nb / n3:.0f}")
    assert n3 <= nb / 32, (n32, n3, nb)


# ---------------------------------------------------------------------------------- model
def test_model_feature_precision(cuda, monkeypatch):
    from mcgmil import features
    from mcgmil.model import MultiHeadGatedAttentionMIL
    monkeypatch.delenv("MCGMIL_CONV32_PRECISION", raising=False)
    torch.manual_seed(3)
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False, shared_attention=False).to(cuda)
    t = copy.deepcopy(m).train().enable_head_training().enable_backbone_training()
    x = torch.rand(1, 3, 3, 64, 64, device=cuda)
    routed = []
    real = features.packed_conv_weight_f32x3
    monkeypatch.setattr(features, "packed_conv_weight_f32x3", lambda conv, t: routed.append(conv) or real(conv, t))
    assert m.feature_precision == "fp32"
    Y0, A0 = m.mc_inference(x, N=4, device=cuda, seed=11)
    assert not routed
    m.feature_precision = "bf16x3"
    Y1, A1 = m.mc_inference(x, N=4, device=cuda, seed=11)
    assert len(routed) == 19                     # every convolution of r18 but the 3-channel stem
    assert len({id(c) for c in routed}) == 19
    assert not (torch.equal(Y0, Y1) and torch.equal(A0, A1))
    assert float((Y1 - Y0).abs().max()) <= 1e-3 * float(Y0.abs().max())
    # training with the backbone opt-in: autograd's ops stay exact fp32
    del routed[:]
    t.feature_precision = "bf16x3"
    target = torch.tensor([1], device=cuda)
    Yt, At, aux = t(x, target, seed=99)
    (F.cross_entropy(Yt, target) + aux).backward()
    assert not routed
    t.feature_precision = "fp32"
    t.zero_grad()
    Ye, Ae, _ = t(x, target, seed=99)
    assert torch.equal(Yt, Ye) and torch.equal(At, Ae)
    # back to the default: the same bits as before
    m.feature_precision = "fp32"
    Y2, A2 = m.mc_inference(x, N=4, device=cuda, seed=11)
    assert not routed
    assert torch.equal(Y0, Y2) and torch.equal(A0, A2)
