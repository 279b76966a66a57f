"""The closed form of include/mcgmil_pool_grad.h (pool_grad_ref.formula, with the window codes
derived from torch's own pool indices) against float64 CPU autograd of
max_pool2d(relu?(batch_norm(z))), on every geometry of the GPU tests; and the host-side pieces of
the opt-in (no GPU needed)."""
import pytest
import torch
import torch.nn as nn

import pool_grad_ref as P
from mcgmil import MultiHeadGatedAttentionMIL, _lib, features

CASES = P.cases(_lib.BN_POOL_GRAD_PART_ELEMS)


@pytest.mark.parametrize("name", list(CASES))
def test_closed_form_with_reference_codes_is_float64_autograd(name):
    shape, pool, relu, seed, integer = CASES[name]
    c = P.make(shape, pool, seed, relu, integer)
    r = P.autograd(c, torch.float64)
    code = P.codes(r["idx"], r["y"], shape[3], pool, relu)
    dz, dgamma, dbeta = P.formula(c["z"].double(), code, c["dy"].double(), c["gamma"].double(), r["mean"],
                                  r["invstd"], pool)
    got = {"dz": dz, "dgamma": dgamma, "dbeta": dbeta}
    err = P.R.errors(got, r, P.GRADS)
    print(name, {k: f"{e:.1e}" for k, e in err.items()})
    assert all(e <= 1e-12 for e in err.values()), err
    if integer:
        # several hundred windows whose maximum is positive and attained more than once: torch names
        # the first of them in row-major (kh, kw) order, which is what the codes must say
        k, st, pd = pool
        a = torch.nn.functional.pad(r["a"], (pd, pd, pd, pd), value=float("-inf"))
        win = torch.nn.functional.unfold(a, k, stride=st).view(shape[0], shape[1], k * k, -1)
        top = win.max(2, keepdim=True).values
        tied = ((win == top).sum(2) > 1) & (top[:, :, 0] > 0)
        print("windows with an exact positive tie:", int(tied.sum()))
        assert int(tied.sum()) >= 300
        first = (win == top).float().argmax(2)              # the first maximum in (kh, kw) order
        assert torch.equal(first[tied], code.view(shape[0], shape[1], -1).long()[tied])


def test_partition_constant_and_block_case():
    assert _lib.BN_POOL_GRAD_PART_ELEMS == 32768 and _lib.POOL_ARGMAX_NONE == P.NONE == 255
    N, C, H, W = CASES["blocks"][0]
    rpp = _lib.BN_POOL_GRAD_PART_ELEMS // C
    assert C == 64 and N * H * W // rpp >= 4 and N * H * W % rpp != 0
    assert N * C * H * W * 4 < 2 ** 20


def test_bn_pool_untrainable_reasons():
    bn = nn.BatchNorm2d(64)
    bn.track_running_stats, bn.running_mean, bn.running_var = False, None, None
    x = torch.randn(2, 64, 8, 8)
    reason = features.bn_pool_untrainable_reason
    assert reason(x, bn, nn.MaxPool2d(3, 2, 1)).startswith("device")      # everything but the device holds
    assert reason(x, bn, nn.MaxPool2d(2)).startswith("device")
    for pool in (nn.MaxPool2d(4, 2, 1), nn.MaxPool2d(3, 2, 1, ceil_mode=True), nn.MaxPool2d(3, 2, 1, dilation=2),
                 nn.MaxPool2d(5, 2, 2), nn.MaxPool2d(2, 3), nn.MaxPool2d((3, 2), 2), nn.AvgPool2d(3, 2, 1)):
        assert reason(x, bn, pool).startswith("pool"), pool
        assert not features.bn_pool_trainable(x, bn, pool)
    assert reason(x[:, :, :1, :1], bn, nn.MaxPool2d(3, 2, 0)).startswith("pool")
    assert reason(x.double(), bn, nn.MaxPool2d(3, 2, 1)).startswith("dtype")
    assert reason(x, nn.BatchNorm2d(64), nn.MaxPool2d(3, 2, 1)).startswith("statistics")


def test_native_stem_training_context_nests_and_restores():
    assert features._native_stem_training is False
    with features.native_stem_training():
        assert features._native_stem_training is True
        with features.native_stem_training(False):
            assert features._native_stem_training is False
        assert features._native_stem_training is True and features._native_norm_training is False
    assert features._native_stem_training is False


def test_enable_backbone_training_stem_keyword():
    m = MultiHeadGatedAttentionMIL(num_classes=2, pretrained=False)
    assert m._stem_training is False
    assert m.enable_backbone_training() is m and m._stem_training is False
    assert m.enable_backbone_training(stem=True) is m and m._backbone_training and m._stem_training
    assert m._norm_training is False                                   # stem does not depend on norm
    assert m.enable_backbone_training(norm=True, stem=True) is m and m._norm_training and m._stem_training
    assert m.enable_backbone_training(False, stem=True) is m and not m._backbone_training and not m._stem_training
    with pytest.raises(TypeError):
        m.enable_backbone_training(True, False, True)                  # stem is keyword-only


def test_cpu_layers_are_untouched_inside_the_context():
    bn = nn.BatchNorm2d(8)
    bn.track_running_stats, bn.running_mean, bn.running_var = False, None, None
    pool = nn.MaxPool2d(3, 2, 1)
    x = torch.randn(2, 8, 5, 6, requires_grad=True)
    with features.native_stem_training():
        y = features.bn_act(bn, x, True, pool=pool)
    assert torch.equal(y, pool(torch.relu(bn(x))))
