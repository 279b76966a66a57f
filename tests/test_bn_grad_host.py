"""Host-side checks of the fused BatchNorm/add/ReLU training op (no kernel launches): the fake
kernels of the two ops, the predicate and the context manager that route `features.bn_act`, the
opt-in on the module, and the closed-form backward of include/mcgmil_bn_grad.h restated in float64
against torch.autograd of F.batch_norm (+ add, + relu)."""
import pytest
import torch
import torch.nn as nn

import bn_grad_ref as R
from mcgmil import MultiHeadGatedAttentionMIL, features, library  # noqa: F401
from mcgmil.resnet import deactivate_batchnorm

CL = torch.channels_last


@pytest.mark.parametrize("relu,res,affine", [(True, True, True), (True, False, True), (False, True, False)])
def test_fake_kernels_shapes_strides_and_empty_gradients(relu, res, affine):
    x = torch.empty(3, 64, 9, 7, device="meta").contiguous(memory_format=CL)
    w = torch.empty(64, device="meta") if affine else None
    y, mean, invstd = torch.ops.mcgmil.bn_act_f32(x, w, w, x if res else None, 1e-5, relu)
    assert y.shape == x.shape and y.dtype == torch.float32 and y.device.type == "meta"
    assert y.is_contiguous(memory_format=CL) and y.stride(1) == 1
    for t in (mean, invstd):
        assert t.shape == (64,) and t.dtype == torch.float32 and t.device.type == "meta"
    dx, dres, dw, db = torch.ops.mcgmil.bn_act_f32_backward(x, y, y, w, mean, invstd, relu, True, True, True)
    assert dx.shape == x.shape and dx.dtype == torch.float32 and dx.is_contiguous(memory_format=CL)
    assert dx.stride(1) == 1 and dw.shape == db.shape == (64,)
    if relu:
        assert dres.shape == x.shape and dres.is_contiguous(memory_format=CL) and dres.stride(1) == 1
    else:
        assert dres.numel() == 0               # without ReLU the residual gradient is dy itself
    for flags in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        out = torch.ops.mcgmil.bn_act_f32_backward(x, y, y, w, mean, invstd, relu, *flags)
        need = (flags[0], flags[1] and relu, flags[2], flags[2])
        assert [t.numel() > 0 for t in out] == list(need), flags


def test_ops_have_no_cpu_kernel():
    x = torch.zeros(2, 8, 2, 2).contiguous(memory_format=CL)
    v = torch.ones(8)
    with pytest.raises((RuntimeError, ValueError)):
        torch.ops.mcgmil.bn_act_f32(x, v, v, None, 1e-5, True)
    with pytest.raises((RuntimeError, ValueError)):
        torch.ops.mcgmil.bn_act_f32_backward(x, x, x, v, v, v, True, True, False, True)


def _bn(C=64):
    bn = nn.BatchNorm2d(C)
    deactivate_batchnorm(bn)
    return bn


def test_bn_trainable_clauses():
    x = torch.zeros(2, 64, 4, 4)
    why = features.bn_untrainable_reason
    assert not features.bn_trainable(x, _bn()) and why(x, _bn()).startswith("device")     # a CPU tensor
    assert not features.bn_trainable(x.bfloat16(), _bn()) and why(x.bfloat16(), _bn()).startswith("dtype")
    x12 = torch.zeros(2, 12, 4, 4)
    assert not features.bn_trainable(x12, _bn(12)) and why(x12, _bn(12)).startswith("channels")
    assert why(torch.zeros(2, 64, 4, 4), _bn(128)).startswith("channels")
    assert why(torch.zeros(1, 64, 1, 1), _bn()).startswith("rows")
    tracking = nn.BatchNorm2d(64)                       # train mode, tracks running statistics
    assert not features.bn_trainable(x, tracking) and "pending" in why(x, tracking)
    assert "running-statistics mode" in why(x, tracking.eval())
    assert why(x, _bn(), torch.zeros(2, 64, 4, 5)).startswith("residual")
    assert why(x, _bn(), x.double()).startswith("residual")
    assert why(x, nn.Identity()).startswith("layer")
    # eval mode without running statistics (deactivate_batchnorm) still normalises with the batch's
    assert why(x, _bn().eval()).startswith("device")


def test_bn_act_keeps_the_torch_layers_on_the_cpu_inside_the_context():
    bn = _bn(8)
    x = torch.randn(2, 8, 3, 3, requires_grad=True)
    want = torch.relu(bn(x) + x)
    with features.native_norm_training():
        got = features.bn_act(bn, x, True, x)
    assert torch.equal(got, want)


def test_native_norm_training_context_nests_and_restores():
    assert features._native_norm_training is False
    with features.native_norm_training():
        assert features._native_norm_training is True
        with features.native_norm_training(False):
            assert features._native_norm_training is False
        assert features._native_norm_training is True and features._native_training is False
    assert features._native_norm_training is False


def test_enable_backbone_training_norm_keyword():
    m = MultiHeadGatedAttentionMIL(pretrained=False)
    assert m._norm_training is False
    assert m.enable_backbone_training() is m and m._backbone_training is True and m._norm_training is False
    assert m.enable_backbone_training(norm=True) is m and m._backbone_training is True and m._norm_training is True
    m.train()
    with pytest.raises(NotImplementedError):          # still no training without the head opt-in
        m(torch.zeros(1, 2, 3, 32, 32))
    assert m.enable_backbone_training() is m and m._norm_training is False
    assert m.enable_backbone_training(False, norm=True) is m
    assert m._backbone_training is False and m._norm_training is False
    with pytest.raises(TypeError):
        m.enable_backbone_training(True, True)        # norm is keyword-only


@pytest.mark.parametrize("rows_shape,C,relu,res", [((2, 1, 1), 8, True, False), ((3, 9, 7), 64, True, True),
                                                   ((3, 2, 2), 2048, True, True), ((3, 4, 4), 512, False, True),
                                                   ((2, 5, 3), 16, False, False)])
def test_closed_form_matches_float64_autograd(rows_shape, C, relu, res):
    c = R.make(rows_shape, C, 17, relu, res)
    r = R.autograd(c, torch.float64)
    dx, g, dgamma, dbeta = R.formula(c["x"].double(), r["y"], c["dy"].double(), c["gamma"].double(), r["mean"],
                                     r["invstd"], relu)
    got = {"dx": dx, "dres": g, "dgamma": dgamma, "dbeta": dbeta}
    err = R.errors(got, r)
    print(err)
    assert set(err) == {"dx", "dgamma", "dbeta"} | ({"dres"} if res else set())
    assert all(e <= 1e-12 for e in err.values()), err
    if res and not relu:
        assert torch.equal(r["dres"], c["dy"].double())
