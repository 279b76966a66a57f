"""Host-side checks of the fp32 convolution backward (no kernel launches): the flipped-weight
identity the native data gradient rests on, the fake kernels of the two ops, and the opt-in."""
import pytest
import torch
import torch.nn.functional as F

from mcgmil import MultiHeadGatedAttentionMIL, features, library  # noqa: F401


@pytest.mark.parametrize("k,p", [(3, 1), (1, 0), (5, 2), (3, 0)])
def test_flipped_weight_reproduces_autograd_dx(k, p):
    gen = torch.Generator().manual_seed(k * 10 + p)
    x = torch.randn(2, 5, 8, 7, dtype=torch.float64, generator=gen, requires_grad=True)
    w = torch.randn(6, 5, k, k, dtype=torch.float64, generator=gen)
    y = F.conv2d(x, w, None, 1, p)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=gen)
    y.backward(dy)
    wf = features.flipped_weight(w)
    assert wf.shape == (5, 6, k, k) and wf.is_contiguous()
    dx = F.conv2d(dy, wf, None, 1, k - 1 - p)
    assert dx.shape == x.shape
    assert float((dx - x.grad).abs().max()) <= 1e-13


@pytest.mark.parametrize("stride,pad,k", [(1, 1, 3), (2, 1, 3), (2, 0, 1)])
def test_fake_kernels_shapes_and_channels_last_strides(stride, pad, k):
    x = torch.empty(3, 64, 9, 11, device="meta").contiguous(memory_format=torch.channels_last)
    w = torch.empty(128, 64, k, k, device="meta")
    y = torch.ops.mcgmil.conv2d_f32(x, w, stride, pad)
    oh, ow = (9 + 2 * pad - k) // stride + 1, (11 + 2 * pad - k) // stride + 1
    assert y.shape == (3, 128, oh, ow) and y.dtype == torch.float32 and y.device.type == "meta"
    assert y.is_contiguous(memory_format=torch.channels_last) and y.stride(1) == 1
    dx, dw = torch.ops.mcgmil.conv2d_f32_backward(x, w, y, stride, pad, True, True)
    assert dx.shape == x.shape and dx.is_contiguous(memory_format=torch.channels_last) and dx.stride(1) == 1
    assert dw.shape == w.shape and dw.is_contiguous()
    dx, dw = torch.ops.mcgmil.conv2d_f32_backward(x, w, y, stride, pad, False, False)
    assert dx.numel() == 0 and dw.numel() == 0


def test_conv32_trainable_has_no_cpu_or_autograd_clause():
    conv = torch.nn.Conv2d(64, 64, 3, 1, 1, bias=False)
    assert not features.conv32_trainable(conv, torch.zeros(1, 64, 4, 4))     # a CPU tensor
    shim = features._ConvShim(conv.weight, 2, 1)
    assert isinstance(shim, torch.nn.Conv2d) and shim.weight.data_ptr() == conv.weight.data_ptr()
    assert (shim.in_channels, shim.out_channels, shim.kernel_size, shim.stride, shim.padding) == \
        (64, 64, (3, 3), (2, 2), (1, 1))
    assert not shim.weight.requires_grad and shim.bias is None
    assert features.dgrad_native(conv) and not features.dgrad_native(shim)


def test_native_conv_training_context_restores():
    assert features._native_training is False
    with features.native_conv_training():
        assert features._native_training is True
        with features.native_conv_training(False):
            assert features._native_training is False
        assert features._native_training is True
    assert features._native_training is False


def test_enable_backbone_training_toggles_and_train_mode_still_needs_the_head_opt_in():
    m = MultiHeadGatedAttentionMIL(pretrained=False)
    assert m._backbone_training is False
    assert m.enable_backbone_training() is m and m._backbone_training is True
    m.train()
    with pytest.raises(NotImplementedError):          # the backbone opt-in alone does not train
        m(torch.zeros(1, 2, 3, 32, 32))
    assert m.enable_backbone_training(False) is m and m._backbone_training is False
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 2, 3, 32, 32))
