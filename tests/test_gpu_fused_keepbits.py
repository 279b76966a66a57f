"""The affine launch's scoring phase (mcgmil_kernels.h: fill_fused_const, finish_scores): the
attention keep bits of a region are drawn once into LDS (byte (row >> 3) * C + c, bit row & 7), the
scoring item of thread tid is (row tid % 128, class tid / 128), and the partial scores are summed
by a loop-free body. None of it may change a bit: every case runs the forced fused launch against the forced two-kernel launch
(mcgmil_args.flags) and requires Y, A, A_mean and A_var bitwise equal, and the fused launch bitwise
repeatable.

Shapes are the smallest at which the bitmap's indexing can go wrong: 32 t-groups of one tile in a
region followed by a region of a single t-group (N = 128, T = 33), two tiles per t-group (N = 256),
the bitmap at full size with one t-group per region (N = 4096), the benchmark's region shape
(N = 2048, T = 4: two t-groups of 16 tiles), and the four-class instantiation whose regions hold a
quarter of the rows (N = 1024, C = 4; two waves per class) and a single class (shared gate: all
eight waves per class). Each with 3 and 8 bags (the plain and the XCD region map), the bags' Philox
counters given explicitly (non-contiguous) and as a base; a sample counter base t_base != 0, also
against one call per sample (the serial form: T = 1, t_base + t); attention dropout of 0, 0.1, 0.5
and just below 1; and two bags per shape against the CPU oracle (oracle/mcdo_ref.py) on the same
bf16 operands with the kernel's own Philox masks, at the bounds of tests/test_gpu_parity.py, so that
an error common to both launches cannot hide."""
import numpy as np
import pytest
import torch

from oracle import mcdo_ref
from mcgmil import synthetic
from test_gpu_parity import TOL_BF16_IN

pytestmark = pytest.mark.gpu

L = 512
#         N     T   C  D
SHAPES = [(128, 33, 2, 128), (256, 3, 2, 128), (4096, 2, 2, 128), (2048, 4, 2, 128),
          (1024, 5, 4, 64), (1024, 5, 1, 128)]
SHAPE_IDS = [f"N{n}_T{t}_C{c}" for n, t, c, _ in SHAPES]
KEYS = ("Y", "A", "A_mean", "A_var")


def head_on(arrays, dev):
    from mcgmil.ops import HeadTensors
    return HeadTensors(*[torch.from_numpy(np.ascontiguousarray(arrays[k])).to(dev)
                         for k in HeadTensors._fields])


def launch(cuda, H, B, N, T, C, D, path, sd=None, ids="base", p_att=0.1, t_base=0, seed=99):
    from mcgmil import ops
    sd = sd if sd is not None else synthetic.head_state_dict(5, L=L, D=D, C=C, shared=False)
    head = head_on(synthetic.head_arrays(sd, C, False), cuda)
    kw = dict(p_feat=0.1, p_att=p_att, seed=seed, t_base=t_base, return_stats=True)
    if ids == "explicit":
        kw["bag_ids"] = torch.tensor([13 * b + 4 for b in range(B)], dtype=torch.int32, device=cuda)
    else:
        kw["bag_id_base"] = 21
    # bf16 heads of <= 8 gate tile pairs fuse only with the gate forced to the 8-wave tile
    gate = "pipe" if head.G * D // 16 <= 8 else "auto"
    return ops.mcdo_forward(H, ops.bag_offsets_tensor([N] * B, cuda), head, T, path=path, gate=gate, **kw)


def features(cuda, rows, seed=77):
    g = torch.Generator(device=cuda).manual_seed(seed)
    return torch.randn(rows, L, device=cuda, generator=g).abs_().bfloat16().contiguous()


def fused_equals_two_kernel(cuda, B, N, T, C, D, H=None, **kw):
    H = H if H is not None else features(cuda, B * N)
    out = launch(cuda, H, B, N, T, C, D, "fused", **kw)
    ref = launch(cuda, H, B, N, T, C, D, "two_kernel", **kw)
    again = launch(cuda, H, B, N, T, C, D, "fused", **kw)
    torch.cuda.synchronize()
    assert set(ref) >= set(KEYS)
    for k in KEYS:
        assert torch.equal(out[k], ref[k]), k
        assert torch.equal(out[k], again[k]), k
    return out


@pytest.mark.parametrize("ids", ["explicit", "base"])
@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("N,T,C,D", SHAPES, ids=SHAPE_IDS)
def test_keep_bits_equal_two_kernel(cuda, N, T, C, D, B, ids):
    fused_equals_two_kernel(cuda, B, N, T, C, D, ids=ids)


# just below 1: the 16-bit threshold 65,529 of 65,536, where nearly every logit is dropped
@pytest.mark.parametrize("p_att", [0.0, 0.1, 0.5, 0.9999])
@pytest.mark.parametrize("N,T,C,D", SHAPES, ids=SHAPE_IDS)
def test_attention_dropout_rates(cuda, N, T, C, D, p_att):
    out = fused_equals_two_kernel(cuda, 3, N, T, C, D, p_att=p_att, ids="explicit")
    assert torch.isfinite(out["A"]).all()


@pytest.mark.parametrize("N,T,C,D", SHAPES, ids=SHAPE_IDS)
def test_sample_counter_base(cuda, N, T, C, D):
    """t_base != 0 in one call of T samples, and the serial form of the same samples: one call per
    sample with T = 1 and t_base + t draws the same masks, so its A and Y are bitwise the rows of
    the call of T samples."""
    B, t_base = 3, 1000
    H = features(cuda, B * N)
    out = fused_equals_two_kernel(cuda, B, N, T, C, D, H=H, t_base=t_base)
    A = out["A"].view(B, T, C, N)
    for t in sorted({0, T // 2, T - 1}):
        one = launch(cuda, H, B, N, 1, C, D, "fused", t_base=t_base + t)
        torch.cuda.synchronize()
        assert torch.equal(one["A"].view(B, 1, C, N)[:, 0], A[:, t]), t
        assert torch.equal(one["Y"][:, 0], out["Y"][:, t]), t


@pytest.mark.parametrize("N,T,C,D", SHAPES, ids=SHAPE_IDS)
def test_two_bags_against_oracle(cuda, N, T, C, D):
    B, seed, p_f, p_a = 2, 321, 0.1, 0.1
    sd = synthetic.head_state_dict(12, L=L, D=D, C=C, shared=False)
    Hs = [synthetic.bf16_round(synthetic.bag_features(500 + b, N)) for b in range(B)]
    H = torch.from_numpy(np.concatenate(Hs)).to(cuda).bfloat16()
    out = fused_equals_two_kernel(cuda, B, N, T, C, D, H=H, sd=sd, seed=seed)
    prm = mcdo_ref.HeadParams(synthetic.head_arrays(synthetic.round_state_dict_bf16(sd), C, False))
    for b in range(B):
        kF, kA = mcdo_ref.masks_for_bag(seed, 21 + b, T, N, L, C, p_f, p_a)
        Yr, Ar = mcdo_ref.mc_inference(Hs[b], prm, kF, kA, p_f, p_a)
        Yr, Ar = Yr.numpy()[:, 0], Ar.numpy()[:, 0]
        o = T * C * N * b
        A = out["A"][o:o + T * C * N].cpu().numpy().reshape(T, C, N)
        Am = out["A_mean"][C * N * b:C * N * (b + 1)].cpu().numpy().reshape(C, N)
        np.testing.assert_allclose(out["Y"][b].cpu().numpy(), Yr, rtol=0, atol=TOL_BF16_IN["Y"])
        assert np.abs(A - Ar).max() / np.abs(Ar).max() <= TOL_BF16_IN["A"]
        assert np.abs(Am - Ar.mean(0)).max() / np.abs(Ar.mean(0)).max() <= TOL_BF16_IN["A_mean"]
