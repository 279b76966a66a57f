"""The two row sources of the single-launch hot path (mcgmil_kernels.h, fused_region): the affine
launch gate_fused_kernel (uniform bags of whole 128-row tiles whose regions fit LDS: no row table,
region constants and head vectors in LDS) and the row-table launch gate_fused_table_kernel (every
other batch). Each case runs the forced-fused launch against the forced two-kernel launch through
mcgmil_args.flags: Y, A, A_mean and A_var bitwise equal, and the fused launch bitwise repeatable.

Shapes are the small ones where the affine path can go wrong: one tile per t-group with many
t-groups per region (N = 128), two tiles per t-group (N = 256), a last region of a single t-group
(N = 2048, T = 3), two regions of unequal length (N = 128, T = 40), the XCD region map (B = 8) and
the plain one (B = 3), per-bag Philox counters given explicitly and as a base, T = 1, 3, 5 and
C = 1, 2; then the batches that must keep the row table (N = 200, a ragged batch that contains a
whole-tile bag, a bag above the LDS cap), both head layouts, fp32, and one case against the CPU
oracle so that an error common to both launches cannot hide."""
import numpy as np
import pytest
import torch

from oracle import mcdo_ref
from mcgmil import synthetic

pytestmark = pytest.mark.gpu

L = 512


def head_on(arrays, dev):
    from mcgmil.ops import HeadTensors
    return HeadTensors(*[torch.from_numpy(np.ascontiguousarray(arrays[k])).to(dev)
                         for k in HeadTensors._fields])


def features(sizes, dev, dtype, seed=77):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(sum(sizes), L, device=dev, generator=g).abs_().to(dtype).contiguous()


def both_paths(cuda, sizes, T, C, shared=False, dtype=torch.bfloat16, ids="explicit", D=128, H=None, sd=None,
               seed=99):
    """Forced fused (twice) and forced two-kernel launches of one batch; asserts the bitwise
    equalities and returns the fused outputs."""
    from mcgmil import ops
    sd = sd if sd is not None else synthetic.head_state_dict(5, L=L, D=D, C=C, shared=shared)
    head = head_on(synthetic.head_arrays(sd, C, shared), cuda)
    H = H if H is not None else features(sizes, cuda, dtype)
    offs = ops.bag_offsets_tensor(sizes, cuda)
    kw = dict(p_feat=0.1, p_att=0.1, seed=seed, return_stats=True)
    if ids == "explicit":
        kw["bag_ids"] = torch.tensor([13 * b + 4 for b in range(len(sizes))], dtype=torch.int32, device=cuda)
    else:
        kw["bag_id_base"] = 21
    # bf16 heads of <= 8 gate tile pairs fuse only with the gate forced to the 8-wave tile
    gate = "pipe" if dtype == torch.bfloat16 and head.G * D // 16 <= 8 else "auto"
    out = ops.mcdo_forward(H, offs, head, T, path="fused", gate=gate, **kw)
    ref = ops.mcdo_forward(H, offs, head, T, path="two_kernel", gate=gate, **kw)
    again = ops.mcdo_forward(H, offs, head, T, path="fused", gate=gate, **kw)
    torch.cuda.synchronize()
    assert set(ref) >= {"Y", "A", "A_mean", "A_var"}
    for k in ref:
        a, r, g = out[k], ref[k], again[k]
        if k == "A_var" and T == 1:       # the variance of one sample may be NaN: NaN must meet NaN
            a, r, g = (torch.nan_to_num(x, nan=7.0) for x in (a, r, g))
        assert torch.equal(a, r), k
        assert torch.equal(a, g), k
    return out


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("ids", ["explicit", "base"])
@pytest.mark.parametrize("T", [1, 3, 5])
@pytest.mark.parametrize("B", [8, 3])
@pytest.mark.parametrize("N", [128, 256, 2048])
def test_affine_rows_equal_two_kernel(cuda, N, B, T, ids, C):
    both_paths(cuda, [N] * B, T, C, ids=ids)


@pytest.mark.parametrize("ids", ["explicit", "base"])
def test_affine_two_regions_of_unequal_length(cuda, ids):
    """N = 128, T = 40: a region of 32 t-groups (32 tiles, the most a region holds) and one of 8."""
    both_paths(cuda, [128] * 8, 40, 2, ids=ids)


@pytest.mark.parametrize("sizes", [[200] * 3, [200] * 8, [130, 128, 300], [128, 256, 128]],
                         ids=["uniform200_B3", "uniform200_B8", "ragged", "ragged_whole_tiles"])
@pytest.mark.parametrize("ids", ["explicit", "base"])
def test_row_table_batches_stay_equal(cuda, sizes, ids):
    """Bags of partial tiles and ragged batches (even of whole-tile bags) keep the row table."""
    both_paths(cuda, sizes, 5, 2, ids=ids)


def test_bag_above_lds_cap(cuda):
    """Uniform bags of 33 whole tiles (4,224 > 4,096 rows): logits through the global workspace,
    row-table launch."""
    both_paths(cuda, [4224] * 2, 2, 2)


@pytest.mark.parametrize("N,T", [(128, 5), (256, 3), (2048, 3), (200, 3)])
def test_shared_heads_on_the_forced_tile(cuda, N, T):
    """Shared heads fuse on the 8-wave tile when the gate is forced (gate="pipe"): every class per
    wave, head vectors from global memory, affine and row-table rows."""
    both_paths(cuda, [N] * 3, T, 2, shared=True)


@pytest.mark.parametrize("N,T,C,D", [(256, 3, 2, 128), (128, 5, 4, 64), (200, 3, 2, 128)])
def test_fp32_and_four_classes(cuda, N, T, C, D):
    both_paths(cuda, [N] * 3, T, C, dtype=torch.float32, D=D)


def test_affine_rows_against_oracle(cuda):
    """3 bags of N = 256, T = 5 (two tiles per t-group, one region per bag), bf16 separate heads:
    the affine launch against the reference restatement (mcdo_ref, model.py:280-316) on the same
    bf16 operands with the kernel's own Philox masks, at the bounds of tests/test_gpu_parity.py."""
    from test_gpu_parity import TOL_BF16_IN
    N, B, T, seed = 256, 3, 5, 321
    sd = synthetic.head_state_dict(12, C=2, shared=False)
    Hs = [synthetic.bf16_round(synthetic.bag_features(500 + b, N)) for b in range(B)]
    H = torch.from_numpy(np.concatenate(Hs)).to(cuda).bfloat16()
    out = both_paths(cuda, [N] * B, T, 2, ids="base", H=H, sd=sd, seed=seed)
    prm = mcdo_ref.HeadParams(synthetic.head_arrays(synthetic.round_state_dict_bf16(sd), 2, False))
    for b in range(B):
        kF, kA = mcdo_ref.masks_for_bag(seed, 21 + b, T, N, L, 2, 0.1, 0.1)
        Yr, Ar = mcdo_ref.mc_inference(Hs[b], prm, kF, kA, 0.1, 0.1)
        Yr, Ar = Yr.numpy()[:, 0], Ar.numpy()[:, 0]
        o = T * 2 * N * b
        A = out["A"][o:o + T * 2 * N].cpu().numpy().reshape(T, 2, N)
        Am = out["A_mean"][2 * N * b:2 * N * (b + 1)].cpu().numpy().reshape(2, N)
        np.testing.assert_allclose(out["Y"][b].cpu().numpy(), Yr, rtol=0, atol=TOL_BF16_IN["Y"])
        assert np.abs(A - Ar).max() / np.abs(Ar).max() <= TOL_BF16_IN["A"]
        assert np.abs(Am - Ar.mean(0)).max() / np.abs(Ar.mean(0)).max() <= TOL_BF16_IN["A_mean"]
