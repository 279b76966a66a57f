"""Codegen of the scoring phase of the launch bench.py times, gate_fused_kernel<bf16, 2, 2, separate
heads> (mcgmil_kernels.h finish_scores, affine launch), on the device assembly of mcgmil_fused.hip
compiled with the library's own flags (the recipe of tests/test_codegen_guard.py):

* the scoring block -- from the s_barrier that follows the tile loop's last v_exp_f32 (the epilogue's;
  finish_scores' barrier) to the next s_barrier in the text -- holds at most 4 v_mad_u64_u32. The
  parent of this change had 22 there: a whole Philox4x32-10 per output for one attention keep
  decision, which now comes from the region's keep bits in LDS (fill_fused_const);
* no branch of that block goes back to a label inside it: the rolled partial-score sum (an unrolled
  loop and its remainder loop in the parent) is gone. (The block also holds the tile loop's own back
  edges, whose targets lie before it: the next barrier in the text is the one after the tile loop.)
* the K loop, the loop body with 66 MFMAs (two K steps), keeps its instruction counts, and the
  kernel its register budget: the scoring changes must not move the loop.
"""
import re

from test_codegen_guard import FUSED, fused_asm, kernel_meta  # noqa: F401  (fused_asm: fixture)

PARENT_SCORING_MAD64 = 22
KLOOP_COUNTS = {"v_mfma_f32_16x16x32_bf16": 66, "v_mad_u64_u32": 34, "ds_read_b128": 20,
                "buffer_load_dwordx4": 8, "global_load_dwordx4": 2, "ds_write_b128": 2, "s_barrier": 2}
BRANCH = re.compile(r"s_c?branch\w*\s+(\S+)")


def _body(text, sym):
    i = text.index("\n" + sym + ":")
    j = text.index(".Lfunc_end", i)
    return [x.split(";")[0].strip() for x in text[i:j].split("\n")]


def _loops(lines):
    """(first, last) line of every backward branch's span: label .. branch."""
    labels = {x[:-1]: k for k, x in enumerate(lines) if x.endswith(":")}
    out = []
    for k, x in enumerate(lines):
        m = BRANCH.match(x)
        if m and labels.get(m.group(1), k) < k:
            out.append((labels[m.group(1)], k))
    return out


def _k_loop(lines):
    found = [(a, b) for a, b in _loops(lines) if sum(x.startswith("v_mfma") for x in lines[a:b + 1]) == 66]
    assert len(found) == 1, found
    return found[0]


def _scoring_block(lines):
    ka, kb = _k_loop(lines)
    # the tile loop: the innermost loop around the K loop; its last v_exp_f32 is the epilogue's
    ta, tb = min(((a, b) for a, b in _loops(lines) if a < ka and b > kb), key=lambda ab: ab[1] - ab[0])
    last_exp = max(k for k in range(ta, tb + 1) if lines[k].startswith("v_exp_f32"))
    assert last_exp > kb
    b1 = next(k for k in range(last_exp, len(lines)) if lines[k].startswith("s_barrier"))
    b2 = next(k for k in range(b1 + 1, len(lines)) if lines[k].startswith("s_barrier"))
    return b1, b2


def test_scoring_block_draws_no_philox_and_has_no_loop(fused_asm):
    lines = _body(fused_asm, FUSED)
    b1, b2 = _scoring_block(lines)
    mad64 = sum(1 for x in lines[b1:b2] if x.startswith("v_mad_u64_u32"))
    print(f"scoring block: lines {b1}..{b2}, {mad64} v_mad_u64_u32 (parent {PARENT_SCORING_MAD64})")
    assert mad64 <= 4, mad64
    inner = [(a, b) for a, b in _loops(lines) if b1 < a and b < b2]
    assert not inner, f"backward branches inside the scoring block: {inner}"


def test_k_loop_counts_and_registers(fused_asm):
    lines = _body(fused_asm, FUSED)
    ka, kb = _k_loop(lines)
    body = [x.split()[0] for x in lines[ka:kb + 1] if x and not x.endswith(":")]
    counts = {op: body.count(op) for op in KLOOP_COUNTS}
    print("K loop:", counts)
    assert counts == KLOOP_COUNTS
    assert sum(1 for x in body if x.startswith("v_mfma")) == 66
    assert kernel_meta(fused_asm, FUSED, "num_vgpr") + kernel_meta(fused_asm, FUSED, "num_agpr") <= 256
    assert kernel_meta(fused_asm, FUSED, "private_seg_size") == 0
