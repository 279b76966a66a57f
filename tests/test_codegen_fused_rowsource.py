"""Codegen of the launch bench.py times, gate_fused_kernel<bf16, 2, 2, separate heads> (the affine
launch of mcgmil_kernels.h fused_region), on the device assembly of mcgmil_fused.hip compiled with
the library's own flags (the recipe of tests/test_codegen_guard.py):

* no flat_load_ instruction: the region constants, the logits and the classifier projections are
  all read as LDS (ds_read), never through a generic pointer. The parent of this change had 73
  (5 per tile for the Region struct, the rest in the softmax phase).
* v_rcp_iflag_f32, the head of every 32-bit integer division chain: 4, all in decode_region before
  the tile loop. The parent's assembly had 8 by the same count: those 4 plus 4 in the tile loop
  (region_tile before and after the row-table barrier, r / Nb in the row table, q / (D / 16) in the
  epilogue). The assertion is the parent's count less those four.
"""
import re

from test_codegen_guard import FUSED, fused_asm, kernel_meta  # noqa: F401  (fused_asm: fixture)

PARENT_RCP_IFLAG = 8
TILE_LOOP_DIVISIONS = 4


def _body(text, sym):
    i = text.index("\n" + sym + ":")
    j = text.index(".Lfunc_end", i)
    return [x.split(";")[0].strip() for x in text[i:j].split("\n")]


def test_headline_fused_kernel_reads_no_generic_pointer(fused_asm):
    found = [x for x in _body(fused_asm, FUSED) if x.startswith("flat_load_")]
    assert not found, f"{len(found)} flat_load instructions in {FUSED}"


def test_headline_fused_kernel_has_no_division_in_the_tile_loop(fused_asm):
    lines = _body(fused_asm, FUSED)
    n = sum(1 for x in lines if re.match(r"v_rcp_iflag_f32\b", x))
    assert n <= PARENT_RCP_IFLAG - TILE_LOOP_DIVISIONS, n
    # and none of them after the tile loop's first MFMA
    first_mfma = next(k for k, x in enumerate(lines) if x.startswith("v_mfma"))
    assert not [x for x in lines[first_mfma:] if re.match(r"v_rcp_iflag_f32\b", x)]
    assert kernel_meta(fused_asm, FUSED, "private_seg_size") == 0
