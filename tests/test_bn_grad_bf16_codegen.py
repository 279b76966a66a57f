"""Codegen properties DESIGN.md §4 ("Fused bf16 BatchNorm backward") states for
mcgmil_bn_grad_bf16.hip, checked on its device assembly compiled with the library's own flags (hipcc
cross-compiles for gfx950 without a GPU): the source is part of the library; it holds the bf16
instantiations of the shared partial and apply kernels and nothing else (the finalize stays the
fp32 source's one kernel); no kernel uses scratch or spills a vector register; every kernel stays
within 128 vector registers; the apply kernels use no LDS; loads and stores are 16 bytes wide; and
there is no packed-fp32 VALU and no floating-point atomic."""
import os
import re
import subprocess

import pytest

from mcgmil import _build

HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
SRC = "mcgmil_bn_grad_bf16.hip"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("asm") / "mcgmil_bn_grad_bf16.s")
    cmd = [HIPCC, f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", f"-I{_build.INCLUDE}",
           "--cuda-device-only", "-S", "-o", out] + _build.DEVICE_FLAGS + \
        _build.SOURCE_FLAGS.get(SRC, []) + [os.path.join(_build.CSRC, SRC)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    with open(out) as f:
        return f.read()


def _meta(asm):
    """{kernel name: {field: int}} from the code object's metadata."""
    out = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(v) for k, v in re.findall(
            r"\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", block)}
    return out


def test_source_and_headers_are_built_into_the_library():
    assert SRC in _build.SOURCES and SRC in _build.DEPS and "mcgmil_bn_grad_kernels.h" in _build.DEPS
    assert os.path.exists(os.path.join(_build.INCLUDE, "mcgmil_bn_grad_bf16.h"))
    assert os.path.exists(os.path.join(_build.CSRC, "mcgmil_bn_grad_kernels.h"))


def test_kernels_no_scratch_no_spills_and_register_budgets(asm):
    meta = _meta(asm)
    partial = [n for n in meta if "bn_grad_partial_kernel" in n]
    finalize = [n for n in meta if "finalize" in n]
    apply_ = [n for n in meta if "bn_grad_apply_kernel" in n]
    # partial: ReLU or not; apply: (ReLU, dx, dresidual) in the four combinations the launcher uses;
    # no second finalize kernel, and no fp32 instantiation (DF16b: __bf16 in the mangled name)
    assert len(partial) == 2 and len(apply_) == 4 and not finalize and len(meta) == 6, sorted(meta)
    assert all("IDF16b" in n for n in meta), sorted(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)
        assert m["group_segment_fixed_size"] <= 16 * 1024, (name, m)
    for name in apply_:
        assert meta[name]["group_segment_fixed_size"] == 0, (name, meta[name])


def test_wide_accesses_no_packed_fp32_no_float_atomics(asm):
    assert "global_load_dwordx4" in asm and "global_store_dwordx4" in asm       # 16-byte loads and stores
    # x, y, dy, dx and dresidual never move in narrower pieces: the only other global accesses are the
    # partial pass's per-channel sums (one fp32 per thread)
    assert not re.search(r"\bglobal_(load|store)_(ushort|short|sbyte|ubyte|byte|short_d16\w*)\b", asm)
    assert "v_cvt_pk_bf16_f32" in asm                                           # the one rounding, in hardware
    assert not re.search(r"\bv_pk_(fma|add|mul)_f32\b", asm)
    assert not re.search(r"\b(global|flat|ds|buffer)_atomic\w*_f(32|64)\b|\bds_(add|max|min)\w*_f(32|64)\b", asm)
