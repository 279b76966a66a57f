"""Codegen properties DESIGN.md §4 ("Head backward") states for mcgmil_grad.hip, checked on its
device assembly compiled with the library's own flags (hipcc cross-compiles for gfx950 without a
GPU): no kernel of the file uses scratch or spills a vector register, grad_rows_kernel (8 waves,
two per SIMD) fits 256 VGPRs, no packed-fp32 VALU, no floating-point atomic, and the GEMMs are on
v_mfma_f32_16x16x4_f32."""
import os
import re
import subprocess

import pytest

from mcgmil import _build

HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("asm") / "mcgmil_grad.s")
    cmd = [HIPCC, f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", f"-I{_build.INCLUDE}",
           "--cuda-device-only", "-S", "-o", out] + _build.DEVICE_FLAGS + \
        _build.SOURCE_FLAGS.get("mcgmil_grad.hip", []) + [os.path.join(_build.CSRC, "mcgmil_grad.hip")]
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


def test_no_scratch_and_no_vector_spills(asm):
    meta = _meta(asm)
    names = " ".join(meta)
    for k in ("grad_rows_kernelILi1E", "grad_rows_kernelILi2E", "grad_weights_kernel", "grad_reduce_kernel",
              "grad_ra_kernel", "grad_pack_kernel"):
        assert k in names, k
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)


def test_fp32_mfma_no_packed_fp32_no_float_atomics(asm):
    assert "v_mfma_f32_16x16x4_f32" in asm or "v_mfma_f32_16x16x4f32" in asm
    assert not re.search(r"\bv_pk_(fma|add|mul)_f32\b", asm)
    assert not re.search(r"\b(global|flat|ds|buffer)_atomic\w*_f(32|64)\b|\bds_(add|max|min)\w*_f(32|64)\b", asm)
