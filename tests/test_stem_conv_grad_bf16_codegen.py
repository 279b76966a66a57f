"""Codegen properties DESIGN.md §4 ("bf16 stem convolution backward") states for
mcgmil_stem_grad_bf16.hip, checked on its device assembly compiled with the library's own flags
(hipcc cross-compiles for gfx950 without a GPU): no kernel of the file uses scratch or spills a
vector register, the four stem_wgrad_bf16_kernel variants fit the 256 registers their launch bounds
(two waves per SIMD) allow and 64 KB of LDS, the reduce kernel 128 registers, the GEMM is on
v_mfma_f32_16x16x32_bf16, and there is no packed-fp32 VALU and no floating-point atomic."""
import os
import re
import subprocess

import pytest

from mcgmil import _build

HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
SRC = "mcgmil_stem_grad_bf16.hip"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("asm") / "mcgmil_stem_grad_bf16.s")
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


def test_source_and_header_are_built_into_the_library():
    assert SRC in _build.SOURCES and SRC in _build.DEPS
    assert os.path.exists(os.path.join(_build.INCLUDE, "mcgmil_stem_grad_bf16.h"))
    import inspect
    assert "mcgmil_stem_grad_bf16.h" in inspect.getsource(_build._stale)


def test_no_scratch_no_spills_and_register_budgets(asm):
    meta = _meta(asm)
    wgrad = [n for n in meta if "stem_wgrad_bf16_kernel" in n]
    reduce_ = [n for n in meta if "stem_wgrad_bf16_reduce_kernel" in n]
    assert len(wgrad) == 4 and len(reduce_) == 1 and len(meta) == 5, sorted(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
    for name in wgrad:       # __launch_bounds__(256, 2): two waves per SIMD share 512 registers
        assert meta[name]["vgpr_count"] <= 256, (name, meta[name])
        assert meta[name]["group_segment_fixed_size"] <= 64 * 1024, (name, meta[name])
    assert meta[reduce_[0]]["vgpr_count"] <= 128, meta[reduce_[0]]


def test_bf16_mfma_no_packed_fp32_no_float_atomics(asm):
    assert "v_mfma_f32_16x16x32_bf16" in asm
    assert not re.search(r"\bv_pk_(fma|add|mul)_f32\b", asm)
    assert not re.search(r"\b(global|flat|ds|buffer)_atomic\w*_f(32|64)\b|\bds_(add|max|min)\w*_f(32|64)\b", asm)
