"""Codegen properties DESIGN.md §4 ("fp32 block convolutions on split bf16") states for
mcgmil_conv32x3.hip, checked on its device assembly compiled with the library's own flags (hipcc
cross-compiles for gfx950 without a GPU): no conv32x3_kernel variant uses scratch or spills a
vector register, all fit the 256 registers their launch bounds (two waves per SIMD) allow, the
GEMM is on v_mfma_f32_16x16x32_bf16 with no fp32 MFMA left, and there is no atomic."""
import os
import re
import subprocess

import pytest

from mcgmil import _build

HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
SRC = "mcgmil_conv32x3.hip"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("asm") / "mcgmil_conv32x3.s")
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
    assert SRC in _build.SOURCES and SRC in _build.DEPS
    assert "mcgmil_conv_tile_stats.h" in _build.DEPS            # shared with mcgmil_conv32.hip
    assert os.path.exists(os.path.join(_build.CSRC, "mcgmil_conv_tile_stats.h"))
    assert _build.SOURCE_FLAGS.get(SRC, []) == _build.SOURCE_FLAGS.get("mcgmil_conv32.hip", [])


def test_no_scratch_no_spills_and_register_budgets(asm):
    meta = _meta(asm)
    kernels = {n: m for n, m in meta.items() if "conv32x3_kernel" in n and "pack_" not in n}
    # two tile shapes x with / without the input BatchNorm x with / without statistics, and the pack kernel
    assert len(kernels) == 8 and len(meta) == 9 and any("pack_conv32x3_kernel" in n for n in meta), sorted(meta)
    for name, m in meta.items():
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
    for name, m in kernels.items():
        assert m["vgpr_count"] <= 256, (name, m)     # __launch_bounds__(256, 2): two waves per SIMD share 512
        assert m["group_segment_fixed_size"] == 0, (name, m)      # dynamic LDS only: the two stages


def test_bf16_mfma_only_and_no_atomics(asm):
    assert "v_mfma_f32_16x16x32_bf16" in asm
    assert "v_mfma_f32_16x16x4_f32" not in asm
    assert not re.search(r"\b(global|flat|buffer)_atomic", asm)      # no atomics at all: every element has one writer
