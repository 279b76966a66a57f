"""Codegen properties DESIGN.md §4 ("fp32 convolution backward on split bf16") states for
mcgmil_conv_grad_x3.hip, checked on its device assembly compiled with the library's own flags
(hipcc cross-compiles for gfx950 without a GPU): no kernel of the file uses scratch or spills a
vector register, the two wgrad_x3_kernel tiles fit the 256 registers their launch bounds (two
waves per SIMD) allow and the reduce kernel 128, the GEMM is on v_mfma_f32_16x16x32_bf16 fed by the
transposed LDS read with no fp32 MFMA, and there is no packed-fp32 VALU and no floating-point
atomic. The LDS is dynamic, so its budget -- two workgroups per CU within the 160 KiB, 73,728 B for
the 128 x 128 tile and 45,056 B for the 64 x 256 one -- is checked on the tile arithmetic the
source states and on the absence of any static LDS."""
import os
import re
import subprocess

import pytest

from mcgmil import _build

HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
SRC = "mcgmil_conv_grad_x3.hip"
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("asm") / "mcgmil_conv_grad_x3.s")
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


def _body(asm, name):
    """The instructions of one kernel: from its label to its .end_amdhsa_kernel / s_endpgm."""
    start = asm.index(f"\n{name}:")
    return asm[start:asm.index("s_endpgm", start)]


def test_source_and_header_are_built_into_the_library():
    assert SRC in _build.SOURCES and SRC in _build.DEPS
    with open(os.path.abspath(_build.__file__)) as f:
        assert "mcgmil_conv_grad_x3.h" in f.read()


def test_no_scratch_no_spills_and_register_budgets(asm):
    meta = _meta(asm)
    wgrad = [n for n in meta if "wgrad_x3_kernel" in n]
    reduce_ = [n for n in meta if "wgrad_x3_reduce_kernel" in n]
    assert len(wgrad) == 2 and len(reduce_) == 1 and len(meta) == 3, sorted(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)        # the stages are dynamic LDS
    for name in wgrad:       # __launch_bounds__(256, 2): two waves per SIMD share 512 registers
        assert meta[name]["vgpr_count"] <= 256, (name, meta[name])
    assert meta[reduce_[0]]["vgpr_count"] <= 128, meta[reduce_[0]]


def test_lds_budget_of_the_two_tiles(asm):
    """DESIGN.md §4's budget: [A hi][A lo][B hi][B lo] of [32][BM + 16] and [32][BN + 16] bf16, two stages
    for the 128 x 128 tile (73,728 B), one for the 64 x 256 tile (45,056 B), two workgroups per CU
    either way. The stages are dynamic LDS, so the code object carries no size (asserted 0 above) and
    the check the compiler makes is the source's static_asserts on Tile<>::STAGE and Tile<>::LDS, the
    constant the launcher passes: the `asm` fixture compiled the file, so they hold. Here the
    figures those static_asserts pin are read back from the source and held to the budget."""
    with open(os.path.join(_build.CSRC, SRC)) as f:
        src = f.read()
    pins = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(
        r"static_assert\(Tile<(\d, \d)>::STAGE \* sizeof\(__bf16\) == (\d+) && Tile<\1>::LDS == (\d+),", src)}
    assert pins == {"2, 2": (36864, 73728), "1, 4": (45056, 45056)}, pins
    assert re.search(r"hipLaunchKernelGGL\(\(wgrad_x3_kernel<WCO, WN>\), [^;]*dim3\(256\), T::LDS, s,", src)

    def stage(bm, bn):
        return 2 * 32 * ((bm + 16) + (bn + 16)) * 2
    assert pins["2, 2"] == (stage(128, 128), 2 * stage(128, 128))
    assert pins["1, 4"] == (stage(64, 256), stage(64, 256))
    for _, lds in pins.values():
        assert 2 * lds <= LDS_PER_CU                                # two workgroups per CU
    assert 2 * (2 * stage(64, 256)) > LDS_PER_CU                    # why the 64 x 256 tile keeps one stage


def test_bf16_mfma_transposed_reads_no_fp32_mfma_no_packed_fp32_no_float_atomics(asm):
    for name in [n for n in _meta(asm) if "wgrad_x3_kernel" in n]:
        body = _body(asm, name)
        assert body.count("v_mfma_f32_16x16x32_bf16") == 48, name   # 16 fragment pairs x 3 terms, one K step
        assert body.count("ds_read_b64_tr_b16") == 32, name         # 4 operands x 4 fragments x 2 reads
        assert "v_mfma_f32_16x16x4_f32" not in body and "v_mfma_f32_16x16x4f32" not in body
    assert not re.search(r"v_mfma_f32_\w+_f32\b", asm) and "v_mfma_f32_16x16x4f32" not in asm
    assert not re.search(r"\bv_pk_(fma|add|mul)_f32\b", asm)
    assert not re.search(r"\b(global|flat|ds|buffer)_atomic\w*_f(32|64)\b|\bds_(add|max|min)\w*_f(32|64)\b", asm)
