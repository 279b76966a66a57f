"""Codegen properties DESIGN.md §4 ("Fused bf16 stem BatchNorm / pool backward") states for
mcgmil_pool_grad_bf16.hip, checked on its device assembly compiled with the library's own flags
(hipcc cross-compiles for gfx950 without a GPU): the source is part of the library; it holds the
bf16 instantiations of the shared forward, partial and apply kernels and nothing else (the finalize
stays mcgmil_bn_grad.hip's one kernel); no kernel uses scratch or spills a vector register; every
kernel stays within its vector-register budget; only the partial kernel uses LDS; z, dy and dz move
in 16-byte loads and stores and the codes in 8-byte ones; and there is no packed-fp32 VALU and no
floating-point atomic.

Measured with this build (ROCm 7.2, gfx950), VGPRs / scratch bytes / LDS bytes:
  bn_pool_argmax_kernel<__bf16, relu>    59 / 0 / 0         (fp32: 62)
  bn_pool_argmax_kernel<__bf16, no relu> 56 / 0 / 0         (fp32: 60)
  bn_pool_grad_kernel<__bf16, false>     86 / 0 / 16,384    (the partial sums; fp32: 90)
  bn_pool_grad_kernel<__bf16, true>      84 / 0 / 0         (the apply pass; fp32: 88)
The budgets below are those figures rounded up to the next occupancy step of a 512-register SIMD
(64 registers: 8 waves per SIMD; 96: 5 waves), the steps the fp32 instantiations sit on as well."""
import os
import re
import subprocess

import pytest

from mcgmil import _build

HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
SRC = "mcgmil_pool_grad_bf16.hip"
BUDGET = {"bn_pool_argmax_kernel": 64, "bn_pool_grad_kernel": 96}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("asm") / "mcgmil_pool_grad_bf16.s")
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
    """The instructions of one kernel: from its label to its s_endpgm."""
    start = asm.index(f"\n{name}:")
    return asm[start:asm.index("s_endpgm", start)]


def test_source_and_headers_are_built_into_the_library():
    assert SRC in _build.SOURCES and SRC in _build.DEPS and "mcgmil_pool_grad_kernels.h" in _build.DEPS
    assert os.path.exists(os.path.join(_build.INCLUDE, "mcgmil_pool_grad_bf16.h"))
    assert os.path.exists(os.path.join(_build.CSRC, "mcgmil_pool_grad_kernels.h"))


def test_kernels_no_scratch_no_spills_and_register_budgets(asm):
    meta = _meta(asm)
    forward = [n for n in meta if "bn_pool_argmax_kernel" in n]
    grad = [n for n in meta if "bn_pool_grad_kernel" in n]
    finalize = [n for n in meta if "finalize" in n]
    # forward: ReLU or not; backward: the partial sums and the apply pass; no second finalize kernel,
    # and no fp32 instantiation (DF16b: __bf16 in the mangled name)
    assert len(forward) == 2 and len(grad) == 2 and not finalize and len(meta) == 4, sorted(meta)
    assert all("IDF16b" in n for n in meta), sorted(meta)
    for name, m in meta.items():
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        budget = next(v for k, v in BUDGET.items() if k in name)
        assert m["vgpr_count"] <= budget, (name, m, budget)
    # LDS in the partial kernel alone: [2][256 * 8] fp32
    lds = sorted(m["group_segment_fixed_size"] for m in meta.values())
    assert lds == [0, 0, 0, 16 * 1024], lds
    partial = [n for n in grad if meta[n]["group_segment_fixed_size"]]
    assert len(partial) == 1 and "Lb0E" in partial[0], partial          # APPLY == false
    for name in meta:
        assert bool(re.search(r"\bds_(read|write|load|store)", _body(asm, name))) == (name == partial[0]), name


def test_wide_accesses_no_packed_fp32_no_float_atomics(asm):
    meta = _meta(asm)
    for name in meta:
        body = _body(asm, name)
        assert "global_load_dwordx4" in body, name                              # z / dy: 16 bytes, 8 bf16
        # z, y, dy and dz never move in narrower pieces than a thread's 8 channels
        assert not re.search(r"\bglobal_(load|store)_(ushort|short|sbyte|ubyte|byte|short_d16\w*)\b", body), name
    for name in (n for n in meta if "bn_pool_argmax_kernel" in n):
        body = _body(asm, name)
        assert "global_store_dwordx4" in body and "global_store_dwordx2" in body, name     # y, and the 8 codes
        assert "v_cvt_pk_bf16_f32" in body, name                                # the one rounding, in hardware
    for name in (n for n in meta if "bn_pool_grad_kernel" in n):
        assert "global_load_dwordx2" in _body(asm, name), name                  # the 8 codes of a window
    apply_ = next(n for n in meta if "bn_pool_grad_kernel" in n and "Lb1E" in n)
    assert "global_store_dwordx4" in _body(asm, apply_) and "v_cvt_pk_bf16_f32" in _body(asm, apply_)
    assert not re.search(r"\bv_pk_(fma|add|mul)_f32\b", asm)
    assert not re.search(r"\b(global|flat|ds|buffer)_atomic\w*_f(32|64)\b|\bds_(add|max|min)\w*_f(32|64)\b", asm)
