"""The bf16x3 convolution weight gradient's C ABI (include/mcgmil_conv_grad_x3.h) under
AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program.

tests/asan/build_conv_grad_x3.sh compiles mcgmil_conv_grad_x3.hip and the sources it links
against with the sanitizers on the host pass only (-Xarch_host; no GPU sanitizer) and links
tests/asan/conv_grad_x3_host_check.cpp, which drives every validation path and the workspace-size
arithmetic (sizes past 32 and 64 bits included) without a GPU. The binary is cached under
build/asan_conv_grad_x3/ (rebuilt when a source is newer)."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "montecarlo-gated-mil_amd", "csrc")
SOURCES = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + \
    [os.path.join(REPO, "include", h) for h in ("mcgmil.h", "mcgmil_features.h", "mcgmil_conv_grad.h",
                                                "mcgmil_conv_grad_x3.h")] + \
    [os.path.join(REPO, "tests", "asan", f) for f in ("conv_grad_x3_host_check.cpp", "build_conv_grad_x3.sh")]


def _binary():
    out = os.path.join(REPO, "build", "asan_conv_grad_x3")
    exe = os.path.join(out, "conv_grad_x3_host_check")
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(s) for s in SOURCES):
        return exe
    subprocess.run(["bash", os.path.join(REPO, "tests", "asan", "build_conv_grad_x3.sh"), out], check=True,
                   capture_output=True, timeout=900)
    return exe


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_conv_grad_x3_capi_host_code_under_asan_ubsan():
    exe = _binary()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failure(s)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
