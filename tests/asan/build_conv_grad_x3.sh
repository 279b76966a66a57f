#!/bin/bash
# Build tests/asan/conv_grad_x3_host_check against mcgmil_conv_grad_x3.hip and the sources it links
# against (mcgmil.hip for the error reporting, mcgmil_fused.hip for mcgmil.hip) with
# AddressSanitizer and UndefinedBehaviorSanitizer on the HOST pass only (-Xarch_host; GPU
# sanitizers are not used).
# Usage: bash tests/asan/build_conv_grad_x3.sh OUT_DIR   (prints the binary path)
set -euo pipefail
OUT=${1:?out dir}
REPO=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$OUT"
SAN="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined"
HIPCC=${ROCM_PATH:-/opt/rocm}/bin/hipcc
objs=()
for f in mcgmil mcgmil_fused mcgmil_conv_grad_x3; do
    # the host pass warns that it does not know the device feature: keep the output, show it on failure
    if ! "$HIPCC" --offload-arch=gfx950 -std=c++17 -O1 -I"$REPO/include" $SAN \
        -Xclang -target-feature -Xclang -packed-fp32-ops \
        -c "$REPO/montecarlo-gated-mil_amd/csrc/$f.hip" -o "$OUT/$f.o" > "$OUT/$f.log" 2>&1; then
        cat "$OUT/$f.log" >&2
        exit 1
    fi
    objs+=("$OUT/$f.o")
done
"$HIPCC" --offload-arch=gfx950 -std=c++17 -O1 -I"$REPO/include" $SAN -x c++ \
    -c "$REPO/tests/asan/conv_grad_x3_host_check.cpp" -o "$OUT/conv_grad_x3_host_check.o"
"$HIPCC" --offload-arch=gfx950 $SAN "${objs[@]}" "$OUT/conv_grad_x3_host_check.o" -o "$OUT/conv_grad_x3_host_check"
echo "$OUT/conv_grad_x3_host_check"
