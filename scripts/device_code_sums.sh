#!/bin/bash
# SHA-256 of the gfx950 code object of every kernel object file of a build directory: two builds with equal sums
# run the same device code, whatever their host code does.
# usage: scripts/device_code_sums.sh [build dir, default gnot-replication_amd/csrc/build]
set -euo pipefail
BUILD=${1:-$(dirname "$0")/../gnot-replication_amd/csrc/build}
LLVM=${ROCM_LLVM:-/opt/rocm/llvm/bin}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
for o in "$BUILD"/*.hip.o; do
  n=$(basename "$o" .o)
  "$LLVM/llvm-objcopy" --dump-section .hip_fatbin="$TMP/$n.fatbin" "$o"
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 \
    --input="$TMP/$n.fatbin" --output="$TMP/$n.co"
  printf '%s  %s\n' "$(sha256sum < "$TMP/$n.co" | cut -d' ' -f1)" "$n"
done
