#!/bin/bash
# rocprofv3 kernel stats of a short full bench run with the weight-gradient side stream disabled
# (uncontended per-kernel durations).  Outputs go to $OUT_DIR (default bench_out/).
#   bash scripts/gpu_prof_serial.sh <tag>
set -o pipefail
TAG=${1:-serial}
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT_DIR:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$PWD/$OUT/prof_$TAG" -o run \
  --output-format csv -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_$TAG.log 2>&1
