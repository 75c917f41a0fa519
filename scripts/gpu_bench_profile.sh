#!/bin/bash
# Run on the GPU box: full bench line (with the per-class breakdown) + rocprofv3 kernel-trace summary of a
# short full run.  Outputs go to $OUT_DIR (default bench_out/).
#   bash scripts/gpu_bench_profile.sh <tag> [bench args...]
set -o pipefail
TAG=${1:-run}; shift
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT_DIR:-bench_out}
mkdir -p $OUT
timeout -k 10 400 python -u bench.py --full --breakdown "$@" > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit 1
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$PWD/$OUT/prof_$TAG" -o run --output-format csv \
  -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline "$@" > $OUT/prof_$TAG.log 2>&1
