#!/bin/bash
# PMC counter passes over a short full bench run (one rocprofv3 --pmc pass per counter group).  Outputs go to
# $OUT_DIR (default bench_out/).
#   BENCH_ARGS="--fp32-only" bash scripts/gpu_pmc.sh <tag> "<counters pass 1>" "<counters pass 2>" ...
set -o pipefail
TAG=${1:-pmc}; shift
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT_DIR:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
i=0
for C in "$@"; do
  i=$((i+1))
  timeout -s KILL 150 rocprofv3 --pmc $C --output-format csv -d "$PWD/$OUT/pmc_${TAG}_$i" -o run \
    -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline ${BENCH_ARGS} > $OUT/pmc_${TAG}_$i.log 2>&1 || exit 1
done
