#!/bin/bash
# GPU box iteration: kernel microbenchmark, parity tests, full bench line with the per-class breakdown (no
# CPU baseline, no rocprof).  Outputs go to $OUT_DIR (default bench_out/).
#   bash scripts/gpu_iter.sh <tag> [bench args...]
set -o pipefail
TAG=${1:-it}; shift
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT_DIR:-bench_out}
mkdir -p $OUT
timeout -k 10 120 ./gnot-replication_amd/lib/microbench > $OUT/mb_$TAG.txt 2>&1 || exit 1
cat $OUT/mb_$TAG.txt
timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/tests_$TAG.log 2>&1
rc=$?
tail -3 $OUT/tests_$TAG.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python -u bench.py --full --breakdown --no-cpu-baseline "$@" > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit 1
cat $OUT/bench_$TAG.json; grep breakdown $OUT/bench_$TAG.err
