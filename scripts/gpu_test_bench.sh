#!/bin/bash
# GPU box: parity tests, then full bench + rocprofv3 summary.  Outputs go to $OUT_DIR (default bench_out/).
#   bash scripts/gpu_test_bench.sh <tag> [bench args]
set -o pipefail
TAG=${1:-run}; shift
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT_DIR:-bench_out}
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/tests_$TAG.log 2>&1
rc=$?
tail -3 $OUT/tests_$TAG.log
[ $rc -eq 0 ] || exit $rc
bash scripts/gpu_bench_profile.sh "$TAG" "$@"
