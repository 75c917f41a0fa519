#!/bin/bash
# GPU box A/B of one tuning knob: parity tests once, then the bench (--full with the per-class breakdown, no
# CPU baseline) twice per value.  Outputs go to $OUT_DIR (default bench_out/).
#   bash scripts/gpu_ab.sh <ENV_VAR> "<v1> <v2> ..." [bench args...]
set -o pipefail
VAR=$1; VALS=$2; shift 2
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT_DIR:-bench_out}
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/tests_ab.log 2>&1
rc=$?
tail -3 $OUT/tests_ab.log
[ $rc -eq 0 ] || exit $rc
for v in $VALS; do
  for i in 1 2; do
    env "$VAR=$v" timeout -k 10 200 python -u bench.py --full --no-cpu-baseline --breakdown "$@" > $OUT/ab_${v}_$i.json 2> $OUT/ab_${v}_$i.err || exit 1
    python3 -c "import json; d=json.load(open('$OUT/ab_${v}_$i.json')); print('$VAR=$v run $i', d['value'], d['ms_per_step'])"
  done
done
