#!/bin/bash
# GPU box sweep of one environment setting over values, interleaved rounds: bench.py --full (no CPU baseline)
# per value.  Outputs go to $OUT_DIR (default bench_out/).
#   bash scripts/gpu_env_sweep.sh <tag> <rounds> <VAR> "<v1> <v2> ..." [bench args...]
set -o pipefail
TAG=$1; R=$2; VAR=$3; VALS=$4; shift 4
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT_DIR:-bench_out}
mkdir -p $OUT
for i in $(seq 1 $R); do
  for v in $VALS; do
    env "$VAR=$v" timeout -k 10 300 python -u bench.py --full --no-cpu-baseline "$@" > $OUT/${TAG}_${v}_$i.json 2> $OUT/${TAG}_${v}_$i.err || exit 1
    python3 -c "
import json; d=json.load(open('$OUT/${TAG}_${v}_$i.json'))
b=d.get('bf16_mode',{})
print('$VAR=$v run $i', d['value'], d['ms_per_step'], 'bf16', b.get('ms_per_step'))"
  done
done
