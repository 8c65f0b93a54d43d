#!/bin/bash
# cumulative stage times of the fused kernel (stop-stage hook), plain runs without a profiler; ST_ARGS = extra bench.py arguments
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}          # where the lines and logs go
mkdir -p $OUT
# needs a profiling build: MCQ_HIPCC_FLAGS=-DMCQ_PROFILE_HOOKS (the stop-stage bits are rejected otherwise)
export MCQ_HIPCC_FLAGS="$MCQ_HIPCC_FLAGS -DMCQ_PROFILE_HOOKS"
for s in 1 2 3 4 5 0; do
  timeout -k 10 400 python3 bench.py --full --steps 12 --warmup 2 --no-cpu-baseline --stop-stage $s $ST_ARGS > $OUT/st_$s.json 2> $OUT/st_$s.err || exit 1
  python3 -c "
import json; d=json.load(open('$OUT/st_$s.json')); print('stop', $s, 'kernel ms %.3f' % d['roofline']['kernel_ms_sum'])"
done
