#!/bin/bash
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
OUT=${PCGRL_PROFILE_OUT:-profile_out}
mkdir -p $OUT
for w in C2 C3 C2w C3w C5; do timeout 500 tools/profile_gpu.sh $w trace sq mem; done
timeout 900 tools/profile_gpu.sh C4 trace sq mem
timeout 300 tools/profile_gpu.sh B1 trace
timeout 300 tools/profile_gpu.sh C2 rtrace
for w in C2 C3 C4 C5 C5b B1 K1 C2w C3w; do
  timeout 500 python bench.py --full --workload $w --no-legs > $OUT/bench_$w.json 2> $OUT/bench_$w.err
done
( time timeout 600 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err ) 2> $OUT/bench_default.time
python tools/timeline.py C2 > $OUT/timeline_C2.txt 2>&1
python tools/big_microbench.py 100 100 1024 > $OUT/big_microbench.txt 2>&1
tail -c 400 $OUT/bench_default.json
