set -x
cd "$(dirname "$0")/../.."
O=${PCGRL_PROFILE_OUT:-profile_out}/r5b
mkdir -p $O
(timeout 1800 python -m pytest tests/test_gpu_parity.py tests/test_gpu_round5.py -x -q) > $O/pytest_parity5.txt 2>&1
(timeout 600 python bench.py --full --workload B1 --steps 50 --warmup 10 --no-cpu-baseline --no-legs --steady-warmup 7000) > $O/bench_B1g.json 2> $O/bench_B1g.err
(timeout 300 python tools/probe/big_prof.py 50 7000) > $O/big_prof8.txt 2>&1
tail -n 5 $O/pytest_parity5.txt $O/big_prof8.txt
python - <<PY
import json
d=json.loads(open("$O/bench_B1g.json").read().strip().splitlines()[-1])
print("B1", d["value"], d["ms_per_step"], d["steady_state"]["value"], d["steady_state"]["ms_per_step"])
PY
