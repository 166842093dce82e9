# The bench command with --full on the final library: wall time, line size and the figures read first.
# usage: final_bench_check.sh <output directory>
O=${1:?usage: final_bench_check.sh <output directory>}
mkdir -p $O
( time python bench.py --gpus 1 --steps 20 --warmup 5 --full > $O/bench.json 2> $O/bench.err ) 2>&1 | grep real
wc -c $O/bench.json
python - $O/bench.json <<'P'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["roofline"]["frac"], d["lib"], d["alt_cfg3"]["stats_ms"], d["alt_dplda"]["B256_bce"]["ms_per_step"], list(d)[-6:])
P
