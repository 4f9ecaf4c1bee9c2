cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${O:-/tmp/polus_out}; mkdir -p $O
t0=$(date +%s)
python3 bench.py --full > $O/r04_bench_full.json 2> $O/r04_bench_full.err || { tail -20 $O/r04_bench_full.err; exit 1; }
t1=$(date +%s); echo "wall $((t1 - t0)) s"
python3 - $O/r04_bench_full.json <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
r = d["roofline"]
print(d["value"], d["ms_per_step"], r["frac"], r.get("traffic"), r.get("traffic_note"), r.get("traffic_measurement"))
PY
