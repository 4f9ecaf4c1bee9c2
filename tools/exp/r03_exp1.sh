# round 3, experiment 1: tests of the reworked host code, tile-order A/B (isolated warm / cold, and in the step)
cd $GRAFT_REPO_ROOT
O=${O:-/tmp/polus_out}; mkdir -p $O
python3 tools/pp_bench.py --ab POLUS_GEMM_ORDER=0,2,3,4,6 --rounds 5 --iters 10 > $O/r03_order_warm.txt 2>&1 || exit 1
python3 tools/pp_bench.py --ab POLUS_GEMM_ORDER=0,2,3,4,6 --rounds 3 --iters 6 --cold > $O/r03_order_cold.txt 2>&1 || exit 1
for o in 0 4 0 4; do
  POLUS_GEMM_ORDER=$o python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-f32-leg --no-loss100 > $O/r03_bench_order$o.json 2>> $O/r03_bench_order.err || exit 1
  python3 -c "import json;d=json.load(open('$O/r03_bench_order$o.json'));print('order $o', d['ms_per_step'], d['roofline']['avg_launch_us'], d['roofline']['frac'])" >> $O/r03_order_step.txt
done
timeout -k 10 900 python3 -m pytest tests -m gpu -x -q > $O/r03_tests1.log 2>&1
echo "tests rc=$?" >> $O/r03_tests1.log
tail -5 $O/r03_tests1.log; cat $O/r03_order_step.txt
