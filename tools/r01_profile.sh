# Round-1 measurement set (run on the GPU box from the repo root): bench line, per-kernel stats, HBM traffic.
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${O:-/tmp/polus_out}; mkdir -p $O
python3 bench.py --full > $O/r01_bench_line.json 2> $O/r01_bench.err || exit 1
POLUS_OVERLAP_DW=0 rocprofv3 --kernel-trace --stats --output-format csv -d $O/r01_stats -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $O/r01_stats.log 2>&1 || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/r01_stats_ov -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $O/r01_stats_ov.log 2>&1 || exit 1
POLUS_OVERLAP_DW=0 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/r01_pmc_fetch -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/r01_pmc_fetch.log 2>&1 || exit 1
POLUS_OVERLAP_DW=0 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/r01_pmc_write -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/r01_pmc_write.log 2>&1 || exit 1
python3 tools/kstats.py $O/r01_stats/*/*kernel_stats.csv 8 > $O/r01_step_kernel_stats_summary.txt
python3 tools/kstats.py $O/r01_stats_ov/*/*kernel_stats.csv 8 > $O/r01_step_kernel_stats_overlap_summary.txt
python3 tools/hbm_traffic.py $O/r01_pmc_fetch $O/r01_pmc_write $O/r01_gemm_hbm_traffic.json
cat $O/r01_bench_line.json
