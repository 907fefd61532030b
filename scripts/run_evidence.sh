#!/bin/bash
# round evidence in one call: the --full bench line (with cpu_baseline), the same command under rocprofv3 --kernel-trace --stats,
# step breakdown, per-layer profile, HBM traffic (two PMC passes).  Outputs under $OUT/<tag>_*.
TAG=${1:-r02}
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${JPDSE_OUT_DIR:-$R/out}          # where this script writes its files
mkdir -p "$OUT"
cd $R
python bench.py --full > $OUT/${TAG}_bench.json.log 2> $OUT/${TAG}_bench.err
tail -1 $OUT/${TAG}_bench.json.log | cut -c1-160
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_${TAG}
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG} -f csv -- python3 $R/bench.py --steps 8 --warmup 2 --no-cpu-baseline > $OUT/${TAG}_bench_profiled.json.log 2> $OUT/${TAG}_bench_profiled.err
cd $R
python scripts/trace_summary.py $OUT/prof_${TAG} 70 16 > $OUT/${TAG}_step_breakdown.txt
find $OUT/prof_${TAG} -name "*kernel_stats.csv" -exec cp {} $OUT/${TAG}_kernel_stats.csv \;
find $OUT/prof_${TAG} -name "*_kernel_trace.csv" -delete
head -3 $OUT/${TAG}_step_breakdown.txt
python scripts/layer_profile.py > $OUT/${TAG}_layer_profile.txt 2>&1
sed -n 3,4p $OUT/${TAG}_layer_profile.txt
bash scripts/run_pmc_hbm.sh
echo evidence done
