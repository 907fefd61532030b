#!/bin/bash
# bench + rocprofv3 kernel trace of the bench step -> $OUT/<tag>_bench.json.log, <tag>_step_breakdown.txt
set -e
TAG=${1:-r02}
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${JPDSE_OUT_DIR:-$R/out}          # where this script writes its files
mkdir -p "$OUT"
python $R/bench.py --full --no-cpu-baseline > $OUT/${TAG}_bench.json.log 2> $OUT/${TAG}_bench.err
tail -1 $OUT/${TAG}_bench.json.log | cut -c1-400
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_${TAG}
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG} -f csv -- python3 $R/bench.py --steps 8 --warmup 2 --no-cpu-baseline > $OUT/${TAG}_bench_profiled.json.log 2> $OUT/${TAG}_bench_profiled.err
cd $R
python scripts/trace_summary.py $OUT/prof_${TAG} 70 16 > $OUT/${TAG}_step_breakdown.txt
find $OUT/prof_${TAG} -name "*kernel_stats.csv" -exec cp {} $OUT/${TAG}_kernel_stats.csv \;
find $OUT/prof_${TAG} -name "*_kernel_trace.csv" -delete     # large; the summaries stay
head -45 $OUT/${TAG}_step_breakdown.txt
