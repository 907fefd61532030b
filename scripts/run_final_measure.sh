set -e
R=$GRAFT_REPO_ROOT
OUT=${JPDSE_OUT_DIR:-$R/out}          # where this script writes its files
mkdir -p "$OUT"
python -m pytest tests -m gpu -x -q 2>&1 | tail -3
python __graft_entry__.py smoke 2>&1 | tail -2
python bench.py --full > $OUT/bench_final.json.log 2> $OUT/bench_final.err
tail -1 $OUT/bench_final.json.log
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_final -f csv -- python3 $R/bench.py --steps 8 --warmup 2 --no-cpu-baseline > $OUT/bench_final_profiled.json.log 2> $OUT/bench_final_profiled.err
cd $R
python scripts/trace_summary.py $OUT/prof_final 60 12 > $OUT/step_breakdown_final.txt
tail -1 $OUT/bench_final_profiled.json.log | cut -c1-200
