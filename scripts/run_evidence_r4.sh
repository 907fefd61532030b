#!/bin/bash
# round-4 evidence, part 1: the --full bench line (with cpu_baseline), the same command under rocprofv3 --kernel-trace --stats, step
# breakdown, per-layer profiles (global bf16, LocalEnhancer, config 2 fp32), HBM traffic (two PMC passes).  Outputs: $OUT/<tag>_*
TAG=${1:-r04}
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${JPDSE_OUT_DIR:-$R/out}          # where this script writes its files
mkdir -p "$OUT"
cd $R
python bench.py --steps 20 --warmup 5 --full > $OUT/${TAG}_bench.json.log 2> $OUT/${TAG}_bench.err
tail -1 $OUT/${TAG}_bench.json.log | cut -c1-200
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_${TAG}
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG} -f csv -- python3 $R/bench.py --steps 8 --warmup 2 --no-cpu-baseline > $OUT/${TAG}_bench_profiled.json.log 2> $OUT/${TAG}_bench_profiled.err
cd $R
python scripts/trace_summary.py $OUT/prof_${TAG} 80 20 > $OUT/${TAG}_step_breakdown.txt
find $OUT/prof_${TAG} -name "*kernel_stats.csv" -exec cp {} $OUT/${TAG}_kernel_stats.csv \;
rm -rf $OUT/prof_${TAG}
head -3 $OUT/${TAG}_step_breakdown.txt
python scripts/layer_profile.py > $OUT/${TAG}_layer_profile.txt 2>&1
sed -n 3,4p $OUT/${TAG}_layer_profile.txt
python scripts/layer_profile.py --netG local > $OUT/${TAG}_layer_profile_local.txt 2>&1
sed -n 3,4p $OUT/${TAG}_layer_profile_local.txt
python scripts/layer_profile.py --dtype fp32 --width 512 --height 256 --no-vgg --batch 1 > $OUT/${TAG}_layer_profile_fp32.txt 2>&1
sed -n 3,4p $OUT/${TAG}_layer_profile_fp32.txt
bash scripts/run_pmc_hbm.sh
python scripts/make_hbm_table.py ${TAG} > /dev/null
mv profiles/${TAG}_hbm_traffic.txt $OUT/${TAG}_hbm_traffic.txt
cp profiles/hbm_traffic.json $OUT/${TAG}_hbm_traffic.json
rm -rf gpurun_out/pmc_hbm_FETCH_SIZE gpurun_out/pmc_hbm_WRITE_SIZE
echo evidence part 1 done
