#!/bin/bash
# Round-end evidence on the GPU box:  bash tools/gpu_round.sh <tag>      (output directory: $OUT, default ./out)
#   bench.py --full (driver settings) -> $OUT/<tag>_bench_c3.json
#   rocprofv3 --kernel-trace --stats of the same command (default streams and --streams 1) -> <tag>_c3_kernel_stats_*.md
#   PMC passes (tools/pmc_run.sh) -> <tag>_pmc_c3.json, stamped with lr_version()
TAG=${1:-r05}
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$(realpath -m ${OUT:-$R/out})
export OUT
export TMPDIR=/tmp
mkdir -p $OUT
cd $R
python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench_c3.json 2> $OUT/${TAG}_bench_c3.err
tail -c 300 $OUT/${TAG}_bench_c3.err
for wl in c2 c3box c4shape c5shape ld512; do
  python bench.py --workload $wl --steps 5 --warmup 2 --full --no-cpu-baseline --no-extras > $OUT/${TAG}_bench_${wl}.json 2>/dev/null
done
# single-stream kernel statistics of the 512^2 dense shape (one view alone on the GPU: what the training loop sees)
(cd /tmp && rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_c5shape -o ${TAG}_c5shape -- python $R/bench.py --workload c5shape --full --no-cpu-baseline --no-extras --steps 5 --warmup 2 --sustain-seconds 0 --streams 1 > /dev/null 2>&1)
db=$(ls $OUT/prof_${TAG}_c5shape/*.db 2>/dev/null | head -1)
[ -n "$db" ] && python tools/rocprof_summary.py $db $OUT/${TAG}_c5shape_kernel_stats_streams1.md "rocprofv3 --kernel-trace --stats -- python bench.py --workload c5shape --full --no-cpu-baseline --no-extras --steps 5 --warmup 2 --sustain-seconds 0 --streams 1"
rm -rf $OUT/prof_${TAG}_c5shape
cd /tmp
CMD="python bench.py --full --no-cpu-baseline --no-extras --steps 10 --warmup 3 --sustain-seconds 0"
rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_default -o ${TAG}_default -- python $R/bench.py --full --no-cpu-baseline --no-extras --steps 10 --warmup 3 --sustain-seconds 0 > /dev/null 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_streams1 -o ${TAG}_streams1 -- python $R/bench.py --full --no-cpu-baseline --no-extras --steps 10 --warmup 3 --sustain-seconds 0 --streams 1 > /dev/null 2>&1
cd $R
for v in default streams1; do
  db=$(ls $OUT/prof_${TAG}_$v/*.db 2>/dev/null | head -1)
  [ -n "$db" ] && python tools/rocprof_summary.py $db $OUT/${TAG}_c3_kernel_stats_$v.md "rocprofv3 --kernel-trace --stats -- $CMD$([ $v = streams1 ] && echo ' --streams 1')"
done
bash tools/pmc_run.sh $TAG > $OUT/pmc_${TAG}.log 2>&1
python tools/pmc_summary.py $OUT/pmc_$TAG $OUT/${TAG}_pmc_c3.json "tools/pmc_run.sh $TAG"
rm -rf $OUT/pmc_$TAG/*/*.csv $OUT/pmc_$TAG/*/*.db
# the shapes LucidDreamer itself runs (512^2, every Gaussian in view) and the dense 1080p cloud, same counters
for wl in c5shape c3box; do
  bash tools/pmc_run.sh ${TAG}_$wl --workload $wl > $OUT/pmc_${TAG}_$wl.log 2>&1
  python tools/pmc_summary.py $OUT/pmc_${TAG}_$wl $OUT/${TAG}_pmc_$wl.json "tools/pmc_run.sh ${TAG}_$wl --workload $wl"
  rm -rf $OUT/pmc_${TAG}_$wl/*/*.csv $OUT/pmc_${TAG}_$wl/*/*.db
done
rm -rf $OUT/prof_${TAG}_default $OUT/prof_${TAG}_streams1
head -30 $OUT/${TAG}_c3_kernel_stats_streams1.md
python - <<PY
import json
d=json.loads(open('$OUT/${TAG}_bench_c3.json').read().strip().splitlines()[-1])
print(d['value'], d['sustained'], d['entry_points'])
print(d['roofline']['stage_ms_per_view'])
PY
