#!/bin/bash
# Round-end evidence on the GPU box:  bash tools/profile_round.sh <tag>      (output directory: $OUT, default ./out)
#   1. bench.py --full (default C3) -> $OUT/<tag>_bench_c3.json
#   2. rocprofv3 --kernel-trace --stats of the same command, default streams and --streams 1
# PMC passes are separate (tools/pmc_run.sh).  Summaries: tools/rocprof_summary.py on the merged .db files.
TAG=${1:-r01}
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$(realpath -m ${OUT:-$R/out})
export TMPDIR=/tmp
mkdir -p $OUT
cd $R
python bench.py --full > $OUT/${TAG}_bench_c3.json 2> $OUT/${TAG}_bench_c3.err
tail -c 600 $OUT/${TAG}_bench_c3.json
cd /tmp
rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_default -o ${TAG}_default -- python $R/bench.py --full --no-cpu-baseline --no-extras > /dev/null 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_streams1 -o ${TAG}_streams1 -- python $R/bench.py --full --no-cpu-baseline --no-extras --streams 1 > /dev/null 2>&1
ls $OUT/prof_${TAG}_default $OUT/prof_${TAG}_streams1
