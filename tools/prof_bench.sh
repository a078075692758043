#!/bin/bash
# GPU box: rocprofv3 kernel stats of a short bench run, per-frame summary -> $OUT/<tag>.txt (OUT: bench_out unless set)
# usage: tools/prof_bench.sh <tag> [steps]
tag=${1:-prof}; steps=${2:-30}
OUT=${OUT:-bench_out}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
mkdir -p $OUT
rm -rf $OUT/$tag
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$tag -o r -- python3 bench.py --steps $steps --warmup 4 --full --no-cpu $BENCH_EXTRA > $OUT/$tag.log 2>&1 || exit 1
python3 tools/prof_summary.py $OUT/$tag $((steps + 16)) > $OUT/$tag.txt
rm -f $OUT/$tag/r_results.db $OUT/$tag/r_kernel_trace.csv
head -${3:-16} $OUT/$tag.txt; tail -1 $OUT/$tag.txt
