#!/bin/bash
# kernel-trace statistics of the full bench command only (the quick look while iterating): prof_out/<tag>_kernel_stats.csv (PROF_OUT=<dir> to change)
tag=${1:-q}
cd "$(dirname "$0")/.." && export TMPDIR=${TMPDIR:-/tmp}
top=${PROF_OUT:-prof_out}
out=$top/$tag
mkdir -p $out
rocprofv3 --kernel-trace --stats -d $out/trace -o $tag --output-format csv -- python3 bench.py --full --cpu-seconds 0 ${@:2} > $out/bench_under_rocprof.json 2> $out/rocprof_trace.log
cp $(find $out/trace -name "*kernel_stats.csv" | head -1) $top/${tag}_kernel_stats.csv
head -14 $top/${tag}_kernel_stats.csv
