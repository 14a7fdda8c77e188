#!/bin/bash
# rocprofv3 kernel-trace summary of the full bench command (the numbers DESIGN.md / profiles/ quote), then the full bench line without the profiler.
# usage (GPU box): bash tools/prof_bench.sh r01g        -- writes under prof_out/<tag>/ (PROF_OUT=<dir> to change)
tag=${1:-prof}
cd "$(dirname "$0")/.." && export TMPDIR=${TMPDIR:-/tmp}
out=${PROF_OUT:-prof_out}/$tag
mkdir -p $out
rocprofv3 --kernel-trace --stats -d $out -o $tag --output-format csv -- python3 bench.py --full > $out/bench_under_rocprof.json 2> $out/rocprof.log
python3 bench.py --full > $out/bench.json 2> $out/bench.err
tail -1 $out/bench.json
