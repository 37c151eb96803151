#!/bin/bash
# Artefacts behind the numbers of a round (run on the MI355X box from the repo root): full bench line + per-launch table, rocprofv3
# kernel stats of the same command (3 streams, and 1 stream for attribution), PMC traffic of the conv kernels (separate passes),
# per-layer tables of the Winograd kernels, SQ counters.      tools/final_profiles.sh <tag> [outdir, default build/profiles/<tag>]
set -x
T=${1:-r6}
OUT=$(realpath -m ${2:-build/profiles/$T}); mkdir -p $OUT
python bench.py --full --detail $OUT/detail.json > $OUT/bench_line.json 2> $OUT/bench_err.log && cut -c1-200 $OUT/bench_line.json
R=$(pwd); cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o f32w -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-configs --no-cpu-baseline --no-io --no-clock-probes --modes '' > $OUT/prof_bench.json 2> $OUT/prof_err.log
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_s1 -o f32w_s1 -- python3 $R/bench.py --full --steps 3 --warmup 1 --streams 1 --no-configs --no-cpu-baseline --no-io --no-clock-probes --modes '' > $OUT/prof_s1_bench.json 2> $OUT/prof_s1_err.log
cd $R
bash tools/pmc_traffic.sh $OUT/pmc f32w > $OUT/pmc.log 2>&1; tail -8 $OUT/pmc.log
# (per-layer tables, SQ counters, the direct-form training line: tools/final_profiles_b.sh <tag>, a GPU call of its own)
ls $OUT
