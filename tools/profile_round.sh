#!/bin/bash
# Round profile of the bench workload: (1) the bench line itself (--full: in-run PMC traffic, parity gate, CPU baseline),
# (2) rocprofv3 --kernel-trace --stats of the plain bench command (no child processes under the profiler).
# usage (GPU box): tools/profile_round.sh TAG [OUT]  -> OUT/TAG_bench.json, OUT/TAG_kernel_stats.csv, OUT/TAG_pmc/  (OUT: profile_out/)
R=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:-r2}
OUT=${2:-$R/profile_out}
mkdir -p $OUT && OUT=$(cd $OUT && pwd)
python3 $R/bench.py --full --steps 4 --warmup 1 --keep-pmc $OUT/${TAG}_pmc > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_kt -o run -- python3 $R/bench.py --steps 4 --warmup 1 > $OUT/${TAG}_kt.log 2>&1
cp $OUT/${TAG}_kt/*/run_kernel_stats.csv $OUT/${TAG}_kernel_stats.csv 2>/dev/null || cp $OUT/${TAG}_kt/run_kernel_stats.csv $OUT/${TAG}_kernel_stats.csv
head -8 $OUT/${TAG}_kernel_stats.csv
tail -c 400 $OUT/${TAG}_bench.json
