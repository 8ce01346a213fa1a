#!/bin/bash
# One GPU-box visit: the -m gpu tests, the default bench line with its --full figures, and a single-lane rocprofv3 kernel
# profile whose summaries land in $OUT (default run_out/; copy what should be judged into profiles/).
# Usage: tools/gpu_round.sh TAG [pytest-args]
TAG=$1; shift
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
OUT=${OUT:-run_out}
mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests -m gpu -x -q -s "$@" > $OUT/${TAG}_gputest.log 2>&1
rc=$?
echo "pytest rc=$rc"; grep -E "passed|failed" $OUT/${TAG}_gputest.log | tail -2
grep -E "FAILED|Error" $OUT/${TAG}_gputest.log | head -5
# a time limit (124, 137), an abort (134), a segfault (139) or any other signal: start nothing more on the GPU;
# an ordinary test failure (rc 1) still goes on to the bench line
if [ $rc -ge 124 ]; then echo "pytest ended abnormally (rc=$rc): stopping"; exit $rc; fi
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $OUT/${TAG}_bench.log 2>&1 || exit 1
tail -1 $OUT/${TAG}_bench.log | cut -c1-400
rm -rf $OUT/prof_${TAG}
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG} -- python3 bench.py --lanes 1 --steps 5 --warmup 7 --no-cpu-baseline --no-pcie --no-kernel-events > $OUT/${TAG}_prof.log 2>&1 || exit 1
ST=$(find $OUT/prof_${TAG} -name "*kernel_stats.csv" | head -1); TR=$(find $OUT/prof_${TAG} -name "*kernel_trace.csv" | head -1)
python3 tools/prof_summary.py "$ST" $OUT/${TAG}_kernel_stats.md "${TAG}: bench.py --lanes 1 --steps 5 --warmup 7 (DepthAnythingV2 vitl, batch 8, f16x3), single lane under rocprofv3"
python3 tools/prof_by_grid.py "$TR" $OUT/${TAG}_by_grid.md "${TAG} single-lane by grid" 58
rm -rf $OUT/prof_${TAG}
head -30 $OUT/${TAG}_kernel_stats.md
