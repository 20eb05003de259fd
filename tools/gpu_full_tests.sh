#!/bin/bash
# the whole GPU suite in one process, then the full bench (no CPU baseline)
set -o pipefail
OUT=${TOOL_OUT:-tool_out}
mkdir -p $OUT
python -m pytest tests -m gpu -x -q > $OUT/gpu_all.log 2>&1; echo "gpu tests rc=$?"; tail -4 $OUT/gpu_all.log
python bench.py --full --no-cpu > $OUT/bench_full.log 2>&1; echo "bench rc=$?"; tail -1 $OUT/bench_full.log | cut -c1-6000
