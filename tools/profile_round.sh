#!/bin/bash
# GPU box: per-kernel time of the bench command and HBM traffic of every kernel (separate --pmc passes).
set -e
REPO=$PWD
OUT=${TOOL_OUT:-$REPO/tool_out}   # tools/profile_collect.py reads the same directory
mkdir -p $OUT
export TMPDIR=/tmp
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_stats -o k -- python3 $REPO/bench.py --full --steps 20 --warmup 2 --no-cpu --no-concurrent > $OUT/prof_stats.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o k -- python3 $REPO/tools/gpu_prof_driver.py 2 > $OUT/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o k -- python3 $REPO/tools/gpu_prof_driver.py 2 > $OUT/pmc_write.log 2>&1
cd $REPO
tail -2 $OUT/prof_stats.log | cut -c1-400
