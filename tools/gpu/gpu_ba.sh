#!/bin/bash
set -o pipefail
export TMPDIR=/tmp
OUT=gpurun_out/${1:-ba}
mkdir -p $OUT
R=$PWD
make -j16 > $OUT/build.log 2>&1 &&
timeout -k 10 600 python -m pytest tests/test_ba_gpu.py -x -q > $OUT/pytest_ba.log 2>&1 &&
OSG_LBA_PROFILE=1 timeout -k 10 300 python bench.py --full --no-cpu --no-stream --steps 50 > $OUT/bench.json 2> $OUT/bench.err &&
cd $TMPDIR && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/prof -o prof -- python3 $R/bench.py --full --no-cpu --no-stream --steps 50 --ba-reps 5 > $R/$OUT/prof.log 2>&1
echo "exit=$?"
