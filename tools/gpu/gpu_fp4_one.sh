#!/bin/bash
# FP4 top-2 with one running top-2 pair per query (OSG_TOP2_MFMA_SHAPE=7) against the default: the top-2 GPU
# tests, then the headline step alternating.
set -o pipefail
export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=$R/gpurun_out/${1:-fp4one}
mkdir -p $OUT
cd $R
timeout -k 10 300 python -u -m pytest tests/test_top2_gpu.py -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/pytest_top2.log 2>&1 || { echo "top2 tests failed"; exit 1; }
ARGS="--no-frames --no-ba --no-gba --no-cpu --no-stream --steps 200 --warmup 20"
for sh in 0 7 0 7; do
  OSG_TOP2_MFMA_SHAPE=$sh timeout -k 10 200 python bench.py --full $ARGS --detail $OUT/c2_$sh.json >> $OUT/c2_$sh.jsonl 2>> $OUT/bench.err || exit 1
done
echo "exit=0"
