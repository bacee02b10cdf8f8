#!/bin/bash
# Quick GPU check after a kernel change: TB kernel + solver tests, a depth
# sweep over the per-rank slab shapes (DEPTHS, default 8,12) and the bench
# with its verification (--full).  Logs go to LOGDIR (default build/gpu_logs).
set -o pipefail
cd "$(dirname "$0")/.."
LOGDIR=${LOGDIR:-build/gpu_logs}
mkdir -p "$LOGDIR"
timeout -k 10 300 python -u -m pytest tests/test_gpu_kernels.py tests/test_gpu_solver.py -x -q \
    --timeout 120 --timeout-method thread > "$LOGDIR/pytest_quick.log" 2>&1 || { tail -30 "$LOGDIR/pytest_quick.log"; exit 1; }
tail -2 "$LOGDIR/pytest_quick.log"
DEPTHS=${DEPTHS:-8,12} bash tools/sweep_depth.sh || exit 1
timeout -k 10 300 python bench.py --full --steps 5 --warmup 2 > "$LOGDIR/bench.log" 2>&1 || { cat "$LOGDIR/bench.log"; exit 1; }
cat "$LOGDIR/bench.log"
