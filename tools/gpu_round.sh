#!/bin/bash
# One GPU-box session: tests, bench (--full: with its verification), kernel
# profile.  Every GPU step has its own time limit and the chain stops at the
# first failure.  Logs go to LOGDIR (default build/gpu_logs).
set -o pipefail
cd "$(dirname "$0")/.."
LOGDIR=$(realpath -m "${LOGDIR:-build/gpu_logs}")
mkdir -p "$LOGDIR"
export TMPDIR=/tmp
STAGE=${1:-all}
run() { echo "== $*" ; "$@"; }
if [[ $STAGE == all || $STAGE == test ]]; then
  run timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > "$LOGDIR/pytest_gpu.log" 2>&1 || { tail -50 "$LOGDIR/pytest_gpu.log"; exit 1; }
  tail -5 "$LOGDIR/pytest_gpu.log"
fi
if [[ $STAGE == all || $STAGE == bench ]]; then
  run timeout -k 10 300 python bench.py --full --steps 5 --warmup 2 --verbose > "$LOGDIR/bench.log" 2>&1 || { cat "$LOGDIR/bench.log"; exit 1; }
  cat "$LOGDIR/bench.log"
fi
if [[ $STAGE == all || $STAGE == prof ]]; then
  cd /tmp && run timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$LOGDIR/prof" -o run -- python3 $OLDPWD/bench.py --steps 2 --warmup 1 > "$LOGDIR/prof.log" 2>&1 || { tail -30 "$LOGDIR/prof.log"; exit 1; }
  cd $OLDPWD
  find "$LOGDIR/prof" -name "*stats*" | head
fi
