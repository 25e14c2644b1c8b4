#!/bin/bash
# Pinned slab pool for fired rows: GPU tests, headline bench x2, config 4 and 6, kernel trace.
# Logs go to $OUT (default bench_out/).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
ROOT=$(pwd)
mkdir -p "${OUT:=bench_out}"
OUT=$(cd "$OUT" && pwd)  # absolute: the profile below runs from another directory
export PYTHONPATH=$PWD
timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/pool_tests.log" 2>&1 &&
timeout -k 10 300 python bench.py --full --steps 24 --warmup 6 > "$OUT/pool_bench_1.log" 2>&1 &&
timeout -k 10 300 python bench.py --full > "$OUT/pool_bench_2.log" 2>&1 &&
timeout -k 10 400 python -m mxstream.models.bench_configs --config 4 --steps 30 --warmup 30 > "$OUT/pool_cfg4.log" 2>&1 &&
timeout -k 10 300 python -m mxstream.models.bench_configs --config 6 --steps 20 --warmup 14 > "$OUT/pool_cfg6.log" 2>&1 &&
cd /tmp && export TMPDIR=/tmp &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/pool_prof" -o run -- \
  python3 "$ROOT/bench.py" --steps 24 --warmup 3 > "$OUT/pool_prof.log" 2>&1
