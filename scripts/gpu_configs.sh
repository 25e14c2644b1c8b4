#!/bin/bash
# GPU tests, configs 2 and 4, headline bench. Logs go to $OUT (default bench_out/).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 300 python -m pytest tests -m gpu -x -q > "$OUT/pytest_gpu.log" 2>&1 &&
timeout -k 10 300 python -m mxstream.models.bench_configs --config 2 --steps 20 --warmup 5 > "$OUT/cfg2.log" 2>&1 &&
timeout -k 10 400 python -m mxstream.models.bench_configs --config 4 --steps 30 --warmup 30 > "$OUT/cfg4.log" 2>&1 &&
timeout -k 10 300 python bench.py --full --steps 24 --warmup 6 > "$OUT/bench.log" 2>&1
