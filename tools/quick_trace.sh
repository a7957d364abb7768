#!/usr/bin/env bash
# Kernel trace of a short bench run (run on the GPU box from the repo root): $LSR_OUT_DIR (bench_out)/<tag>_qt/
set -euo pipefail
tag=${1:-qt}
export TMPDIR=/tmp
out=${LSR_OUT_DIR:-$(pwd)/bench_out}
mkdir -p "$out"
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$out/${tag}_qt" -o trace -- \
    python3 "$(pwd)/bench.py" --full --steps 20 --warmup 5 --no-cpu-baseline > "$out/${tag}_qt.log" 2>&1
