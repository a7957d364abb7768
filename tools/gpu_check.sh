#!/usr/bin/env bash
# GPU suite + two bench runs (run on the GPU box from the repo root); outputs under $LSR_OUT_DIR (bench_out/).
set -euo pipefail
out=${LSR_OUT_DIR:-bench_out}
mkdir -p "$out"
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$out/gpu_tests.log" 2>&1
timeout -k 10 150 python bench.py --full --no-cpu-baseline > "$out/bench.log" 2>&1
timeout -k 10 150 python bench.py --full --no-cpu-baseline > "$out/bench2.log" 2>&1
