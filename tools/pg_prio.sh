#!/usr/bin/env bash
# Pipelined-graph A/B: when the next view's geometry starts (run on the GPU box from the repo root)
set -euo pipefail
out=${LSR_OUT_DIR:-bench_out}
mkdir -p "$out"
export LSR_BENCH_RGB=0
for g in fwd start fwd start; do
    LSR_PG_GEO=$g timeout -k 10 150 python bench.py --full --no-cpu-baseline > "$out/pg_$g.log" 2>&1
    python3 - "$out/pg_$g.log" "$g" <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1])
print(sys.argv[2], d["ms_per_step_forms"])
PY
done
