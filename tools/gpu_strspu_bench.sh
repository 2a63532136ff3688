#!/bin/bash
# Format 8 beside STRCD, one stream and eight per call (tools/gpu_strspu_bench.py): every GPU step under its own time limit, the
# steps chained, so that a step that fails or hangs starts nothing after it.  Run from the repository root on a machine with an MI355X.
set -o pipefail
OUT=${1:-build/strspu_bench}
mkdir -p "$OUT" &&
timeout -k 10 300 python tools/gpu_strspu_bench.py --streams 1 --steps 60 --out "$OUT/strspu_bench_S1.json" &&
timeout -k 10 300 python tools/gpu_strspu_bench.py --streams 8 --steps 20 --out "$OUT/strspu_bench_S8.json"
