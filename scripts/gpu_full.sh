#!/bin/bash
# the round-end sequence: GPU suite, smoke(), the full bench line; writes under ${OUT:-results}/; every step has its own time
# limit and the first step that fails ends the sequence
set -e -o pipefail
OUT=${OUT:-results}; mkdir -p "$OUT"
timeout -k 10 1800 python -m pytest tests -x -q -m gpu 2>&1 | tail -5
timeout -k 10 600 python __graft_entry__.py smoke 2>&1 | tail -3
timeout -k 10 900 python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.err" || { tail -3 "$OUT/bench_default.err"; exit 1; }
tail -c 3000 "$OUT/bench_default.json"; tail -3 "$OUT/bench_default.err"
