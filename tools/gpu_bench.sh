#!/bin/bash
# smoke + bench + rocprof kernel trace of the bench command
# (results under $OUT, default bench_out/)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT/prof"
export TMPDIR=/tmp
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { cat "$OUT/smoke.log"; exit 1; }
cat "$OUT/smoke.log"
timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" || { cat "$OUT/bench.err"; exit 1; }
cat "$OUT/bench.json"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o run -- python3 bench.py --full --no-cpu-baseline --no-latency > "$OUT/bench_prof.json" 2> "$OUT/prof.err" || { tail -20 "$OUT/prof.err"; exit 1; }
cat "$OUT/bench_prof.json"
find "$OUT/prof" -name "*stats*" | head
