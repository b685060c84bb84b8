#!/bin/bash
# all bench configs (every check and baseline: --full), one process each, logs under
# $OUT (default bench_logs/); stop at the first fault-like exit
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_logs}
mkdir -p "$OUT"
TAG=${TAG:-b}
for c in ${CONFIGS:-2 3 4 5}; do
  timeout -k 10 400 python bench.py --full --config $c --steps ${STEPS:-10} --warmup 3 > "$OUT/${TAG}_cfg$c.log" 2>&1
  rc=$?; echo "cfg$c rc=$rc"; tail -1 "$OUT/${TAG}_cfg$c.log"
  [ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc
done
