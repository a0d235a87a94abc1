#!/bin/bash
# One GPU-box session: parity tests, smoke, bench, rocprofv3 kernel-trace summary.
# Every GPU step has its own time limit; a crash/fault/timeout (rc other than 0/1) ends the script.
# Logs and traces go to $GPU_CHECK_OUT (default: check_out/ in the repository, git-ignored).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT="${GPU_CHECK_OUT:-check_out}"
mkdir -p "$OUT"
export TMPDIR=/tmp
STEP="${1:-all}"

fatal() { case "$1" in 0|1) return 1;; *) return 0;; esac; }

if [ "$STEP" = all ] || [ "$STEP" = test ]; then
  timeout -k 10 900 python -m pytest tests -m gpu -q -p no:cacheprovider -x ${PYTEST_ARGS:-} > "$OUT/pytest_gpu.log" 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -40 "$OUT/pytest_gpu.log"
  if fatal $rc; then exit $rc; fi
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
  rc=$?; echo "smoke rc=$rc"; tail -5 "$OUT/smoke.log"
  if fatal $rc; then exit $rc; fi
fi
if [ "$STEP" = all ] || [ "$STEP" = bench ]; then
  # the whole line (variants, strong, train, CPU baselines): --full
  timeout -k 10 600 python bench.py --full ${BENCH_ARGS:-} > "$OUT/bench.log" 2>&1
  rc=$?; echo "bench rc=$rc"; tail -5 "$OUT/bench.log"
  if fatal $rc; then exit $rc; fi
fi
if [ "$STEP" = all ] || [ "$STEP" = prof ]; then
  rm -rf "$OUT/prof"
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o run -- \
      python3 bench.py --steps 20 --warmup 3 ${PROF_ARGS:-} > "$OUT/prof.log" 2>&1
  rc=$?; echo "rocprof rc=$rc"; tail -3 "$OUT/prof.log"
  find "$OUT/prof" -name "*stats*" | head
  python3 tools/prof_summary.py "$OUT/prof" "$OUT/prof.log" 20 "$OUT/prof/rollout_summary.json"
fi
