# GPU suite + the bench with everything it can measure (--full) on one MI355X, from the repo root.
# Usage: bash tools/gpu_suite.sh TAG [pytest -k expression]     (logs go to $OUT_DIR, default bench_out/)
cd "$(dirname "$0")/.."; OUT=${OUT_DIR:-bench_out}; mkdir -p "$OUT"
tag=${1:-suite}; k=${2:-}
args=(tests/ -x -v -m gpu --timeout 150 --timeout-method thread)
[ -n "$k" ] && args+=(-k "$k")
timeout -k 10 900 python -u -m pytest "${args[@]}" > $OUT/${tag}_pytest.log 2>&1; rc=$?
tail -3 $OUT/${tag}_pytest.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 600 python -u bench.py --full > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err; rc=$?
tail -c 1500 $OUT/${tag}_bench.json
exit $rc
