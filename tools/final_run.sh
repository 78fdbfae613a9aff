# GPU suite, then one `bench.py --full` line and its README summary; logs go to the directory given as $1.
# Each GPU step has its own time limit, and a failed step (a fault, an abort, a time limit) ends the script.
OUT=${1:?usage: tools/final_run.sh OUTDIR}
mkdir -p "$OUT" || exit 1
timeout -k 10 800 python -m pytest tests -m gpu -x -q > "$OUT/full_gpu.log" 2>&1
rc=$?
tail -2 "$OUT/full_gpu.log"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" || exit $?
python tools/bench_summary.py "$OUT/bench.json"
