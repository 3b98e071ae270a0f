# The GPU-box recipe of this repository: all GPU tests, the full bench line, the whole-path timings, smoke.
#   bash tools/gpu_check.sh [OUTDIR]      (run from the repository root; logs and JSON lines go to OUTDIR, default gpu_check_out)
set -o pipefail
OUT=${1:-gpu_check_out}
mkdir -p "$OUT"
timeout -k 10 1100 python -m pytest tests -q -m gpu -p no:cacheprovider > "$OUT/check_tests.log" 2>&1
rc=$?; echo "pytest rc=$rc"; tail -8 "$OUT/check_tests.log"
if [ $rc -ge 124 ]; then exit $rc; fi
timeout -k 10 600 python bench.py --steps 20 --warmup 5 --full > "$OUT/check_bench.json" 2> "$OUT/check_bench.err" || exit 1
cat "$OUT/check_bench.json"
timeout -k 10 300 python tools/bench_paths.py --snps 2000000 --inds 500 --pops 8 --loo --partitions 3 > "$OUT/check_paths_c4.json" 2> "$OUT/check_paths.err" || exit 1
cat "$OUT/check_paths_c4.json"
timeout -k 10 300 python __graft_entry__.py --smoke 2>&1 | tail -2
