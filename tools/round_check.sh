# Full GPU check of the current tree (run on the GPU box from the repo root):
#   bash tools/round_check.sh <tag>  -> $OUT/{gpu_tests,smoke,bench,bench_celeba}_<tag>.log + rocprof stats / PMC
set -o pipefail
T=${1:-cur}
cd $GRAFT_REPO_ROOT
OUT=${OUT_DIR:-bench_out}; mkdir -p $OUT
timeout -k 10 700 python -u -m pytest tests -m gpu -q --timeout 300 --timeout-method thread > $OUT/gpu_tests_$T.log 2>&1
rc=$?
tail -3 $OUT/gpu_tests_$T.log
[ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc
[ $rc -eq 1 ] && echo TESTS_FAILED   # the later steps still run for their data; the script exits 1 at the end
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$T.log 2>&1 || { cat $OUT/smoke_$T.log; exit 1; }
tail -1 $OUT/smoke_$T.log
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 > $OUT/bench_$T.log 2>&1 || { tail -20 $OUT/bench_$T.log; exit 1; }
cut -c1-300 $OUT/bench_$T.log
timeout -k 10 300 python bench.py --full --config celebahq256 --batch 4 --steps 3 --warmup 1 > $OUT/bench_celeba_$T.log 2>&1 || { tail -20 $OUT/bench_celeba_$T.log; exit 1; }
cut -c1-300 $OUT/bench_celeba_$T.log
bash tools/profile_round.sh $T > /dev/null 2>&1 || { echo PROFILE_FAILED; exit 1; }
echo PROFILE_OK
if [ $rc -eq 1 ]; then echo TESTS_FAILED; exit 1; fi
