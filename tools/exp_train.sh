# training step: parts breakdown, the bench line, and the idle-gap analysis of a kernel trace
set -e
R=$GRAFT_REPO_ROOT
OUT=${OUT_DIR:-$R/bench_out}
mkdir -p $OUT/tr
cd $R
timeout -k 10 300 python3 tools/train_step_parts.py --steps 4 > $OUT/tr/parts.txt 2>&1
timeout -k 10 300 python3 bench.py --full --mode train --steps 6 --warmup 2 > $OUT/tr/bench.log 2>&1
cd /tmp && export TMPDIR=/tmp
timeout -s KILL 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/tr/trace -o run -- python3 $R/bench.py --full --mode train --steps 4 --warmup 2 > $OUT/tr/bench_prof.log 2>&1
F=$(find $OUT/tr/trace -name '*kernel_trace.csv' | head -1)
python3 $R/tools/timeline_gaps.py $F --skip 0.4 --top 40 > $OUT/tr/gaps.txt
S=$(find $OUT/tr/trace -name '*kernel_stats.csv' | head -1)
cp $S $OUT/tr/kernel_stats.csv
rm -rf $OUT/tr/trace
