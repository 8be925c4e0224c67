# rocprofv3 kernel trace + stats of the default bench (4 timed graph replays), then the per-kernel table
set -o pipefail
cd "$(dirname "$0")/.."; export TMPDIR=/tmp; OUT=${OUT:-build/out}; mkdir -p $OUT
T=${1:-prof}
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${T}_prof -o ${T} -- python3 bench.py --steps 4 --warmup 2 --no-cpu-baseline --no-census > $OUT/${T}_prof.log 2>&1 || exit 14
tail -1 $OUT/${T}_prof.log | cut -c1-200
python3 tools/trace_gaps.py $OUT/${T}_prof/${T}_kernel_trace.csv --queues > $OUT/${T}_queues.txt; tail -40 $OUT/${T}_queues.txt
python3 tools/trace_top.py $OUT/${T}_prof/${T}_kernel_trace.csv 3 45 > $OUT/${T}_top.txt
