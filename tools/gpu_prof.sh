#!/bin/bash
# rocprofv3 kernel trace + stats of the blocking sweep and of bench.py --full (no PMC counters here).
# Usage: tools/gpu_prof.sh [OUTDIR]   (default prof_out/)
cd "$(dirname "$0")/.."
O=${1:-prof_out}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/prof_sweep -o run --output-format csv -- \
   python3 tools/sweep_tb.py --reps 2 ${SWEEP_ARGS} > $O/prof_sweep.log 2>&1
rc=$?; echo "prof sweep rc=$rc"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/prof_bench -o run --output-format csv -- \
   python3 bench.py --full --no-cpu-baseline ${BENCH_ARGS} > $O/prof_bench.log 2>&1
rc=$?; echo "prof bench rc=$rc"; [ $rc -eq 0 ] || exit $rc
exit 0
