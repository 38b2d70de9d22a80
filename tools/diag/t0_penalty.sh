#!/bin/bash
# Why are a day's first two steps ~0.7 us slower in the graph (profiles/r06b_trace_split.txt)?  Per-timestep step
# times from a kernel trace of the bench, for the product and for variants (LIBS, built with tools/diag/variant.sh).
set -uo pipefail
OUT=${OUT:-diag_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
L=smart-nanogrid-gym_amd/lib
for v in ${LIBS:-libsng libsng_recpol}; do
 rm -rf $OUT/t0_$v
 SNG_LIBRARY=$L/$v.so timeout -k 10 300 rocprofv3 --kernel-trace -d $OUT/t0_$v -o run --output-format csv -- python bench.py --full --no-cpu-baseline --steps 100 --warmup 10 > $OUT/t0_$v.log 2>&1 || exit 1
 echo "== $v"; python tools/trace_split.py $OUT/t0_$v/run_kernel_trace.csv 2>&1 | grep "graph"
done
