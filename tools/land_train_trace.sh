#!/bin/bash
# Kernel trace of a short tools/land_train_bench.py run (DESIGN.md §6 "Land in training"):
# the duration of the kernels land mode adds or re-routes, per kind of step.
#   bash tools/land_train_trace.sh [OUTDIR]   -> profiles/land_train_trace.txt,
#                                                 profiles/land_train_kernel_stats.csv
R=$(cd "$(dirname "$0")/.." && pwd)
O=${1:-$R/bench_outputs/land_trace}
W=2; S=5
mkdir -p "$O"
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$O" -o t -- \
  python3 "$R/tools/land_train_bench.py" --repeats 1 --steps $S --warmup $W --out "$O/run.json" > "$O/run.log" 2>&1 \
  || { echo "trace failed"; tail -5 "$O/run.log"; exit 1; }
T=$(find "$O" -name "*kernel_trace.csv" | head -1)
K=$(find "$O" -name "*kernel_stats.csv" | head -1)
{
  echo "rocprofv3 --kernel-trace --stats -- tools/land_train_bench.py --repeats 1 --steps $S --warmup $W   (tools/land_train_trace.sh)"
  echo "mean duration per launch over the timed steps of each kind of step; two 32-tile engines a step;"
  echo "a trace serialises the engines' streams.  All dispatches: land_train_kernel_stats.csv"
  echo
  python3 "$R/tools/land_train_trace.py" "$T" --warmup $W --steps $S
} > "$R/profiles/land_train_trace.txt" || exit 2
cp "$K" "$R/profiles/land_train_kernel_stats.csv"
cat "$R/profiles/land_train_trace.txt"
