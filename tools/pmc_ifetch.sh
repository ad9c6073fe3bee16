#!/bin/bash
# Instruction-fetch and instruction-cache counters of the bench training leg, per kernel,
# for several library builds (name:lib, empty lib = in-tree):
#   bash tools/pmc_ifetch.sh "parent:alt/libsrmi_parent.so" "new:"
# Two rocprofv3 --pmc passes per build, no tracing (the SQ and the SQC counters in a pass
# each) -> $OUT/ifetch_<name>.json (tools/pmc_ifetch_parse.py); OUT defaults to bench_outputs/
R=$(cd "$(dirname "$0")/.." && pwd); O=${OUT:-$R/bench_outputs}; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
SQ="SQ_IFETCH SQ_WAIT_INST_ANY SQ_WAVE_CYCLES SQ_BUSY_CYCLES"
SQC="SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE"
for v in "$@"; do
  IFS=: read -r name lib <<< "$v"
  for pass in SQ SQC; do
    SRMI_LIB=${lib:+$R/$lib} timeout -k 10 280 rocprofv3 --pmc ${!pass} --output-format csv -d $O/ifetch_$name/$pass -o run -- \
      python3 $R/bench.py --steps 2 --warmup 1 > $O/ifetch_${name}_$pass.log 2>&1 || { echo "pmc $name $pass failed"; exit 1; }
  done
  python3 $R/tools/pmc_ifetch_parse.py $O/ifetch_$name $O/ifetch_$name.json || exit 2
  rm -rf $O/ifetch_$name
done
echo done
