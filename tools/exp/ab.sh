#!/bin/bash
# A/B two builds of libviterbi.so on the same box: alternating runs of the headline bench kernel time
R=$(cd "$(dirname "$0")/../.." && pwd)
for i in 1 2 3; do
  for v in base "$@"; do
    if [ "$v" = base ]; then unset VITERBI_AMD_LIB; else export VITERBI_AMD_LIB=$R/tools/exp/libviterbi_$v.so; fi
    python3 $R/bench.py --no-cpu --no-pipelined --steps 30 --warmup 3 2>/dev/null | python3 -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$v', d['roofline']['kernel_ms'], d['value'])"
  done
done
