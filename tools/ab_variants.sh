#!/bin/bash
# A/B: run the bench (--full for its checks_ok, no CPU baseline) against each tools/variants/*.so,
# interleaved rounds.  Pass --no-alt to leave the alternatives out.  Output under $AB_OUT (default build/ab).
set -uo pipefail
OUT=${AB_OUT:-build/ab}
mkdir -p "$OUT"
for round in 1 2; do
  for so in tools/variants/*.so; do
    n=$(basename $so .so)
    GPDLA_LIB=$PWD/$so timeout -k 10 300 python bench.py --full --cpu-budget 0 "$@" > "$OUT/ab_${n}_${round}.json" 2> "$OUT/ab_${n}_${round}.err" || { echo "FAIL $n"; exit 1; }
    python -c "import json,sys; d=json.loads(open('$OUT/ab_${n}_${round}.json').read().strip().splitlines()[-1]); print('$n', $round, round(d['value']/1e6,2), 'Mevals/s', round(d['kernel_ms']['likelihood'],2), 'ms', d['checks_ok'])"
  done
done
