#!/bin/bash
# same box: the default build under pesto_debug_edge_mode 0 (chosen per launch), 1 (rendezvous), 2 (node waves); $OUT/modes/m<mode>_<rep>.json
export OUT=${PESTO_PROFILE_OUT:-profiles/out}; mkdir -p $OUT      # (results of this script: $OUT/...)
R=$(cd "$(dirname "$0")/../.." && pwd); cd $R
rm -rf $OUT/modes; mkdir -p $OUT/modes
for rep in 1 2; do for m in 0 1 2; do
  timeout 300 python bench.py --full --batch ${B:-8} --steps 10 --warmup 3 --cpu-budget 0 --no-extras --no-latency --no-check --precision f16_split --edge-mode $m > $OUT/modes/m${m}_$rep.json 2>/dev/null
done; done
python profiles/ab_show.py $OUT/modes
