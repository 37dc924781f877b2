#!/bin/bash
# same box: one-structure latency (bench.py's ms_per_structure_batch1, precision auto, device tensors) of tagged builds: bash profiles/dev/lat_ab.sh tagA tagB ...
export OUT=${PESTO_PROFILE_OUT:-profiles/out}; mkdir -p $OUT      # (results of this script: $OUT/...)
R=$(cd "$(dirname "$0")/../.." && pwd); cd $R; mkdir -p $OUT/lat
for rep in 1 2 3; do for t in "$@"; do
  if [ "$t" = default ]; then unset PESTO_LIB; else export PESTO_LIB=$R/pesto_amd/csrc/libpesto_hip_$t.so; fi
  timeout 300 python bench.py --full --steps 5 --warmup 2 --cpu-budget 0 --no-extras > $OUT/lat/${t}_$rep.json 2>/dev/null
  python -c "import json;d=json.load(open('$OUT/lat/${t}_$rep.json'));print('$t', $rep, 'batch1 ms', round(d['ms_per_structure_batch1'],4), ' step ms', round(d['ms_per_step'],3))"
done; done
