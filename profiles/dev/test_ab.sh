#!/bin/bash
# one gpurun call: the whole GPU suite on the default build, then a same-box A/B of tagged builds: bash profiles/dev/test_ab.sh tagA tagB ...
# ("default" = pesto_amd/csrc/libpesto_hip.so); results: $OUT/test.log, $OUT/ab/*.json
export OUT=${PESTO_PROFILE_OUT:-profiles/out}; mkdir -p $OUT      # (results of this script: $OUT/...)
R=$(cd "$(dirname "$0")/../.." && pwd); cd $R
timeout 900 python -m pytest tests -m gpu -x -q > $OUT/test.log 2>&1; echo "pytest rc=$?"; tail -5 $OUT/test.log
rm -rf $OUT/ab; mkdir -p $OUT/ab
for rep in 1 2; do for t in "$@"; do
  if [ "$t" = default ]; then unset PESTO_LIB; else export PESTO_LIB=$R/pesto_amd/csrc/libpesto_hip_$t.so; fi
  timeout 300 python bench.py --full --batch 8 --steps 10 --warmup 3 --cpu-budget 0 --no-extras --no-latency --no-check --precision f16_split > $OUT/ab/${t}_$rep.json 2>/dev/null
done; done
unset PESTO_LIB
python profiles/ab_show.py $OUT/ab
