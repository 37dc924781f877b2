#!/bin/bash
# same box, three interleaved repetitions of 20 steps: bash profiles/dev/ab3.sh tagA tagB ...  (libpesto_hip_<tag>.so)
export OUT=${PESTO_PROFILE_OUT:-profiles/out}; mkdir -p $OUT      # (results of this script: $OUT/...)
R=$(cd "$(dirname "$0")/../.." && pwd); cd $R; rm -rf $OUT/ab; mkdir -p $OUT/ab
for rep in 1 2 3; do for t in "$@"; do
  PESTO_LIB=$R/pesto_amd/csrc/libpesto_hip_$t.so timeout 300 python bench.py --full --batch 8 --steps 20 --warmup 5 --cpu-budget 0 --no-extras --no-latency --no-check --precision f16_split > $OUT/ab/${t}_$rep.json 2>/dev/null
done; done
python profiles/ab_show.py $OUT/ab
