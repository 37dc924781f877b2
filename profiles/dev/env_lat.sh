#!/bin/bash
# one structure per call against HIP runtime switches (kernel arguments in device memory, ...): bash profiles/dev/env_lat.sh
export OUT=${PESTO_PROFILE_OUT:-profiles/out}; mkdir -p $OUT      # (results of this script: $OUT/...)
R=$(cd "$(dirname "$0")/../.." && pwd); cd $R; mkdir -p $OUT/envlat
run() { tag=$1; shift
  for rep in 1 2; do
    env "$@" timeout 300 python bench.py --full --steps 5 --warmup 2 --cpu-budget 0 --no-extras > $OUT/envlat/${tag}_$rep.json 2>/dev/null
    python -c "import json;d=json.load(open('$OUT/envlat/${tag}_$rep.json'));print('$tag', $rep, 'batch1 ms', round(d['ms_per_structure_batch1'],4), ' step ms', round(d['ms_per_step'],3))"
  done; }
run default X=1
run kernarg0 HIP_FORCE_DEV_KERNARG=0
run kernarg1 HIP_FORCE_DEV_KERNARG=1
run default_b X=1
