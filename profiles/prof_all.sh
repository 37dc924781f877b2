#!/bin/bash
# kernel-trace stats + PMC passes of the bench workload on the shipped build (GPU box, repo root)
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${PESTO_PROFILE_OUT:-$R/profiles/out}      # results (prof_round.sh and the scripts it runs share it)
TAG=${1:-r02}
export TMPDIR=/tmp
mkdir -p $OUT/$TAG
cd /tmp
timeout 300 rocprofv3 --kernel-trace --stats -d $OUT/$TAG/trace -o trace --output-format csv -- python $R/bench.py --full --steps 20 --warmup 5 --cpu-budget 0 --no-latency --no-extras --precision f16_split > $OUT/$TAG/trace.log 2>&1
cp $(find $OUT/$TAG/trace -name "*kernel_stats.csv" | head -1) $OUT/$TAG/kernel_stats.csv 2>/dev/null
cd $R
bash profiles/pmc_collect.sh $TAG > $OUT/$TAG/pmc.log 2>&1
cp $OUT/pmc_$TAG/summary.txt $OUT/$TAG/pmc_summary.txt; cp $OUT/pmc_$TAG/traffic.json $OUT/$TAG/traffic.json
# the kernel trace's average durations go into the same hash-stamped file: bench.py quotes roofline.frac_rocprof from it
python - $OUT/$TAG/kernel_stats.csv $OUT/$TAG/traffic.json <<'PY'
import csv, json, re, sys
stats, tpath = sys.argv[1], sys.argv[2]
t = json.load(open(tpath))
tr = {}
for row in csv.DictReader(open(stats)):
    m = re.search(r"k_edge<([^>]*)>", row["Name"])
    if m:
        tr["k_edge<" + m.group(1).replace(" ", "") + ">"] = {"calls": int(row["Calls"]), "avg_ns": float(row["AverageNs"])}
    elif "k_node16" in row["Name"]:
        tr["pesto::k_node16"] = {"calls": int(row["Calls"]), "avg_ns": float(row["AverageNs"])}
t["rocprof_kernel_trace"] = {"kernels": tr, "how": "rocprofv3 --kernel-trace --stats of python bench.py --full --steps 20 --warmup 5 --precision f16_split "
                                                    "(the same call as the PMC passes; the profiler adds ~5 % to a launch)"}
json.dump(t, open(tpath, "w"), indent=1)
PY
