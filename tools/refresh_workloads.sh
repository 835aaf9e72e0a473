#!/bin/bash
# Bench lines of every workload -> build/wl/*.json (profiles/r03_workloads.json is assembled from them)
cd "$(dirname "$0")/.."
O=build/wl
mkdir -p $O
python bench.py --full > $O/c2.json 2>/dev/null
python bench.py --full --workload c3 > $O/c3.json 2>/dev/null
python bench.py --full --workload c3 --batch 64 --cpu-seconds 0 > $O/c3_b64.json 2>/dev/null
python bench.py --full --workload c3 --graph --cpu-seconds 0 > $O/c3_graph.json 2>/dev/null
python bench.py --full --workload c4 > $O/c4.json 2>/dev/null
python bench.py --full --workload c4 --heads 16 --cpu-seconds 0 > $O/c4_h16.json 2>/dev/null
python bench.py --full --workload c5 > $O/c5.json 2>/dev/null
python bench.py --full --workload c5 --batch 1024 > $O/c5_1024.json 2>/dev/null
for f in $O/*.json; do python - "$f" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(sys.argv[1].split("/")[-1], d["value"], d["unit"], d["ms_per_step"], d.get("ms_per_step_no_spinup"))
PY
done
