#!/bin/bash
# end-of-round check on the GPU box: full -m gpu suite, then the full bench line (bash scratch/final_check.sh [out_dir])
OUT=${1:-bench_out}; mkdir -p "$OUT"
python -m pytest tests -x -q -m gpu > "$OUT/t_all.log" 2>&1; tail -2 "$OUT/t_all.log"
python bench.py --full 2>"$OUT/final_bench.err" | tail -1 > "$OUT/final_bench.json"
python - "$OUT/final_bench.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["phase_ms_per_step"]["rollout"], d["phase_ms_per_step"]["update"], d["roofline"]["frac"], d["roofline"]["avg_launch_ms"], d["fp32"]["value"], d["cpu_baseline"]["value"])
PY
