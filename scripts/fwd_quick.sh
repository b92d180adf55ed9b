#!/bin/bash
# quick forward measurement of the headline configuration with its per-kernel second pass (--full, but no CPU leg, no other
# configs, no training leg); the line and stderr land in $OUT (default: bench_out/)
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
python bench.py --full --steps 20 --warmup 5 --cpu-passes 0 --other-configs 0 --train-steps 0 "$@" > "$OUT/_fq.json" 2> "$OUT/_fq.err"
python - <<'PY'
import json, os
d = json.load(open(os.path.join(os.environ["OUT"], "_fq.json")))
print("fwd ms_per_step", d["ms_per_step"], "recurrence", d["roofline"]["recurrence_ms_per_forward"], "frac", d["roofline"]["frac"], d.get("kernels_ms_per_step"))
PY
