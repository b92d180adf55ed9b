#!/bin/bash
# quick training-step measurement (--full, but no CPU leg, no other configs): prints ms_per_step and the training-step kernel
# spans; the line and stderr land in $OUT (default: bench_out/)
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
python bench.py --full --steps 10 --warmup 3 --cpu-passes 0 --other-configs 0 --train-steps 10 "$@" > "$OUT/_tq.json" 2> "$OUT/_tq.err"
python - <<'PY'
import json, os
d = json.load(open(os.path.join(os.environ["OUT"], "_tq.json")))
t = d["training_step"]
print("fwd ms_per_step", d["ms_per_step"], "recurrence", d["roofline"]["recurrence_ms_per_forward"])
print("train ms_per_step", t["ms_per_step"], "median", t["ms_per_step_median"], t["kernels_ms_per_step"])
PY
