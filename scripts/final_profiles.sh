#!/bin/bash
# round-end artefacts: kernel stats of the forward and of the training leg, ISA metadata, the default bench line
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
R=${1:-r04}
export OUT=${OUT:-bench_out}   # where everything lands
mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/${R}_fwd -o tr -- python bench.py --full --steps 5 --warmup 2 --cpu-passes 0 --train-steps 0 --other-configs 0 > "$OUT"/${R}_fwd.log 2>&1
cp $(find "$OUT"/${R}_fwd -name "*kernel_stats.csv" | head -1) "$OUT"/${R}_kernel_stats.csv
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/${R}_train -o tr -- python bench.py --full --steps 2 --warmup 1 --cpu-passes 0 --train-steps 5 --other-configs 0 > "$OUT"/${R}_train.log 2>&1
cp $(find "$OUT"/${R}_train -name "*kernel_stats.csv" | head -1) "$OUT"/${R}_train_kernel_stats.csv
head -6 "$OUT"/${R}_kernel_stats.csv | cut -c1-150
head -8 "$OUT"/${R}_train_kernel_stats.csv | cut -c1-150
python bench.py --full > "$OUT"/${R}_final_bench.json 2> "$OUT"/${R}_final_bench.err
python - "$R" <<'PY'
import json, os, sys
d = json.load(open(os.path.join(os.environ["OUT"], "%s_final_bench.json" % sys.argv[1])))
print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["recurrence_ms_per_forward"], d["roofline"]["traffic"])
print(d["loader_side_plan"]["ms_per_step"], {k: v for k, v in d["training_step"].items() if k in ("ms_per_step", "ms_per_step_median", "kernels_ms_per_step")})
print({k: v.get("ms_per_batch", v) for k, v in d["other_configs"].items()}, d["cpu_baseline"]["value"], d["cpu_baseline"]["vectorised"]["value"])
PY
