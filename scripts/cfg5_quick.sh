#!/bin/bash
# cfg 5 (B = 256, h = 512, L = 5) forward with its per-kernel second pass (--full, every other leg off) -> $OUT (default: bench_out/)
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
python bench.py --full --batch 256 --hidden 512 --layers 5 --steps 6 --warmup 2 --cpu-passes 0 --other-configs 0 --train-steps 0 "$@" > "$OUT/_c5.json" 2> "$OUT/_c5.err"
python -c "
import json, os; d=json.load(open(os.path.join(os.environ['OUT'], '_c5.json'))); print('cfg5 ms_per_step', d['ms_per_step'], d.get('kernels_ms_per_step'))"
