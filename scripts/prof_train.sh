#!/bin/bash
# rocprofv3 kernel stats of the training step (and the forward) of the headline configuration -> $OUT/<name>/ (default: bench_out/)
name=${1:-prof_train}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/$name" -o tr -- python bench.py --full --steps 5 --warmup 2 --cpu-passes 0 --other-configs 0 --train-steps 10 --no-kernel-timer > "$OUT/$name.log" 2>&1
python - "$name" <<'PY'
import csv, glob, os, sys
f = glob.glob(os.path.join(os.environ["OUT"], sys.argv[1], "**", "*kernel_stats.csv"), recursive=True)[0]
for r in list(csv.DictReader(open(f)))[:50]:
    print("%-100s %6s %12s %10s %6s" % (r["Name"][:100], r["Calls"], r["TotalDurationNs"], r["AverageNs"], r["Percentage"]))
PY
