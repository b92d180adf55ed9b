#!/usr/bin/env python
"""Times the three embedding-table gradients of a training step's backward (`autograd.EncodeAST.backward`) three ways, in one
process and one run, at the headline batch (`synth.code2_batch(0)`: N = 16 561, width 256) and at the emb_dim-300 training
batch (`synth.code2_batch(0, 160)`, width 300):

  index_add        the three `torch.zeros(...).index_add_(0, idx, g)` calls as the default path makes them (float atomics)
  index_add_det    the same under `torch.use_deterministic_algorithms(True)` (torch's sort-and-accumulate fallback)
  table_grads      `engine.table_grads`: one call, six launches, one fixed summation order; `index` and `sum` are its two
                   stages timed apart over a kept workspace (the four index launches / the two sum launches)

Device events around the calls only (the gradient, the keys and - for the stages - the workspace exist before the first event),
`--warmup` calls first, median (and p90) of `--steps`; the variants alternate in two rounds, so a drift shows as a difference
between the rounds.  Before anything is timed the new path is compared with its host mirror (bits) and with `index_add_`
(rounding).  One JSON line at the end.

    python scripts/bench_table_grads.py [--steps 100] [--warmup 20]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagnn_amd import _lib, engine, synth  # noqa: E402
from dagnn_amd.autograd import table_grads_host  # noqa: E402

ROWS = (98, 10030, 21)   # node types, node attributes, depths 0..20 (ogbg-code/main_pyg.py: ASTNodeEncoder)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if args.steps < 50:
        raise SystemExit("bench_table_grads: a median wants at least 50 runs")
    if not torch.cuda.is_available():
        raise SystemExit("bench_table_grads: needs a GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    lib = _lib.load()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return [float(np.median(ts)), float(np.percentile(ts, 90))]

    result = {"script": "bench_table_grads", "steps": args.steps, "warmup": args.warmup, "shapes": {}}
    for name, graphs, H in (("headline_B128_H256", 128, 256), ("ogb_tok_B160_H300", 160, 300)):
        batch = synth.code2_batch(0, graphs)
        batch.x[:, 1] %= ROWS[1]
        x = batch.x.to(dev)
        depth = batch.node_depth.view(-1).clamp(max=ROWS[2] - 1).to(dev)
        keys = (x[:, 0], x[:, 1], depth)
        N = x.shape[0]
        g = torch.randn(N, H, generator=torch.Generator().manual_seed(1)).to(dev)
        counts = [torch.bincount(k, minlength=R) for k, R in zip(keys, ROWS)]

        def index_add():
            return [torch.zeros(R, H, dtype=g.dtype, device=dev).index_add_(0, k, g) for k, R in zip(keys, ROWS)]

        def index_add_det():
            torch.use_deterministic_algorithms(True)
            try:
                return index_add()
            finally:
                torch.use_deterministic_algorithms(False)

        ws = torch.empty(lib.dagnn_table_grads_workspace_bytes(N, H, (C.c_int64 * 3)(*ROWS), 3), dtype=torch.uint8, device=dev)
        variants = {
            "index_add": index_add, "index_add_det": index_add_det, "table_grads": lambda: engine.table_grads(g, keys, ROWS),
            "index": lambda: engine.table_grads(g, keys, ROWS, stages=_lib.TABLE_GRADS_INDEX, workspace=ws),
            "sum": lambda: engine.table_grads(g, keys, ROWS, stages=_lib.TABLE_GRADS_SUM, workspace=ws),
        }
        got = engine.table_grads(g, keys, ROWS)
        want = table_grads_host(g, keys, ROWS)
        assert all(torch.equal(a.cpu(), torch.from_numpy(w)) for a, w in zip(got, want)), "table_grads differs from its host mirror"
        for a, ref in zip(got, index_add()):
            assert float((a - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), "table_grads differs from index_add_"
        rounds = {k: [] for k in variants}
        for rnd in range(2):
            for k, fn in variants.items():
                rounds[k].append(timed(fn))
            print("%s round %d  " % (name, rnd) + "  ".join("%s %.1f us (p90 %.1f)" % (k, *rounds[k][-1]) for k in variants))
        result["shapes"][name] = {
            "N": N, "H": H, "rows": list(ROWS), "workspace_bytes": ws.numel(),
            "largest_row": [int(c.max()) for c in counts], "rows_with_members": [int((c > 0).sum()) for c in counts],
            "median_us": {k: min(m for m, _ in v) for k, v in rounds.items()}, "rounds": rounds,
        }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
