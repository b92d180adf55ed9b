#!/usr/bin/env python
"""Times one training step (zero_grad, forward, `seq_cross_entropy`, backward, `ClipAdam`) of the aggregator ablation
`agg` = `add` / `max` (the reference's `--dagnn_agg`) at the headline shape - `synth.code2_batch(0)`: 128 graphs, N = 16 561;
H = 256, L = 2, bidirectional, five 5002-word heads, edge features - under both HIP backends of the constructor-string variants,
with the attention model's step beside them, all in ONE process and one run:

  add-hip, max-hip              `variant_backend = "hip"`: per-layer variant launches forward, the lock-step reverse sweep
  add-dataflow, max-dataflow    `variant_backend = "dataflow"`: the two persistent dataflow kernels (`variants.PlainRecurrence`)
  attn_h                        the tuned main path (the yardstick the ablation is read against)

Device events around every step (the batch copies exist before the first event), `--warmup` steps first, median and p90 of
`--steps`; the configurations alternate in `--rounds` rounds, so a drift shows as a difference between the rounds.  The path
every variant step took (`model.last_variant_path`) is part of the result, and a `dataflow` configuration that fell back is an
error.  One JSON line at the end; `ratio` = hip / dataflow per aggregator (above 1: the dataflow kernels win).

The lock-step variant pass hands its states to the read-out as differentiable outputs its own context also holds: it keeps
about 0.7 GB per step alive until a collection, hence the `gc.collect()` every 8 steps and the modest default step count.

    python scripts/bench_variant_train.py [--steps 30] [--warmup 5] [--rounds 2] [--configs add-hip,add-dataflow,...]
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagnn_amd import DAGNN, ASTNodeEncoder, synth  # noqa: E402
from dagnn_amd.train import ClipAdam, seq_cross_entropy  # noqa: E402

H, L, V, S = 256, 2, 5002, 5
CONFIGS = {
    "add-hip": ("add", "hip"), "add-dataflow": ("add", "dataflow"),
    "max-hip": ("max", "hip"), "max-dataflow": ("max", "dataflow"),
    "attn_h": ("attn_h", "hip"),
}


def fresh_inputs(m, n):
    """forward() mutates its batch (G.x becomes the embedding, node_depth is clamped, G.batch may be narrowed): one namespace
    per step, cloned on the device before the timed region."""
    return [SimpleNamespace(x=m.x.clone(), node_depth=m.node_depth.clone(), edge_index=m.edge_index, edge_attr=m.edge_attr,
                            batch=m.batch, _bi_layer_idx0=m._bi_layer_idx0, _bi_layer_index0=m._bi_layer_index0,
                            _bi_layer_idx1=m._bi_layer_idx1, _bi_layer_index1=m._bi_layer_index1, num_graphs=m.num_graphs)
            for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--configs", default=",".join(CONFIGS), help="comma-separated subset of: " + ", ".join(CONFIGS))
    args = ap.parse_args()
    names = [c for c in args.configs.split(",") if c]
    if not names or any(c not in CONFIGS for c in names):
        raise SystemExit("bench_variant_train: --configs takes names out of " + ", ".join(CONFIGS))
    if not torch.cuda.is_available():
        raise SystemExit("bench_variant_train: needs a GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    master = synth.code2_batch(0).to(dev)
    B = int(master.num_graphs)
    y = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(1)).to(dev)

    runs = {}
    for name in names:
        agg, backend = CONFIGS[name]
        torch.manual_seed(0)
        model = DAGNN(num_vocab=V, max_seq_len=S, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(H, 98, 10030, 20),
                      w_edge_attr=True, num_layers=L, agg=agg, bidirectional=True, out_pool_all=False, out_pool="max",
                      out_wx=False, dropout=0.0).to(dev).train()
        model.variant_backend = backend
        opt = ClipAdam(model.parameters(), lr=1e-3, max_norm=0.25)

        def step(G, model=model, opt=opt):
            opt.zero_grad(set_to_none=True)
            loss = seq_cross_entropy(model(G), y)
            loss.backward()
            opt.step()
            return loss

        runs[name] = (model, step)

    def timed(name):
        model, step = runs[name]
        inputs = fresh_inputs(master, args.warmup + args.steps)
        gc.collect()
        inputs.reverse()   # (popped from the end: a used batch holds its step's autograd graph through G.x - dropped outside the events)
        for _ in range(args.warmup):
            step(inputs.pop())
        gc.collect()
        torch.cuda.synchronize()
        ts = []
        while inputs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            G = inputs.pop()
            a.record()
            step(G)
            b.record()
            b.synchronize()
            del G
            ts.append(a.elapsed_time(b))
            if len(ts) % 8 == 0:
                # (whatever reference cycles a step left behind hold device memory the collector knows nothing about)
                gc.collect()
        return [float(np.median(ts)), float(np.percentile(ts, 90))]

    rounds = {k: [] for k in names}
    for rnd in range(args.rounds):
        for name in names:
            rounds[name].append(timed(name))
        print("round %d  " % rnd + "  ".join("%s %.3f ms (p90 %.3f)" % (k, *rounds[k][-1]) for k in names), flush=True)
    paths = {k: runs[k][0].last_variant_path for k in names}
    for k in names:
        if k.endswith("-dataflow") and paths[k] != "dataflow":
            raise SystemExit("bench_variant_train: %s ran on %r (%s)" % (k, paths[k], getattr(runs[k][0].last_variant_route, "why", None)))
    med = {k: min(m for m, _ in v) for k, v in rounds.items()}
    ratio = {a: round(med[a + "-hip"] / med[a + "-dataflow"], 3) for a in ("add", "max") if a + "-hip" in med and a + "-dataflow" in med}
    print(json.dumps({"script": "bench_variant_train", "shape": {"graphs": B, "N": int(master.x.shape[0]), "H": H, "L": L, "V": V, "S": S},
                      "steps": args.steps, "warmup": args.warmup, "median_ms": med, "ratio_hip_over_dataflow": ratio,
                      "rounds": rounds, "paths": paths, "peak_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))


if __name__ == "__main__":
    main()
