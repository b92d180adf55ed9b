#!/usr/bin/env python
"""Times the loader side at the headline batch (`synth.code2_graphs(0, 128)`: N = 16 561, E = 25 377): a batch from the
device-resident `GraphStore` against the host path it replaces, and the LP evaluation loop fed by each.

  store_batch      `store.batch(idx)` - one pinned copy, one launch of `dagnn_store_gather` - then a device synchronisation
  store_enqueue    the host's share of it: `--steps` calls back to back, one synchronisation at the end, per call
  host_batch       `GraphBatch.from_data_list(graphs).to(device)` over graphs that already went through `augment_edge2` and
                   `add_order_info_01` (collation and the copies only: the per-graph transforms are NOT in this figure)
  eval_store / eval_host   graphs per second of `evaluate_lp` over `--batches` such batches (LP script's model: gated_sum,
                   1 layer, unidirectional, H = 300, 275 classes), every batch produced inside the loop by the store / by
                   the host path

The store is built from the raw graphs (next-token edges and layer ids stripped, the leaves attributed), so the pack step
redoes both transforms.  Median (and p90) over `--steps` after `--warmup`; the two paths alternate in two rounds; the store's
batch is compared with the host path's before anything is timed.  One JSON line at the end.

    python scripts/bench_store.py [--steps 50] [--warmup 10] [--batches 50]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagnn_amd import DAGNN, ASTNodeEncoder2, GraphBatch, GraphData, GraphStore, evaluate_lp, synth  # noqa: E402


def stats(ts, scale):
    ts = np.array(ts) * scale
    return [float(np.median(ts)), float(np.percentile(ts, 90))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--graphs", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_store: needs a GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    prepared = synth.code2_graphs(0, args.graphs)
    raw = []
    for g in prepared:
        ast = g.edge_index[:, g.edge_attr[:, 0] == 0].contiguous()
        leaf = torch.ones(g.x.shape[0], dtype=torch.long)
        leaf[ast[0]] = 0
        raw.append(GraphData(x=g.x, node_depth=g.node_depth, edge_index=ast, node_is_attributed=leaf.view(-1, 1)))
    t0 = time.perf_counter()
    store = GraphStore.from_graphs(raw, dev)
    torch.cuda.synchronize()
    pack_ms = (time.perf_counter() - t0) * 1e3
    idx = np.arange(args.graphs)

    def host_batch():
        return GraphBatch.from_data_list(prepared).to(dev)

    a, b = store.batch(idx), host_batch()
    for k in ("x", "node_depth", "edge_index", "edge_attr", "batch", "ptr", "_bi_layer_idx0", "_bi_layer_idx1", "_bi_layer_index0",
              "_bi_layer_index1"):
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    N, E = a.x.shape[0], a.edge_index.shape[1]

    torch.manual_seed(0)
    H, C = 300, 275
    model = DAGNN(num_vocab=None, max_seq_len=None, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder2(H, 98, 10030, 20),
                  w_edge_attr=0, num_layers=1, bidirectional=0, agg="gated_sum", mapper_bias=True, out_wx=False, out_pool_all=0,
                  out_pool="max", dropout=0.0, num_class=C).to(dev).eval()

    def timed(fn):
        ts = []
        for k in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= args.warmup:
                ts.append(time.perf_counter() - t0)
        return ts

    def enqueue():
        for _ in range(args.warmup):
            store.batch(idx)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            store.batch(idx)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return (t1 - t0) / args.steps, (time.perf_counter() - t0) / args.steps

    def eval_rate(make):
        evaluate_lp(model, (make() for _ in range(3)))      # warm-up: arenas, caches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = evaluate_lp(model, (make() for _ in range(args.batches)))   # (`compute()` synchronises)
        return args.batches * args.graphs / (time.perf_counter() - t0), res

    out = {"store_batch_us": [], "host_batch_us": [], "store_enqueue_us": [], "store_back_to_back_us": [], "eval_store_graphs_s": [],
           "eval_host_graphs_s": []}
    for rnd in range(2):   # two alternating rounds: a drift shows as a difference between them
        out["store_batch_us"].append(stats(timed(lambda: store.batch(idx)), 1e6))
        out["host_batch_us"].append(stats(timed(host_batch), 1e6))
        enq, b2b = enqueue()
        out["store_enqueue_us"].append(enq * 1e6)
        out["store_back_to_back_us"].append(b2b * 1e6)
        rs, res_s = eval_rate(lambda: store.batch(idx))
        rh, res_h = eval_rate(host_batch)
        assert res_s == res_h, (res_s, res_h)
        out["eval_store_graphs_s"].append(rs)
        out["eval_host_graphs_s"].append(rh)
        print("round %d  store.batch %.1f us (p90 %.1f)  host collate+copy %.1f us (p90 %.1f)  enqueue %.1f us  back to back %.1f us  "
              "evaluate_lp %.0f graphs/s from the store, %.0f from the host path"
              % (rnd, *out["store_batch_us"][-1], *out["host_batch_us"][-1], enq * 1e6, b2b * 1e6, rs, rh))
    print(json.dumps({"script": "bench_store", "graphs": args.graphs, "N": N, "E": E, "steps": args.steps, "warmup": args.warmup,
                      "batches": args.batches, "pack_ms": pack_ms,
                      "store_batch_us_median": min(m for m, _ in out["store_batch_us"]),
                      "host_batch_us_median": min(m for m, _ in out["host_batch_us"]),
                      "store_enqueue_us": min(out["store_enqueue_us"]), "store_back_to_back_us": min(out["store_back_to_back_us"]),
                      "eval_store_graphs_per_s": max(out["eval_store_graphs_s"]), "eval_host_graphs_per_s": max(out["eval_host_graphs_s"]),
                      "rounds": out}))


if __name__ == "__main__":
    main()
