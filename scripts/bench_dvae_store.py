#!/usr/bin/env python
"""Times the D-VAE loader side: batches from the device-resident `DagStore` against the host path they replace, and the
loops fed by each.  The comparison base is the list-fed path (what the package did before the store), run in this process.

  batch            per data set (ENAS n = 8, BN n = 10) and B (32, 64):
                     store_us   `store.batch(idx)` - one pinned copy, one launch of `dagnn_dag_store_gather` - then a device
                                synchronisation
                     enqueue_us the host's share of it: `--steps` calls back to back, one synchronisation at the end, per call
                     host_us    what the list path does per batch on the host: `_collate_fn`'s deep copies,
                                `GraphBatch.from_data_list(...).to(device)`, `decode_schedule` and its two pinned copies
  extract_latent   graphs per second of `extract_latent` over `--graphs` synthetic ENAS graphs at batch 64 (hs = 501, 2 layers),
                   from the list and from `(store, idx)`
  train_step       the step of scripts/dvae_train_step.py (B = 32, hs = 501, L = 2: encode + loss + backward + clip 0.25 + Adam),
                   fed by lists and fed by the store, ENAS and BN

Median (and p90) over `--steps` after `--warmup`; the two paths alternate in two rounds and the better round is reported;
the store's batch is compared with the host path's before anything is timed.  One JSON line at the end.

    python scripts/bench_dvae_store.py [--steps 50] [--warmup 10] [--graphs 4096] [--train-steps 20]
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
from dagnn_amd import DAGNN_BN, DAGNN_NA, DagStore, GraphBatch, synth  # noqa: E402
from dagnn_amd.dvae import decode_schedule, extract_latent  # noqa: E402

SETS = {"enas": ("ENAS", synth.enas_rows, synth.decode_enas_row, 8), "bn": ("BN", synth.bn_rows, synth.decode_bn_row, 10)}


def stats(ts, scale):
    ts = np.array(ts) * scale
    return [float(np.median(ts)), float(np.percentile(ts, 90))]


def make_model(name, hs, L, dev):
    n = SETS[name][3]
    if name == "enas":
        return DAGNN_NA(n, hs, hs, n, n, 0, 1, hs=hs, nz=56, num_nodes=n, num_layers=L, bidirectional=False, agg="attn_h").to(dev)
    return DAGNN_BN(n, hs, hs, n, n, 0, 1, hs=hs, nz=56, num_nodes=n, num_layers=L, bidirectional=True).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--hs", type=int, default=501)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dvae_store: needs a GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")

    def timed(fn, steps=None, warmup=None):
        ts = []
        steps, warmup = args.steps if steps is None else steps, args.warmup if warmup is None else warmup
        for k in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= warmup:
                ts.append(time.perf_counter() - t0)
        return ts

    res = {"script": "bench_dvae_store", "steps": args.steps, "warmup": args.warmup, "batch": {}, "train_step": {}}

    # ---------------------------------------------------------------- a batch
    for name, (kind, gen, decode, n) in SETS.items():
        rows = gen(1, 64)
        graphs = [decode(r) for r in rows]
        t0 = time.perf_counter()
        store = DagStore.from_rows(rows, kind, n, dev)
        torch.cuda.synchronize()
        pack_ms = (time.perf_counter() - t0) * 1e3
        model = make_model(name, 32, 1, dev)     # (only `_collate_fn` of it is used here)
        for B in (32, 64):
            idx = np.arange(B)

            def host_batch():
                G = model._collate_fn(graphs[:B])
                b = GraphBatch.from_data_list(G).to(dev)
                types, preds = decode_schedule(G, n, n, 0)
                b.types = torch.from_numpy(types).pin_memory().to(dev, non_blocking=True)
                b.preds = torch.from_numpy(preds).pin_memory().to(dev, non_blocking=True)
                return b

            a, b = store.batch(idx), host_batch()
            for k in ("x", "edge_index", "bi_layer_index", "batch", "ptr", "types", "preds"):
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (name, B, k)

            def enqueue():
                for _ in range(args.warmup):
                    store.batch(idx)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    store.batch(idx)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                return (t1 - t0) / args.steps

            rounds = {"store_us": [], "host_us": [], "enqueue_us": []}
            for _ in range(2):   # two alternating rounds: a drift shows as a difference between them
                rounds["store_us"].append(stats(timed(lambda: store.batch(idx)), 1e6))
                rounds["host_us"].append(stats(timed(host_batch), 1e6))
                rounds["enqueue_us"].append(enqueue() * 1e6)
            res["batch"]["%s_b%d" % (name, B)] = dict(N=int(a.x.shape[0]), E=int(a.edge_index.shape[1]), pack_ms=pack_ms,
                                                      store_us_median=min(m for m, _ in rounds["store_us"]),
                                                      host_us_median=min(m for m, _ in rounds["host_us"]),
                                                      enqueue_us=min(rounds["enqueue_us"]), rounds=rounds)
            print("%-4s B=%-3d store.batch %.1f us  enqueue %.1f us  host collate + schedule + copies %.1f us"
                  % (name, B, res["batch"]["%s_b%d" % (name, B)]["store_us_median"], min(rounds["enqueue_us"]),
                     res["batch"]["%s_b%d" % (name, B)]["host_us_median"]))

    # ---------------------------------------------------------------- extract_latent over a data set
    kind, gen, decode, n = SETS["enas"]
    rows = gen(2, args.graphs)
    graphs = [decode(r) for r in rows]
    store = DagStore.from_rows(rows, kind, n, dev)
    ids = np.arange(args.graphs)
    torch.manual_seed(0)
    model = make_model("enas", args.hs, 2, dev).eval()
    assert torch.equal(extract_latent(model, graphs[:256], 64), extract_latent(model, (store, ids[:256]), 64))
    rates = {"list": [], "store": []}
    for _ in range(2):
        for how, data in (("list", graphs), ("store", (store, ids))):
            ts = timed(lambda: extract_latent(model, data, 64), steps=3, warmup=1)
            rates[how].append(args.graphs / float(np.median(ts)))
    res["extract_latent"] = dict(graphs=args.graphs, batch=64, hs=args.hs, list_graphs_per_s=max(rates["list"]),
                                 store_graphs_per_s=max(rates["store"]), rounds=rates)
    print("extract_latent  %d graphs at batch 64: %.0f graphs/s from the list, %.0f graphs/s from the store"
          % (args.graphs, max(rates["list"]), max(rates["store"])))

    # ---------------------------------------------------------------- the training step
    B = 32
    for name, (kind, gen, decode, n) in SETS.items():
        torch.manual_seed(0)
        rows = gen(1, B)
        graphs = [decode(r) for r in rows]
        store = DagStore.from_rows(rows, kind, n, dev)
        idx = np.arange(B)
        model = make_model(name, args.hs, 2, dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)

        def step_list():
            opt.zero_grad()
            mu, logvar = model.encode([g.clone() for g in graphs])     # (the step of scripts/dvae_train_step.py)
            loss, _, _ = model.loss(mu, logvar, graphs)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 0.25)
            opt.step()

        def step_store():
            opt.zero_grad()
            b = store.batch(idx)
            types, preds = b.types, b.preds
            mu, logvar = model.encode_batch(b)
            loss, _, _ = model.loss_dense(mu, logvar, types, preds)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 0.25)
            opt.step()

        rounds = {"list_ms": [], "store_ms": []}
        for _ in range(2):
            rounds["list_ms"].append(stats(timed(step_list, args.train_steps, 5), 1e3))
            rounds["store_ms"].append(stats(timed(step_store, args.train_steps, 5), 1e3))
        res["train_step"][name] = dict(batch=B, hs=args.hs, layers=2, list_ms_median=min(m for m, _ in rounds["list_ms"]),
                                       store_ms_median=min(m for m, _ in rounds["store_ms"]), rounds=rounds)
        print("%-4s training step B=32 hs=%d L=2: %.2f ms fed by lists, %.2f ms fed by the store"
              % (name, args.hs, res["train_step"][name]["list_ms_median"], res["train_step"][name]["store_ms_median"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
