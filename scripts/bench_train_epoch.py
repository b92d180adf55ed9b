#!/usr/bin/env python
"""Times a training epoch of the TOK task at the headline shape (`synth.code2_graphs(0, 128)`: N = 16 561, E = 25 377; H = 256,
2 layers, bidirectional, V = 5 002, S = 5; `ClipAdam(max_norm=0.25)`) fed by a device-resident `GraphStore`, three ways:

  train_tok   (a) `store.train_tok`: the loss launch (`dagnn_seq_ce_step`) leaves the tokens, the F1 counts and the epoch's
              loss sum on the device; ONE read at the end of the epoch
  hand_loop   (b) the reference's `train()` written out on the pieces the library had before: `seq_cross_entropy`,
              `loss.item()`, `evaluate.rows_argmax`, `SeqF1.update` per step, `SeqF1.compute()` at the end
  bare_step   (c) forward, loss, backward, optimizer - no metric, no read: what `bench.py --full` times as the training
              step (there on batches cloned in advance, here on batches the store collates inside the loop, like (a) and (b))

An "epoch" is `--steps` batches of the same 128 graphs.  Per-step time = wall time of one epoch, synchronised at its end,
divided by its steps; median (and p90) over `--epochs` epochs after `--warmup`; the three alternate in two rounds, so a
drift shows as a difference between the rounds.  Kernel launches per step are counted by torch's profiler over one epoch of
each (kernels, and copies / fills apart).  (a) and (b) are checked to return the same numbers before anything is timed.  One
JSON line at the end.

    python scripts/bench_train_epoch.py [--steps 10] [--epochs 12] [--warmup 3]
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagnn_amd import DAGNN, ASTNodeEncoder, GraphData, GraphStore, SeqF1, engine, synth  # noqa: E402
from dagnn_amd.evaluate import rows_argmax  # noqa: E402
from dagnn_amd.train import ClipAdam, seq_cross_entropy  # noqa: E402

H, L, V, S = 256, 2, 5002, 5


def build_store(num, dev):
    rng = np.random.default_rng(1)
    idx2vocab = ["w%d" % i for i in range(V - 2)] + ["__UNK__", "__EOS__"]
    vocab = {w: i for i, w in enumerate(idx2vocab)}
    raw = []
    for g in synth.code2_graphs(0, num):
        ast = g.edge_index[:, g.edge_attr[:, 0] == 0].contiguous()
        leaf = torch.ones(g.x.shape[0], dtype=torch.long)
        leaf[ast[0]] = 0
        d = GraphData(x=g.x, node_depth=g.node_depth, edge_index=ast, node_is_attributed=leaf.view(-1, 1),
                      y_arr=torch.from_numpy(rng.integers(0, V, size=(1, S))))
        d.y = [idx2vocab[int(i)] for i in rng.integers(0, V - 2, size=int(rng.integers(1, 7)))]
        raw.append(d)
    return GraphStore.from_graphs(raw, dev, vocab)


def build_model(dev):
    torch.manual_seed(0)
    model = DAGNN(num_vocab=V, max_seq_len=S, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(H, 98, 10030, 20),
                  w_edge_attr=True, num_layers=L, bidirectional=True, agg="attn_h", out_wx=False, out_pool_all=False,
                  out_pool="max", dropout=0.0)
    return model.to(dev)


def hand_loop(store, model, opt, ids, bs):
    """(b): main_pyg.py:39-88 on the public API without the fused step."""
    model.train()
    metric, accum, steps = SeqF1(store.eos_id), 0, 0
    for batch in store.loader(ids, bs, training=True):
        y_arr, ref_ids, ref_extra = batch.y_arr, batch.ref_ids, batch.ref_extra
        pred = model(batch)
        opt.zero_grad()
        loss = seq_cross_entropy(pred, y_arr)
        loss.backward()
        opt.step()
        accum += loss.item()
        metric.update(rows_argmax(pred), ref_ids, ref_extra)
        steps += 1
    return accum / steps, metric.compute()


def bare_loop(store, model, opt, ids, bs):
    """(c): the step alone."""
    model.train()
    for batch in store.loader(ids, bs, training=True):
        y_arr = batch.y_arr
        pred = model(batch)
        opt.zero_grad()
        loss = seq_cross_entropy(pred, y_arr)
        loss.backward()
        opt.step()
    return loss


def stats(ts, scale):
    ts = np.array(ts) * scale
    return [float(np.median(ts)), float(np.percentile(ts, 90))]


def count_launches(fn, steps):
    """(kernels, copies and fills) per step of one epoch, from torch's profiler; None where it gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
    except Exception as exc:   # noqa: BLE001
        print("profiler unavailable: %s" % exc)
        return None
    if not names:
        return None
    moves = sum(1 for n in names if n.lower().startswith(("memcpy", "memset")) or "copybuffer" in n.lower() or "fillbuffer" in n.lower())
    return [round((len(names) - moves) / steps, 1), round(moves / steps, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_epoch: needs a GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    store = build_store(args.graphs, dev)
    ids = np.tile(np.arange(args.graphs), args.steps)
    bs = args.graphs
    master = build_model(dev)

    def fresh():
        m = copy.deepcopy(master)
        return m, ClipAdam(m.parameters(), lr=1e-3, max_norm=0.25)

    # (a) and (b) compute the same epoch (bitwise with the embedding tables' fixed summation order)
    was = engine.TABLE_GRADS
    engine.TABLE_GRADS = 1
    ma, oa = fresh()
    mb, ob = fresh()
    ra, rb = store.train_tok(ma, oa, ids[:3 * bs], bs), hand_loop(store, mb, ob, ids[:3 * bs], bs)
    assert ra == rb, (ra, rb)
    engine.TABLE_GRADS = was
    print("check: train_tok == hand-written loop over 3 steps: mean loss %.6f, F1 %.6f" % (ra[0], ra[1]["F1"]))

    runs = {}
    for name, fn in (("train_tok", lambda m, o: store.train_tok(m, o, ids, bs)),
                     ("hand_loop", lambda m, o: hand_loop(store, m, o, ids, bs)),
                     ("bare_step", lambda m, o: bare_loop(store, m, o, ids, bs))):
        m, o = fresh()
        runs[name] = (lambda fn=fn, m=m, o=o: fn(m, o))

    def timed(fn):
        ts = []
        for k in range(args.warmup + args.epochs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= args.warmup:
                ts.append((time.perf_counter() - t0) / args.steps)
        return ts

    out = {k: [] for k in runs}
    for rnd in range(2):
        for name, fn in runs.items():
            out[name].append(stats(timed(fn), 1e3))
        print("round %d  " % rnd + "  ".join("%s %.3f ms/step (p90 %.3f)" % (k, *out[k][-1]) for k in runs))
    launches = {k: count_launches(fn, args.steps) for k, fn in runs.items()}
    print("launches per step [kernels, copies + fills]: %s" % launches)
    print(json.dumps({"script": "bench_train_epoch", "graphs": args.graphs, "steps": args.steps, "epochs": args.epochs, "warmup": args.warmup,
                      "H": H, "L": L, "V": V, "S": S,
                      "train_tok_ms_per_step": min(m for m, _ in out["train_tok"]),
                      "hand_loop_ms_per_step": min(m for m, _ in out["hand_loop"]),
                      "bare_step_ms_per_step": min(m for m, _ in out["bare_step"]),
                      "launches_per_step": launches, "rounds": out}))


if __name__ == "__main__":
    main()
