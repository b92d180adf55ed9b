#!/usr/bin/env python
"""Times `DAGNN.score` (`dagnn_heads_score`: top-k, log-sum-exp and row losses without the logits) next to `predict` and to the
torch form it replaces, at the headline shape (B = 128, H = 256, L = 2, bidirectional: D = 1024, S = 5, V = 5002) and at the LP
shape (one head of 275 classes, H = 300, L = 1, D = 300), in one run:

  head step alone, on pooled vectors that exist (device time, hip events around `--inner` back-to-back calls):
    heads_argmax | heads_score k=1 | heads_score y k=1 | heads_score y k=8 | torch: addmm + cross_entropy + topk(8) per head
  whole passes (host time around one call, ending in a synchronisation):
    predict | score k=1 | score y k=1 | score y k=8 | torch: forward + seq_cross_entropy (class_cross_entropy) + topk(8) per head
  a whole `GraphStore.evaluate_tok` over a synthetic store, with and without `loss=True`.

Prints median and p90 per case for two interleaved rounds, then one JSON line.

    python scripts/bench_score.py [--steps 30] [--warmup 10] [--inner 20] [--graphs 512]
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
from dagnn_amd import DAGNN, ASTNodeEncoder, ASTNodeEncoder2, GraphData, GraphStore, engine, synth  # noqa: E402
from dagnn_amd.lp import class_cross_entropy  # noqa: E402
from dagnn_amd.train import seq_cross_entropy  # noqa: E402


def stats(ts):
    ts = np.array(ts)
    return [float(np.median(ts)), float(np.percentile(ts, 90))]


def device_ms(fn, steps, warmup, inner):
    """ms per call on the device: events around `inner` calls queued back to back"""
    ts = []
    for k in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        if k >= warmup:
            ts.append(a.elapsed_time(b) / inner)
    return stats(ts)


def host_ms(fn, fresh, steps, warmup):
    """ms per call on the host, each on its own copy of the batch (a pass replaces G.x), ending in a synchronisation"""
    ts = []
    for k in range(warmup + steps):
        G = fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(G)
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def shape_cases(model, batch, y, S, V, single):
    """(head-step cases, whole-pass cases) of one model"""
    dev = y.device
    heads = [model.graph_pred_linear] if single else list(model.graph_pred_linear_list)
    wcat, bcat = (heads[0].weight.detach(), heads[0].bias.detach()) if single else tuple(t.detach() for t in model._head_storage())
    out = torch.rand(y.shape[0], wcat.shape[1], device=dev) * 2 - 1
    arena = model._arena_for(out)
    y2 = y.reshape(-1, S)

    def torch_heads():
        logits = torch.addmm(bcat, out, wcat.t())
        loss = torch.nn.functional.cross_entropy(logits.view(-1, V), y2.reshape(-1))
        return loss, [logits[:, s * V:(s + 1) * V].topk(8, dim=1) for s in range(S)]

    def torch_pass(G):
        with torch.no_grad():
            pred = model(G)
            if single:
                return class_cross_entropy(pred, y), pred.topk(8, dim=1)
            return seq_cross_entropy(pred, y), [p.topk(8, dim=1) for p in pred]

    step = [("heads_argmax", lambda: engine.heads_argmax(out, wcat, bcat, S, V, arena=arena)),
            ("heads_score k=1", lambda: engine.heads_score(out, wcat, bcat, S, V, arena=arena)),
            ("heads_score y k=1", lambda: engine.heads_score(out, wcat, bcat, S, V, y=y2, arena=arena)),
            ("heads_score y k=8", lambda: engine.heads_score(out, wcat, bcat, S, V, y=y2, k=8, arena=arena)),
            ("torch addmm+ce+topk8", torch_heads)]
    whole = [("predict", lambda G: model.predict(G)),
             ("score k=1", lambda G: model.score(G)),
             ("score y k=1", lambda G: model.score(G, y)),
             ("score y k=8", lambda G: model.score(G, y, topk=8)),
             ("torch forward+ce+topk8", torch_pass)]
    return step, whole


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--graphs", type=int, default=512, help="graphs of the synthetic store")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_score: needs a GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, V, S = args.batch, 5002, 5
    tok_model = DAGNN(num_vocab=V, max_seq_len=S, emb_dim=256, hidden_dim=256, out_dim=None, encoder=ASTNodeEncoder(256, 98, 10030, 20),
                      w_edge_attr=True, num_layers=2, bidirectional=True, agg="attn_h", out_wx=False, out_pool_all=False,
                      out_pool="max", dropout=0.0).to(dev).eval()
    C = 275
    lp_model = DAGNN(num_vocab=None, max_seq_len=None, emb_dim=300, hidden_dim=300, out_dim=None,
                     encoder=ASTNodeEncoder2(300, 98, 10030, 20), w_edge_attr=0, num_layers=1, bidirectional=0, agg="gated_sum",
                     mapper_bias=True, out_wx=False, out_pool_all=0, out_pool="max", dropout=0.0, num_class=C).to(dev).eval()
    batch = synth.code2_batch(seed=0, num_graphs=B, mean_n=125).to(dev)
    g = torch.Generator().manual_seed(1)
    shapes = {"headline": (tok_model, torch.randint(0, V, (B, S), generator=g).to(dev), S, V, False),
              "lp": (lp_model, torch.randint(0, C, (B,), generator=g).to(dev), 1, C, True)}
    res = {}
    for name, (model, y, s_, v_, single) in shapes.items():
        step, whole = shape_cases(model, batch, y, s_, v_, single)
        for rnd in range(2):   # two interleaved rounds: a drift of the clocks shows as a difference between them
            for case, fn in step:
                r = device_ms(fn, args.steps, args.warmup, args.inner)
                res.setdefault(name + " | " + case, []).append(r)
                print("round %d  %-9s %-24s median %.4f ms  p90 %.4f ms  (device, per call)" % (rnd, name, case, r[0], r[1]))
            for case, fn in whole:
                r = host_ms(fn, batch.clone, args.steps, args.warmup)
                res.setdefault(name + " | " + case, []).append(r)
                print("round %d  %-9s %-24s median %.4f ms  p90 %.4f ms  (host, whole pass)" % (rnd, name, case, r[0], r[1]))
        model.check()

    # a whole evaluation over a synthetic store
    raw = []
    rng = np.random.default_rng(2)
    vocab = {"w%d" % i: i for i in range(V - 2)}
    vocab["__UNK__"], vocab["__EOS__"] = V - 2, V - 1
    for gr in synth.code2_graphs(0, args.graphs):
        ast = gr.edge_index[:, gr.edge_attr[:, 0] == 0].contiguous()
        leaf = torch.ones(gr.x.shape[0], dtype=torch.long)
        leaf[ast[0]] = 0
        d = GraphData(x=gr.x, node_depth=gr.node_depth, edge_index=ast, node_is_attributed=leaf.view(-1, 1),
                      y_arr=torch.from_numpy(rng.integers(0, V, size=(1, S))))
        d.y = ["w%d" % int(i) for i in rng.integers(0, V + 500, size=int(rng.integers(1, 8)))]
        raw.append(d)
    store = GraphStore.from_graphs(raw, dev, vocab)
    ids = np.arange(args.graphs)
    for rnd in range(2):
        for case, loss in (("evaluate_tok", False), ("evaluate_tok loss=True", True)):
            ts = []
            for k in range(3 + max(args.steps // 3, 3)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = store.evaluate_tok(tok_model, ids, B, loss=loss)
                torch.cuda.synchronize()
                if k >= 3:
                    ts.append((time.perf_counter() - t0) * 1e3)
            r = stats(ts)
            res.setdefault("store | " + case, []).append(r)
            print("round %d  store     %-24s median %.3f ms  p90 %.3f ms  (%d graphs, %s)" % (rnd, case, r[0], r[1], args.graphs, out))
    print(json.dumps({"script": "bench_score", "B": B, "steps": args.steps, "inner": args.inner, "graphs": args.graphs,
                      "ms": {k: {"median": min(m for m, _ in v), "rounds": v} for k, v in res.items()}}))


if __name__ == "__main__":
    main()
