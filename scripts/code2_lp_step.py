#!/usr/bin/env python
"""Times the two loops of the ogbg-code2 LP task (ogbg-code/main_pyg_lp.py) at the LP script's shape - `gated_sum`,
`w_edge_attr=0`, 1 layer, unidirectional, max-pool over the output nodes, emb_dim = hidden = 300, num_class = 275 - at
B = 20 (the script's default batch) and B = 128, each beside the reference loop's own operations on the same model:

  train       forward + `F.cross_entropy(pred, targ.to(torch.long))` + backward + ClipAdam      [main_pyg_lp.py:53-62]
  train_lp    forward + `class_cross_entropy` (loss and d logits in one launch) + backward + ClipAdam
  eval        forward + `torch.argmax(pred, dim=1).view(-1, 1).cpu()` + targets to the host + compare  [main_pyg_lp.py:86-96]
  eval_lp     the body of `evaluate_lp`: `lp_targets` + `predict` + `ClassAccuracy.update` (nothing leaves the device)
  depth       `lp_targets` on a batch WITHOUT the `len_longest_path` attribute (`dagnn_graph_depth`, one launch)

The batch carries `len_longest_path` as the reference's reader stores it (a float per graph), clamped to num_class - 1:
the synthetic ASTs are deeper than the data set's.  Every timed step ends with a device synchronisation; median and p90
over `--steps` steps after `--warmup`, two interleaved rounds, then one JSON line.

    python scripts/code2_lp_step.py [--steps 30] [--warmup 5] [--batches 20,128]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagnn_amd import DAGNN, ASTNodeEncoder2, ClassAccuracy, class_cross_entropy, lp_targets, synth  # noqa: E402
from dagnn_amd.train import ClipAdam  # noqa: E402


def stats(ts):
    ts = np.array(ts) * 1e3
    return float(np.median(ts)), float(np.percentile(ts, 90))


def run_shape(B, H, C, args, dev):
    torch.manual_seed(0)
    model = DAGNN(num_vocab=None, max_seq_len=None, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder2(H, 98, 10030, 20),
                  w_edge_attr=0, num_layers=1, bidirectional=0, agg="gated_sum", mapper_bias=True, out_wx=False, out_pool_all=0,
                  out_pool="max", dropout=0.0, num_class=C).to(dev)
    opt = ClipAdam(model.parameters(), lr=1e-3)
    bare = synth.code2_batch(seed=0, num_graphs=B, mean_n=125).to(dev)
    batch = bare.clone()
    batch.len_longest_path = lp_targets(bare, B).clamp(max=C - 1).float()
    acc_host, metric = [], ClassAccuracy()

    def train(G, loss_fn):
        model.train()
        pred = model(G)
        opt.zero_grad()
        loss = loss_fn(pred, G.len_longest_path)
        loss.backward()
        opt.step()
        return loss

    def eval_ref(G):
        model.eval()
        with torch.no_grad():
            pred = model(G)
        y_true = G.len_longest_path.view(-1, 1).detach().cpu().numpy()
        y_pred = torch.argmax(pred.detach(), dim=1).view(-1, 1).cpu().numpy()
        is_labeled = y_true[:, 0] == y_true[:, 0]                       # ogb/graphproppred/evaluate.py:225-227
        correct = y_true[is_labeled, 0] == y_pred[is_labeled, 0]
        acc_host.append((float(np.sum(correct)), len(correct)))

    def eval_lp(G):
        model.eval()
        targ = lp_targets(G, B)
        metric.update(model.predict(G), targ)

    cases = [("train", lambda G: train(G, lambda p, t: F.cross_entropy(p, t.to(torch.long)))),
             ("train_lp", lambda G: train(G, class_cross_entropy)),
             ("eval", eval_ref), ("eval_lp", eval_lp),
             ("depth", lambda G: lp_targets(G, B))]
    res = {}
    for rnd in range(2):   # two interleaved rounds: a drift of the clocks shows as a difference between them
        for name, fn in cases:
            ts = []
            for k in range(args.warmup + args.steps):
                G = (bare if name == "depth" else batch).clone()   # (a pass replaces G.x: every step gets its own copy)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(G)
                torch.cuda.synchronize()
                if k >= args.warmup:
                    ts.append(time.perf_counter() - t0)
            med, p90 = stats(ts)
            res.setdefault(name, []).append((med, p90))
            print("B %3d round %d  %-9s median %.3f ms  p90 %.3f ms  (%d steps)" % (B, rnd, name, med, p90, len(ts)))
    model.check()
    lp_acc = metric.compute()
    host = sum(a for a, _ in acc_host) / sum(n for _, n in acc_host)
    print("B %3d accuracy: device %.4f over %d graphs, host loop %.4f" % (B, lp_acc["acc"], lp_acc["n"], host))
    return {k: {"median": min(m for m, _ in v), "rounds": v} for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=str, default="20,128")
    ap.add_argument("--hidden", type=int, default=300)
    ap.add_argument("--classes", type=int, default=275)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for B in [int(b) for b in args.batches.split(",")]:
        out["B%d" % B] = run_shape(B, args.hidden, args.classes, args, dev)
    print(json.dumps({"script": "code2_lp_step", "H": args.hidden, "C": args.classes, "steps": args.steps, "ms": out}))


if __name__ == "__main__":
    main()
