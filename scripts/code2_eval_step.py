#!/usr/bin/env python
"""Times one batch of the ogbg-code2 evaluation loop (ogbg-code/main_pyg.py:91-124) at the headline shape (B = 128, H = 256,
L = 2, bidirectional, V = 5002, S = 5), two ways:

  logits   `forward` + the reference's `argmax` / `cat` lines (main_pyg.py:106-109)       [what a caller had before `predict`]
  predict  `DAGNN.predict` (the heads and their argmax in one pass, no logits)
  logits+metric   the above + copy to the host + `decode_arr_to_seq` per row + the evaluator's set arithmetic per graph
  predict+metric  `predict` + `encode_ref_sets` + `SeqF1.update` (counts stay on the device)

Every timed step ends with a device synchronisation; prints median and p90 per case, then one JSON line.

    python scripts/code2_eval_step.py [--steps 30] [--warmup 10] [--batch 128] [--hidden 256]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/code2_eval_step.py --profile
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
from dagnn_amd import DAGNN, ASTNodeEncoder, SeqF1, evaluate, synth  # noqa: E402


def stats(ts):
    ts = np.array(ts) * 1e3
    return float(np.median(ts)), float(np.percentile(ts, 90))


def decode_arr_to_seq(arr, idx2vocab):
    """utils.py:166-179, restated: cut at the first __EOS__ (the last vocabulary entry), ids to words."""
    eos_idx_list = (arr == len(idx2vocab) - 1).nonzero()
    clipped = arr[: torch.min(eos_idx_list)] if len(eos_idx_list) > 0 else arr
    return list(map(lambda x: idx2vocab[x], clipped.cpu()))


def eval_f1_lists(seq_ref, seq_pred):
    """ogb/graphproppred/evaluate.py:231-267, restated: the per-graph lists the evaluator averages at the end."""
    out = []
    for l, p in zip(seq_ref, seq_pred):
        label, prediction = set(l), set(p)
        tp, fp, fn = len(label & prediction), len(prediction - label), len(label - prediction)
        precision = tp / (tp + fp) if tp + fp > 0 else 0
        recall = tp / (tp + fn) if tp + fn > 0 else 0
        out.append((precision, recall, 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--vocab", type=int, default=5002)
    ap.add_argument("--seq", type=int, default=5)
    ap.add_argument("--profile", action="store_true", help="a few untimed steps of 'logits' and 'predict' (kernel traces)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    H, V, S, B = args.hidden, args.vocab, args.seq, args.batch
    model = DAGNN(num_vocab=V, max_seq_len=S, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(H, 98, 10030, 20),
                  w_edge_attr=True, num_layers=args.layers, bidirectional=True, agg="attn_h", out_wx=False, out_pool_all=False,
                  out_pool="max", dropout=0.0).to(dev).eval()
    with torch.no_grad():   # random heads never predict __EOS__: let about half of every head's rows end there
        for hd in model.graph_pred_linear_list:
            hd.bias[V - 1] += 0.12
    batch = synth.code2_batch(seed=0, num_graphs=B, mean_n=125).to(dev)
    idx2vocab = ["w%d" % i for i in range(V - 2)] + ["__UNK__", "__EOS__"]
    vocab2idx = {w: i for i, w in enumerate(idx2vocab)}
    rng = np.random.default_rng(0)
    seq_ref = [["w%d" % int(i) for i in rng.integers(0, V + 500, size=int(rng.integers(1, 8)))] for _ in range(B)]

    def logits_step(G):
        with torch.no_grad():
            pred_list = model(G)
        mat = []
        for i in range(len(pred_list)):
            mat.append(torch.argmax(pred_list[i], dim=1).view(-1, 1))
        return torch.cat(mat, dim=1)

    def predict_step(G):
        return model.predict(G)

    lists, metric = [], SeqF1(V - 1)

    def logits_metric(G):
        mat = logits_step(G)
        lists.extend(eval_f1_lists(seq_ref, [decode_arr_to_seq(arr, idx2vocab) for arr in mat]))

    def predict_metric(G):
        tok = model.predict(G)
        metric.update(tok, *evaluate.encode_ref_sets(seq_ref, vocab2idx))

    cases = [("logits", logits_step), ("predict", predict_step)]
    if args.profile:
        for name, fn in cases:
            for _ in range(5):
                fn(batch.clone())
            torch.cuda.synchronize()
        return
    cases += [("logits+metric", logits_metric), ("predict+metric", predict_metric)]
    res = {}
    for rnd in range(2):   # two interleaved rounds: a drift of the clocks shows as a difference between them
        for name, fn in cases:
            ts = []
            for k in range(args.warmup + args.steps):
                G = batch.clone()   # (a pass replaces G.x: every step gets its own copy, outside the timed span)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(G)
                torch.cuda.synchronize()
                if k >= args.warmup:
                    ts.append(time.perf_counter() - t0)
            med, p90 = stats(ts)
            res.setdefault(name, []).append((med, p90))
            print("round %d  %-16s median %.3f ms  p90 %.3f ms  (%d steps)" % (rnd, name, med, p90, len(ts)))
    model.check()
    a = logits_step(batch.clone())
    b = predict_step(batch.clone())
    same = float((a == b).float().mean())
    eos = float((b == V - 1).float().mean())
    f1 = metric.compute()
    print("predict == argmax(forward) on %.4f of the entries; EOS share %.3f; F1 over %d graphs %.4f" % (same, eos, f1["n"], f1["F1"]))
    print(json.dumps({"script": "code2_eval_step", "B": B, "H": H, "L": args.layers, "V": V, "S": S, "steps": args.steps,
                      "ms": {k: {"median": min(m for m, _ in v), "rounds": v} for k, v in res.items()},
                      "same_tokens": same, "eos_share": eos}))


if __name__ == "__main__":
    main()
