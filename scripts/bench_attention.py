#!/usr/bin/env python
"""Times `model.attention(G)` beside the evaluation pass it rides on, in one run:

  headline shape  - `DAGNN` B = 128, H = 256, L = 2, bidirectional, attn_h with the edge encoder (mean 125 nodes per graph):
                    predict | attention | attention logits=True      (host time around one call, ending in a synchronisation)
                    and the two launches of `dagnn_attention_weights` alone, on the states of a finished pass (device time)
  D-VAE shape     - `DAGNN_NA` B = 32, hs = 501, L = 2 (ENAS rows, 8 vertices): forward | attention | attention logits=True
                    (`forward` takes the fused call, `attention` the step-by-step route: the difference is both)

Prints median and p90 per case for two interleaved rounds, then one JSON line.

    python scripts/bench_attention.py [--steps 30] [--warmup 10] [--inner 20]
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
from dagnn_amd import DAGNN, DAGNN_NA, ASTNodeEncoder, synth  # noqa: E402
from dagnn_amd import attention as A  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention: needs a GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tok = DAGNN(num_vocab=5002, max_seq_len=5, emb_dim=256, hidden_dim=256, out_dim=None, encoder=ASTNodeEncoder(256, 98, 10030, 20),
                w_edge_attr=True, num_layers=2, bidirectional=True, agg="attn_h", out_wx=False, out_pool_all=False, out_pool="max",
                dropout=0.0).to(dev).eval()
    batch = synth.code2_batch(seed=0, num_graphs=128, mean_n=125).to(dev)
    na = DAGNN_NA(8, 501, 501, 8, 8, 0, 1, hs=501, nz=56, num_nodes=8, agg="attn_h", num_layers=2, bidirectional=False, out_wx=False,
                  out_pool_all=False, out_pool="max", dropout=0.0).to(dev).eval()
    na_batch = synth.dvae_batch([synth.decode_enas_row(r) for r in synth.enas_rows(3, 32)]).to(dev)

    # the states of one finished pass, for the kernels alone
    with torch.no_grad():
        _, cap = A.forward_with_states(tok, batch.clone())
    E = int(batch.edge_index.shape[1])

    def kernels(logits):
        with torch.no_grad():
            return A.weights_of(tok, cap["plan"], cap["x"], cap["h"], E, logits)

    cases = [("headline", "predict", lambda G: tok.predict(G), batch.clone),
             ("headline", "attention", lambda G: tok.attention(G), batch.clone),
             ("headline", "attention logits", lambda G: tok.attention(G, logits=True), batch.clone),
             ("dvae", "forward", lambda G: na(G), na_batch.clone),
             ("dvae", "attention", lambda G: na.attention(G), na_batch.clone),
             ("dvae", "attention logits", lambda G: na.attention(G, logits=True), na_batch.clone)]
    res = {}
    with torch.no_grad():
        for rnd in range(2):   # two interleaved rounds: a drift of the clocks shows as a difference between them
            for shape, case, fn, fresh in cases:
                r = host_ms(fn, fresh, args.steps, args.warmup)
                res.setdefault(shape + " | " + case, []).append(r)
                print("round %d  %-9s %-22s median %.4f ms  p90 %.4f ms  (host, whole pass)" % (rnd, shape, case, r[0], r[1]))
            for case, lg in (("kernels alpha", False), ("kernels alpha+logit", True)):
                r = device_ms(lambda: kernels(lg), args.steps, args.warmup, args.inner)
                res.setdefault("headline | " + case, []).append(r)
                print("round %d  %-9s %-22s median %.4f ms  p90 %.4f ms  (device, per call)" % (rnd, "headline", case, r[0], r[1]))
    tok.check()
    na.check()
    print(json.dumps({"script": "bench_attention", "steps": args.steps, "inner": args.inner, "N": int(batch.x.shape[0]), "E": E,
                      "ms": {k: {"best_round_median": min(m for m, _ in v), "rounds_median_p90": v} for k, v in res.items()}}))


if __name__ == "__main__":
    main()
