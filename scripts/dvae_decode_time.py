#!/usr/bin/env python
"""Times `decode_dense` (the sampling D-VAE decoder, csrc/dvae_sample.hip) with HIP events, median of --steps calls
after --warmup, for the ENAS (DAGNN_NA, max_n 8) and BN (DAGNN_BN, max_n 10) models at hs = 501, L = 2:
B = 32 argmax and sampled, and --attempts attempts x 32 points sampled.  For the large case it reports the FLOPs of the
MFMA products the call issues and their share of the fp32 matrix peak (157.3 TFLOP/s) over the whole call; then one
JSON line.

    python scripts/dvae_decode_time.py [--steps 20] [--warmup 3] [--attempts 500] [--hs 501] [--agg attn_h]

--agg gated_sum times the ENAS model with the gated_sum aggregator ('enas_gated') beside its attn_h numbers from the same
run (DAGNN_BN has no gated_sum).
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/dvae_decode_time.py --steps 3 --warmup 1
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagnn_amd import DAGNN_BN, DAGNN_NA  # noqa: E402
from oracle.seeding import seeded_fill  # noqa: E402

PEAK_F32_MATRIX = 157.3e12


def product_flops(R, n, hs, L, edge_hidden, vertex_hidden, bn, gated=False):
    """FLOPs (2 per multiply-add) of the MFMA products of one call, on the padded width HP = hs rounded up to 4."""
    HP = (hs + 3) // 4 * 4
    updates = 1 + sum(idx + 1 for idx in range(1, n - 1)) + 2   # idx = n-1: the fresh update and the END step only
    agg_updates = updates - (n - 1)                             # the fresh updates skip the W_hh product
    gh = 2 * R * HP * 3 * hs * L * agg_updates
    gi = 2 * R * HP * 3 * hs * (L - 1) * updates
    edge_steps = sum(range(1, n - 1))
    edge = 2 * R * HP * edge_hidden * (edge_steps + (n - 1) + (1 if bn else 0))   # H_v part per step, H_vi part per vertex, H0
    vert = 2 * R * HP * vertex_hidden * (n - 2)
    msg = 2 * R * HP * 2 * hs * (n - 1) if gated else 0   # gated_sum: one message product per final vertex
    return gh + gi + edge + vert + msg


def time_call(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.percentile(ts, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--attempts", type=int, default=500)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hs", type=int, default=501)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--agg", choices=("attn_h", "gated_sum"), default="attn_h")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hs, L, B = args.hs, args.layers, args.batch
    res = {}
    for kind in ("enas", "bn") if args.agg == "attn_h" else ("enas", "enas_gated"):
        if kind in ("enas", "enas_gated"):
            model = DAGNN_NA(8, hs, hs, 8, 8, 0, 1, hs=hs, nz=56, num_nodes=8, num_layers=L, bidirectional=False,
                             agg="gated_sum" if kind == "enas_gated" else "attn_h")
        else:
            model = DAGNN_BN(10, hs, hs, 10, 10, 0, 1, hs=hs, nz=56, num_nodes=10, num_layers=L, bidirectional=True)
        seeded_fill(model, 7)
        model = model.to(dev).eval()
        z = torch.randn(B, 56, generator=torch.Generator().manual_seed(1)).to(dev)
        for stochastic in (False, True):
            tag = "%s_B%d_%s" % (kind, B, "sample" if stochastic else "argmax")
            med, p90 = time_call(lambda: model.decode_dense(z, stochastic), args.steps, args.warmup)
            res[tag] = dict(median_ms=med, p90_ms=p90)
            print("%-28s median %8.3f ms   p90 %8.3f ms" % (tag, med, p90))
        A = args.attempts
        tag = "%s_%dx%d_sample" % (kind, A, B)
        med, p90 = time_call(lambda: model.decode_dense(z, True, attempts=A), max(3, args.steps // 4), 1)
        fl = product_flops(A * B, model.max_n, hs, L, model.add_edge[0].weight.shape[0], model.add_vertex[0].weight.shape[0],
                           kind == "bn", kind == "enas_gated")
        frac = fl / (med * 1e-3) / PEAK_F32_MATRIX
        res[tag] = dict(median_ms=med, p90_ms=p90, product_tflop=fl / 1e12, product_peak_fraction=frac)
        print("%-28s median %8.3f ms   p90 %8.3f ms   products %.2f TFLOP = %.1f %% of the fp32 matrix peak over the call"
              % (tag, med, p90, fl / 1e12, 100 * frac))
        del model
        torch.cuda.empty_cache()
    print(json.dumps(dict(metric="dvae_decode_ms", hs=hs, L=L, B=B, attempts=args.attempts, results=res)))


if __name__ == "__main__":
    main()
