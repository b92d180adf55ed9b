#!/usr/bin/env python
"""Times the reference-shaped D-VAE training step (dvae/train.py:241-257; scripts/na_train.sh: B = 32, hs = 501, 2 layers,
attn_h) for the ENAS (DAGNN_NA) and BN (DAGNN_BN) models: encode + loss + backward + clip 0.25 + Adam, and the loss
forward + backward alone (csrc/dvae_decode.hip).  Every timed step ends with a device synchronisation; prints median and
p90 per case and the FLOPs the decoder's products perform, then one JSON line.

    python scripts/dvae_train_step.py [--steps 20] [--warmup 5] [--batch 32] [--hs 501] [--layers 2] [--agg attn_h]

--agg gated_sum times the ENAS model with the gated_sum aggregator ('enas_gated') beside its attn_h numbers from the same
run (DAGNN_BN has no gated_sum).
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/dvae_train_step.py --profile
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
from dagnn_amd import DAGNN_BN, DAGNN_NA, synth  # noqa: E402


def decoder_flops(B, n, hs, L, nvt, edge_in, edge_hidden, vertex_hidden, gated=False):
    """Multiply-add FLOPs (x2) of the decoder's dense products, forward; the reverse pass does about twice as many."""
    NU = 1 + sum(v + 1 for v in range(1, n))
    RU, RE, RV = NU * B, n * (n - 1) // 2 * B, (n - 1) * B
    gru = 2 * RU * 3 * hs * hs * (1 + 2 * (L - 1))
    edge = 2 * RE * edge_hidden * edge_in + 2 * RE * edge_hidden
    vert = 2 * RV * (vertex_hidden * hs + nvt * vertex_hidden)
    agg = 2 * (n - 1) * B * 2 * hs * hs if gated else 4 * RU * n * hs   # gated_sum: one message product per vertex
    return gru + edge + vert + agg


def stats(ts):
    ts = np.array(ts) * 1e3
    return float(np.median(ts)), float(np.percentile(ts, 90))


def run(kind, args, dev):
    torch.manual_seed(0)
    B, hs, L = args.batch, args.hs, args.layers
    if kind in ("enas", "enas_gated"):
        n = nvt = 8
        graphs = [synth.decode_enas_row(r) for r in synth.enas_rows(1, B)]
        model = DAGNN_NA(n, hs, hs, n, nvt, 0, 1, hs=hs, nz=56, num_nodes=n, num_layers=L, bidirectional=False,
                         agg="gated_sum" if kind == "enas_gated" else "attn_h")
    else:
        n = nvt = 10
        graphs = [synth.decode_bn_row(r) for r in synth.bn_rows(1, B)]
        model = DAGNN_BN(n, hs, hs, n, nvt, 0, 1, hs=hs, nz=56, num_nodes=n, num_layers=L, bidirectional=True)
    model = model.to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)

    def full():
        opt.zero_grad()
        mu, logvar = model.encode([g.clone() for g in graphs])
        loss, _, _ = model.loss(mu, logvar, graphs)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 0.25)
        opt.step()

    mu0 = torch.randn(B, 56, device=dev)
    lv0 = torch.randn(B, 56, device=dev) * 0.1

    def loss_only():
        mu, lv = mu0.clone().requires_grad_(True), lv0.clone().requires_grad_(True)
        loss, _, _ = model.loss(mu, lv, graphs)
        loss.backward()

    out = {}
    for name, fn in (("step", full), ("loss_fwd_bwd", loss_only)):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[name + "_ms_median"], out[name + "_ms_p90"] = stats(ts)
    e = model.add_edge[0].weight
    out["decoder_fwd_gflop"] = decoder_flops(B, n, hs, L, nvt, e.shape[1], e.shape[0],
                                             model.add_vertex[0].weight.shape[0], kind == "enas_gated") / 1e9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hs", type=int, default=501)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--agg", choices=("attn_h", "gated_sum"), default="attn_h")
    ap.add_argument("--profile", action="store_true", help="few steps, for a separate rocprofv3 --kernel-trace --stats run")
    args = ap.parse_args()
    if args.profile:
        args.steps, args.warmup = 5, 2
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    dev = torch.device("cuda")
    res = {}
    for kind in ("enas", "bn") if args.agg == "attn_h" else ("enas", "enas_gated"):
        r = run(kind, args, dev)
        res[kind] = r
        print("%-10s B=%d hs=%d L=%d  step %.2f ms (p90 %.2f)  loss fwd+bwd %.2f ms (p90 %.2f)  decoder fwd %.2f GFLOP"
              % (kind, args.batch, args.hs, args.layers, r["step_ms_median"], r["step_ms_p90"], r["loss_fwd_bwd_ms_median"],
                 r["loss_fwd_bwd_ms_p90"], r["decoder_fwd_gflop"]))
    print(json.dumps(dict(workload="dvae_train_step", batch=args.batch, hs=args.hs, layers=args.layers, steps=args.steps, **res)))


if __name__ == "__main__":
    main()
