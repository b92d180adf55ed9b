#!/usr/bin/env python
"""Times the BN D-VAE decoders with type-keyed attention (`agg='attn_x'`: a slot's score is a table entry,
csrc/dvae_decode.hip / csrc/dvae_sample.hip) beside the state-keyed ones they stand next to (`agg='attn_h'`: a slot's score
is a product with a state row), in this process, on the same graphs and latent points.

  loss_ms      `loss_dense(mu, logvar, types, preds)` forward + backward (the teacher-forced decoder and its reverse pass) at
               B = 32, hs = 501, L = 2 on `synth.bn_rows` graphs
  decode_ms    `decode_dense(z, stochastic=True)` of the same B latent rows with fixed draws

Median (and p90) over `--steps` after `--warmup`; the two aggregators alternate in two rounds and the better round is
reported.  One JSON line at the end.

    python scripts/bench_dvae_attn_x.py [--steps 50] [--warmup 10] [--batch 32] [--hs 501] [--layers 2]
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
from dagnn_amd import DAGNN_BN, synth  # noqa: E402
from dagnn_amd.dvae import decode_schedule, draw_shapes  # noqa: E402

N = 10


def stats(ts, scale):
    ts = np.array(ts) * scale
    return [float(np.median(ts)), float(np.percentile(ts, 90))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hs", type=int, default=501)
    ap.add_argument("--layers", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dvae_attn_x: needs a GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    B, hs, L = args.batch, args.hs, args.layers

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

    graphs = [synth.decode_bn_row(r) for r in synth.bn_rows(1, B)]
    types, preds = (torch.from_numpy(t).to(dev) for t in decode_schedule(graphs, N, N, 0))
    rng = np.random.default_rng(0)
    mu = torch.from_numpy(rng.standard_normal((B, 56)).astype(np.float32)).to(dev).requires_grad_(True)
    logvar = torch.from_numpy((0.3 * rng.standard_normal((B, 56))).astype(np.float32)).to(dev).requires_grad_(True)
    st, se = draw_shapes(N, B, 1)
    gen = torch.Generator(device=dev).manual_seed(1)
    draws = (torch.rand(st, device=dev, generator=gen), torch.rand(se, device=dev, generator=gen))
    steps = {}
    for agg in ("attn_h", "attn_x"):
        torch.manual_seed(0)
        model = DAGNN_BN(N, hs, hs, N, N, 0, 1, hs=hs, nz=56, num_nodes=N, num_layers=L, bidirectional=True, agg=agg).to(dev).eval()

        def loss_step(model=model):
            model.zero_grad(set_to_none=True)
            mu.grad = logvar.grad = None
            model.loss_dense(mu, logvar, types, preds)[0].backward()

        def decode_step(model=model):
            model.decode_dense(mu.detach(), True, draws=draws)

        steps[agg] = (loss_step, decode_step)
    rounds = {agg: {"loss_ms": [], "decode_ms": []} for agg in steps}
    for _ in range(2):   # two alternating rounds: a drift shows as a difference between them
        for agg, (loss_step, decode_step) in steps.items():
            rounds[agg]["loss_ms"].append(stats(timed(loss_step), 1e3))
            rounds[agg]["decode_ms"].append(stats(timed(decode_step), 1e3))
    res = {"script": "bench_dvae_attn_x", "steps": args.steps, "warmup": args.warmup, "batch": B, "hs": hs, "layers": L}
    for agg in steps:
        res[agg] = dict(loss_ms_median=min(m for m, _ in rounds[agg]["loss_ms"]),
                        decode_ms_median=min(m for m, _ in rounds[agg]["decode_ms"]), rounds=rounds[agg])
        print("%-6s B=%d hs=%d L=%d: loss forward + backward %.3f ms, decode_dense %.3f ms"
              % (agg, B, hs, L, res[agg]["loss_ms_median"], res[agg]["decode_ms_median"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
