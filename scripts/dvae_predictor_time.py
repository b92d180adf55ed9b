#!/usr/bin/env python
"""Times the D-VAE performance predictor (dagnn_amd/predictor.py, csrc/predictor.hip) on one GPU against its torch-ops form -
`model.predictor(mu)` + `model.mseloss` + autograd, the baseline: the reference's own lines, same process, same GPU:

  * `predictor_mse` forward + backward at B = 32 and 128, nz = 56, hs = 501 (dvae/train.py:244-247, 255);
  * `predict_latent` over M = 19 020 latent rows (the ENAS Z_train of bo.py:251, 277);
  * the whole training step of scripts/dvae_train_step.py's shape (ENAS, B = 32, hs = 501, 2 layers: encode + loss + backward
    + clip 0.25 + Adam) without the predictor, with `predictor_mse`, and with the torch-ops predictor.

The predictor is not where a step's time goes (under 2 MFLOP at B = 32): the numbers say what the branch ADDS to a step.
The small calls are timed in windows of `--calls` back-to-back calls closed by one device synchronisation (time per call =
window / calls: what a loop that never reads back pays), the variants alternating window by window; a step is timed call
by call, each closed by a synchronisation.  Medians and p90 over the windows; then one JSON line.

    python scripts/dvae_predictor_time.py [--windows 15] [--calls 200] [--steps 20] [--warmup 5]
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
from dagnn_amd import DAGNN_NA, attach_predictor, predict_latent, predictor_mse, synth  # noqa: E402

NZ, HS = 56, 501


def alternate(fns, windows, calls, warmup):
    """{name: (median, p90) of the time per call in microseconds}: the variants take turns, window by window."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) / calls * 1e6)
    return {k: (float(np.median(v)), float(np.percentile(v, 90))) for k, v in ts.items()}


def mse_case(model, B, dev, args):
    gen = torch.Generator().manual_seed(B)
    mu0 = torch.randn(B, NZ, generator=gen).to(dev)
    y = torch.rand(B, generator=gen).to(dev)

    def fused():
        model.zero_grad(set_to_none=True)
        predictor_mse(model, mu0.detach().requires_grad_(True), y)[0].backward()

    def torch_ops():
        model.zero_grad(set_to_none=True)
        model.mseloss(model.predictor(mu0.detach().requires_grad_(True)), y.unsqueeze(1)).backward()

    return alternate({"fused": fused, "torch": torch_ops}, args.windows, args.calls, args.warmup)


def latent_case(model, M, dev, args):
    Z = torch.randn(M, NZ, generator=torch.Generator().manual_seed(M)).to(dev)

    def torch_ops():
        with torch.no_grad():
            model.predictor(Z)

    return alternate({"fused": lambda: predict_latent(model, Z), "torch": torch_ops}, args.windows, args.calls, args.warmup)


def step_case(dev, args):
    torch.manual_seed(0)
    B, n = 32, 8
    graphs = [synth.decode_enas_row(r) for r in synth.enas_rows(1, B)]
    y = torch.rand(B, generator=torch.Generator().manual_seed(1)).to(dev)
    model = attach_predictor(DAGNN_NA(n, HS, HS, n, n, 0, 1, hs=HS, nz=NZ, num_nodes=n, num_layers=2, bidirectional=False)).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)

    def step(how):
        opt.zero_grad()
        mu, logvar = model.encode([g.clone() for g in graphs])
        loss, _, _ = model.loss(mu, logvar, graphs)
        if how == "fused":
            loss = loss + predictor_mse(model, mu, y)[0]
        elif how == "torch":
            loss = loss + model.mseloss(model.predictor(mu), y.unsqueeze(1))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 0.25)
        opt.step()

    fns = {"plain": lambda: step(None), "fused": lambda: step("fused"), "torch": lambda: step("torch")}
    return alternate(fns, args.steps, 1, args.warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=19020)
    args = ap.parse_args()
    if min(args.windows, args.calls, args.steps) < 1:
        raise SystemExit("--windows, --calls and --steps must be >= 1")
    dev = torch.device("cuda")
    torch.manual_seed(0)

    class Shape(torch.nn.Module):
        nz, hs = NZ, HS

    model = attach_predictor(Shape()).to(dev)
    res = {}
    for B in (32, 128):
        r = res["mse_B%d" % B] = mse_case(model, B, dev, args)
        print("predictor_mse fwd+bwd  B=%-4d nz=%d hs=%d   fused %.1f us (p90 %.1f)   torch ops %.1f us (p90 %.1f)"
              % (B, NZ, HS, r["fused"][0], r["fused"][1], r["torch"][0], r["torch"][1]))
    r = res["latent_M%d" % args.rows] = latent_case(model, args.rows, dev, args)
    print("predict_latent         M=%-6d              fused %.1f us (p90 %.1f)   torch ops %.1f us (p90 %.1f)"
          % (args.rows, r["fused"][0], r["fused"][1], r["torch"][0], r["torch"][1]))
    r = res["step"] = step_case(dev, args)
    print("training step (ENAS, B=32, hs=%d, L=2)   plain %.2f ms (p90 %.2f)   + fused %.2f ms (p90 %.2f)   + torch ops %.2f ms (p90 %.2f)"
          % ((HS,) + tuple(v / 1e3 for k in ("plain", "fused", "torch") for v in r[k])))
    print(json.dumps(dict(workload="dvae_predictor_time", nz=NZ, hs=HS, windows=args.windows, calls=args.calls, steps=args.steps,
                          us_median_p90=res)))


if __name__ == "__main__":
    main()
