"""Time of a `DAGNN_NA(agg='gated_sum')` training step at the reference's shape (dvae/train.py:55: hs = 501; B = 32, L = 2):
(a) the encoder alone, forward + backward (`encode` and a backward of sum(mu) + sum(logvar)), (b) the full step of
dvae/train.py:241-257 (encode, loss, backward, clip 0.25, Adam).  Median of `--steps` steps after `--warmup`, wall clock around
a device synchronisation.  Prints one JSON line.

    python scripts/dvae_gated_train_time.py [--steps 30] [--warmup 5] [--hs 501] [--batch 32]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hs", type=int, default=501)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--layers", type=int, default=2)
    a = ap.parse_args()
    from dagnn_amd import DAGNN_NA, synth
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    graphs = [synth.decode_enas_row(r) for r in synth.enas_rows(5, a.batch)]
    model = DAGNN_NA(8, a.hs, a.hs, 8, 8, 0, 1, hs=a.hs, nz=56, num_nodes=8, num_layers=a.layers, bidirectional=False,
                     agg="gated_sum").to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)

    def encoder():
        opt.zero_grad()
        mu, logvar = model.encode([g.clone() for g in graphs])
        (mu.sum() + logvar.sum()).backward()

    def step():
        opt.zero_grad()
        mu, logvar = model.encode([g.clone() for g in graphs])
        loss, _, _ = model.loss(mu, logvar, graphs)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 0.25)
        opt.step()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    enc = timed(encoder)
    full = timed(step)
    print(json.dumps({"hs": a.hs, "B": a.batch, "L": a.layers, "steps": a.steps,
                      "encoder_fwd_bwd_ms": {"median": round(enc[0], 3), "min": round(enc[1], 3), "max": round(enc[2], 3)},
                      "step_ms": {"median": round(full[0], 3), "min": round(full[1], 3), "max": round(full[2], 3)}}))


if __name__ == "__main__":
    main()
