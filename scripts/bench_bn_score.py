#!/usr/bin/env python
"""Times BIC scoring of Bayesian networks (dagnn_amd/bn_score.py, csrc/bn_score.hip) on Asia-shaped data.

  bn_scores        M = --structures random BN structures (8 variables) on `synth.asia_samples(0, 5000)`, by HIP events around
                   the call, both staging paths ('lds': the table staged once per workgroup; 'global': streamed)
  store_scores     the same structures as a `DagStore` of dense BN rows (rows -> masks kernel + score kernel + the fills)
  decode_and_score a BO round - --points latent points x --attempts decode attempts on a DAGNN_BN (hs = 501, 2 layers) -
                   beside `decode_from_latent_space` alone, wall clock including the one synchronisation
  host             the yardstick: the module's float64 numpy mirror `scores_host` on --host-structures of the same structures,
                   per structure (it is never the code under test against itself; the device scores are checked against it
                   before anything is timed)

Median over --steps after --warmup.  One JSON line at the end.

    python scripts/bench_bn_score.py [--structures 200000] [--steps 10] [--warmup 3]
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
from dagnn_amd import DAGNN_BN, DagStore, dvae, engine, synth  # noqa: E402
from dagnn_amd.bn_score import BnData, bn_scores, decode_and_score, scores_host, store_scores  # noqa: E402


def random_bn_rows(seed, M, n=10):
    """Dense rows (types, preds) int32 [M, n] of M random valid BN graphs: middle types a permutation, parent w.p. 0.3."""
    rng = np.random.default_rng(seed)
    k = n - 2
    types = np.zeros((M, n), dtype=np.int32)
    types[:, 1:n - 1] = 2 + np.argsort(rng.random((M, k)), axis=1)
    types[:, n - 1] = 1
    preds = np.zeros((M, n), dtype=np.uint32)
    loose = np.ones((M, n), dtype=bool)
    for v in range(1, n - 1):
        for u in range(1, v):
            e = rng.random(M) < 0.3
            preds[:, v] |= e.astype(np.uint32) << np.uint32(u)
            loose[:, u] &= ~e
        preds[:, v] |= (preds[:, v] == 0).astype(np.uint32)
    for u in range(1, n - 1):
        preds[:, n - 1] |= loose[:, u].astype(np.uint32) << np.uint32(u)
    return types, preds.view(np.int32)


def event_ms(fn, steps, warmup):
    ts = []
    for k in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.percentile(ts, 90))


def wall_ms(fn, steps, warmup):
    ts = []
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.percentile(ts, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=200000)
    ap.add_argument("--host-structures", type=int, default=2000)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--points", type=int, default=50)
    ap.add_argument("--attempts", type=int, default=500)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bn_score: needs a GPU (the host mirror is only the yardstick)")
    dev = torch.device("cuda:0")
    M = args.structures
    X = synth.asia_samples(0, args.samples)
    data = BnData.from_samples(X, [2] * 8, device=dev)
    types, preds = random_bn_rows(1, M)
    store = DagStore.from_dense(types, preds, 10, dev)
    nv = torch.full((M,), 10, dtype=torch.int32, device=dev)
    parents, valid = engine.bn_rows_to_parents(store.arrays["types"], store.arrays["preds"], nv, 10, 0, 1)
    assert bool(valid.all())
    res = {"script": "bench_bn_score", "structures": M, "samples": args.samples, "steps": args.steps, "warmup": args.warmup}

    # ---------------------------------------------------------------- the yardstick, and the check against it
    H = min(args.host_structures, M)
    host_masks = parents[:H].cpu().numpy().view(np.uint32)
    t0 = time.perf_counter()
    want = scores_host(X, data.cards, host_masks)
    res["host_us_per_structure"] = (time.perf_counter() - t0) / H * 1e6
    for stage in ("lds", "global"):
        got = bn_scores(data, parents[:H], stage=stage)[0].cpu().numpy()
        assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), stage
    print("host mirror: %.1f us per structure (%d structures)" % (res["host_us_per_structure"], H))

    # ---------------------------------------------------------------- bn_scores, both staging paths
    for stage in ("lds", "global"):
        med, p90 = event_ms(lambda: bn_scores(data, parents, stage=stage), args.steps, args.warmup)
        res["bn_scores_%s_ms" % stage] = [med, p90]
        print("bn_scores %-6s M=%d: %.3f ms (p90 %.3f) = %.1f ns per structure" % (stage, M, med, p90, med * 1e6 / M))

    # ---------------------------------------------------------------- store_scores
    a = store_scores(data, store)[0]
    assert torch.equal(a.view(torch.int64), bn_scores(data, parents)[0].view(torch.int64))
    med, p90 = event_ms(lambda: store_scores(data, store), args.steps, args.warmup)
    res["store_scores_ms"] = [med, p90]
    print("store_scores M=%d: %.3f ms (p90 %.3f)" % (M, med, p90))

    # ---------------------------------------------------------------- a BO round
    torch.manual_seed(0)
    model = DAGNN_BN(10, 501, 501, 10, 10, 0, 1, hs=501, nz=56, num_nodes=10, num_layers=2, bidirectional=True).to(dev).eval()
    z = torch.randn(args.points, 56, device=dev)
    st, se = dvae.draw_shapes(10, args.points, args.attempts)
    draws = (torch.rand(st, device=dev), torch.rand(se, device=dev))
    steps, warmup = max(3, args.steps // 2), 2
    both = wall_ms(lambda: decode_and_score(z, model, data, args.attempts, draws=draws), steps, warmup)
    alone = wall_ms(lambda: dvae.decode_from_latent_space(z, model, args.attempts, "variable", False, "BN", draws=draws), steps, warmup)
    both2 = wall_ms(lambda: decode_and_score(z, model, data, args.attempts, draws=draws), steps, warmup)
    res["decode_and_score_ms"] = [min(both[0], both2[0]), max(both[1], both2[1])]
    res["decode_from_latent_space_ms"] = list(alone)
    print("BO round %d x %d: decode_and_score %.2f ms, decode_from_latent_space alone %.2f ms (difference %.2f ms)"
          % (args.points, args.attempts, res["decode_and_score_ms"][0], alone[0], res["decode_and_score_ms"][0] - alone[0]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
