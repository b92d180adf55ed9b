#!/usr/bin/env python
"""Times the D-VAE evaluation metrics (dagnn_amd/dvae.py, csrc/dvae_match.hip) for the ENAS (DAGNN_NA, max_n 8) and BN
(DAGNN_BN, max_n 10) models at hs = 501, L = 2, with HIP events, median of --steps calls after --warmup:

  recon     `recon_accuracy` at B = 32 graphs, 10 encodes x 10 decodes: the whole call, its decodes alone (the same ten
            `decode_dense(attempts=10)` calls) and the compare-and-count alone (ten `same_dag_dense` calls);
  prior     `prior_validity` at 1000 points x 10 decodes against a training set of 19 020 (ENAS) / 180 000 (BN) seeded
            synthetic rows: the whole call, its decode alone, and everything after the decode (select_dense, the distinct
            set, the training-set lookup); the one-time build of the training set is timed separately.

Next to each, once, by wall clock: what a caller without these functions has to do for the same numbers - the same
`decode_dense` calls, one copy of the rows to the host, then the host mirrors (`same_dag_host`; `select_host`, the
string forms into a Python set, and a Python set of training records with its build).  The counts must agree.  Last, the
largest supported set: build from 2^20 rows of 32 vertices and a query of 2^20 rows.  Then one JSON line.

    python scripts/dvae_eval_time.py [--steps 10] [--warmup 2]
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
from dagnn_amd import DAGNN_BN, DAGNN_NA, dvae, synth  # noqa: E402
from oracle.seeding import seeded_fill  # noqa: E402


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
    return float(np.median(ts))


def train_rows(kind, N, n, nvt, decoded):
    """N seeded training rows: decoder-shaped rows of another seed, and every 16th one a row of `decoded` (so that the
    lookup has something to find)."""
    t, p, k = (x[0] for x in synth.decoded_rows(11, kind, 1, 4096, n, nvt))
    idx = np.random.default_rng(12).integers(0, 4096, size=N)
    rows = [t[idx].copy(), p[idx].copy(), k[idx].copy()]
    flip = np.random.default_rng(13).integers(1, n - 1, size=N)   # one bit per row: 4096 templates become ~N distinct rows
    rows[1][np.arange(N), flip] ^= (1 << np.random.default_rng(14).integers(0, flip)).astype(np.int32)
    flat = [x.reshape((-1,) + x.shape[2:]) for x in decoded]
    src = np.random.default_rng(15).integers(0, flat[0].shape[0], size=(N + 15) // 16)
    for r, f in zip(rows, flat):
        r[::16] = f[src]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--hs", type=int, default=501)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hs, P, E, D, B = args.hs, args.points, 10, 10, 32
    res = dict(hs=hs, L=2, points=P, decode_times=D, recon_graphs=B)
    for kind, cls, n, N in (("ENAS", DAGNN_NA, 8, 19020), ("BN", DAGNN_BN, 10, 180000)):
        model = cls(n, hs, hs, n, n, 0, 1, hs=hs, nz=56, num_nodes=n, num_layers=2, bidirectional=kind == "BN").eval()
        seeded_fill(model, 7)
        model = model.to(dev)
        r = {}
        # ---- reconstruction accuracy
        graphs = [(synth.decode_enas_row if kind == "ENAS" else synth.decode_bn_row)(row)
                  for row in (synth.enas_rows if kind == "ENAS" else synth.bn_rows)(3, B)]
        tt, pt, nt = (torch.from_numpy(x).to(dev) for x in dvae.dense_rows(graphs, n, n))
        with torch.no_grad():
            mu, _ = model.encode(graphs)
        draws = dvae._take_draws(None, n, B, E * D, dev, "")
        dr = [(draws[0][e * D:(e + 1) * D].contiguous(), draws[1][e * D:(e + 1) * D].contiguous()) for e in range(E)]
        decs = [model.decode_dense(mu, True, D, dr[e]) for e in range(E)]
        r["recon_call_ms"] = time_call(lambda: dvae.recon_accuracy(model, graphs, E, D, draws=draws), args.steps, args.warmup)
        r["recon_encode_ms"] = time_call(lambda: model.encode(graphs), args.steps, args.warmup)
        r["recon_decode_ms"] = time_call(lambda: [model.decode_dense(mu, True, D, dr[e]) for e in range(E)], args.steps, args.warmup)
        r["recon_match_ms"] = time_call(lambda: [dvae.same_dag_dense(d, tt, pt, nt) for d in decs], args.steps, args.warmup)
        ours = dvae.recon_accuracy(model, graphs, E, D, draws=draws)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = torch.cat([torch.cat([d.types, d.preds, d.nv.unsqueeze(2)], 2) for d in decs]).cpu().numpy()
        same = dvae.same_dag_host(host[..., :n], host[..., n:2 * n], host[..., 2 * n], *(x.cpu().numpy() for x in (tt, pt, nt)))
        r["recon_host_after_decode_ms"] = 1e3 * (time.perf_counter() - t0)
        assert ours[0] == same[2] and ours[2].tolist() == same[1].tolist(), kind
        r["recon_perfect"] = ours[0]
        # ---- prior validity
        z = torch.from_numpy(np.random.default_rng(1).standard_normal((P, 56)).astype(np.float32)).to(dev)
        pdraws = dvae._take_draws(None, n, P, D, dev, "")
        d = model.decode_dense(z, True, D, pdraws)
        dense = [x.cpu().numpy() for x in (d.types, d.preds, d.nv)]
        rows = train_rows(kind, N, n, n, dense)
        dev_rows = [torch.from_numpy(x).to(dev) for x in rows]
        train = dvae.GraphSet.from_dense(*dev_rows)
        W = dvae.select_key_words(kind, n, n)

        def after_decode():
            sel = model.select_dense(d, kind)
            keys = dvae.DistinctKeys(W, P * D, dev)
            keys.add(sel.keys, sel.valid)
            return train.contains(d, sel.valid)
        r["train_rows"] = N
        r["train_build_ms"] = time_call(lambda: dvae.GraphSet.from_dense(*dev_rows), args.steps, args.warmup)
        r["prior_call_ms"] = time_call(lambda: dvae.prior_validity(model, train, decode_times=D, data_type=kind, z=z, draws=pdraws),
                                       args.steps, args.warmup)
        r["prior_decode_ms"] = time_call(lambda: model.decode_dense(z, True, D, pdraws), args.steps, args.warmup)
        r["prior_after_decode_ms"] = time_call(after_decode, args.steps, args.warmup)
        ours = dvae.prior_validity(model, train, decode_times=D, data_type=kind, z=z, draws=pdraws)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = torch.cat([d.types, d.preds, d.nv.unsqueeze(2)], 2).cpu().numpy()
        ht, hp, hk = host[..., :n], host[..., n:2 * n], host[..., 2 * n]
        valid = dvae.select_host(ht, hp, hk, kind, n, 0, 1)[0]
        form = dvae.enas_string if kind == "ENAS" else dvae.bn_adj_string
        strings = {form(ht[a, b], hp[a, b], hk[a, b]) for a, b in zip(*np.nonzero(valid))}
        t1 = time.perf_counter()
        host_set = dvae.GraphSet.from_dense(*rows)
        t2 = time.perf_counter()
        n_in = int(host_set.contains((ht, hp, hk), valid.astype(np.int32))[1])
        t3 = time.perf_counter()
        r["prior_host_after_decode_ms"] = 1e3 * ((t1 - t0) + (t3 - t2))
        r["train_build_host_ms"] = 1e3 * (t2 - t1)
        assert (ours.n_valid, ours.n_unique, ours.n_in_train) == (int(valid.sum()), len(strings), n_in), kind
        r.update(n_valid=ours.n_valid, n_unique=ours.n_unique, n_in_train=ours.n_in_train, train_distinct=train.distinct())
        print("%-4s recon: call %.2f ms = encode %.2f + decode %.2f + match %.3f (host after decode %.1f ms) | prior: call %.2f ms "
              "= decode %.2f + after %.3f (host after decode %.0f ms) | set build %.3f ms (host %.0f ms) | valid %d unique %d "
              "in train %d" % (kind, r["recon_call_ms"], r["recon_encode_ms"], r["recon_decode_ms"], r["recon_match_ms"],
                               r["recon_host_after_decode_ms"], r["prior_call_ms"], r["prior_decode_ms"], r["prior_after_decode_ms"],
                               r["prior_host_after_decode_ms"], r["train_build_ms"], r["train_build_host_ms"], ours.n_valid,
                               ours.n_unique, ours.n_in_train))
        res[kind.lower()] = r
    # ---- the largest supported sizes: 2^20 training rows of 32 vertices, 2^20 queried rows (half of them stored rows)
    N, n = 1 << 20, 32
    gen = torch.Generator(device=dev).manual_seed(5)
    big = [torch.randint(0, 64, (N, n), generator=gen, device=dev, dtype=torch.int32),
           torch.randint(0, 1 << 31, (N, n), generator=gen, device=dev, dtype=torch.int32),
           torch.randint(2, n + 1, (N,), generator=gen, device=dev, dtype=torch.int32)]
    query = [torch.cat([x[:N // 2], y[N // 2:]]) for x, y in zip(big, [t.flip(0) ^ 1 if t.dim() == 2 else t.flip(0) for t in big])]
    train = dvae.GraphSet.from_dense(*big)
    hits = int(train.contains(tuple(query))[1])
    res["large"] = dict(rows=N, n=n, storage_mb=train._dev.storage.numel() * 4 / 1e6, hits=hits, distinct=train.distinct(),
                        build_ms=time_call(lambda: dvae.GraphSet.from_dense(*big), args.steps, args.warmup),
                        query_ms=time_call(lambda: train.contains(tuple(query)), args.steps, args.warmup))
    print("large: 2^20 rows x 32 vertices: build %.2f ms, query of 2^20 rows %.2f ms (%d hits, %.0f MB)"
          % (res["large"]["build_ms"], res["large"]["query_ms"], hits, res["large"]["storage_mb"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
