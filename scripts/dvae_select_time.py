#!/usr/bin/env python
"""Times `decode_from_latent_space` (dagnn_amd/dvae.py) at bo.py's shape - 500 attempts x 50 latent points - for the ENAS
(DAGNN_NA, max_n 8) and BN (DAGNN_BN, max_n 10) models at hs = 501, L = 2, with HIP events, median of --steps calls after
--warmup: the decode alone (`decode_dense`), the validity and selection alone (`select_dense`, csrc/dvae_select.hip), and
the whole call (strings on the host).  Next to it, once per model, the host loop the reference runs on the same rows:
`graphs_from_dense` into DecodedGraph, then is_valid_* and decode_igraph_to_* restated over those graphs and a Counter
per point (wall clock).  Then one JSON line.

    python scripts/dvae_select_time.py [--steps 10] [--warmup 2] [--attempts 500] [--points 50]
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagnn_amd import DAGNN_BN, DAGNN_NA, dvae  # noqa: E402
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


def _valid_dag(g, S, E):   # dvae/util.py:599-618, over a DecodedGraph
    n_start = n_end = 0
    for v in g.vs:
        if v["type"] == S:
            n_start += 1
        elif v["type"] == E:
            n_end += 1
        if v.indegree() == 0 and v["type"] != S:
            return False
        if v.outdegree() == 0 and v["type"] != E:
            return False
    return g.is_dag() and n_start == 1 and n_end == 1


def _valid_enas(g, S, E):   # :621-631
    res = _valid_dag(g, S, E)
    for i in range(g.vcount() - 2):
        res = res and g.are_connected(i, i + 1)
        if not res:
            return res
    return res and g.vs[g.vcount() - 1].indegree() == 1


def _valid_bn(g, S, E, nvt):   # :634-649
    ts = g.vs["type"]
    return g.is_dag() and ts.count(S) == 1 and ts.count(E) == 1 and len(set(ts)) == nvt and g.vcount() == nvt


def _enas(g):   # :168-180
    res, adj = [], g.get_adjlist(dvae.IGRAPH_IN)
    for i in range(1, g.vcount() - 1):
        res.append(int(g.vs[i]["type"]) - 2)
        row = [0] * (i - 1)
        for j in adj[i]:
            if j < i - 1:
                row[j] = 1
        res += row
    return " ".join(str(x) for x in res)


def _bn(g):   # :388-394
    order = np.argsort(g.vs["type"][1:-1]).tolist()
    adj = np.array(g.get_adjacency().data)[1:-1, 1:-1][order][:, order]
    return " ".join(str(x) for x in adj.reshape(-1))


def host_loop(model, d, kind):
    """The reference's post-processing on the decoded rows, after one copy to the host."""
    t0 = time.perf_counter()
    A, B, n = d.types.shape
    host = torch.cat([d.types.view(A * B, n), d.preds.view(A * B, n), d.nv.view(A * B, 1)], 1).cpu().numpy()
    graphs = dvae.graphs_from_dense(host[:, :n], host[:, n:2 * n], host[:, 2 * n], model.END_TYPE, use_igraph=False)
    S, E = model.START_TYPE, model.END_TYPE
    out = []
    for b in range(B):
        cur = []
        for a in range(A):
            g = graphs[a * B + b]
            if kind == "ENAS" and _valid_enas(g, S, E):
                cur.append(_enas(g))
            elif kind == "BN" and _valid_bn(g, S, E, model.nvt):
                cur.append(_bn(g))
        out.append(list(collections.Counter(cur).items())[0][0] if cur else None)
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--attempts", type=int, default=500)
    p.add_argument("--points", type=int, default=50)
    p.add_argument("--hs", type=int, default=501)
    args = p.parse_args()
    dev = torch.device("cuda:0")
    A, B, hs = args.attempts, args.points, args.hs
    res = dict(attempts=A, points=B, hs=hs, L=2)
    for kind, cls, n in (("ENAS", DAGNN_NA, 8), ("BN", DAGNN_BN, 10)):
        model = cls(n, hs, hs, n, n, 0, 1, hs=hs, nz=56, num_nodes=n, num_layers=2, bidirectional=kind == "BN").eval()
        seeded_fill(model, 7)
        model = model.to(dev)
        z = torch.from_numpy(np.random.default_rng(1).standard_normal((B, 56)).astype(np.float32)).to(dev)
        d = model.decode_dense(z, True, attempts=A)
        t_decode = time_call(lambda: model.decode_dense(z, True, attempts=A), args.steps, args.warmup)
        t_select = time_call(lambda: model.select_dense(d, kind), args.steps, args.warmup)
        t_mode = time_call(lambda: model.select_dense(d, kind, select="most_common"), args.steps, args.warmup)
        t_call = time_call(lambda: dvae.decode_from_latent_space(z, model, A, "variable", False, kind), args.steps, args.warmup)
        t_graph = time_call(lambda: dvae.decode_from_latent_space(z, model, A, "variable", True, kind), args.steps, args.warmup)
        torch.manual_seed(3)
        ours = dvae.decode_from_latent_space(z, model, A, "variable", False, kind)
        torch.manual_seed(3)
        d3 = model.decode_dense(z, True, attempts=A)
        ref, t_host = host_loop(model, d3, kind)
        assert ours == ref, kind
        sel = model.select_dense(d3, kind)
        r = dict(decode_ms=t_decode, select_ms=t_select, select_most_common_ms=t_mode, call_ms=t_call,
                 call_igraph_ms=t_graph, host_loop_ms=t_host, valid_fraction=float(sel.valid.float().mean()),
                 points_without_valid=int((sel.pick < 0).sum()))
        print("%-4s decode %.2f ms  select %.3f ms (most_common %.3f)  whole call %.2f ms (return_igraph %.2f)  host loop "
              "%.0f ms  valid %.3f" % (kind, t_decode, t_select, t_mode, t_call, t_graph, t_host, r["valid_fraction"]))
        res[kind.lower()] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
