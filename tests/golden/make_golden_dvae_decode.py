#!/usr/bin/env python
"""Generate the `dvae_decode_*` fixtures from the REAL reference's `DVAE_PYG.decode()` (dvae/models_pyg.py:338-396).

Runs only in the build container (needs the reference).  The reference's `DAGNN` / `DAGNN_BN` run unmodified in eval()
mode on an igraph stand-in (tests/golden/decode_standin, ahead of oracle/pyg_standin on the path).  Three things are
wrapped at run time, not copied:
  - `np.random.choice`: fed seeded float32 uniforms through numpy's own rule (searchsorted(cumsum(p)/sum(p), u,
    'right')), recorded as u_type [1, n, B];
  - `torch.rand_like`: returns seeded float32 uniforms, recorded as u_edge [1, n(n-1)/2, B] in call order;
  - `_ipropagate_to`: records the padding width P of every call, and whether some graph being updated had fewer
    predecessors than P (its P came from another graph).
Each fixture stores z, the draws, every decoded graph (types, predecessor bitmasks, vertex counts), the final top-layer
states (kept by the stand-in when the reference deletes them) and the smallest decision margin; seeds whose margin is
below 1e-4 are rejected, so exact graph equality does not hinge on fp32 rounding.

    python tests/golden/make_golden_dvae_decode.py
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _save, _setup_paths  # noqa: E402
from oracle.seeding import seeded_fill  # noqa: E402

MIN_MARGIN = 1e-4


def _decode(model, z, n, B, stochastic, draw_seed):
    """Run the reference's decode() once; returns (graphs, u_type, u_edge, widths, coupled, margin).  The margin only
    counts decisions the decode reads: the type of vertex idx in graphs that get one, the edge steps (idx, vi) of
    graphs whose vertex idx is not END."""
    rng = np.random.default_rng(draw_seed)
    NE = n * (n - 1) // 2
    u_type = rng.random((n, B), dtype=np.float32)
    u_edge = rng.random((NE, B), dtype=np.float32)
    u_type[0] = u_type[n - 1] = 0.0   # (rows the decode never reads)
    state = dict(choice=0, edge=0)
    type_gap = np.full((n, B), np.inf)    # per (idx, row): distance of the decision from flipping
    edge_gap = np.full((NE, B), np.inf)
    widths, coupled = [], []

    def choice(a, p=None, **_):
        k = state["choice"]
        state["choice"] += 1
        u = float(u_type[1 + k // B, k % B])
        cdf = np.asarray(p, dtype=np.float64).cumsum()
        cdf /= cdf[-1]
        type_gap[1 + k // B, k % B] = float(np.min(np.abs(cdf[:-1] - u))) if len(cdf) > 1 else np.inf
        return list(a)[int(cdf.searchsorted(u, side="right"))]

    def rand_like(t, **_):
        k = state["edge"]
        state["edge"] += 1
        u = torch.from_numpy(u_edge[k].copy()).view(t.shape).to(t.dtype)
        edge_gap[k] = (u - t.detach()).abs().view(-1).double().numpy()
        return u

    calls = dict(vertex=0, edge=0)

    def vertex_hook(_m, _i, out):
        if not stochastic:
            top = torch.topk(out.detach(), 2, dim=1).values
            type_gap[1 + calls["vertex"]] = (top[:, 0] - top[:, 1]).double().numpy()
        calls["vertex"] += 1

    def edge_hook(_m, _i, out):
        if not stochastic:
            edge_gap[calls["edge"]] = (torch.sigmoid(out.detach()) - 0.5).abs().view(-1).double().numpy()
        calls["edge"] += 1

    inner = model._ipropagate_to

    def wrapped(G, v, propagator, H=None, reverse=False):
        alive = [g for g in G if g.vcount() > v]
        counts = [len(g.predecessors(v)) for g in alive] if H is None else [0]
        widths.append(max(counts) if counts else 0)
        coupled.append(int(bool(counts) and min(counts) < max(counts)))
        return inner(G, v, propagator, H, reverse)

    model._ipropagate_to = wrapped
    h1 = model.add_vertex.register_forward_hook(vertex_hook)
    h2 = model.add_edge.register_forward_hook(edge_hook)
    saved = np.random.choice, torch.rand_like
    np.random.choice, torch.rand_like = choice, rand_like
    try:
        with torch.no_grad():
            G = model.decode(z, stochastic=stochastic)
    finally:
        np.random.choice, torch.rand_like = saved
        h1.remove()
        h2.remove()
        del model._ipropagate_to
    assert calls["vertex"] == n - 2 and calls["edge"] == NE, (calls, n)
    if stochastic:
        assert state["choice"] == (n - 2) * B and state["edge"] == NE, (state, n, B)
    margin = np.inf
    for b, g in enumerate(G):
        k = g.vcount()
        types = g.vs["type"]
        for idx in range(1, min(k, n - 1)):
            margin = min(margin, type_gap[idx, b])
        for idx in range(1, k):
            if types[idx] != model.END_TYPE:
                for vi in range(idx - 1, -1, -1):
                    margin = min(margin, edge_gap[idx * (idx - 1) // 2 + (idx - 1 - vi), b])
    return G, u_type, u_edge, widths, coupled, float(margin)


def make_decode(ref_mod, cls_name, name, *, kind, hs, L, B, w_seed, z_seed, stochastic):
    nvt = n = 8 if kind == "na" else 10
    model = getattr(ref_mod, cls_name)(nvt, hs, hs, n, nvt, 0, 1, hs=hs, nz=56, num_nodes=nvt, agg="attn_h",
                                       num_layers=L, bidirectional=kind == "bn", out_wx=False, out_pool_all=False,
                                       out_pool="max", dropout=0.0).eval()
    for attempt in range(50):
        # (argmax decodes of a vertex without predecessors do not depend on z: a flat decision there needs other weights)
        ws, seed = w_seed + 100 * attempt, z_seed + 1000 * attempt
        seeded_fill(model, ws)
        rng = np.random.default_rng(seed)
        z = torch.from_numpy(rng.standard_normal((B, 56)).astype(np.float32))
        G, u_type, u_edge, widths, coupled, margin = _decode(model, z, n, B, stochastic, seed + 1)
        if margin >= MIN_MARGIN:
            break
        print("%s: seeds %d / %d rejected (margin %.2e)" % (name, ws, seed, margin))
    else:
        raise SystemExit("%s: no seed with a decision margin >= %g" % (name, MIN_MARGIN))
    types = np.full((B, n), -1, dtype=np.int32)
    preds = np.zeros((B, n), dtype=np.int64)
    nv = np.zeros(B, dtype=np.int32)
    states = np.zeros((B, n, hs), dtype=np.float32)
    edges = []
    for b, g in enumerate(G):
        nv[b] = g.vcount()
        types[b, :nv[b]] = g.vs["type"]
        for u, v in g.get_edgelist():
            preds[b, v] |= 1 << u
        edges.append(g.get_edgelist())
        top = g.vs.deleted["H_forward%d" % (L - 1)]
        for v in range(nv[b]):
            states[b, v] = top[v].numpy()[0]
    loose = [bin(int(preds[b, nv[b] - 1])).count("1") for b in range(B)]
    meta = dict(kind=kind, hs=hs, L=L, B=B, n=n, w_seed=ws, z_seed=seed, stochastic=stochastic, bidir=kind == "bn",
                margin=margin, edge_order=[[list(e) for e in es] for es in edges],
                coverage=dict(early_end=int((nv < n).sum()), forced_end=int((nv == n).sum()),
                              end_joins_two=int(sum(x >= 2 for x in loose)), coupled_updates=int(sum(coupled))))
    print(name, meta["coverage"], "margin %.2e" % margin)
    _save(name, meta, z=z.numpy(), u_type=u_type[None], u_edge=u_edge[None], types=types, preds=preds, nv=nv,
          states=states, widths=np.array(widths, dtype=np.int64))


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not found at %s - fixtures can only be regenerated in the build container" % REF)
    _setup_paths()
    sys.path.insert(0, os.path.join(HERE, "decode_standin"))   # ahead of oracle/pyg_standin's igraph
    torch.manual_seed(0)
    ref_na = importlib.import_module("dagnn")
    ref_bn = importlib.import_module("dagnn_bn")
    for st in (False, True):
        tag = "sample" if st else "argmax"
        make_decode(ref_na, "DAGNN", "dvae_decode_na_h64_L2_" + tag, kind="na", hs=64, L=2, B=16, w_seed=241, z_seed=51,
                    stochastic=st)
        make_decode(ref_bn, "DAGNN_BN", "dvae_decode_bn_h32_L3_" + tag, kind="bn", hs=32, L=3, B=12, w_seed=242, z_seed=52,
                    stochastic=st)
    make_decode(ref_na, "DAGNN", "dvae_decode_na_h501_L2_sample", kind="na", hs=501, L=2, B=32, w_seed=243, z_seed=53,
                stochastic=True)
    make_decode(ref_bn, "DAGNN_BN", "dvae_decode_bn_h501_L2_sample", kind="bn", hs=501, L=2, B=32, w_seed=244, z_seed=54,
                stochastic=True)


if __name__ == "__main__":
    main()
