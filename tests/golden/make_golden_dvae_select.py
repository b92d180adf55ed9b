#!/usr/bin/env python
"""Generate the `dvae_select_*` fixtures from the REAL reference's `decode_from_latent_space` (dvae/util.py:408-466).

Runs only in the build container (needs the reference).  dvae/util.py runs unmodified: argv is cleared (it parses
arguments at import), networkx is stubbed (util.py imports it, the functions used here do not touch it), and its igraph
is the stand-in of tests/golden/decode_standin with what util.py's checks and string forms call patched on at run time
(`igraph.IN / OUT`, `vertex.indegree() / outdegree()`, `are_connected`, `get_adjlist`, `get_adjacency`, `neighbors`,
`indegree`, `is_dag`).  A stub model's `decode()` returns prepared decoder-shaped graphs, attempt by attempt: the
rows of `dagnn_amd.synth.decoded_rows(seed, ...)`, which cover a middle START vertex, a middle vertex without
predecessors, a missing chain edge with END of in-degree 2, early END, duplicate BN types, BN graphs equal up to vertex
order, points without a valid attempt and points whose first valid string is not the most frequent one.

Each fixture stores the dense rows (small fixtures) or only their seed (A = 500: the tests regenerate them), and per
run (n_nodes variable / fixed): `is_valid_*` per attempt, the reference's returned strings and which decoded graph
(point, attempt) `return_igraph` returned, per point the valid count and the count of the returned string, and the
`Counter.most_common(1)` pick over the same valid strings.  Small fixtures also keep `decode_igraph_to_*` of every
attempt.

    python tests/golden/make_golden_dvae_select.py
"""
from __future__ import annotations

import collections
import importlib
import os
import sys
import types as pytypes

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _save, _setup_paths  # noqa: E402
from dagnn_amd import synth  # noqa: E402


def _patch_igraph():
    """The decode stand-in plus what dvae/util.py's validity checks and string forms read of a graph."""
    sys.path.insert(0, os.path.join(HERE, "decode_standin"))
    sys.modules.pop("igraph", None)
    ig = importlib.import_module("igraph")
    ig.OUT, ig.IN, ig.ALL = 1, 2, 3
    G = ig.Graph

    class _V(dict):
        def __init__(self, graph, index, attrs):
            dict.__init__(self, attrs)
            self._graph, self.index = graph, index

        def indegree(self):
            return len(self._graph.predecessors(self.index))

        def outdegree(self):
            return len(self._graph.successors(self.index))

    def add_vertex(self, **attrs):
        self.vs.append(_V(self, len(self.vs), attrs))

    def neighbors(self, v, mode="all"):
        mode = {"out": 1, "in": 2, "all": 3}.get(mode, mode)
        return sorted((self.predecessors(v) if mode != 1 else []) + (self.successors(v) if mode != 2 else []))

    def is_dag(self):
        indeg = [len(self.predecessors(v)) for v in range(self.vcount())]
        ready, seen = [v for v in range(self.vcount()) if indeg[v] == 0], 0
        while ready:
            u = ready.pop()
            seen += 1
            for w in self.successors(u):
                indeg[w] -= 1
                if indeg[w] == 0:
                    ready.append(w)
        return seen == self.vcount()

    def get_adjacency(self):
        data = [[0] * self.vcount() for _ in range(self.vcount())]
        for u, v in self._edges:
            data[u][v] += 1
        return pytypes.SimpleNamespace(data=data)

    G.add_vertex = add_vertex
    G.are_connected = lambda self, u, v: (u, v) in self._edges
    G.get_adjlist = lambda self, mode=1: [neighbors(self, v, mode) for v in range(self.vcount())]
    G.get_adjacency = get_adjacency
    G.neighbors = neighbors
    G.is_dag = is_dag
    G.indegree = lambda self, v=None: [len(self.predecessors(x)) for x in range(self.vcount())] if v is None else \
        len(self.predecessors(v))
    return ig


class _StubModel:
    """`model.decode(z)` returns attempt a's B prepared graphs on its a-th call."""

    def __init__(self, ig, types, preds, nv, nvt):
        self.START_TYPE, self.END_TYPE, self.nvt = 0, 1, nvt
        self.origin = {}
        self.graphs = []
        A, B, _ = types.shape
        for a in range(A):
            row = []
            for b in range(B):
                g = ig.Graph(directed=True)
                k = int(nv[a, b])
                for v in range(k):
                    g.add_vertex(type=int(types[a, b, v]))
                for v in range(1, k):
                    m = int(preds[a, b, v]) & 0xFFFFFFFF
                    for u in range(v - 1, -1, -1):
                        if m >> u & 1:
                            g.add_edge(u, v)
                self.origin[id(g)] = (b, a)
                row.append(g)
            self.graphs.append(row)
        self.calls = 0

    def decode(self, z):
        g = self.graphs[self.calls]
        self.calls += 1
        return g


def make_select(util, ig, name, *, kind, A, B, seed, store_rows):
    n = nvt = 8 if kind == "ENAS" else 10
    types, preds, nv = synth.decoded_rows(seed, kind, A, B, n, nvt)
    valid_fn = (lambda g: util.is_valid_ENAS(g, 0, 1)) if kind == "ENAS" else (lambda g: util.is_valid_BN(g, 0, 1, nvt=nvt))
    form = util.decode_igraph_to_ENAS if kind == "ENAS" else util.decode_igraph_to_BN_adj
    runs = []
    strings_all = None
    for n_nodes in (["variable", n] if kind == "ENAS" else ["variable"]):
        model = _StubModel(ig, types, preds, nv, nvt)
        z = torch.zeros(B, 4)
        graphs, final = util.decode_from_latent_space(z, model, A, n_nodes, True, kind)
        assert model.calls == A
        valid = np.zeros((A, B), dtype=bool)
        strings = [[form(model.graphs[a][b]) for b in range(B)] for a in range(A)]
        for a in range(A):
            for b in range(B):
                g = model.graphs[a][b]
                valid[a, b] = valid_fn(g) and (n_nodes == "variable" or g.vcount() == n_nodes)
        strings_all = strings
        first, n_same, mode, mode_same, n_valid = [], [], [], [], []
        for b in range(B):
            cur = [(a, strings[a][b]) for a in range(A) if valid[a, b]]
            n_valid.append(len(cur))
            if not cur:
                assert final[b] is None and graphs[b] is None
                first.append(-1), n_same.append(0), mode.append(-1), mode_same.append(0)
                continue
            counts = collections.Counter(s for _, s in cur)
            assert final[b] == cur[0][1], (name, b)   # the reference returns the first valid string
            first.append(cur[0][0])
            n_same.append(counts[cur[0][1]])
            best, cnt = counts.most_common(1)[0]
            mode.append(next(a for a, s in cur if s == best))
            mode_same.append(cnt)
        source = [None if g is None else list(model.origin[id(g)]) for g in graphs]
        runs.append(dict(n_nodes=n_nodes, strings=final, source=source, pick=first, n_same=n_same, n_valid=n_valid,
                         mode_pick=mode, mode_same=mode_same))
        runs[-1]["_valid"] = valid
    cov = dict(points_without_valid=sum(p < 0 for p in runs[0]["pick"]),
               first_is_not_mode=sum(int(p != m) for p, m in zip(runs[0]["pick"], runs[0]["mode_pick"])),
               source_elsewhere=sum(int(s is not None and (s[1] != p or s[0] != b))
                                    for b, (s, p) in enumerate(zip(runs[0]["source"], runs[0]["pick"]))))
    meta = dict(kind=kind, A=A, B=B, n=n, nvt=nvt, start_type=0, end_type=1, seed=seed, rows_stored=store_rows,
                runs=[{k: v for k, v in r.items() if k != "_valid"} for r in runs], coverage=cov)
    arrays = {"valid%d" % i: np.packbits(r["_valid"]) for i, r in enumerate(runs)}
    if store_rows:
        meta["attempt_strings"] = strings_all
        arrays.update(types=types, preds=preds, nv=nv)
    print(name, cov, "valid %.2f" % runs[0]["_valid"].mean())
    _save(name, meta, **arrays)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not found at %s - fixtures can only be regenerated in the build container" % REF)
    _setup_paths()
    os.environ.setdefault("TQDM_DISABLE", "1")
    sys.modules["networkx"] = pytypes.ModuleType("networkx")   # imported by util.py, unused by what runs here
    ig = _patch_igraph()
    util = importlib.import_module("util")
    assert util.igraph is ig
    make_select(util, ig, "dvae_select_enas_a12", kind="ENAS", A=12, B=16, seed=301, store_rows=True)
    make_select(util, ig, "dvae_select_bn_a12", kind="BN", A=12, B=16, seed=302, store_rows=True)
    make_select(util, ig, "dvae_select_enas_a64", kind="ENAS", A=64, B=8, seed=303, store_rows=True)
    make_select(util, ig, "dvae_select_enas_a500", kind="ENAS", A=500, B=50, seed=304, store_rows=False)
    make_select(util, ig, "dvae_select_bn_a500", kind="BN", A=500, B=50, seed=305, store_rows=False)


if __name__ == "__main__":
    main()
