#!/usr/bin/env python
"""Generate the `dvae_match_*` fixtures from the REAL reference's evaluation primitives (dvae/util.py): `is_same_DAG`
(:576-585), `ratio_same_DAG` (:588-596), `is_valid_ENAS` / `is_valid_BN` (:621-649) and the string forms
`decode_igraph_to_ENAS` / `decode_igraph_to_BN_adj`.

Runs only in the build container (needs the reference).  dvae/util.py runs unmodified, set up as in
make_golden_dvae_select.py (argv cleared, networkx stubbed, the igraph stand-in patched by its `_patch_igraph`);
`ratio_same_DAG` iterates through tqdm; the name `tqdm` in the imported module is rebound to the identity at run time
(TQDM_DISABLE alone does not silence every tqdm version).  The rows are `dagnn_amd.synth.match_rows(seed, ...)`:
decodes equal to their true graph, equal but for one type, one edge bit or the vertex count, BN graphs equal up to
vertex order, training sets with duplicates and with invalid decoded rows, a point without a valid attempt, and (the
`*_none` fixtures) no valid decode at all.

Each fixture stores the seed and shape (the tests regenerate the rows; the small ones keep the rows too) and the
reference's results: `is_same_DAG` of every decode against its true graph, validity per decode, per valid decode
whether `ratio_same_DAG`'s inner loop finds it in the training set, the ratio itself, and len(set(strings)).

    python tests/golden/make_golden_dvae_match.py
"""
from __future__ import annotations

import importlib
import os
import sys
import types as pytypes

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _save, _setup_paths  # noqa: E402
from make_golden_dvae_select import _patch_igraph  # noqa: E402
from dagnn_amd import synth  # noqa: E402


def _graph(ig, types, preds, nv):
    g = ig.Graph(directed=True)
    k = int(nv)
    for v in range(k):
        g.add_vertex(type=int(types[v]))
    for v in range(1, k):
        m = int(preds[v]) & 0xFFFFFFFF
        for u in range(v - 1, -1, -1):
            if m >> u & 1:
                g.add_edge(u, v)
    return g


def make_match(util, ig, name, *, kind, A, B, seed, n_train, store_rows, n=None, nvt=None, all_invalid=False):
    n = n or (8 if kind == "ENAS" else 10)
    nvt = nvt or n
    r = synth.match_rows(seed, kind, A, B, n, nvt, n_train, all_invalid=all_invalid)
    dec = [[_graph(ig, r["types"][a, b], r["preds"][a, b], r["nv"][a, b]) for b in range(B)] for a in range(A)]
    true = [_graph(ig, r["types_true"][b], r["preds_true"][b], r["nv_true"][b]) for b in range(B)]
    train = [_graph(ig, r["types_train"][i], r["preds_train"][i], r["nv_train"][i]) for i in range(n_train)]
    valid_fn = (lambda g: util.is_valid_ENAS(g, 0, 1)) if kind == "ENAS" else (lambda g: util.is_valid_BN(g, 0, 1, nvt=nvt))
    form = util.decode_igraph_to_ENAS if kind == "ENAS" else util.decode_igraph_to_BN_adj
    same = np.array([[bool(util.is_same_DAG(true[b], dec[a][b])) for b in range(B)] for a in range(A)])
    valid = np.array([[bool(valid_fn(dec[a][b])) for b in range(B)] for a in range(A)])
    G_valid = [dec[a][b] for a in range(A) for b in range(B) if valid[a, b]]   # attempt-major, as the script decodes
    in_train = np.zeros((A, B), dtype=bool)
    for a in range(A):
        for b in range(B):
            in_train[a, b] = any(util.is_same_DAG(dec[a][b], g0) for g0 in train)   # every decode, valid or not
    ratio = util.ratio_same_DAG(train, G_valid) if G_valid else None
    n_in = int((in_train & valid).sum())
    assert ratio is None or abs(ratio - n_in / len(G_valid)) < 1e-12
    strings = [form(g) for g in G_valid]
    # whole-call uniqueness differs from the per-point one whenever two points share a string
    per_point = sum(len({form(dec[a][b]) for a in range(A) if valid[a, b]}) for b in range(B))
    cov = dict(n_same=int(same.sum()), n_valid=len(G_valid), n_unique=len(set(strings)), n_unique_per_point_sum=per_point,
               n_in_train=n_in, in_train_invalid=int((in_train & ~valid).sum()),
               points_without_valid=int((valid.sum(0) == 0).sum()),
               train_distinct=len({(int(k),) + tuple(map(int, t[:k])) + tuple(int(p) & ((1 << v) - 1) for v, p in enumerate(p_[:k].view(np.uint32)))
                                   for t, p_, k in zip(r["types_train"], r["preds_train"], r["nv_train"])}))
    meta = dict(kind=kind, A=A, B=B, n=n, nvt=nvt, seed=seed, n_train=n_train, all_invalid=all_invalid, rows_stored=store_rows,
                ratio_same_DAG=ratio, per_graph=same.sum(0).astype(int).tolist(), **cov)
    arrays = dict(same=np.packbits(same), valid=np.packbits(valid), in_train=np.packbits(in_train))
    if store_rows:
        arrays.update(r)
    print(name, cov)
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
    util.tqdm = lambda it, *a, **k: it   # progress bars off; the loop itself is the reference's
    make_match(util, ig, "dvae_match_enas_a12", kind="ENAS", A=12, B=16, seed=401, n_train=60, store_rows=True)
    make_match(util, ig, "dvae_match_bn_a12", kind="BN", A=12, B=16, seed=402, n_train=60, store_rows=True)
    make_match(util, ig, "dvae_match_enas_a40", kind="ENAS", A=40, B=60, seed=403, n_train=300, store_rows=False)
    make_match(util, ig, "dvae_match_bn_a40", kind="BN", A=40, B=60, seed=404, n_train=300, store_rows=False)
    make_match(util, ig, "dvae_match_enas_none", kind="ENAS", A=6, B=8, seed=405, n_train=40, store_rows=False,
               all_invalid=True)
    make_match(util, ig, "dvae_match_bn_none", kind="BN", A=6, B=8, seed=406, n_train=40, store_rows=False, all_invalid=True)


if __name__ == "__main__":
    main()
