#!/usr/bin/env python
"""Generate the fixture of the D-VAE store (`dvae_store_small.npz`) from the REAL reference.

Runs only where the reference is present.  Same pattern as `make_golden_code2_store.py`: the reference's files are imported
unmodified (`dvae/util.py`, `dvae/batch.py`), only data goes into this directory.

    python tests/golden/make_golden_dvae_store.py

Six ENAS rows (8 vertices) and six BN rows (10 vertices) in the format of the reference's data files, and what the
reference makes of them: per row the graph of `decode_ENAS_to_pygraph` / `decode_BN_to_pygraph` (dvae/util.py:290-385) - `x`,
`edge_index`, `bi_layer_index`, the `vs` types - and, for two index lists (the identity, and a permutation with a repeat),
`Batch.from_data_list` of dvae/batch.py over deep copies of the graphs, as `_collate_fn` makes them (that collation shifts
`bi_layer_index` in place).  ENAS row 0 has no skip connection (7 edges, fewer than vertices), row 1 every one (7 + 15 = 22 edges, the most
a row can say: the end vertex only ever follows the last layer); in
BN row 0 every vertex is parentless (all hang off the start vertex and feed the end vertex), row 1 is a pure chain.
"""
from __future__ import annotations

import copy
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _np, _save, _setup_paths  # noqa: E402
from dagnn_amd import synth  # noqa: E402

GRAPH_KEYS = ("x", "edge_index", "bi_layer_index")
BATCH_KEYS = ("x", "edge_index", "bi_layer_index", "batch")
LISTS = {"identity": [0, 1, 2, 3, 4, 5], "permuted": [5, 2, 0, 2, 4, 1, 3]}


def enas_rows():
    bare = [[t] + [0] * i for i, t in enumerate([3, 0, 5, 1, 4, 2])]
    full = [[t] + [1] * i for i, t in enumerate([0, 0, 1, 5, 2, 2])]
    return [bare, full] + synth.enas_rows(811, 4)


def bn_rows():
    orphans = [[t] + [0] * i for i, t in enumerate([7, 2, 0, 5, 1, 3, 6, 4])]
    chain = [[t] + [int(j == i - 1) for j in range(i)] for i, t in enumerate([1, 0, 3, 2, 5, 4, 7, 6])]
    return [orphans, chain] + synth.bn_rows(812, 4)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not found at %s - fixtures can only be regenerated where it is present" % REF)
    _setup_paths()
    ref_util = importlib.import_module("util")
    ref_batch = importlib.import_module("batch")
    arrays, meta = {}, dict(kind="dvae_store", lists=sorted(LISTS), graph_keys=list(GRAPH_KEYS), batch_keys=list(BATCH_KEYS), sets={})
    for name, rows, decode, n_types in (("enas", enas_rows(), ref_util.decode_ENAS_to_pygraph, 6),
                                        ("bn", bn_rows(), ref_util.decode_BN_to_pygraph, 8)):
        graphs = []
        for i, row in enumerate(rows):
            g, nvt = decode(row, n_types)
            graphs.append(g)
            for k in GRAPH_KEYS:
                arrays["%s::g%d::%s" % (name, i, k)] = _np(g[k])
            arrays["%s::g%d::types" % (name, i)] = np.array([v["type"] for v in g.vs], dtype=np.int64)
        arrays[name + "::rows"] = np.array([json.dumps(r) for r in rows])
        meta["sets"][name] = dict(graphs=len(rows), n=int(graphs[0].x.shape[0]), nvt=int(nvt),
                                  edges=[int(g.edge_index.shape[1]) for g in graphs])
        for lname, ids in LISTS.items():
            b = ref_batch.Batch.from_data_list([copy.deepcopy(graphs[i]) for i in ids])   # models_pyg.py:114-115
            arrays["%s::%s::idx" % (name, lname)] = np.asarray(ids, dtype=np.int64)
            for k in BATCH_KEYS:
                arrays["%s::%s::%s" % (name, lname, k)] = _np(b[k])
            arrays["%s::%s::vs" % (name, lname)] = np.array([[v["type"] for v in vs] for vs in b.vs], dtype=np.int64)
            print("%-5s %-9s B %d  N %d  E %d" % (name, lname, len(ids), b.x.shape[0], b.edge_index.shape[1]))
    _save("dvae_store_small", meta, **arrays)


if __name__ == "__main__":
    main()
