#!/usr/bin/env python
"""Generate the fixture of the graph store (`code2_store_small.npz`) from the REAL reference.

Runs only where the reference is present.  Same pattern as `make_golden_code2_lp.py`: the reference's files are imported
unmodified (`ogbg-code/utils2.py`, `src/utils_dag.py`), only data goes into this directory.

    python tests/golden/make_golden_code2_store.py

Eight small RAW graphs (AST edges only, `node_is_attributed`, `y_arr`) and what the reference's loader side makes of them:
`augment_edge2` (utils2.py:31-79) and `add_order_info_01` (src/utils_dag.py:39-52) per graph, `len_longest_path` as the
reference's reader stores it (ogb/io/read_graph_pyg.py:51-54), then the PyG collation - for two index lists: the identity, and
a permuted list with a repeat.  The graphs: one node without / with the attributed flag, exactly one attributed node, a chain,
three `synth.gen_ast` trees (their next-token edges removed, the leaves attributed), and - last - a graph without AST edge.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _load_file, _np, _save, _setup_paths  # noqa: E402
from dagnn_amd import synth  # noqa: E402
from dagnn_amd.data import GraphBatch, GraphData  # noqa: E402

S = 3
BATCH_KEYS = ("x", "node_depth", "edge_index", "edge_attr", "batch", "ptr", "_bi_layer_idx0", "_bi_layer_idx1",
              "_bi_layer_index0", "_bi_layer_index1", "y_arr")
LISTS = {"identity": [0, 1, 2, 3, 4, 5, 6, 7], "permuted": [7, 5, 0, 5, 2, 6, 1, 3, 4]}


def raw_graphs():
    rng = np.random.default_rng(173)
    out = []

    def add(n, edges, attributed, depth=None):
        out.append(dict(x=np.stack([rng.integers(0, 98, n), rng.integers(0, 10030, n)], 1).astype(np.int64),
                        node_depth=(np.arange(n) if depth is None else np.asarray(depth)).astype(np.int64).reshape(n, 1),
                        edge_index=np.asarray(edges, dtype=np.int64).reshape(2, -1),
                        node_is_attributed=np.asarray(attributed, dtype=np.int64).reshape(n, 1),
                        y_arr=rng.integers(0, 50, size=(1, S)).astype(np.int64)))

    add(1, [[], []], [0])                                           # one node, not attributed
    add(1, [[], []], [1])                                           # one node, attributed: still no next-token edge
    add(3, [[0, 0], [1, 2]], [0, 0, 1], depth=[0, 1, 1])            # exactly one attributed node
    add(6, [[0, 1, 2, 3, 4], [1, 2, 3, 4, 5]], [0, 1, 0, 1, 0, 1])  # a chain; next-token edges skip along it
    for n in (11, 23, 40):
        g = synth.gen_ast(rng, n)
        ast = g["ei"][:, g["ea"][:, 0] == 0]
        leaf = np.zeros(n, dtype=np.int64)
        leaf[np.setdiff1d(np.arange(n), ast[0])] = 1
        add(n, ast, leaf, depth=g["depth"])
    add(4, [[], []], [1, 0, 1, 1], depth=[0, 0, 0, 0])              # no AST edge (placed last): next-token edges only
    return out


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not found at %s - fixtures can only be regenerated where it is present" % REF)
    _setup_paths()
    import importlib
    ref_dagutils = importlib.import_module("src.utils_dag")
    ref_utils2 = _load_file("ref_ogbg_utils2", os.path.join(REF, "ogbg-code", "utils2.py"))
    raw = raw_graphs()
    arrays = {}
    prepared = []
    for i, r in enumerate(raw):
        for k, v in r.items():
            arrays["raw%d::%s" % (i, k)] = v
        d = GraphData(**{k: torch.from_numpy(v.copy()) for k, v in r.items()})
        d = ref_utils2.augment_edge2(d)
        ref_dagutils.add_order_info_01(d)
        d._bi_layer_index1 = d._bi_layer_index1.clone()
        d.llp = float(torch.max(d._bi_layer_idx0).item())   # ogb/io/read_graph_pyg.py:54
        prepared.append(d)
    for name, ids in LISTS.items():
        graphs = []
        for i in ids:
            g = prepared[i].clone()
            del g.__dict__["llp"]
            graphs.append(g)
        b = GraphBatch.from_data_list(graphs)
        arrays[name + "::idx"] = np.asarray(ids, dtype=np.int64)
        for k in BATCH_KEYS:
            arrays[name + "::" + k] = _np(b[k])
        arrays[name + "::len_longest_path"] = _np(torch.tensor([prepared[i].llp for i in ids]))
        print("%-9s B %d  N %d  E %d" % (name, len(ids), b.x.shape[0], b.edge_index.shape[1]))
    _save("code2_store_small", dict(kind="code2_store", graphs=len(raw), S=S, lists=sorted(LISTS), batch_keys=list(BATCH_KEYS)),
          **arrays)


if __name__ == "__main__":
    main()
