"""Host side of the sampling D-VAE decoder (`decode()`, csrc/dvae_sample.hip): argument checks of the C entry point, the
draw layout, the host graphs built from dense results, and the coverage of the `dvae_decode_*` fixtures - none of it
needs a GPU."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from dagnn_amd import _lib, dvae
from tests import helpers as Hh

FIXTURES = ["dvae_decode_na_h64_L2_argmax", "dvae_decode_bn_h32_L3_argmax", "dvae_decode_na_h64_L2_sample",
            "dvae_decode_bn_h32_L3_sample", "dvae_decode_na_h501_L2_sample", "dvae_decode_bn_h501_L2_sample"]


def _args(**kw):
    a = _lib.DvaeSampleArgs()
    a.G, a.B, a.n, a.hs, a.L, a.nvt, a.start_type, a.end_type = 2, 4, 8, 16, 2, 8, 0, 1
    a.bn, a.stochastic, a.edge_hidden, a.vertex_hidden = 0, 1, 64, 32
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_sample_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    good = _args()
    assert lib.dagnn_dvae_sample_work_bytes(C.byref(good)) > 0
    assert lib.dagnn_dvae_sample_work_bytes(C.byref(_args(bn=1, stochastic=0))) > 0
    bad = [dict(G=0), dict(B=0), dict(n=1), dict(n=33), dict(hs=0), dict(L=0), dict(L=9), dict(nvt=0), dict(nvt=65),
           dict(start_type=8), dict(end_type=-1), dict(end_type=8), dict(bn=2), dict(stochastic=2), dict(edge_hidden=0),
           dict(vertex_hidden=-1), dict(G=1 << 20, B=1 << 20)]
    for kw in bad:
        a = _args(**kw)
        assert lib.dagnn_dvae_sample_work_bytes(C.byref(a)) == 0, kw
        assert lib.dagnn_dvae_sample(C.byref(a), None) == -22, kw
    # a well-shaped struct with null pointers is refused before any HIP call
    assert lib.dagnn_dvae_sample(C.byref(good), None) == -22
    assert lib.dagnn_dvae_sample(None, None) == -22
    assert lib.dagnn_dvae_sample_work_bytes(None) == 0


def test_edge_draws_follow_the_reference_call_order():
    n = 10
    order = [(idx, vi) for idx in range(1, n) for vi in range(idx - 1, -1, -1)]
    assert [dvae.edge_draw_index(idx, vi) for idx, vi in order] == list(range(n * (n - 1) // 2))
    assert dvae.draw_shapes(n, 32, 5) == ((5, n, 32), (5, n * (n - 1) // 2, 32))
    with pytest.raises(ValueError):
        dvae.edge_draw_index(3, 3)


def _random_dense(rng, B, n, end_type=1):
    """Random decoded graphs in dense form: types, predecessor bitmasks, vertex counts."""
    types = np.full((B, n), -1, np.int32)
    preds = np.zeros((B, n), np.int64)
    nv = rng.integers(2, n + 1, size=B).astype(np.int32)
    for b in range(B):
        types[b, 0] = 0
        types[b, 1:nv[b]] = rng.integers(2, 8, size=nv[b] - 1)
        types[b, nv[b] - 1] = end_type
        for v in range(1, nv[b]):
            preds[b, v] = int(rng.integers(1, 1 << v))
    return types, preds, nv


def test_decoded_graph_agrees_with_brute_force():
    rng = np.random.default_rng(3)
    types, preds, nv = _random_dense(rng, 40, 9)
    graphs = dvae.graphs_from_dense(types, preds, nv, 1, use_igraph=False)
    for b, g in enumerate(graphs):
        k = int(nv[b])
        edges = {(u, v) for v in range(k) for u in range(k) if preds[b, v] >> u & 1}
        assert isinstance(g, dvae.DecodedGraph)
        assert g.vcount() == k and g.ecount() == len(edges) and set(g.get_edgelist()) == edges
        assert g.vs["type"] == list(types[b, :k]) and all(g.vs[v]["type"] == types[b, v] for v in range(k))
        for v in range(k):
            assert g.predecessors(v) == sorted(u for u, w in edges if w == v)
            assert g.successors(v) == sorted(w for u, w in edges if u == v)
        assert g.indegree() == [len(g.predecessors(v)) for v in range(k)]
        assert g.outdegree() == [len(g.successors(v)) for v in range(k)]
        assert g.indegree(k - 1) == len(g.predecessors(k - 1))
        assert g.is_dag()
        # the reference's insertion order: per vertex its predecessors descending, the END vertex's ascending
        order = dvae.decoded_edges(types[b], preds[b], k, 1)
        want = []
        for v in range(1, k):
            us = sorted(u for u, w in edges if w == v)
            want += [(u, v) for u in (list(set(us)) if types[b, v] == 1 else us[::-1])]
        assert order == want == g.get_edgelist()
    cyc = dvae.DecodedGraph([0, 2, 1], [(0, 1), (1, 2), (2, 1)])
    assert not cyc.is_dag()


def test_fixture_edge_order_is_the_insertion_order_of_the_reference():
    for name in FIXTURES:
        meta, arr = Hh.load(name)
        for b in range(meta["B"]):
            got = dvae.decoded_edges(arr["types"][b], arr["preds"][b], arr["nv"][b], 1)
            assert [list(e) for e in got] == meta["edge_order"][b], (name, b)


def test_fixtures_cover_the_decoder_cases():
    """Early END, END forced at max_n-1, an END joining two or more loose ends, an update whose P comes from another
    graph - across the set; every fixture's decisions lie at least 1e-4 from flipping."""
    cov = dict(early_end=0, forced_end=0, end_joins_two=0, coupled_updates=0)
    for name in FIXTURES:
        meta, arr = Hh.load(name)
        assert meta["margin"] >= 1e-4, name
        for k in cov:
            cov[k] += meta["coverage"][k]
        assert len(arr["widths"]) == (36 if meta["n"] == 8 else 55)
    assert all(v > 0 for v in cov.values()), cov


def test_decode_raises_off_the_gpu_and_for_bad_arguments():
    meta, arr = Hh.load("dvae_decode_na_h64_L2_argmax")
    model, _ = Hh.dvae_model(meta)
    z = torch.from_numpy(arr["z"].copy())
    with pytest.raises(_lib.DagnnHipError, match="GPU"):
        model.decode(z)
    with pytest.raises(ValueError, match="nz"):
        model.decode(z[:, :10])
    with pytest.raises(ValueError, match="nz"):
        model.decode(z[0])
    model_add, _ = Hh.dvae_model(dict(meta, agg="add"))
    with pytest.raises(NotImplementedError, match="attn_h"):
        model_add.decode(z)
    big, _ = Hh.dvae_model(meta)
    big.max_n = 33
    with pytest.raises(ValueError, match="32"):
        big.decode_dense(z)
