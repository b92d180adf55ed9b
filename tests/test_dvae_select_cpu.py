"""Host side of `decode_from_latent_space` (csrc/dvae_select.hip): the host mirror of the validity rules, the string
forms and the selection against the `dvae_select_*` fixtures of the reference's own dvae/util.py, the completed
`DecodedGraph` surface, the C struct and the argument checks of the entry point - none of it needs a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from dagnn_amd import _lib, dvae, synth
from tests import helpers as Hh

FIXTURES = ["dvae_select_enas_a12", "dvae_select_bn_a12", "dvae_select_enas_a64", "dvae_select_enas_a500",
            "dvae_select_bn_a500"]


def fixture_rows(name):
    """(meta, types, preds, nv, valid per run) of a fixture; rows of the big ones come back from their seed."""
    meta, arr = Hh.load(name)
    if meta["rows_stored"]:
        types, preds, nv = arr["types"], arr["preds"], arr["nv"]
    else:
        types, preds, nv = synth.decoded_rows(meta["seed"], meta["kind"], meta["A"], meta["B"], meta["n"], meta["nvt"])
    A, B = meta["A"], meta["B"]
    valid = [np.unpackbits(arr["valid%d" % i])[:A * B].reshape(A, B).astype(bool) for i in range(len(meta["runs"]))]
    return meta, types, preds, nv, valid


def _n_nodes(run):
    return None if run["n_nodes"] == "variable" else run["n_nodes"]


@pytest.mark.parametrize("name", FIXTURES)
def test_host_mirror_reproduces_the_reference(name):
    meta, types, preds, nv, valid = fixture_rows(name)
    kind, nvt = meta["kind"], meta["nvt"]
    form = dvae.enas_string if kind == "ENAS" else dvae.bn_adj_string
    if meta["rows_stored"]:
        for a in range(meta["A"]):
            for b in range(meta["B"]):
                assert form(types[a, b], preds[a, b], nv[a, b]) == meta["attempt_strings"][a][b], (name, a, b)
    for run, want_valid in zip(meta["runs"], valid):
        for select, pick, same in (("first", "pick", "n_same"), ("most_common", "mode_pick", "mode_same")):
            got_valid, got_pick, n_valid, n_same, strings = dvae.select_host(types, preds, nv, kind, nvt, 0, 1,
                                                                            _n_nodes(run), select)
            np.testing.assert_array_equal(got_valid, want_valid)
            assert got_pick.tolist() == run[pick] and n_same.tolist() == run[same], (name, select)
            assert n_valid.tolist() == run["n_valid"]
        for b, s in enumerate(run["strings"]):
            p = run["pick"][b]
            assert (None if p < 0 else form(types[p, b], preds[p, b], nv[p, b])) == s


@pytest.mark.parametrize("name", FIXTURES)
def test_decode_from_latent_space_matches_the_reference_on_host_rows(name):
    """The whole function, strings, Nones and return_igraph's graphs included, on a stand-in model that serves the
    fixture's rows as host tensors (select_dense then runs the host mirror)."""
    meta, types, preds, nv, _ = fixture_rows(name)
    A, B, n = meta["A"], meta["B"], meta["n"]

    class Rows(object):
        max_n, nvt, START_TYPE, END_TYPE = n, meta["nvt"], 0, 1

        def __init__(self):
            self.at = 0

        def decode_dense(self, z, stochastic, attempts, draws):
            assert stochastic and tuple(draws[0].shape) == (attempts, n, B)
            sl = slice(self.at, self.at + attempts)
            self.at += attempts
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x[sl]))  # noqa: E731
            return dvae.DecodedDense(t(types), t(preds), t(nv), None)

        def select_dense(self, d, data_type, n_nodes, select):
            return dvae.select_decoded(d, data_type, self.nvt, 0, 1, n_nodes, select)

    for run in meta["runs"]:
        graphs, strings = dvae.decode_from_latent_space(torch.zeros(B, 4), Rows(), A, run["n_nodes"], True, meta["kind"],
                                                        chunk=7)
        assert strings == run["strings"]
        for b, (g, src) in enumerate(zip(graphs, run["source"])):
            if src is None:
                assert g is None
                continue
            sb, sa = src
            want = dvae.graphs_from_dense(types[sa, sb][None], preds[sa, sb][None], nv[sa, sb][None], 1, use_igraph=False)[0]
            assert g.vs["type"] == want.vs["type"] and g.get_edgelist() == want.get_edgelist(), (name, b)
        assert dvae.decode_from_latent_space(torch.zeros(B, 4), Rows(), A, run["n_nodes"], False, meta["kind"]) == strings


def test_keys_are_equal_exactly_when_strings_are():
    for name in FIXTURES:
        meta, types, preds, nv, valid = fixture_rows(name)
        kind, n, nvt = meta["kind"], meta["n"], meta["nvt"]
        form = dvae.enas_string if kind == "ENAS" else dvae.bn_adj_string
        seen = {}
        for a, b in zip(*np.nonzero(valid[0])):
            key = tuple(dvae.select_key(types[a, b], preds[a, b], nv[a, b], kind, n, nvt))
            s = form(types[a, b], preds[a, b], nv[a, b])
            assert seen.setdefault(key, s) == s, name
        assert len(set(seen.values())) == len(seen)
        assert len(key) == dvae.select_key_words(kind, n, nvt) == 1
    assert dvae.select_key_words("ENAS", 32, 64) == 10 and dvae.select_key_words("BN", 32, 32) == 15


def test_decoded_graph_runs_the_reference_utilities_surface():
    rng = np.random.default_rng(7)
    types, preds, nv = synth.decoded_rows(11, "BN", 6, 5, 10, 10)
    for a in range(6):
        gs = dvae.graphs_from_dense(types[a], preds[a], nv[a], 1, use_igraph=False)
        for b, g in enumerate(gs):
            k = int(nv[a, b])
            edges = set(g.get_edgelist())
            verts = list(g.vs)
            assert [v.index for v in verts] == list(range(k)) and [v["type"] for v in verts] == g.vs["type"]
            assert g.vs[k - 1] == {"type": int(types[a, b, k - 1])} and g.vs[-1].index == k - 1
            for v in verts:
                assert v.indegree() == len([e for e in edges if e[1] == v.index])
                assert v.outdegree() == len([e for e in edges if e[0] == v.index])
            for u in range(k):
                for w in range(k):
                    assert g.are_connected(u, w) == ((u, w) in edges)
            adj = g.get_adjacency().data
            assert adj == [[int((u, w) in edges) for w in range(k)] for u in range(k)]
            assert g.get_adjlist(dvae.IGRAPH_IN) == g.get_adjlist("in") == [g.predecessors(v) for v in range(k)]
            assert g.get_adjlist() == g.get_adjlist(dvae.IGRAPH_OUT) == [g.successors(v) for v in range(k)]
            v = int(rng.integers(0, k))
            assert g.neighbors(v, "in") == g.predecessors(v) and g.neighbors(v, "out") == g.successors(v)
            assert g.neighbors(v) == sorted(g.predecessors(v) + g.successors(v))
    with pytest.raises(ValueError):
        g.neighbors(0, "sideways")


FAKE = 1 << 20   # a non-null pointer (never dereferenced: nothing here launches)


def _args(**kw):
    a = _lib.DvaeSelectArgs()
    a.A, a.B, a.n, a.nvt, a.start_type, a.end_type, a.kind, a.n_nodes, a.select = 500, 50, 8, 8, 0, 1, 0, 0, 0
    for f in ("types", "preds", "nv", "valid", "pick", "n_valid", "n_same", "work"):
        setattr(a, f, FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_select_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.dagnn_dvae_select_work_bytes(C.byref(_args())) == 500 * 50 * 8
    assert lib.dagnn_dvae_select_key_words(0, 8, 8) == 1 and lib.dagnn_dvae_select_key_words(1, 10, 10) == 1
    assert lib.dagnn_dvae_select_key_words(0, 32, 64) == 10 and lib.dagnn_dvae_select_key_words(1, 32, 64) == 15
    assert lib.dagnn_dvae_select_key_words(2, 8, 8) == 0 and lib.dagnn_dvae_select_key_words(0, 33, 8) == 0
    bad = [dict(A=0), dict(B=0), dict(A=1 << 20, B=1 << 11), dict(n=1), dict(n=33), dict(nvt=0), dict(nvt=65),
           dict(start_type=8), dict(end_type=-1), dict(kind=2), dict(kind=-1), dict(select=2), dict(n_nodes=-1),
           dict(n_nodes=33)]
    for kw in bad:
        a = _args(**kw)
        assert lib.dagnn_dvae_select_work_bytes(C.byref(a)) == 0, kw
        assert lib.dagnn_dvae_select(C.byref(a), None) == -22, kw
    for f in ("types", "preds", "nv", "valid", "pick", "n_valid", "n_same", "work"):
        assert lib.dagnn_dvae_select(C.byref(_args(**{f: None})), None) == -22, f
    assert lib.dagnn_dvae_select(C.byref(_args(work_bytes=500 * 50 * 8 - 1)), None) == -28
    assert lib.dagnn_dvae_select(None, None) == -22 and lib.dagnn_dvae_select_work_bytes(None) == 0


def test_python_layer_refuses_bad_arguments():
    d = dvae.DecodedDense(*(torch.zeros(2, 3, 8, dtype=torch.int32) for _ in range(2)), torch.zeros(2, 3, dtype=torch.int32),
                          None)
    for kw in (dict(data_type="NAS"), dict(select="mode"), dict(n_nodes="fixed"), dict(n_nodes=40)):
        args = dict(data_type="ENAS", nvt=8, start_type=0, end_type=1)
        args.update(kw)
        with pytest.raises(ValueError):
            dvae.select_decoded(d, **args)
    meta, _ = Hh.load("dvae_decode_na_h64_L2_argmax")
    model, _ = Hh.dvae_model(meta)
    with pytest.raises(ValueError, match="decode_attempts"):
        dvae.decode_from_latent_space(torch.zeros(3, 56), model, 0)
    with pytest.raises(ValueError, match="data_type"):
        dvae.decode_from_latent_space(torch.zeros(3, 56), model, 5, data_type="NAS")
    with pytest.raises(_lib.DagnnHipError, match="GPU"):
        dvae.decode_from_latent_space(torch.zeros(3, 56), model, 5)
    model_add, _ = Hh.dvae_model(dict(meta, agg="add"))
    with pytest.raises(NotImplementedError, match="attn_h"):
        dvae.decode_from_latent_space(torch.zeros(3, 56), model_add, 5)
