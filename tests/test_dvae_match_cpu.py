"""Host side of the D-VAE evaluation metrics (csrc/dvae_match.hip): the host mirrors of `is_same_DAG`, the training-set
lookup and the distinct count against the `dvae_match_*` fixtures of the reference's own dvae/util.py, `prior_validity`
on host rows, `GraphSet.from_graphs`, the C structs and the argument checks of the entry points - none of it needs a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from dagnn_amd import _lib, dvae, synth
from tests import helpers as Hh

FIXTURES = ["dvae_match_enas_a12", "dvae_match_bn_a12", "dvae_match_enas_a40", "dvae_match_bn_a40", "dvae_match_enas_none",
            "dvae_match_bn_none"]


def fixture_rows(name):
    """(meta, rows dict, same [A,B], valid [A,B], in_train [A,B]) of a fixture; rows of the big ones come back from their seed."""
    meta, arr = Hh.load(name)
    A, B = meta["A"], meta["B"]
    if meta["rows_stored"]:
        rows = {k: arr[k] for k in ("types", "preds", "nv", "types_true", "preds_true", "nv_true", "types_train", "preds_train",
                                    "nv_train")}
    else:
        rows = synth.match_rows(meta["seed"], meta["kind"], A, B, meta["n"], meta["nvt"], meta["n_train"],
                                all_invalid=meta["all_invalid"])
    flags = [np.unpackbits(arr[k])[:A * B].reshape(A, B).astype(bool) for k in ("same", "valid", "in_train")]
    return (meta, rows) + tuple(flags)


def host_metrics(rows, kind, nvt):
    """The reference's prior-validity numbers from the host mirrors: (valid, n_unique, n_in_train)."""
    valid = dvae.select_host(rows["types"], rows["preds"], rows["nv"], kind, nvt, 0, 1)[0]
    form = dvae.enas_string if kind == "ENAS" else dvae.bn_adj_string
    strings = {form(rows["types"][a, b], rows["preds"][a, b], rows["nv"][a, b]) for a, b in zip(*np.nonzero(valid))}
    train = dvae.GraphSet.from_dense(rows["types_train"], rows["preds_train"], rows["nv_train"])
    _, count = train.contains((rows["types"], rows["preds"], rows["nv"]), valid.astype(np.int32))
    return valid, len(strings), int(count)


def test_stored_rows_are_the_generators():
    for name in FIXTURES[:2]:
        meta, arr = Hh.load(name)
        rows = synth.match_rows(meta["seed"], meta["kind"], meta["A"], meta["B"], meta["n"], meta["nvt"], meta["n_train"])
        for k, v in rows.items():
            np.testing.assert_array_equal(arr[k], v, err_msg=name + " " + k)


@pytest.mark.parametrize("name", FIXTURES)
def test_same_dag_host_reproduces_the_reference(name):
    meta, rows, same, _, _ = fixture_rows(name)
    got, per, total = dvae.same_dag_host(rows["types"], rows["preds"], rows["nv"], rows["types_true"], rows["preds_true"],
                                         rows["nv_true"])
    np.testing.assert_array_equal(got, same)
    assert per.tolist() == meta["per_graph"] and total == meta["n_same"]
    d = dvae.DecodedDense(*(torch.from_numpy(rows[k]) for k in ("types", "preds", "nv")), None)
    res = dvae.same_dag_dense(d, rows["types_true"], rows["preds_true"], rows["nv_true"])
    np.testing.assert_array_equal(res.same.numpy().astype(bool), same)
    assert res.per_graph.tolist() == meta["per_graph"] and res.total.tolist() == [meta["n_same"]]


@pytest.mark.parametrize("name", FIXTURES)
def test_graph_set_and_distinct_keys_host_mirrors_reproduce_the_reference(name):
    meta, rows, _, valid, in_train = fixture_rows(name)
    kind, n, nvt = meta["kind"], meta["n"], meta["nvt"]
    train = dvae.GraphSet.from_dense(rows["types_train"], rows["preds_train"], rows["nv_train"])
    assert len(train) == meta["n_train"] and train.distinct() == meta["train_distinct"]
    dense = (rows["types"], rows["preds"], rows["nv"])
    member, count = train.contains(dense)
    np.testing.assert_array_equal(member.numpy().astype(bool), in_train)
    got_valid, n_unique, n_in = host_metrics(rows, kind, nvt)
    np.testing.assert_array_equal(got_valid, valid)
    member, count = train.contains(dense, torch.from_numpy(valid.astype(np.int32)))
    np.testing.assert_array_equal(member.numpy().astype(bool), in_train & valid)
    assert count.tolist() == [meta["n_in_train"]] == [n_in]
    assert n_unique == meta["n_unique"]
    d = dvae.DecodedDense(*(torch.from_numpy(x) for x in dense), None)
    sel = dvae.select_decoded(d, kind, nvt, 0, 1)
    for chunks in (1, 3):
        keys = dvae.DistinctKeys(dvae.select_key_words(kind, n, nvt), valid.size)
        for a in np.array_split(np.arange(meta["A"]), chunks):
            keys.add(sel.keys[:, a], sel.valid[a])
        assert keys.count() == meta["n_unique"]


class _Rows(object):
    """A stand-in model that serves prepared rows as host tensors, point-sliced like a decode of z's rows."""

    def __init__(self, rows, kind, n, nvt):
        self.rows, self.kind, self.max_n, self.nvt, self.nz, self.START_TYPE, self.END_TYPE = rows, kind, n, nvt, 4, 0, 1

    def get_device(self):
        return torch.device("cpu")

    def decode_dense(self, z, stochastic, attempts, draws):
        idx = z[:, 0].long().numpy()
        assert stochastic and tuple(draws[0].shape) == (attempts, self.max_n, len(idx))
        t = lambda k: torch.from_numpy(np.ascontiguousarray(self.rows[k][:, idx]))  # noqa: E731
        return dvae.DecodedDense(t("types"), t("preds"), t("nv"), None)

    def select_dense(self, d, data_type):
        return dvae.select_decoded(d, data_type, self.nvt, 0, 1)


@pytest.mark.parametrize("name", FIXTURES)
def test_prior_validity_matches_the_reference_on_host_rows(name):
    meta, rows, _, _, _ = fixture_rows(name)
    A, B, kind = meta["A"], meta["B"], meta["kind"]
    model = _Rows(rows, kind, meta["n"], meta["nvt"])
    train = dvae.GraphSet.from_dense(rows["types_train"], rows["preds_train"], rows["nv_train"])
    z = torch.arange(B, dtype=torch.float32).view(B, 1).repeat(1, 4)
    for batch in (None, 5):
        res = dvae.prior_validity(model, train, decode_times=A, data_type=kind, z=z, batch_size=batch)
        assert (res.n_valid, res.n_total, res.n_unique, res.n_in_train) == (meta["n_valid"], A * B, meta["n_unique"],
                                                                            meta["n_in_train"])
        assert res.r_valid == meta["n_valid"] / (A * B)
        if meta["n_valid"]:
            assert res.r_unique == meta["n_unique"] / meta["n_valid"]
            assert abs(res.r_novel - (1 - meta["ratio_same_DAG"])) < 1e-12
        else:
            assert res.r_unique == 0.0 and res.r_novel == 0.0


def test_fixtures_hold_the_deciding_cases():
    for name in FIXTURES[:4]:
        meta, rows, same, valid, in_train = fixture_rows(name)
        A, B = meta["A"], meta["B"]
        for b in range(1, B):
            a0 = b % A
            assert same[a0, b] and not same[[(a0 + j) % A for j in (1, 2, 3, 4)], b].any(), (name, b)
            k = rows["nv_true"][b]
            assert (rows["nv"][[(a0 + 3) % A, (a0 + 4) % A], b] != k).any()
        assert meta["points_without_valid"] >= 1 and meta["in_train_invalid"] >= 1
        assert meta["train_distinct"] < meta["n_train"] and 0 < meta["n_in_train"] < meta["n_valid"]
        assert meta["n_unique"] < meta["n_valid"]
    assert Hh.load("dvae_match_enas_a40")[0]["n_unique"] < Hh.load("dvae_match_enas_a40")[0]["n_unique_per_point_sum"]
    # BN: both vertex orders of a graph among the valid rows - one string, two DAGs
    meta, rows, _, valid, _ = fixture_rows("dvae_match_bn_a40")
    seen = {}
    for a, b in zip(*np.nonzero(valid)):
        r = (rows["types"][a, b], rows["preds"][a, b], rows["nv"][a, b])
        seen.setdefault(dvae.bn_adj_string(*r), set()).add(dvae._record(*r))
    assert any(len(v) > 1 for v in seen.values())
    for name in FIXTURES[4:]:
        assert Hh.load(name)[0]["n_valid"] == 0


def test_graph_set_from_graphs_reads_what_decode_schedule_reads():
    types, preds = Hh.dvae_dense_graphs("random0.5", 9, 8, 8, 0, 3)
    G = Hh.dvae_graphs_from_dense(types, preds, 8)
    t2, p2 = dvae.decode_schedule(G, 8, 8)
    t3, p3, nv = dvae.dense_rows(G, 8, 8)
    np.testing.assert_array_equal(t2, t3)
    np.testing.assert_array_equal(p2, p3)
    assert nv.tolist() == [8] * 9
    gs = dvae.GraphSet.from_graphs(G, 8, 8)
    assert len(gs) == 9 and gs.contains((types, preds, nv))[1].tolist() == [9]
    short = Hh.dvae_graphs_from_dense(types[:, :5], preds[:, :5], 8)
    t4, p4, nv4 = dvae.dense_rows(short, 8, 8)
    assert nv4.tolist() == [5] * 9 and (t4[:, 5:] == -1).all() and (p4[:, 5:] == 0).all()
    np.testing.assert_array_equal(t4[:, :5], types[:, :5])
    assert dvae.GraphSet.from_graphs(short, 8, 8).contains((types, preds, nv))[1].tolist() == [0]
    with pytest.raises(ValueError, match="vertices"):
        dvae.dense_rows(G, 7, 8)


FAKE = 1 << 20   # a non-null pointer (never dereferenced: nothing here launches)


def _set(form=0, width=8, max_rows=1000, data=FAKE, nbytes=None):
    s = _lib.DvaeSet()
    s.form, s.width, s.max_rows, s.data = form, width, max_rows, data
    s.bytes = _lib.load().dagnn_dvae_set_bytes(form, width, max_rows) if nbytes is None else nbytes
    return s


def _rows_args(s, **kw):
    a = _lib.DvaeSetRowsArgs()
    a.set, a.base, a.A, a.B = s, 0, 10, 50
    for f in ("types", "preds", "nv", "keys", "mask", "member", "count"):
        setattr(a, f, FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    # capacity rule: 16 header words, the power of two >= 2 * max_rows slots (at least 64), max_rows records
    assert lib.dagnn_dvae_set_bytes(0, 8, 1000) == 4 * (16 + 2048 + 1000 * 17)
    assert lib.dagnn_dvae_set_bytes(1, 1, 10) == 4 * (16 + 64 + 10 * 2)
    assert lib.dagnn_dvae_set_bytes(0, 32, 1 << 20) == 4 * (16 + (1 << 21) + (1 << 20) * 65)
    for form, width, rows in ((2, 8, 10), (-1, 8, 10), (0, 1, 10), (0, 33, 10), (1, 0, 10), (1, 17, 10), (0, 8, 0),
                              (0, 8, (1 << 20) + 1)):
        assert lib.dagnn_dvae_set_bytes(form, width, rows) == 0, (form, width, rows)
        assert lib.dagnn_dvae_set_init(C.byref(_set(form, width, rows, nbytes=1 << 30)), None) == -22
        assert lib.dagnn_dvae_set_add(C.byref(_rows_args(_set(form, width, rows, nbytes=1 << 30))), None) == -22
    need = lib.dagnn_dvae_set_bytes(0, 8, 1000)
    # an undersized buffer, and rows beyond max_rows, are refused before anything is launched
    assert lib.dagnn_dvae_set_init(C.byref(_set(nbytes=need - 1)), None) == -28
    assert lib.dagnn_dvae_set_add(C.byref(_rows_args(_set(nbytes=need - 1))), None) == -28
    assert lib.dagnn_dvae_set_query(C.byref(_rows_args(_set(nbytes=need - 1))), None) == -28
    assert lib.dagnn_dvae_set_add(C.byref(_rows_args(_set(), base=501)), None) == -28
    assert lib.dagnn_dvae_set_add(C.byref(_rows_args(_set(), A=21)), None) == -28
    for kw in (dict(A=0), dict(B=0), dict(A=1 << 11, B=1 << 10), dict(base=-1), dict(types=None), dict(preds=None)):
        assert lib.dagnn_dvae_set_add(C.byref(_rows_args(_set(), **kw)), None) == -22, kw
        assert lib.dagnn_dvae_set_query(C.byref(_rows_args(_set(), **kw)), None) == -22, kw
    assert lib.dagnn_dvae_set_add(C.byref(_rows_args(_set(1, 2), keys=None)), None) == -22
    assert lib.dagnn_dvae_set_query(C.byref(_rows_args(_set(1, 2))), None) == -22   # keys cannot be queried
    for f in ("member", "count"):
        assert lib.dagnn_dvae_set_query(C.byref(_rows_args(_set(), **{f: None})), None) == -22, f
    assert lib.dagnn_dvae_set_init(C.byref(_set(data=None)), None) == -22 and lib.dagnn_dvae_set_init(None, None) == -22
    assert lib.dagnn_dvae_set_add(None, None) == -22 and lib.dagnn_dvae_set_query(None, None) == -22

    def same(**kw):
        a = _lib.DvaeSameDagArgs()
        a.A, a.B, a.n = 10, 32, 8
        for f in ("types", "preds", "nv", "types_true", "preds_true", "nv_true", "same", "per_graph", "total"):
            setattr(a, f, FAKE)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for kw in (dict(A=0), dict(B=0), dict(A=1 << 11, B=1 << 10), dict(n=1), dict(n=33), dict(types=None), dict(preds=None),
               dict(nv=None), dict(types_true=None), dict(preds_true=None), dict(same=None), dict(per_graph=None),
               dict(total=None)):
        assert lib.dagnn_dvae_same_dag(C.byref(same(**kw)), None) == -22, kw
    assert lib.dagnn_dvae_same_dag(None, None) == -22


def test_python_layer_refuses_bad_arguments():
    rows = synth.match_rows(1, "ENAS", 5, 4, 8, 8, 10)
    train = dvae.GraphSet.from_dense(rows["types_train"], rows["preds_train"], rows["nv_train"])
    model = _Rows(rows, "ENAS", 8, 8)
    z = torch.zeros(4, 4)
    with pytest.raises(ValueError, match="data_type"):
        dvae.prior_validity(model, train, decode_times=5, data_type="NAS", z=z)
    with pytest.raises(ValueError, match="decode_times"):
        dvae.prior_validity(model, train, decode_times=0, z=z)
    with pytest.raises(ValueError, match="at most"):
        dvae.prior_validity(model, train, decode_times=1 << 19, z=z)
    with pytest.raises(ValueError, match="GraphSet"):
        dvae.prior_validity(model, None, decode_times=5, z=z)
    with pytest.raises(ValueError, match="draws"):
        dvae.prior_validity(model, train, decode_times=5, z=z, draws=(torch.zeros(1), torch.zeros(1)))
    with pytest.raises(ValueError, match="rows of 8"):
        train.contains((rows["types"][..., :7], rows["preds"][..., :7], rows["nv"]))
    meta, _ = Hh.load("dvae_decode_na_h64_L2_argmax")
    real, _ = Hh.dvae_model(meta)
    G = Hh.dvae_graphs_from_dense(*Hh.dvae_dense_graphs("chain", 3, 8, 8, 0, 1), 8)
    with pytest.raises(_lib.DagnnHipError, match="GPU"):
        dvae.recon_accuracy(real, G)
    with pytest.raises(ValueError, match="encode_times"):
        dvae.recon_accuracy(real, G, encode_times=0)
    with pytest.raises(_lib.DagnnHipError, match="GPU"):   # the engine wrappers have no CPU path
        dvae.engine.dvae_same_dag(torch.zeros(2, 3, 8, dtype=torch.int32), torch.zeros(2, 3, 8, dtype=torch.int32),
                                  torch.zeros(2, 3, dtype=torch.int32), torch.zeros(3, 8, dtype=torch.int32),
                                  torch.zeros(3, 8, dtype=torch.int32))
