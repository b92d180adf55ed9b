"""The D-VAE store on the host (-m "not gpu"): the pack step and the numpy definition of the gather (`dvae_store.gather_host`)
against the reference-generated fixture (tests/golden/make_golden_dvae_store.py) and against this package's own decoders and
host collation, the layerings, the error cases, the loader, and the entry points' argument refusals.  Every comparison is exact."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from dagnn_amd import DagStore, GraphBatch, _lib, dag_utils, synth
from dagnn_amd.dvae import decode_schedule
from dagnn_amd.dvae_store import BATCH_KEYS, gather_host, layers_host, rows_to_dense, transpose_masks
from tests import helpers as Hh

FIXTURE = "dvae_store_small"
EINVAL = -22
SETS = {"enas": ("ENAS", synth.decode_enas_row, 8, 8), "bn": ("BN", synth.decode_bn_row, 10, 10)}   # kind, decoder, n, nvt


# ------------------------------------------------------------------ shared with tests/test_dvae_store_gpu.py
def fixture_rows(name):
    meta, arr = Hh.load(FIXTURE)
    return meta, arr, [json.loads(r) for r in arr[name + "::rows"]]


def host_batch(graphs, idx, nvt, y=None):
    """The host path a store batch must equal, as a dict: the collation of clones (without `vs`), `decode_schedule`, y."""
    picked = [graphs[i].clone() for i in idx]
    b = GraphBatch.from_data_list(picked)
    want = {k: b[k] for k in ("x", "edge_index", "bi_layer_index", "batch", "ptr")}
    t, p = decode_schedule(picked, int(picked[0].x.shape[0]), nvt)
    want["types"], want["preds"] = torch.from_numpy(t), torch.from_numpy(p)
    if y is not None:
        want["y"] = torch.as_tensor(np.asarray(y, dtype=np.float32)[np.asarray(idx)])
    return want


def assert_batch(got, want, num_graphs):
    keys = set(got.keys) - {"num_graphs"}
    assert keys == set(want), keys ^ set(want)
    assert "vs" not in got.keys
    assert got.num_graphs == num_graphs and isinstance(got.num_graphs, int)
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (k, g.dtype, w.dtype, tuple(g.shape), tuple(w.shape))
        assert g.is_contiguous(), k
        assert torch.equal(g.cpu(), w.cpu()), k


def complete_and_chain():
    """(types, preds) of two 32-vertex graphs: the complete DAG (496 edges; bit 31 set in succs, bits up to 30 in preds) and
    the chain."""
    n = 32
    types = np.full((2, n), 2, dtype=np.int32)
    types[:, 0], types[:, -1] = 0, 1
    preds = np.zeros((2, n), dtype=np.uint32)
    for v in range(n):
        preds[0, v] = (1 << v) - 1
        preds[1, v] = (1 << (v - 1)) if v else 0
    return types, preds.view(np.int32)


def dense_graphs(types, preds, nvt):
    return Hh.dvae_graphs_from_dense(types, preds, nvt)


def index_lists(rng, M, count):
    lists = [list(range(M - 1, -1, -1)), [int(rng.integers(0, M))], [M // 2] * 5, list(range(M))]
    while len(lists) < count:
        B = int(rng.integers(1, M + 1))
        lists.append([int(i) for i in (rng.integers(0, M, size=B) if len(lists) % 2 else rng.permutation(M)[:B])])
    return lists


# ------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("name", sorted(SETS))
def test_pack_equals_the_reference_decoders(name):
    meta, arr, rows = fixture_rows(name)
    kind, _, n, nvt = SETS[name]
    info = meta["sets"][name]
    assert (info["n"], info["nvt"], info["graphs"]) == (n, nvt, 6)
    if name == "enas":
        assert info["edges"][0] == 7 < n and info["edges"][1] == 22 == max(info["edges"])   # no skip; every skip
    else:
        assert info["edges"][0] == 16 and info["edges"][1] == 9                            # all parentless; the chain
    st = DagStore.from_rows(rows, kind, nvt, "cpu")
    a = {k: v.numpy() for k, v in st.arrays.items()}
    assert st.num_graphs == 6 and st.n == n and sorted(a) == ["layer_b", "layer_f", "preds", "succs", "types"]
    assert all(v.dtype == np.int32 and v.shape == (6, n) for v in a.values())
    assert st.edge_count.dtype == np.int64 and st.edge_count.tolist() == info["edges"]
    for g in range(6):
        assert np.array_equal(a["types"][g], arr["%s::g%d::types" % (name, g)])
        assert np.array_equal(a["types"][g], arr["%s::g%d::x" % (name, g)].argmax(1))
        ei = arr["%s::g%d::edge_index" % (name, g)]
        want_p, want_s = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for u, v in ei.T:
            want_p[v] |= 1 << u
            want_s[u] |= 1 << v
        assert np.array_equal(a["preds"][g], want_p) and np.array_equal(a["succs"][g], want_s)
        bi = arr["%s::g%d::bi_layer_index" % (name, g)]
        assert np.array_equal(a["layer_f"][g], bi[0, 0]) and np.array_equal(a["layer_b"][g], bi[1, 0])
        one = st.batch([g])
        for k in ("x", "edge_index", "bi_layer_index"):
            assert np.array_equal(one[k].numpy(), arr["%s::g%d::%s" % (name, g, k)]), (g, k)


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("which", ["identity", "permuted"])
def test_fixture_batches(name, which):
    meta, arr, rows = fixture_rows(name)
    kind, _, n, nvt = SETS[name]
    st = DagStore.from_rows(rows, kind, nvt, "cpu")
    ids = arr["%s::%s::idx" % (name, which)]
    b = st.batch(ids)
    for k in meta["batch_keys"]:
        w = arr["%s::%s::%s" % (name, which, k)]
        assert b[k].numpy().dtype == w.dtype and np.array_equal(b[k].numpy(), w), k
    assert np.array_equal(b.types.numpy(), arr["%s::%s::vs" % (name, which)])
    assert b.num_graphs == len(ids) and b.ptr.tolist() == [i * n for i in range(len(ids) + 1)]
    raw = gather_host(st._host, ids, nvt)
    assert sorted(raw) == sorted(BATCH_KEYS)
    for k in BATCH_KEYS:
        assert np.array_equal(raw[k], b[k].numpy()), k


# ------------------------------------------------------------------ 2. against this package's decoders and collation
@pytest.mark.parametrize("name", sorted(SETS))
def test_batches_equal_the_host_collation(name):
    kind, decode, n, nvt = SETS[name]
    M = 23
    rows = (synth.enas_rows if name == "enas" else synth.bn_rows)(5, M)
    y = np.random.default_rng(1).random(M)
    graphs = [decode(r) for r in rows]
    st = DagStore.from_rows(rows, kind, nvt, "cpu", y=y)
    lists = index_lists(np.random.default_rng(2), M, 12)
    assert {len(l) for l in lists} >= {1, M}
    for ids in lists:
        assert_batch(st.batch(ids), host_batch(graphs, ids, nvt, y), len(ids))
    for ids in (np.array(lists[0]), torch.tensor(lists[0]), np.array(lists[0], dtype=np.int32)):
        assert torch.equal(st.batch(ids).edge_index, st.batch(lists[0]).edge_index)
    assert st.arrays["y"].dtype == torch.float32


@pytest.mark.parametrize("name", sorted(SETS))
def test_constructors_agree_and_strings_equal_lists(name):
    kind, decode, n, nvt = SETS[name]
    rows = (synth.enas_rows if name == "enas" else synth.bn_rows)(9, 17)
    graphs = [decode(r) for r in rows]
    a = DagStore.from_rows(rows, kind, nvt, "cpu")
    b = DagStore.from_graphs(graphs, n, nvt, "cpu")
    c = DagStore.from_dense(a.arrays["types"], a.arrays["preds"].numpy(), nvt, "cpu")
    d = DagStore.from_rows([str(r) for r in rows], kind, nvt, "cpu")
    e = DagStore.from_rows([str(rows[0])] + rows[1:], kind, nvt, "cpu")          # mixed
    types, preds = decode_schedule(graphs, n, nvt)
    assert np.array_equal(a.arrays["types"].numpy(), types) and np.array_equal(a.arrays["preds"].numpy(), preds)
    for other in (b, c, d, e):
        assert sorted(other.arrays) == sorted(a.arrays)
        for k, v in a.arrays.items():
            assert torch.equal(other.arrays[k], v), k
        assert np.array_equal(other.edge_count, a.edge_count)
    with pytest.raises(ValueError):   # strings are parsed as literals, never evaluated
        DagStore.from_rows(["__import__('os').getcwd()"], kind, nvt, "cpu")


def test_thirty_two_vertices():
    types, preds = complete_and_chain()
    st = DagStore.from_dense(types, preds, 3, "cpu")
    assert st.edge_count.tolist() == [496, 31]
    succs = st.arrays["succs"].numpy().view(np.uint32)
    assert succs[0, 0] == 0xFFFFFFFE and succs[0, 30] == 0x80000000 and succs[0, 31] == 0 and succs[1, 30] == 0x80000000
    assert st.arrays["succs"][0, 30].item() < 0                                  # bit 31 in an int32 word
    graphs = dense_graphs(types, preds, 3)
    for ids in ([0], [1], [1, 0, 0, 1]):
        assert_batch(st.batch(ids), host_batch(graphs, ids, 3), len(ids))
    assert st.arrays["layer_f"][0].tolist() == list(range(32)) and st.arrays["layer_b"][1].tolist() == list(range(31, -1, -1))


# ------------------------------------------------------------------ 3. the layerings
def test_layers_equal_longest_path_layers():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 10, 32):
        M = 9
        preds = np.zeros((M, n), dtype=np.uint32)
        for g in range(M):
            for v in range(1, n):
                preds[g, v] = int(rng.integers(0, 1 << v)) & (int(rng.integers(0, 1 << v)) if g % 2 else (1 << v) - 1)
        succs = transpose_masks(preds)
        lf, lb = layers_host(preds.view(np.int32), succs)
        assert lf.dtype == np.int32 and lb.dtype == np.int32
        for g in range(M):
            ei = np.array([(u, v) for v in range(n) for u in range(v) if preds[g, v] >> u & 1], dtype=np.int64).reshape(-1, 2).T
            assert np.array_equal(lf[g], dag_utils.longest_path_layers(ei, n)), (n, g)
            assert np.array_equal(lb[g], dag_utils.longest_path_layers(ei[::-1], n)), (n, g)
            assert np.array_equal(transpose_masks(succs)[g], preds[g].view(np.int32))


# ------------------------------------------------------------------ 4. what is refused
def test_pack_errors():
    types = np.array([[0, 2, 3, 1], [0, 3, 2, 1]], dtype=np.int32)
    preds = np.array([[0, 1, 3, 4], [0, 1, 1, 6]], dtype=np.int32)
    DagStore.from_dense(types, preds, 4, "cpu")
    bad = types.copy()
    bad[1, 2] = 4
    with pytest.raises(ValueError, match=r"\[0, nvt=4\)"):
        DagStore.from_dense(bad, preds, 4, "cpu")
    bad[1, 2] = -1                                                               # a graph of fewer vertices, padded
    with pytest.raises(ValueError, match="exactly n"):
        DagStore.from_dense(bad, preds, 4, "cpu")
    bad[1, 2] = 0
    with pytest.raises(ValueError, match="START_TYPE"):
        DagStore.from_dense(bad, preds, 4, "cpu")
    DagStore.from_dense(bad, preds, 4, "cpu", start_type=1 << 20)                # (the rule follows start_type)
    for v, mask in ((1, 2), (2, 8), (0, 1), (3, -(1 << 31))):                   # u == v, u > v, vertex 0, bit 31
        worse = preds.copy()
        worse[0, v] = mask
        with pytest.raises(ValueError, match="u >= v"):
            DagStore.from_dense(types, worse, 4, "cpu")
    with pytest.raises(ValueError, match="at most 32"):
        DagStore.from_dense(np.zeros((1, 33), np.int32), np.zeros((1, 33), np.int32), 4, "cpu", start_type=9)
    with pytest.raises(ValueError):
        DagStore.from_dense(types, preds[:, :3], 4, "cpu")
    with pytest.raises(ValueError, match="one value per graph"):
        DagStore.from_dense(types, preds, 4, "cpu", y=[1.0, 2.0, 3.0])
    rows = synth.enas_rows(1, 3)
    with pytest.raises(ValueError, match="exactly n"):
        DagStore.from_rows(rows[:2] + [rows[2][:5]], "ENAS", 8, "cpu")
    with pytest.raises(ValueError, match="1 \\+ i entries"):
        DagStore.from_rows(rows[:2] + [rows[2][:5] + [[1, 0, 0]]], "ENAS", 8, "cpu")
    with pytest.raises(ValueError, match="kind"):
        DagStore.from_rows(rows, "NAS", 8, "cpu")
    with pytest.raises(ValueError, match=r"\[0, nvt=7\)"):
        DagStore.from_rows([[[5] + [0] * i for i in range(6)]], "ENAS", 7, "cpu")
    with pytest.raises(ValueError, match="at most 32|n = nodes"):
        DagStore.from_rows([[[0] + [0] * i for i in range(31)]], "ENAS", 8, "cpu")
    graphs = [synth.decode_enas_row(r) for r in rows]
    with pytest.raises(ValueError, match="exactly max_n"):
        DagStore.from_graphs(graphs + [synth.decode_bn_row(synth.bn_rows(1, 1)[0])], 10, 10, "cpu")
    back = graphs[1].clone()
    back.edge_index = torch.cat([back.edge_index, torch.tensor([[5], [2]])], dim=1)
    with pytest.raises(ValueError, match="u >= v"):
        DagStore.from_graphs([graphs[0], back], 8, 8, "cpu")


def test_batch_errors_and_no_aliasing():
    rows = synth.bn_rows(2, 5)
    st = DagStore.from_rows(rows, "BN", 10, "cpu", y=np.arange(5))
    for bad in ([], [5], [-1], [0.5], np.zeros(0, np.int64)):
        with pytest.raises(ValueError):
            st.batch(bad)
    with pytest.raises(ValueError):
        list(st.loader([0, 1], 0))
    keep = {k: v.clone() for k, v in st.arrays.items()}
    b = st.batch([0, 1, 2, 3, 4])
    for k in b.keys:
        if isinstance(b[k], torch.Tensor):
            assert all(b[k].data_ptr() != v.data_ptr() for v in st.arrays.values()), k
            b[k].fill_(7)
    for k, v in keep.items():
        assert torch.equal(st.arrays[k], v), k
    c = st.batch([0, 1, 2, 3, 4])
    assert all(c[k].data_ptr() != b[k].data_ptr() for k in BATCH_KEYS) and int(c.batch.max()) == 4


# ------------------------------------------------------------------ 5. the loader
def test_loader_order_short_last_batch_and_seeded_shuffle():
    rows = synth.enas_rows(4, 11)
    st = DagStore.from_rows(rows, "ENAS", 8, "cpu", y=np.arange(11))
    ids_of = lambda it: [[int(v) for v in b.y.tolist()] for b in it]   # noqa: E731  (y names the graph)
    pool = [9, 3, 3, 0, 10, 7, 1]
    assert ids_of(st.loader(pool, 3)) == [[9, 3, 3], [0, 10, 7], [1]]
    assert ids_of(st.loader(pool, 7)) == [pool] and ids_of(st.loader(pool, 100)) == [pool]
    perm = torch.randperm(len(pool), generator=torch.Generator().manual_seed(5)).tolist()
    one = ids_of(st.loader(pool, 2, shuffle=True, seed=5))
    assert one == ids_of(st.loader(pool, 2, shuffle=True, seed=5))
    assert [i for b in one for i in b] == [pool[p] for p in perm] and [len(b) for b in one] == [2, 2, 2, 1]
    other = ids_of(st.loader(pool, 2, shuffle=True, seed=6))
    assert other != one and sorted(i for b in other for i in b) == sorted(pool)


def test_graph_set_holds_the_packed_rows():
    rows = synth.bn_rows(6, 8)
    st = DagStore.from_rows(rows, "BN", 10, "cpu")
    gs = st.graph_set()
    assert len(gs) == 8 and gs.n == 10
    t, p = st.arrays["types"], st.arrays["preds"]
    member, count = gs.contains((t, p, torch.full((8,), 10, dtype=torch.int32)))
    assert member.tolist() == [1] * 8 and int(count) == 8
    t2 = t.clone()
    t2[3, 4] = (t2[3, 4] - 2 + 1) % 8 + 2
    assert gs.contains((t2, p, torch.full((8,), 10, dtype=torch.int32)))[0].tolist() == [1, 1, 1, 0, 1, 1, 1, 1]


# ------------------------------------------------------------------ 6. the C ABI (its layout: tests/test_abi_cpu.py)
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.dagnn_dag_store_gather(None, None) == EINVAL
    good = dict(B=2, n=8, nvt=8, E=9)
    ptrs = [k for k, t in _lib.DagStoreGatherArgs._fields_ if t is C.c_void_p]

    def call(**kw):
        a = _lib.DagStoreGatherArgs()
        for k in ptrs:
            setattr(a, k, 4096)   # (never dereferenced: every case below is refused before any HIP call)
        for k, v in {**good, **kw}.items():
            setattr(a, k, v)
        return lib.dagnn_dag_store_gather(C.byref(a), None)

    for k in ("B", "n", "nvt", "E"):
        assert call(**{k: -1}) == EINVAL, k
    assert call(n=0) == EINVAL and call(n=33) == EINVAL and call(nvt=0) == EINVAL
    assert call(B=0) == EINVAL                                            # B = 0 with edges
    assert call(B=0, E=0) == 0                                            # nothing to do
    assert call(E=2 * 28 + 1) == EINVAL                                   # more edges than B complete DAGs hold
    for k in ("types", "succs", "layer_f", "layer_b", "idx", "offsets", "out_x", "out_edge_index", "out_bi_layer_index",
              "out_batch", "out_ptr"):
        assert call(**{k: None}) == EINVAL, k
    assert call(preds=None) == EINVAL and call(y=None) == EINVAL          # an optional output without its source
    assert lib.dagnn_dag_store_gather(C.byref(_lib.DagStoreGatherArgs()), None) == EINVAL   # n = 0
    layers = lib.dagnn_dag_store_layers
    assert layers(4096, 4096, 0, 8, 4096, 4096, None) == 0                # M = 0: nothing to do
    assert layers(4096, 4096, -1, 8, 4096, 4096, None) == EINVAL
    assert layers(4096, 4096, 3, 0, 4096, 4096, None) == EINVAL and layers(4096, 4096, 3, 33, 4096, 4096, None) == EINVAL
    for hole in range(4):
        args = [4096, 4096, 3, 8, 4096, 4096, None]
        args[hole if hole < 2 else hole + 2] = None
        assert layers(*args) == EINVAL, hole
