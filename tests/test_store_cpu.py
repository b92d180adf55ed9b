"""The graph store on the host (-m "not gpu"): the packed layout, the numpy definition of the gather (`store.gather_host`)
against the reference-generated fixture (tests/golden/make_golden_code2_store.py) and against this package's own host
collation, the loader's order and filters, the error cases, and the entry point's argument refusals.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from dagnn_amd import GraphBatch, GraphData, GraphStore, _lib, augment_edge2, dag_utils, synth
from dagnn_amd.evaluate import encode_ref_sets
from dagnn_amd.store import gather_host
from tests import helpers as Hh

FIXTURE = "code2_store_small"
RAW_KEYS = ("x", "node_depth", "edge_index", "node_is_attributed", "y_arr")
# what a store batch carries (plus the host int `num_graphs`), and nothing else
ATTRS = ("x", "node_depth", "edge_index", "edge_attr", "batch", "ptr", "_bi_layer_idx0", "_bi_layer_idx1", "_bi_layer_index0",
         "_bi_layer_index1", "len_longest_path", "y_arr")
EINVAL = -22


# ------------------------------------------------------------------ shared with tests/test_store_gpu.py
def fixture_graphs():
    meta, arr = Hh.load(FIXTURE)
    raw = [GraphData(**{k: torch.from_numpy(arr["raw%d::%s" % (i, k)].copy()) for k in RAW_KEYS}) for i in range(meta["graphs"])]
    return meta, arr, raw


def fixture_batch(arr, name):
    return {k: torch.from_numpy(arr["%s::%s" % (name, k)].copy()) for k in ATTRS}


def raw_synth(seed, num, mean_n=30, max_n=1000, S=3):
    """`synth.code2_graphs` as RAW graphs: next-token edges and layer ids removed, the leaves attributed, a `y_arr` row."""
    rng = np.random.default_rng(seed + 1000)
    out = []
    for g in synth.code2_graphs(seed, num, mean_n, max_n):
        ast = g.edge_index[:, g.edge_attr[:, 0] == 0]
        leaf = torch.ones(g.x.shape[0], dtype=torch.long)
        leaf[ast[0]] = 0
        out.append(GraphData(x=g.x, node_depth=g.node_depth, edge_index=ast.contiguous(), node_is_attributed=leaf.view(-1, 1),
                             y_arr=torch.from_numpy(rng.integers(0, 50, size=(1, S)))))
    return out


def prep(g):
    d = g.clone()
    augment_edge2(d)
    dag_utils.add_order_info_01(d)
    return d


def host_batch(raw, idx):
    """The host path a store batch must equal, as a dict over ATTRS: clone, augment_edge2, add_order_info_01, collate."""
    graphs = [prep(raw[i]) for i in idx]
    b = GraphBatch.from_data_list(graphs)
    want = {k: b[k] for k in ATTRS if k != "len_longest_path" and b[k] is not None}
    want["len_longest_path"] = torch.tensor([float(g._bi_layer_idx0.max()) for g in graphs], dtype=torch.float32)
    return want


def assert_batch(got, want, num_graphs, extra=()):
    keys = set(got.keys) - {"num_graphs"}
    assert keys == set(want) | set(extra), keys ^ (set(want) | set(extra))
    assert got.num_graphs == num_graphs and isinstance(got.num_graphs, int)
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (k, g.dtype, w.dtype, tuple(g.shape), tuple(w.shape))
        assert g.is_contiguous(), k
        assert torch.equal(g.cpu(), w.cpu()), k
    assert got._bi_layer_index0.data_ptr() != got._bi_layer_index1.data_ptr()


def index_lists(rng, G, count):
    """`count` id lists over G graphs: B from 1 to G, a descending one, ones with repeats, the rest random."""
    lists = [list(range(G - 1, -1, -1)), [int(rng.integers(0, G))], [3] * 7, list(range(G))]
    while len(lists) < count:
        B = int(rng.integers(1, G + 1))
        lists.append([int(i) for i in (rng.integers(0, G, size=B) if len(lists) % 2 else rng.permutation(G)[:B])])
    return lists


# ------------------------------------------------------------------ 1. the packed layout
def test_packed_layout_of_the_fixture_graphs():
    meta, arr, raw = fixture_graphs()
    st = GraphStore.from_graphs(raw, "cpu")
    a = {k: v.numpy() for k, v in st.arrays.items()}
    n = np.array([1, 1, 3, 6, 11, 23, 40, 4])
    assert st.num_graphs == 8 and a["node_ptr"].dtype == np.int64
    assert np.array_equal(a["node_ptr"], np.concatenate([[0], np.cumsum(n)]))
    assert np.array_equal(a["edge_ptr"], np.concatenate([[0], np.cumsum([0, 0, 2, 5, 10, 22, 39, 0])]))
    toks = [[], [0], [2], [1, 3, 5], None, None, None, [0, 2, 3]]
    for g in (4, 5, 6):   # the trees: the leaves, ascending
        ei = arr["raw%d::edge_index" % g]
        toks[g] = sorted(set(range(int(n[g]))) - set(ei[0].tolist()))
    assert np.array_equal(a["tok_ptr"], np.concatenate([[0], np.cumsum([len(t) for t in toks])]))
    assert a["tok"].dtype == np.int32 and a["tok"].tolist() == [v for t in toks for v in t]
    assert np.array_equal(st.counts, np.stack([n, np.diff(a["edge_ptr"]), [len(t) for t in toks]]))
    nxt = np.maximum(st.counts[2] - 1, 0)
    assert nxt.tolist()[:4] == [0, 0, 0, 2] and nxt[7] == 2
    for k in ("x", "depth", "layer_f", "layer_b", "src", "dst", "depth_max", "y_arr"):
        assert a[k].dtype == np.int32, k
    # AST edges keep their order and their ids inside the graph
    assert a["src"][:7].tolist() == [0, 0, 0, 1, 2, 3, 4] and a["dst"][:7].tolist() == [1, 2, 1, 2, 3, 4, 5]
    assert np.array_equal(a["src"], np.concatenate([arr["raw%d::edge_index" % g][0] for g in range(8)]))
    assert np.array_equal(a["x"], np.concatenate([arr["raw%d::x" % g] for g in range(8)]))
    assert np.array_equal(a["depth"], np.concatenate([arr["raw%d::node_depth" % g][:, 0] for g in range(8)]))
    assert np.array_equal(a["y_arr"], np.concatenate([arr["raw%d::y_arr" % g] for g in range(8)]))
    # longest paths of the AUGMENTED graphs: the chain 0..5 has depth 5, the edge-less graphs 0, tok edges 0->2->3 give 2
    assert a["depth_max"][:4].tolist() == [0, 0, 1, 5] and a["depth_max"][7] == 2
    assert a["layer_f"][-4:].tolist() == [0, 0, 1, 2] and a["layer_b"][-4:].tolist() == [2, 0, 1, 0]
    assert np.array_equal(a["depth_max"], arr["identity::len_longest_path"].astype(np.int32))


# ------------------------------------------------------------------ 2. the numpy definition against the reference's batches
@pytest.mark.parametrize("name", ["identity", "permuted"])
def test_gather_host_equals_the_reference_batches(name):
    meta, arr, raw = fixture_graphs()
    st = GraphStore.from_graphs(raw, "cpu")
    idx = arr[name + "::idx"]
    assert_batch(st.batch(idx), fixture_batch(arr, name), len(idx))
    out = gather_host({k: v.numpy() for k, v in st.arrays.items()}, idx)
    assert sorted(out) == sorted(ATTRS)


# ------------------------------------------------------------------ 3. against this package's host collation
def test_gather_host_equals_host_collation_on_random_lists():
    raw = raw_synth(5, 40)
    st = GraphStore.from_graphs(raw, "cpu")
    lists = index_lists(np.random.default_rng(11), 40, 20)
    assert len(lists) == 20 and {1, 40} <= {len(l) for l in lists}
    for ids in lists:
        assert_batch(st.batch(ids), host_batch(raw, ids), len(ids))
    # a list, a numpy array and a CPU tensor are the same ids
    a, b, c = st.batch([4, 2, 4]), st.batch(np.array([4, 2, 4], dtype=np.int32)), st.batch(torch.tensor([4, 2, 4]))
    assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.edge_index, c.edge_index)


def test_batches_do_not_alias_the_store():
    meta, arr, raw = fixture_graphs()
    st = GraphStore.from_graphs(raw, "cpu")
    first = st.batch([6, 3])
    keep = {k: first[k].clone() for k in ATTRS}
    for k in ATTRS:
        first[k].fill_(7)
    second = st.batch([6, 3])
    assert all(torch.equal(second[k], keep[k]) for k in ATTRS)


# ------------------------------------------------------------------ 4. the PyG in-memory form
def test_from_slices_equals_from_graphs():
    raw = raw_synth(6, 12)
    words = [["w%d" % (i % 5), "oov"][: 1 + i % 2] for i in range(12)]
    vocab = {"w%d" % i: i for i in range(5)}
    vocab.update({"__UNK__": 5, "__EOS__": 6})
    for g, w in zip(raw, words):
        g.y = w
    a = GraphStore.from_graphs(raw, "cpu", vocab)
    data = GraphData(x=torch.cat([g.x for g in raw]), node_depth=torch.cat([g.node_depth for g in raw]),
                     node_is_attributed=torch.cat([g.node_is_attributed for g in raw]),
                     edge_index=torch.cat([g.edge_index for g in raw], dim=1), y_arr=torch.cat([g.y_arr for g in raw]), y=words)
    nodes = torch.tensor([0] + [g.x.shape[0] for g in raw]).cumsum(0)
    slices = {"x": nodes, "node_depth": nodes, "node_is_attributed": nodes,
              "edge_index": torch.tensor([0] + [g.edge_index.shape[1] for g in raw]).cumsum(0)}
    b = GraphStore.from_slices(data, slices, "cpu", vocab)
    assert sorted(a.arrays) == sorted(b.arrays) and "ref_ids" in a.arrays
    for k in a.arrays:
        assert a.arrays[k].dtype == b.arrays[k].dtype and torch.equal(a.arrays[k], b.arrays[k]), k
    assert np.array_equal(a.counts, b.counts) and a.eos_id == b.eos_id == 6


# ------------------------------------------------------------------ 5. errors
def test_value_errors():
    meta, arr, raw = fixture_graphs()
    st = GraphStore.from_graphs(raw, "cpu")
    for bad in ([], np.zeros(0, dtype=np.int64), [8], [0, -1], [0, 1 << 40], [0.5]):
        with pytest.raises(ValueError):
            st.batch(bad)
    with pytest.raises(ValueError):
        list(st.loader([], 4))
    big = [g.clone() for g in raw]
    big[5].x[3, 1] = 2 ** 31
    with pytest.raises(ValueError, match="int32"):
        GraphStore.from_graphs(big, "cpu")
    big[5].x[3, 1] = 2 ** 31 - 1   # the largest value that fits
    assert int(GraphStore.from_graphs(big, "cpu").arrays["x"].max()) == 2 ** 31 - 1
    cyc = [g.clone() for g in raw]
    cyc[2].edge_index = torch.tensor([[0, 1, 2], [1, 2, 0]])
    with pytest.raises(ValueError, match="cycle"):
        GraphStore.from_graphs(cyc, "cpu")
    for k in ("x", "node_depth", "edge_index", "node_is_attributed"):
        miss = [g.clone() for g in raw]
        delattr(miss[4], k)
        with pytest.raises(ValueError, match=k):
            GraphStore.from_graphs(miss, "cpu")
    out_of_graph = [g.clone() for g in raw]
    out_of_graph[2].edge_index = torch.tensor([[0, 0], [1, 3]])   # node 3 of a 3-node graph
    with pytest.raises(ValueError):
        GraphStore.from_graphs(out_of_graph, "cpu")
    words = [GraphData(**dict(g.__dict__, y=["a"])) for g in raw]
    with pytest.raises(ValueError, match="vocab2idx"):
        GraphStore.from_graphs(words, "cpu")
    with pytest.raises(ValueError):
        st.evaluate_tok(None, [0], 1)   # packed without label words


# ------------------------------------------------------------------ 6. the loader
def _ids_of(st, batches):
    """The graph ids of loader batches, recovered from their node counts and first rows."""
    out = []
    for b in batches:
        ids = []
        for s in range(b.num_graphs):
            v0, v1 = int(b.ptr[s]), int(b.ptr[s + 1])
            hit = [g for g in range(st.num_graphs) if st.counts[0][g] == v1 - v0
                   and torch.equal(st.arrays["x"][int(st.arrays["node_ptr"][g]):int(st.arrays["node_ptr"][g + 1])].long(), b.x[v0:v1])]
            assert len(hit) == 1
            ids.append(hit[0])
        out.append(ids)
    return out


def test_loader_order_filters_and_shuffle():
    meta, arr, raw = fixture_graphs()
    st = GraphStore.from_graphs(raw, "cpu")
    ids = [7, 6, 5, 4, 3, 2, 1]
    assert _ids_of(st, st.loader(ids, 3)) == [[7, 6, 5], [4, 3, 2]]                 # the last batch is graph 1 alone: ONE node
    assert _ids_of(st, st.loader([7, 6, 5, 4, 3, 2, 1, 0], 3)) == [[7, 6, 5], [4, 3, 2], [1, 0]]   # short, two nodes: kept
    assert _ids_of(st, st.loader([3, 4, 2], 2)) == [[3, 4], [2]]                     # one graph of 3 nodes: kept ...
    assert _ids_of(st, st.loader([3, 4, 2], 2, training=True)) == [[3, 4]]           # ... but not by a training loop
    assert _ids_of(st, st.loader([0, 3, 1], 1)) == [[3]] and list(st.loader([0, 3, 1], 1, training=True)) == []
    pool = [2, 3, 4, 5, 6, 7, 3]
    one = _ids_of(st, st.loader(pool, 2, shuffle=True, seed=5))
    assert one == _ids_of(st, st.loader(pool, 2, shuffle=True, seed=5))
    perm = torch.randperm(len(pool), generator=torch.Generator().manual_seed(5)).tolist()
    assert [i for b in one for i in b] == [pool[p] for p in perm] and [len(b) for b in one] == [2, 2, 2, 1]
    other = _ids_of(st, st.loader(pool, 2, shuffle=True, seed=6))
    assert other != one and sorted(i for b in other for i in b) == sorted(pool)


# ------------------------------------------------------------------ 7. the C ABI (its layout: tests/test_abi_cpu.py)
def test_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.dagnn_store_gather(None, None) == EINVAL
    good = dict(B=2, N=3, E=1, ld_offsets=3, S=1, R=1)
    ptrs = [k for k, t in _lib.StoreGatherArgs._fields_ if t is C.c_void_p]

    def call(**kw):
        a = _lib.StoreGatherArgs()
        for k in ptrs:
            setattr(a, k, 4096)   # (never dereferenced: every case below is refused before any HIP call)
        for k, v in {**good, **kw}.items():
            setattr(a, k, v)
        return lib.dagnn_store_gather(C.byref(a), None)

    for k in ("B", "N", "E", "S", "R"):
        assert call(**{k: -1}) == EINVAL, k
    assert call(B=0) == EINVAL and call(B=0, N=0) == EINVAL           # B = 0 with nodes, with edges
    assert call(ld_offsets=2) == EINVAL
    for k in ("idx", "offsets", "node_ptr", "x", "depth", "edge_ptr", "tok_ptr", "src", "dst", "tok", "out_x", "out_depth",
              "out_edge_index", "out_edge_attr", "out_batch", "out_ptr", "out_index0", "out_index1"):
        assert call(**{k: None}) == EINVAL, k
    for out, src in (("out_layer_f", "layer_f"), ("out_layer_b", "layer_b"), ("out_llp", "depth_max"), ("out_y_arr", "y_arr"),
                     ("out_ref_ids", "ref_ids"), ("out_ref_ids", "ref_extra")):
        assert call(**{src: None}) == EINVAL, src
    assert call(out_ref_ids=None) == EINVAL and call(out_ref_extra=None) == EINVAL   # both or neither
    assert call(S=0) == EINVAL and call(R=0) == EINVAL
    assert call(out_x=4104) == EINVAL                                                  # a row of x is one 16-byte store
    a = _lib.StoreGatherArgs()
    assert lib.dagnn_store_gather(C.byref(a), None) == 0                               # B = N = E = 0: nothing to do


# ------------------------------------------------------------------ 8. the label id sets
def test_reference_sets_of_a_batch():
    raw = raw_synth(7, 10)
    vocab = {"w%d" % i: i for i in range(12)}
    vocab.update({"__UNK__": 12, "__EOS__": 13})
    rng = np.random.default_rng(3)
    words = [[("w%d" % rng.integers(0, 12)) if rng.random() < 0.7 else "oov%d" % rng.integers(0, 3) for _ in range(int(rng.integers(0, 9)))]
             for _ in raw]
    words[4] = ["w1", "w1", "__UNK__", "oov0", "oov0", "w3"]
    for g, w in zip(raw, words):
        g.y = w
    st = GraphStore.from_graphs(raw, "cpu", vocab)
    all_ids, _ = encode_ref_sets(words, vocab)
    R = all_ids.shape[1]
    assert tuple(st.arrays["ref_ids"].shape) == (10, R) and R > 1
    for ids in ([0], [9, 4, 4, 1], list(range(10)), [4]):
        b = st.batch(ids)
        want_ids, want_extra = encode_ref_sets([words[i] for i in ids], vocab)
        padded = torch.full((len(ids), R), -1, dtype=torch.int32)
        padded[:, :want_ids.shape[1]] = want_ids
        assert b.ref_ids.dtype == torch.int32 and torch.equal(b.ref_ids, padded)
        assert b.ref_extra.dtype == torch.int32 and torch.equal(b.ref_extra, want_extra)
        assert set(b.keys) - {"num_graphs"} == set(ATTRS) | {"ref_ids", "ref_extra"}
    assert st.batch([4]).ref_ids[0, :3].tolist() == [1, 12, 3] and int(st.batch([4]).ref_extra) == 1
