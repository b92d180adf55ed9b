"""The graph store on the GPU (-m gpu): `dagnn_store_gather` against the reference-generated fixture, the host collation and
its numpy definition; what it may and may not write; no synchronisation; staging reuse; and the loops it feeds.  Every
comparison is exact - the feature has no floating-point arithmetic.  Shapes are the smallest that reach each path: graphs
of 1, ~30, 300 and 1 100 nodes (the last two larger than a workgroup), B around the wave size."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from dagnn_amd import (DAGNN, ASTNodeEncoder, ASTNodeEncoder2, GraphBatch, GraphData, GraphStore, _lib, class_cross_entropy, dag_utils,
                       engine, evaluate, evaluate_lp, lp_targets, synth)
from dagnn_amd.store import gather_host
from oracle.seeding import seeded_fill
from tests.test_store_cpu import ATTRS, assert_batch, fixture_batch, fixture_graphs, host_batch, prep, raw_synth

pytestmark = pytest.mark.gpu
N_ATTR = 10030
S = 3


def _sync_count(fn):
    """Synchronisations torch reports while fn runs (blocking copies and reads of device values)."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, sum("synchroniz" in str(x.message) for x in w)


def _tree(rng, n):
    g = synth.gen_ast(rng, n)
    ast = g["ei"][:, g["ea"][:, 0] == 0]
    leaf = np.ones(n, dtype=np.int64)
    leaf[ast[0]] = 0
    return GraphData(x=torch.from_numpy(g["x"]).long(), node_depth=torch.from_numpy(g["depth"]).long().view(-1, 1),
                     edge_index=torch.from_numpy(ast).long().contiguous(), node_is_attributed=torch.from_numpy(leaf).view(-1, 1),
                     y_arr=torch.from_numpy(rng.integers(0, 50, size=(1, S))))


_CACHE = {}
ONE, MID, BIG = 40, 41, 42     # the graphs of 1, 300 and 1 100 nodes behind the 40 small ones


def sweep_graphs():
    """40 code2-like graphs of about 30 nodes, then one of 1 node (no edge at all), of 300 and of 1 100 nodes; label words on
    every graph.  Built once; nothing changes them."""
    if "raw" not in _CACHE:
        rng = np.random.default_rng(77)
        raw = raw_synth(21, 40)
        raw.append(GraphData(x=torch.tensor([[5, 9]]), node_depth=torch.zeros(1, 1, dtype=torch.long),
                             edge_index=torch.zeros(2, 0, dtype=torch.long), node_is_attributed=torch.zeros(1, 1, dtype=torch.long),
                             y_arr=torch.tensor([[1, 2, 3]])))
        raw += [_tree(rng, 300), _tree(rng, 1100)]
        vocab = {"w%d" % i: i for i in range(48)}
        vocab["__UNK__"], vocab["__EOS__"] = 48, 49
        for g in raw:
            g.y = [("w%d" % rng.integers(0, 48)) if rng.random() < 0.8 else "oov%d" % rng.integers(0, 4) for _ in range(int(rng.integers(0, 7)))]
        _CACHE["raw"], _CACHE["vocab"] = raw, vocab
    return _CACHE["raw"], _CACHE["vocab"]


def sweep_store(device):
    if "store" not in _CACHE:
        raw, vocab = sweep_graphs()
        _CACHE["store"] = GraphStore.from_graphs(raw, device, vocab)
    return _CACHE["store"]


def sweep_lists():
    rng = np.random.default_rng(9)
    small = lambda k: [int(i) for i in rng.integers(0, 40, size=k)]   # noqa: E731
    return {"big_alone": [BIG],                                 # B = 1: one graph larger than any workgroup
            "one_node_first": [ONE, 17],                        # B = 2, the first graph without edges
            "last_without_edges": small(60) + [MID, BIG, ONE],  # B = 63
            "all_identical": [23] * 64,                         # B = 64, one id
            "first_and_last_without_edges": [ONE] + small(61) + [MID, 3, ONE],   # B = 65
            "descending": list(range(42, -1, -1))}


def test_sweep_lists_cover_the_cases():
    raw, _ = sweep_graphs()
    sizes = {k: (len(ids), sum(raw[i].x.shape[0] for i in ids),
                 sum(raw[i].edge_index.shape[1] + max(int(raw[i].node_is_attributed.sum()) - 1, 0) for i in ids))
             for k, ids in sweep_lists().items()}
    assert {v[0] for v in sizes.values()} >= {1, 2, 63, 64, 65}
    assert {v[1] % 2 for v in sizes.values()} == {0, 1} and {v[2] % 2 for v in sizes.values()} == {0, 1}, sizes
    assert raw[MID].x.shape[0] == 300 and raw[BIG].x.shape[0] == 1100 and raw[BIG].edge_index.shape[1] > 1024


# ------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("name", ["identity", "permuted"])
def test_fixture_batches(device, name):
    meta, arr, raw = fixture_graphs()
    st = GraphStore.from_graphs(raw, device)
    b = st.batch(arr[name + "::idx"])
    assert all(b[k].device == device for k in ATTRS)
    assert_batch(b, fixture_batch(arr, name), len(arr[name + "::idx"]))


# ------------------------------------------------------------------ 2. the sweep
@pytest.mark.parametrize("case", sorted(sweep_lists()))
def test_sweep_equals_host_collation(device, case):
    raw, vocab = sweep_graphs()
    ids = sweep_lists()[case]
    b = sweep_store(device).batch(ids)
    want = host_batch(raw, ids)
    want_ids, want_extra = evaluate.encode_ref_sets([raw[i].y for i in ids], vocab)
    R = sweep_store(device).arrays["ref_ids"].shape[1]
    want["ref_ids"] = torch.full((len(ids), R), -1, dtype=torch.int32)
    want["ref_ids"][:, :want_ids.shape[1]] = want_ids
    want["ref_extra"] = want_extra
    assert_batch(b, want, len(ids))


# ------------------------------------------------------------------ 3. the raw entry point
PAD = 37                         # sentinel words behind every output
SENT_I, SENT_F = -7777777, -12345.0
_OUT = {"out_x": ("x", torch.int64), "out_depth": ("node_depth", torch.int64), "out_edge_index": ("edge_index", torch.int64),
        "out_edge_attr": ("edge_attr", torch.float32), "out_batch": ("batch", torch.int64), "out_ptr": ("ptr", torch.int64),
        "out_index0": ("_bi_layer_index0", torch.int64), "out_index1": ("_bi_layer_index1", torch.int64),
        "out_layer_f": ("_bi_layer_idx0", torch.int64), "out_layer_b": ("_bi_layer_idx1", torch.int64),
        "out_llp": ("len_longest_path", torch.float32), "out_y_arr": ("y_arr", torch.int64), "out_ref_ids": ("ref_ids", torch.int32),
        "out_ref_extra": ("ref_extra", torch.int32)}
_OPTIONAL = ("out_layer_f", "out_layer_b", "out_llp", "out_y_arr", "out_ref_ids", "out_ref_extra")


def _raw_call(device, packed, dev_arrays, ids, skip=()):
    want = gather_host(packed, ids)
    ids = np.asarray(ids, dtype=np.int64)
    B = ids.size
    ext = np.stack([np.diff(packed["node_ptr"])[ids], np.diff(packed["edge_ptr"])[ids],
                    np.maximum(np.diff(packed["tok_ptr"])[ids] - 1, 0)])
    table = np.zeros((4, B + 5), dtype=np.int64)     # (a row pitch larger than B + 1)
    table[0, :B] = ids
    table[1:, 1:B + 1] = np.cumsum(ext, axis=1)
    table_d = torch.from_numpy(table).to(device)
    a = _lib.StoreGatherArgs()
    for k, t in dev_arrays.items():
        setattr(a, k, t.data_ptr())
    a.idx, a.offsets, a.ld_offsets = table_d.data_ptr(), table_d.data_ptr() + 8 * (B + 5), B + 5
    a.B, a.N, a.E = B, want["x"].shape[0], want["edge_index"].shape[1]
    a.S, a.R = packed["y_arr"].shape[1], packed["ref_ids"].shape[1]
    bufs = {}
    for field, (key, dtype) in _OUT.items():
        if field in skip:
            continue
        bufs[field] = torch.full((want[key].size + PAD,), SENT_F if dtype == torch.float32 else SENT_I, dtype=dtype, device=device)
        setattr(a, field, bufs[field].data_ptr())
    assert _lib.load().dagnn_store_gather(C.byref(a), engine._stream(table_d)) == 0
    torch.cuda.synchronize()
    return want, {k: v.cpu().numpy() for k, v in bufs.items()}


def test_entry_point_writes_its_extents_and_nothing_else(device):
    raw, vocab = sweep_graphs()
    host = GraphStore.from_graphs(raw, "cpu", vocab)
    packed = {k: v.numpy() for k, v in host.arrays.items()}
    dev_arrays = {k: v.to(device) for k, v in host.arrays.items()}
    for ids in ([BIG], [ONE, 7, ONE], [4, MID, 4, 9, ONE]):
        want, full = _raw_call(device, packed, dev_arrays, ids)
        for field, (key, dtype) in _OUT.items():
            n = want[key].size
            sent = np.float32(SENT_F) if dtype == torch.float32 else SENT_I
            assert np.array_equal(full[field][:n], np.ascontiguousarray(want[key]).reshape(-1)), (ids, field)
            assert not (full[field][:n] == sent).any(), (ids, field)          # every word inside was written
            assert (full[field][n:] == sent).all(), (ids, field)              # and none outside
        want, part = _raw_call(device, packed, dev_arrays, ids, skip=_OPTIONAL)
        assert sorted(part) == sorted(set(_OUT) - set(_OPTIONAL))
        for field in part:
            assert np.array_equal(part[field], full[field]), (ids, field)


# ------------------------------------------------------------------ 4. nothing synchronises
class _Replay(object):
    """A stand-in model whose `predict` hands out tokens computed before: the loop around it is what is counted."""
    training = False

    def __init__(self, toks):
        self.toks = list(toks)

    def eval(self):
        return self

    def predict(self, batch):
        return self.toks.pop(0)


def test_batch_and_evaluation_loop_do_not_synchronise(device):
    st = sweep_store(device)
    lists = sweep_lists()
    st.batch(lists["descending"])                      # warm-up: the pinned pool, the allocator
    torch.cuda.synchronize()
    for ids in lists.values():
        _, syncs = _sync_count(lambda: st.batch(ids))
        assert syncs == 0, syncs
    ids = list(range(43))
    g = torch.Generator().manual_seed(0)
    toks = [torch.randint(0, 50, (len(ids[i:i + 16]), S), generator=g).to(device) for i in range(0, 43, 16)]
    want = st.evaluate_tok(_Replay(toks), ids, 16)     # (also the warm-up)
    got, syncs = _sync_count(lambda: st.evaluate_tok(_Replay(toks), ids, 16))
    assert syncs == 1, syncs                           # the one copy in compute()
    assert got == want and got["n"] == 43


# ------------------------------------------------------------------ 5. staging reuse
def test_sixty_four_batches_in_flight(device):
    raw, _ = sweep_graphs()
    st = sweep_store(device)
    rng = np.random.default_rng(4)
    # (the first two ids number the list, so the 64 lists are different)
    lists = [[k % 43, k // 43] + [int(i) for i in rng.integers(0, 43, size=int(rng.integers(0, 11)))] for k in range(64)]
    assert len({tuple(l) for l in lists}) == 64
    torch.cuda.synchronize()
    batches, syncs = _sync_count(lambda: [st.batch(l) for l in lists])
    assert syncs == 0
    prepared = [prep(g) for g in raw]
    for l, b in zip(lists, batches):
        want = GraphBatch.from_data_list([prepared[i].clone() for i in l])
        for k in ("x", "node_depth", "edge_index", "edge_attr", "batch", "ptr", "_bi_layer_idx0", "_bi_layer_idx1", "y_arr"):
            assert torch.equal(b[k].cpu(), want[k]), (l, k)


# ------------------------------------------------------------------ 6. a pass does not reach the store
def _lp_model(device, H=32, L=2, max_depth=20, num_class=1200, seed=5):
    """(num_class above every graph's node count: each longest path is a class, the loss is finite)"""
    enc = ASTNodeEncoder2(H, 98, N_ATTR, max_depth)
    model = DAGNN(num_vocab=None, max_seq_len=None, emb_dim=H, hidden_dim=H, out_dim=None, encoder=enc, w_edge_attr=0,
                  num_layers=L, bidirectional=1, agg="attn_h", mapper_bias=True, out_wx=False, out_pool_all=0, out_pool="max",
                  dropout=0.0, num_class=num_class).eval()
    seeded_fill(model, seed)
    return model.to(device)


def test_forward_does_not_mutate_the_store(device):
    st = sweep_store(device)
    ids = [3, MID, 8]
    model = _lp_model(device, max_depth=2)
    first = st.batch(ids)
    keep = {k: first[k].clone() for k in ATTRS}
    assert int(keep["node_depth"].max()) > 2
    with torch.no_grad():
        model(first)
    assert not torch.equal(first.node_depth, keep["node_depth"]) and int(first.node_depth.max()) == 2   # the clamp, in place
    assert first.x.dtype != torch.int64 or not torch.equal(first.x, keep["x"])                           # x replaced
    second = st.batch(ids)
    for k in ATTRS:
        assert torch.equal(second[k], keep[k]), k


# ------------------------------------------------------------------ 7. the stored layers
def test_stored_layers(device):
    raw, _ = sweep_graphs()
    st = sweep_store(device)
    b = st.batch(list(range(43)))
    lf, lb, status = engine.topo_layers(b.edge_index, b.batch, 43)
    assert int(status) == 0
    assert torch.equal(st.arrays["layer_f"].long(), lf) and torch.equal(st.arrays["layer_b"].long(), lb)
    assert st.arrays["layer_f"].dtype == torch.int32 and st.arrays["depth_max"].dtype == torch.int32
    want_f, want_b = [], []
    for g in raw:
        ei = prep(g).edge_index.numpy()
        want_f.append(dag_utils.longest_path_layers(ei, g.x.shape[0]))
        want_b.append(dag_utils.longest_path_layers(ei[::-1], g.x.shape[0]))
    assert np.array_equal(st.arrays["layer_f"].cpu().numpy(), np.concatenate(want_f))
    assert np.array_equal(st.arrays["layer_b"].cpu().numpy(), np.concatenate(want_b))
    assert st.arrays["depth_max"].cpu().tolist() == [int(l.max()) for l in want_f]
    cyc = [g.clone() for g in raw[:3]]
    cyc[1].edge_index = torch.cat([cyc[1].edge_index, torch.tensor([[1], [0]])], dim=1)   # 0 -> 1 -> 0
    with pytest.raises(ValueError, match="cycle"):
        GraphStore.from_graphs(cyc, device, sweep_graphs()[1])


def test_pack_in_chunks_equals_pack_at_once(device, monkeypatch):
    from dagnn_amd import store as store_mod
    raw, vocab = sweep_graphs()
    monkeypatch.setattr(store_mod, "PACK_NODE_BUDGET", 100)    # many chunks; the two large graphs get one each
    st = GraphStore.from_graphs(raw, device, vocab)
    for k, v in sweep_store(device).arrays.items():
        assert torch.equal(st.arrays[k], v), k


# ------------------------------------------------------------------ 8. end to end
def _host_batches(raw, chunks, device):
    return [GraphBatch.from_data_list([prep(raw[i]) for i in c]).to(device) for c in chunks]


def test_lp_loops_equal_the_host_path(device):
    raw, _ = sweep_graphs()
    st = sweep_store(device)
    model = _lp_model(device)
    ids = list(range(43))
    chunks = [ids[i:i + 16] for i in range(0, 43, 16)]
    for c in chunks[:2]:
        assert torch.equal(model.predict(st.batch(c)), model.predict(_host_batches(raw, [c], device)[0]))
    got = evaluate_lp(model, st.loader(ids, 16))
    want = evaluate_lp(model, _host_batches(raw, chunks, device))
    assert got == want and got["n"] == 43
    # one training step: forward, the class loss against the batch's targets, backward
    # The two embedding-table gradients are torch's `index_add_` (autograd.EncodeAST.backward): float atomics by default, whose
    # sums differ in the last bits between two runs on the SAME batch (measured: host batch against host batch).  Its
    # deterministic form makes the step repeatable, so that equal inputs must give equal bits.
    model.train()
    res = []
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        for batch in (st.batch(chunks[0]), _host_batches(raw, chunks[:1], device)[0]):
            model.zero_grad(set_to_none=True)
            targ = lp_targets(batch)          # (before the pass, which may rewrite the batch)
            loss = class_cross_entropy(model(batch), targ)
            loss.backward()
            res.append((loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    assert torch.equal(res[0][0], res[1][0]) and torch.isfinite(res[0][0])
    assert sorted(res[0][1]) == sorted(res[1][1]) and len(res[0][1]) > 4
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_evaluate_tok_equals_evaluate_over_host_batches(device):
    raw, vocab = sweep_graphs()
    st = sweep_store(device)
    H = 32
    model = DAGNN(num_vocab=len(vocab), max_seq_len=S, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(H, 98, N_ATTR, 20),
                  w_edge_attr=True, num_layers=2, bidirectional=1, agg="attn_h", out_wx=False, out_pool_all=False, out_pool="max",
                  dropout=0.0).eval()
    seeded_fill(model, 6)
    model = model.to(device)
    ids = [int(i) for i in np.random.default_rng(8).permutation(43)]
    chunks = [ids[i:i + 16] for i in range(0, 43, 16)]
    got = st.evaluate_tok(model, ids, 16)
    want = evaluate.evaluate(model, _host_batches(raw, chunks, device), vocab)
    assert got == want and got["n"] == 43 and set(got) == {"precision", "recall", "F1", "n"}
    assert not model.training
