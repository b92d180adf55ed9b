"""The ogbg-code2 training epoch, CPU tier (-m "not gpu"): the numpy mirrors of the STEP kernels of csrc/loss.hip, `EpochMeter`,
the host route of `seq_ce_step` / `class_ce_step`, `GraphStore.train_tok` / `train_lp` on a CPU store with a small torch model,
against torch's own operations and against fixtures generated from the reference's `train()` loop bodies
(tests/golden/make_golden_code2_train.py).  Integer results and the float64 epoch sum are compared exactly."""
import json

import numpy as np
import pytest
import torch

import dagnn_amd
from dagnn_amd import EpochMeter, GraphData, GraphStore, _lib, lp, train
from dagnn_amd.evaluate import encode_ref_sets, f1_counts_host, f1_from_counts
from dagnn_amd.lp import class_hits_host
from dagnn_amd.train import ClipAdam, seq_ce_step, seq_ce_step_host
from tests import helpers as Hh

TOK, LP = "code2_train_tok_h32", "code2_train_lp_gated_h64"
EINVAL, ENOSPC = -22, -28
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ shared with tests/test_code2_train_gpu.py
def _json(a):
    return json.loads(bytes(a).decode())


def fixture_raw(name):
    """(meta, arr, raw graphs, vocab2idx or None): the fixture's three batches split back into RAW graphs - AST edges only,
    the leaves attributed - as `GraphStore.from_graphs` takes them, with `y_arr` and (TOK) the label words."""
    meta, arr = Hh.load(name)
    tok = meta["kind"] == "code2_train_tok"
    seq_ref = _json(arr["seq_ref"]) if tok else None
    vocab = {w: i for i, w in enumerate(_json(arr["idx2vocab"]))} if tok else None
    raw = []
    for s in range(meta["steps"]):
        x, depth, ei, ea, batch = (torch.from_numpy(arr["s%d::%s" % (s, k)].copy()) for k in ("x", "node_depth", "edge_index", "edge_attr", "batch"))
        for b in range(meta["B"]):
            nodes = torch.nonzero(batch == b).view(-1)
            v0, n = int(nodes[0]), nodes.numel()
            ast = ei[:, (ea[:, 0] == 0) & (batch[ei[0]] == b)] - v0
            leaf = torch.ones(n, dtype=torch.long)
            leaf[ast[0]] = 0
            g = len(raw)
            d = GraphData(x=x[v0:v0 + n], node_depth=depth[v0:v0 + n], edge_index=ast.contiguous(), node_is_attributed=leaf.view(-1, 1),
                          y_arr=torch.from_numpy(arr["y_arr"][g:g + 1].copy()) if tok else torch.zeros(1, 1, dtype=torch.long))
            if tok:
                d.y = seq_ref[g]
            raw.append(d)
    return meta, arr, raw, vocab


def fixture_store(name, device):
    meta, arr, raw, vocab = fixture_raw(name)
    return meta, arr, GraphStore.from_graphs(raw, device, vocab)


def assert_fixture_batches(meta, arr, store):
    """The store's batches of 12 in order ARE the batches the reference ran on."""
    B = meta["B"]
    for s in range(meta["steps"]):
        b = store.batch(np.arange(s * B, (s + 1) * B))
        for k, attr in (("x", "x"), ("node_depth", "node_depth"), ("edge_index", "edge_index"), ("edge_attr", "edge_attr"),
                        ("batch", "batch"), ("layer0", "_bi_layer_idx0"), ("layer1", "_bi_layer_idx1")):
            assert torch.equal(b[attr].cpu(), torch.from_numpy(arr["s%d::%s" % (s, k)])), (s, k)
        if meta["kind"] == "code2_train_lp":
            assert torch.equal(b.len_longest_path.cpu(), torch.from_numpy(arr["len_longest_path"][s * B:(s + 1) * B]))
        else:
            assert torch.equal(b.y_arr.cpu(), torch.from_numpy(arr["y_arr"][s * B:(s + 1) * B]))


def special_rows(x, V, finite=False):
    """Rows of `x` [rows, V] overwritten, as far as there are rows and columns, with the cases the argmax order is about.
    Returns {case: row}.  `finite` leaves out the NaN and the -inf row, whose losses are not finite (the sum over the rows
    can then be compared as a number)."""
    rows, done = x.shape[0], {}
    g = torch.Generator().manual_seed(1000 * rows + V)
    r = iter(range(rows - 1, -1, -1))   # from the back: row 0 stays random (or gets EOS from the caller)

    def take(name, ok=True):
        if not ok:
            return None
        i = next(r, None)
        if i is not None:
            done[name] = i
        return i

    i = take("tie", V >= 2)
    if i is not None:
        lo, hi = (3, 3 + 64 * min((V - 4) // 64, 3)) if V >= 68 else (V // 3, V - 1)   # columns of different waves when V allows
        x[i] = torch.randn(V, generator=g).clamp(max=1.0)
        x[i, lo] = x[i, hi] = 2.5
        done["tie_cols"] = (lo, hi)
    i = take("nan", V >= 2 and not finite)
    if i is not None:
        x[i, V // 2] = NAN
        x[i, 0] = 50.0
    i = take("one_finite", V >= 2 and not finite)
    if i is not None:
        x[i] = -INF
        x[i, V - 2] = -3.0
    i = take("zeros", V >= 5)
    if i is not None:
        x[i] = -torch.rand(V, generator=g) - 0.5
        x[i, 1], x[i, 4] = -0.0, 0.0
    return done


# ------------------------------------------------------------------ 1. names, ABI
def test_public_names():
    for k in ("EpochMeter", "seq_ce_step", "class_ce_step"):
        assert hasattr(dagnn_amd, k), k
    assert {"class_ce_step", "class_ce_step_host"} <= set(lp.__all__)
    for k in ("train_tok", "train_lp"):
        assert callable(getattr(GraphStore, k))
    assert callable(train.seq_ce_step_host)


def test_library_exports_the_step_symbols():
    lib = _lib.load()
    for name in ("dagnn_seq_ce_step", "dagnn_class_ce_step"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call below fails validation, so the made-up (aligned, non-NULL) addresses are never touched."""
    lib = _lib.load()
    P = 4096

    def seq(**kw):
        a = dict(logits=P, ld=35, y=P, B=3, S=5, V=7, dl=P, ld_d=36, row=P, loss=P, tok=P, eos=6, ref=P, R=2, extra=P, counts=P,
                 rows=10, off=0, esum=P, esteps=P, counter=P)
        a.update(kw)
        return lib.dagnn_seq_ce_step(a["logits"], a["ld"], a["y"], a["B"], a["S"], a["V"], a["dl"], a["ld_d"], a["row"], a["loss"],
                                     a["tok"], a["eos"], a["ref"], a["R"], a["extra"], a["counts"], a["rows"], a["off"], a["esum"],
                                     a["esteps"], a["counter"], None)

    for bad in (dict(logits=None), dict(y=None), dict(row=None), dict(loss=None), dict(counter=None), dict(B=0), dict(S=0), dict(V=0),
                dict(ld=34), dict(ld_d=34), dict(tok=None), dict(esum=None), dict(esteps=None), dict(esum=P + 4), dict(R=0),
                dict(off=-1), dict(counts=None), dict(counts=P + 8), dict(ref=None, R=0), dict(ref=None, off=-1)):
        assert seq(**bad) == EINVAL, bad
    for bad in (dict(off=8), dict(rows=2), dict(off=11)):      # 3 graphs from row 8 of 10; of 2 rows; behind the table
        assert seq(**bad) == ENOSPC, bad

    def cls(**kw):
        a = dict(logits=P, ld=9, targ=P, kind=_lib.LP_FLOAT32, B=4, C=9, dl=P, ld_d=12, row=P, loss=P, tok=P, hits=P, esum=P, esteps=P,
                 counter=P)
        a.update(kw)
        return lib.dagnn_class_ce_step(a["logits"], a["ld"], a["targ"], a["kind"], a["B"], a["C"], a["dl"], a["ld_d"], a["row"],
                                       a["loss"], a["tok"], a["hits"], a["esum"], a["esteps"], a["counter"], None)

    for bad in (dict(logits=None), dict(targ=None), dict(kind=7), dict(B=0), dict(C=0), dict(ld=8), dict(ld_d=8), dict(tok=None),
                dict(hits=None), dict(hits=P + 4), dict(esum=None), dict(esteps=None), dict(counter=None), dict(row=None), dict(loss=None)):
        assert cls(**bad) == EINVAL, bad


# ------------------------------------------------------------------ 2. the mirrors
@pytest.mark.parametrize("B,S,V", [(1, 1, 1), (1, 5, 7), (3, 5, 255), (4, 2, 300)])
def test_seq_mirror_against_torch(B, S, V):
    g = torch.Generator().manual_seed(B * 1000 + V)
    x = torch.randn(B * S, V, generator=g)
    cases = special_rows(x, V)
    x = x.view(B, S, V)
    y = torch.randint(0, V, (B, S), generator=g)
    eos = V - 1
    ref_ids = torch.randint(-1, V, (B, 3), generator=g).to(torch.int32)
    ref_extra = torch.randint(0, 3, (B,), generator=g).to(torch.int32)
    out = seq_ce_step_host(x.reshape(B, S * V), y, eos, ref_ids, ref_extra, epoch_sum=1.25)
    assert np.array_equal(out["tok"], torch.argmax(x, dim=2).numpy())          # torch's CPU argmax IS the stated order
    if "tie" in cases:
        assert out["tok"].reshape(-1)[cases["tie"]] == cases["tie_cols"][0]
    if "nan" in cases:
        assert out["tok"].reshape(-1)[cases["nan"]] == V // 2
    if "zeros" in cases:
        assert out["tok"].reshape(-1)[cases["zeros"]] == 1
    assert np.array_equal(out["counts"], f1_counts_host(out["tok"], eos, ref_ids, ref_extra)) and out["counts"].dtype == np.int32
    want_rows = torch.nn.functional.cross_entropy(x.double().view(B * S, V), y.view(-1), reduction="none").numpy()
    fin = np.isfinite(want_rows)
    assert np.array_equal(fin, np.isfinite(out["row_loss"]))
    assert np.allclose(out["row_loss"][fin], want_rows[fin], rtol=1e-6, atol=1e-6)
    acc = np.float32(0)
    for v in out["row_loss"]:
        acc = np.float32(acc + v)
    assert out["loss"].dtype == np.float32 and (out["loss"] == np.float32(acc / np.float32(B * S)) or np.isnan(acc))
    if np.isfinite(out["loss"]):
        want = sum(torch.nn.functional.cross_entropy(x[:, i], y[:, i]) for i in range(S)) / S
        assert abs(float(out["loss"]) - float(want)) <= 4e-6 * max(1.0, abs(float(want)))
        assert out["epoch_sum"] == 1.25 + float(out["loss"])
    # a target outside [0, V) makes its row, and the loss, NaN
    y2 = y.clone()
    y2[0, 0] = V
    o2 = seq_ce_step_host(x, y2, eos)
    assert np.isnan(o2["row_loss"][0]) and np.isnan(o2["loss"]) and o2["counts"] is None


def test_class_mirror_against_torch_and_class_hits_host():
    g = torch.Generator().manual_seed(5)
    B, Cn = 9, 24
    x = torch.randn(B, Cn, generator=g)
    targ = torch.tensor([3.0, 3.5, NAN, 0.0, 23.0, 7.9, 1.0, 2.0, 5.0])
    x[3, 0] = 9.0   # a sure hit: target 0
    out = lp.class_ce_step_host(x, targ, epoch_hits=(2, 5), epoch_sum=0.5)
    assert np.array_equal(out["tok"], torch.argmax(x, dim=1).numpy())
    assert np.array_equal(out["hits"], np.array([2, 5]) + class_hits_host(x, targ))
    assert np.array_equal(class_hits_host(x, targ), class_hits_host(torch.from_numpy(out["tok"]), targ))
    assert np.isnan(out["row_loss"][2]) and np.isnan(out["loss"])               # the NaN target
    ok = torch.tensor([0, 1, 3, 4, 5, 6, 7, 8])
    o2 = lp.class_ce_step_host(x[ok], targ[ok])
    want = torch.nn.functional.cross_entropy(x[ok], targ[ok].to(torch.long))     # 3.5 -> 3, 7.9 -> 7: truncation
    assert abs(float(o2["loss"]) - float(want)) <= 4e-6 * float(want) and o2["epoch_sum"] == float(o2["loss"])
    o3 = lp.class_ce_step_host(x[ok], targ[ok].to(torch.long))
    assert o3["loss"] == o2["loss"] and int(o3["hits"][1]) == 8


# ------------------------------------------------------------------ 3. the fixtures' own numbers
def test_tok_fixture_f1_from_the_stored_tokens_exactly():
    meta, arr, raw, vocab = fixture_raw(TOK)
    assert meta["ambiguous"] == 0 and all(float(arr["s%d::margin" % s].min()) > meta["tau"] for s in range(3))
    tok = np.concatenate([arr["s%d::tok" % s] for s in range(3)])
    ref_ids, ref_extra = encode_ref_sets(_json(arr["seq_ref"]), vocab)
    got = f1_from_counts(f1_counts_host(tok, len(vocab) - 1, ref_ids, ref_extra))
    assert [got["precision"], got["recall"], got["F1"]] == arr["f1"].tolist() and got["n"] == 36
    assert 0 < got["F1"] < 1
    assert meta["mean_loss"] == sum(float(v) for v in arr["loss"]) / 3
    assert np.array_equal(arr["loss_err_ref"], np.abs(arr["loss"] - arr["loss64"]))


def test_lp_fixture_acc_from_the_stored_tokens_exactly():
    meta, arr = Hh.load(LP)
    assert meta["ambiguous"] == 0 and all(float(arr["s%d::margin" % s].min()) > meta["tau"] for s in range(3))
    tok = np.concatenate([arr["s%d::tok" % s] for s in range(3)])
    hits, labelled = class_hits_host(torch.from_numpy(tok), arr["len_longest_path"])
    assert float(hits) / labelled == float(arr["acc"]) and labelled == 36 and hits > 0
    assert meta["mean_loss"] == sum(float(v) for v in arr["loss"]) / 3


@pytest.mark.parametrize("name", [TOK, LP])
def test_a_cpu_store_of_the_fixture_graphs_gives_the_fixture_batches(name):
    meta, arr, store = fixture_store(name, "cpu")
    assert store.num_graphs == 36
    assert_fixture_batches(meta, arr, store)


# ------------------------------------------------------------------ 4. the meter
def test_epoch_meter_tok_and_lp():
    m = EpochMeter("cpu", 5, eos_id=6)
    assert m.counts.shape == (5, 4) and m.counts.dtype == torch.int32 and m.loss_sum.dtype == torch.float64 and m.steps.dtype == torch.int64
    x = torch.randn(3, 5 * 7, generator=torch.Generator().manual_seed(1))
    y = torch.randint(0, 7, (3, 5), generator=torch.Generator().manual_seed(2))
    ref_ids, ref_extra = torch.tensor([[1, 2], [-1, -1], [3, 3]], dtype=torch.int32), torch.tensor([0, 2, 0], dtype=torch.int32)
    pl = [x[:, i * 7:(i + 1) * 7].clone().requires_grad_() for i in range(5)]
    loss = seq_ce_step(pl, y, m, ref_ids, ref_extra)
    loss.backward()
    assert all(p.grad is not None for p in pl)
    host = seq_ce_step_host(x, y, 6, ref_ids, ref_extra)
    assert torch.equal(m.tok, torch.from_numpy(host["tok"])) and np.array_equal(m.counts[:3].numpy(), host["counts"])
    assert m.graphs == 3 and int(m.steps) == 1 and float(m.loss_sum) == float(loss.detach())
    mean, metric = m.result(2)
    assert mean == float(loss.detach()) / 2 and metric == f1_from_counts(host["counts"])
    with pytest.raises(ValueError, match="do not fit"):
        seq_ce_step(pl, y, m, ref_ids, ref_extra)                                # 3 + 3 > 5
    assert m.graphs == 3 and int(m.steps) == 1                                   # ... refused before anything was added
    seq_ce_step(pl, y, m)                                                        # without label sets: loss and tokens only
    assert m.graphs == 3 and int(m.steps) == 2
    m.reset()
    assert m.graphs == 0 and int(m.steps) == 0 and float(m.loss_sum) == 0 and not m.counts.any() and m.tok is None
    with pytest.raises(ValueError, match="no graph"):
        m.result(1)
    with pytest.raises(ValueError):
        seq_ce_step(pl, y, m, ref_ids, None)
    with pytest.raises(ValueError, match="LP meter"):
        seq_ce_step(pl, y, EpochMeter("cpu", 5))
    q = EpochMeter("cpu", 0)
    with pytest.raises(ValueError, match="TOK meter"):
        lp.class_ce_step(torch.randn(2, 3), torch.tensor([0, 1]), m)
    pred = torch.randn(4, 9, generator=torch.Generator().manual_seed(3)).requires_grad_()
    targ = torch.tensor([1.0, 8.0, 3.5, 2.0])
    l2 = lp.class_ce_step(pred, targ, q)
    l2.backward()
    host = lp.class_ce_step_host(pred, targ)
    assert torch.equal(q.tok, torch.from_numpy(host["tok"])) and q.hits.tolist() == host["hits"].tolist()
    mean, metric = q.result(1)
    assert mean == float(l2) and metric == {"acc": float(host["hits"][0]) / 4, "n": 4}
    with pytest.raises(ValueError, match="no labelled"):
        EpochMeter("cpu", 0).result(1)


# ------------------------------------------------------------------ 5. the epoch on a CPU store
class _TinyTok(torch.nn.Module):
    """A stand-in model for the host route: per graph the sum of an embedding of the node types, S heads side by side."""

    def __init__(self, S, V, seed):
        super().__init__()
        self.S, self.V = S, V
        self.emb = torch.nn.Embedding(98, 8)
        self.lin = torch.nn.Linear(8, max(S, 1) * V)   # (S = 0: one [B, V] head, the LP model's output)
        from oracle.seeding import seeded_fill
        seeded_fill(self, seed)

    def forward(self, batch):
        B = batch.num_graphs
        pooled = torch.zeros(B, 8).index_add_(0, batch.batch, self.emb(batch.x[:, 0]))
        out = self.lin(torch.tanh(pooled))
        return [out[:, i * self.V:(i + 1) * self.V] for i in range(self.S)] if self.S else out


def _hand_loop_tok(store, model, opt, ids, bs, clip):
    from dagnn_amd.evaluate import SeqF1, rows_argmax
    model.train()
    metric, accum, chunks = SeqF1(store.eos_id), 0, 0
    for i in range(0, len(ids), bs):
        chunks += 1
        chunk = ids[i:i + bs]
        if len(chunk) == 1:
            continue
        batch = store.batch(chunk)
        y_arr, ref_ids, ref_extra = batch.y_arr, batch.ref_ids, batch.ref_extra
        pred_list = model(batch)
        opt.zero_grad()
        loss = train.seq_cross_entropy(pred_list, y_arr)
        loss.backward()
        if clip > 0:
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
        opt.step()
        accum += float(loss.detach())
        metric.update(rows_argmax([p.detach() for p in pred_list]), ref_ids, ref_extra)
    return accum / chunks, metric.compute()


def test_train_tok_on_a_cpu_store_divides_by_every_chunk():
    meta, arr, store = fixture_store(TOK, "cpu")
    ids = list(range(36)) + [4]                       # chunks of 12, 12, 12 and ONE graph: the last one is skipped, and counted
    a, b = _TinyTok(meta["S"], meta["V"], 3), _TinyTok(meta["S"], meta["V"], 3)
    oa, ob = torch.optim.Adam(a.parameters(), lr=1e-2), torch.optim.Adam(b.parameters(), lr=1e-2)
    got = store.train_tok(a, oa, ids, 12, clip=0.25)
    want = _hand_loop_tok(store, b, ob, ids, 12, 0.25)
    assert got == want and got[1]["n"] == 36 and a.training
    assert got[0] != want[0] * 4 / 3                   # (the divisor is 4, not the 3 steps that ran)
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    # a shuffled epoch visits the loader's order
    c = _TinyTok(meta["S"], meta["V"], 3)
    res = store.train_tok(c, torch.optim.Adam(c.parameters(), lr=1e-2), ids, 12, seed=5)
    assert res[1]["n"] == 36 and res != got


def test_train_lp_on_a_cpu_store():
    meta, arr, store = fixture_store(LP, "cpu")
    ids = list(range(36)) + [4]
    a, b = _TinyTok(0, meta["num_class"], 4), _TinyTok(0, meta["num_class"], 4)
    oa, ob = torch.optim.SGD(a.parameters(), lr=0.1), torch.optim.SGD(b.parameters(), lr=0.1)
    got = store.train_lp(a, oa, ids, 12)
    metric, accum = lp.ClassAccuracy(), 0
    b.train()
    for i in range(0, 36, 12):
        batch = store.batch(ids[i:i + 12])
        targ = batch.len_longest_path
        pred = b(batch)
        ob.zero_grad()
        loss = lp.class_cross_entropy(pred, targ)
        loss.backward()
        ob.step()
        accum += float(loss.detach())
        metric.update(pred.detach(), targ)
    assert got == (accum / 4, metric.compute())
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)


def test_train_epoch_value_errors():
    meta, arr, raw, vocab = fixture_raw(TOK)
    model = _TinyTok(meta["S"], meta["V"], 1)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    no_y = [GraphData(x=g.x, node_depth=g.node_depth, edge_index=g.edge_index, node_is_attributed=g.node_is_attributed) for g in raw[:4]]
    st = GraphStore.from_graphs(no_y, "cpu")
    with pytest.raises(ValueError, match="y_arr"):
        st.train_tok(model, opt, [0, 1, 2], 2)
    with pytest.raises(ValueError, match="y_arr"):
        st.train_lp(model, opt, [0, 1, 2], 2)
    no_words = [GraphData(x=g.x, node_depth=g.node_depth, edge_index=g.edge_index, node_is_attributed=g.node_is_attributed, y_arr=g.y_arr)
                for g in raw[:4]]
    with pytest.raises(ValueError, match="label words"):
        GraphStore.from_graphs(no_words, "cpu").train_tok(model, opt, [0, 1, 2], 2)
    store = GraphStore.from_graphs(raw[:4], "cpu", vocab)
    clip_adam = ClipAdam(model.parameters(), max_norm=0.25)
    with pytest.raises(ValueError, match="max_norm"):
        store.train_tok(model, clip_adam, [0, 1, 2], 2, clip=0.25)
    with pytest.raises(ValueError, match="max_norm"):
        store.train_lp(model, clip_adam, [0, 1, 2], 2, clip=0.25)
    with pytest.raises(ValueError, match="batch_size"):
        store.train_tok(model, opt, [0, 1, 2], 0)
    with pytest.raises(ValueError):
        store.train_tok(model, opt, [0, 99], 2)
    assert "max_norm" in GraphStore.train_tok.__doc__
