"""The D-VAE store on the GPU (-m gpu): `dagnn_dag_store_gather` / `dagnn_dag_store_layers` against the reference-generated
fixture, the host collation and the numpy definition; what the entry point may and may not write; no synchronisation; and
the model entry points and loops the store feeds against their list forms.  The store itself has no floating-point
arithmetic: every comparison of a batch is exact.  Passes fed by the store get the SAME tensors as passes fed by lists, so
their results are compared bitwise - except a gradient that two runs of the list path itself do not reproduce bitwise
(float atomics), which is held to 4x that run-to-run difference.  Shapes: 8- and 10-vertex graphs, B up to 257 (graph
slots and nodes cross a workgroup), hidden width 32 / 64, two layers."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from dagnn_amd import DagStore, _lib, dvae, engine, synth
from dagnn_amd.dvae_store import gather_host, layers_host, test_nll as store_test_nll, train_epoch, transpose_masks
from tests import helpers as Hh
from tests.test_dvae_store_cpu import SETS, assert_batch, complete_and_chain, dense_graphs, fixture_rows, host_batch

pytestmark = pytest.mark.gpu
_CACHE = {}
M_SYNTH = 40
BARE, FULL = M_SYNTH, M_SYNTH + 1      # the graphs with the fewest / the most edges, behind the 40 synthetic ones


def sweep_set(name, device):
    """(rows, graphs, y, store) of 40 synthetic rows plus the fixture's two extreme rows (ENAS: no skip, E = 7 < n, and every
    skip, E = 22 > n; BN: the chain, E = 9 < n, and all parentless, E = 16 > n).  Built once; nothing changes them."""
    if name not in _CACHE:
        kind, decode, n, nvt = SETS[name]
        _, _, fx = fixture_rows(name)
        lo, hi = (fx[0], fx[1]) if name == "enas" else (fx[1], fx[0])
        rows = (synth.enas_rows if name == "enas" else synth.bn_rows)(31, M_SYNTH) + [lo, hi]
        y = np.random.default_rng(3).random(len(rows)).astype(np.float32)
        graphs = [decode(r) for r in rows]
        _CACHE[name] = (rows, graphs, y, DagStore.from_rows(rows, kind, nvt, device, y=y))
    return _CACHE[name]


def sweep_lists():
    rng = np.random.default_rng(9)
    draw = lambda k: [int(i) for i in rng.integers(0, M_SYNTH + 2, size=k)]   # noqa: E731
    return {"one": [17], "repeat": [5, 5], "b33": draw(33), "b257": draw(257), "minimal": [BARE] * 40, "maximal": [FULL] * 40}


# ------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("name", sorted(SETS))
def test_fixture_batches(device, name):
    meta, arr, rows = fixture_rows(name)
    kind, _, n, nvt = SETS[name]
    st = DagStore.from_rows(rows, kind, nvt, device)
    for which in meta["lists"]:
        b = st.batch(arr["%s::%s::idx" % (name, which)])
        for k in meta["batch_keys"]:
            w = torch.from_numpy(arr["%s::%s::%s" % (name, which, k)])
            assert b[k].device == device and b[k].dtype == w.dtype and torch.equal(b[k].cpu(), w), (which, k)
        assert np.array_equal(b.types.cpu().numpy(), arr["%s::%s::vs" % (name, which)])


# ------------------------------------------------------------------ 2. the sweep
@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("case", sorted(sweep_lists()))
def test_sweep_equals_host_collation(device, name, case):
    rows, graphs, y, st = sweep_set(name, device)
    n, nvt = SETS[name][2:]
    ids = sweep_lists()[case]
    b = st.batch(ids)
    E, N = b.edge_index.shape[1], len(ids) * n
    if case == "minimal":
        assert E < N
    if case == "maximal":
        assert E > N
    if case == "b257":
        assert N > 2048 and len(ids) + 1 > 256
    assert all(b[k].device == device for k in b.keys if isinstance(b[k], torch.Tensor))
    assert_batch(b, host_batch(graphs, ids, nvt, y), len(ids))


def test_thirty_two_vertices(device):
    types, preds = complete_and_chain()
    st = DagStore.from_dense(types, preds, 3, device)
    graphs = dense_graphs(types, preds, 3)
    for ids in ([0], [1], [1, 0, 0, 1]):
        b = st.batch(ids)
        assert_batch(b, host_batch(graphs, ids, 3), len(ids))
    assert b.edge_index.shape[1] == 2 * 496 + 2 * 31 and int(b.edge_index.max()) == 4 * 32 - 1


# ------------------------------------------------------------------ 3. the raw entry point
PAD = 1                          # every output buffer is one element longer than its extent
SENT_I, SENT_F = -7777777, -12345.0
_OUT = {"out_x": ("x", torch.float32), "out_edge_index": ("edge_index", torch.int64), "out_bi_layer_index": ("bi_layer_index", torch.int64),
        "out_batch": ("batch", torch.int64), "out_ptr": ("ptr", torch.int64), "out_types": ("types", torch.int32),
        "out_preds": ("preds", torch.int32), "out_y": ("y", torch.float32)}
_OPTIONAL = ("out_types", "out_preds", "out_y")


def _raw_call(device, packed, dev_arrays, edge_count, ids, nvt, skip=()):
    want = gather_host(packed, ids, nvt)
    ids = np.asarray(ids, dtype=np.int64)
    B = ids.size
    table = np.zeros((2, B + 1), dtype=np.int64)
    table[0, :B] = ids
    table[1, 1:] = np.cumsum(edge_count[ids])
    table_d = torch.from_numpy(table).to(device)
    a = _lib.DagStoreGatherArgs()
    for k, t in dev_arrays.items():
        setattr(a, k, t.data_ptr())
    a.idx, a.offsets = table_d.data_ptr(), table_d.data_ptr() + 8 * (B + 1)
    a.B, a.n, a.nvt, a.E = B, packed["types"].shape[1], nvt, want["edge_index"].shape[1]
    bufs = {}
    for field, (key, dtype) in _OUT.items():
        if field in skip:
            continue
        bufs[field] = torch.full((want[key].size + PAD,), SENT_F if dtype == torch.float32 else SENT_I, dtype=dtype, device=device)
        setattr(a, field, bufs[field].data_ptr())
    assert _lib.load().dagnn_dag_store_gather(C.byref(a), engine._stream(table_d)) == 0
    torch.cuda.synchronize()
    return want, {k: v.cpu().numpy() for k, v in bufs.items()}


@pytest.mark.parametrize("name", sorted(SETS))
def test_entry_point_writes_its_extents_and_nothing_else(device, name):
    kind, _, n, nvt = SETS[name]
    rows, graphs, y, _ = sweep_set(name, device)
    host = DagStore.from_rows(rows, kind, nvt, "cpu", y=y)
    packed = {k: v.numpy() for k, v in host.arrays.items()}
    dev_arrays = {k: v.to(device) for k, v in host.arrays.items()}
    for ids in ([FULL], [BARE, 7, BARE], sweep_lists()["b33"]):
        want, full = _raw_call(device, packed, dev_arrays, host.edge_count, ids, nvt)
        for field, (key, dtype) in _OUT.items():
            k = want[key].size
            sent = np.float32(SENT_F) if dtype == torch.float32 else SENT_I
            assert np.array_equal(full[field][:k], np.ascontiguousarray(want[key]).reshape(-1)), (ids, field)
            assert not (full[field][:k] == sent).any(), (ids, field)          # every word inside was written
            assert (full[field][k:] == sent).all(), (ids, field)              # and none outside
        _, part = _raw_call(device, packed, dev_arrays, host.edge_count, ids, nvt, skip=_OPTIONAL)
        assert sorted(part) == sorted(set(_OUT) - set(_OPTIONAL))
        for field in part:
            assert np.array_equal(part[field], full[field]), (ids, field)


# ------------------------------------------------------------------ 4. the stored layers
def test_device_layers_equal_the_host_mirror(device):
    rng = np.random.default_rng(12)
    for n, M in ((1, 3), (7, 5), (10, 300), (32, 9)):     # (300 graphs: more than one workgroup)
        preds = np.zeros((M, n), dtype=np.uint32)
        for v in range(1, n):
            preds[:, v] = rng.integers(0, 1 << v, size=M) & rng.integers(0, 1 << v, size=M)
        preds[0] = [(1 << v) - 1 for v in range(n)]
        types = np.full((M, n), 2, dtype=np.int32)
        types[:, 0] = 0
        st = DagStore.from_dense(types, preds.view(np.int32), 3, device)
        lf, lb = layers_host(preds.view(np.int32), transpose_masks(preds))
        assert st.arrays["layer_f"].dtype == torch.int32 and st.arrays["layer_f"].device == device
        assert np.array_equal(st.arrays["layer_f"].cpu().numpy(), lf) and np.array_equal(st.arrays["layer_b"].cpu().numpy(), lb)
        assert lf[0].tolist() == list(range(n))
    for name in sorted(SETS):
        rows, _, _, st = sweep_set(name, device)
        host = DagStore.from_rows(rows, SETS[name][0], SETS[name][3], "cpu")
        for k, v in host.arrays.items():
            assert torch.equal(st.arrays[k].cpu(), v), (name, k)


# ------------------------------------------------------------------ 5. nothing synchronises; batches in flight
class _no_sync(object):
    """Inside, torch raises on every synchronising call (blocking copies, reads of device values)."""

    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")


def _model(kind, agg="attn_h", hs=32, seed=0):
    n, nvt = (8, 8) if kind == "na" else (10, 10)
    return Hh.dvae_decoder_model(kind, max_n=n, nvt=nvt, hs=hs, L=2, nz=8, agg=agg, seed=seed)


def test_batch_and_extract_latent_do_not_synchronise(device):
    rows, graphs, y, st = sweep_set("enas", device)
    model = _model("na").to(device)
    ids = list(range(M_SYNTH + 2))
    want = dvae.extract_latent(model, (st, ids), 16)         # warm-up: the pinned pool, the allocator, derived weights
    for l in sweep_lists().values():
        st.batch(l)
    with _no_sync():
        for l in sweep_lists().values():
            st.batch(l)
        got = dvae.extract_latent(model, (st, ids), 16)
    assert torch.equal(got, want) and tuple(got.shape) == (len(ids), 8)


def test_sixty_four_batches_in_flight(device):
    rows, graphs, y, st = sweep_set("bn", device)
    rng = np.random.default_rng(4)
    G = M_SYNTH + 2
    lists = [[k % G, k // G] + [int(i) for i in rng.integers(0, G, size=int(rng.integers(0, 11)))] for k in range(64)]
    assert len({tuple(l) for l in lists}) == 64
    st.batch(lists[0])
    with _no_sync():
        batches = [st.batch(l) for l in lists]
    for l, b in zip(lists, batches):
        assert_batch(b, host_batch(graphs, l, 10, y), len(l))


# ------------------------------------------------------------------ 6. the model side
CASES = [("na", "attn_h", "enas", 32), ("na", "gated_sum", "enas", 64), ("bn", "attn_h", "bn", 32)]


def test_forward_does_not_change_the_store(device):
    rows, graphs, y, st = sweep_set("bn", device)
    model = _model("bn").to(device)
    keep = {k: v.clone() for k, v in st.arrays.items()}
    ids = [3, FULL, 8, 3]
    first = st.batch(ids)
    before = {k: first[k].clone() for k in first.keys if isinstance(first[k], torch.Tensor)}
    with torch.no_grad():
        model.encode_batch(first)
    assert first.batch.shape[0] == len(ids)                 # the pass replaced `batch` by the read-out rows' ids
    for k, v in keep.items():
        assert torch.equal(st.arrays[k], v), k
    second = st.batch(ids)
    for k, v in before.items():
        assert torch.equal(second[k], v), k


@pytest.mark.parametrize("kind,agg,name,hs", CASES)
def test_encode_batch_and_loss_dense_equal_the_list_forms(device, kind, agg, name, hs):
    rows, graphs, y, st = sweep_set(name, device)
    model = _model(kind, agg, hs).to(device)
    ids = sweep_lists()["b33"]
    G = [graphs[i] for i in ids]
    with torch.no_grad():
        want = model.encode(G)
        b = st.batch(ids)
        types, preds = b.types, b.preds
        got = model.encode_batch(b)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        wl = model.loss(want[0], want[1], G)
        gl = model.loss_dense(got[0], got[1], types, preds)
        for w, g in zip(wl, gl):
            assert torch.equal(w, g) and torch.isfinite(g)
    with pytest.raises(ValueError, match="int32"):
        model.loss_dense(got[0], got[1], types.long(), preds)
    with pytest.raises(ValueError, match="int32"):
        model.loss_dense(got[0][:5], got[1][:5], types, preds)


def _step_list(model, G):
    mu, logvar = model.encode(G)
    return model.loss(mu, logvar, G)


def _step_store(model, st, ids):
    b = st.batch(ids)
    types, preds = b.types, b.preds
    mu, logvar = model.encode_batch(b)
    return model.loss_dense(mu, logvar, types, preds)


def _held(name, got, one, two):
    """`got` against run `one` of the list path: bitwise, or - where its second run `two` differs - within 4x that
    difference."""
    noise = float((one.double() - two.double()).abs().max()) if one.numel() else 0.0
    if noise == 0.0:
        assert torch.equal(got, one), (name, float((got.double() - one.double()).abs().max()))
    else:
        print("not bitwise repeatable on the list path: %s (run-to-run %.3e)" % (name, noise))
        assert float((got.double() - one.double()).abs().max()) <= 4 * noise, (name, noise)


@pytest.mark.parametrize("kind,agg,name,hs", CASES)
def test_training_gradients_equal_the_list_path(device, kind, agg, name, hs):
    rows, graphs, y, st = sweep_set(name, device)
    model = _model(kind, agg, hs).to(device).train()
    ids = sweep_lists()["b33"]
    G = [graphs[i] for i in ids]
    runs = []
    for step in (lambda: _step_list(model, G), lambda: _step_list(model, G), lambda: _step_store(model, st, ids)):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(11)                                # (training mode: reparameterize draws)
        out = step()
        out[0].backward()
        runs.append(([t.detach().clone() for t in out], {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    one, two, got = runs
    for i in range(3):
        assert torch.equal(got[0][i], one[0][i]) and torch.isfinite(got[0][i])
    assert sorted(got[1]) == sorted(one[1]) and len(got[1]) > 8
    for k in one[1]:
        _held(k, got[1][k], one[1][k], two[1][k])


def _epoch_lists(model, opt, graphs, ids, batch_size, clip):
    model.train()
    sums = None
    for i in range(0, len(ids), batch_size):
        G = [graphs[j] for j in ids[i:i + batch_size]]
        opt.zero_grad()
        mu, logvar = model.encode(G)
        loss, recon, kld = model.loss(mu, logvar, G)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
        part = torch.stack([loss.detach().reshape(()), recon.detach().reshape(()), kld.detach().reshape(())])
        sums = part if sums is None else sums + part
        opt.step()
    return tuple(float(v) for v in sums.tolist())


@pytest.mark.parametrize("kind,agg,name,hs", CASES[:2])
def test_train_epoch_equals_three_steps_over_lists(device, kind, agg, name, hs):
    rows, graphs, y, st = sweep_set(name, device)
    base = _model(kind, agg, hs).to(device)
    ids = sweep_lists()["b33"][:20]                          # batches of 8, 8 and 4
    res = []
    for how in ("list", "list", "store"):
        model = copy.deepcopy(base)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        torch.manual_seed(21)
        if how == "list":
            sums = _epoch_lists(model, opt, graphs, ids, 8, 0.25)
        else:
            sums = train_epoch(model, opt, st, ids, 8, clip=0.25)
            assert model.training
        res.append((torch.tensor(sums, dtype=torch.float64), {k: p.detach().clone() for k, p in model.named_parameters()}))
    one, two, got = res
    assert torch.isfinite(got[0]).all() and len(got[0]) == 3
    _held("sums", got[0], one[0], two[0])
    moved = 0
    for k, p in base.named_parameters():
        _held(k, got[1][k], one[1][k], two[1][k])
        moved += int(not torch.equal(got[1][k], p.detach()))
    assert moved > 8
    # the seeded order: the batches of `store.loader(..., shuffle=True, seed)`, one optimizer step each
    perm = torch.randperm(len(ids), generator=torch.Generator().manual_seed(3)).tolist()
    assert perm != sorted(perm)
    sums = []
    for how in ("list", "list", "store"):
        model = copy.deepcopy(base)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        torch.manual_seed(21)
        sums.append(torch.tensor(_epoch_lists(model, opt, graphs, [ids[p] for p in perm], 8, 0.25) if how == "list" else
                                 train_epoch(model, opt, st, ids, 8, clip=0.25, seed=3), dtype=torch.float64))
    _held("sums of the shuffled epoch", sums[2], sums[0], sums[1])
    assert not torch.equal(sums[2], got[0])


@pytest.mark.parametrize("kind,agg,name,hs", CASES)
def test_evaluation_loops_equal_their_list_forms(device, kind, agg, name, hs):
    rows, graphs, y, st = sweep_set(name, device)
    model = _model(kind, agg, hs).to(device).train()
    n = SETS[name][2]
    ids = sweep_lists()["b33"][:21]
    G = [graphs[i] for i in ids]
    # test(): the NLL per graph; the mode is restored
    got = store_test_nll(model, st, ids, 8)
    assert model.training
    model.eval()
    total = None
    with torch.no_grad():
        for i in range(0, len(G), 8):
            mu, logvar = model.encode(G[i:i + 8])
            nll = model.loss(mu, logvar, G[i:i + 8])[1]
            total = nll if total is None else total + nll
    assert got == float(total) / len(ids) and np.isfinite(got)
    assert store_test_nll(model, st, ids, 8) == got and not model.training
    # extract_latent
    mu = dvae.extract_latent(model, (st, ids), 8)
    assert torch.equal(mu, dvae.extract_latent(model, G, 8)) and tuple(mu.shape) == (21, 8)
    assert torch.equal(dvae.extract_latent(model, (st, np.array(ids)), 64), dvae.extract_latent(model, G, 64))
    # recon_accuracy under fixed draws
    E, D = 2, 3
    torch.manual_seed(5)
    draws = dvae._take_draws(None, n, len(ids), E * D, device, "")
    for batch in (None, 8):
        a = dvae.recon_accuracy(model, (st, ids), E, D, draws=draws, batch_size=batch)
        b = dvae.recon_accuracy(model, G, E, D, draws=draws, batch_size=batch)
        assert a[:2] == b[:2] and a[1] == len(ids) * E * D and torch.equal(a[2], b[2])
    with pytest.raises(ValueError):
        dvae.recon_accuracy(model, (st, []), E, D)


@pytest.mark.parametrize("name,kind", [("enas", "ENAS"), ("bn", "BN")])
def test_prior_validity_with_the_store_graph_set(device, name, kind):
    rows, graphs, y, st = sweep_set(name, device)
    n, nvt = SETS[name][2:]
    model = _model("na" if name == "enas" else "bn").to(device)
    P, D = 40, 4
    z = torch.from_numpy(np.random.default_rng(9).standard_normal((P, 8)).astype(np.float32)).to(device)
    torch.manual_seed(31)
    draws = dvae._take_draws(None, n, P, D, device, "")
    a = st.graph_set()
    b = dvae.GraphSet.from_graphs(graphs, n, nvt, device)
    assert len(a) == len(b) == M_SYNTH + 2 and a.distinct() == b.distinct()
    got = dvae.prior_validity(model, a, decode_times=D, data_type=kind, z=z, draws=draws)
    want = dvae.prior_validity(model, b, decode_times=D, data_type=kind, z=z, draws=draws)
    assert got == want and got.n_total == P * D
