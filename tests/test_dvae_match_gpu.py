"""The D-VAE evaluation metrics on the GPU (csrc/dvae_match.hip): each kernel against the `dvae_match_*` fixtures of the
reference's own dvae/util.py and against the host mirrors on larger seeded rows, and `recon_accuracy` / `prior_validity`
end to end against `decode_dense` under the same draws followed by the host mirrors."""
from __future__ import annotations

import warnings

import numpy as np
import pytest
import torch

from dagnn_amd import _lib, dvae, engine, synth
from tests import helpers as Hh
from tests.test_dvae_match_cpu import FIXTURES, fixture_rows, host_metrics

pytestmark = pytest.mark.gpu

E2E = [("dvae_decode_na_h64_L2_sample", "ENAS"), ("dvae_gated_decode_na_h64_L2_sample", "ENAS"),
       ("dvae_decode_bn_h32_L3_sample", "BN")]


def _model(name, device):
    meta, _ = Hh.load(name)
    model, _ = Hh.dvae_model(meta)
    return model.to(device).eval()


def _t(x, device):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _dense(rows, device, keys=("types", "preds", "nv")):
    return tuple(_t(rows[k], device) for k in keys)


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


@pytest.mark.parametrize("name", FIXTURES)
def test_kernels_match_the_reference_fixtures(device, name):
    meta, rows, same, valid, in_train = fixture_rows(name)
    kind, n, nvt, A, B = meta["kind"], meta["n"], meta["nvt"], meta["A"], meta["B"]
    d = dvae.DecodedDense(*_dense(rows, device), None)
    res = dvae.same_dag_dense(d, *_dense(rows, device, ("types_true", "preds_true", "nv_true")))
    np.testing.assert_array_equal(res.same.cpu().numpy().astype(bool), same)
    assert res.per_graph.tolist() == meta["per_graph"] and res.total.tolist() == [meta["n_same"]]
    train = dvae.GraphSet.from_dense(*_dense(rows, device, ("types_train", "preds_train", "nv_train")))
    assert len(train) == meta["n_train"] and train.distinct() == meta["train_distinct"]
    member, count = train.contains(d)
    np.testing.assert_array_equal(member.cpu().numpy().astype(bool), in_train)
    assert count.tolist() == [int(in_train.sum())]
    sel = dvae.select_decoded(d, kind, nvt, 0, 1)
    np.testing.assert_array_equal(sel.valid.cpu().numpy().astype(bool), valid)
    member, count = train.contains(d, sel.valid)
    np.testing.assert_array_equal(member.cpu().numpy().astype(bool), in_train & valid)
    assert count.tolist() == [meta["n_in_train"]]
    for chunks in (1, 4):
        keys = dvae.DistinctKeys(sel.keys.shape[2], A * B, device)
        for a in np.array_split(np.arange(A), chunks):
            a = torch.from_numpy(a).to(device)
            keys.add(sel.keys[:, a].contiguous(), sel.valid[a].contiguous())
        assert keys.count() == meta["n_unique"]
    assert train.status().tolist()[1] == 0


@pytest.mark.parametrize("kind,n,nvt,A,B,N", [("ENAS", 8, 8, 2048, 64, 200000), ("BN", 10, 10, 1024, 128, 200000),
                                              ("ENAS", 32, 64, 64, 96, 50000), ("BN", 32, 30, 48, 64, 20000)])
def test_large_inputs_match_the_host_mirrors(device, kind, n, nvt, A, B, N):
    """A x B up to 2^17 decoded rows against N training rows: the set holds far more rows than slots per hash value, so
    probes meet foreign rows all the time and only the full compare tells them apart."""
    rows = synth.match_rows(900 + n + nvt, kind, 40, 60, n, nvt, 600)
    rng = np.random.default_rng(N + n)
    pick = rng.integers(0, 40 * 60, size=A * B)
    dense = [rows[k].reshape((2400,) + rows[k].shape[2:])[pick].reshape((A, B) + rows[k].shape[2:]) for k in ("types", "preds", "nv")]
    # the training set: the 600 prepared rows, then rows of other seeds with one random edge bit flipped each (near-duplicates)
    other = synth.decoded_rows(17 + n, kind, 1, 4000, n, nvt)
    src = rng.integers(0, 4000, size=N - 600)
    tt, tp, tk = other[0][0][src].copy(), other[1][0][src].copy(), other[2][0][src].copy()
    v = np.minimum(rng.integers(1, n, size=N - 600), np.maximum(tk - 1, 1))
    tp[np.arange(N - 600), v] ^= (1 << rng.integers(0, np.maximum(v, 1))).astype(np.int32)
    train_rows = [np.concatenate([rows["types_train"], tt]), np.concatenate([rows["preds_train"], tp]),
                  np.concatenate([rows["nv_train"], tk])]
    host_set = dvae.GraphSet.from_dense(*train_rows)
    dev_set = dvae.GraphSet.from_dense(*(_t(x, device) for x in train_rows))
    assert len(dev_set) == N and dev_set.distinct() == host_set.distinct()
    d = dvae.DecodedDense(*(_t(x, device) for x in dense), None)
    sel = dvae.select_decoded(d, kind, nvt, 0, 1)
    valid = sel.valid.cpu().numpy()
    for mask, hmask in ((None, None), (sel.valid, valid)):
        member, count = dev_set.contains(d, mask)
        hmember, hcount = host_set.contains(tuple(dense), hmask)
        np.testing.assert_array_equal(member.cpu().numpy(), hmember.numpy())
        assert count.tolist() == hcount.tolist()
    # queries that differ from a stored row in exactly one bit, and the stored rows themselves
    q = [x[:4096].copy() for x in train_rows]
    q[1][np.arange(4096), 1] ^= 1
    member, count = dev_set.contains(tuple(_t(x, device) for x in q))
    hmember, hcount = host_set.contains(tuple(q))
    np.testing.assert_array_equal(member.cpu().numpy(), hmember.numpy())
    assert dev_set.contains(tuple(_t(x[:4096], device) for x in train_rows))[1].tolist() == [4096]
    tb = rng.integers(0, 60, size=B)
    true = [rows[k][tb] for k in ("types_true", "preds_true", "nv_true")]
    res = dvae.same_dag_dense(d, *(_t(x, device) for x in true))
    same, per, total = dvae.same_dag_host(*dense, *true)
    np.testing.assert_array_equal(res.same.cpu().numpy().astype(bool), same)
    assert res.per_graph.tolist() == per.tolist() and res.total.tolist() == [total]
    # distinct keys: one call, and accumulated over chunks of attempts
    hk = sel.keys.cpu().numpy()
    want = len({tuple(hk[b, a]) for a, b in zip(*np.nonzero(valid))})
    for chunks in (1, 7):
        keys = dvae.DistinctKeys(sel.keys.shape[2], A * B, device)
        for a in np.array_split(np.arange(A), chunks):
            a = torch.from_numpy(a).to(device)
            keys.add(sel.keys[:, a].contiguous(), sel.valid[a].contiguous())
        assert keys.count() == want
    assert dev_set.status().tolist()[1] == 0


def test_heavy_duplicates_and_nv_none(device):
    """One graph 100 000 times, then 1 000 graphs 100 times each: every insert but the first meets its own record."""
    rows = synth.decoded_rows(5, "ENAS", 1, 1000, 8, 8)
    types, preds, nv = (np.ascontiguousarray(x[0]) for x in rows)
    rep = [np.concatenate([np.repeat(x[:1], 100000, 0), np.tile(x, (100,) + (1,) * (x.ndim - 1))]) for x in (types, preds, nv)]
    gs = dvae.GraphSet.from_dense(*(_t(x, device) for x in rep))
    host = dvae.GraphSet.from_dense(types, preds, nv)
    assert len(gs) == 200000 and gs.distinct() == host.distinct()
    assert gs.contains(tuple(_t(x, device) for x in (types, preds, nv)))[1].tolist() == [1000]
    full = dvae.GraphSet.from_dense(_t(types, device), _t(preds, device))   # nv None: all 8 entries take part
    hfull = dvae.GraphSet.from_dense(types, preds)
    assert full.distinct() == hfull.distinct()
    m, c = full.contains((_t(types, device), _t(preds, device), _t(np.full(1000, 8, np.int32), device)))
    assert c.tolist() == [1000]


def _graph_of_row(types, preds, nv, nvt):
    k = int(nv)
    adj = np.zeros((k, k))
    for v in range(k):
        for u in range(v):
            if int(preds[v]) >> u & 1:
                adj[u, v] = 1
    return synth._adj_to_graph(adj, [int(x) for x in types[:k]], nvt)


class _ReconCase(object):
    """Graphs that their own decodes reproduce, by construction.  The latent rows are fixed (model.encode is replaced
    by a lookup of chosen mu rows), all E * D attempts are decoded in ONE call per batch under given draws, and graph b IS the
    decode of attempt a_b = (3 b) mod (E D - 5) of row b.  In column b the draws of attempt a_b are repeated in the
    next b mod 5 attempts, so graph b is reproduced at least 1 + b mod 5 times.  `want` counts, on the host, the
    attempts of that one call that are is_same_DAG to graph b - a route that shares no slicing with recon_accuracy."""

    def __init__(self, model, device, N, E, D, seed, batch=None):
        n, nvt = model.max_n, model.nvt
        self.model, self.N = model, N
        rng = np.random.default_rng(seed)
        self.mu = _t(rng.standard_normal((N, 56)).astype(np.float32), device)
        self.logvar = torch.full((N, 56), -2.0, device=device)
        st, se = dvae.draw_shapes(n, N, E * D)
        torch.manual_seed(seed)
        u = torch.rand(int(np.prod(st)) + int(np.prod(se)), device=device)
        u_type, u_edge = u[:int(np.prod(st))].view(st).clone(), u[int(np.prod(st)):].view(se).clone()
        self.at = [(3 * b) % (E * D - 5) for b in range(N)]
        for b, a in enumerate(self.at):
            for j in range(1, 1 + b % 5):
                u_type[a + j, :, b], u_edge[a + j, :, b] = u_type[a, :, b], u_edge[a, :, b]
        self.draws = (u_type, u_edge)
        # the attn_h decoders couple the rows of one decode call (the reference's padded soft-max gives the padding
        # weight, and the padding width is the call's largest predecessor count), so a graph is defined by a decode
        # among the rows recon_accuracy will decode it with: one call per batch of graphs
        step = N if batch is None else batch
        parts = [model.decode_dense(self.mu[g0:g0 + step], True, E * D,
                                    (u_type[:, :, g0:g0 + step], u_edge[:, :, g0:g0 + step])) for g0 in range(0, N, step)]
        self.rows = [torch.cat([getattr(q, f) for q in parts], 1).cpu().numpy() for f in ("types", "preds", "nv")]
        t, p, k = self.rows
        self.G = [_graph_of_row(t[a, b], p[a, b], k[a, b], nvt) for b, a in enumerate(self.at)]
        self.index = {id(g): b for b, g in enumerate(self.G)}
        self.want = self.count(self.G, self.rows)

    def count(self, G, rows):
        tt, pt, nt = dvae.dense_rows(G, self.model.max_n, self.model.nvt)
        return dvae.same_dag_host(*rows, tt, pt, nt)[1]

    def __enter__(self):
        def encode(graphs):
            idx = torch.tensor([self.index[id(g)] for g in graphs], device=self.mu.device)
            return self.mu[idx], self.logvar[idx]
        self.model.encode = encode
        return self

    def __exit__(self, *exc):
        del self.model.encode


@pytest.mark.parametrize("name,kind", E2E)
def test_recon_accuracy_counts_constructed_matches(device, name, kind):
    model = _model(name, device)
    N, E, D = 24, 3, 10
    with _ReconCase(model, device, N, E, D, 77) as case:
        want = case.want
        assert all(want[b] >= 1 + b % 5 for b in range(N)) and len(set(want.tolist())) > 1
        assert len({int(want[g0:g0 + 7].sum()) for g0 in range(0, N, 7)}) > 1   # the batches differ too
        n_perfect, n_total, per = dvae.recon_accuracy(model, case.G, E, D, draws=case.draws)
        assert per.tolist() == want.tolist() and n_perfect == int(want.sum()) > 0 and n_total == N * E * D
        # a permutation of the graphs: counts follow their graphs (true rows, draw columns and latent rows stay aligned)
        perm = np.random.default_rng(1).permutation(N)
        pd = (case.draws[0][:, :, perm].contiguous(), case.draws[1][:, :, perm].contiguous())
        got = dvae.recon_accuracy(model, [case.G[b] for b in perm], E, D, draws=pd)
        assert got[2].tolist() == want[perm].tolist()
        # stochastic=False: D identical argmax decodes per encode - all E * D or none
        d0 = model.decode_dense(case.mu, False)
        r0 = [x.cpu().numpy() for x in (d0.types, d0.preds, d0.nv)]
        G2 = [_graph_of_row(r0[0][0, b], r0[1][0, b], r0[2][0, b], model.nvt) if b % 2 == 0 else case.G[b] for b in range(N)]
        case.index.update({id(g): b for b, g in enumerate(G2)})
        want0 = case.count(G2, r0) * (E * D)
        assert all(want0[b] == E * D for b in range(0, N, 2))
        got = dvae.recon_accuracy(model, G2, E, D, stochastic=False, batch_size=9)
        assert got[2].tolist() == want0.tolist() and got[0] == int(want0.sum())
        # training mode: reparameterize samples around mu, so the encodes differ; the seed reproduces the run
        model.train()
        torch.manual_seed(5)
        a = dvae.recon_accuracy(model, case.G, E, D, draws=case.draws)
        torch.manual_seed(5)
        b = dvae.recon_accuracy(model, case.G, E, D, draws=case.draws)
        assert a[0] == b[0] > 0 and torch.equal(a[2], b[2])
        model.eval()


@pytest.mark.parametrize("name,kind", E2E)
def test_recon_accuracy_in_batches_counts_constructed_matches(device, name, kind):
    """Batches of 7 (the last one of 3): graphs defined by decodes of their own batch.  The counts differ between graphs
    and between batches.  For gated_sum, whose decoder does not couple rows, the batch size does not change anything."""
    model = _model(name, device)
    N, E, D = 24, 3, 10
    with _ReconCase(model, device, N, E, D, 78, batch=7) as case:
        want = case.want
        assert all(want[b] >= 1 + b % 5 for b in range(N))
        assert len({int(want[g0:g0 + 7].sum()) for g0 in range(0, N, 7)}) > 1
        n_perfect, n_total, per = dvae.recon_accuracy(model, case.G, E, D, draws=case.draws, batch_size=7)
        assert per.tolist() == want.tolist() and n_perfect == int(want.sum()) > 0 and n_total == N * E * D
        if "gated" in name:
            for batch in (None, 1, 23):
                assert dvae.recon_accuracy(model, case.G, E, D, draws=case.draws, batch_size=batch)[2].tolist() == want.tolist()


@pytest.mark.parametrize("name,kind", E2E)
def test_recon_accuracy_draws_and_synchronisation_with_the_real_encoder(device, name, kind):
    """With model.encode itself (the counts are those of one decode of the same mu, whatever they are): uniforms drawn
    inside equal given ones under the seed, and the call adds one synchronisation to what its encode() calls need."""
    model = _model(name, device)
    n, N, E, D = model.max_n, 24, 3, 10
    seedG = Hh.dvae_graphs_from_dense(*Hh.dvae_dense_graphs("chain", N, n, model.nvt, 0, 4), model.nvt)
    with torch.no_grad():
        mu = model.encode(seedG)[0]
    torch.manual_seed(77)
    draws = dvae._take_draws(None, n, N, E * D, device, "")
    d = model.decode_dense(mu, True, E * D, draws)
    rows = [x.cpu().numpy() for x in (d.types, d.preds, d.nv)]
    torch.manual_seed(77)
    inside = dvae.recon_accuracy(model, seedG, E, D)
    given = dvae.recon_accuracy(model, seedG, E, D, draws=draws)
    assert inside[0] == given[0] and torch.equal(inside[2], given[2])
    tt, pt, nt = dvae.dense_rows(seedG, n, model.nvt)
    assert given[2].tolist() == dvae.same_dag_host(*rows, tt, pt, nt)[1].tolist()

    def encodes():
        with torch.no_grad():
            return [model.encode(seedG[g0:g0 + 7]) for g0 in range(0, N, 7)]
    _, base = _sync_count(encodes)
    _, syncs = _sync_count(lambda: dvae.recon_accuracy(model, seedG, E, D, draws=draws, batch_size=7))
    assert syncs == base + 1, (syncs, base)


def test_prior_validity_refuses_a_host_training_set_with_a_gpu_model(device):
    model = _model("dvae_decode_na_h64_L2_sample", device)
    rows = synth.match_rows(1, "ENAS", 5, 4, 8, 8, 10)
    host = dvae.GraphSet.from_dense(rows["types_train"], rows["preds_train"], rows["nv_train"])
    with pytest.raises(ValueError, match="train_set lives on"):
        dvae.prior_validity(model, host, 10, 2)


def test_extract_latent_restores_the_mode(device):
    model = _model("dvae_decode_na_h64_L2_sample", device)
    G = Hh.dvae_graphs_from_dense(*Hh.dvae_dense_graphs("random0.5", 5, 8, 8, 0, 2), 8)
    model.train()
    dvae.extract_latent(model, G, 4)
    assert model.training
    model.eval()
    dvae.extract_latent(model, G, 4)
    assert not model.training


@pytest.mark.parametrize("name,kind", E2E)
def test_prior_validity_matches_the_composition(device, name, kind):
    model = _model(name, device)
    n, nvt, P, D = model.max_n, model.nvt, 300, 10
    z = _t(np.random.default_rng(9).standard_normal((P, 56)).astype(np.float32), device)
    st, se = dvae.draw_shapes(n, P, D)
    torch.manual_seed(31)
    u = torch.rand(int(np.prod(st)) + int(np.prod(se)), device=device)
    draws = (u[:int(np.prod(st))].view(st), u[int(np.prod(st)):].view(se))
    d = model.decode_dense(z, True, D, draws)
    dense = {k: getattr(d, k).cpu().numpy() for k in ("types", "preds", "nv")}
    # training set: every third decoded row (valid or not) and prepared rows that match nothing
    flat = [dense[k].reshape((P * D,) + dense[k].shape[2:])[::3] for k in ("types", "preds", "nv")]
    extra = synth.decoded_rows(3, kind, 1, 500, n, nvt)
    train_rows = [np.concatenate([a, b[0]]) for a, b in zip(flat, extra)]
    dense.update(types_train=train_rows[0], preds_train=train_rows[1], nv_train=train_rows[2])
    valid, n_unique, n_in = host_metrics(dense, kind, nvt)
    train = dvae.GraphSet.from_dense(*(_t(x, device) for x in train_rows))
    res = dvae.prior_validity(model, train, decode_times=D, data_type=kind, z=z, draws=draws)
    assert (res.n_valid, res.n_total, res.n_unique, res.n_in_train) == (int(valid.sum()), P * D, n_unique, n_in)
    assert res.r_valid == valid.sum() / (P * D)
    if res.n_valid:
        assert res.r_unique == n_unique / res.n_valid and res.r_novel == 1.0 - n_in / res.n_valid
    else:
        assert res.r_unique == 0.0 and res.r_novel == 0.0
    for batch in (64, 299, 7):
        got = dvae.prior_validity(model, train, decode_times=D, data_type=kind, z=z, draws=draws, batch_size=batch)
        if "gated" in name:   # this decoder does not couple the rows of a call: batches of points change nothing
            assert got == res, batch
        # attn_h couples them (the reference's padded soft-max): the same batches, decoded here, through the host mirrors
        parts = [model.decode_dense(z[p0:p0 + batch], True, D, (draws[0][:, :, p0:p0 + batch], draws[1][:, :, p0:p0 + batch]))
                 for p0 in range(0, P, batch)]
        bd = {k: torch.cat([getattr(q, k) for q in parts], 1).cpu().numpy() for k in ("types", "preds", "nv")}
        bd.update(types_train=train_rows[0], preds_train=train_rows[1], nv_train=train_rows[2])
        bvalid, bunique, bin_ = host_metrics(bd, kind, nvt)
        assert (got.n_valid, got.n_total, got.n_unique, got.n_in_train) == (int(bvalid.sum()), P * D, bunique, bin_), batch
    torch.manual_seed(31)
    assert dvae.prior_validity(model, train, decode_times=D, data_type=kind, z=z) == res   # the same uniforms, drawn inside
    out, syncs = _sync_count(lambda: dvae.prior_validity(model, train, decode_times=D, data_type=kind, z=z, draws=draws,
                                                         batch_size=64))
    assert out == res and syncs == 1, syncs
    torch.manual_seed(8)
    zm, zs = torch.full((56,), 0.25, device=device), torch.full((56,), 2.0, device=device)
    a = dvae.prior_validity(model, train, 100, D, kind, z_mean=zm, z_std=zs)
    torch.manual_seed(8)
    zz = torch.randn(100, 56, device=device) * zs + zm
    dr = dvae._take_draws(None, n, 100, D, device, "")
    assert a == dvae.prior_validity(model, train, decode_times=D, data_type=kind, z=zz, draws=dr)


def test_extract_latent_is_encode_in_batches(device):
    model = _model("dvae_decode_na_h64_L2_sample", device)
    G = Hh.dvae_graphs_from_dense(*Hh.dvae_dense_graphs("random0.5", 20, 8, 8, 0, 2), 8)
    mu = dvae.extract_latent(model, G, 8)
    with torch.no_grad():
        want = torch.cat([model.encode(G[i:i + 8])[0] for i in range(0, 20, 8)])
    assert mu.is_cuda and tuple(mu.shape) == (20, 56) and torch.equal(mu, want)


def test_engine_calls_do_not_synchronise_and_repeat_bitwise(device):
    rows = synth.match_rows(21, "ENAS", 64, 128, 8, 8, 5000)
    d = dvae.DecodedDense(*_dense(rows, device), None)
    true = _dense(rows, device, ("types_true", "preds_true", "nv_true"))
    train_rows = _dense(rows, device, ("types_train", "preds_train", "nv_train"))
    sel = dvae.select_decoded(d, "ENAS", 8, 0, 1)

    def run():
        train = dvae.GraphSet.from_dense(*train_rows)
        keys = dvae.DistinctKeys(sel.keys.shape[2], 64 * 128, device)
        keys.add(sel.keys, sel.valid)
        return tuple(dvae.same_dag_dense(d, *true)) + train.contains(d, sel.valid) + (keys.status().clone(), train.status().clone())
    first = run()   # (warm-up: library load, allocator)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_undersized_storage_is_refused_before_any_launch(device):
    rows = synth.match_rows(2, "ENAS", 5, 40, 8, 8, 100)
    train = _dense(rows, device, ("types_train", "preds_train", "nv_train"))
    words = engine.dvae_set_words(_lib.DVAE_SET_GRAPHS, 8, 100)
    small = torch.full((words - 1,), 7, dtype=torch.int32, device=device)
    for call in (lambda: engine.dvae_set_init(small, _lib.DVAE_SET_GRAPHS, 8, 100),
                 lambda: engine.dvae_set_add(small, _lib.DVAE_SET_GRAPHS, 8, 100, 0, train),
                 lambda: engine.dvae_set_query(small, 8, 100, *train)):
        with pytest.raises(_lib.DagnnHipError, match="ENOSPC"):
            call()
    assert bool((small == 7).all())   # nothing was written
    ok = torch.empty(words, dtype=torch.int32, device=device)
    engine.dvae_set_init(ok, _lib.DVAE_SET_GRAPHS, 8, 100)
    with pytest.raises(_lib.DagnnHipError, match="ENOSPC"):
        engine.dvae_set_add(ok, _lib.DVAE_SET_GRAPHS, 8, 100, 1, train)   # 100 rows from record 1: one too many
    assert ok[_lib.DVAE_SET_COUNT:_lib.DVAE_SET_ERR + 1].tolist() == [0, 0]
    with pytest.raises(ValueError, match="unsupported"):
        engine.dvae_set_words(_lib.DVAE_SET_GRAPHS, 8, (1 << 20) + 1)
