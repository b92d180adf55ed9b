"""GPU parity tier (-m gpu): the HIP path, called through the C ABI, against
(a) golden vectors produced by the real reference, (b) the CPU oracle on the same seeded inputs,
(c) size-independent properties at the BASELINE sizes.  fp32 tolerance 1e-4 (north_star)."""
import copy
import warnings

import numpy as np
import pytest
import torch

from dagnn_amd import engine, synth
from dagnn_amd._lib import DagnnHipError
from oracle import dagnn_oracle as O
from oracle.seeding import seeded_fill
from tests import helpers as Hh
from tests.helpers import _degenerate_batch, _train_step

pytestmark = pytest.mark.gpu
TOL = 1e-4  # BASELINE.json north_star: "within 1e-4 fp32"


@pytest.fixture(params=["dataflow", "lockstep", "pergraph"])
def schedule(request, monkeypatch):
    """The three HIP schedules of the recurrence: the persistent graph-affine dataflow launch (default for H <= 256),
    lock-step frontier launches (its fallback; the default for wider models) and persistent per-(graph, direction)
    workgroups."""
    monkeypatch.setenv("DAGNN_AMD_SCHEDULE", "pergraph" if request.param == "pergraph" else "lockstep")
    monkeypatch.setattr(engine, "DATAFLOW", 1 if request.param == "dataflow" else 0)
    return request.param


# ----------------------------------------------------------------------------- unit: kernels
def _plan_arrays(plan):
    ws = plan.ws.cpu().numpy()
    lay = plan.layout()
    return ws, lay


@pytest.mark.parametrize("small", [1, 0])   # 1: batches of <= 2048 nodes on the one-workgroup build (csrc/small.hip)
@pytest.mark.parametrize("seed,B,mean_n", [(1, 5, 20), (2, 17, 60), (0, 128, 125)])
def test_plan_matches_oracle_csr(device, monkeypatch, seed, B, mean_n, small):
    monkeypatch.setattr(engine, "PLAN_SMALL", small)
    b = synth.code2_batch(seed, B, mean_n)
    plan = engine.build_plan(b.edge_index.to(device), b._bi_layer_idx0.to(device), b._bi_layer_idx1.to(device),
                             b.batch.to(device), B, b.edge_attr.to(device))
    torch.cuda.synchronize()
    plan.check_status()
    ws, lay = _plan_arrays(plan)
    N, E = b.x.shape[0], b.edge_index.shape[1]
    node_ptr = ws[lay["node_ptr"]:lay["node_ptr"] + B + 1]
    assert np.array_equal(node_ptr, b.ptr.numpy())
    ei = b.edge_index.numpy()
    for d in (0, 1):
        layer = (b._bi_layer_idx0 if d == 0 else b._bi_layer_idx1).numpy()
        order = ws[lay["order%d" % d]:lay["order%d" % d] + N]
        depth = ws[lay["depth%d" % d]:lay["depth%d" % d] + B]
        col = ws[lay["col%d" % d]:lay["col%d" % d] + E]
        eattr = ws[lay["eattr%d" % d]:lay["eattr%d" % d] + 2 * E].view(np.float32).reshape(E, 2)
        assert sorted(order.tolist()) == list(range(N))
        feed, other = ei[1 - d], ei[d]
        for g in range(B):
            n0, n1 = node_ptr[g], node_ptr[g + 1]
            assert depth[g] == layer[n0:n1].max() + 1
            ls = ws[lay["lstart%d" % d] + n0 + g: lay["lstart%d" % d] + n0 + g + depth[g] + 1]
            rp = ws[lay["rowptr%d" % d] + n0 + g: lay["rowptr%d" % d] + n0 + g + (n1 - n0) + 1]
            assert ls[0] == n0 and ls[-1] == n1
            for t in range(depth[g]):
                rows = order[ls[t]:ls[t + 1]]
                # frontier t of graph g, in increasing node id (the reference's order, dagnn.py:146-147)
                expect = n0 + np.flatnonzero(layer[n0:n1] == t)
                assert np.array_equal(rows, expect)
            for p in range(n0, n1):
                v = order[p]
                e_ids = np.flatnonzero(feed == v)  # original edge order (dagnn.py:153-156)
                seg = slice(rp[p - n0], rp[p - n0 + 1])
                assert np.array_equal(col[seg], other[e_ids])
                assert np.array_equal(eattr[seg], b.edge_attr.numpy()[e_ids])
        # batch-level (lock-step) schedule: slots ordered by layer, every node exactly once
        T = int(layer.max()) + 1
        bl = ws[lay["blptr%d" % d]:lay["blptr%d" % d] + N + 2]
        assert bl[N + 1] == T and bl[0] == 0 and bl[T] == N
        rec16 = ws[lay["rowrec%d" % d]:lay["rowrec%d" % d] + 16 * N].reshape(N, 16)
        rec = rec16[:, :4]
        assert sorted(rec[:, 0].tolist()) == list(range(N))
        for t in range(T):
            nodes = rec[bl[t]:bl[t + 1], 0]
            assert np.array_equal(np.sort(nodes), np.flatnonzero(layer == t))
        pos = np.empty(N, dtype=np.int64)
        pos[order] = np.arange(N)
        gid = b.batch.numpy()
        rp_flat = lambda v: ws[lay["rowptr%d" % d] + pos[v] + gid[v]: lay["rowptr%d" % d] + pos[v] + gid[v] + 2]  # noqa
        for row in rec16[:: max(1, N // 200)]:
            v, eb, ee, g = row[:4]
            assert g == gid[v] and [eb, ee] == rp_flat(v).tolist()
            k = min(4, ee - eb)
            assert np.array_equal(row[4:4 + k], col[eb:eb + k])  # inline predecessors
            assert np.array_equal(row[8:8 + 2 * k].view(np.float32), eattr[eb:eb + k].reshape(-1))
        # backward-pass indices: rowrec slot of every node, original edge id of every CSR slot
        slot = ws[lay["slot%d" % d]:lay["slot%d" % d] + N]
        assert np.array_equal(rec[slot, 0], np.arange(N))
        eidx = ws[lay["eidx%d" % d]:lay["eidx%d" % d] + E]
        assert sorted(eidx.tolist()) == list(range(E))
        assert np.array_equal(col, other[eidx])
        owner = np.empty(E, dtype=np.int64)
        for row in rec:
            owner[row[1]:row[2]] = row[0]
        assert np.array_equal(owner, feed[eidx])
    items = ws[lay["items"]:lay["items"] + 2 * B]
    dep = [ws[lay["depth%d" % (i & 1)] + (i >> 1)] for i in items]
    assert sorted(items.tolist()) == list(range(2 * B)) and dep == sorted(dep, reverse=True)


@pytest.mark.parametrize("small", [1, 0])
def test_plan_flags_contract_violations(device, monkeypatch, small):
    monkeypatch.setattr(engine, "PLAN_SMALL", small)
    b = synth.code2_batch(4, 4, 20)
    dev = lambda t: t.to(device)   # noqa: E731
    N = b.x.shape[0]
    bad_batch = b.batch.clone()
    bad_batch[3] = 2  # not sorted
    crossing = b.edge_index.clone()
    crossing[1, 0] = N - 1   # an edge from the first graph into the last
    ungrouped = torch.cat([b.edge_index[:, -1:], b.edge_index[:, :-1]], 1)   # the last graph's edge first
    deep = b._bi_layer_idx0.clone()
    deep[0] = N   # a layer id >= nodes of its graph
    seen = set()
    cases = [(b.edge_index, b._bi_layer_idx0, bad_batch, "not sorted"), (crossing, b._bi_layer_idx0, b.batch, "crosses"),
             (ungrouped, b._bi_layer_idx0, b.batch, "not grouped"), (b.edge_index, deep, b.batch, "layer id")]
    for ei, l0, bt, what in cases * 2:
        fused = what in seen   # second round: the same batches through the fused pipeline (csrc/prepare.hip)
        seen.add(what)
        plan = engine.build_plan(dev(ei), dev(l0), dev(b._bi_layer_idx1), dev(bt), 4, None, launch=not fused)
        if fused:
            plan.launch_prepare(2)
        torch.cuda.synchronize()
        with pytest.raises(DagnnHipError, match=what):
            plan.check_status()
        ws, lay = _plan_arrays(plan)   # sealed: no depths, no batch-level layers
        for d in (0, 1):
            assert not ws[lay["depth%d" % d]:lay["depth%d" % d] + 4].any()
            assert not ws[lay["blptr%d" % d]:lay["blptr%d" % d] + N + 2].any()


@pytest.mark.parametrize("H", [32, 256, 300])
def test_encoder_kernel(device, H):
    g = torch.Generator().manual_seed(H)
    N = 1000
    tw, aw, dw = torch.randn(98, H, generator=g), torch.randn(500, H, generator=g), torch.randn(21, H, generator=g)
    x = torch.stack([torch.randint(0, 98, (N,), generator=g), torch.randint(0, 500, (N,), generator=g)], 1)
    depth = torch.randint(0, 40, (N,), generator=g)
    d_dev = depth.clone().to(device)
    out = engine.encode_ast(x.to(device), d_dev, tw.to(device), aw.to(device), dw.to(device), 20)
    dc = depth.clamp(max=20)
    ref = tw[x[:, 0]] + aw[x[:, 1]] + dw[dc]
    assert torch.equal(out.cpu(), ref)  # same association order -> bit exact
    assert torch.equal(d_dev.cpu(), dc)  # in-place clamp side effect (utils.py:27)


@pytest.mark.parametrize("M,Nc,K", [(1, 96, 8), (77, 768, 10), (300, 384, 256), (1000, 900, 300), (129, 1536, 512),
                                     (4099, 768, 256), (64, 128, 256), (515, 96, 32), (2049, 300, 100)])   # (the last three, and the first: the small-matrix kernel)
def test_gemm_nt_bias(device, M, Nc, K):
    g = torch.Generator().manual_seed(M + Nc + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(Nc, K, generator=g) * 0.3  # asymmetric operands: catches a transposed C-write
    b = torch.randn(Nc, generator=g)
    (C,) = engine.gemm_nt_bias([A.to(device)], [W.to(device)], [b.to(device)])
    ref = (A.double() @ W.double().t() + b.double())
    scale = (A.abs().double() @ W.abs().double().t()).max()
    assert float((C.cpu().double() - ref).abs().max()) < 2e-6 * float(scale)
    # grouped launch == separate launches, bitwise
    W2 = torch.randn(Nc, K, generator=g)
    C1, C2 = engine.gemm_nt_bias([A.to(device)] * 2, [W.to(device), W2.to(device)], [b.to(device), None])
    assert torch.equal(C1, C)
    assert float((C2.cpu().double() - A.double() @ W2.double().t()).abs().max()) < 2e-6 * float(scale) * 4


def test_parameter_writes_the_version_counters_miss_are_reported(device):
    """core.ParamGuard: an evaluation loop that updates parameters through `.data` (or a fused optimizer) WITHOUT a train() /
    eval() call in between reads derived weights cached from the old values; the version counters the caches key on do not
    move.  The pass after such a write must not go unnoticed: the guard's fingerprint of the parameters differs, the error
    word says so, check() raises; `invalidate_caches()` is the remedy and the pass after it sees the new values."""
    model = _headline_model().to(device)
    b = synth.code2_batch(0, 16)
    with torch.no_grad():
        base = [o.clone() for o in model(b.clone().to(device))]
        again = [o.clone() for o in model(b.clone().to(device))]
    model.check()   # two clean passes: recorded, then compared - no report
    assert max(Hh.maxdiff(a, c) for a, c in zip(again, base)) == 0.0
    v = model.cells_0[0].weight_hh._version
    model.cells_0[0].weight_hh.data.mul_(1.25)   # (no version bump: DerivedCache keeps serving the packed old matrix)
    assert model.cells_0[0].weight_hh._version == v
    with torch.no_grad():
        stale = [o.clone() for o in model(b.clone().to(device))]
    assert max(Hh.maxdiff(a, c) for a, c in zip(stale, base)) == 0.0   # the stale read itself ...
    with pytest.raises(DagnnHipError, match="version counter"):
        model.check()                                                  # ... is reported
    model.invalidate_caches()
    with torch.no_grad():
        fresh = [o.clone() for o in model(b.clone().to(device))]
    model.check()
    assert max(Hh.maxdiff(a, c) for a, c in zip(fresh, base)) > 1e-4
    # an update the counters DO see re-records instead of reporting
    with torch.no_grad():
        model.cells_1[0].bias_hh.add_(0.5)
        model(b.clone().to(device))
        model(b.clone().to(device))
    model.check()
    # the D-VAE encoders carry the same guard
    meta, arr = Hh.load("bn_h256_bidir")
    enc, _ = Hh.dvae_model(meta)
    enc = enc.to(device)
    with torch.no_grad():
        enc(Hh.dvae_batch(arr, device))
        enc(Hh.dvae_batch(arr, device))
    enc.check()
    next(p_ for n_, p_ in enc.named_parameters() if "weight_hh" in n_).data.mul_(1.5)
    with torch.no_grad():
        enc(Hh.dvae_batch(arr, device))
    with pytest.raises(DagnnHipError, match="version counter"):
        enc.check()
    enc.invalidate_caches()
    with torch.no_grad():
        enc(Hh.dvae_batch(arr, device))
    enc.check()


def test_pack_whh(device):
    W = torch.randn(3 * 76, 76)
    assert torch.equal(engine.pack_whh(W.to(device)).cpu(), W.t().contiguous())


def test_cpu_tensors_fail_loudly():
    with pytest.raises(DagnnHipError):
        engine.pack_whh(torch.randn(12, 4))


# ----------------------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("name", Hh.CODE2)
def test_code2_forward_matches_reference_golden(device, name, schedule):
    meta, arr = Hh.load(name)
    model = Hh.code2_model(meta).to(device)
    G = Hh.code2_batch(arr, device)
    with torch.no_grad():
        out = model(G)
    out = out if isinstance(out, list) else [out]
    assert len(out) == arr["pred"].shape[0]
    for o, ref in zip(out, arr["pred"]):
        assert tuple(o.shape) == ref.shape
        assert Hh.maxdiff(o, ref) < TOL
    # which input path the pass took is part of what this test pins: an evaluation pass on the lock-step schedule reads stacked
    # layer 0's input side from the folded embedding tables (model._folded_tables) wherever its conditions hold - if they ever
    # stop holding, the folded path would otherwise lose its reference check without anybody noticing
    fold_applies = schedule != "pergraph" and engine.FOLD_INPUT and meta["H"] % 4 == 0 and not model.agg_x
    assert model.__dict__.get("fold_passes", 0) == (1 if fold_applies else 0)
    rows = arr["rows"]
    assert Hh.maxdiff(G.x[rows], arr["x_emb"]) < 1e-6
    assert np.array_equal(G.node_depth.cpu().numpy(), arr["node_depth_after"])
    assert tuple(G.bi_layer_index.shape) == (2, 2, arr["x"].shape[0])
    if isinstance(G.h, list):
        for d, hd in enumerate(G.h):
            for i, h in enumerate(hd):
                assert Hh.maxdiff(h[rows], arr["h_%d_%d" % (d, i)]) < TOL
    else:
        assert Hh.maxdiff(G.h, arr["h_cat"]) < TOL
        assert np.array_equal(G.batch.cpu().numpy(), arr["batch_after"])


@pytest.mark.parametrize("name", Hh.DVAE)
def test_dvae_encode_matches_reference_golden(device, name, schedule):
    meta, arr = Hh.load(name)
    model, nn_ = Hh.dvae_model(meta)
    model = model.to(device)
    G = Hh.dvae_batch(arr, device)
    with torch.no_grad():
        Hg = model(G)
        mu, logvar = model.fc1(Hg), model.fc2(Hg)
    assert Hh.maxdiff(Hg, arr["Hg"]) < TOL
    assert Hh.maxdiff(mu, arr["mu"]) < TOL and Hh.maxdiff(logvar, arr["logvar"]) < TOL
    assert np.array_equal(G.batch.cpu().numpy(), arr["batch_after"])
    # encode(list[Data]) path: rebuild the graphs from the stored rows with OUR decoders
    import json
    rows = [json.loads(r) for r in arr["rows"]]
    dec = synth.decode_enas_row if meta["kind"] == "na" else synth.decode_bn_row
    with torch.no_grad():
        mu2, lv2 = model.encode([dec(r) for r in rows])
    assert Hh.maxdiff(mu2, arr["mu"]) < TOL and Hh.maxdiff(lv2, arr["logvar"]) < TOL


@pytest.mark.parametrize("name", ["na_h64_add", "bn_h64_max", "na_h64_gated_sum"])
def test_dvae_aggregator_weights_follow_silent_parameter_updates(device, name):
    """`add` / `max` on the D-VAE encoders derive their weights through a cached view object (variants._derive).  A fused
    optimizer (or a write through `.data`) changes parameters without bumping `_version`: a train() / eval() switch has
    to drop that cache too (round-4 advisor finding: eval -> silent update -> eval returned the OLD weights)."""
    meta, arr = Hh.load(name)
    model, _ = Hh.dvae_model(meta)
    model = model.to(device)
    with torch.no_grad():
        before = model(Hh.dvae_batch(arr, device)).clone()   # eval: fills the derived-weight cache of the view
    model.train()
    with torch.no_grad():
        for p_ in model.parameters():
            p_.data.mul_(0.5)                                # no `_version` bump, like torch.optim.Adam(fused=True)
    model.eval()
    fresh, _ = Hh.dvae_model(meta)
    fresh = fresh.to(device)
    with torch.no_grad():
        for q, p_ in zip(fresh.parameters(), model.parameters()):
            q.copy_(p_)
        after, want = model(Hh.dvae_batch(arr, device)), fresh(Hh.dvae_batch(arr, device))
    assert Hh.maxdiff(after, want) < 1e-6
    assert Hh.maxdiff(after, before) > 1e-4                  # (the update really changed the outputs)


@pytest.mark.parametrize("name", ["code2_h256_bidir", "code2_h64_unidir", "code2_h128_deep", "code2_h64_attn_x",
                                  "code2_h512_L5"])
@pytest.mark.parametrize("knob", ["mfma_tiles", "no_tail"])
def test_launch_shape_variants_match_reference_golden(device, name, knob, monkeypatch):
    """Force the code paths the small fixtures would not reach on their own: 64-row MFMA tiles (csrc/fat.hip) for
    every launch, every layer as its own launch (no persistent tail)."""
    monkeypatch.setenv("DAGNN_AMD_SCHEDULE", "lockstep")
    monkeypatch.setattr(engine, "DATAFLOW", 0)
    if knob == "mfma_tiles":
        monkeypatch.setattr(engine, "MFMA_MIN_ROWS", 1)
        monkeypatch.setattr(engine, "TAIL_REPLICAS", 0)
    else:
        monkeypatch.setattr(engine, "TAIL_REPLICAS", 0)
        monkeypatch.setattr(engine, "MFMA_MIN_ROWS", 0)
    meta, arr = Hh.load(name)
    model = Hh.code2_model(meta).to(device)
    G = Hh.code2_batch(arr, device)
    with torch.no_grad():
        out = model(G)
    out = out if isinstance(out, list) else [out]
    for o, ref in zip(out, arr["pred"]):
        assert Hh.maxdiff(o, ref) < TOL


# ----------------------------------------------------------------------------- oracle at scale
def _headline_model(H=256, L=2, V=64, seed=0):
    from dagnn_amd import DAGNN, ASTNodeEncoder
    enc = ASTNodeEncoder(H, 98, 10030, 20)
    m = DAGNN(num_vocab=V, max_seq_len=5, emb_dim=H, hidden_dim=H, out_dim=None, encoder=enc, w_edge_attr=True,
              num_layers=L, bidirectional=True, agg="attn_h", out_wx=False, out_pool_all=False, out_pool="max",
              dropout=0.0).eval()
    seeded_fill(m, 1000 + seed)
    return m


@pytest.mark.parametrize("split", [0, 1])
def test_headline_batch_split_modes_agree(device, split, monkeypatch):
    """The headline batch with and without the split mode (deep graphs on a side stream).  A row may be handled by a
    different kernel in the two modes (MFMA tile vs slice FMA: another summation order), so the results agree to
    rounding, not bit for bit; each mode by itself is deterministic (test_headline_properties, stress test)."""
    from bench import build_model
    b = synth.code2_batch(0, 128)
    b.x[:, 1] %= 10030
    y = torch.randint(0, 48, (128, 3), generator=torch.Generator().manual_seed(9)).to(device)
    res = {}
    monkeypatch.setattr(engine, "DATAFLOW", 0)
    for mode in (1 - split, split):
        monkeypatch.setattr(engine, "SPLIT_DEEP", mode)
        model = build_model(128, 2, 48, 3, device)
        with torch.no_grad():
            out = [o.clone() for o in model(b.clone().to(device))]
        _, grads = _train_step(model, b.clone().to(device), y)
        res[mode] = (out, {k: v.clone() for k, v in grads.items() if "encoder." not in k})
    assert max(Hh.maxdiff(a, c) for a, c in zip(res[0][0], res[1][0])) < 2e-5
    for k in res[0][1]:
        scale = float(res[0][1][k].abs().max())
        assert Hh.maxdiff(res[0][1][k], res[1][1][k]) <= 2e-5 * scale + 1e-7, k


def test_headline_batch_matches_oracle(device, schedule):
    """cfg 2 at full size (seed-0 batch: B=128, N=16 561, E=25 377, T=374; h=256, L=2, bidir)."""
    model = _headline_model()
    b = synth.code2_batch(0, 128)
    ref = _oracle_forward("cfg2_full", model, b, 2)
    model = model.to(device)
    G = b.to(device)
    with torch.no_grad():
        out = model(G)
    assert max(Hh.maxdiff(o, r) for o, r in zip(out, ref)) < TOL


def test_folded_input_tables_and_side_stream_plan_agree_with_the_plain_path(device, monkeypatch):
    """Evaluation passes fold the three embedding tables through `W_ih` of stacked layer 0 (model._folded_gi0: gi0 = three
    folded rows summed per node instead of the [N, emb] x [emb, 3H] GEMM) and build plan + schedule on a side stream next to
    the encoder (`engine.PLAN_OVERLAP`): both against the in-line GEMM path on the headline batch - the logits agree to
    rounding (another summation order of the same products), and the folded tables follow a parameter update."""
    model = _headline_model().to(device)
    b = synth.code2_batch(0, 128)
    outs = {}
    for fold, overlap in ((0, 0), (1, 0), (0, 1), (1, 1)):
        monkeypatch.setattr(engine, "FOLD_INPUT", fold)
        monkeypatch.setattr(engine, "PLAN_OVERLAP", overlap)
        with torch.no_grad():
            G = b.clone().to(device)
            outs[(fold, overlap)] = [o.clone() for o in model(G)]
            assert G.bi_layer_index.shape == (2, 2, b.x.shape[0])
            assert torch.equal(G.bi_layer_index[1][1].cpu(), b._bi_layer_index1)   # (side effect 1, made on the side stream)
    model.check()
    base = outs[(0, 0)]
    assert max(Hh.maxdiff(a, c) for a, c in zip(outs[(0, 1)], base)) == 0.0      # the same kernels on another stream: bitwise
    assert max(Hh.maxdiff(a, c) for a, c in zip(outs[(1, 1)], outs[(1, 0)])) == 0.0
    assert max(Hh.maxdiff(a, c) for a, c in zip(outs[(1, 0)], base)) < 2e-5
    # a parameter update (version counter bumped) reaches the folded tables
    monkeypatch.setattr(engine, "FOLD_INPUT", 1)
    with torch.no_grad():
        model.encoder.depth_encoder.weight.mul_(1.5)
        model.cells_0[0].bias_ih.add_(0.25)
        folded = [o.clone() for o in model(b.clone().to(device))]
        monkeypatch.setattr(engine, "FOLD_INPUT", 0)
        plain = [o.clone() for o in model(b.clone().to(device))]
    assert max(Hh.maxdiff(a, c) for a, c in zip(folded, plain)) < 2e-5
    assert max(Hh.maxdiff(a, c) for a, c in zip(plain, base)) > 1e-3


def test_bn_config_full_batch_matches_oracle(device, schedule):
    """cfg 4 at BASELINE.json's full size: `DAGNN_BN`, the bench's own batch (B = 128 synthetic Bayesian-network rows of seed 0,
    N = 1 280), h = 256, L = 2, bidirectional - `(mu, logvar)` and the graph vectors against the oracle (the reference fixture
    `bn_h256_bidir` holds 32 graphs; the plan / schedule word-for-word tests run at 128 but compare no states)."""
    from dagnn_amd import DAGNN_BN
    model = DAGNN_BN(10, 256, 256, 10, 10, 0, 1, hs=256, nz=56, num_nodes=10, num_layers=2, bidirectional=True).eval()
    seeded_fill(model, 4128)
    G = synth.dvae_batch([synth.decode_bn_row(r) for r in synth.bn_rows(0, 128)])
    key = "cfg4_full"
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = O.dvae_encode(model.state_dict(), copy.deepcopy(G), num_layers=2, bidirectional=True, num_nodes=10,
                                           vids=False)
    mu_ref, lv_ref = _ORACLE_CACHE[key]
    model = model.to(device)
    with torch.no_grad():
        Hg = model(G.to(device))
        mu, lv = model.fc1(Hg), model.fc2(Hg)
    assert Hh.maxdiff(mu, mu_ref) < TOL and Hh.maxdiff(lv, lv_ref) < TOL


def test_reference_training_shape_matches_oracle(device):
    """The reference's own training shape (scripts/ogb_tok.sh:17,63: emb_dim = hidden = 300, batch 160, L = 2, bidirectional) on
    the bench's batch (seed 0, B = 160: N = 20 168): the 320-wide dataflow kernels against the oracle at the model's own width -
    logits of all five heads (the 18-graph tests of the wide shape do not reach the bench batch's depth of 374 layers)."""
    model = _headline_model(H=300, L=2, V=32, seed=6)
    b = synth.code2_batch(0, 160)
    ref = _oracle_forward("ogb_tok_h300_B160", model, b, 2)
    model = model.to(device)
    with torch.no_grad():
        out = model(b.to(device))
    assert max(Hh.maxdiff(o, r) for o, r in zip(out, ref)) < TOL
    model.check()


def test_headline_properties(device, schedule):
    """Size-independent properties at BASELINE size: run-to-run bitwise determinism, graph
    independence (any sharding of the batch gives the same rows), graph-order equivariance."""
    model = _headline_model().to(device)
    graphs = synth.code2_graphs(0, 128)
    full = synth.GraphBatch.from_data_list(graphs)
    with torch.no_grad():
        out_a = torch.stack(model(full.clone().to(device)))
        out_b = torch.stack(model(full.clone().to(device)))
    assert torch.equal(out_a, out_b)
    # Collater split for 8 devices (tg/dataloader.py:17-27): concatenated shard outputs == full batch
    from dagnn_amd import collate_sharded
    shards = collate_sharded(graphs, 8)
    assert len(shards) == 8 and sum(s.num_graphs for s in shards) == 128
    with torch.no_grad():
        parts = [torch.stack(model(s.to(device))) for s in shards]
    # a shard is narrower than the full batch, so some of its layers take a different launch shape (fp32
    # FMA slices instead of fp32 MFMA tiles: same products, different summation order) - equal to
    # rounding, not bitwise
    assert Hh.maxdiff(torch.cat(parts, dim=1), out_a) < 2e-5
    # reversing the graph order permutes the rows and nothing else
    rev = synth.GraphBatch.from_data_list(graphs[::-1])
    with torch.no_grad():
        out_r = torch.stack(model(rev.to(device)))
    assert torch.equal(out_r.flip(1), out_a)


def test_wide_deep_config_full_size_properties(device):
    """cfg 5 at BASELINE.json's full size (B=256, h=512, L=5, bidirectional; the oracle needs minutes there): bitwise
    run-to-run determinism, graph-order equivariance, and the 64 deepest / widest graphs alone give the rows they
    give inside the full batch (to rounding: another batch takes other launch shapes)."""
    model = _headline_model(H=512, L=5, V=32, seed=5).to(device)
    graphs = synth.code2_graphs(3, 256)
    full = synth.GraphBatch.from_data_list(graphs)
    with torch.no_grad():
        a = torch.stack(model(full.clone().to(device)))
        b = torch.stack(model(full.clone().to(device)))
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        rev = torch.stack(model(synth.GraphBatch.from_data_list(graphs[::-1]).to(device)))
        assert Hh.maxdiff(rev.flip(1), a) < 2e-5
        order = sorted(range(256), key=lambda g: -graphs[g].x.shape[0])[:64]
        sub = torch.stack(model(synth.GraphBatch.from_data_list([graphs[g] for g in order]).to(device)))
        assert Hh.maxdiff(sub, a[:, order]) < 2e-5


def test_persistent_launches_of_two_streams_never_overlap(device):
    """Device-wide rule (engine.persistent_launch): the all-resident persistent kernels size their grids to the whole
    device, so passes issued on DIFFERENT streams must not run their recurrences at the same time (round 4's micro-batch
    experiment deadlocked until the bounded waits expired).  Eight forwards alternating over two streams - headline shape
    (dataflow kernel) and a 512-wide model (tile kernel) - give the bits of the one-stream passes, no bounded wait
    expires, and the rule records the handover (the later launch waited on the earlier stream's event)."""
    for H, L in ((256, 2), (512, 2)):
        model = _headline_model(H=H, L=L, V=32, seed=4).to(device)
        batches = [synth.code2_batch(30 + k, 48, 60).to(device) for k in range(2)]
        with torch.no_grad():
            ref = [torch.stack(model(b.clone())) for b in batches]
            torch.cuda.synchronize()
            streams = [torch.cuda.Stream(device) for _ in range(2)]
            outs = []
            for k in range(8):
                with torch.cuda.stream(streams[k % 2]):
                    outs.append(torch.stack(model(batches[k % 2].clone())))
            last = engine.persistent_launch._last.get(torch.device(device).index or 0)
            assert last is not None and last[1] == streams[1].cuda_stream
            torch.cuda.synchronize()
        model.check()
        for k, o in enumerate(outs):
            assert torch.equal(o, ref[k % 2]), (H, k)


_ORACLE_CACHE = {}


def _oracle_forward(key, model, b, L):
    """The CPU oracle's logits of (model, batch): computed once per session and key - the schedule parametrisations compare
    three GPU paths against the SAME reference, and the oracle is what these tests spend their time in."""
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = O.code2_forward(model.state_dict(), copy.deepcopy(b), num_layers=L, bidirectional=True, out_wx=False,
                                             out_pool_all=False, out_pool="max", max_seq_len=5)
    return _ORACLE_CACHE[key]


@pytest.mark.parametrize("path", ["default", "fat_launches", "fat_one_chain"])
def test_wide_deep_config_matches_oracle(device, schedule, path, monkeypatch):
    """cfg 5 shape (h=512, L=5, bidir) on a 24-graph batch (the oracle runs once per session): the default policy (the
    tile kernel alone at this size), every layer as a fat launch of 64-row MFMA tiles (csrc/fat.hip) on two chains, and
    the same on one chain."""
    if path != "default":
        if schedule != "lockstep":
            pytest.skip("the fat launches belong to the lock-step schedule")
        monkeypatch.setattr(engine, "TILES", 0)
        monkeypatch.setattr(engine, "MFMA_MIN_ROWS", 1)
        monkeypatch.setattr(engine, "DUAL_CHAINS", 1 if path == "fat_launches" else 0)
    model = _headline_model(H=512, L=5, V=32, seed=5)
    b = synth.code2_batch(21, 24)
    ref = _oracle_forward("cfg5_24", model, b, 5)
    model = model.to(device)
    with torch.no_grad():
        out = model(b.to(device))
    assert max(Hh.maxdiff(o, r) for o, r in zip(out, ref)) < TOL


def test_deep_stack_runs_on_the_dataflow_kernel(device, monkeypatch):
    """L = 5 stacked layers, h = 256, bidirectional = 18 kernel cells (more than round 2's 16-cell cap): forward and
    one training step on the persistent dataflow kernels, against the oracle; the same model with the dataflow path
    switched off agrees; and a model the dataflow kernel does not cover says so once."""
    import warnings
    calls = []
    lib = engine._lib.load()
    orig = lib.dagnn_dataflow_run
    monkeypatch.setattr(engine, "DATAFLOW", 1)
    model = _headline_model(H=256, L=5, V=24, seed=9)
    b = synth.code2_batch(17, 20, 40)
    ref = O.code2_forward(model.state_dict(), copy.deepcopy(b), num_layers=5, bidirectional=True, out_wx=False,
                          out_pool_all=False, out_pool="max", max_seq_len=5)
    model = model.to(device)
    assert engine.dataflow_groups(device, 2, 5, 256, 20) > 0
    with torch.no_grad():
        with warnings.catch_warnings():
            warnings.simplefilter("error")   # on the dataflow path: no fall-back warning
            out = model(b.clone().to(device))
        assert max(Hh.maxdiff(o, r) for o, r in zip(out, ref)) < TOL
        monkeypatch.setattr(engine, "DATAFLOW", 0)
        for c in model._derived.values():
            c.invalidate()
        out0 = model(b.clone().to(device))
        monkeypatch.setattr(engine, "DATAFLOW", 1)
        for c in model._derived.values():
            c.invalidate()
        assert max(Hh.maxdiff(o, r) for o, r in zip(out, out0)) < 2e-5
    model.check()
    y = torch.randint(0, 24, (20, 5), generator=torch.Generator().manual_seed(2))
    sd_cpu = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    loss_ref, grads_ref = O.code2_grads(sd_cpu, copy.deepcopy(b), y, num_layers=5, bidirectional=True, max_seq_len=5)
    loss, grads = _train_step(model, b.clone().to(device), y.to(device))
    model.check()
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    for k, g in grads_ref.items():
        scale = max(float(g.abs().max()), 1e-6)
        got = grads.get(k)
        got = torch.zeros_like(g) if got is None else got.cpu()
        assert float((got - g).abs().max()) <= 2e-4 * scale + 2e-7, k
    # a shape neither persistent kernel covers (h = 384, one layer: the dataflow kernels stop at 320, the tile kernel is
    # built for 512 and stacked models - engine.state_width leaves this one at 384) falls back to the per-layer launches
    # and says so, once
    from dagnn_amd import core
    core._OFF_DATAFLOW_SEEN.clear()
    assert engine.state_width(384, 1, 2) == 384
    wide = _headline_model(H=384, L=1, V=8, seed=1).to(device)
    small = synth.code2_batch(3, 4, 12)
    with torch.no_grad():
        with pytest.warns(RuntimeWarning, match="per-layer launch path"):
            wide(small.clone().to(device))
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            wide(small.clone().to(device))


def test_xcd_placement_changes_speed_not_results(device, monkeypatch):
    """The XCD-aware workgroup placement of the dataflow kernels (hand-offs through the shared L2 where a cell and its
    readers are SEEN on one XCD at run time) against the linear placement with write-through stores everywhere: logits,
    hidden states and every parameter gradient are bitwise the same, on the headline shape and on a small one whose
    group count (and therefore placement table) differs."""
    for H, L, B, mean_n in ((256, 2, 128, 125), (64, 3, 6, 30)):
        model = _headline_model(H=H, L=L, V=32, seed=4).to(device)
        b = synth.code2_batch(11, B, mean_n)
        y = torch.randint(0, 32, (B, 5), generator=torch.Generator().manual_seed(3)).to(device)
        res = {}
        for mode in (1, 0):
            monkeypatch.setattr(engine, "DF_XCD", mode)
            model.eval()
            with torch.no_grad():
                G = b.clone().to(device)
                out = torch.stack(model(G))
                hid = [h.clone() for hd in G.h for h in hd]
            loss, grads = _train_step(model, b.clone().to(device), y)
            model.check()
            res[mode] = (out, hid, loss, {k: v.clone() for k, v in grads.items()})
        assert torch.equal(res[0][0], res[1][0])
        assert all(torch.equal(a, c) for a, c in zip(res[0][1], res[1][1]))
        assert torch.equal(res[0][2], res[1][2])
        for k in res[0][3]:
            if "encoder." in k:   # (the embedding gradients are an atomic index_add: equal to rounding run to run, not bitwise)
                scale = float(res[0][3][k].abs().max()) + 1e-12
                assert float((res[0][3][k] - res[1][3][k]).abs().max()) <= 1e-5 * scale, k
            else:
                assert torch.equal(res[0][3][k], res[1][3][k]), k


def test_training_pass_leaves_room_for_a_collective(device, monkeypatch):
    """The co-residency rule of the persistent kernels (`engine.reserved_cus`): a data-parallel training step overlaps the
    heads' gradient all-reduce with the reverse sweep, and the collective's workgroups - launched FIRST - hold CUs.  With
    the reservation (what an active communicator switches on; forced here) the training pass sizes its dataflow launches
    for `num_cus - 64`, spread evenly over the XCDs, so a 40-workgroup kernel that spins on a second stream across the
    whole forward + backward (the stand-in for RCCL's channels: it only ends by itself, i.e. it never yields its CUs)
    changes neither bits nor - beyond 1.3x - time, and no bounded wait expires.  The inference pass keeps every CU."""
    from dagnn_amd import _lib
    lib = _lib.load()
    model = _headline_model(H=256, L=2, V=32, seed=4).to(device)
    b = synth.code2_batch(11, 128, 125)
    y = torch.randint(0, 32, (128, 5), generator=torch.Generator().manual_seed(3)).to(device)
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    full = engine.dataflow_groups(device, 2, 2, 256, 128)
    monkeypatch.setattr(engine, "RESERVED_CUS", 64)
    assert engine.reserved_cus(False) == 0 and engine.dataflow_groups(device, 2, 2, 256, 128) == full
    reserved = engine.dataflow_groups(device, 2, 2, 256, 128, training=True)
    assert 0 < reserved <= full and (reserved < full or cus < 256)
    side = torch.cuda.Stream(device)
    sink = torch.zeros(1, device=device)

    def step(occupied):
        torch.cuda.synchronize()
        if occupied:   # 40 workgroups x 256 threads that spin for ~30 ms: far longer than the step they sit next to
            _lib.check(lib.dagnn_debug_occupy(40, 256, 3_000_000, sink.data_ptr(), side.cuda_stream), "dagnn_debug_occupy")
            import time
            time.sleep(0.002)   # (the spinner is running before the step's first launch)
        a, c = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss, grads = _train_step(model, b.clone().to(device), y)
        c.record()
        c.synchronize()
        model.check()   # raises if any bounded wait of the pass expired
        ms = a.elapsed_time(c)
        torch.cuda.synchronize()
        return loss, {k: v.clone() for k, v in grads.items()}, ms

    step(False)
    ref = step(False)
    t_free = min(step(False)[2] for _ in range(3))
    occ = [step(True) for _ in range(3)]
    for loss, grads, _ in occ:
        assert torch.equal(loss, ref[0])
        for k in grads:
            if "encoder." not in k:   # (torch's embedding backward accumulates with atomics)
                assert torch.equal(grads[k], ref[1][k]), k
    t_occ = min(o[2] for o in occ)
    assert t_occ < 1.3 * t_free, (t_occ, t_free)
    # and the evaluation pass next to it: every CU, same logits as alone
    model.eval()
    with torch.no_grad():
        alone = torch.stack(model(b.clone().to(device)))
    torch.cuda.synchronize()
    assert engine.reserved_cus(False) == 0


def test_fused_sequence_loss_is_the_loss_loop(device):
    """`train.seq_cross_entropy` on the list `DAGNN.forward` returns: the value of the reference's loop
    `sum_i CrossEntropyLoss()(pred[i], y[:, i]) / S` and the same gradients (one launch for loss + d logits, the heads' weight
    gradients as one product); the heads' parameters stay ordinary entries of `state_dict` although they share one matrix;
    lists that are not views of one tensor take the plain loop; an out-of-range target is loud."""
    from dagnn_amd.train import seq_cross_entropy
    model = _headline_model(H=256, L=2, V=5002, seed=6).to(device)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    b = synth.code2_batch(13, 64, 125)
    y = torch.randint(0, 5002, (64, 5), generator=torch.Generator().manual_seed(5)).to(device)
    loss_a, grads_a = _train_step(model, b.clone().to(device), y, fused_loss=False)
    grads_a = {k: v.clone() for k, v in grads_a.items()}
    loss_b, grads_b = _train_step(model, b.clone().to(device), y, fused_loss=True)
    assert abs(float(loss_a) - float(loss_b)) < 2e-6
    for k, g in grads_a.items():
        assert Hh.maxdiff(grads_b[k], g) <= 2e-6 * max(1.0, float(g.abs().max())) + 1e-9, k
    # bitwise reproducible (fixed summation order)
    loss_c, grads_c = _train_step(model, b.clone().to(device), y, fused_loss=True)
    assert torch.equal(loss_b, loss_c)
    for k in ("graph_pred_linear_list.0.weight", "graph_pred_linear_list.4.bias"):
        assert torch.equal(grads_b[k], grads_c[k])
    # the heads still are five ordinary parameters
    sd1 = model.state_dict()
    assert list(sd1.keys()) == list(sd0.keys())
    for k, v in sd0.items():
        assert sd1[k].shape == v.shape and torch.equal(sd1[k], v), k
    w, _ = model._head_storage()
    with torch.no_grad():
        model.graph_pred_linear_list[3].weight.add_(1.0)       # an in-place update of a head IS an update of the matrix
    assert torch.equal(w[3 * 5002:4 * 5002], model.graph_pred_linear_list[3].weight)
    # not views of one tensor: the plain loop
    model.eval()
    with torch.no_grad():
        pred = [p.clone() for p in model(b.clone().to(device))]
        ref = sum(torch.nn.functional.cross_entropy(p, y[:, s]) for s, p in enumerate(pred)) / 5
        assert abs(float(seq_cross_entropy(pred, y)) - float(ref)) < 1e-6
        views = model(b.clone().to(device))
        assert abs(float(seq_cross_entropy(views, y)) - float(ref)) < 2e-6     # (no gradient asked for: the same kernel, no d logits)
        bad = y.clone()
        bad[3, 2] = 5002
        assert torch.isnan(seq_cross_entropy(views, bad))


@pytest.mark.parametrize("max_norm,wd", [(0.25, 0.0), (None, 0.0), (1e6, 0.01)])
def test_clip_adam_is_clip_grad_norm_plus_adam(device, max_norm, wd):
    """`train.ClipAdam.step()` against `torch.nn.utils.clip_grad_norm_` + `torch.optim.Adam.step()` (main_pyg.py:63-65) over
    four steps: parameters and both moments, the reported norm, the state_dict layout (a torch Adam loads it and continues),
    gradients left untouched; tensors of odd sizes and views at unaligned offsets (how the heads' biases sit in their matrix)."""
    from dagnn_amd.train import ClipAdam
    g0 = torch.Generator().manual_seed(7)
    flat = torch.randn(5 * 5002 + 3, generator=g0)
    shapes = [(768, 256), (768,), (1, 512), (33,), (5002, 64), (1,)]
    def make():
        base = flat.clone().to(device)
        ps = [torch.nn.Parameter(torch.randn(*sh, generator=torch.Generator().manual_seed(10 + i)).to(device)) for i, sh in enumerate(shapes)]
        views = []
        for i in range(5):   # five "bias" views of one buffer: offsets 5002 * 4 bytes apart (not 16-byte aligned)
            p = torch.nn.Parameter(torch.empty(0, device=device))
            p.data = base[i * 5002:(i + 1) * 5002]
            views.append(p)
        return ps + views
    pa, pb = make(), make()
    opt_a = torch.optim.Adam(pa, lr=1e-2, weight_decay=wd)
    opt_b = ClipAdam(pb, lr=1e-2, weight_decay=wd, max_norm=max_norm)
    for it in range(4):
        gs = [torch.randn(p.shape, generator=torch.Generator().manual_seed(100 * it + i)).to(device) * (3.0 if it % 2 else 0.01) for i, p in enumerate(pa)]
        for p, q, g in zip(pa, pb, gs):
            p.grad, q.grad = g.clone(), g.clone()
        if it == 2:
            pa[3].grad = pb[3].grad = None   # a parameter without a gradient this step is skipped (its step counter too)
        norm_a = torch.nn.utils.clip_grad_norm_(pa, max_norm) if max_norm else None
        opt_a.step()
        opt_b.step()
        if max_norm:
            assert abs(float(opt_b.last_norm) - float(norm_a)) <= 1e-5 * float(norm_a)
        for q, g in zip(pb, gs):
            if q.grad is not None:
                assert torch.equal(q.grad, g)   # not scaled in place
        for i, (p, q) in enumerate(zip(pa, pb)):
            assert Hh.maxdiff(q, p) <= 2e-6 * max(1.0, float(p.abs().max())), (it, i)
            if p in opt_a.state:
                for k in ("exp_avg", "exp_avg_sq"):
                    ref = opt_a.state[p][k]
                    assert Hh.maxdiff(opt_b.state[q][k], ref) <= 2e-6 * max(1e-3, float(ref.abs().max())), (it, i, k)
                assert float(opt_b.state[q]["step"]) == float(opt_a.state[p]["step"])
    # the state travels: a torch Adam continues from ClipAdam's state_dict
    opt_c = torch.optim.Adam(pb, lr=1e-2, weight_decay=wd)
    opt_c.load_state_dict(opt_b.state_dict())
    for p, q in zip(pa, pb):
        p.grad = q.grad = torch.ones_like(p) * 1e-3
    opt_a.step()
    opt_c.step()
    for i, (p, q) in enumerate(zip(pa, pb)):
        assert Hh.maxdiff(q, p) <= 2e-6 * max(1.0, float(p.abs().max())), i


def test_reserved_cus_change_the_schedule_not_the_gradients(device, monkeypatch):
    """`DAGNN_AMD_RESERVED_CUS` = 0 / 32 / 64 (what `engine.reserved_cus` derives from the gradient exchange's group and RCCL's
    channel count): a training pass sized for fewer CUs deals the graphs to fewer groups - another schedule, the same
    arithmetic per row in the same order: loss and every gradient of the cells, heads and attention must agree to the last
    bit (the embedding tables' backward in torch accumulates with atomics: rounding), and the rule reports why it reserved."""
    model = _headline_model(H=256, L=2, V=32, seed=5).to(device)
    b = synth.code2_batch(12, 128, 125)
    y = torch.randint(0, 32, (128, 5), generator=torch.Generator().manual_seed(4)).to(device)
    got = {}
    for r in (0, 32, 64):
        monkeypatch.setattr(engine, "RESERVED_CUS", r)
        assert engine.reserved_cus(True) == r and engine.reserved_cus(False) == 0
        assert "DAGNN_AMD_RESERVED_CUS" in engine.reserved_cus_info(True)[1]
        groups = engine.dataflow_groups(device, 2, 2, 256, 128, training=True)
        loss, grads = _train_step(model, b.clone().to(device), y)
        model.check()
        got[r] = (groups, loss.clone(), {k: v.clone() for k, v in grads.items()})
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    if cus >= 256:
        assert got[0][0] > got[64][0]   # 5 workgroup sets against 4 at the headline shape
    for r in (32, 64):
        assert torch.equal(got[r][1], got[0][1])
        for k, g in got[r][2].items():
            if "encoder." in k:
                assert Hh.maxdiff(g, got[0][2][k]) <= 1e-6 * max(1.0, float(got[0][2][k].abs().max())), k
            else:
                assert torch.equal(g, got[0][2][k]), k
    monkeypatch.setattr(engine, "RESERVED_CUS", -1)
    assert engine.reserved_cus_info(True) == (0, "no communicator")   # (a single process without torch.distributed)


@pytest.mark.parametrize("H,L", [(256, 2), (128, 1), (320, 1)])
def test_static_rows_from_the_forward_launch_feed_the_reverse_sweep(device, monkeypatch, H, L):
    """`DAGNN_AMD_STAT_FWD` (`Route.stat_rows`): the forward launch of a training pass writes the reverse sweep's static
    record rows - state and gate coefficients (csrc/dataflow.hip, the AUX == 2 epilogue) - and `dagnn_bwd_dataflow_prepare`
    only adds the external-gradient row.  The same loss; gradients within fp32 rounding of the ones from the records
    `bd_stat_kernel` builds out of the kept pre-activations (it re-evaluates the gates with expf / tanhf, the forward
    epilogue uses the gates it applied); the widths cover the zero-filled record (128), both parts of the 320 one."""
    from dagnn_amd import _lib
    lib = _lib.load()
    model = _headline_model(H=H, L=L, V=32, seed=6).to(device)
    b = synth.code2_batch(13, 96, 125)
    y = torch.randint(0, 32, (96, 5), generator=torch.Generator().manual_seed(2)).to(device)
    got, flags = {}, {}
    orig = lib.dagnn_bwd_dataflow_prepare

    class _Spy(object):
        def __call__(self, plan, args, stream):
            flags.setdefault(cur[0], []).append(int(args._obj.stat_rows_written))
            return orig(plan, args, stream)
    monkeypatch.setattr(lib, "dagnn_bwd_dataflow_prepare", _Spy(), raising=False)
    cur = [None]
    for flag in (0, 1):
        cur[0] = flag
        monkeypatch.setattr(engine, "STAT_FWD", flag)
        loss, grads = _train_step(model, b.clone().to(device), y)
        model.check()
        got[flag] = (loss.clone(), {k: v.clone() for k, v in grads.items()})
    assert flags[0] == [0] and flags[1] == [1], flags
    assert torch.equal(got[0][0], got[1][0])
    for k, g in got[1][1].items():
        ref = got[0][1][k]
        assert Hh.maxdiff(g, ref) <= 2e-5 * max(float(ref.abs().max()), 1e-3), k


def test_a_pass_runs_the_route_it_computed_once(device, monkeypatch):
    """Seven passes on 3-graph batches of at most 40 nodes, one per path: the launch functions that ran are exactly those of
    the route the pass computed (`route.with_plan`, asked once), a dataflow schedule was built at most once and for
    `route.groups`, and the reverse function that ran is `route.reverse`."""
    from dagnn_amd import DAGNN, ASTNodeEncoder, route
    runs = {"dataflow": ["dataflow_run"], "tiles": ["tiles_run"], "launches+tiles": ["frontier_run", "tiles_run"], "launches": ["frontier_run"]}
    reverse = {"dataflow": ["bwd_dataflow_sweep"], "lockstep": ["backward_sweep"], None: []}
    ran, routes, asked, built = [], [], [], []

    def spy(owner, name, log, note=None):
        orig = getattr(owner, name)

        def wrapper(*a, **k):
            out = orig(*a, **k)
            log.append(name if note is None else note(out))
            return out
        monkeypatch.setattr(owner, name, wrapper)
    for name in ("dataflow_run", "tiles_run", "frontier_run", "bwd_dataflow_sweep", "backward_sweep"):
        spy(engine, name, ran)
    spy(route, "with_plan", routes, lambda r: r)
    spy(route, "before_plan", asked)
    for name in ("dataflow_schedule", "launch_prepare"):   # a schedule is built by the call that leaves it in the plan's cache
        orig = getattr(engine.PlanHandle, name)

        def builder(self, groups=0, *a, _orig=orig, **k):
            had = set(self.__dict__.get("_df", {}))
            out = _orig(self, groups, *a, **k)
            built.extend(key[0] for key in set(self.__dict__.get("_df", {})) - had)
            return out
        monkeypatch.setattr(engine.PlanHandle, name, builder)

    cases = [(64, 1, True, {}, False, (64, "dataflow", None)), (300, 2, True, {}, False, (320, "dataflow", None)),
             (300, 1, False, {}, False, (320, "launches", None)), (512, 2, True, {}, False, (512, "tiles", None)),
             (64, 2, True, {"DATAFLOW": 0}, False, (64, "launches", None)), (64, 2, True, {}, True, (64, "dataflow", "dataflow")),
             (64, 2, True, {"BWD_DF_MAX_BYTES": 0}, True, (64, "dataflow", "lockstep"))]
    for k, (H, L, wea, flags, train, expect) in enumerate(cases):
        with monkeypatch.context() as m:
            for name, v in flags.items():
                m.setattr(engine, name, v)
            model = DAGNN(num_vocab=8, max_seq_len=5, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(H, 98, 10030, 20),
                          w_edge_attr=wea, num_layers=L, bidirectional=True, agg="attn_h", out_wx=False, out_pool_all=False,
                          out_pool="max", dropout=0.0)
            seeded_fill(model, 70 + k)
            model = model.to(device)
            b = synth.code2_batch(20 + k, 3, 20, 40).to(device)
            del ran[:], routes[:], asked[:], built[:]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)   # (the per-layer launches say once that they are not the dataflow kernel)
                if train:
                    y = torch.randint(0, 8, (3, 5), generator=torch.Generator().manual_seed(k)).to(device)
                    _train_step(model, b, y)
                else:
                    with torch.no_grad():
                        model.eval()(b)
            model.check()
            assert len(routes) == 1 and len(asked) == 1, (H, L, routes, asked)
            r = routes[0]
            assert (r.Hp, r.kind, r.reverse) == expect, r
            assert ran == runs[r.kind] + reverse[r.reverse], (r, ran)
            assert built == ([r.groups] if r.groups > 0 else []) and (r.groups > 0) == (r.kind == "dataflow"), (r, built)


def test_edge_cases(device, schedule):
    """Single-node graphs, a chain, a star with a 200-way fan-in, and a graph with no edges."""
    b = _degenerate_batch()
    model = _headline_model(H=64, L=2, V=16, seed=9)
    # shrink the attribute table use: x[:,1] < 300 already
    ref = O.code2_forward(model.state_dict(), copy.deepcopy(b), num_layers=2, bidirectional=True, out_wx=False,
                          out_pool_all=False, out_pool="max", max_seq_len=5)
    model = model.to(device)
    with torch.no_grad():
        out = model(b.to(device))
    assert max(Hh.maxdiff(o, r) for o, r in zip(out, ref)) < TOL


def test_out_wx_and_other_pools(device, schedule):
    from dagnn_amd import DAGNN, ASTNodeEncoder
    b = synth.code2_batch(31, 9, 30)
    for kw in (dict(out_wx=True, out_pool="max"), dict(out_wx=False, out_pool="mean"),
               dict(out_wx=False, out_pool="add", out_pool_all=True), dict(out_wx=False, out_pool="attn"),
               dict(out_wx=False, out_pool="mean", out_pool_all=True), dict(out_pool="attn", out_pool_all=True),
               dict(bidirectional=False, out_pool="mean"), dict(bidirectional=False, out_pool="add", out_wx=True),
               dict(bidirectional=False, out_pool="max", out_pool_all=True)):
        enc = ASTNodeEncoder(32, 98, 10030, 20)
        args = dict(w_edge_attr=True, num_layers=2, bidirectional=True, agg="attn_h", out_wx=False,
                    out_pool_all=False, out_pool="max", dropout=0.0)
        args.update(kw)
        m = DAGNN(num_vocab=12, max_seq_len=3, emb_dim=32, hidden_dim=32, out_dim=None, encoder=enc, **args).eval()
        seeded_fill(m, 77)
        ref = O.code2_forward(m.state_dict(), copy.deepcopy(b), num_layers=2, bidirectional=args["bidirectional"],
                              out_wx=args["out_wx"], out_pool_all=args["out_pool_all"], out_pool=args["out_pool"],
                              max_seq_len=3)
        m = m.to(device)
        G = copy.deepcopy(b).to(device)
        with torch.no_grad():
            out = m(G)
        assert max(Hh.maxdiff(o, r) for o, r in zip(out, ref)) < TOL, kw
        if not (args["bidirectional"] and not args["out_pool_all"]):
            # side effects of dagnn.py:194-202: G.h is the concatenation (of the output nodes only without
            # out_pool_all, and then G.batch is narrowed with it)
            rows = b.x.shape[0] if args["out_pool_all"] else int((b._bi_layer_idx1 == 0).sum())
            assert G.h.shape == (rows, m.out_hidden_dim) and G.batch.shape[0] == rows


def test_smoke_entry(device):
    import __graft_entry__ as ge
    ge.smoke()


# ----------------------------------------------------------------------------- training step
@pytest.mark.parametrize("fused_loss", [False, True])
@pytest.mark.parametrize("name", Hh.GRAD)
def test_training_step_gradients_match_reference_golden(device, name, fused_loss):
    """forward + `loss.backward()` through the HIP path against the reference's own autograd on the same
    seeded step: loss and every parameter gradient - with the reference's loss loop (main_pyg.py:55-60) and with the
    library's fused loss entry in its place."""
    meta, arr = Hh.load(name)
    model = Hh.code2_model(meta).to(device)
    G = Hh.code2_batch(arr, device)
    if fused_loss and model.num_class > 0:
        pytest.skip("a single classification head: the fused entry is the S-head loss")
    loss, grads = _train_step(model, G, torch.from_numpy(arr["y"]).to(device), fused_loss=fused_loss)
    assert abs(float(loss) - float(arr["loss"])) < 1e-5
    with torch.no_grad():
        assert Hh.maxdiff(torch.stack(model(Hh.code2_batch(arr, device))), arr["pred"]) < TOL
    assert Hh.check_grads(meta, arr, grads, rtol=1e-4) < 1e-4


def test_training_step_matches_oracle_autograd_and_is_deterministic(device):
    """A batch the fixtures do not cover (wider layers: 8-row blocks; fan-in/out > 4) against autograd
    through the CPU oracle; two runs give bitwise-identical cell gradients (gradients are pulled, no atomics)."""
    meta = dict(H=64, n_attr=300, V=40, S=3, w_seed=77,
                ctor=dict(w_edge_attr=True, num_layers=2, bidirectional=True, agg="attn_h", out_wx=False,
                          out_pool_all=False, out_pool="max", dropout=0.0))
    model = Hh.code2_model(meta)
    b = synth.code2_batch(31, 48, 70)
    b.x[:, 1] %= 300
    y = torch.from_numpy(np.random.default_rng(5).integers(0, 40, size=(48, 3)))
    loss_ref, ref = O.code2_grads(model.state_dict(), b.clone(), y, num_layers=2, bidirectional=True, max_seq_len=3)
    model = model.to(device)
    loss, grads = _train_step(model, b.clone().to(device), y.to(device))
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    for k, g in grads.items():
        scale = float(ref[k].abs().max())
        assert Hh.maxdiff(g, ref[k]) <= 1e-4 * scale + 2e-7, k
    _, again = _train_step(model, b.clone().to(device), y.to(device))
    for k in grads:
        if "encoder." not in k:  # the embedding-table gradients are torch index_add_ (atomics)
            assert torch.equal(grads[k], again[k]), k


def test_training_step_six_stacked_layers_with_edge_features(device):
    """L = 6, bidirectional, edge features: 12 cells = 36 column-sum jobs and 24 weight-gradient jobs in the backward
    epilogue - more than ONE `dagnn_colsum_run` takes (32; `engine.colsums` / `engine.wgrad` go in several launches).
    Every gradient against autograd through the CPU oracle."""
    meta = dict(H=32, n_attr=300, V=12, S=2, w_seed=17,
                ctor=dict(w_edge_attr=True, num_layers=6, bidirectional=True, agg="attn_h", out_wx=False,
                          out_pool_all=False, out_pool="max", dropout=0.0))
    model = Hh.code2_model(meta)
    b = synth.code2_batch(9, 6, 20)
    b.x[:, 1] %= 300
    y = torch.from_numpy(np.random.default_rng(2).integers(0, 12, size=(6, 2)))
    loss_ref, ref = O.code2_grads(model.state_dict(), b.clone(), y, num_layers=6, bidirectional=True, max_seq_len=2)
    model = model.to(device)
    loss, grads = _train_step(model, b.clone().to(device), y.to(device))
    model.check()
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    for k, g in grads.items():
        scale = float(ref[k].abs().max())
        assert Hh.maxdiff(g, ref[k]) <= 1e-4 * scale + 2e-7, k


def test_training_step_edge_cases_match_oracle_autograd(device):
    """Gradients on the degenerate graphs of `test_edge_cases` (single nodes, no edges, a chain, 200-way fan-in
    and fan-out, duplicate edges; attention ties in the max read-out) and with a w_edge_attr=False model."""
    from dagnn_amd import GraphData
    from dagnn_amd.dag_utils import add_order_info_01

    def g(n, edges, attr=None):
        ei = torch.tensor(edges, dtype=torch.long).t().reshape(2, -1)
        ea = torch.zeros(ei.shape[1], 2) if attr is None else torch.tensor(attr, dtype=torch.float32)
        d = GraphData(x=torch.stack([torch.arange(n) % 98, (7 * torch.arange(n)) % 300], 1),
                      node_depth=(torch.arange(n) % 30).view(-1, 1), edge_index=ei, edge_attr=ea)
        add_order_info_01(d)
        return d

    graphs = [g(1, []), g(5, []), g(40, [(i, i + 1) for i in range(39)]),
              g(201, [(i, 200) for i in range(200)], [[i % 2, 0] for i in range(200)]),
              g(201, [(0, i) for i in range(1, 201)], [[(i // 3) % 2, 0] for i in range(200)]),
              g(3, [(0, 1), (0, 1), (1, 2)], [[0, 0], [1, 0], [0, 0]])]
    b = synth.GraphBatch.from_data_list(graphs)
    y = torch.from_numpy(np.random.default_rng(8).integers(0, 16, size=(len(graphs), 5)))
    for wea in (True, False):
        meta = dict(H=64, n_attr=300, V=16, S=5, w_seed=91 + wea,
                    ctor=dict(w_edge_attr=wea, num_layers=2, bidirectional=True, agg="attn_h", out_wx=False,
                              out_pool_all=False, out_pool="max", dropout=0.0))
        model = Hh.code2_model(meta)
        loss_ref, ref = O.code2_grads(model.state_dict(), b.clone(), y, num_layers=2, bidirectional=True, max_seq_len=5)
        model = model.to(device)
        loss, grads = _train_step(model, b.clone().to(device), y.to(device))
        assert abs(float(loss) - float(loss_ref)) < 1e-5
        for k, gk in grads.items():
            scale = float(ref[k].abs().max())
            assert Hh.maxdiff(gk, ref[k]) <= 1e-4 * scale + 2e-7, (wea, k)


def test_training_and_inference_forward_agree(device):
    meta, arr = Hh.load("grad_h32_bidir")
    model = Hh.code2_model(meta).to(device)
    with torch.no_grad():
        ref = model(Hh.code2_batch(arr, device))
    out = model.train()(Hh.code2_batch(arr, device))
    assert all(torch.equal(a, b) or Hh.maxdiff(a, b) < 1e-6 for a, b in zip(ref, out))
    assert out[0].requires_grad


# ----------------------------------------------------------------------------- loader-side plan
@pytest.mark.parametrize("seed,B,mean_n", [(2, 17, 60), (0, 128, 125), (5, 1, 12), (6, 3, 11), (7, 64, 14), (8, 300, 20),
                                           (11, 150, 4), (12, 2, 900), (13, 1, 1500), (-1, 6, 0)])
@pytest.mark.parametrize("small", [1, 0])   # 1: batches of <= 2048 nodes on the one-workgroup build (csrc/small.hip)
def test_host_plan_equals_device_plan_word_for_word(device, monkeypatch, seed, B, mean_n, small):
    from dagnn_amd import host_plan
    monkeypatch.setattr(engine, "PLAN_SMALL", small)
    b = _degenerate_batch() if seed < 0 else synth.code2_batch(seed, B, mean_n)   # -1: single nodes, no edges, stars
    plan = engine.build_plan(b.edge_index.to(device), b._bi_layer_idx0.to(device), b._bi_layer_idx1.to(device),
                             b.batch.to(device), B, b.edge_attr.to(device))
    torch.cuda.synchronize()
    dev_words = plan.ws.cpu().numpy()
    ws, sched, splits, written = host_plan.build_plan_host(b.edge_index, b._bi_layer_idx0, b._bi_layer_idx1, b.batch, B,
                                                   b.edge_attr, return_written=True)
    assert ws.shape == dev_words.shape
    assert written.sum() > 0.5 * ws.shape[0] - 32 * b.x.shape[0] - 64
    assert np.array_equal(ws[written], dev_words[written])
    for d in (0, 1):
        assert np.array_equal(sched[d], plan.read_schedule()[d])


@pytest.mark.parametrize("seed,B,mean_n,G", [(2, 17, 60, 5), (0, 128, 125, 10), (5, 1, 12, 1), (7, 64, 14, 21), (8, 300, 20, 8),
                                             (12, 2, 900, 2), (13, 1, 1500, 1), (-1, 6, 0, 3), (0, 128, 125, 0)])
@pytest.mark.parametrize("small", [1, 0])
def test_fused_prepare_equals_the_separate_calls_word_for_word(device, monkeypatch, seed, B, mean_n, G, small):
    """`dagnn_prepare` (csrc/prepare.hip: plan + schedule + encoder rows + index stack in 7 launches, several device bodies per
    launch) against `dagnn_plan_build` + `dagnn_dataflow_schedule` + `dagnn_encode_ast`: both workspaces start from the same
    fill pattern, so every word outside the build's `cursor` scratch must come out the same; the rows bit for bit."""
    monkeypatch.setattr(engine, "PLAN_SMALL", small)
    b = _degenerate_batch() if seed < 0 else synth.code2_batch(seed, B, mean_n)
    N = b.x.shape[0]
    dev = lambda t: t.to(device)   # noqa: E731
    # edge features: the two of ogbg-code2, none (seed 5), three (seed 7: beyond the FAST form of plan_graph_body)
    ea = None if seed == 5 else torch.cat([b.edge_attr, b.edge_attr[:, :1] * 0.5 + 0.25], 1) if seed == 7 else b.edge_attr
    args = (dev(b.edge_index), dev(b._bi_layer_idx0), dev(b._bi_layer_idx1), dev(b.batch), B, None if ea is None else dev(ea))
    gen = torch.Generator().manual_seed(3)
    tabs = [[dev(torch.randn(r, w, generator=gen)) for r in (98, 10030, 21)] for w in (64, 192)]
    x = dev(torch.stack([torch.randint(0, 98, (N,), generator=gen), torch.randint(0, 10030, (N,), generator=gen)], 1))
    depth0 = torch.randint(0, 40, (N,), generator=gen)
    srcs = [dev(t) for t in (b._bi_layer_idx0, b._bi_layer_index0, b._bi_layer_idx1, b._bi_layer_index1)]

    def words(plan, fused):
        plan.ws.fill_(-7)
        sched = None
        if G > 0:
            sched = plan.dataflow_schedule(G, launch=False)
            sched.fill_(-7)
        depth = dev(depth0.clone())
        if fused:
            outs = [torch.empty(N, w, device=device) for w in (64, 192)]
            stack = torch.empty(4, N, dtype=torch.int64, device=device)
            plan.launch_prepare(G, enc=(x, depth, 20, [(t[0], t[1], t[2], o) for t, o in zip(tabs, outs)]), stack=(srcs, stack))
        else:
            plan.launch_build()
            if G > 0:
                plan.dataflow_schedule(G)
            outs = [engine.encode_ast(x, depth, t[0], t[1], t[2], 20) for t in tabs]
            stack = torch.stack(srcs, 0)
        torch.cuda.synchronize()
        assert int(plan.status[0]) == 0
        return plan.ws.cpu().numpy(), None if sched is None else plan.dataflow_schedule(G).cpu().numpy(), outs, stack, depth

    ref_plan = engine.build_plan(*args, launch=False)
    ref = words(ref_plan, False)
    got = words(engine.build_plan(*args, launch=False), True)
    lay = ref_plan.layout()
    c0, c1 = lay["slot1"] + (N + 3) // 4 * 4, lay["eidx0"]   # the two `cursor` arrays: scratch of the build (the fused item ranking needs none)
    assert np.array_equal(ref[0][:c0], got[0][:c0]) and np.array_equal(ref[0][c1:], got[0][c1:])
    if G > 0:
        assert np.array_equal(ref[1], got[1])
    for a, c in zip(ref[2], got[2]):
        assert torch.equal(a, c)
    assert torch.equal(ref[3], got[3]) and torch.equal(ref[4], got[4]) and int(got[4].max()) <= 20


def test_plan_of_graphs_beyond_the_lds_paths(device, monkeypatch):
    """`plan_graph_body` has three forms: FAST (<= 1024 nodes, <= 2048 edges: everything read once, placement by LDS masks), SMALL
    (<= 2048 nodes: LDS arrays, the trip-per-key placement) and the global-memory form.  One batch with a graph of each kind
    (a 700-node and a 1500-node AST-like tree with skip edges, a 5000-node path with skip edges) - separate calls and the fused
    pipeline against the host build, word for word."""
    from dagnn_amd import GraphData, host_plan
    from dagnn_amd.dag_utils import add_order_info_01
    monkeypatch.setattr(engine, "PLAN_SMALL", 0)

    def g(n, step):
        ei = torch.cat([torch.stack([torch.arange(n - 1), torch.arange(1, n)]),
                        torch.stack([torch.arange(0, n - step, 3), torch.arange(step, n, 3)])], 1)
        ea = (torch.arange(ei.shape[1] * 2) % 2).float().view(-1, 2)
        d = GraphData(x=torch.stack([torch.arange(n) % 98, torch.arange(n) % 300], 1), node_depth=(torch.arange(n) % 30).view(-1, 1),
                      edge_index=ei, edge_attr=ea)
        add_order_info_01(d)
        return d

    b = synth.GraphBatch.from_data_list([g(700, 5), g(1500, 7), g(5000, 11), g(30, 2)])
    B, N = 4, b.x.shape[0]
    args = [t.to(device) for t in (b.edge_index, b._bi_layer_idx0, b._bi_layer_idx1, b.batch)] + [B, b.edge_attr.to(device)]
    ws, sched, splits, written = host_plan.build_plan_host(b.edge_index, b._bi_layer_idx0, b._bi_layer_idx1, b.batch, B, b.edge_attr,
                                                          return_written=True)
    for fused in (False, True):
        plan = engine.build_plan(*args, launch=not fused)
        if fused:
            plan.launch_prepare(3)
        torch.cuda.synchronize()
        assert int(plan.status[0]) == 0
        assert np.array_equal(ws[written], plan.ws.cpu().numpy()[written]), fused
        for d in (0, 1):
            assert np.array_equal(sched[d], plan.read_schedule()[d])


def _schedule_words_equal(host, dev, lay, G, whole):
    """Tables word for word; records over what the groups use (`whole`: and the -1 fill of the unused tail)."""
    assert host.shape == dev.shape
    assert np.array_equal(host[:lay["grec0"]], dev[:lay["grec0"]])
    ends = [lay["grec1"], lay["total"]]
    for d in (0, 1):
        gtab = host[lay["gtab%d" % d]:lay["gtab%d" % d] + 2 * G]
        used = 16 * int(gtab[2 * (G - 1)] + 4 * gtab[2 * (G - 1) + 1])
        g0 = lay["grec%d" % d]
        assert np.array_equal(host[g0:g0 + used], dev[g0:g0 + used])
        if whole:
            assert np.array_equal(host[g0:ends[d]], dev[g0:ends[d]])


@pytest.mark.parametrize("small", [1, 0])   # 1: batches of <= 2048 nodes on the one-workgroup builds (csrc/small.hip)
@pytest.mark.parametrize("seed,B,mean_n,G", [(2, 17, 60, 5), (0, 128, 125, 5), (5, 1, 12, 1), (7, 64, 14, 21), (8, 300, 20, 8),
                                             (9, 40, 4, 6), (10, 7, 4, 16),   # every graph 11 nodes: the round-robin deal
                                             (11, 150, 4, 64), (12, 2, 900, 2), (13, 1, 1500, 3), (-1, 6, 0, 3)])
def test_dataflow_schedule_host_equals_device_word_for_word(device, monkeypatch, seed, B, mean_n, G, small):
    """`dagnn_dataflow_schedule` (LPT groups, group-ordered padded records) against its numpy mirror."""
    from dagnn_amd import host_plan
    monkeypatch.setattr(engine, "PLAN_SMALL", small)
    b = _degenerate_batch() if seed < 0 else synth.code2_batch(seed, B, mean_n)
    plan = engine.build_plan(b.edge_index.to(device), b._bi_layer_idx0.to(device), b._bi_layer_idx1.to(device),
                             b.batch.to(device), B, b.edge_attr.to(device))
    dev = plan.dataflow_schedule(G).cpu().numpy()
    ws = host_plan.build_plan_host(b.edge_index, b._bi_layer_idx0, b._bi_layer_idx1, b.batch, B, b.edge_attr)[0]
    N, E = b.x.shape[0], b.edge_index.shape[1]
    host = host_plan.build_dataflow_schedule_host(ws, N, E, B, 2, G, engine.DF_COST_LAYER, engine.DF_COST_ROW)
    assert plan.dataflow_layout(G) == host_plan.dataflow_layout(N, B, G)
    lib_small = bool(small) and bool(engine._lib.load().dagnn_plan_is_small(N, 0, B))
    _schedule_words_equal(host, dev, plan.dataflow_layout(G), G, whole=not lib_small)


@pytest.mark.parametrize("n_graphs,kind", [(64, "enas"), (128, "bn"), (1, "enas"), (200, "bn")])
def test_small_builds_equal_the_general_kernels_on_dvae_batches(device, monkeypatch, n_graphs, kind):
    """The D-VAE batches (uniform graphs, no edge features): plan and schedule of csrc/small.hip against plan.hip /
    dataflow.hip's kernels, and both against the host mirror."""
    from dagnn_amd import host_plan
    rows = synth.enas_rows(3, n_graphs) if kind == "enas" else synth.bn_rows(3, n_graphs)
    dec = synth.decode_enas_row if kind == "enas" else synth.decode_bn_row
    b = synth.dvae_batch([dec(r) for r in rows])
    N, E, B = b.x.shape[0], b.edge_index.shape[1], n_graphs
    bl = b.bi_layer_index
    G = min(10, B)
    got = []
    for small in (1, 0):
        monkeypatch.setattr(engine, "PLAN_SMALL", small)
        plan = engine.build_plan(b.edge_index.to(device), bl[0][0].to(device), bl[1][0].to(device), b.batch.to(device), B, None)
        sched = plan.dataflow_schedule(G).cpu().numpy()
        plan.check_status()
        got.append((plan.ws.cpu().numpy(), sched, plan.dataflow_layout(G)))
    ws, _, _, written = host_plan.build_plan_host(b.edge_index, bl[0][0], bl[1][0], b.batch, B, None, return_written=True)
    host = host_plan.build_dataflow_schedule_host(ws, N, E, B, 0, G, engine.DF_COST_LAYER, engine.DF_COST_ROW)
    for words, sched, lay in got:
        assert np.array_equal(ws[written], words[written])
    _schedule_words_equal(host, got[0][1], got[0][2], G, whole=False)
    _schedule_words_equal(host, got[1][1], got[1][2], G, whole=True)


def test_dataflow_with_loader_side_schedule(device, monkeypatch):
    """`attach_plan(..., dataflow_groups=G)`: plan AND dataflow schedule from the loader - the forward pass launches
    neither the plan nor the schedule kernels and gives bitwise the same logits."""
    from dagnn_amd.host_plan import attach_plan
    monkeypatch.setattr(engine, "DATAFLOW", 1)
    model = _headline_model(H=128, L=2, V=32, seed=5).to(device)
    graphs = synth.code2_graphs(21, 40, 50)
    plain = synth.GraphBatch.from_data_list(graphs).to(device)
    G = engine.dataflow_groups(device, 2, 2, 128, 40)
    assert G > 0
    planned = attach_plan(synth.GraphBatch.from_data_list(graphs), dataflow_groups=G, cost_layer=engine.DF_COST_LAYER,
                          cost_row=engine.DF_COST_ROW).to(device)
    lib = engine._lib.load()
    with torch.no_grad():
        a = model(plain.clone())
        calls = []
        orig = lib.dagnn_dataflow_schedule

        def spy(*args):
            calls.append(1)
            return orig(*args)
        monkeypatch.setattr(lib, "dagnn_dataflow_schedule", spy, raising=False)
        bb = model(planned.clone())
    assert not calls
    assert all(torch.equal(x, y) for x, y in zip(a, bb))


def test_device_side_failures_raise(device, monkeypatch):
    """A bounded device-side wait that expires (here: a spin budget of one poll) and a batch that violates the plan
    contract (unsorted `batch` vector) both surface as DagnnHipError - at the latest at the next forward pass, with
    no synchronisation on the healthy path."""
    monkeypatch.setattr(engine, "DATAFLOW", 1)
    model = _headline_model(H=64, L=2, V=16, seed=3).to(device)
    b = synth.code2_batch(4, 24, 60)
    with torch.no_grad():
        model(b.clone().to(device))
        monkeypatch.setattr(engine, "SPIN_LIMIT", 1)
        model(b.clone().to(device))          # every dependent poll gives up at once: garbage, flagged
        torch.cuda.synchronize()
        monkeypatch.setattr(engine, "SPIN_LIMIT", 0)
        with pytest.raises(DagnnHipError, match="bounded device-side wait"):
            model(b.clone().to(device))
            torch.cuda.synchronize()
            model(b.clone().to(device))
        torch.cuda.synchronize()
        out = model(b.clone().to(device))     # the flag was consumed: healthy again
        ref = model(b.clone().to(device))
        assert all(torch.equal(x, y) for x, y in zip(out, ref))
        bad = b.clone().to(device)
        bad.batch = bad.batch.flip(0).contiguous()
        with pytest.raises(DagnnHipError, match="plan contract"):
            try:
                model(bad)
            except DagnnHipError:
                raise
            torch.cuda.synchronize()
            model(b.clone().to(device))


def test_data_parallel_shim_runs_the_first_batch_on_the_gpu(device):
    """`dagnn_amd.DataParallel(model)(list_of_batches)` on one device = `model(list[0].to(device))`
    (`tg/data_parallel.py:48-50`), batches handed over on the host as the reference's loader does; and one launch of
    the k max read-out jobs equals k launches of one job (the job index picks the right matrix, scope and columns)."""
    from dagnn_amd import DataParallel, collate_sharded
    model = _headline_model(H=64, L=2, V=16, seed=5).to(device)
    graphs = synth.code2_graphs(9, 10, 40)
    shards = collate_sharded(graphs, 2)
    dp = DataParallel(model)
    assert dp.src_device.type == "cuda"
    with torch.no_grad():
        a = dp([s.clone() for s in shards])
        b = model(shards[0].clone().to(device))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    G = shards[0].clone().to(device)
    with torch.no_grad():
        model(G)
    plan = engine.build_plan(G.edge_index, G._bi_layer_idx0, G._bi_layer_idx1, G.batch, shards[0].num_graphs, G.edge_attr)
    hs = [G.h[d][i] for d in range(2) for i in range(2)]
    one = torch.zeros(shards[0].num_graphs, 4 * 64, device=device)
    many = torch.zeros_like(one)
    engine.readout_pool_batch(plan, [(h, k // 2, "max", 64 * k) for k, h in enumerate(hs)], one)
    for k, h in enumerate(hs):
        engine.readout_pool_batch(plan, [(h, k // 2, "max", 64 * k)], many)
    assert torch.equal(one, many)


def test_loader_side_plan_with_edge_features_the_model_does_not_use(device):
    """`collate_with_plan` packs `edge_attr` into the plan; a model built with `w_edge_attr=False` has no gain for
    them: forward and the training step then build the plan on the device without the features (same results as
    the plain batch) instead of failing in `dagnn_backward_prepare`."""
    from dagnn_amd import collate_with_plan
    meta = dict(H=64, n_attr=300, V=40, S=3, w_seed=79,
                ctor=dict(w_edge_attr=False, num_layers=2, bidirectional=True, agg="attn_h", out_wx=False,
                          out_pool_all=False, out_pool="max", dropout=0.0))
    model = Hh.code2_model(meta).to(device)
    graphs = synth.code2_graphs(34, 12, 40)
    for g in graphs:
        g.x[:, 1] %= 300
    plain = synth.GraphBatch.from_data_list(graphs).to(device)
    planned = collate_with_plan(graphs).to(device)
    assert planned._dagnn_plan_meta["R"] == 2
    with torch.no_grad():
        a, bb = model(plain.clone()), model(planned.clone())
    assert all(torch.equal(x, y) for x, y in zip(a, bb))
    y = torch.randint(0, 40, (12, 3), generator=torch.Generator().manual_seed(2)).to(device)
    _, g1 = _train_step(model, plain.clone(), y)
    _, g2 = _train_step(model, planned.clone(), y)
    for k in g1:
        if "encoder." not in k:   # (torch's embedding backward accumulates with atomics: not bitwise repeatable)
            assert torch.equal(g1[k], g2[k]), k
        else:
            assert torch.allclose(g1[k], g2[k], atol=1e-6), k


def test_forward_and_training_with_loader_side_plan(device):
    """`collate_with_plan` batches: no plan kernels, no device->host read, bitwise the same results."""
    from dagnn_amd import collate_with_plan
    meta = dict(H=64, n_attr=300, V=40, S=3, w_seed=78,
                ctor=dict(w_edge_attr=True, num_layers=2, bidirectional=True, agg="attn_h", out_wx=False,
                          out_pool_all=False, out_pool="max", dropout=0.0))
    model = Hh.code2_model(meta).to(device)
    graphs = synth.code2_graphs(33, 20, 60)
    for g in graphs:
        g.x[:, 1] %= 300
    plain = synth.GraphBatch.from_data_list(graphs).to(device)
    planned = collate_with_plan(graphs).to(device)
    assert planned._dagnn_plan.is_cuda and planned._dagnn_plan.dtype == torch.int32
    with torch.no_grad():
        a = model(plain.clone())
        calls = []
        orig = engine.build_plan
        engine.build_plan = lambda *x, **k: calls.append(1) or orig(*x, **k)
        try:
            bb = model(planned.clone())
        finally:
            engine.build_plan = orig
    assert not calls
    assert all(torch.equal(x, y) for x, y in zip(a, bb))
    y = torch.randint(0, 40, (20, 3), generator=torch.Generator().manual_seed(2)).to(device)
    _, g1 = _train_step(model, plain.clone(), y)
    _, g2 = _train_step(model, planned.clone(), y)
    for k in g1:
        if "encoder." not in k:
            assert torch.equal(g1[k], g2[k]), k


# ----------------------------------------------------------------------------- device top_sort
@pytest.mark.parametrize("name", ["code2_h32_bidir", "code2_h128_deep", "code2_h256_bidir"])
def test_device_layering_matches_reference_top_sort(device, name):
    """csrc/toposort.hip against the layer ids the REFERENCE's top_sort produced for the fixtures."""
    from dagnn_amd import dag_utils
    meta, arr = Hh.load(name)
    G = Hh.code2_batch(arr, device)
    G._bi_layer_idx0 = G._bi_layer_idx1 = None
    dag_utils.add_order_info_batch(G, check=True)
    assert np.array_equal(G._bi_layer_idx0.cpu().numpy(), arr["layer0"])
    assert np.array_equal(G._bi_layer_idx1.cpu().numpy(), arr["layer1"])
    assert torch.equal(G._bi_layer_index0, torch.arange(arr["x"].shape[0], device=device))


def test_device_layering_full_batch_big_graph_and_cycle(device):
    from dagnn_amd import dag_utils
    b = synth.code2_batch(0, 128).to(device)
    lf, lb, status = engine.topo_layers(b.edge_index, b.batch, 128)
    assert torch.equal(lf, b._bi_layer_idx0) and torch.equal(lb, b._bi_layer_idx1) and int(status) == 0
    # one graph beyond the LDS capacity (global-memory path): a 9000-node path with skip edges
    n = 9000
    ei = torch.cat([torch.stack([torch.arange(n - 1), torch.arange(1, n)]),
                    torch.stack([torch.arange(0, n - 7, 5), torch.arange(7, n, 5)])], 1)
    ref0 = dag_utils.longest_path_layers(ei.numpy(), n)
    ref1 = dag_utils.longest_path_layers(ei.numpy()[::-1], n)
    lf, lb, status = engine.topo_layers(ei.to(device), torch.zeros(n, dtype=torch.long, device=device), 1)
    assert np.array_equal(lf.cpu().numpy(), ref0) and np.array_equal(lb.cpu().numpy(), ref1) and int(status) == 0
    cyc = torch.tensor([[0, 1, 2], [1, 2, 0]], device=device)
    _, _, status = engine.topo_layers(cyc, torch.zeros(3, dtype=torch.long, device=device), 1)
    assert int(status) & 16


# ----------------------------------------------------------------------------- decoder-side single-vertex step (f4)
@pytest.mark.parametrize("name", ["iprop_na_h64_L2", "iprop_bn_h32_L3"])
def test_ipropagate_to_matches_reference_on_the_gpu(device, name):
    """`_ipropagate_to(G, v, self.grud)` of both D-VAE encoders as ONE HIP launch per decoder step
    (`dagnn_iprop_step`) against the reference's own (`dvae/dagnn.py:187-239`, `dvae/dagnn_bn.py:179-238`): returned
    states, the states written into the vertices, a vertex without predecessors, graphs too short for `v`, the
    `H`-given form - and against the CPU restatement in oracle/."""
    from oracle.iprop_oracle import ipropagate_to
    Hh.check_ipropagate(name, lambda model, G, v, H=None: model._ipropagate_to(G, v, model.grud, H=H), device, 5e-6)
    meta, arr = Hh.load(name)
    model, _ = Hh.dvae_model(dict(meta, bidir=False))
    v = meta["vs"][-1]
    with torch.no_grad():
        ref = ipropagate_to(model, Hh.iprop_graphs(meta, arr, "cpu"), v, model.grud)
        got = model.to(device)._ipropagate_to(Hh.iprop_graphs(meta, arr, device), v, model.grud)
    assert Hh.maxdiff(got, ref.numpy()) < 5e-6


@pytest.mark.parametrize("name", ["iprop_na_h64_L2", "iprop_bn_h32_L3"])
def test_ipropagate_to_is_differentiable(device, name):
    """The training caller of `_ipropagate_to` (`dvae/models_pyg.py:398-442`: `loss()` -> `_update_iv`) backpropagates
    through the returned states into `grud`, `attn_lin` and the predecessors' states.  The HIP step under autograd against
    autograd through the CPU restatement: every parameter gradient and the gradient of every predecessor state, also
    for the `H`-given form; under `no_grad` the step stays the bare launch."""
    from oracle.iprop_oracle import ipropagate_to
    import copy
    meta, arr = Hh.load(name)
    model, _ = Hh.dvae_model(dict(meta, bidir=False))
    ref_model = copy.deepcopy(model)
    model = model.to(device)
    v = meta["vs"][-1]

    def run(m, dev, H):
        G = Hh.iprop_graphs(meta, arr, dev)
        leaves = []
        for g in G:
            for u in range(g.vcount()):
                for l in range(meta["L"]):
                    t = g.vs[u]["H_forward%d" % l].requires_grad_(True)
                    leaves.append(t)
        if H is not None:
            H = H.detach().clone().to(dev).requires_grad_(True)
        step = (lambda: m._ipropagate_to(G, v, m.grud, H=H)) if dev != "cpu" else (lambda: ipropagate_to(m, G, v, m.grud, H=H))
        out = step()
        assert out.requires_grad
        wts = torch.linspace(-1.0, 1.0, out.numel()).view_as(out).to(out.device)
        # the states written into the vertices carry the graph as well (the decoder reads them in later steps)
        extra = sum((g.vs[v]["H_forward0"] * 0.5).sum() for g in G if g.vcount() > v)
        ((out * wts).sum() + extra).backward()
        pg = {k: (p.grad.detach().cpu().clone() if p.grad is not None else None) for k, p in m.named_parameters()}
        lg = [None if t.grad is None else t.grad.detach().cpu().clone() for t in leaves]
        hg = None if H is None else H.grad.detach().cpu().clone()
        m.zero_grad()
        return out.detach().cpu(), pg, lg, hg

    for H in (None, torch.from_numpy(arr["H_given"].copy())):
        out_r, pg_r, lg_r, hg_r = run(ref_model, "cpu", H)
        out_g, pg_g, lg_g, hg_g = run(model, device, H)
        assert float((out_r - out_g).abs().max()) < 5e-6
        touched = 0
        for k, r in pg_r.items():
            g = pg_g[k]
            if r is None or float(r.abs().max()) < 1e-6:   # (bias of attn_lin: exact zeros here, ~1e-9 noise in the oracle)
                assert g is None or float(g.abs().max()) < 1e-6, k
                continue
            assert g is not None, k
            scale = float(r.abs().max())
            assert float((g - r).abs().max()) <= 1e-4 * scale + 1e-7, k
            touched += 1
        assert touched >= 4 * meta["L"] + (1 if H is None else 0)
        for r, g in zip(lg_r, lg_g):
            if r is None:
                assert g is None or float(g.abs().max()) == 0.0
            else:
                assert g is not None and float((g - r).abs().max()) <= 1e-4 * float(r.abs().max()) + 1e-7
        if H is not None:
            assert float((hg_g - hg_r).abs().max()) <= 1e-4 * float(hg_r.abs().max()) + 1e-7
    with torch.no_grad():
        assert not model._ipropagate_to(Hh.iprop_graphs(meta, arr, device), v, model.grud).requires_grad


def test_check_raises_for_the_last_forward_of_a_loop(device, monkeypatch):
    """A device-side failure of the LAST forward of a loop has no next forward to report it: `model.check()` (and the
    `DataParallel` wrapper in eval mode, which calls it) raises; earlier healthy passes of the same async loop do not
    mask it, and the flag is consumed."""
    from dagnn_amd import DataParallel
    monkeypatch.setattr(engine, "DATAFLOW", 1)
    model = _headline_model(H=64, L=2, V=16, seed=3).to(device).eval()
    b = synth.code2_batch(4, 24, 60)
    with torch.no_grad():
        for _ in range(3):
            model(b.clone().to(device))
        model.check()                         # healthy: returns
        monkeypatch.setattr(engine, "SPIN_LIMIT", 1)
        model(b.clone().to(device))           # every dependent poll gives up at once: garbage, flagged
        monkeypatch.setattr(engine, "SPIN_LIMIT", 0)
        with pytest.raises(DagnnHipError, match="bounded device-side wait"):
            model.check()
        model.check()                         # consumed
        out = model(b.clone().to(device))
        ref = model(b.clone().to(device))
        model.check()
        assert all(torch.equal(x, y) for x, y in zip(out, ref))
        dp = DataParallel(model, device_ids=[torch.cuda.current_device()]).eval()
        monkeypatch.setattr(engine, "SPIN_LIMIT", 1)
        with pytest.raises(DagnnHipError, match="bounded device-side wait"):
            dp([b.clone()])
        monkeypatch.setattr(engine, "SPIN_LIMIT", 0)
        dp([b.clone()])


# ----------------------------------------------------------------------------- concurrency stress
def test_back_to_back_forwards_and_steps_are_race_free(device):
    """Split mode runs the persistent kernel on a side stream next to the per-layer launches, and nothing in
    `forward` synchronises except the schedule read-back: 150 forwards and 20 training steps issued back to back
    (buffers recycled by the caching allocator every iteration) must reproduce the first result bit for bit, and no
    bounded wait may have expired."""
    from bench import build_model, fresh_inputs
    model = build_model(64, 2, 48, 3, device)
    master = synth.code2_batch(5, 96, 110).to(device)
    ins = fresh_inputs(master, 150)
    with torch.no_grad():
        first = [o.clone() for o in model(ins[0])]
        for g in ins[1:]:
            out = model(g)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, out))
    for arena in model._arenas.values():
        arena.check()
    y = torch.randint(0, 48, (96, 3), generator=torch.Generator().manual_seed(4)).to(device)
    ref = None
    for g in fresh_inputs(master, 20):
        _, grads = _train_step(model, g, y)
        cell = {k: v.clone() for k, v in grads.items() if "encoder." not in k}
        if ref is None:
            ref = cell
    torch.cuda.synchronize()
    assert all(torch.equal(ref[k], cell[k]) for k in ref)
    for arena in model._arenas.values():
        arena.check()


# ----------------------------------------------------------------------------- D-VAE encoders under autograd
@pytest.mark.parametrize("name", Hh.DVAE_GRAD)
def test_dvae_encoder_gradients_match_reference_golden(device, name):
    """`encode(list_of_graphs)` of DAGNN_NA / DAGNN_BN under autograd (dvae/dagnn.py:177-184): loss and the gradients
    of every encoder parameter against the reference's own `.backward()`."""
    meta, arr = Hh.load(name)
    model, nn_ = Hh.dvae_model(meta)
    model = model.to(device).train()
    graphs = Hh.dvae_graphs(meta, arr)
    mu, logvar = model.encode([g.clone() for g in graphs])
    assert Hh.maxdiff(mu, arr["mu"]) < TOL and Hh.maxdiff(logvar, arr["logvar"]) < TOL
    loss = (mu * torch.from_numpy(arr["r1"]).to(device)).sum() + (logvar * torch.from_numpy(arr["r2"]).to(device)).sum()
    model.zero_grad(set_to_none=True)
    loss.backward()
    assert abs(float(loss.detach()) - float(arr["loss"])) < 1e-4 * max(1.0, abs(float(arr["loss"])))
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    sd = model.state_dict()
    for k in list(grads):   # aliased encoder GRUs (cells_d == grue_forward / grue_backward)
        for k2, v2 in sd.items():
            if k2 not in grads and v2.data_ptr() == sd[k].data_ptr():
                grads[k2] = grads[k]
    assert Hh.check_grads(meta, arr, grads, rtol=1e-4) < 1e-4


@pytest.mark.parametrize("name", ["code2_h64_attn_x", "code2_h64_self_attn_h", "code2_h64_self_attn_x"])
def test_training_step_other_additive_aggregators_match_oracle_autograd(device, name):
    """The other additive-attention aggregators (keys from the inputs: static scores; no query) under autograd,
    against autograd through the oracle (itself pinned against the reference's forward for these aggregators)."""
    meta, arr = Hh.load(name)
    kw = meta["ctor"]
    model = Hh.code2_model(meta)
    y = torch.from_numpy(np.random.default_rng(3).integers(0, meta["V"], size=(int(arr["batch"].max()) + 1, meta["S"])))
    loss_ref, ref = O.code2_grads(model.state_dict(), Hh.code2_batch(arr), y, num_layers=kw["num_layers"],
                                  bidirectional=True, out_wx=kw["out_wx"], max_seq_len=meta["S"], agg=kw["agg"])
    model = model.to(device)
    loss, grads = _train_step(model, Hh.code2_batch(arr, device), y.to(device))
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    for k, g in grads.items():
        scale = float(ref[k].abs().max())
        assert Hh.maxdiff(g, ref[k]) <= 1e-4 * scale + 2e-7, k


@pytest.mark.parametrize("H,L,pad", [(512, 3, 1), (320, 2, 1), (320, 2, 0), (320, 1, 1)])
def test_training_step_wide_hidden_matches_oracle_autograd(device, monkeypatch, H, L, pad):
    """Hidden sizes beyond the register-resident path: H = 512 (streamed slice kernel, K-chunked MFMA tiles), H = 320
    stacked (zero-padded to 512 by engine.state_width, so the same kernels - and with DAGNN_AMD_TILES_PAD=0 at its own
    width, not MFMA-eligible: 8-row blocks) and H = 320 single-layer (never padded), with fat layers present."""
    monkeypatch.setattr(engine, "TILES_PAD", pad)
    assert engine.state_width(H, L, 2) == (512 if (H == 512 or (pad and L >= 2)) else 320)
    meta = dict(H=H, n_attr=300, V=24, S=2, w_seed=55,
                ctor=dict(w_edge_attr=True, num_layers=L, bidirectional=True, agg="attn_h", out_wx=False,
                          out_pool_all=False, out_pool="max", dropout=0.0))
    model = Hh.code2_model(meta)
    b = synth.code2_batch(41, 40, 60)
    b.x[:, 1] %= 300
    y = torch.from_numpy(np.random.default_rng(6).integers(0, 24, size=(40, 2)))
    loss_ref, ref = O.code2_grads(model.state_dict(), b.clone(), y, num_layers=L, bidirectional=True, max_seq_len=2)
    model = model.to(device)
    loss, grads = _train_step(model, b.clone().to(device), y.to(device))
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    for k, g in grads.items():
        scale = float(ref[k].abs().max())
        assert Hh.maxdiff(g, ref[k]) <= 1e-4 * scale + 2e-7, k


@pytest.mark.parametrize("H,L,E", [(33, 2, 64), (255, 2, 300), (501, 2, 300)])
def test_training_step_odd_hidden_sizes_match_oracle_autograd(device, H, L, E):
    """Odd hidden widths (the reference's D-VAE default is 501; nothing in `ogbg-code/model/dagnn.py` asks for an even one):
    the padded units of every path, and the weight-gradient kernel's paired input columns (engine.wgrad), on a full
    step; an embedding width that is not a multiple of 4 is refused loudly for training and runs under no_grad."""
    from dagnn_amd import DAGNN, ASTNodeEncoder

    def make(emb):
        m = DAGNN(num_vocab=24, max_seq_len=2, emb_dim=emb, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(emb, 98, 300, 20),
                  w_edge_attr=True, num_layers=L, bidirectional=True, agg="attn_h", out_wx=False, out_pool_all=False,
                  out_pool="max", dropout=0.0)
        seeded_fill(m, 77 + H)
        return m
    model = make(E)
    b = synth.code2_batch(43, 12, 40)
    b.x[:, 1] %= 300
    y = torch.from_numpy(np.random.default_rng(8).integers(0, 24, size=(12, 2)))
    loss_ref, ref = O.code2_grads(model.state_dict(), b.clone(), y, num_layers=L, bidirectional=True, max_seq_len=2)
    model = model.to(device)
    loss, grads = _train_step(model, b.clone().to(device), y.to(device))
    model.check()
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    for k, g in grads.items():
        scale = float(ref[k].abs().max())
        assert Hh.maxdiff(g, ref[k]) <= 1e-4 * scale + 2e-7, k
    odd = make(H)   # embedding as wide as the states: odd
    want = O.code2_forward(odd.state_dict(), b.clone(), num_layers=L, bidirectional=True, out_wx=False, out_pool_all=False,
                           out_pool="max", max_seq_len=2)
    odd = odd.to(device)
    with pytest.raises(NotImplementedError):
        _train_step(odd, b.clone().to(device), y.to(device))
    odd.eval()
    with torch.no_grad():
        out = odd(b.clone().to(device))
    odd.check()
    assert max(Hh.maxdiff(o, r) for o, r in zip(out, want)) < TOL


# ----------------------------------------------------------------------------- constructor-string variants (row a12)
@pytest.mark.parametrize("name", Hh.VARIANTS)
def test_variant_forward_matches_reference_golden(device, name):
    """`mattn_h`, `gated_sum` (with and without mapper bias), `add`, `max` (incl. the reference's shared-module flow in
    the reverse direction), `agg_x`, `recurr=0`: outputs and hidden rows against the reference's own forward."""
    meta, arr = Hh.load(name)
    model = Hh.code2_model(meta).to(device)
    G = Hh.code2_batch(arr, device)
    with torch.no_grad():
        out = model(G)
    assert len(out) == arr["pred"].shape[0]
    for o, ref in zip(out, arr["pred"]):
        assert Hh.maxdiff(o, ref) < TOL
    rows = arr["rows"]
    for d, hd in enumerate(G.h):
        for i, h in enumerate(hd):
            assert Hh.maxdiff(h[rows], arr["h_%d_%d" % (d, i)]) < TOL


@pytest.mark.parametrize("agg", ["add", "max"])
def test_plain_aggregators_on_the_dataflow_kernel(device, agg, monkeypatch):
    """`agg` = `add` / `max` (AggConv, dagnn.py:232-251) evaluation passes run on the persistent dataflow kernel - the generic
    loader folds the messages h_j + edge_encoder(edge_attr_j) by sum / maximum, the reverse direction aggregates nothing (the
    reference's shared module).  The reference fixture must come out of THAT path (the pass says which one it took), the
    per-layer variant launches must agree with it on a headline-shaped batch, and the result is bitwise reproducible."""
    from dagnn_amd import variants
    name = "var_h64_" + agg
    meta, arr = Hh.load(name)
    model = Hh.code2_model(meta).to(device)
    calls = []
    real = variants.run_plain_dataflow
    monkeypatch.setattr(variants, "run_plain_dataflow", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        G = Hh.code2_batch(arr, device)
        out = model(G)
    assert calls and len(out) == arr["pred"].shape[0]
    for o, ref in zip(out, arr["pred"]):
        assert Hh.maxdiff(o, ref) < TOL
    rows = arr["rows"]
    for d, hd in enumerate(G.h):
        for i, h in enumerate(hd):
            assert Hh.maxdiff(h[rows], arr["h_%d_%d" % (d, i)]) < TOL
    monkeypatch.setattr(variants, "run_plain_dataflow", real)
    # a wider model on a code2-like batch with fan-in beyond one chunk: both paths, and twice the same bits
    from dagnn_amd import DAGNN, ASTNodeEncoder
    enc = ASTNodeEncoder(128, 98, 10030, 20)
    big = DAGNN(num_vocab=32, max_seq_len=3, emb_dim=128, hidden_dim=128, out_dim=None, encoder=enc, w_edge_attr=True, num_layers=2,
                bidirectional=True, agg=agg, out_wx=False, out_pool_all=False, out_pool="max", dropout=0.0).eval()
    seeded_fill(big, 77)
    big = big.to(device)
    b = synth.code2_batch(5, 48)
    outs = {}
    for flag in (1, 0, 1):
        monkeypatch.setattr(engine, "VARIANT_DATAFLOW", flag)
        with torch.no_grad():
            Gb = b.clone().to(device)
            o = torch.stack(big(Gb))
            hs = [h.clone() for hd in Gb.h for h in hd]
        big.check()
        if flag in outs:
            assert torch.equal(outs[flag][0], o)
        outs[flag] = (o, hs)
    assert Hh.maxdiff(outs[1][0], outs[0][0]) < TOL
    for a_, b_ in zip(outs[1][1], outs[0][1]):
        assert Hh.maxdiff(a_, b_) < TOL


@pytest.mark.parametrize("name", Hh.GRAD_VAR)
def test_variant_training_step_gradients_match_reference_golden(device, name, monkeypatch):
    """`gated_sum` (with / without mapper bias), `mattn_h` (L = 2 and 3), `add`, `max`, and `gated_sum` / `mattn_h` on the
    Linear cell of `recurr=0`: forward + `loss.backward()` with the
    reverse sweep in HIP (`dagnn_variant_backward_run`, csrc/variants_bwd.hip) against the reference's own autograd on the
    same seeded step: loss and every parameter gradient; the HIP entry point really ran."""
    meta, arr = Hh.load(name)
    lib = engine._lib.load()
    calls = []
    orig = lib.dagnn_variant_backward_run

    class _Spy(object):
        def __call__(self, *a):
            calls.append(1)
            return orig(*a)
    monkeypatch.setattr(lib, "dagnn_variant_backward_run", _Spy(), raising=False)
    model = Hh.code2_model(meta).to(device)
    G = Hh.code2_batch(arr, device)
    loss, grads = _train_step(model, G, torch.from_numpy(arr["y"]).to(device))
    assert calls, "the variant's training step did not go through the HIP reverse sweep"
    assert abs(float(loss) - float(arr["loss"])) < 1e-5
    # every gradient within 1e-4 of its own largest entry + 2e-7 (check_grads asserts that); the returned worst RELATIVE
    # error is dominated by the dot-product attention's projections in the reverse direction, whose gradients are ~5e-5
    # (and down to 1e-5 with the Linear cell) in size next to 1e-2 elsewhere: 2e-8 of fp32 rounding reads as 5e-4..2e-3 there
    assert Hh.check_grads(meta, arr, grads, rtol=1e-4) < 5e-3
    loss2, grads2 = _train_step(model, Hh.code2_batch(arr, device), torch.from_numpy(arr["y"]).to(device))
    assert all(torch.equal(grads[k], grads2[k]) for k in grads if "encoder." not in k)   # deterministic


@pytest.mark.parametrize("name", ["var_h64_mattn_h", "var_h64_gated_sum", "var_h64_recurr0", "var_h64_aggx_attn_h",
                                  "var_h64_aggx_add"])
def test_variant_training_step_matches_oracle_autograd(device, name):
    meta, arr = Hh.load(name)
    kw = meta["ctor"]
    model = Hh.code2_model(meta)
    y = torch.from_numpy(np.random.default_rng(2).integers(0, meta["V"], size=(int(arr["batch"].max()) + 1, meta["S"])))
    # the reference is the float64 oracle: the bound below measures fp32 against exact arithmetic, not against another fp32 sum
    loss_ref, ref = Hh.code2_grads64(None, model, Hh.code2_batch(arr), y, num_layers=kw["num_layers"],
                                     bidirectional=True, out_wx=kw["out_wx"], max_seq_len=meta["S"], agg=kw["agg"],
                                     agg_x=kw.get("agg_x", False), recurr=kw.get("recurr", 1))
    model = model.to(device)
    loss, grads = _train_step(model, Hh.code2_batch(arr, device), y.to(device))
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    for k, g in grads.items():
        scale = float(ref[k].abs().max())
        assert Hh.maxdiff(g, ref[k]) <= 1e-4 * scale + 2e-7, k


_VARIANT_CTORS = [dict(agg="gated_sum"), dict(agg="gated_sum", mapper_bias=False), dict(agg="mattn_h"), dict(agg="add"),
                  dict(agg="max"), dict(agg="attn_h", agg_x=True), dict(agg="self_attn_h", agg_x=True),
                  dict(agg="add", agg_x=True), dict(agg="max", agg_x=True), dict(agg="gated_sum", agg_x=True),
                  dict(agg="mattn_h", agg_x=True), dict(agg="attn_h", recurr=0), dict(agg="attn_x", recurr=0),
                  dict(agg="self_attn_x", recurr=0), dict(agg="gated_sum", recurr=0), dict(agg="mattn_h", recurr=0),
                  dict(agg="max", recurr=0, agg_x=True), dict(agg="max", w_edge_attr=False),
                  dict(agg="gated_sum", w_edge_attr=False), dict(agg="mattn_h", w_edge_attr=False),
                  dict(agg="mattn_h", bidirectional=False, out_pool_all=True), dict(agg="gated_sum", num_layers=3)]


def test_variant_hip_kernels_wide_hidden(device):
    """H = 512 and 1024: 8-row workgroups, more than 64 KB of LDS per workgroup at 1024, 16 message elements per lane."""
    for H, kw in ((512, dict(agg="mattn_h")), (1024, dict(agg="gated_sum")), (1024, dict(agg="max", recurr=0))):
        _variant_hip_vs_torch(device, kw, H, graphs=6)


@pytest.mark.parametrize("H", [72, 256])
@pytest.mark.parametrize("kw", _VARIANT_CTORS, ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()))
def test_variant_hip_kernels_match_torch_ops_path(device, kw, H):
    """Every constructor-string variant through csrc/variants.hip (evaluation path) against the differentiable
    torch-ops path the fixtures pin to the reference - on a batch wide and deep enough for every launch shape,
    H = 72 (ragged last slice / lane tail) and 256."""
    _variant_hip_vs_torch(device, kw, H, graphs=24)


@pytest.mark.parametrize("kw", [dict(agg="mattn_h"), dict(agg="gated_sum"), dict(agg="max"), dict(agg="add", agg_x=True),
                                dict(agg="self_attn_h", recurr=0)],
                         ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()))
def test_variant_hip_kernels_on_degenerate_graphs(device, kw):
    """The variant kernels on single-node graphs, graphs without edges, a chain, 200-way fan-in (50 four-edge trips
    of the aggregate, online softmax) and fan-out, a duplicate edge."""
    _variant_hip_vs_torch(device, kw, 64, batch=_degenerate_batch())


def _variant_hip_vs_torch(device, kw, H, graphs=24, batch=None):
    from dagnn_amd import DAGNN, ASTNodeEncoder
    ctor = dict(num_layers=2, bidirectional=True, out_wx=True, out_pool_all=False, out_pool="max")
    ctor.update(kw)
    torch.manual_seed(11)
    model = DAGNN(num_vocab=37, max_seq_len=3, emb_dim=H, hidden_dim=H, out_dim=None,
                  encoder=ASTNodeEncoder(H, 98, 300, 20), **ctor).eval().to(device)
    b = batch if batch is not None else synth.code2_batch(77, graphs, 70)
    b.x[:, 1] %= 300
    outs, hs = [], []
    for backend in ("hip", "torch"):
        model.variant_backend = backend
        G = b.clone().to(device)
        with torch.no_grad():
            outs.append(model(G))
        hs.append(G.h)
    def close(a, r):   # sum aggregators grow with fan-in and depth: tolerance relative to the largest entry
        return Hh.maxdiff(a, r) <= TOL * max(1.0, float(r.abs().max()))

    for a, r in zip(outs[0], outs[1]):
        assert close(a, r)
    if isinstance(hs[0], list):
        for ha, hr in zip(hs[0], hs[1]):
            for a, r in zip(ha, hr):
                assert close(a, r)
    else:
        assert close(hs[0], hs[1])


def test_fused_optimizer_updates_reach_the_kernels(device):
    """`torch.optim.Adam(fused=True)` changes the parameters WITHOUT bumping their version counters; the packed
    weights the kernels read must follow anyway (core.DerivedCache): two models trained with the foreach and the
    fused optimizer stay together, in train mode and with the module left in eval mode, and the evaluation forward
    after the steps sees the new weights."""
    meta, arr = Hh.load("grad_h32_bidir")
    y = torch.from_numpy(arr["y"]).to(device) if "y" in arr else None
    outs = {}
    for fused in (False, True):
        for mode in ("train", "eval"):
            model = Hh.code2_model(meta).to(device)
            getattr(model, mode)()
            opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2, fused=fused)
            with torch.no_grad():
                before = torch.stack(model(Hh.code2_batch(arr, device)))   # fills the evaluation caches
            for _ in range(3):
                opt.zero_grad()
                pred = model(Hh.code2_batch(arr, device))
                tgt = y if y is not None else torch.zeros(pred[0].shape[0], len(pred), dtype=torch.long, device=device)
                loss = sum(torch.nn.functional.cross_entropy(p, tgt[:, s]) for s, p in enumerate(pred)) / len(pred)
                loss.backward()
                opt.step()
            with torch.no_grad():
                after = torch.stack(model(Hh.code2_batch(arr, device)))
            assert Hh.maxdiff(after, before) > 1e-3   # the steps did something
            outs[(fused, mode)] = (float(loss.detach()), after)
    for mode in ("train", "eval"):
        (l0, a0), (l1, a1) = outs[(False, mode)], outs[(True, mode)]
        assert abs(l0 - l1) < 1e-4 * max(1.0, abs(l0)), (mode, l0, l1)
        assert Hh.maxdiff(a0, a1) < 1e-3, mode


def test_batched_weight_packing_equals_single_packs(device):
    """`dagnn_pack_batch` (one launch for all matrices and layouts) writes exactly what `dagnn_pack_slices` /
    `dagnn_pack_mfma` write one matrix and one layout at a time; more matrices than one launch takes."""
    g = torch.Generator().manual_seed(4)
    for H, n in ((64, 3), (256, 18)):
        mats = [torch.randn(3 * H, H, generator=g).to(device) for _ in range(n)]
        for w, packed in zip(mats, engine.pack_batch(mats, H)):
            assert torch.equal(packed[16], engine.pack_slices(w, H, 16))
            assert torch.equal(packed[32], engine.pack_slices(w, H, 32))
            assert torch.equal(packed["mfma"], engine.pack_mfma(w, H))


def _random_ctor(rng):
    agg = str(rng.choice(["attn_h", "attn_h", "attn_x", "self_attn_h", "self_attn_x"]))
    bidir = bool(rng.integers(0, 2))
    out_pool_all = bool(rng.integers(0, 2))
    out_wx = bool(rng.integers(0, 2)) and not (bidir and out_pool_all)   # the reference's head width is wrong there
    return dict(agg=agg, bidirectional=bidir, num_layers=int(rng.integers(1, 4)), w_edge_attr=bool(rng.integers(0, 2)),
                out_wx=out_wx, out_pool_all=out_pool_all, out_pool=str(rng.choice(["max", "mean", "add", "attn"])),
                num_class=int(rng.choice([0, 0, 7])))


@pytest.mark.parametrize("case", range(24))
def test_random_configurations_match_oracle(device, case):
    """Seeded random walk over the constructor space of the HIP recurrence (aggregator, directions, 1-3 stacked
    layers, edge encoder on/off, every read-out, classification head) x hidden sizes that are not multiples of 64
    x batch shapes, forward against the oracle."""
    from dagnn_amd import DAGNN, ASTNodeEncoder
    rng = np.random.default_rng(1000 + case)
    H = int(rng.choice([20, 32, 48, 64, 100, 128, 192, 256, 300]))
    kw = _random_ctor(rng)
    B, mean_n = int(rng.integers(1, 40)), int(rng.choice([12, 30, 80]))
    b = synth.code2_batch(int(rng.integers(0, 10 ** 6)), B, mean_n)
    b.x[:, 1] %= 300
    model = DAGNN(num_vocab=11, max_seq_len=3, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(H, 98, 300, 20),
                  dropout=0.0, **kw).eval()
    seeded_fill(model, 5000 + case)
    ref = O.code2_forward(model.state_dict(), copy.deepcopy(b), num_layers=kw["num_layers"], bidirectional=kw["bidirectional"],
                          out_wx=kw["out_wx"], out_pool_all=kw["out_pool_all"], out_pool=kw["out_pool"], max_seq_len=3,
                          num_class=kw["num_class"], agg=kw["agg"])
    model = model.to(device)
    with torch.no_grad():
        out = model(b.to(device))
    out, ref = (out if isinstance(out, (list, tuple)) else [out]), (ref if isinstance(ref, (list, tuple)) else [ref])
    scale = max(1.0, max(float(r.abs().max()) for r in ref))
    assert max(Hh.maxdiff(o, r) for o, r in zip(out, ref)) < TOL * scale, (H, kw, B, mean_n)


@pytest.mark.parametrize("case", range(10))
def test_random_configurations_gradients_match_oracle(device, case):
    """The same random walk for one training step: loss and every parameter gradient against autograd through the
    oracle (multi-head models; hidden sizes that are multiples of 4)."""
    from dagnn_amd import DAGNN, ASTNodeEncoder
    rng = np.random.default_rng(2000 + case)
    H = int(rng.choice([20, 32, 64, 100, 128, 192]))
    kw = _random_ctor(rng)
    kw["num_class"] = 0
    B, mean_n = int(rng.integers(2, 24)), int(rng.choice([12, 30, 60]))
    b = synth.code2_batch(int(rng.integers(0, 10 ** 6)), B, mean_n)
    b.x[:, 1] %= 300
    model = DAGNN(num_vocab=11, max_seq_len=3, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(H, 98, 300, 20),
                  dropout=0.0, **kw).eval()
    seeded_fill(model, 6000 + case)
    y = torch.from_numpy(rng.integers(0, 11, size=(B, 3)))
    loss_ref, ref = O.code2_grads(model.state_dict(), copy.deepcopy(b), y, num_layers=kw["num_layers"],
                                  bidirectional=kw["bidirectional"], out_wx=kw["out_wx"], out_pool_all=kw["out_pool_all"],
                                  out_pool=kw["out_pool"], max_seq_len=3, agg=kw["agg"])
    model = model.to(device)
    loss, grads = _train_step(model, b.to(device), y.to(device))
    assert abs(float(loss) - float(loss_ref)) < 1e-5 * max(1.0, abs(float(loss_ref))), (H, kw)
    for k, g in grads.items():
        scale = float(ref[k].abs().max())
        assert Hh.maxdiff(g, ref[k]) <= 1e-4 * scale + 2e-7, (k, H, kw)


@pytest.mark.parametrize("case", range(10))
def test_random_dvae_encoders_match_oracle(device, case):
    """Seeded random D-VAE encoder configurations (NA with vertex-id keys / BN, 1-3 stacked layers, uni- and
    bidirectional, end-vertex read-out or pooling over all nodes, hidden sizes off the 64 grid) against the oracle."""
    from dagnn_amd import DAGNN_NA, DAGNN_BN
    rng = np.random.default_rng(3000 + case)
    na = bool(rng.integers(0, 2))
    hs = int(rng.choice([24, 56, 64, 100, 128, 200, 256]))
    L, bidir = int(rng.integers(1, 4)), bool(rng.integers(0, 2))
    pool_all = bool(rng.integers(0, 2))
    pool = str(rng.choice(["max", "mean", "add"]))
    B = int(rng.integers(1, 70))
    cls, nn_ = (DAGNN_NA, 8) if na else (DAGNN_BN, 10)
    model = cls(nn_, hs, hs, nn_, nn_, 0, 1, hs=hs, nz=56, num_nodes=nn_, agg="attn_h", num_layers=L, bidirectional=bidir,
                out_wx=False, out_pool_all=pool_all, out_pool=pool, dropout=0.0).eval()
    seeded_fill(model, 7000 + case)
    rows = (synth.enas_rows if na else synth.bn_rows)(int(rng.integers(0, 10 ** 6)), B)
    graphs = [(synth.decode_enas_row if na else synth.decode_bn_row)(r) for r in rows]
    G = synth.dvae_batch(graphs)
    ref = O.dvae_forward(model.state_dict(), copy.deepcopy(G), num_layers=L, bidirectional=bidir, num_nodes=nn_, vids=na,
                         out_pool_all=pool_all, out_pool=pool)
    model = model.to(device)
    with torch.no_grad():
        out = model(G.to(device))
    assert Hh.maxdiff(out, ref) < TOL * max(1.0, float(ref.abs().max())), (na, hs, L, bidir, pool_all, pool, B)


def test_large_batch_properties(device):
    """B = 1024 graphs (N ~ 130 k nodes, 8x the headline batch): bitwise run-to-run determinism, and the four
    256-graph quarters give the rows they give inside the big batch (to rounding)."""
    model = _headline_model(H=256, L=2, V=32, seed=3).to(device)
    graphs = synth.code2_graphs(11, 1024)
    full = synth.GraphBatch.from_data_list(graphs)
    assert full.x.shape[0] > 100000
    with torch.no_grad():
        a = torch.stack(model(full.clone().to(device)))
        b = torch.stack(model(full.clone().to(device)))
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        parts = [torch.stack(model(synth.GraphBatch.from_data_list(graphs[q:q + 256]).to(device)))
                 for q in range(0, 1024, 256)]
    assert Hh.maxdiff(torch.cat(parts, dim=1), a) < 2e-5


# ----------------------------------------------------------------------------- weight-stationary tile kernel (H = 512, csrc/tiles.hip)
def _both_paths(model, make_G, monkeypatch):
    """Logits and state rows of `model` on the tile kernel (forced) and on the per-layer launches."""
    res, ran = {}, []
    orig = engine.tiles_run
    monkeypatch.setattr(engine, "tiles_run", lambda *a, **k: (ran.append(1), orig(*a, **k))[1])
    for mode in (2, 0):
        monkeypatch.setattr(engine, "TILES", mode)
        for c in model._derived.values():
            c.invalidate()
        G = make_G()
        with torch.no_grad():
            out = model(G)
        model.check()
        hs = [h.clone() for d in G.h for h in (d if isinstance(d, (list, tuple)) else [d]) if h is not None] \
            if isinstance(G.h, (list, tuple)) else [G.h.clone()]
        res[mode] = ([o.clone() for o in (out if isinstance(out, list) else [out])], hs)
    assert ran, "the tile kernel did not run"
    return res


def test_tile_kernel_matches_reference_golden_and_launches(device, monkeypatch):
    """`code2_h512_L5` (the reference's own logits) through dagnn_tiles_run; its state rows against the per-layer launches;
    bitwise run to run."""
    meta, arr = Hh.load("code2_h512_L5")
    model = Hh.code2_model(meta).to(device)
    res = _both_paths(model, lambda: Hh.code2_batch(arr, device), monkeypatch)
    for mode in (2, 0):
        assert max(Hh.maxdiff(o, r) for o, r in zip(res[mode][0], arr["pred"])) < TOL
    assert max(Hh.maxdiff(a, b) for a, b in zip(res[2][1], res[0][1])) < 5e-6
    monkeypatch.setattr(engine, "TILES", 2)
    with torch.no_grad():
        again = model(Hh.code2_batch(arr, device))
    assert all(torch.equal(a, b) for a, b in zip(again, res[2][0]))


@pytest.mark.parametrize("kw", [dict(L=5), dict(L=3), dict(L=1), dict(L=4, bidirectional=False), dict(L=3, w_edge_attr=False)])
def test_tile_kernel_shapes_and_edge_cases(device, monkeypatch, kw):
    """Chunking (stacked layer 0 alone, the layers above together; one direction: two replicas per cell there), no edge
    features, and the degenerate graphs: single nodes, no edges, a chain, 200-way fan-in / fan-out (rows with more than two
    predecessors take further trips through the plan's CSR), duplicate edges - against the oracle and the launches."""
    from dagnn_amd import DAGNN, ASTNodeEncoder
    L = kw["L"]
    enc = ASTNodeEncoder(512, 98, 10030, 20)
    args = dict(w_edge_attr=kw.get("w_edge_attr", True), num_layers=L, bidirectional=kw.get("bidirectional", True), agg="attn_h",
                out_wx=False, out_pool_all=False, out_pool="max", dropout=0.0)
    model = DAGNN(num_vocab=16, max_seq_len=2, emb_dim=512, hidden_dim=512, out_dim=None, encoder=enc, **args).eval()
    seeded_fill(model, 4242 + L)
    b = _degenerate_batch(synth.code2_graphs(12, 10, 40))
    ref = O.code2_forward(model.state_dict(), copy.deepcopy(b), num_layers=L, bidirectional=args["bidirectional"], out_wx=False,
                          out_pool_all=False, out_pool="max", max_seq_len=2)
    model = model.to(device)
    res = _both_paths(model, lambda: copy.deepcopy(b).to(device), monkeypatch)
    assert max(Hh.maxdiff(o, r) for o, r in zip(res[2][0], ref)) < TOL
    assert max(Hh.maxdiff(a, c) for a, c in zip(res[2][0], res[0][0])) < 2e-5
    assert max(Hh.maxdiff(a, c) for a, c in zip(res[2][1], res[0][1])) < 5e-6


def test_dvae_default_width_takes_the_tile_kernel(device, monkeypatch):
    """The reference's default D-VAE width (`dvae/train.py:55`: --hs 501) is 512 wide on the lock-step path: the BN
    encoder (two stacked layers, both directions) and the NA encoder (one direction; its keys carry the vertex-id bias of
    `dvae/dagnn.py:130-134`: the kernel's VID instantiation) are ONE launch of the tile kernel each - against the
    reference's own outputs and against themselves on the per-layer launches."""
    monkeypatch.setenv("DAGNN_AMD_SCHEDULE", "lockstep")
    lib = engine._lib.load()
    calls = []
    orig = lib.dagnn_tiles_run

    class _Spy(object):
        def __call__(self, *a):
            calls.append(1)
            return orig(*a)
    monkeypatch.setattr(lib, "dagnn_tiles_run", _Spy(), raising=False)
    for name, on_tiles in (("bn_h501_bidir", True), ("na_h501_unidir", True)):
        meta, arr = Hh.load(name)
        model = Hh.dvae_model(meta)[0].to(device)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with torch.no_grad():
                Hg = model(Hh.dvae_batch(arr, device))
        model.check()
        assert bool(calls) == on_tiles, name
        calls.clear()
        assert Hh.maxdiff(Hg, arr["Hg"]) < TOL
        if on_tiles:
            monkeypatch.setattr(engine, "TILES", 0)
            for c in model._derived.values():
                c.invalidate()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                with torch.no_grad():
                    Hg0 = model(Hh.dvae_batch(arr, device))
            model.check()
            assert not calls and Hh.maxdiff(Hg, Hg0) < 2e-5
            monkeypatch.setattr(engine, "TILES", 1)
            # 384 such graphs are 384 rows in each of 8-10 layers: too flat for the tile kernel under the policy
            # (engine.tiles_batch_too_flat), which agrees with the kernel forced on
            big = synth.dvae_batch([synth.decode_bn_row(r) for r in synth.bn_rows(4, 384)] if meta["kind"] == "bn" else
                                   [synth.decode_enas_row(r) for r in synth.enas_rows(4, 384)]).to(device)
            for c in model._derived.values():
                c.invalidate()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                with torch.no_grad():
                    a = model(big.clone())
                    assert not calls
                    monkeypatch.setattr(engine, "TILES", 2)
                    b = model(big.clone())
                    assert calls
            model.check()
            calls.clear()
            assert Hh.maxdiff(a, b) < 2e-5
            monkeypatch.setattr(engine, "TILES", 1)


@pytest.mark.parametrize("H,L", [(300, 3), (448, 1), (384, 2)])
def test_hidden_sizes_between_256_and_512_run_padded_to_512(device, monkeypatch, H, L):
    """engine.state_width: a stacked model with 256 < H < 512 (and a single-layer one above 384) is zero-padded to 512 -
    the tile kernel takes the stacked ones - and nothing of the padding shows: logits and every state row against the
    oracle and against the same model at its own width (`DAGNN_AMD_TILES_PAD=0`), state rows H wide."""
    monkeypatch.setattr(engine, "DF_WIDE", 0)   # (with it, 257..320 run 320 wide on the dataflow kernel: the test below)
    model = _headline_model(H=H, L=L, V=16, seed=9)
    b = _degenerate_batch(synth.code2_graphs(17, 12, 40))
    ref = O.code2_forward(model.state_dict(), copy.deepcopy(b), num_layers=L, bidirectional=True, out_wx=False,
                          out_pool_all=False, out_pool="max", max_seq_len=5)
    model = model.to(device)
    lib = engine._lib.load()
    calls = []
    orig = lib.dagnn_tiles_run

    class _Spy(object):
        def __call__(self, *a):
            calls.append(1)
            return orig(*a)
    monkeypatch.setattr(lib, "dagnn_tiles_run", _Spy(), raising=False)
    res = {}
    for pad in (1, 0):
        monkeypatch.setattr(engine, "TILES_PAD", pad)
        for c in model._derived.values():
            c.invalidate()
        G = copy.deepcopy(b).to(device)
        with torch.no_grad():
            out = model(G)
        model.check()
        assert all(h.shape[1] == H for hd in G.h for h in hd)
        res[pad] = ([o.clone() for o in out], [h.clone() for hd in G.h for h in hd])
        if pad:
            assert engine.state_width(H, L, 2) == 512 and bool(calls) == (L >= 2)
            calls.clear()
        else:
            assert engine.state_width(H, L, 2) == (H + 63) // 64 * 64 and not calls
    assert max(Hh.maxdiff(o, r) for o, r in zip(res[1][0], ref)) < TOL
    assert max(Hh.maxdiff(a, c) for a, c in zip(res[1][0], res[0][0])) < 2e-5
    assert max(Hh.maxdiff(a, c) for a, c in zip(res[1][1], res[0][1])) < 5e-6


@pytest.mark.parametrize("H,L", [(300, 2), (300, 3), (320, 1)])
def test_hidden_sizes_up_to_320_run_on_the_wide_dataflow_kernel(device, monkeypatch, H, L):
    """Hidden sizes 257..320 (the reference trains at emb_dim = 300, scripts/ogb_tok.sh:17) run zero-padded to 320 on the
    8-wave shape of the dataflow kernel (`dagnn_dataflow_run_wide`, csrc/dataflow_w.hip): logits and every state row against
    the oracle and against the other paths (`DAGNN_AMD_DF_WIDE=0`), bitwise run to run, on a batch with fan-in / fan-out
    of 200, single nodes and no-edge graphs; a training step through the same forward against autograd through the oracle;
    models the wide shape does not take (no edge features) keep their old path."""
    model = _headline_model(H=H, L=L, V=16, seed=9)
    b = _degenerate_batch(synth.code2_graphs(17, 12, 40))
    ref = O.code2_forward(model.state_dict(), copy.deepcopy(b), num_layers=L, bidirectional=True, out_wx=False,
                          out_pool_all=False, out_pool="max", max_seq_len=5)
    y = torch.from_numpy(np.random.default_rng(4).integers(0, 16, size=(b.num_graphs, 5)))
    loss_ref, gref = O.code2_grads(model.state_dict(), copy.deepcopy(b), y, num_layers=L, bidirectional=True, max_seq_len=5)
    model = model.to(device)
    lib = engine._lib.load()
    calls = []
    orig = lib.dagnn_dataflow_run

    class _Spy(object):
        def __call__(self, plan, args, stream):
            calls.append(args._obj.H)
            return orig(plan, args, stream)
    monkeypatch.setattr(lib, "dagnn_dataflow_run", _Spy(), raising=False)
    res = {}
    for wide in (1, 0):
        monkeypatch.setattr(engine, "DF_WIDE", wide)
        for c in model._derived.values():
            c.invalidate()
        model.eval()
        outs = []
        for rep in range(2):
            G = copy.deepcopy(b).to(device)
            with torch.no_grad():
                out = model(G)
            model.check()
            assert all(h.shape[1] == H for hd in G.h for h in hd)
            outs.append(([o.clone() for o in out], [h.clone() for hd in G.h for h in hd]))
        assert all(torch.equal(a, c) for a, c in zip(outs[0][0] + outs[0][1], outs[1][0] + outs[1][1]))
        res[wide] = outs[0]
        if wide:
            assert engine.state_width(H, L, 2, wide_ok=True) == 320 and calls and all(h == 320 for h in calls)
            loss, grads = _train_step(model, copy.deepcopy(b).to(device), y.to(device))
            model.check()
            assert abs(float(loss) - float(loss_ref)) < 1e-5
            for k, g in grads.items():
                scale = float(gref[k].abs().max())
                assert Hh.maxdiff(g, gref[k]) <= 1e-4 * scale + 2e-7, k
        else:
            assert not calls
        calls.clear()
    assert max(Hh.maxdiff(o, r) for o, r in zip(res[1][0], ref)) < TOL
    assert max(Hh.maxdiff(a, c) for a, c in zip(res[1][0], res[0][0])) < 2e-5
    assert max(Hh.maxdiff(a, c) for a, c in zip(res[1][1], res[0][1])) < 5e-6
    monkeypatch.setattr(engine, "DF_WIDE", 1)
    assert engine.state_width(300, 2, 0, wide_ok=False) == 512 and engine.state_width(300, 2, 2, wide_ok=False) == 512


def test_tile_kernel_full_size_properties(device, monkeypatch):
    """cfg 5 at BASELINE.json's full size (B=256, h=512, L=5, bidirectional) on the tile kernel: bitwise run to run, graph
    order permutes the rows and nothing else (to rounding), the per-layer launches agree to rounding, and the policy (`DAGNN_AMD_TILES=1`) picks the kernel by batch size."""
    monkeypatch.setattr(engine, "TILES", 2)
    model = _headline_model(H=512, L=5, V=32, seed=5).to(device)
    graphs = synth.code2_graphs(3, 256)
    full = synth.GraphBatch.from_data_list(graphs)
    with torch.no_grad():
        a = torch.stack(model(full.clone().to(device)))
        b = torch.stack(model(full.clone().to(device)))
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        rev = torch.stack(model(synth.GraphBatch.from_data_list(graphs[::-1]).to(device)))
        assert Hh.maxdiff(rev.flip(1), a) < 2e-5   # (a row's bits depend on its tile through the tile's shape only: <= 8 rows take 4x4x1 products)
        order = sorted(range(256), key=lambda g: -graphs[g].x.shape[0])[:64]
        sub = torch.stack(model(synth.GraphBatch.from_data_list([graphs[g] for g in order]).to(device)))
        assert Hh.maxdiff(sub, a[:, order]) < 2e-5
        model.check()
        monkeypatch.setattr(engine, "TILES", 0)
        for c in model._derived.values():
            c.invalidate()
        c0 = torch.stack(model(full.clone().to(device)))
        assert Hh.maxdiff(c0, a) < 2e-5
        # the default path at this size: per-layer launches for the wide first layers, the tile kernel for the thin tail
        monkeypatch.setattr(engine, "TILES", 1)
        for c in model._derived.values():
            c.invalidate()
        ran = {"frontier": [], "tiles": []}
        f_orig, t_orig = engine.frontier_run, engine.tiles_run
        monkeypatch.setattr(engine, "frontier_run", lambda *a_, **k: (ran["frontier"].append(k.get("stop_layer")), f_orig(*a_, **k))[1])
        monkeypatch.setattr(engine, "tiles_run", lambda *a_, **k: (ran["tiles"].append(k.get("first_layer")), t_orig(*a_, **k))[1])
        G1 = full.clone().to(device)
        s1 = torch.stack(model(G1))
        s2 = torch.stack(model(full.clone().to(device)))
        model.check()
        assert len(ran["frontier"]) == 2 and ran["frontier"][0] is not None and ran["frontier"][0] == ran["tiles"][0]
        assert min(ran["tiles"][0]) > 0 and torch.equal(s1, s2) and Hh.maxdiff(s1, c0) < 2e-5 and Hh.maxdiff(s1, a) < 2e-5
        monkeypatch.setattr(engine, "TILES", 0)
        for c in model._derived.values():
            c.invalidate()
        G0 = full.clone().to(device)
        model(G0)
        assert max(Hh.maxdiff(x, y) for d in range(2) for x, y in zip(G1.h[d], G0.h[d])) < 5e-6   # every state row
    N = full.x.shape[0]
    monkeypatch.setattr(engine, "TILES", 1)
    assert engine.tiles_launches(device, 2, 5, 512, 2, N) == 0 and engine.tiles_launches(device, 2, 5, 512, 2, 8000) == 2
    assert engine.tiles_launches(device, 2, 2, 512, 2, 8000) == 1 and engine.tiles_launches(device, 2, 4, 512, 2, 8000) == 1   # (every cell fits at once)
    assert engine.tiles_launches(device, 2, 1, 512, 2, 8000) == 0 and engine.tiles_launches(device, 2, 5, 256, 2, 8000) == 0


def test_tile_kernel_failures_surface(device, monkeypatch):
    """A bounded wait that expires (spin limit 1) and a batch that violates the plan contract both reach `model.check()`;
    the next healthy pass is clean."""
    monkeypatch.setattr(engine, "TILES", 2)
    model = _headline_model(H=512, L=3, V=8, seed=2).to(device).eval()
    b = synth.code2_batch(4, 12, 60)
    with torch.no_grad():
        ref = model(b.clone().to(device))
        model.check()
        monkeypatch.setattr(engine, "SPIN_LIMIT", 1)
        model(b.clone().to(device))
        monkeypatch.setattr(engine, "SPIN_LIMIT", 0)
        with pytest.raises(DagnnHipError, match="bounded device-side wait"):
            model.check()
        bad = b.clone().to(device)
        bad.batch = bad.batch.flip(0).contiguous()
        model(bad)
        with pytest.raises(DagnnHipError, match="plan contract"):
            model.check()
        out = model(b.clone().to(device))
        model.check()
        assert all(torch.equal(x, y) for x, y in zip(out, ref))


def test_tile_kernel_feeds_the_backward_pass(device, monkeypatch):
    """A training step of an h = 512, L = 3 model with the forward on the tile kernel: the state rows and the partial
    attention scores it leaves behind are what the reverse sweep (csrc/backward.hip) reads - loss and every parameter
    gradient against the same step on the per-layer launches and against autograd through the oracle."""
    model = _headline_model(H=512, L=3, V=12, seed=6)
    b = synth.code2_batch(8, 10, 40)
    y = torch.randint(0, 12, (10, 5), generator=torch.Generator().manual_seed(5))
    sd_cpu = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    loss_ref, grads_ref = O.code2_grads(sd_cpu, copy.deepcopy(b), y, num_layers=3, bidirectional=True, max_seq_len=5)
    model = model.to(device)
    res, ran = {}, []
    orig = engine.tiles_run
    monkeypatch.setattr(engine, "tiles_run", lambda *a, **k: (ran.append(1), orig(*a, **k))[1])
    for mode in (2, 0):
        monkeypatch.setattr(engine, "TILES", mode)
        loss, grads = _train_step(model, b.clone().to(device), y.to(device))
        model.check()
        res[mode] = (float(loss), {k: v.detach().cpu().clone() for k, v in grads.items()})
    assert len(ran) == 1
    assert abs(res[2][0] - float(loss_ref)) < 1e-5 and abs(res[2][0] - res[0][0]) < 1e-6
    for k, g in grads_ref.items():
        scale = max(float(g.abs().max()), 1e-6)
        assert float((res[2][1][k] - g).abs().max()) <= 2e-4 * scale + 2e-7, k
        assert float((res[2][1][k] - res[0][1][k]).abs().max()) <= 2e-5 * scale + 2e-7, k


@pytest.mark.parametrize("mode", ["alone", "split"])
def test_tile_kernel_back_to_back_forwards_are_race_free(device, monkeypatch, mode):
    """60 forwards issued back to back with nothing synchronising in between (state buffers and progress counters recycled
    every pass, epochs advancing): every pass reproduces the first bit for bit and no bounded wait expires - on the tile
    kernel alone and behind the per-layer launches of the wide first layers."""
    from bench import fresh_inputs
    monkeypatch.setattr(engine, "TILES", 2 if mode == "alone" else 1)
    if mode == "split":
        monkeypatch.setattr(engine, "TILES_MAX_NODES", 0)
    model = _headline_model(H=512, L=3, V=16, seed=8).to(device)
    master = synth.code2_batch(6, 48, 110).to(device)
    ins = fresh_inputs(master, 60)
    with torch.no_grad():
        first = [o.clone() for o in model(ins[0])]
        for g in ins[1:]:
            out = model(g)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, out))
    model.check()


def test_tile_kernel_split_feeds_the_backward_pass(device, monkeypatch):
    """The same for a batch that is split (per-layer launches for the wide first layers, tile kernel for the thin tail): one
    training step against the step on the launches alone."""
    model = _headline_model(H=512, L=3, V=12, seed=7).to(device)
    b = synth.code2_batch(9, 48, 110)
    y = torch.randint(0, 12, (48, 5), generator=torch.Generator().manual_seed(6)).to(device)
    monkeypatch.setattr(engine, "TILES_MAX_NODES", 0)
    res, ran = {}, []
    orig = engine.tiles_run
    monkeypatch.setattr(engine, "tiles_run", lambda *a, **k: (ran.append(k.get("first_layer")), orig(*a, **k))[1])
    for mode in (1, 0):
        monkeypatch.setattr(engine, "TILES", mode)
        loss, grads = _train_step(model, b.clone().to(device), y)
        model.check()
        res[mode] = (float(loss), {k: v.detach().clone() for k, v in grads.items()})
    assert len(ran) == 1 and ran[0] is not None and max(ran[0]) > 0
    assert abs(res[1][0] - res[0][0]) < 1e-6
    for k, g in res[0][1].items():
        scale = max(float(g.abs().max()), 1e-6)
        assert float((res[1][1][k] - g).abs().max()) <= 2e-5 * scale + 2e-7, k


# ----------------------------------------------------------------------------- training at the bench's own shapes, against float64
def _spy_entries(monkeypatch, fields):
    """{C entry point: [the named fields of its argument struct (second argument), one tuple per call]} - which paths a
    pass really took (a flag that silently falls back to the default path must not pass for the path it names)."""
    lib = engine._lib.load()
    seen = {}
    for name, fl in fields.items():
        seen[name] = []
        orig = getattr(lib, name)

        def spy(*a, _name=name, _fl=fl, _orig=orig):
            seen[_name].append(tuple(int(getattr(a[1]._obj, f)) for f in _fl))
            return _orig(*a)
        monkeypatch.setattr(lib, name, spy, raising=False)
    return seen


_TRAIN_ENTRIES = {"dagnn_dataflow_run": ("H", "stat_rows"), "dagnn_bwd_dataflow_prepare": ("H", "stat_rows_written"),
                  "dagnn_bwd_dataflow_run": ("H",), "dagnn_backward_run": ("H",)}


def _full_size_training_step(device, model, b, y, key):
    """One bench-shaped training step (fused loss, `ClipAdam(max_norm=0.25)`) against float64 autograd through the oracle:
    the loss, every parameter's gradient (the `encoder.*` tables, the heads and the attention weights included) and the
    global gradient norm `ClipAdam` clips with.  Returns (worst relative gradient error, its parameter)."""
    from dagnn_amd.train import ClipAdam
    L = model.num_layers
    loss_ref, ref = Hh.code2_grads64(key, model, b, y, num_layers=L, bidirectional=True, max_seq_len=5)
    model = model.to(device)
    opt = ClipAdam(model.parameters(), lr=1e-3, max_norm=0.25)
    loss, _ = _train_step(model, b.clone().to(device), y.to(device), fused_loss=True)
    model.check()
    assert abs(float(loss) - float(loss_ref)) < 1e-5, (float(loss), float(loss_ref))
    worst = Hh.check_grads_full(model, ref)
    opt.step()
    norm_ref = Hh.grad_norm64(model, ref)
    assert abs(float(opt.last_norm) - norm_ref) <= 1e-5 * norm_ref, (float(opt.last_norm), norm_ref)
    print("%s: loss %.8f (float64 %.8f), worst relative gradient error %.3e on %s, norm %.6f (float64 %.6f)"
          % (key, float(loss), float(loss_ref), worst[0], worst[1], float(opt.last_norm), norm_ref))
    return worst


@pytest.mark.parametrize("path", ["default", "stat_fwd0", "bwd_per_layer"])
def test_headline_training_step_matches_float64_autograd(device, monkeypatch, path):
    """The bench's training leg at its own shape (B = 128, N = 16 561, T = 374 layers; h = 256, L = 2, 5 heads of 5002) against
    float64 autograd: the reverse sweep (csrc/bwd_dataflow.hip) fed by the forward launch's static rows (the default), by
    `bd_stat_kernel`'s records (`STAT_FWD=0`) and the per-layer and persistent-tail launches of csrc/backward.hip
    (`BWD_DATAFLOW=0`) - each against the same reference, and each really on the path it names."""
    flags = dict(BWD_DATAFLOW=1, STAT_FWD=1)
    flags.update({"stat_fwd0": dict(STAT_FWD=0), "bwd_per_layer": dict(BWD_DATAFLOW=0)}.get(path, {}))
    for k, v in flags.items():
        monkeypatch.setattr(engine, k, v)
    model = _headline_model(H=256, L=2, V=5002)
    b = synth.code2_batch(0, 128)
    y = torch.randint(0, 5002, (128, 5), generator=torch.Generator().manual_seed(128))
    seen = _spy_entries(monkeypatch, _TRAIN_ENTRIES)
    _full_size_training_step(device, model, b, y, "cfg2_train_f64")
    fwd = seen["dagnn_dataflow_run"]
    assert fwd and all(h == 256 for h, _ in fwd), fwd
    if path == "bwd_per_layer":
        assert seen["dagnn_backward_run"] and not seen["dagnn_bwd_dataflow_run"], seen
        assert [s for _, s in fwd] == [0], fwd
    else:
        assert seen["dagnn_bwd_dataflow_run"] == [(256,)] and not seen["dagnn_backward_run"], seen
        assert seen["dagnn_bwd_dataflow_prepare"] == [(256, flags["STAT_FWD"])], seen
        assert [s for _, s in fwd] == [flags["STAT_FWD"]], fwd


def test_reference_training_shape_step_matches_float64_autograd(device, monkeypatch):
    """The reference's training shape (emb_dim = hidden = 300, B = 160: N = 20 168; L = 2, 5 heads of 5002): the 320-wide forward
    (csrc/dataflow_w.hip) writing the padded 320-float static records, the 320-wide reverse sweep (csrc/bwd_dataflow_w.hip),
    against float64 autograd."""
    model = _headline_model(H=300, L=2, V=5002, seed=6)
    b = synth.code2_batch(0, 160)
    y = torch.randint(0, 5002, (160, 5), generator=torch.Generator().manual_seed(160))
    seen = _spy_entries(monkeypatch, _TRAIN_ENTRIES)
    _full_size_training_step(device, model, b, y, "ogb_tok_h300_B160_train_f64")
    assert seen["dagnn_dataflow_run"] == [(320, 1)], seen
    assert seen["dagnn_bwd_dataflow_prepare"] == [(320, 1)] and seen["dagnn_bwd_dataflow_run"] == [(320,)], seen
    assert not seen["dagnn_backward_run"], seen


@pytest.mark.parametrize("cfg", ["cfg1_na_B64_h128", "cfg4_bn_B128_h256"])
def test_dvae_encoder_training_at_full_batch_matches_float64_autograd(device, cfg):
    """The D-VAE encoders at the bench's batch sizes (cfg 1: NA, 64 ENAS graphs, hs 128, unidirectional; cfg 4: BN, 128 graphs,
    hs 256, bidirectional; L = 2): gradients of <mu, r1> + <logvar, r2> against float64 autograd through the oracle (the
    reference fixtures hold 12-32 graphs), and the norm `ClipAdam` clips with."""
    from dagnn_amd import DAGNN_NA, DAGNN_BN
    from dagnn_amd.train import ClipAdam
    na = cfg.startswith("cfg1")
    cls, nn_, hs, B, bidir = (DAGNN_NA, 8, 128, 64, False) if na else (DAGNN_BN, 10, 256, 128, True)
    model = cls(nn_, hs, hs, nn_, nn_, 0, 1, hs=hs, nz=56, num_nodes=nn_, num_layers=2, bidirectional=bidir).eval()
    seeded_fill(model, 4000 + B)
    rows = synth.enas_rows(0, B) if na else synth.bn_rows(0, B)
    G = synth.dvae_batch([(synth.decode_enas_row if na else synth.decode_bn_row)(r) for r in rows])
    gen = torch.Generator().manual_seed(B)
    r1, r2 = torch.randn(B, 56, generator=gen), torch.randn(B, 56, generator=gen)
    loss_ref, ref = Hh.dvae_grads64(cfg, model, G, r1, r2, num_layers=2, bidirectional=bidir, num_nodes=nn_, vids=na)
    model = model.to(device).train()
    opt = ClipAdam(model.parameters(), lr=1e-3, max_norm=0.25)
    model.zero_grad(set_to_none=True)
    Hg = model(G.clone().to(device))
    loss = (model.fc1(Hg) * r1.to(device)).sum() + (model.fc2(Hg) * r2.to(device)).sum()
    loss.backward()
    model.check()
    assert abs(float(loss) - float(loss_ref)) < 1e-4 * max(1.0, abs(float(loss_ref))), (float(loss), float(loss_ref))
    worst = Hh.check_grads_full(model, ref)
    opt.step()
    norm_ref = Hh.grad_norm64(model, ref)
    assert abs(float(opt.last_norm) - norm_ref) <= 1e-5 * norm_ref, (float(opt.last_norm), norm_ref)
    print("%s: loss %.6f (float64 %.6f), worst relative gradient error %.3e on %s" % (cfg, float(loss), float(loss_ref), *worst))


# ----------------------------------------------------------------------------- optimizer steps reach every later pass
_EVAL_MODE_PATHS = ["code2_default", "code2_h512_L3", "code2_gated_sum", "code2_mattn_h", "code2_add_dataflow",
                    "code2_max_dataflow", "na_attn_h", "bn_attn_h", "na_add", "na_max", "bn_add", "bn_max"]


def _eval_mode_case(path, device):
    """(model on `device` in eval(), batch on the CPU, outputs of a pass, loss of the outputs, float64 oracle outputs of a state
    dict, float64 oracle gradients of the model as it stands) for one path of `test_optimizer_steps_reach_every_later_pass`."""
    if path.startswith("code2"):
        from dagnn_amd import DAGNN, ASTNodeEncoder
        H, L = (512, 3) if path == "code2_h512_L3" else (64, 2)
        agg = {"gated_sum": "gated_sum", "mattn_h": "mattn_h", "add_dataflow": "add", "max_dataflow": "max"}.get(path[6:], "attn_h")
        kw = dict(num_layers=L, bidirectional=True, out_wx=False, out_pool_all=False, out_pool="max")
        model = DAGNN(num_vocab=24, max_seq_len=5, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(H, 98, 10030, 20),
                      w_edge_attr=True, agg=agg, dropout=0.0, **kw).eval()
        seeded_fill(model, 500 + H + L)
        b = synth.code2_batch(41, 10, 40)
        y = torch.randint(0, 24, (10, 5), generator=torch.Generator().manual_seed(41))
        model = model.to(device)
        yd = y.to(device)
        run = lambda: list(model(b.clone().to(device)))   # noqa: E731
        loss_of = lambda out: sum(torch.nn.functional.cross_entropy(p, yd[:, s]) for s, p in enumerate(out)) / len(out)  # noqa: E731
        ref_out = lambda sd: O.code2_forward(sd, copy.deepcopy(b), max_seq_len=5, agg=agg, dtype=torch.float64, **kw)  # noqa: E731
        ref_grads = lambda: Hh.code2_grads64(None, model, b, y, max_seq_len=5, agg=agg, **kw)   # noqa: E731
        return model, run, loss_of, ref_out, ref_grads
    kind, agg = path.split("_", 1)
    bidir = kind == "bn"
    model, nn_ = Hh.dvae_model(dict(kind=kind, hs=64, L=2, bidir=bidir, agg=agg, w_seed=600 + len(path)))
    rows = synth.enas_rows(5, 12) if kind == "na" else synth.bn_rows(6, 10)
    G = synth.dvae_batch([(synth.decode_enas_row if kind == "na" else synth.decode_bn_row)(r) for r in rows])
    gen = torch.Generator().manual_seed(7)
    r1, r2 = torch.randn(len(rows), 56, generator=gen), torch.randn(len(rows), 56, generator=gen)
    kw = dict(num_layers=2, bidirectional=bidir, num_nodes=nn_, vids=kind == "na", agg=agg)
    model = model.to(device)
    r1d, r2d = r1.to(device), r2.to(device)

    def run():
        Hg = model(G.clone().to(device))
        return [model.fc1(Hg), model.fc2(Hg)]
    loss_of = lambda out: (out[0] * r1d).sum() + (out[1] * r2d).sum()   # noqa: E731
    ref_out = lambda sd: list(O.dvae_encode(sd, copy.deepcopy(G), dtype=torch.float64, **kw))   # noqa: E731
    ref_grads = lambda: Hh.dvae_grads64(None, model, G, r1, r2, **kw)   # noqa: E731
    return model, run, loss_of, ref_out, ref_grads


@pytest.mark.parametrize("optim", ["clip_adam", "fused_adam"])
@pytest.mark.parametrize("path", _EVAL_MODE_PATHS)
def test_optimizer_steps_reach_every_later_pass(device, monkeypatch, path, optim):
    """A training loop that leaves the module in eval() (dropout 0: both modes compute the same) and runs an evaluation pass
    between `backward()` and the optimizer step - which builds the derived-weight caches from the OLD parameters.  With
    `train.ClipAdam` (its kernel writes through raw pointers and bumps the version counters itself) the evaluation pass after
    the step and the next training pass must see the new parameters: outputs and gradients against the float64 oracle on the
    updated state.  `torch.optim.Adam(fused=True)` moves no version counter; there the stale evaluation pass must at least be
    reported at `check()`.  Paths: code2 on the dataflow kernel and the tile kernel (H = 512), the variants on
    csrc/variants.hip and `add` / `max` on the dataflow kernel, the D-VAE encoders with `attn_h`, `add` and `max`."""
    from dagnn_amd.train import ClipAdam
    monkeypatch.setattr(engine, "VARIANT_DATAFLOW", 1)
    model, run, loss_of, ref_out, ref_grads = _eval_mode_case(path, device)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = ClipAdam(params, lr=1e-2, max_norm=0.25) if optim == "clip_adam" else torch.optim.Adam(params, lr=1e-2, fused=True)
    model.zero_grad(set_to_none=True)
    loss_of(run()).backward()                                    # 1. a training pass (the module stays in eval())
    with torch.no_grad():
        before = [o.clone() for o in run()]                      # 2. evaluation: caches built from the old parameters
    opt.step()                                                   # 3.
    with torch.no_grad():
        after = [o.clone() for o in run()]                       # 4.
    assert not model.training
    if optim == "fused_adam":
        with pytest.raises(DagnnHipError, match="version counter"):
            model.check()                                        # (stale or not: the pass after the silent write is reported)
        return
    model.zero_grad(set_to_none=True)
    loss = loss_of(run())                                        # 5. the next training pass
    loss.backward()
    model.check()
    assert max(Hh.maxdiff(a, c) for a, c in zip(after, before)) > 1e-4   # (the step really happened)
    sd = Hh._cpu_state(model)
    for o, r in zip(after, ref_out(sd)):
        assert Hh.maxdiff(o, r) <= TOL * max(1.0, float(r.abs().max()))
    loss_ref, ref = ref_grads()
    # (the neighbouring tests' loss tolerances: 1e-5 for the mean cross-entropy, 1e-4 relative for the D-VAE sums)
    assert abs(float(loss) - float(loss_ref)) < (1e-5 if path.startswith("code2") else 1e-4 * max(1.0, abs(float(loss_ref))))
    Hh.check_grads_full(model, ref)


def test_fused_loss_backward_can_run_twice(device):
    """`backward(retain_graph=True)` twice through the fused sequence loss (csrc/loss.hip) accumulates exactly twice the
    gradients of one pass, as the loss loop does - and the same gradients as the loop."""
    from dagnn_amd.train import seq_cross_entropy
    model = _headline_model(H=64, L=2, V=40, seed=3).to(device).train()
    b = synth.code2_batch(17, 16, 40)
    y = torch.randint(0, 40, (16, 5), generator=torch.Generator().manual_seed(6)).to(device)
    got = {}
    for fused in (True, False):
        for times in (1, 2):
            model.zero_grad(set_to_none=True)
            pred = model(b.clone().to(device))
            loss = seq_cross_entropy(pred, y) if fused else \
                sum(torch.nn.functional.cross_entropy(p, y[:, s]) for s, p in enumerate(pred)) / len(pred)
            for _ in range(times):
                loss.backward(retain_graph=True)
            got[(fused, times)] = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    one, two = got[(True, 1)], got[(True, 2)]
    assert one.keys() == two.keys() and "graph_pred_linear_list.4.weight" in one
    for k in one:
        if "encoder." not in k:   # (torch's embedding backward accumulates with atomics)
            assert torch.equal(two[k], 2 * one[k]), k
        else:
            assert Hh.maxdiff(two[k], 2 * one[k]) <= 1e-6 * max(1.0, float(one[k].abs().max())), k
        ref = got[(False, 2)][k]
        assert Hh.maxdiff(two[k], ref) <= 2e-6 * max(1.0, float(ref.abs().max())) + 1e-9, k
