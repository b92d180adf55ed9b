"""Input-keyed attention on the BN D-VAE in HIP (`DAGNN_BN(agg='attn_x' | 'self_attn_x')`): the encoder on the static-score
path of the recurrence kernels, the type-keyed aggregate of csrc/dvae_decode.hip (`loss()` and its reverse), of
csrc/dvae_sample.hip (`decode()`) and of `dagnn_iprop_step_typed` (`_ipropagate_to`), and the loops built on them - against
the fixtures the unmodified reference wrote and, beyond them, the float64 restatement of `tests/dvae_attn_x_f64.py`
(pinned to those fixtures by `test_dvae_bn_attn_x_cpu.py`).

Bounds.  Fixtures: 1e-4 on Hg / mu / logvar, `helpers.check_grads`' defaults on gradients, 1e-5 relative on loss values,
graph-for-graph equality and 5e-6 on the decoded states.  Beyond the fixtures the yardstick is the float32 torch
evaluation of the SAME restatement: per tensor e_hip <= 4 x max(e_torch, 2^-23 x max|ref|) - one float32 ulp of the
largest entry is the floor, a float32 result cannot be asked to be closer -, and |hip| <= 1e-6 where the float64 value
is an exact zero."""
from __future__ import annotations

import copy
import functools

import numpy as np
import pytest
import torch

import dagnn_amd
from dagnn_amd import DagStore, dvae, engine, route, synth
from dagnn_amd.dvae_store import test_nll as store_test_nll, train_epoch
from tests import dvae_attn_x_f64 as X64
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

ENCODER = ["bn_h64_attn_x", "bn_h64_self_attn_x"]
GRAD = ["grad_bn_h64_attn_x", "grad_bn_h64_self_attn_x"]
LOSS = ["dvae_loss_bn_attn_x_h32_L3", "dvae_loss_bn_attn_x_h501_L2", "dvae_loss_bn_attn_x_h32_encode"]
DECODE = ["dvae_decode_bn_attn_x_h32_L3_argmax", "dvae_decode_bn_attn_x_h32_L3_sample", "dvae_decode_bn_attn_x_h501_L2_sample"]
ATTN_W, ATTN_B = "node_aggr_0.0.attn_lin.weight", "node_aggr_0.0.attn_lin.bias"
E = 10          # emb_dim = nvt of the fixtures' models
ATOL = 2e-7     # `helpers.check_grads`' atol: the reference's rounding noise on gradients that are exactly zero
FACTOR, ULP, ZERO_FLOOR = 4.0, 2.0 ** -23, 1e-6


@pytest.fixture(params=["dataflow", "lockstep", "pergraph"])
def schedule(request, monkeypatch):
    """The three HIP schedules of the recurrence, as the golden parity tests parametrise them."""
    monkeypatch.setenv("DAGNN_AMD_SCHEDULE", "pergraph" if request.param == "pergraph" else "lockstep")
    monkeypatch.setattr(engine, "DATAFLOW", 1 if request.param == "dataflow" else 0)
    return request.param


def _spy_routes(monkeypatch):
    """Every `Route` a pass computes and the recurrence launch functions it ran."""
    routes, ran = [], []
    orig = route.with_plan
    monkeypatch.setattr(route, "with_plan", lambda *a, **k: routes.append(orig(*a, **k)) or routes[-1])
    for name in ("dataflow_run", "tiles_run", "frontier_run", "bwd_dataflow_sweep", "backward_sweep"):
        fn = getattr(engine, name)
        monkeypatch.setattr(engine, name, lambda *a, _fn=fn, _name=name, **k: ran.append(_name) or _fn(*a, **k))
    return routes, ran


def _param_grads(model):
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    sd = model.state_dict()
    for k in list(grads):   # aliased encoder GRUs (cells_0 == grue_forward)
        for k2, v2 in sd.items():
            if k2 not in grads and v2.data_ptr() == sd[k].data_ptr():
                grads[k2] = grads[k]
    return grads


# ------------------------------------------------------------------ encoder
@pytest.mark.parametrize("name", ENCODER)
def test_encoder_matches_the_reference(device, name, schedule, monkeypatch):
    meta, arr = Hh.load(name)
    model, _ = Hh.dvae_model(meta)
    model = model.to(device)
    assert model.schedule == ("pergraph" if schedule == "pergraph" else "lockstep")
    routes, ran = _spy_routes(monkeypatch)
    monkeypatch.setattr(model, "_encode_fused", lambda *a, **k: pytest.fail("the fused evaluation call does not take _x models"))
    G = Hh.dvae_batch(arr, device)
    with torch.no_grad():
        Hg = model(G)
        mu, logvar = model.fc1(Hg), model.fc2(Hg)
    model.check()
    assert Hh.maxdiff(Hg, arr["Hg"]) < 1e-4
    assert Hh.maxdiff(mu, arr["mu"]) < 1e-4 and Hh.maxdiff(logvar, arr["logvar"]) < 1e-4
    if schedule == "pergraph":
        assert routes == [] and ran == []
    else:   # the static-score pass on the kernel the route names: the dataflow kernel at this width unless it is switched off
        assert len(routes) == 1 and routes[0].kind == ("dataflow" if schedule == "dataflow" else "launches"), routes
        assert ran == ["dataflow_run" if schedule == "dataflow" else "frontier_run"]
    with torch.no_grad():   # encode(list of graphs): the graphs rebuilt from the stored rows
        mu2, lv2 = model.encode(Hh.dvae_graphs(meta, arr))
    assert Hh.maxdiff(mu2, arr["mu"]) < 1e-4 and Hh.maxdiff(lv2, arr["logvar"]) < 1e-4


@pytest.mark.parametrize("name", GRAD)
def test_encoder_gradients_match_the_reference(device, name, monkeypatch):
    meta, arr = Hh.load(name)
    model, _ = Hh.dvae_model(meta)
    model = model.to(device).train()
    routes, ran = _spy_routes(monkeypatch)
    mu, logvar = model.encode([g.clone() for g in Hh.dvae_graphs(meta, arr)])
    assert Hh.maxdiff(mu, arr["mu"]) < 1e-4 and Hh.maxdiff(logvar, arr["logvar"]) < 1e-4
    loss = (mu * torch.from_numpy(arr["r1"]).to(device)).sum() + (logvar * torch.from_numpy(arr["r2"]).to(device)).sum()
    model.zero_grad(set_to_none=True)
    loss.backward()
    model.check()
    assert abs(float(loss.detach()) - float(arr["loss"])) < 1e-4 * max(1.0, abs(float(arr["loss"])))
    grads = {k: g for k, g in _param_grads(model).items() if "g::" + k in arr}
    Hh.check_grads(meta, arr, grads)
    dq = E if meta["agg"] == "attn_x" else 0
    for d in (0, 1):
        for l in range(meta["L"]):
            lin = getattr(model, "node_aggr_%d" % d)[l].attn_lin
            assert float(lin.weight.grad[0, dq:].abs().max()) > 1e-4            # the key half, through the static-score reverse
            assert float(lin.weight.grad[0, :dq].abs().max()) <= ATOL if dq else True
    assert len(routes) == 1 and routes[0].kind == "dataflow" and routes[0].reverse == "dataflow", routes
    assert ran == ["dataflow_run", "bwd_dataflow_sweep"]


@functools.lru_cache(maxsize=None)
def _cfg4_reference(agg):
    """128 `synth.bn_rows` graphs at hs = 256, L = 2, both directions (the shape of benchmark configuration 4): the model,
    the graphs and (Hg, mu, logvar) of the float64 restatement - computed once."""
    model = dagnn_amd.DAGNN_BN(10, 256, 256, 10, 10, 0, 1, hs=256, nz=56, num_nodes=10, agg=agg, num_layers=2,
                               bidirectional=True).eval()
    Hh.seeded_fill(model, 291)
    graphs = [synth.decode_bn_row(r) for r in synth.bn_rows(17, 128)]
    b = dagnn_amd.GraphBatch.from_data_list([g.clone() for g in graphs])
    with torch.no_grad():
        ref = X64.encode(Hh._cpu_state(model), b, L=2, bidirectional=True, num_nodes=10, agg=agg)
    return model, graphs, ref


@pytest.mark.parametrize("agg", ["attn_x", "self_attn_x"])
def test_encoder_at_128_graphs_hs256_matches_float64(device, agg, monkeypatch):
    """Beyond the fixtures, at the fixtures' own bound of 1e-4: the error of a graph's row does not depend on how many
    graphs share the batch, and |Hg| <= 1 (GRU states) behind Linear layers with rows of the same norms."""
    model, graphs, (Hg_r, mu_r, lv_r) = _cfg4_reference(agg)
    model = copy.deepcopy(model).to(device)
    routes, ran = _spy_routes(monkeypatch)
    b = dagnn_amd.GraphBatch.from_data_list([g.clone() for g in graphs])
    with torch.no_grad():
        Hg = model(b)
        mu, logvar = model.fc1(Hg), model.fc2(Hg)
    model.check()
    assert len(routes) == 1 and routes[0].kind == "dataflow" and routes[0].Hp == 256 and routes[0].groups > 0, routes
    assert ran == ["dataflow_run"]
    errs = [Hh.maxdiff(a, r) for a, r in ((Hg, Hg_r), (mu, mu_r), (logvar, lv_r))]
    print("%s 128 x hs256: |Hg - f64| %.2e  mu %.2e  logvar %.2e" % (agg, *errs))
    assert max(errs) < 1e-4, errs


# ------------------------------------------------------------------ loss: the fixtures
def _run_loss(name, device, grad=True):
    meta, arr = Hh.load(name)
    model, _ = Hh.dvae_model(meta)
    model = model.to(device).eval()
    graphs = Hh.dvae_graphs(meta, arr)
    with torch.set_grad_enabled(grad):
        if meta["encode"]:
            mu, logvar = model.encode([g.clone() for g in graphs])
            if grad:
                mu.retain_grad()
                logvar.retain_grad()
        else:
            mu = torch.from_numpy(arr["mu"].copy()).to(device).requires_grad_(grad)
            logvar = torch.from_numpy(arr["logvar"].copy()).to(device).requires_grad_(grad)
        loss, res, kld = model.loss(mu, logvar, graphs)
    grads = {}
    if grad:
        loss.backward()
        grads = dict(_param_grads(model), mu=mu.grad, logvar=logvar.grad)
    model.check()
    return meta, arr, model, loss.detach(), res.detach(), kld.detach(), grads


@pytest.mark.parametrize("name", LOSS)
def test_loss_and_gradients_match_the_reference(device, name):
    meta, arr, model, loss, res, kld, grads = _run_loss(name, device)
    for key, got in (("loss", loss), ("res", res), ("kld", kld)):
        ref = float(arr[key])
        print("%s %s: %.9g (reference %.9g)" % (name, key, float(got), ref))
        assert abs(float(got) - ref) <= 1e-5 * abs(ref) + 1e-6, (key, float(got), ref)
    Hh.check_grads(meta, arr, grads, verbose=True)
    g = model.node_aggr_0[0].attn_lin.weight.grad
    assert tuple(g.shape) == (1, 2 * E)
    ref_key = torch.from_numpy(arr["g::" + ATTN_W])[0, E:]
    assert float(ref_key.abs().max()) > 1e-4
    assert Hh.maxdiff(g[0, E:], ref_key) <= 2e-4 * float(ref_key.abs().max()) + ATOL      # d_key_type lands in the key half
    assert float(g[0, :E].abs().max()) <= ATOL                                           # the query half cancels
    b = model.node_aggr_0[0].attn_lin.bias.grad
    assert b is None or float(b.abs().max()) <= ATOL
    if not meta["encode"]:   # the decoder alone: exact zeros there, and nothing for the encoder's other aggregators
        assert not g[0, :E].any() and model.node_aggr_0[1].attn_lin.weight.grad is None


@pytest.mark.parametrize("name", LOSS[:2])
def test_loss_and_gradients_are_bitwise_repeatable(device, name):
    _, _, _, loss, _, _, g1 = _run_loss(name, device)
    _, _, _, loss2, _, _, g2 = _run_loss(name, device)
    assert torch.equal(loss, loss2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    _, _, _, loss3, res3, _, _ = _run_loss(name, device, grad=False)
    assert torch.equal(loss3, loss) and not loss3.requires_grad


# ------------------------------------------------------------------ loss: beyond the fixtures
N6 = 6
# six-vertex graphs by hand (types, predecessor lists per vertex); vertex 2 has no predecessor in ANY graph (P == 0 for a
# whole vertex), at vertex 3 graph 0 has two predecessors of the SAME type (two slots feed one table entry), graph 1 none
# and graph 2 three (padding takes weight in graphs 0 and 1), vertex 5 joins everything in graph 0 only
HAND = [([0, 3, 3, 4, 2, 1], [[], [0], [], [1, 2], [3], [0, 1, 2, 3, 4]]),
        ([0, 2, 5, 5, 3, 1], [[], [0], [], [], [1, 3], [4]]),
        ([0, 4, 2, 3, 3, 1], [[], [], [], [0, 1, 2], [0, 3], [2, 4]])]


def _hand_batch(rows):
    types = np.array([HAND[r][0] for r in rows], dtype=np.int32)
    preds = np.array([[sum(1 << u for u in p) for p in HAND[r][1]] for r in rows], dtype=np.int64)
    return types, preds.astype(np.uint32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _hand_case(hs, L, rows):
    """(model, types, preds, mu, logvar, float64 result, float32 result) of the restatement - computed once per case."""
    model = Hh.dvae_decoder_model("bn", max_n=N6, nvt=N6, hs=hs, L=L, agg="attn_x", seed=300 + hs + L)
    types, preds = _hand_batch(rows)
    rng = np.random.default_rng(hs * 10 + L)
    mu = torch.from_numpy(rng.standard_normal((len(rows), model.nz)).astype(np.float32))
    logvar = torch.from_numpy((0.1 * rng.standard_normal((len(rows), model.nz))).astype(np.float32))
    sd = Hh._cpu_state(model)
    ref = X64.loss_grads(sd, types, preds, mu, logvar, L=L)
    base = X64.loss_grads(sd, types, preds, mu, logvar, L=L, dtype=torch.float32)
    return model, types, preds, mu, logvar, ref, base


def _within(name, got, base, ref, report):
    got, base, ref = (torch.as_tensor(t).detach().cpu().double() for t in (got, base, ref))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    e_base, e_got = Hh.maxdiff(base, ref), Hh.maxdiff(got, ref)
    bound = FACTOR * max(e_base, ULP * scale)
    report.append((name, scale, e_base, e_got, e_got / bound if bound > 0 else 0.0))
    zero = ref == 0
    if zero.any():
        assert float(got[zero].abs().max()) <= ZERO_FLOOR, (name, float(got[zero].abs().max()))
    assert e_got <= bound, (name, e_got, e_base, scale)


@pytest.mark.parametrize("rows", [(0, 1, 2), (0,)], ids=["B3", "B1"])
@pytest.mark.parametrize("hs,L", [(32, 1), (32, 3), (36, 1), (36, 3), (501, 1), (501, 3)])
def test_loss_dense_beyond_the_fixtures_matches_float64(device, hs, L, rows):
    """`loss_dense` on the hand-made int32 schedule: values and every gradient within 4 x the float32 restatement's own
    error against float64 (floored at one float32 ulp of the tensor's largest entry)."""
    model, types, preds, mu, logvar, ref, base = _hand_case(hs, L, rows)
    widths = dvae.update_widths(preds, N6)
    if len(rows) == 3:   # the cases the schedule was made for
        upd = lambda v, k: widths[1 + sum(u + 1 for u in range(1, v)) + (v - k)]  # noqa: E731  (call order: k = v .. 0)
        assert all(upd(2, k) == 0 for k in range(3)) and upd(3, 0) == 3 and upd(3, 2) == 1
        assert types[0, 1] == types[0, 2]
    model = copy.deepcopy(model).to(device).eval()
    mu_d = mu.to(device).requires_grad_(True)
    lv_d = logvar.to(device).requires_grad_(True)
    loss, res, kld = model.loss_dense(mu_d, lv_d, torch.from_numpy(types).to(device), torch.from_numpy(preds).to(device))
    loss.backward()
    model.check()
    report = []
    for k, i in (("loss", 0), ("res", 1), ("kld", 2)):
        _within(k, (loss, res, kld)[i], base[i], ref[i], report)
    grads = dict({k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()},
                 mu=mu_d.grad, logvar=lv_d.grad)
    took_part = ("grud.", "fc3.", "add_vertex.", "add_edge.", ATTN_W, ATTN_B, "mu", "logvar")
    for k, g in grads.items():
        if k.startswith(took_part):
            _within(k, g, base[5][k], ref[5][k], report)
        else:
            assert not g.any(), k
    worst = max(report, key=lambda r: r[4])
    print("hs %d L %d B %d: closest to its bound %s (scale %.2e: torch32 %.2e, hip %.2e, ratio %.2f of the bound)"
          % (hs, L, len(rows), worst[0], worst[1], worst[2], worst[3], worst[4]))
    g = model.node_aggr_0[0].attn_lin.weight.grad[0]
    assert not g[:N6].any() and float(g[N6:].abs().max()) > 0
    used = set(int(t) for r in rows for v, t in enumerate(HAND[r][0]) if any(v in p for p in HAND[r][1]))
    assert len(used) < N6 and all(float(g[N6 + t]) == 0.0 for t in range(N6) if t not in used)   # entries no slot selects


# ------------------------------------------------------------------ decode
def _replay(name, device, **kw):
    meta, arr = Hh.load(name)
    model, _ = Hh.dvae_model(meta)
    model = model.to(device).eval()
    z = torch.from_numpy(arr["z"].copy()).to(device)
    draws = None
    if meta["stochastic"]:
        draws = (torch.from_numpy(arr["u_type"].copy()).to(device), torch.from_numpy(arr["u_edge"].copy()).to(device))
    return meta, arr, model, z, model.decode_dense(z, stochastic=meta["stochastic"], draws=draws, states=True, **kw)


@pytest.mark.parametrize("name", DECODE)
def test_decode_matches_the_reference(device, name):
    meta, arr, model, z, d = _replay(name, device)
    nv, types, preds = d.nv[0].cpu().numpy(), d.types[0].cpu().numpy(), d.preds[0].cpu().numpy()
    assert np.array_equal(nv, arr["nv"])
    assert np.array_equal(types, arr["types"])
    assert np.array_equal(preds.view(np.uint32).astype(np.int64), arr["preds"])
    err = float(np.abs(d.states[0].cpu().numpy() - arr["states"]).max())
    print("%s: states %.2e" % (name, err))
    assert err <= 5e-6, (name, err)
    if not meta["stochastic"]:   # the public call: host graphs equal to the reference's, edges in its insertion order
        graphs = model.decode(z, stochastic=False)
        assert len(graphs) == meta["B"]
        for b, g in enumerate(graphs):
            assert g.vcount() == arr["nv"][b] and list(g.vs["type"]) == list(arr["types"][b, :arr["nv"][b]])
            assert [list(e) for e in g.get_edgelist()] == meta["edge_order"][b]


def test_attempts_equal_separate_calls(device):
    meta, arr = Hh.load(DECODE[1])
    model, _ = Hh.dvae_model(meta)
    model = model.to(device).eval()
    z = torch.from_numpy(arr["z"].copy()).to(device)
    st, se = dvae.draw_shapes(model.max_n, z.shape[0], 3)
    g = torch.Generator(device=device).manual_seed(11)
    u_type, u_edge = torch.rand(st, device=device, generator=g), torch.rand(se, device=device, generator=g)
    both = model.decode_dense(z, True, attempts=3, draws=(u_type, u_edge), states=True)
    for i in range(3):
        one = model.decode_dense(z, True, attempts=1, draws=(u_type[i:i + 1].contiguous(), u_edge[i:i + 1].contiguous()),
                                 states=True)
        for k in ("types", "preds", "nv", "states"):
            assert torch.equal(getattr(both, k)[i], getattr(one, k)[0]), (i, k)
    assert not torch.equal(both.preds[0], both.preds[1])


# ------------------------------------------------------------------ _ipropagate_to
def _iprop_setup(device):
    """The stand-in graphs of the `iprop_bn_h32_L3` fixture (a vertex without predecessors, ragged predecessor lists)
    under an attn_x model; their reference values are the float64 restatement's."""
    meta, arr = Hh.load("iprop_bn_h32_L3")
    meta = dict(meta, bidir=False, agg="attn_x", w_seed=311)
    model, _ = Hh.dvae_model(meta)
    return meta, arr, model


def _iprop_inputs(meta, arr, v):
    alive = [k for k in range(meta["K"]) if arr["counts"][k] > v]
    preds = [[u for u in range(v) if arr["adj"][k, u, v]] for k in alive]
    ptypes = [[int(arr["types"][k, u]) for u in p] for k, p in zip(alive, preds)]
    values = [torch.from_numpy(np.stack([arr["states"][k, u, 0] for u in p])) if p else None for k, p in zip(alive, preds)]
    return alive, preds, ptypes, values, [int(arr["types"][k, v]) for k in alive]


def test_ipropagate_to_matches_float64(device):
    meta, arr, model = _iprop_setup(device)
    sd = Hh._cpu_state(model)
    model = model.to(device)
    L, n = meta["L"], meta["n"]
    seen = set()
    with torch.no_grad():
        for v in meta["vs"]:
            alive, preds, ptypes, values, xt = _iprop_inputs(meta, arr, v)
            seen |= {len(p) for p in preds}
            want = X64.iprop_step(sd, xt, ptypes, values, L=L)
            G = Hh.iprop_graphs(meta, arr, device)
            Hv = model._ipropagate_to(G, v, model.grud)
            assert Hh.maxdiff(Hv, want[L - 1]) < 5e-6
            got = torch.stack([torch.cat([G[k].vs[v]["H_forward%d" % l] for k in alive]) for l in range(L)])
            assert Hh.maxdiff(got, want) < 5e-6
            Hgiven = torch.from_numpy(arr["H_given"].copy())
            want_g = X64.iprop_step(sd, xt, None, None, L=L, H=Hgiven[:len(alive)])
            Hg = model._ipropagate_to(Hh.iprop_graphs(meta, arr, device), v, model.grud, H=Hgiven.to(device))
            assert Hh.maxdiff(Hg, want_g[L - 1]) < 5e-6
        assert 0 in seen and len(seen) >= 3                       # no predecessors, ragged lists
        assert model._ipropagate_to(Hh.iprop_graphs(meta, arr, device), n + 3, model.grud) is None
        # a vertex NO graph has a predecessor for: the zero aggregate
        G = Hh.iprop_graphs(meta, arr, device)
        for g in G:
            g._pred[1] = []
        want = X64.iprop_step(sd, [int(arr["types"][k, 1]) for k in range(meta["K"])], [[] for _ in G], None, L=L)
        assert Hh.maxdiff(model._ipropagate_to(G, 1, model.grud), want[L - 1]) < 5e-6


def test_ipropagate_to_gradients_equal_autograd_on_the_dense_form(device):
    """`_IpropStep` (the HIP launch forward, the dense torch form differentiated in reverse) against plain autograd through
    `_iprop_dense` with the type table in place of w_key / vid_bias - and that dense form against the float64 restatement."""
    meta, arr, model = _iprop_setup(device)
    sd = Hh._cpu_state(model)
    model = model.to(device)
    L, v = meta["L"], meta["vs"][1]
    alive, preds, ptypes, values, xt = _iprop_inputs(meta, arr, v)
    P = max(len(p) for p in preds)
    G = Hh.iprop_graphs(meta, arr, device)
    for k in alive:
        for u in range(v):
            G[k].vs[u]["H_forward0"].requires_grad_(True)
    cot = torch.from_numpy(np.random.default_rng(5).standard_normal((len(alive), meta["hs"])).astype(np.float32)).to(device)
    names = [k for k, _ in model.named_parameters() if k.startswith("grud.") or k == ATTN_W]
    params = dict(model.named_parameters())

    def grads_of(out):
        model.zero_grad(set_to_none=True)
        leaves = [G[k].vs[u]["H_forward0"] for k, p in zip(alive, preds) for u in p]
        gs = torch.autograd.grad((out * cot).sum(), leaves + [params[k] for k in names], allow_unused=True)
        return [torch.zeros(1, device=device) if g is None else g for g in gs]

    Hv = model._ipropagate_to(G, v, model.grud)
    assert Hv.requires_grad
    got = grads_of(Hv)
    # the same step on dense torch ops
    w = params[ATTN_W][0]
    vals = torch.stack([torch.cat([G[k].vs[u]["H_forward0"] for u in p] + [torch.zeros(P - len(p), meta["hs"], device=device)])
                        for k, p in zip(alive, preds)])
    ids = torch.tensor([t + [-1] * (P - len(t)) for t in ptypes], dtype=torch.int32, device=device)
    X = torch.nn.functional.one_hot(torch.tensor(xt, device=device), 10).float()
    cells = list(model.grud)[:L]
    dense = dvae._iprop_dense(vals, ids, None, w[E:], None, X, cells)
    want64 = X64.iprop_step(sd, xt, ptypes, values, L=L)
    assert Hh.maxdiff(dense, want64) < 5e-6 and Hh.maxdiff(Hv, dense[L - 1]) < 5e-6
    want = grads_of(dense[L - 1])
    for k, a, b in zip(["state"] * (len(got) - len(names)) + names, got, want):
        assert Hh.maxdiff(a, b) <= 1e-6 * max(float(b.abs().max()), 1e-3), k
    gw = dict(zip(names, got[len(got) - len(names):]))[ATTN_W]
    assert not gw[0, :E].any() and float(gw[0, E:].abs().max()) > 0


# ------------------------------------------------------------------ loops
@functools.lru_cache(maxsize=None)
def _store(device_str):
    rows = synth.bn_rows(33, 24)
    y = np.random.default_rng(3).random(len(rows)).astype(np.float32)
    return rows, [synth.decode_bn_row(r) for r in rows], DagStore.from_rows(rows, "BN", 10, torch.device(device_str), y=y)


def _loop_model(seed=0):
    return Hh.dvae_decoder_model("bn", max_n=10, nvt=10, hs=32, L=2, nz=8, agg="attn_x", seed=seed)


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


def test_train_epoch_equals_two_steps_over_lists(device):
    """Two optimizer steps (batches of 8) through `DagStore.train_epoch` and through lists of graphs: the same tensors go
    into the same launches, so the loss sums, every parameter and Adam's state are bitwise equal."""
    rows, graphs, st = _store(str(device))
    base = _loop_model().to(device)
    ids = [3, 17, 5, 5, 20, 11, 0, 9, 23, 1, 14, 7, 2, 8, 19, 6]
    res = []
    for how in ("list", "store"):
        model = copy.deepcopy(base)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        torch.manual_seed(21)
        sums = _epoch_lists(model, opt, graphs, ids, 8, 0.25) if how == "list" else train_epoch(model, opt, st, ids, 8, clip=0.25)
        model.check()
        state = {k: opt.state[p] for k, p in model.named_parameters() if p in opt.state}
        res.append((sums, {k: p.detach().clone() for k, p in model.named_parameters()}, state))
    (s1, p1, a1), (s2, p2, a2) = res
    assert all(np.isfinite(s2)) and s1 == s2, (s1, s2)
    moved = 0
    for k, p in base.named_parameters():
        assert torch.equal(p1[k], p2[k]), k
        moved += int(not torch.equal(p2[k], p.detach()))
    assert moved > 8 and not torch.equal(p2[ATTN_W][0, E:], dict(base.named_parameters())[ATTN_W].detach()[0, E:])
    assert sorted(a1) == sorted(a2) and ATTN_W in a2
    for k in a1:
        for f in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a1[k][f], a2[k][f]), (k, f)
    # the evaluation loop on the store: the list form's reconstruction loss per graph
    model = copy.deepcopy(base).eval()
    with torch.no_grad():
        want = sum(float(model.loss(*model.encode([graphs[j] for j in ids[i:i + 8]]), [graphs[j] for j in ids[i:i + 8]])[1])
                   for i in range(0, len(ids), 8)) / len(ids)
    assert abs(store_test_nll(model, st, ids, 8) - want) <= 1e-6 * abs(want)


def test_decode_from_latent_space_equals_the_host_selection(device):
    model = _loop_model(seed=4).to(device).eval()
    z = torch.from_numpy(np.random.default_rng(5).standard_normal((4, 8)).astype(np.float32)).to(device)
    torch.manual_seed(1234)
    d = model.decode_dense(z, True, attempts=12)
    types, preds, nv = (t.cpu().numpy() for t in (d.types, d.preds, d.nv))
    valid, pick, n_valid, n_same, _ = dvae.select_host(types, preds, nv, "BN", model.nvt, model.START_TYPE, model.END_TYPE, None,
                                                       "first")
    strings = [None if p < 0 else dvae.bn_adj_string(types[p, b], preds[p, b], nv[p, b]) for b, p in enumerate(pick)]
    torch.manual_seed(1234)
    assert dvae.decode_from_latent_space(z, model, 12, "variable", False, "BN") == strings
    sel = model.select_dense(d, "BN")
    np.testing.assert_array_equal(sel.valid.cpu().numpy().astype(bool), valid)
    assert sel.pick.tolist() == pick.tolist() and sel.n_valid.tolist() == n_valid.tolist()
    assert tuple(types.shape) == (12, 4, 10) and (nv >= 2).all()


def test_the_other_loops_take_an_attn_x_model(device):
    """What is built on encode / loss / decode and never looks at the aggregator: `extract_latent`, `recon_accuracy` and
    `prior_validity` from the store equal their list forms, `train_epoch(predictor=True)` runs, and `decode_and_score` returns
    the strings of `decode_from_latent_space` with the scores of those strings."""
    from dagnn_amd.bn_score import BnData, decode_and_score, score_strings
    from dagnn_amd.predictor import attach_predictor
    rows, graphs, st = _store(str(device))
    model = _loop_model(seed=2).to(device).eval()
    ids = list(range(0, 21))
    G = [graphs[i] for i in ids]
    mu = dvae.extract_latent(model, (st, ids), 8)
    assert torch.equal(mu, dvae.extract_latent(model, G, 8)) and tuple(mu.shape) == (21, 8)
    torch.manual_seed(5)
    draws = dvae._take_draws(None, 10, len(ids), 6, device, "")
    a = dvae.recon_accuracy(model, (st, ids), 2, 3, draws=draws, batch_size=8)
    b = dvae.recon_accuracy(model, G, 2, 3, draws=draws, batch_size=8)
    assert a[:2] == b[:2] and a[1] == len(ids) * 6 and torch.equal(a[2], b[2])
    z = torch.from_numpy(np.random.default_rng(9).standard_normal((12, 8)).astype(np.float32)).to(device)
    torch.manual_seed(31)
    pdraws = dvae._take_draws(None, 10, 12, 4, device, "")
    got = dvae.prior_validity(model, st.graph_set(), decode_times=4, data_type="BN", z=z, draws=pdraws)
    want = dvae.prior_validity(model, dvae.GraphSet.from_graphs(graphs, 10, 10, device), decode_times=4, data_type="BN", z=z,
                               draws=pdraws)
    assert got == want and got.n_total == 48
    data = BnData.from_samples(synth.asia_samples(2, 300), [2] * 8, device=device)
    sd, se = dvae.draw_shapes(10, 4, 12)
    g = torch.Generator(device=device).manual_seed(21)
    ddraws = (torch.rand(sd, device=device, generator=g), torch.rand(se, device=device, generator=g))
    strings, scores = decode_and_score(z[:4], model, data, 12, draws=ddraws)
    assert strings == dvae.decode_from_latent_space(z[:4], model, 12, "variable", False, "BN", draws=ddraws)
    ref = np.asarray(score_strings(data, strings), dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(scores), [s is None for s in strings])
    np.testing.assert_array_equal(scores[~np.isnan(ref)], ref[~np.isnan(ref)])
    torch.manual_seed(2)
    trained = attach_predictor(_loop_model(seed=2)).to(device)   # (the same weights as `model`, built anew: a model that ran holds its arena)
    opt = torch.optim.Adam(trained.parameters(), lr=1e-3)
    torch.manual_seed(3)
    sums = train_epoch(trained, opt, st, ids[:16], 8, clip=0.25, predictor=True)
    trained.check()
    assert len(sums) == 4 and all(np.isfinite(sums))
    assert not torch.equal(dict(trained.named_parameters())[ATTN_W], dict(model.named_parameters())[ATTN_W])
