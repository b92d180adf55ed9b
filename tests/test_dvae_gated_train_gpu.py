"""Training `DAGNN_NA(agg='gated_sum')`'s encoder through the HIP reverse sweep (csrc/variants_bwd.hip with the vertex-id
columns, `dagnn_vid_colsums`) at any hidden width, against the float64 per-vertex oracle of
tests/test_dvae_gated_train_cpu.py; and plain `DAGNN` at a hidden width that is no multiple of 4.

Tolerance (the convention of §4i): nothing chosen in advance.  For every shape the torch-ops path that trained
this encoder before (`_gated_sum_states`, fp32, on the same GPU) is run against the same oracle, and the HIP path gets 4 x
that path's own largest error per tensor; entries that are zero in exact arithmetic get 1e-6 absolute.  Measured on one
MI355X, largest relative error (max |got - ref| / max |ref|) of a tensor over all cases of a width, torch path / HIP:
`MEASURED` below."""
from __future__ import annotations

import functools
import warnings

import pytest
import torch

from dagnn_amd import dvae, synth, variants
from tests.test_dvae_gated_train_cpu import (N_NODES, cotangent, make_graphs, make_model, oracle_grads, path_grads,
                                             torch_path_encode)

pytestmark = pytest.mark.gpu

FACTOR = 4.0        # x the torch path's own error
ZERO_FLOOR = 1e-6   # absolute, for entries that are zero in exact arithmetic
# hs: (torch path, HIP) - the worst tensor of the worst case, as printed by `_report` on one MI355X
MEASURED = {32: (4.7e-7, 4.2e-7), 37: (6.1e-7, 5.6e-7), 132: (3.8e-7, 4.3e-7), 501: (3.6e-7, 4.2e-7), "37 pool_all": (2.9e-7, 3.3e-7)}
# (the largest HIP : torch ratio of a single tensor was 2.9 - `mu` at hs = 37, L = 1, B = 1: 3.5e-8 against 9.9e-8 - bound 4)

CASES = [(hs, L, bidir, B, False) for hs in (32, 37, 132) for L in (1, 2) for bidir in (False, True) for B in (1, 5)] + \
    [(501, 2, False, 4, False), (37, 2, True, 5, True)]


def _ids(c):
    return "hs%d-L%d-%s-B%d%s" % (c[0], c[1], "bidir" if c[2] else "unidir", c[3], "-poolall" if c[4] else "")


def _refuse(*a, **k):
    raise AssertionError("the torch-ops encoder ran")


@functools.lru_cache(maxsize=None)
def _case(case):
    """(oracle, torch path, HIP, HIP again) = (mu, logvar, {name: gradient}) each, float64 on the CPU - computed once per shape."""
    hs, L, bidir, B, pool_all = case
    dev = torch.device("cuda:0")
    model = make_model(hs, L, bidir, pool_all).to(dev).train()
    graphs = make_graphs(B)
    cot = cotangent(B, 16)
    ref = oracle_grads({k: v.detach().cpu() for k, v in model.state_dict().items()}, graphs, hs, L, bidir, cot, pool_all)
    parent = path_grads(model, lambda: torch_path_encode(model, graphs), cot)
    model._gated_sum_states = _refuse   # (an instance attribute in front of the method: the HIP runs below cannot fall back)
    hip = path_grads(model, lambda: model.encode([g.clone() for g in graphs]), cot)
    hip2 = path_grads(model, lambda: model.encode([g.clone() for g in graphs]), cot)
    torch.cuda.synchronize()
    model.check()
    return ref, parent, hip, hip2


def _check_tensor(name, got, par, ref, report):
    """4 x the torch path's largest error on this tensor; exact zeros of the oracle at 1e-6."""
    zero = ref == 0
    e_par = float((par - ref).abs().max())
    e_got = float((got - ref).abs().max())
    scale = float(ref.abs().max())
    report.append((name, e_par / scale if scale else e_par, e_got / scale if scale else e_got))
    if zero.any():
        assert float(got[zero].abs().max()) <= ZERO_FLOOR, (name, float(got[zero].abs().max()))
    if (~zero).any():
        assert float((got - ref)[~zero].abs().max()) <= FACTOR * e_par, (name, e_got, e_par)


def _report(case, report):
    worst = max(report, key=lambda r: r[2] / r[1] if r[1] > 0 else 0.0)
    print("\n%s: worst relative error torch %.3e / hip %.3e; closest to the bound: %s torch %.3e hip %.3e" % (
        _ids(case), max(r[1] for r in report), max(r[2] for r in report), worst[0], worst[1], worst[2]))
    for r in report:
        print("    %-34s torch %.3e  hip %.3e" % r)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_encoder_gradients_match_the_float64_oracle(device, case):
    """`encode()` + a fixed random cotangent on (mu, logvar): mu, logvar and the gradient of every named parameter."""
    hs, L, bidir, B, pool_all = case
    (mu_r, lv_r, g_r), (mu_p, lv_p, g_p), (mu_h, lv_h, g_h), _ = _case(case)
    report, failures = [], []
    todo = [("mu", mu_h, mu_p, mu_r), ("logvar", lv_h, lv_p, lv_r)]
    for k in g_h:
        ref = g_r.get(k, torch.zeros_like(g_h[k]))
        todo.append((k, g_h[k], g_p[k], ref))
        if k.startswith(("gate_", "mapper_")) and k.endswith("weight") and float(ref.abs().max()) > 0:
            # the vertex-id columns on their own: their scale is not the state columns'
            assert float(ref[:, hs:].abs().max()) > 0 and float(g_h[k][:, hs:].abs().max()) > 0, k
            todo.append((k + "[:, H:]", g_h[k][:, hs:], g_p[k][:, hs:], ref[:, hs:]))
    for name, got, par, ref in todo:
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        try:
            _check_tensor(name, got, par, ref, report)
        except AssertionError as exc:
            failures.append(str(exc))
    _report(case, report)
    sfx = ["forward", "backward"] if bidir else ["forward"]
    for s in sfx:
        for i in range(L):
            assert "gate_%s.%d.0.weight[:, H:]" % (s, i) in [r[0] for r in report]
    assert not failures, failures


@pytest.mark.parametrize("case", [CASES[0], CASES[11], CASES[-2]], ids=_ids)
def test_two_training_passes_are_bitwise_equal(device, case):
    _, _, (mu1, lv1, g1), (mu2, lv2, g2) = _case(case)
    assert torch.equal(mu1, mu2) and torch.equal(lv1, lv2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("N", [8, 40, 8 * 257])
@pytest.mark.parametrize("J", [4, 74, 520])
def test_vid_colsums_against_float64(device, N, J):
    """out[j] = sum of the rows v with v mod n == j, n = 8: one accumulator per element adds m = N / n terms in ascending row
    order, so |got - ref| <= (m - 1) u sum |terms| (u = 2^-24; m = 1: exact); two calls give the same bits."""
    n = 8
    g = torch.Generator().manual_seed(N * 1000 + J)
    t = torch.randn(N, J, generator=g).to(device)
    out = variants.vid_colsums(t, n)
    again = variants.vid_colsums(t, n)
    assert out.shape == (n, J) and torch.equal(out, again)
    t64 = t.double().view(N // n, n, J)
    ref, mass = t64.sum(0), t64.abs().sum(0)
    bound = (N // n - 1) * 2.0 ** -24 * mass
    assert bool(((out.double() - ref).abs() <= bound).all()), float(((out.double() - ref).abs() - bound).max())
    # a row pitch wider than J: the columns of a [N, J + 6] buffer
    wide = torch.randn(N, J + 6, generator=g).to(device)
    from dagnn_amd import _lib, engine
    part = torch.full((n, J), float("nan"), device=device)
    engine.check(_lib.load().dagnn_vid_colsums(wide.data_ptr(), J + 6, N, J, n, part.data_ptr(), J, engine._stream(wide)), "dagnn_vid_colsums")
    assert torch.equal(part, variants.vid_colsums(wide[:, :J].contiguous(), n))


@pytest.mark.parametrize("hs", [32, 37])
def test_training_takes_the_hip_sweep(device, hs, monkeypatch):
    """With `_gated_sum_states` raising, encode + loss + backward of a training step succeed: the encoder's gradients and the
    decoder's add up in the layer-0 gate / mapper."""
    monkeypatch.setattr(dvae._DvaeDagnn, "_gated_sum_states", _refuse)
    model = make_model(hs, 2, False, seed=3).to(device).train()
    graphs = make_graphs(6)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        mu, logvar = model.encode([g.clone() for g in graphs])
        loss, _, _ = model.loss(mu, logvar, graphs)
        loss.backward()
    assert not [w for w in seen if "torch ops" in str(w.message)]
    assert bool(torch.isfinite(loss))
    for k, p in model.named_parameters():
        if k.startswith(("gate_forward", "mapper_forward", "grue_forward", "fc1", "fc2", "out_linear")):
            assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), k
            assert float(p.grad.abs().max()) > 0, k
    enc_only = make_model(hs, 2, False, seed=3).to(device).train()
    mu2, logvar2 = enc_only.encode([g.clone() for g in graphs])
    g_mu, g_lv = torch.autograd.grad(model.loss(mu2, logvar2, graphs)[0], [mu2, logvar2], retain_graph=True)
    enc_only.zero_grad(set_to_none=True)
    torch.autograd.backward([mu2, logvar2], [g_mu, g_lv])
    # layer 1's gate is the encoder's alone, layer 0's also the decoder's: the two shares are one .grad
    w1, e1 = model.gate_forward[1][0].weight.grad, enc_only.gate_forward[1][0].weight.grad
    assert float((w1 - e1).abs().max()) <= 1e-5 * float(e1.abs().max())
    w0, e0 = model.gate_forward[0][0].weight.grad, enc_only.gate_forward[0][0].weight.grad
    assert float((w0 - e0).abs().max()) > 1e-3 * float(e0.abs().max())


def test_a_gate_of_another_width_falls_back_and_warns_once(device, monkeypatch):
    """`_gated_hip_ok()` false: the torch-ops encoder trains, with ONE `warn_torch_path` warning for the shape."""
    hs = 20
    monkeypatch.setattr(variants, "_TORCH_PATH_SEEN", set())
    model = make_model(hs, 1, False)
    model.gate_forward[0][0] = torch.nn.Linear(hs + N_NODES + 4, hs)
    model = model.to(device).train()
    assert not model._gated_hip_ok()
    graphs = make_graphs(3)
    calls = []
    real = dvae._DvaeDagnn._gated_sum_states
    monkeypatch.setattr(dvae._DvaeDagnn, "_gated_sum_states", lambda self, G, x: (calls.append(1), real(self, G, x))[1])
    counts = []
    for _ in range(2):
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            mu, logvar = model.encode([g.clone() for g in graphs])
            (mu.sum() + logvar.sum()).backward()
        counts.append(len([w for w in seen if issubclass(w.category, RuntimeWarning) and "torch ops" in str(w.message)]))
    assert counts == [1, 0] and len(calls) == 2
    assert float(model.gate_forward[0][0].weight.grad.abs().max()) > 0


def test_padding_stays_inside_the_sweep(device):
    """hs = 37 (row pitch 40): the states the recurrence returns and every gradient are exactly hs wide; the padding behind
    the states is zero before and after the reverse sweep.  (The padding must be zero on input - the API offers no way to
    hand the sweep poisoned padding - so this checks what leaves it.)"""
    from dagnn_amd import engine
    from dagnn_amd.data import GraphBatch
    hs, L = 37, 2
    model = make_model(hs, L, True).to(device).train()
    b = GraphBatch.from_data_list(make_graphs(5)).to(device)
    x = b.x.float().contiguous().requires_grad_(True)
    bl = b.bi_layer_index
    plan = engine.build_plan(b.edge_index, bl[0][0], bl[1][0], b.batch, 5, None)
    view = model._agg_view()
    params = [p for d in model.dirs for i in range(L) for _, p in variants._cell_params(view, d, i)]
    outs = variants.VariantRecurrence.apply(view, b, plan, x, *params)
    bases = []
    for t in outs:
        assert t.shape == (5 * N_NODES, hs)
        base = t._base
        assert base is not None and base.shape == (5 * N_NODES, 40) and bool((base[:, hs:] == 0).all())
        bases.append(base)
    g = torch.Generator().manual_seed(2)
    grads = torch.autograd.grad([(t * torch.randn(t.shape, generator=g).to(device)).sum() for t in outs], [x] + params,
                                grad_outputs=[torch.ones((), device=device)] * len(outs), allow_unused=True)
    for p, gr in zip([x] + params, grads):
        assert gr is not None and gr.shape == p.shape and bool(torch.isfinite(gr).all())
    for base in bases:
        assert bool((base[:, hs:] == 0).all())


@pytest.mark.parametrize("agg", ["gated_sum", "add", "max"])
def test_plain_dagnn_trains_through_the_sweep_at_hidden_38(device, agg):
    """`DAGNN(agg=..., hidden_dim=38, emb_dim=8)`: a training step raises no torch-path warning, and the recurrence's
    gradients (node inputs and every cell parameter) match float64 autograd of `variants.run` within 4 x the error of the
    same `variants.run` in fp32."""
    from dagnn_amd import DAGNN, ASTNodeEncoder
    from dagnn_amd.core import num_graphs_of
    H, E = 38, 8

    def build():
        torch.manual_seed(4)
        return DAGNN(num_vocab=11, max_seq_len=2, emb_dim=E, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(E, 98, 300, 20),
                     num_layers=2, bidirectional=True, agg=agg, out_wx=False, out_pool_all=False)

    model = build().to(device).train()
    b = synth.code2_batch(21, 5, 25)
    b.x[:, 1] %= 300
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        pred = model(b.clone().to(device))
        sum(p.sum() for p in pred).backward()
    assert not [w for w in seen if "torch ops" in str(w.message)]
    assert model.cells_0[0].weight_hh.grad is not None and model.cells_0[0].weight_hh.grad.shape == (3 * H, H)

    G = b.clone().to(device)
    G.bi_layer_index = torch.stack([G._bi_layer_idx0, G._bi_layer_index0, G._bi_layer_idx1, G._bi_layer_index1], dim=0).view(2, 2, -1)
    N = G.x.shape[0]
    gen = torch.Generator().manual_seed(9)
    x0 = torch.randn(N, E, generator=gen)
    cots = [torch.randn(N, H, generator=gen) for _ in range(4)]
    names = [(d, i, n) for d in model.dirs for i in range(2) for n, _ in variants._cell_params(model, d, i)]

    def grads_of(mod, GG, dtype, hip):
        x = x0.to(device, dtype).requires_grad_(True)
        params = [p for d in mod.dirs for i in range(2) for _, p in variants._cell_params(mod, d, i)]
        if hip:
            flat = variants.VariantRecurrence.apply(mod, GG, mod._plan_of(GG, num_graphs_of(GG)), x, *params)
        else:
            h = variants.run(mod, GG, x)
            flat = [h[d][i] for d in mod.dirs for i in range(2)]
        loss = sum((t * c.to(device, dtype)).sum() for t, c in zip(flat, cots))
        gr = torch.autograd.grad(loss, [x] + params, allow_unused=True)
        out = {"x": gr[0]}
        for key, p, g_ in zip(names, params, gr[1:]):   # a module shared by several cells appears several times: add up
            g_ = torch.zeros_like(p) if g_ is None else g_
            out[key[2] + "@%d" % id(p)] = g_
        return {k: v.detach().double().cpu() for k, v in out.items()}, [id(p) for p in params]

    g_hip, ids_h = grads_of(model, G, torch.float32, True)
    g_par, _ = grads_of(model, G, torch.float32, False)
    m64 = build().double().to(device).train()
    m64.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    G64 = b.clone().to(device)
    G64.bi_layer_index = G.bi_layer_index
    if getattr(G64, "edge_attr", None) is not None:
        G64.edge_attr = G64.edge_attr.double()
    g_ref, ids_r = grads_of(m64, G64, torch.float64, False)
    remap = dict(zip(ids_r, ids_h))
    g_ref = {(k.split("@")[0] + "@%d" % remap[int(k.split("@")[1])]) if "@" in k else k: v for k, v in g_ref.items()}
    report, failures = [], []
    assert set(g_ref) == set(g_hip) == set(g_par)
    for k in sorted(g_ref):
        try:
            _check_tensor(k.split("@")[0], g_hip[k], g_par[k], g_ref[k], report)
        except AssertionError as exc:
            failures.append(str(exc))
    _report((H, 2, True, 5, False), report)
    assert not failures, failures
