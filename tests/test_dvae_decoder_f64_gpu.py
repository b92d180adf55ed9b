"""The D-VAE decoder kernels (csrc/dvae_decode.hip: `loss()` and its reverse pass; csrc/dvae_sample.hip: `decode_dense()`)
against the float64 decoder oracle (`oracle/dvae_decoder_oracle.py`, pinned to the reference's fixtures by
`test_dvae_decoder_oracle_cpu.py`) at the shapes the fixtures never reach: max_n != nvt, max_n up to 32, odd and tiny
hs, L up to MAX_STACKED, B around the 64-row tiles, other START / END types, the graph families that drive the padding
width, saturated edge logits, and the sampler's per-attempt padding groups."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from dagnn_amd import dvae
from oracle import dvae_decoder_oracle as DO
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

HEADS = ("add_vertex.", "add_edge.0.weight", "add_edge.2.")
GATE = ("gate_forward.0.0.weight", "gate_forward.0.0.bias", "mapper_forward.0.0.weight")

# (name, kind, agg, max_n, nvt, hs, L, B, START_TYPE, END_TYPE, family, seed).  The seeds of the small configurations
# (fewer than SMALL ReLU inputs in add_vertex.0 / add_edge.0) are chosen so that none of those inputs lies within
# 1e-5 x max|.| of zero (asserted): there every gradient is compared elementwise at 1e-4.  The larger ones hold about
# one such input per 10 000 - float32 and float64 may put it on different sides of the kink - and are checked with the
# split rule of `_check_grads` whenever the oracle reports one.
LOSS_CASES = [
    ("na_n2_h1", "na", "attn_h", 2, 3, 1, 1, 1, 0, 1, "chain", 1),
    ("na_n3_h2_st1", "na", "attn_h", 3, 2, 2, 2, 2, 1, 0, "complete", 2),
    ("na_n9_h3_L3", "na", "attn_h", 9, 5, 3, 3, 63, 0, 1, "random0.5", 3),
    ("na_n17_h5_L5", "na", "attn_h", 17, 11, 5, 5, 64, 2, 3, "random0.2", 4),
    ("na_n31_h33_onecomplete", "na", "attn_h", 31, 11, 33, 2, 65, 0, 1, "one_complete", 5),
    ("na_n32_h65_L8_complete", "na", "attn_h", 32, 64, 65, 8, 2, 3, 63, "complete", 6),
    ("na_n17_h127_dense", "na", "attn_h", 17, 3, 127, 1, 65, 0, 1, "random0.8", 7),
    ("na_n9_h129_star", "na", "attn_h", 9, 64, 129, 2, 257, 0, 1, "star", 8),
    ("na_n32_h33_random", "na", "attn_h", 32, 5, 33, 3, 64, 4, 0, "random0.5", 9),
    ("na_n3_h257_none", "na", "attn_h", 3, 11, 257, 2, 257, 0, 1, "none", 10),
    ("na_n17_h2_B257", "na", "attn_h", 17, 5, 2, 2, 257, 1, 2, "random0.5", 11),
    ("bn_n2_h2", "bn", "attn_h", 2, 5, 2, 1, 1, 0, 1, "chain", 21),
    ("bn_n3_h3_L5_star", "bn", "attn_h", 3, 64, 3, 5, 65, 0, 1, "star", 22),
    ("bn_n9_h5_st1", "bn", "attn_h", 9, 2, 5, 2, 2, 1, 0, "random0.8", 23),
    ("bn_n17_h65_onecomplete", "bn", "attn_h", 17, 3, 65, 3, 63, 0, 1, "one_complete", 24),
    ("bn_n31_h33_complete", "bn", "attn_h", 31, 11, 33, 2, 64, 5, 1, "complete", 25),
    ("bn_n32_h127_sparse", "bn", "attn_h", 32, 5, 127, 1, 2, 0, 1, "random0.2", 26),
    ("bn_n9_h129_L8", "bn", "attn_h", 9, 11, 129, 8, 65, 0, 1, "random0.5", 27),
    ("bn_n17_h257_chain", "bn", "attn_h", 17, 2, 257, 2, 2, 1, 0, "chain", 28),
    ("gated_n2_h1_B257", "na", "gated_sum", 2, 11, 1, 2, 257, 0, 1, "chain", 31),
    ("gated_n3_h5_complete", "na", "gated_sum", 3, 5, 5, 1, 63, 0, 1, "complete", 32),
    ("gated_n9_h33_L3", "na", "gated_sum", 9, 3, 33, 3, 64, 2, 1, "random0.5", 33),
    ("gated_n17_h65_onecomplete", "na", "gated_sum", 17, 64, 65, 2, 65, 0, 1, "one_complete", 34),
    ("gated_n31_h3_L5_st1", "na", "gated_sum", 31, 2, 3, 5, 2, 1, 0, "random0.8", 35),
    ("gated_n32_h129_complete", "na", "gated_sum", 32, 11, 129, 2, 1, 0, 1, "complete", 36),
    ("gated_n9_h127_L8_star", "na", "gated_sum", 9, 5, 127, 8, 2, 0, 1, "star", 37),
    ("gated_n17_h2_none", "na", "gated_sum", 17, 3, 2, 2, 64, 0, 1, "none", 38),
    # the reference's training shape (B 32, hs 501, L 2; dvae/train.py:55) with nvt != max_n.  NA's 2 M ReLU inputs
    # always hold some within float32 rounding of 0; its seed keeps the closest at 2e-7 x max|.|
    ("na_ref_h501", "na", "attn_h", 8, 7, 501, 2, 32, 0, 1, "random0.5", 141),
    ("bn_ref_h501", "bn", "attn_h", 10, 9, 501, 2, 32, 0, 1, "random0.5", 42),
    ("gated_ref_h501", "na", "gated_sum", 8, 7, 501, 2, 32, 0, 1, "random0.5", 43),
]
CASE = {c[0]: c for c in LOSS_CASES}
SMALL = 30000


def _relu_inputs(case):
    _, kind, _, n, _, hs, _, B = case[:8]
    return (n - 1) * B * 2 * hs + n * (n - 1) // 2 * B * (hs if kind == "bn" else 4 * hs)


def _inputs(case):
    name, kind, agg, n, nvt, hs, L, B, st, en, family, seed = case
    model = Hh.dvae_decoder_model(kind, max_n=n, nvt=nvt, hs=hs, L=L, start_type=st, end_type=en, agg=agg, seed=seed)
    types, preds = Hh.dvae_dense_graphs(family, B, n, nvt, st, seed + 1000)
    rng = np.random.default_rng(seed + 2000)
    mu = torch.from_numpy(rng.standard_normal((B, model.nz)).astype(np.float32))
    logvar = torch.from_numpy((0.1 * rng.standard_normal((B, model.nz))).astype(np.float32))
    return model, types, preds, mu, logvar


def _kernel(model, types, preds, mu, logvar, device, graphs=None):
    """(ll [2B+1] of DvaeDecode.forward, loss, res, kld, mu.grad, logvar.grad) of the model on the GPU; the parameters'
    .grad hold loss()'s gradients afterwards."""
    model = model.to(device)
    spec, params = model._decode_loss_inputs()
    t_types, t_preds = torch.from_numpy(types).to(device), torch.from_numpy(preds).to(device)
    with torch.no_grad():
        H0 = torch.tanh(model.fc3(mu.to(device)))
        ll = dvae._make_decode(spec, t_types, t_preds, H0, params).forward().clone()
    model.zero_grad(set_to_none=True)
    if graphs is None:
        mu_d = mu.to(device).requires_grad_(True)
        lv_d = logvar.to(device).requires_grad_(True)
    else:
        mu_d, lv_d = model.encode([g.clone() for g in graphs])
        mu_d.retain_grad()
        lv_d.retain_grad()
    loss, res, kld = model.loss(mu_d, lv_d, Hh.dvae_graphs_from_dense(types, preds, model.nvt))
    loss.backward()
    return ll.cpu().double(), loss.detach(), res.detach(), kld.detach(), mu_d.grad, lv_d.grad


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _check_values(ll, res, ref, B):
    _, r_res, _, r_vll, r_ell, _, _ = ref
    assert abs(float(res) - float(r_res)) <= 1e-5 * abs(float(r_res)) + 1e-6, (float(res), float(r_res))
    assert abs(float(ll[2 * B]) - float(r_res)) <= 1e-5 * abs(float(r_res)) + 1e-6
    for got, want in ((ll[:B], r_vll), (ll[B:2 * B], r_ell)):
        err = (got - want).abs()
        assert (err <= 1e-5 * want.abs() + 1e-5).all(), float(err.max())
    return _rel(ll[:2 * B], torch.cat([r_vll, r_ell]))


def _check_grads(model, ref, mu_g, lv_g, split):
    """Every gradient against the oracle's: elementwise at 1e-4 x max|ref| + 2e-7, or - `split`, where some ReLU input
    lies within rounding of 0 - the heads' own weights so and what lies behind the ReLU normwise at 1e-4 and elementwise
    at 1e-2.  Returns the worst error relative to each gradient's largest entry."""
    grads = ref[5]
    worst = 0.0
    named = [("mu", mu_g), ("logvar", lv_g)] + [(k, p.grad) for k, p in model.named_parameters()]
    for k, g in named:
        r = grads.get(k, torch.zeros(g.shape if g is not None else (0,), dtype=torch.float64))
        g = torch.zeros(r.shape) if g is None else g.detach().cpu().double()
        assert g.shape == r.shape, (k, g.shape, r.shape)
        scale = float(r.abs().max()) if r.numel() else 0.0
        err = float((g - r).abs().max()) if r.numel() else 0.0
        assert torch.isfinite(g).all(), k
        if split and not k.startswith(HEADS):
            assert float((g - r).norm()) <= 1e-4 * float(r.norm()) + 2e-7, (k, float((g - r).norm()), float(r.norm()))
            assert err <= 1e-2 * scale + 2e-7, (k, err, scale)
        else:
            assert err <= 1e-4 * scale + 2e-7, (k, err, scale)
        if scale > 2e-5:
            worst = max(worst, err / scale)
    return worst


def _attn_zero_grads(model):
    if model.agg == "attn_h":   # the query half and the bias cancel inside the soft-max: exact zeros
        lin = model.node_aggr_0[0].attn_lin
        dq = model._key_offset(0)
        assert lin.weight.grad is not None and torch.equal(lin.weight.grad[0, :dq], torch.zeros_like(lin.weight.grad[0, :dq]))
        assert lin.bias.grad is None or not lin.bias.grad.any()


@pytest.mark.parametrize("case", LOSS_CASES, ids=[c[0] for c in LOSS_CASES])
def test_loss_and_gradients_match_float64_oracle(device, case):
    model, types, preds, mu, logvar = _inputs(case)
    ref = Hh.dvae_decoder64(case, model, types, preds, mu, logvar)
    diag = ref[6]
    kinks = diag["vertex_kinks"][0] + diag["edge_kinks"][0]
    if _relu_inputs(case) < SMALL:
        assert kinks == 0, (case[0], diag)   # (a seed with a near-kink ReLU input: pick another)
    split = kinks > 0
    B = types.shape[0]
    ll, loss, res, kld, mu_g, lv_g = _kernel(model, types, preds, mu, logvar, device)
    v_err = _check_values(ll, res, ref, B)
    assert abs(float(loss) - float(ref[0])) <= 1e-5 * abs(float(ref[0])) + 1e-6
    g_err = _check_grads(model, ref, mu_g, lv_g, split)
    _attn_zero_grads(model)
    print("%-28s values %.2e  gradients %.2e  (kinks %d, max |logit| %.1f)" % (case[0], v_err, g_err, kinks, diag["max_logit"]))


@pytest.mark.parametrize("name", ["na_n9_h3_L3", "bn_n9_h5_st1", "gated_n9_h33_L3"])
def test_vertex_0_type_does_not_matter(device, name):
    """The decoder sets vertex 0 to START_TYPE whatever the true graph says: any other type there gives the same loss."""
    model, types, preds, mu, logvar = _inputs(CASE[name])
    B = types.shape[0]
    other = types.copy()
    other[:, 0] = (model.START_TYPE + 1 + np.arange(B)) % model.nvt
    ll_a = _kernel(model, types, preds, mu, logvar, device)[0]
    ll_b = _kernel(model, other, preds, mu, logvar, device)[0]
    assert torch.equal(ll_a, ll_b)
    kw = dict(kind="bn" if name.startswith("bn") else "na", agg=model.agg, L=model.num_layers, start_type=model.START_TYPE)
    sd = Hh._cpu_state(model)
    H0 = torch.tanh(mu.double() @ sd["fc3.weight"].double().t() + sd["fc3.bias"].double())
    assert float(DO.decoder_loss(sd, other, preds, H0, **kw)[0]) == float(DO.decoder_loss(sd, types, preds, H0, **kw)[0])


@pytest.mark.parametrize("name", ["na_n9_h3_L3", "gated_n9_h33_L3", "bn_n9_h5_st1"])
def test_encoder_fed_mu_matches_float64_oracle(device, name):
    """mu / logvar from encode() of the same graphs: the gradients reach the encoder, and with gated_sum the layer-0
    gate / mapper gradients are the encoder's and the decoder's added."""
    model, types, preds, mu, logvar = _inputs(CASE[name])
    graphs = Hh.dvae_graphs_from_dense(types, preds, model.nvt)
    ref = Hh.dvae_decoder64((name, "encode"), model, types, preds, mu, logvar, graphs=graphs)
    _, loss, res, kld, _, _ = _kernel(model, types, preds, mu, logvar, device, graphs=graphs)
    assert abs(float(loss) - float(ref[0])) <= 1e-5 * abs(float(ref[0])) + 1e-6
    worst = Hh.check_grads_full(model, ref[5], rtol=1e-4, atol=2e-7)
    if model.agg == "gated_sum":
        for k in GATE:
            assert dict(model.named_parameters())[k].grad.abs().max() > 0
    print("%-28s encode: gradients %.2e (%s)" % (name, worst[0], worst[1]))


@pytest.mark.parametrize("name", ["na_n17_h5_L5", "bn_n9_h5_st1", "gated_n9_h33_L3"])
def test_saturated_edge_logits_match_float64_oracle(device, name):
    """add_edge.2 scaled until many edge logits pass +-30: float32 p is exactly 1 (or its BCE gradient is floored at
    1e-12), the loss hits the -100 clamp; everything stays finite and equal to the oracle's float32-BCE rule."""
    model, types, preds, mu, logvar = _inputs(CASE[name])
    probe = {}
    DO.decoder_loss_grads(Hh._cpu_state(model), types, preds, mu, logvar, diag=probe, kind="bn" if name.startswith("bn") else "na",
                          agg=model.agg, L=model.num_layers, start_type=model.START_TYPE)
    scale = 60.0 / probe["max_logit"]
    with torch.no_grad():
        model.add_edge[2].weight.mul_(scale)
        model.add_edge[2].bias.mul_(scale)
    ref = Hh.dvae_decoder64((name, "saturated"), model, types, preds, mu, logvar)
    diag = ref[6]
    assert diag["saturated"] >= 20 and diag["max_logit"] < 80, diag
    B = types.shape[0]
    ll, loss, res, kld, mu_g, lv_g = _kernel(model, types, preds, mu, logvar, device)
    assert torch.isfinite(ll).all() and torch.isfinite(loss)
    _check_values(ll, res, ref, B)
    _check_grads(model, ref, mu_g, lv_g, diag["vertex_kinks"][0] + diag["edge_kinks"][0] > 0)
    print("%-28s saturated %d logits (max %.1f): res %.6g" % (name, diag["saturated"], diag["max_logit"], float(res)))


# ------------------------------------------------------------------ the sampler
# (name, kind, agg, max_n, nvt, hs, L, B, attempts, stochastic, START_TYPE, END_TYPE, seed)
SAMPLE_CASES = [
    ("na_n17_h6_sample", "na", "attn_h", 17, 11, 6, 2, 65, 3, True, 0, 1, 51),
    ("na_n2_h1_argmax_st1", "na", "attn_h", 2, 2, 1, 1, 1, 1, False, 1, 0, 52),
    ("bn_n32_h7_sample", "bn", "attn_h", 32, 3, 7, 2, 65, 1, True, 2, 0, 53),
    ("bn_n3_h64_argmax", "bn", "attn_h", 3, 11, 64, 3, 65, 3, False, 0, 1, 54),
    ("gated_n32_h3_sample_st1", "na", "gated_sum", 32, 2, 3, 2, 65, 3, True, 1, 0, 55),
    ("na_n17_h501_sample", "na", "attn_h", 17, 3, 501, 2, 65, 1, True, 0, 2, 56),
    ("gated_n3_h64_argmax", "na", "gated_sum", 3, 11, 64, 2, 65, 1, False, 0, 1, 57),
    ("na_n32_h3_sample_st1", "na", "attn_h", 32, 2, 3, 2, 1, 3, True, 1, 0, 58),
    ("bn_n17_h6_sample_st1", "bn", "attn_h", 17, 2, 6, 1, 65, 3, True, 1, 0, 59),
]
TOL = 1e-5


@pytest.mark.parametrize("case", SAMPLE_CASES, ids=[c[0] for c in SAMPLE_CASES])
def test_decode_matches_float64_replay(device, case):
    """Every decision of decode_dense whose float64 margin exceeds 1e-5 equals the oracle's, nv / the -1 fill / the END
    edges are exact, the states agree at 1e-5 x max|ref|; each attempt of a multi-attempt call is replayed ALONE, which
    pins the per-attempt padding groups."""
    name, kind, agg, n, nvt, hs, L, B, att, stochastic, st, en, seed = case
    model = Hh.dvae_decoder_model(kind, max_n=n, nvt=nvt, hs=hs, L=L, start_type=st, end_type=en, agg=agg, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    z = torch.from_numpy(rng.standard_normal((B, model.nz)).astype(np.float32))
    sd = Hh._cpu_state(model)
    H0 = torch.tanh(z.double() @ sd["fc3.weight"].double().t() + sd["fc3.bias"].double())
    draws = None
    if stochastic:
        s_t, s_e = dvae.draw_shapes(n, B, att)
        draws = (torch.from_numpy(rng.random(s_t, dtype=np.float32)), torch.from_numpy(rng.random(s_e, dtype=np.float32)))
    model = model.to(device)
    d = model.decode_dense(z.to(device), stochastic, attempts=att,
                           draws=None if draws is None else tuple(x.to(device) for x in draws), states=True)
    types, preds, nv, states = (x.cpu() for x in (d.types, d.preds, d.nv, d.states))
    total = low = 0
    worst = 0.0
    for a in range(att):
        kw = {} if draws is None else dict(u_type=draws[0][a].numpy(), u_edge=draws[1][a].numpy())
        r = DO.replay_decode(sd, H0, types[a].numpy(), preds[a].numpy(), nv[a].numpy(), kind=kind, agg=agg, L=L,
                             start_type=st, end_type=en, tol=TOL, **kw)
        assert np.array_equal(r["types"], types[a].numpy().astype(np.int64)), a
        assert np.array_equal(r["preds"], preds[a].numpy().view(np.uint32).astype(np.int64)), a
        assert np.array_equal(r["nv"], nv[a].numpy()), a
        m = np.concatenate([r["type_margin"][r["type_margin"] < np.inf], r["edge_margin"][r["edge_margin"] < np.inf]])
        total += m.size
        low += int((m <= TOL).sum())
        ref = r["states"]
        err = float((states[a].double() - ref).abs().max())
        assert err <= 1e-5 * float(ref.abs().max()), (a, err)
        worst = max(worst, err / float(ref.abs().max()))
    assert (total > 0) == (n > 2) and low <= 0.01 * total, (low, total)   # (n = 2: vertex 1 is END, nothing to decide)
    t = types.numpy()
    if nvt == 2 and stochastic and B > 1:   # START drawn at a later vertex, END at vertex 1
        assert (t[..., 1:] == st).any() and (nv.numpy() == 2).any()
    print("%-28s %d decisions (%d within %.0e)  states %.2e" % (name, total, low, TOL, worst))
