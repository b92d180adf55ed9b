"""Input-keyed attention on the BN D-VAE (`DAGNN_BN(agg='attn_x' | 'self_attn_x')`, dvae/dagnn_bn.py:32,48-59,129-131,
203-225) without a GPU: the float64 restatement of `tests/dvae_attn_x_f64.py` against every `*_attn_x` fixture the
unmodified reference wrote - which is what lets `test_dvae_bn_attn_x_gpu.py` trust it beyond the fixtures - and the
constructor / decoder contracts of the module."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import dagnn_amd
from dagnn_amd import DAGNN_BN, DAGNN_NA, _lib, dvae
from oracle import dvae_decoder_oracle as DO
from tests import dvae_attn_x_f64 as X64
from tests import helpers as Hh

ENCODER = ["bn_h64_attn_x", "bn_h64_self_attn_x"]
GRAD = ["grad_bn_h64_attn_x", "grad_bn_h64_self_attn_x"]
LOSS = ["dvae_loss_bn_attn_x_h32_L3", "dvae_loss_bn_attn_x_h501_L2", "dvae_loss_bn_attn_x_h32_encode"]
DECODE = ["dvae_decode_bn_attn_x_h32_L3_argmax", "dvae_decode_bn_attn_x_h32_L3_sample", "dvae_decode_bn_attn_x_h501_L2_sample"]
E = 10   # emb_dim = nvt of the fixtures' models


def _enc_kw(meta):
    return dict(L=meta["L"], bidirectional=meta["bidir"], num_nodes=10, agg=meta["agg"],
                out_pool_all=meta.get("out_pool_all", False), out_pool=meta.get("out_pool", "max"))


# ------------------------------------------------------------------ the restatement reproduces the fixtures
@pytest.mark.parametrize("name", ENCODER)
@pytest.mark.parametrize("mode", ["csr", "faithful"])
def test_restated_encoder_matches_the_reference(name, mode):
    meta, arr = Hh.load(name)
    model, _ = Hh.dvae_model(meta)
    with torch.no_grad():
        Hg, mu, logvar = X64.encode(Hh._cpu_state(model), Hh.dvae_batch(arr), mode=mode, **_enc_kw(meta))
    for key, got in (("Hg", Hg), ("mu", mu), ("logvar", logvar)):
        assert Hh.maxdiff(got, arr[key]) <= 1e-5 * max(1.0, float(np.abs(arr[key]).max())), key


@pytest.mark.parametrize("name", GRAD)
def test_restated_encoder_gradients_match_the_reference(name):
    meta, arr = Hh.load(name)
    model, _ = Hh.dvae_model(meta)
    lv = X64.leaves(Hh._cpu_state(model))
    b = dagnn_amd.GraphBatch.from_data_list([g.clone() for g in Hh.dvae_graphs(meta, arr)])
    _, mu, logvar = X64.encode(lv, b, **_enc_kw(meta))
    assert Hh.maxdiff(mu, arr["mu"]) <= 1e-5 and Hh.maxdiff(logvar, arr["logvar"]) <= 1e-5
    r1, r2 = torch.from_numpy(arr["r1"]).double(), torch.from_numpy(arr["r2"]).double()
    loss = (mu * r1).sum() + (logvar * r2).sum()
    # (a signed sum of float32 terms that largely cancel: the scale of its rounding is the sum of their magnitudes)
    assert abs(float(loss.detach()) - float(arr["loss"])) <= 1e-5 * float(((mu * r1).abs().sum() + (logvar * r2).abs().sum()).detach())
    loss.backward()
    Hh.check_grads(meta, arr, X64.leaf_grads(lv))
    key = lv["node_aggr_0.0.attn_lin.weight"].grad[0, (E if meta["agg"] == "attn_x" else 0):]
    assert float(key.abs().max()) > 1e-4   # the key half takes a real gradient


def _restated_loss(name):
    meta, arr = Hh.load(name)
    model, n = Hh.dvae_model(meta)
    lv = X64.leaves(Hh._cpu_state(model))
    graphs = Hh.dvae_graphs(meta, arr)
    types, preds = dvae.decode_schedule(graphs, n, n)
    if meta["encode"]:
        b = dagnn_amd.GraphBatch.from_data_list([g.clone() for g in graphs])
        _, mu, logvar = X64.encode(lv, b, **_enc_kw(meta))
        mu.retain_grad()
        logvar.retain_grad()
    else:
        mu = torch.from_numpy(arr["mu"].copy()).double().requires_grad_(True)
        logvar = torch.from_numpy(arr["logvar"].copy()).double().requires_grad_(True)
    H0 = torch.tanh(mu @ lv["fc3.weight"].t() + lv["fc3.bias"])
    res, vll, ell = X64.decoder_loss(lv, types, preds, H0, L=meta["L"])
    kld = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
    loss = res + 0.005 * kld
    loss.backward()
    return meta, arr, (types, preds), H0.detach(), loss, res, kld, dict(X64.leaf_grads(lv), mu=mu.grad, logvar=logvar.grad)


@pytest.mark.parametrize("name", LOSS)
def test_restated_loss_and_gradients_match_the_reference(name):
    meta, arr, (types, preds), H0, loss, res, kld, grads = _restated_loss(name)
    for key, got in (("loss", loss), ("res", res), ("kld", kld)):
        ref = float(arr[key])
        assert abs(float(got.detach()) - ref) <= 1e-5 * abs(ref), (key, float(got), ref)
    Hh.check_grads(meta, arr, grads)
    g = grads["node_aggr_0.0.attn_lin.weight"][0]
    assert float(g[E:].abs().max()) > 1e-4 and float(g[:E].abs().max()) <= 1e-12   # key half; the query half cancels
    assert float(grads["node_aggr_0.0.attn_lin.bias"].abs().max()) <= 1e-12
    # the two float64 forms agree: the imported decoder oracle with the type-keyed aggregate in its model's place
    model, _ = Hh.dvae_model(meta)
    with X64.type_keyed(types, np.full(len(types), 10)), torch.no_grad():
        res2 = DO.decoder_loss(Hh._cpu_state(model), types, preds, H0, kind="bn", agg="attn_x", L=meta["L"])[0]
    assert abs(float(res2) - float(res.detach())) <= 1e-12 * abs(float(res2))
    assert dvae.update_widths(preds, 10) == DO.padding_widths(preds) == [int(x) for x in arr["widths"]]


@pytest.mark.parametrize("name", DECODE)
def test_restated_decode_replays_the_reference(name):
    meta, arr = Hh.load(name)
    model, n = Hh.dvae_model(meta)
    sd = Hh._cpu_state(model)
    z = torch.from_numpy(arr["z"].copy()).double()
    H0 = torch.tanh(z @ sd["fc3.weight"].double().t() + sd["fc3.bias"].double())
    draws = dict(u_type=arr["u_type"][0], u_edge=arr["u_edge"][0]) if meta["stochastic"] else {}
    with X64.type_keyed(arr["types"], arr["nv"]):
        r = DO.replay_decode(sd, H0, arr["types"], arr["preds"], arr["nv"], kind="bn", agg="attn_x", L=meta["L"],
                             start_type=0, end_type=1, **draws)
    assert np.array_equal(r["types"], arr["types"])
    assert np.array_equal(r["preds"], arr["preds"])
    assert np.array_equal(r["nv"], arr["nv"])
    assert float(min(r["edge_margin"].min(), r["type_margin"].min())) >= 0.5 * meta["margin"]
    ref = arr["states"]
    assert float(np.abs(r["states"].numpy() - ref).max()) <= 1e-5 * float(np.abs(ref).max())
    assert r["widths"] == [int(x) for x in arr["widths"]]
    assert meta["coverage"]["coupled_updates"] > 0   # padding took weight somewhere


# ------------------------------------------------------------------ constructor contracts
@pytest.mark.parametrize("name", ENCODER + LOSS[:1])
def test_state_dict_is_the_reference_state_dict(name):
    meta, _ = Hh.load(name)
    model, _ = Hh.dvae_model(meta)
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == meta["state_dict"]
    width = 2 * E if meta["agg"] == "attn_x" else E
    for d in (0, 1):
        for l in range(meta["L"]):
            assert tuple(getattr(model, "node_aggr_%d" % d)[l].attn_lin.weight.shape) == (1, width)
    assert [model._key_offset(i) for i in range(meta["L"])] == [E if meta["agg"] == "attn_x" else 0] * meta["L"]


@pytest.mark.parametrize("agg", ["attn_x", "self_attn_x"])
def test_na_model_refuses_input_keyed_attention(agg):
    with pytest.raises(NotImplementedError, match=r"dvae/dagnn\.py:28"):
        DAGNN_NA(8, 16, 16, 8, 8, 0, 1, hs=16, nz=4, num_nodes=8, agg=agg)


def _bn(agg, emb_dim=10, hidden_dim=16):
    return DAGNN_BN(emb_dim, hidden_dim, 16, 10, 10, 0, 1, hs=16, nz=4, num_nodes=10, agg=agg, num_layers=2).eval()


def test_static_scores_are_the_key_products():
    model = _bn("attn_x")
    x = torch.eye(10)[torch.arange(30) % 10]
    cells = {(d, i): type("C", (), {"key_raw": getattr(model, "node_aggr_%d" % d)[i].attn_lin.weight.detach()[0, E:]})()
             for d in (0, 1) for i in range(2)}
    sc = model._static_scores(x, cells)
    for (d, i), s in sc.items():
        assert torch.equal(s, x @ getattr(model, "node_aggr_%d" % d)[i].attn_lin.weight.detach()[0, E:])
    assert _bn("attn_h")._static_scores(x, cells) is None


def test_self_attn_x_decoders_raise():
    model = _bn("self_attn_x")
    z = torch.zeros(2, 4)
    for call in (lambda: model.loss(z, z, []), lambda: model.decode(z), lambda: model.decode_dense(z),
                 lambda: model.loss_dense(z, z, torch.zeros(2, 10, dtype=torch.int32), torch.zeros(2, 10, dtype=torch.int32))):
        with pytest.raises(NotImplementedError, match=r"dagnn_bn\.py:311-315"):
            call()
    with pytest.raises(NotImplementedError, match=r"dagnn_bn\.py:311-315"):
        model._ipropagate_to([Hh.VertexGraph(3)], 1, model.grud)


def test_attn_x_decoders_need_type_wide_keys():
    z = torch.zeros(2, 4)
    model = _bn("attn_x", emb_dim=12)
    for call in (lambda: model.loss(z, z, []), lambda: model.decode(z)):
        with pytest.raises(ValueError, match="emb_dim == nvt"):
            call()
    model = _bn("attn_x", hidden_dim=24)
    for call in (lambda: model.loss(z, z, []), lambda: model.decode(z)):
        with pytest.raises(ValueError, match="hidden_dim == hs"):
            call()
    for agg in ("add", "max"):   # the aggregators without a decoder still get the message that names attn_h
        with pytest.raises(NotImplementedError, match="attn_h"):
            _bn(agg).decode(z)


def test_attn_x_decoders_need_the_gpu():
    meta, arr = Hh.load("dvae_loss_bn_attn_x_h32_L3")
    model, _ = Hh.dvae_model(meta)
    mu, lv = torch.from_numpy(arr["mu"].copy()), torch.from_numpy(arr["logvar"].copy())
    with pytest.raises(_lib.DagnnHipError, match="GPU"):
        model.loss(mu, lv, Hh.dvae_graphs(meta, arr))
    with pytest.raises(_lib.DagnnHipError, match="GPU"):
        model.decode(torch.zeros(2, 56))


def test_entry_points_refuse_bad_type_keyed_arguments_without_a_gpu():
    import ctypes as C
    lib = _lib.load()
    key = (C.c_float * 8)()

    def args(cls, **kw):
        a = cls()
        a.B, a.n, a.hs, a.L, a.nvt, a.start_type, a.bn, a.edge_hidden, a.vertex_hidden = 4, 8, 16, 2, 8, 0, 1, 16, 32
        a.agg, a.key_type = 2, C.addressof(key)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert lib.dagnn_dvae_decode_saved_bytes(C.byref(args(_lib.DvaeDecodeArgsTyped))) > 0
    for kw in (dict(bn=0), dict(key_type=None), dict(agg=3)):
        assert lib.dagnn_dvae_decode_saved_bytes(C.byref(args(_lib.DvaeDecodeArgsTyped, **kw))) == 0, kw
        assert lib.dagnn_dvae_decode_forward(C.byref(args(_lib.DvaeDecodeArgsTyped, **kw)), None) == -22, kw
    assert lib.dagnn_dvae_sample_work_bytes(C.byref(args(_lib.DvaeSampleArgsTyped, G=1, end_type=1))) > 0
    for kw in (dict(bn=0), dict(key_type=None), dict(agg=3)):
        assert lib.dagnn_dvae_sample_work_bytes(C.byref(args(_lib.DvaeSampleArgsTyped, G=1, end_type=1, **kw))) == 0, kw
    # the new fields are appended with no padding in front, and a zero-filled struct is still agg = 0
    for old, new, name in ((_lib.DvaeDecodeArgs, _lib.DvaeDecodeArgsTyped, "key_type"), (_lib.DvaeSampleArgs, _lib.DvaeSampleArgsTyped, "key_type"),
                           (_lib.DvaeDecodeGrads, _lib.DvaeDecodeGradsTyped, "d_key_type")):
        assert getattr(new, name).offset == C.sizeof(old) and C.sizeof(new) == C.sizeof(old) + 8
    assert _lib.DvaeDecodeArgsTyped().agg == 0 and not _lib.DvaeDecodeArgsTyped().key_type
    layer = (_lib.IpropLayer * 1)()
    assert lib.dagnn_iprop_step_typed(None, None, 2, 3, 16, None, 8, None, None, 8, layer, 1, None, None) == -22
    assert lib.dagnn_iprop_step_typed(None, None, 2, 3, 16, C.addressof(key), 0, None, None, 8, layer, 1, None, None) == -22
