"""`DAGNN_NA(agg='gated_sum')`'s D-VAE decoder (the gated_sum paths of csrc/dvae_decode.hip and csrc/dvae_sample.hip)
against the reference's own `loss()` / `.backward()` and `decode()` for `DAGNN(agg='gated_sum')` (`dvae_gated_*`
fixtures), plus repeatability, independence of attempts, structural invariants and a short training loop."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from dagnn_amd import dvae
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

GATE = ("gate_forward.0.0.weight", "gate_forward.0.0.bias", "mapper_forward.0.0.weight")
HEADS = ("add_vertex.", "add_edge.0.weight", "add_edge.2.")
DECODE = ["dvae_gated_decode_na_h64_L2_argmax", "dvae_gated_decode_na_h64_L2_sample", "dvae_gated_decode_na_h501_L2_sample"]


def _loss(name, device):
    """(meta, arr, loss, res, kld, {name: gradient}) of our model on the fixture's inputs."""
    meta, arr = Hh.load(name)
    assert meta["agg"] == "gated_sum"
    model, _ = Hh.dvae_model(meta)
    model = model.to(device).eval()
    graphs = Hh.dvae_graphs(meta, arr)
    if meta["encode"]:
        mu, logvar = model.encode([g.clone() for g in graphs])
        mu.retain_grad()
        logvar.retain_grad()
    else:
        mu = torch.from_numpy(arr["mu"].copy()).to(device).requires_grad_(True)
        logvar = torch.from_numpy(arr["logvar"].copy()).to(device).requires_grad_(True)
    loss, res, kld = model.loss(mu, logvar, graphs)
    loss.backward()
    grads = {"mu": mu.grad, "logvar": logvar.grad}
    sd = model.state_dict()
    for k, p in model.named_parameters():
        grads[k] = p.grad if p.grad is not None else torch.zeros_like(p)
    for k in list(grads):   # aliased names (cells_0 == grue_forward, node_aggr_0.0.gate == gate_forward.0)
        if k in sd:
            for k2, v2 in sd.items():
                if k2 not in grads and v2.data_ptr() == sd[k].data_ptr():
                    grads[k2] = grads[k]
    return meta, arr, loss, res, kld, grads


def _check_values(arr, loss, res, kld, rtol=1e-5):
    for key, got in (("loss", loss), ("res", res), ("kld", kld)):
        ref = float(arr[key])
        assert abs(float(got.detach()) - ref) <= rtol * abs(ref) + 1e-6, (key, float(got), ref)


@pytest.mark.parametrize("name", ["dvae_gated_loss_na_h64_L2", "dvae_gated_loss_na_h64_encode"])
def test_gated_loss_and_gradients_match_the_reference(device, name):
    """Every gradient at 2e-4, the layer-0 gate and mapper included; with `encode`, their gradients are the encoder's and
    the decoder's contributions added in one .grad."""
    meta, arr, loss, res, kld, grads = _loss(name, device)
    _check_values(arr, loss, res, kld)
    for k in GATE:
        assert "g::" + k in arr and float(grads[k].abs().max()) > 0, k
    Hh.check_grads(meta, arr, grads, rtol=2e-4, atol=2e-7)


def test_gated_loss_at_the_reference_training_shape(device):
    """B = 32, hs = 501, L = 2.  Values at 1e-5; the heads' own weight gradients at 2e-4; what flows back through
    add_edge's ReLU (the states, grud, the gate and mapper, fc3, mu) at 1e-2, as in test_dvae_loss_gpu.py."""
    meta, arr, loss, res, kld, grads = _loss("dvae_gated_loss_na_h501_L2", device)
    _check_values(arr, loss, res, kld)
    heads = {k for k in arr if k.startswith("g::") and k[3:].startswith(HEADS)}
    Hh.check_grads(meta, {k: arr[k] for k in arr if k in heads or k.startswith("gsum::")}, grads, rtol=2e-4, atol=2e-7)
    Hh.check_grads(meta, {k: arr[k] for k in arr if k not in heads}, grads, rtol=1e-2, atol=2e-7)


def test_gated_loss_is_bitwise_repeatable(device):
    _, _, loss, _, _, g1 = _loss("dvae_gated_loss_na_h64_L2", device)
    _, _, loss2, _, _, g2 = _loss("dvae_gated_loss_na_h64_L2", device)
    assert torch.equal(loss.detach(), loss2.detach())
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def _model(meta, device):
    model, _ = Hh.dvae_model(meta)
    return model.to(device).eval()


@pytest.mark.parametrize("name", DECODE)
def test_gated_decode_matches_the_reference(device, name):
    meta, arr = Hh.load(name)
    assert meta["agg"] == "gated_sum"
    model = _model(meta, device)
    z = torch.from_numpy(arr["z"].copy()).to(device)
    draws = None
    if meta["stochastic"]:
        draws = (torch.from_numpy(arr["u_type"].copy()).to(device), torch.from_numpy(arr["u_edge"].copy()).to(device))
    d = model.decode_dense(z, stochastic=meta["stochastic"], draws=draws, states=True)
    assert np.array_equal(d.nv[0].cpu().numpy(), arr["nv"])
    assert np.array_equal(d.types[0].cpu().numpy(), arr["types"])
    assert np.array_equal(d.preds[0].cpu().numpy().view(np.uint32).astype(np.int64), arr["preds"])
    ref = arr["states"]
    err = float(np.abs(d.states[0].cpu().numpy() - ref).max())
    assert err <= 1e-5 * float(np.abs(ref).max()), (name, err)
    if not meta["stochastic"]:
        graphs = model.decode(z, stochastic=False)
        for b, g in enumerate(graphs):
            assert list(g.vs["type"]) == list(arr["types"][b, :arr["nv"][b]])
            assert [list(e) for e in g.get_edgelist()] == meta["edge_order"][b]


def test_gated_attempts_equal_separate_calls(device):
    meta, arr = Hh.load("dvae_gated_decode_na_h64_L2_sample")
    model = _model(meta, device)
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


def test_gated_same_seed_gives_bitwise_equal_decodes(device):
    meta, arr = Hh.load("dvae_gated_decode_na_h501_L2_sample")
    model = _model(meta, device)
    z = torch.from_numpy(arr["z"].copy()).to(device)
    out = []
    for _ in range(2):
        torch.manual_seed(123)
        out.append(model.decode_dense(z, True, attempts=4, states=True))
    for k in ("types", "preds", "nv", "states"):
        assert torch.equal(getattr(out[0], k), getattr(out[1], k)), k
    torch.manual_seed(124)
    assert not torch.equal(model.decode_dense(z, True, attempts=4).preds, out[0].preds)


def test_gated_decode_dense_does_not_synchronise(device):
    meta, arr = Hh.load("dvae_gated_decode_na_h64_L2_sample")
    model = _model(meta, device)
    z = torch.from_numpy(arr["z"].copy()).to(device)
    model.decode_dense(z, True, attempts=2)   # (warm-up: library load, allocator)
    model.decode_dense(z, False)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        model.decode_dense(z, True, attempts=2)
        model.decode_dense(z, False, states=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_gated_structural_invariants_at_500x32_rows(device):
    meta, arr = Hh.load("dvae_gated_decode_na_h501_L2_sample")
    model = _model(meta, device)
    z = torch.from_numpy(arr["z"].copy()).to(device)
    assert z.shape[0] == 32
    torch.manual_seed(5)
    d = model.decode_dense(z, True, attempts=500, states=True)
    n = model.max_n
    types = d.types.view(-1, n).cpu().numpy()
    preds = d.preds.view(-1, n).cpu().numpy().view(np.uint32).astype(np.int64)
    nv = d.nv.view(-1).cpu().numpy()
    assert types.shape[0] == 16000
    assert bool(torch.isfinite(d.states).all())
    assert (nv >= 2).all() and (nv <= n).all()
    assert (types[:, 0] == model.START_TYPE).all()
    ids = np.arange(n)
    inside = ids[None, :] < nv[:, None]
    assert ((types >= 0) == inside).all() and (preds[~inside] == 0).all()
    end = types == model.END_TYPE
    assert (end.sum(1) == 1).all() and end[np.arange(len(nv)), nv - 1].all()
    assert (preds[:, 0] == 0).all()
    assert ((preds >> ids[None, :]) == 0).all()   # edges only from lower to higher ids
    succ = np.bitwise_or.reduce(preds, axis=1)
    has_succ = (succ[:, None] >> ids[None, :]) & 1
    need = inside & (ids[None, :] < (nv - 1)[:, None])
    assert (has_succ[need] == 1).all()   # every vertex but END has an out-edge
    assert (preds[np.arange(len(nv)), nv - 1] > 0).all()


def test_gated_training_step_runs(device):
    """`dvae/train.py:241-257`'s step with agg='gated_sum' - encode, loss, backward, clip 0.25, Adam - for a few steps on
    a fixed batch: the loss stays finite and goes down, and the shared gate / mapper receive gradients."""
    from dagnn_amd import DAGNN_NA, synth
    torch.manual_seed(0)
    graphs = [synth.decode_enas_row(r) for r in synth.enas_rows(5, 16)]
    model = DAGNN_NA(8, 32, 32, 8, 8, 0, 1, hs=32, nz=16, num_nodes=8, num_layers=2, bidirectional=False,
                     agg="gated_sum").to(device).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        mu, logvar = model.encode([g.clone() for g in graphs])
        loss, _, _ = model.loss(mu, logvar, graphs)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 0.25)
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0]
    assert model.gate_forward[0][0].weight.grad.abs().sum() > 0 and model.mapper_forward[0][0].weight.grad.abs().sum() > 0
    assert model.grud[0].weight_hh.grad.abs().sum() > 0 and model.fc1.weight.grad.abs().sum() > 0
