"""CPU tier (-m "not gpu") of the D-VAE performance predictor (dagnn_amd/predictor.py, `train_epoch(predictor=True)`): the
checkpoint contract, the host mirror of `predictor_mse` against the reference's own step (`dvae_predictor_*` fixtures), the
loops on a CPU store, the fit sums' definition, argument errors and the library's exports."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch
from torch import nn

from dagnn_amd import DagStore, _lib, attach_predictor, predict_latent, predictor_mse, predictor_report, synth
from dagnn_amd import predictor as P
from dagnn_amd.dvae_store import test_predictor as store_test_predictor
from dagnn_amd.dvae_store import train_epoch
from oracle.seeding import seeded_fill
from tests import helpers as Hh

FIXTURES = ["dvae_predictor_na_h64", "dvae_predictor_bn_h32"]
KEYS = ["predictor.0.weight", "predictor.0.bias", "predictor.2.weight", "predictor.2.bias"]


def fixture_model(meta):
    """Our model of a `dvae_predictor_*` fixture: the D-VAE model of the loss fixtures, the predictor attached, then the
    seeded fill over ALL keys (the generator fills the reference model after attaching, too)."""
    model, _ = Hh.dvae_model(meta)
    attach_predictor(model)
    seeded_fill(model, meta["w_seed"])
    return model.eval()


# ------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_is_the_references(name):
    meta, _ = Hh.load(name)
    model = fixture_model(meta)
    sd = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert list(sd.items()) == list(meta["state_dict"].items())   # names, shapes and order
    assert list(sd)[-4:] == KEYS
    assert sd[KEYS[0]] == [meta["hs"], 56] and sd[KEYS[2]] == [1, meta["hs"]]
    fresh, _ = Hh.dvae_model(meta)
    with pytest.raises(RuntimeError):      # without the predictor the keys are unknown
        fresh.load_state_dict(model.state_dict(), strict=True)
    attach_predictor(fresh)
    fresh.load_state_dict({k: v.clone() for k, v in model.state_dict().items()}, strict=True)
    for k in KEYS:
        assert torch.equal(fresh.state_dict()[k], model.state_dict()[k])
    assert isinstance(model.mseloss, nn.MSELoss) and model.mseloss.reduction == "sum"
    assert {k for k, _ in model.named_parameters()} >= set(KEYS)     # ordinary parameters: the optimizer sees them
    assert attach_predictor(Hh.dvae_model(meta)[0], hs=7).predictor[0].out_features == 7


# ------------------------------------------------------------------ the host mirror against the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_host_mirror_matches_the_reference(name):
    meta, arr = Hh.load(name)
    model = fixture_model(meta)
    B = meta["B"]
    forms = [torch.from_numpy(arr["y"].copy()), torch.from_numpy(arr["y"].copy()).view(B, 1), [float(v) for v in arr["y"]]]
    for y in forms:
        model.zero_grad(set_to_none=True)
        mu = torch.from_numpy(arr["mu"].copy()).requires_grad_(True)
        pred, y_pred = predictor_mse(model, mu, y)
        assert tuple(y_pred.shape) == (B, 1) and pred.dim() == 0
        ref = float(arr["pred"])
        assert abs(float(pred.detach()) - ref) <= 1e-5 * abs(ref) + 1e-6
        assert np.abs(y_pred.detach().numpy().reshape(-1) - arr["y_pred"]).max() <= 1e-5 * np.abs(arr["y_pred"]).max() + 1e-6
        pred.backward()
        grads = {k: p.grad for k, p in model.named_parameters() if k in KEYS}
        assert sorted(grads) == sorted(KEYS) and mu.grad is not None
        only = {k: v for k, v in arr.items() if k.startswith(("g::predictor.", "gsum::predictor."))}
        assert len(only) == 8
        Hh.check_grads(meta, only, grads, rtol=2e-4, atol=2e-7)
    with torch.no_grad():
        pred2, y_pred2 = predictor_mse(model, torch.from_numpy(arr["mu"].copy()), forms[0])
    assert torch.equal(pred2, pred.detach()) and not pred2.requires_grad
    assert torch.equal(predict_latent(model, arr["mu"]), y_pred2.reshape(-1))
    assert torch.equal(predict_latent(model, torch.from_numpy(arr["mu"].copy()), batch_rows=5), y_pred2.reshape(-1))


# ------------------------------------------------------------------ the loops on a CPU store
class _TorchDvae(nn.Module):
    """A stand-in with the two calls `train_epoch` makes, on torch ops (the real `loss_dense` is HIP only): enough to check
    what the loop adds up and steps."""

    def __init__(self, n, nvt, nz=6, hs=5):
        super().__init__()
        self.nz, self.hs, self.n, self.nvt = nz, hs, n, nvt
        self.fc1, self.fc2 = nn.Linear(n * nvt, nz), nn.Linear(n * nvt, nz)
        self.out = nn.Linear(nz, n)

    def encode_batch(self, b):
        x = b.x.view(-1, self.n * self.nvt)
        return self.fc1(x), self.fc2(x)

    def loss_dense(self, mu, logvar, types, preds, beta=0.005):
        res = ((self.out(mu) - types.float()) ** 2).sum()
        kld = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
        return res + beta * kld, res, kld


def _cpu_store(with_y=True):
    rows = synth.enas_rows(9, 21)
    y = np.random.default_rng(3).uniform(0.0, 1.0, 21).astype(np.float32)
    return DagStore.from_rows(rows, "ENAS", nvt=8, device="cpu", y=y if with_y else None), y


def test_train_epoch_with_the_predictor_equals_the_loop_by_hand():
    st, y = _cpu_store()
    torch.manual_seed(5)
    base = attach_predictor(_TorchDvae(8, 8))
    ids = list(range(20, -1, -1))                                # batches of 8, 8 and 5
    model = copy.deepcopy(base)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    got = train_epoch(model, opt, st, ids, 8, clip=0.25, predictor=True)
    hand = copy.deepcopy(base).train()
    opt = torch.optim.Adam(hand.parameters(), lr=1e-2)
    sums = torch.zeros(4)
    for i in range(0, 21, 8):
        b = st.batch(ids[i:i + 8])
        opt.zero_grad()
        mu, logvar = hand.encode_batch(b)
        loss, recon, kld = hand.loss_dense(mu, logvar, b.types, b.preds)
        pred = hand.mseloss(hand.predictor(mu), torch.from_numpy(y[ids[i:i + 8]]).unsqueeze(1))    # train.py:244-247
        loss = loss + pred
        loss.backward()
        torch.nn.utils.clip_grad_norm_(hand.parameters(), 0.25)
        sums += torch.stack([loss.detach(), recon.detach(), kld.detach(), pred.detach()])
        opt.step()
    assert len(got) == 4 and got == tuple(float(v) for v in sums.tolist())
    assert abs(got[0] - (got[1] + 0.005 * got[2] + got[3])) <= 1e-4 * abs(got[0])
    for (k, p), (_, q) in zip(model.named_parameters(), hand.named_parameters()):
        assert torch.equal(p, q), k
    assert not torch.equal(model.predictor[0].weight, base.predictor[0].weight)   # the predictor trains with the rest
    # test_predictor: sqrt(sum of squared errors / len(idx)) in evaluation mode, the mode restored
    rmse = store_test_predictor(model, st, ids, 8)
    assert model.training
    with torch.no_grad():
        mu, _ = model.encode_batch(st.batch(ids))
        want = float(np.sqrt(float(((model.predictor(mu).reshape(-1) - torch.from_numpy(y[ids])) ** 2).sum()) / 21))
    assert abs(rmse - want) <= 1e-6 * want and rmse > 0


def test_train_epoch_default_is_unchanged_and_needs_y_for_the_predictor():
    st, _ = _cpu_store()
    torch.manual_seed(6)
    base = attach_predictor(_TorchDvae(8, 8))
    ids = list(range(21))
    res = []
    for kw in ({}, {"predictor": False}):
        model = copy.deepcopy(base)
        res.append(train_epoch(model, torch.optim.Adam(model.parameters(), lr=1e-2), st, ids, 8, **kw))
    hand = copy.deepcopy(base).train()
    opt = torch.optim.Adam(hand.parameters(), lr=1e-2)
    sums = torch.zeros(3)
    for i in range(0, 21, 8):
        b = st.batch(ids[i:i + 8])
        opt.zero_grad()
        loss, recon, kld = hand.loss_dense(*hand.encode_batch(b), b.types, b.preds)
        loss.backward()
        sums += torch.stack([loss.detach(), recon.detach(), kld.detach()])
        opt.step()
    assert len(res[0]) == 3 and res[0] == res[1] == tuple(float(v) for v in sums.tolist())
    assert torch.equal(model.predictor[0].weight, base.predictor[0].weight)       # no gradient reaches it
    bare, _ = _cpu_store(with_y=False)
    model = copy.deepcopy(base)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    with pytest.raises(ValueError, match="no y"):
        train_epoch(model, opt, bare, ids, 8, predictor=True)
    with pytest.raises(ValueError, match="no y"):
        store_test_predictor(model, bare, ids, 8)
    with pytest.raises(ValueError, match="attach_predictor"):
        train_epoch(_TorchDvae(8, 8), opt, st, ids, 8, predictor=True)


# ------------------------------------------------------------------ fit sums
@pytest.mark.parametrize("M", [1, 257])
def test_fit_sums_host_and_report_match_numpy(M):
    rng = np.random.default_rng(M)
    pred = rng.standard_normal(M).astype(np.float32) * 0.1 - 0.7
    y = rng.standard_normal(M)
    mean, std = -0.72, 0.09
    p = (-pred.astype(np.float64) - mean) / std                       # bo.py:253
    want = np.array([p.sum(), y.sum(), (p * p).sum(), (y * y).sum(), (p * y).sum(), ((p - y) ** 2).sum()])
    got = P.fit_sums_host(torch.from_numpy(pred), y, mean, std)
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-14, atol=0)
    rep = P._report(got, M)
    assert rep["n"] == M and abs(rep["rmse"] - np.sqrt(np.mean((p - y) ** 2))) <= 1e-12 * rep["rmse"]      # bo.py:265
    if M > 1:
        assert abs(rep["pearson"] - np.corrcoef(p, y)[0, 1]) <= 1e-10                                        # bo.py:269
    else:
        assert np.isnan(rep["pearson"])
    # the whole call on a CPU predictor
    torch.manual_seed(1)
    model = attach_predictor(_TorchDvae(8, 8))
    Z = rng.standard_normal((M, 6)).astype(np.float32)
    rep = predictor_report(model, Z, y, mean, std)
    with torch.no_grad():
        p = (-model.predictor(torch.from_numpy(Z)).reshape(-1).double().numpy() - mean) / std
    assert rep["n"] == M and abs(rep["rmse"] - np.sqrt(np.mean((p - y) ** 2))) <= 1e-12 * rep["rmse"]


# ------------------------------------------------------------------ argument errors
def test_argument_errors():
    class Shape(object):
        def __init__(self, nz, hs):
            self.nz, self.hs = nz, hs

    for nz, hs in ((P.MAX_NZ + 1, 8), (8, P.MAX_HS + 1), (0, 8)):
        with pytest.raises(ValueError, match="nz <= %d.*hs <= %d" % (P.MAX_NZ, P.MAX_HS)):
            attach_predictor(Shape(nz, hs))
    assert (P.MAX_NZ, P.MAX_HS) == (128, 1024)
    wide = _TorchDvae(8, 8)
    wide.predictor = nn.Sequential(nn.Linear(6, P.MAX_HS + 1), nn.Tanh(), nn.Linear(P.MAX_HS + 1, 1))   # (set by hand)
    wide.mseloss = nn.MSELoss(reduction="sum")
    with pytest.raises(ValueError, match="hs <= 1024"):
        predictor_mse(wide, torch.zeros(3, 6), torch.zeros(3))
    with pytest.raises(ValueError, match="hs <= 1024"):
        predict_latent(wide, torch.zeros(3, 6))
    model = attach_predictor(_TorchDvae(8, 8))
    mu = torch.zeros(3, 6)
    with pytest.raises(ValueError, match="one score per row"):
        predictor_mse(model, mu, torch.zeros(4))
    with pytest.raises(ValueError, match="one score per row"):
        predictor_mse(model, mu, [0.5, 0.5])
    with pytest.raises(ValueError, match=r"\[B\] or \[B, 1\]"):
        predictor_mse(model, mu, torch.zeros(1, 3))
    with pytest.raises(ValueError, match="nz=6"):
        predictor_mse(model, torch.zeros(3, 7), torch.zeros(3))
    with pytest.raises(ValueError, match="nz=6"):
        predict_latent(model, np.zeros((3, 5), np.float32))
    with pytest.raises(ValueError, match="batch_rows"):
        predict_latent(model, np.zeros((3, 6), np.float32), batch_rows=0)
    bare = _TorchDvae(8, 8)
    for call in (lambda: predictor_mse(bare, mu, torch.zeros(3)), lambda: predict_latent(bare, mu),
                 lambda: predictor_report(bare, mu, np.zeros(3), 0.0, 1.0)):
        with pytest.raises(ValueError, match="attach_predictor"):
            call()
    with pytest.raises(ValueError, match="one value per row"):
        predictor_report(model, mu, np.zeros(2), 0.0, 1.0)
    with pytest.raises(ValueError, match="std"):
        predictor_report(model, mu, np.zeros(3), 0.0, 0.0)


# ------------------------------------------------------------------ the library
def test_library_exports_the_predictor_symbols():
    lib = _lib.load()
    for name in ("dagnn_predictor_mse", "dagnn_predictor_forward", "dagnn_fit_sums"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    # argument checks come before any HIP call: widths over the limits, a pitch below the width, no rows, a short workspace
    assert lib.dagnn_predictor_mse_bytes(32, 56, 501, 1) == 4 * 4 * (501 * 56 + 2 * 501 + 2)
    assert lib.dagnn_predictor_mse_bytes(32, 56, 501, 0) == 4 * 4
    assert lib.dagnn_predictor_mse_bytes(32, 129, 501, 1) == 0 and lib.dagnn_predictor_mse_bytes(32, 56, 1025, 1) == 0
    a = 4096   # (never dereferenced: every call below is refused on the host)
    mse = lambda B=4, nz=8, hs=8, ld=8, nb=1 << 20, w=a: lib.dagnn_predictor_mse(a, ld, a, B, nz, hs, a, a, a, a, a, a, None, w, nb, a, 1, None)   # noqa: E731
    assert mse(nz=129) == -22 and mse(hs=1025) == -22 and mse(nz=0) == -22 and mse(B=0) == -22 and mse(ld=7) == -22
    assert mse(w=None) == -22 and mse(w=a + 2) == -22 and mse(nb=16) == -28
    fwd = lambda M=4, nz=8, hs=8, ld=8, z=a: lib.dagnn_predictor_forward(z, ld, M, nz, hs, a, a, a, a, a, None)   # noqa: E731
    assert fwd(nz=129) == -22 and fwd(hs=1025) == -22 and fwd(ld=7) == -22 and fwd(M=-1) == -22 and fwd(z=None) == -22
    assert fwd(M=0) == 0
    assert lib.dagnn_fit_sums_bytes(1) == 48 and lib.dagnn_fit_sums_bytes(0) == 0
    assert lib.dagnn_fit_sums(a, a, 0, 0, 0.0, 1.0, a, a, 1 << 20, a, None) == -22
    assert lib.dagnn_fit_sums(a, a, 0, 5000, 0.0, 1.0, a, a, 8, a, None) == -28
