"""The D-VAE performance predictor on the GPU (csrc/predictor.hip, dagnn_amd/predictor.py): `dagnn_predictor_mse`,
`dagnn_predictor_forward`, `dagnn_fit_sums` and the loops around them.

  * against the reference's own `--predictor` step (`dvae_predictor_*` fixtures): encode, loss and predictor_mse, all HIP;
  * against float64 at the edges of the kernel, by the rule of test_train_tail_gpu.py: the largest error of every output in
    units of 2^-24 x (the sum of |terms| of that element's own sum, in float64) is at most 4 x the same figure of torch's own
    fp32 ops on the same inputs and device - torch's figure taken as the largest over all cases of this file, measured once
    (a single case where torch's arithmetic happens to be nearly exact would leave no fp32 kernel room).  DESIGN.md 15
    records the ratios measured on an MI355X;
  * bitwise: repeatability, no_grad = grad values, `predict_latent` = `predictor_mse` row by row and chunk by chunk."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch
from torch import nn

from dagnn_amd import DagStore, _lib, attach_predictor, engine, predict_latent, predictor_mse, predictor_report, synth
from dagnn_amd import predictor as P
from dagnn_amd.dvae_store import test_predictor as store_test_predictor
from dagnn_amd.dvae_store import train_epoch
from oracle.seeding import seeded_fill
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FIXTURES = ["dvae_predictor_na_h64", "dvae_predictor_bn_h32"]
KEYS = ["predictor.0.weight", "predictor.0.bias", "predictor.2.weight", "predictor.2.bias"]
TILE = _lib.PREDICTOR_ROWS
# (B, nz, hs): the smallest; one row at the reference's widths; widths that are no multiple of 4 or of a wave; a row more than
# four tiles; the reference's training shape; the limits of both widths with a row more than eight tiles; two tiles and a row
SHAPES = [(1, 1, 1), (1, 56, 501), (3, 57, 63), (33, 56, 64), (32, 56, 501), (65, 128, 1024), (2 * TILE + 1, 56, 501)]
OUTPUTS = ("y_pred", "loss", "dmu", "dW1", "db1", "dW2", "db2")


class _Holder(nn.Module):
    """What `attach_predictor` needs of a model: nz and hs."""

    def __init__(self, nz, hs):
        super().__init__()
        self.nz, self.hs = nz, hs


def _case(B, nz, hs, strided, device):
    """Seeded inputs: mu ~ N(0, 1) (contiguous, or a view of a [B, 2 nz + 3] tensor whose other columns hold NaN), y in
    [0, 1], weights as nn.Linear draws them."""
    gen = torch.Generator().manual_seed(100000 * B + 1000 * nz + hs + (7 if strided else 0))
    mu = torch.randn(B, nz, generator=gen)
    y = torch.rand(B, generator=gen)
    lim1, lim2 = nz ** -0.5, hs ** -0.5
    W1 = (torch.rand(hs, nz, generator=gen) * 2 - 1) * lim1
    b1 = (torch.rand(hs, generator=gen) * 2 - 1) * lim1
    W2 = (torch.rand(1, hs, generator=gen) * 2 - 1) * lim2
    b2 = (torch.rand(1, generator=gen) * 2 - 1) * lim2
    if strided:
        wide = torch.full((B, 2 * nz + 3), float("nan"))
        wide[:, 2:2 + nz] = mu
        mu = wide.to(device)[:, 2:2 + nz]
        assert mu.stride(0) == 2 * nz + 3 and not (B > 1 and mu.is_contiguous())
    else:
        mu = mu.to(device)
    model = attach_predictor(_Holder(nz, hs)).to(device)
    with torch.no_grad():
        for p, v in zip(model.predictor.parameters(), (W1, b1, W2, b2)):
            p.copy_(v.to(device))
    return model, mu, y.to(device)


def _ref64(model, mu, y):
    """Every output in float64 with the sum of |terms| of each element's own sum."""
    W1, b1, W2, b2 = (p.detach().double() for p in model.predictor.parameters())
    m, t = mu.detach().double(), y.double()
    h = torch.tanh(m @ W1.t() + b1)
    yp = h @ W2[0] + b2
    d = yp - t
    dy = 2.0 * d
    dpre = dy[:, None] * W2 * (1.0 - h * h)
    val = dict(y_pred=yp, loss=(d * d).sum(), dmu=dpre @ W1, dW1=dpre.t() @ m, db1=dpre.sum(0), dW2=(dy[:, None] * h).sum(0),
               db2=dy.sum())
    mag = dict(y_pred=h.abs() @ W2[0].abs() + b2.abs(), loss=(d * d).sum(), dmu=dpre.abs() @ W1.abs(), dW1=dpre.abs().t() @ m.abs(),
               db1=dpre.abs().sum(0), dW2=(dy[:, None] * h).abs().sum(0), db2=dy.abs().sum())
    return val, mag


def _ratios(got, ref):
    val, mag = ref
    out = {}
    for k in OUTPUTS:
        g = got[k].detach().double().reshape(val[k].shape)
        assert bool(torch.isfinite(g).all()), k
        out[k] = float(((g - val[k]).abs() / (U * mag[k])).max())
    return out


def _run(model, mu, y, fused, grad_mu=True):
    """All seven outputs of the fused call (`predictor_mse`) or of the torch-ops form (train.py:245-246 + autograd)."""
    model.zero_grad(set_to_none=True)
    leaf = mu.detach().requires_grad_(grad_mu)
    if fused:
        loss, y_pred = predictor_mse(model, leaf, y)
    else:
        y_pred = model.predictor(leaf)
        loss = model.mseloss(y_pred, y.unsqueeze(1))
    loss.backward()
    l1, l2 = model.predictor[0], model.predictor[2]
    return dict(y_pred=y_pred.detach().reshape(-1), loss=loss.detach(), dmu=leaf.grad, dW1=l1.weight.grad, db1=l1.bias.grad,
                dW2=l2.weight.grad.reshape(-1), db2=l2.bias.grad.reshape(()))


@pytest.fixture(scope="module")
def torch_ratios(device):
    """The error of torch's own fp32 ops (Linear, Tanh, Linear, MSELoss and their autograd) against float64 in the units of
    `_ref64`, per output, the largest over every case of this file: computed once, the kernel gets 4 x each."""
    worst = {k: 0.0 for k in OUTPUTS}
    for B, nz, hs in SHAPES:
        for strided in (False, True):
            model, mu, y = _case(B, nz, hs, strided, device)
            r = _ratios(_run(model, mu, y, fused=False), _ref64(model, mu, y))
            worst = {k: max(worst[k], r[k]) for k in OUTPUTS}
    print("torch fp32 against float64 (units of 2^-24 sum|terms|): " + ", ".join("%s %.3f" % (k, worst[k]) for k in OUTPUTS))
    assert all(0.0 < v < float("inf") for v in worst.values()), worst
    return worst


# =========================================================================== the reference's step
def fixture_model(meta):
    model, _ = Hh.dvae_model(meta)
    attach_predictor(model)
    seeded_fill(model, meta["w_seed"])
    return model


@pytest.mark.parametrize("name", FIXTURES)
def test_step_matches_the_reference(device, name):
    """dvae/train.py:241-255 with the predictor: encode (HIP), loss (HIP), predictor_mse (HIP), backward.  Values at rtol 1e-5;
    the gradients of mu, logvar and of every parameter - encoder, decoder, the predictor's four - at the tolerances of
    test_dvae_loss_gpu.py::test_loss_and_gradients_match_the_reference."""
    meta, arr = Hh.load(name)
    model = fixture_model(meta).to(device).eval()
    graphs = Hh.dvae_graphs(meta, arr)
    y = torch.from_numpy(arr["y"].copy()).to(device)
    mu, logvar = model.encode([g.clone() for g in graphs])
    mu.retain_grad()
    logvar.retain_grad()
    loss, res, kld = model.loss(mu, logvar, graphs)
    pred, y_pred = predictor_mse(model, mu, y)
    loss = loss + pred
    loss.backward()
    for key, got in (("loss", loss), ("res", res), ("kld", kld), ("pred", pred)):
        ref = float(arr[key])
        print("%s %s: got %.8g ref %.8g" % (name, key, float(got.detach()), ref))
        assert abs(float(got.detach()) - ref) <= 1e-5 * abs(ref) + 1e-6, (key, float(got.detach()), ref)
    assert tuple(y_pred.shape) == (meta["B"], 1)
    assert Hh.maxdiff(y_pred.reshape(-1), arr["y_pred"]) <= 1e-5 * float(np.abs(arr["y_pred"]).max()) + 1e-6
    grads = {"mu": mu.grad, "logvar": logvar.grad}
    sd = model.state_dict()
    for k, p in model.named_parameters():
        grads[k] = p.grad if p.grad is not None else torch.zeros_like(p)
    for k in list(grads):   # aliased encoder GRUs (cells_0 == grue_forward)
        if k in sd:
            for k2, v2 in sd.items():
                if k2 not in grads and v2.data_ptr() == sd[k].data_ptr():
                    grads[k2] = grads[k]
    assert all(float(grads[k].abs().sum()) > 0 for k in KEYS)
    worst = Hh.check_grads(meta, arr, grads, rtol=2e-4, atol=2e-7, verbose=True)
    print("%s: worst relative gradient error %.3e" % (name, worst))


# =========================================================================== float64 at the edges of the kernel
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("B,nz,hs", SHAPES)
def test_predictor_mse_matches_float64(device, torch_ratios, B, nz, hs, strided):
    model, mu, y = _case(B, nz, hs, strided, device)
    got = _run(model, mu, y, fused=True)
    assert tuple(got["dmu"].shape) == (B, nz) and tuple(got["dW1"].shape) == (hs, nz)
    r = _ratios(got, _ref64(model, mu, y))
    print("B %d nz %d hs %d%s: " % (B, nz, hs, " strided" if strided else "") + ", ".join("%s %.3f" % (k, r[k]) for k in OUTPUTS))
    for k in OUTPUTS:
        assert r[k] <= 4 * torch_ratios[k], (k, r[k], torch_ratios[k])


# =========================================================================== bitwise properties
@pytest.mark.parametrize("B,nz,hs", [(32, 56, 501), (65, 128, 1024)])
def test_bitwise_repeatable_and_no_grad_equals_grad(device, B, nz, hs):
    model, mu, y = _case(B, nz, hs, False, device)
    one = _run(model, mu, y, fused=True)
    one = {k: v.clone() for k, v in one.items()}
    two = _run(model, mu, y, fused=True)
    for k in OUTPUTS:
        assert torch.equal(one[k], two[k]), k
    with torch.no_grad():
        loss, y_pred = predictor_mse(model, mu, y)
    assert not loss.requires_grad
    assert torch.equal(loss, one["loss"]) and torch.equal(y_pred.reshape(-1), one["y_pred"])
    # a row scored by either entry point gives the same bits, wherever it lies in a tile
    assert torch.equal(predict_latent(model, mu), one["y_pred"])
    rows = [B - 1, 0, B // 2]
    assert torch.equal(predict_latent(model, mu[rows]), one["y_pred"][rows])
    assert int(engine._lp_counter(mu)[0]) == 0


@pytest.mark.parametrize("M", [1, TILE + 1, 5000])
def test_predict_latent_equals_itself_in_chunks(device, M):
    model, _, _ = _case(4, 56, 501, False, device)
    Z = torch.randn(M, 56, generator=torch.Generator().manual_seed(M))
    whole = predict_latent(model, Z.numpy())                       # a numpy array, as bo.py holds Z_train
    assert tuple(whole.shape) == (M,) and whole.is_cuda and bool(torch.isfinite(whole).all())
    for rows in (1, TILE - 1, 1001):
        if rows < M or rows == 1:
            assert torch.equal(predict_latent(model, Z.to(device), batch_rows=rows), whole), rows
    with torch.no_grad():
        ref = model.predictor(Z.to(device)).reshape(-1)
    assert Hh.maxdiff(whole, ref) <= 1e-5


# =========================================================================== upstream gradient, gradient skipping
def test_upstream_gradient_scales_and_mu_gradient_is_skipped(device):
    model, mu, y = _case(33, 56, 64, False, device)
    one = {k: v.clone() for k, v in _run(model, mu, y, fused=True).items()}
    model.zero_grad(set_to_none=True)
    leaf = mu.detach().requires_grad_(True)
    loss, _ = predictor_mse(model, leaf, y)
    (3.0 * loss).backward()
    l1, l2 = model.predictor[0], model.predictor[2]
    three = dict(dmu=leaf.grad, dW1=l1.weight.grad, db1=l1.bias.grad, dW2=l2.weight.grad.reshape(-1), db2=l2.bias.grad.reshape(()))
    for k, g in three.items():
        want = 3.0 * one[k].double()
        assert bool(((g.double() - want).abs() <= U * want.abs()).all()), k      # one rounding of the product by 3
        assert float(g.abs().sum()) > 0, k
    none = _run(model, mu, y, fused=True, grad_mu=False)
    assert none["dmu"] is None
    for k in ("y_pred", "loss", "dW1", "db1", "dW2", "db2"):
        assert torch.equal(none[k], one[k]), k


def test_parameters_are_read_in_place_on_every_call(device):
    model, mu, y = _case(32, 56, 501, False, device)
    with torch.no_grad():
        first = predictor_mse(model, mu, y)[0].clone()
        model.predictor[0].weight.data.mul_(0.5)
        model.predictor[2].bias.data.add_(0.25)
        second = predictor_mse(model, mu, y)[0]
        scores = predict_latent(model, mu)
    fresh = copy.deepcopy(model)
    with torch.no_grad():
        want, y_pred = predictor_mse(fresh, mu, y)
    assert torch.equal(second, want) and not torch.equal(second, first)
    assert torch.equal(scores, y_pred.reshape(-1))


def test_forward_and_backward_do_not_synchronise(device):
    model, mu, y = _case(32, 56, 501, False, device)
    _run(model, mu, y, fused=True)   # (warm-up: library load, allocator, the counter word)
    predict_latent(model, mu)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _run(model, mu, y, fused=True)
        predict_latent(model, mu)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


# =========================================================================== fit sums
@pytest.mark.parametrize("M", [1, 257, 5000])
def test_fit_sums_match_numpy_float64(device, M):
    """Each of the six sums within M 2^-52 sum|terms| of numpy float64, for fp32 and float64 y; rmse / pearson of
    `predictor_report` are the formulas on those sums."""
    rng = np.random.default_rng(M)
    pred = (rng.standard_normal(M) * 0.05 - 0.72).astype(np.float32)
    mean, std = -0.7213, 0.0456
    p = (-pred.astype(np.float64) - mean) / std
    for y in (rng.standard_normal(M), rng.standard_normal(M).astype(np.float32)):
        t = y.astype(np.float64)
        terms = [p, t, p * p, t * t, p * t, (p - t) ** 2]
        got = engine.fit_sums(torch.from_numpy(pred).to(device), torch.from_numpy(y).to(device), mean, std)
        again = engine.fit_sums(torch.from_numpy(pred).to(device), torch.from_numpy(y).to(device), mean, std)
        assert got.dtype == torch.float64 and torch.equal(got, again)
        got = got.cpu().numpy()
        assert np.array_equal(P.fit_sums_host(pred, y, mean, std), np.array([v.sum() for v in terms]))
        for q, v in enumerate(terms):
            bound = M * 2.0 ** -52 * np.abs(v).sum()
            print("M %d sum %d: err %.3e bound %.3e" % (M, q, abs(got[q] - v.sum()), bound))
            assert abs(got[q] - v.sum()) <= bound, (q, got[q], v.sum())
    assert int(engine._lp_counter(torch.zeros(1, device=device))[0]) == 0
    model, _, _ = _case(4, 56, 64, False, device)
    Z = rng.standard_normal((M, 56)).astype(np.float32)
    Y = rng.standard_normal(M)
    rep = predictor_report(model, Z, Y, mean, std)
    sums = engine.fit_sums(predict_latent(model, Z), torch.from_numpy(Y).to(device), mean, std).tolist()
    assert rep == P._report(sums, M) or (M == 1 and np.isnan(rep["pearson"]) and rep["rmse"] == P._report(sums, M)["rmse"])
    pz = (-predict_latent(model, Z).double().cpu().numpy() - mean) / std
    assert abs(rep["rmse"] - np.sqrt(np.mean((pz - Y) ** 2))) <= 1e-12 * rep["rmse"] and rep["n"] == M
    if M > 1:
        assert abs(rep["pearson"] - np.corrcoef(pz, Y)[0, 1]) <= 1e-9


# =========================================================================== the loops
def _loop_setup(device):
    rows = synth.enas_rows(77, 64)
    y = np.random.default_rng(78).uniform(0.0, 1.0, 64).astype(np.float32)
    st = DagStore.from_rows(rows, "ENAS", nvt=8, device=device, y=y)
    meta = dict(kind="na", hs=64, L=2, bidir=False, w_seed=79)
    base = fixture_model(meta).to(device)
    return st, y, base


def test_train_epoch_and_test_predictor_equal_the_loops_by_hand(device):
    """Three optimizer steps (48 graphs, B = 16) of `train_epoch(predictor=True)` against the same steps written with
    encode_batch, loss_dense and predictor_mse: losses and parameters bitwise.  `test_predictor` against its hand loop."""
    st, y, base = _loop_setup(device)
    ids = list(range(60, 12, -1))
    model = copy.deepcopy(base)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    torch.manual_seed(31)
    got = train_epoch(model, opt, st, ids, 16, clip=0.25, predictor=True)
    hand = copy.deepcopy(base).train()
    opt = torch.optim.Adam(hand.parameters(), lr=1e-3)
    torch.manual_seed(31)
    sums = None
    for i in range(0, 48, 16):
        b = st.batch(ids[i:i + 16])
        opt.zero_grad()
        types, preds = b.types, b.preds
        mu, logvar = hand.encode_batch(b)
        loss, recon, kld = hand.loss_dense(mu, logvar, types, preds)
        pred = predictor_mse(hand, mu, b.y)[0]
        loss = loss + pred
        loss.backward()
        torch.nn.utils.clip_grad_norm_(hand.parameters(), 0.25)
        part = torch.stack([t.detach().reshape(()) for t in (loss, recon, kld, pred)])
        sums = part if sums is None else sums + part
        opt.step()
    assert len(got) == 4 and got == tuple(float(v) for v in sums.tolist()) and all(np.isfinite(got)) and got[3] > 0
    moved = 0
    for (k, p), (_, q), (_, r) in zip(model.named_parameters(), hand.named_parameters(), base.named_parameters()):
        assert torch.equal(p, q), k
        moved += int(not torch.equal(p, r))
    assert moved > 8 and all(not torch.equal(model.state_dict()[k], base.state_dict()[k]) for k in KEYS)
    # test_predictor
    ev = list(range(64))
    rmse = store_test_predictor(model, st, ev, 24)
    assert model.training
    model.eval()
    total = None
    with torch.no_grad():
        for i in range(0, 64, 24):
            b = st.batch(ev[i:i + 24])
            yb = b.y
            mu, _ = model.encode_batch(b)
            se = predictor_mse(model, mu, yb)[0]
            total = se if total is None else total + se
    assert rmse == float(np.sqrt(float(total) / 64)) and rmse > 0
    assert store_test_predictor(model, st, ev, 24) == rmse and not model.training


def test_first_step_gradients_equal_the_torch_ops_form(device):
    """Step 1 of the loop with `predictor_mse` against the same step with the predictor on torch ops (train.py:245-246 and
    autograd): every parameter's gradient at the tolerances of the reference step's test."""
    st, y, base = _loop_setup(device)
    ids = list(range(16))
    grads = []
    for fused in (True, False):
        model = copy.deepcopy(base).train()
        torch.manual_seed(41)
        b = st.batch(ids)
        types, preds = b.types, b.preds
        mu, logvar = model.encode_batch(b)
        loss, _, _ = model.loss_dense(mu, logvar, types, preds)
        if fused:
            loss = loss + predictor_mse(model, mu, b.y)[0]
        else:
            loss = loss + model.mseloss(model.predictor(mu), b.y.unsqueeze(1))
        loss.backward()
        grads.append((float(loss.detach()), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}))
    (l1, g1), (l2, g2) = grads
    assert abs(l1 - l2) <= 1e-5 * abs(l2)
    assert sorted(g1) == sorted(g2) and set(KEYS) <= set(g1)
    for k in g2:
        scale = float(g2[k].abs().max())
        assert Hh.maxdiff(g1[k], g2[k]) <= 2e-4 * scale + 2e-7, (k, Hh.maxdiff(g1[k], g2[k]), scale)


# =========================================================================== limits
def test_widths_over_the_limits_raise_before_any_launch(device):
    mu = torch.zeros(4, 129, device=device)
    y = torch.zeros(4, device=device)
    with pytest.raises(ValueError, match="nz <= 128"):
        attach_predictor(_Holder(129, 8))
    with pytest.raises(ValueError, match="hs <= 1024"):
        attach_predictor(_Holder(8, 1025))
    for nz, hs in ((129, 8), (8, 1025)):
        model = _Holder(nz, hs)
        model.predictor = nn.Sequential(nn.Linear(nz, hs), nn.Tanh(), nn.Linear(hs, 1)).to(device)   # (set by hand)
        model.mseloss = nn.MSELoss(reduction="sum")
        x = torch.zeros(4, nz, device=device)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(ValueError, match="nz <= 128 and 1 <= hs <= 1024"):
                predictor_mse(model, x, y)
            with pytest.raises(ValueError, match="nz <= 128 and 1 <= hs <= 1024"):
                predict_latent(model, x)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    # the engine and the library refuse them too (no silent clamp)
    W1, b1 = torch.zeros(8, 129, device=device), torch.zeros(8, device=device)
    with pytest.raises(engine.DagnnHipError, match="nz <= 128"):
        engine.predictor_mse(mu, y, W1, b1, torch.zeros(1, 8, device=device), torch.zeros(1, device=device), True, True)
