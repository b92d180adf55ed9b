"""`DAGNN_NA.loss` / `DAGNN_BN.loss` (the teacher-forced decoder of dvae/models_pyg.py:398-456 in HIP,
csrc/dvae_decode.hip) against the reference's own `loss()` and `.backward()` (`dvae_loss_*` fixtures)."""
from __future__ import annotations

import os
import subprocess
import sys

import pytest
import torch

from tests import helpers as Hh

pytestmark = pytest.mark.gpu

SMALL = ["dvae_loss_na_h64_L2", "dvae_loss_bn_h32_L3", "dvae_loss_na_h64_encode"]
WIDE = ["dvae_loss_na_h501_L2", "dvae_loss_bn_h501_L2"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(name, device, grad=True):
    """(loss, res, kld, {name: gradient}) of our model on the fixture's inputs."""
    meta, arr = Hh.load(name)
    model, _ = Hh.dvae_model(meta)
    model = model.to(device).eval()
    graphs = Hh.dvae_graphs(meta, arr)
    with torch.set_grad_enabled(grad):
        if meta["encode"]:
            mu, logvar = model.encode([g.clone() for g in graphs])
            mu.retain_grad()
            logvar.retain_grad()
        else:
            mu = torch.from_numpy(arr["mu"].copy()).to(device).requires_grad_(grad)
            logvar = torch.from_numpy(arr["logvar"].copy()).to(device).requires_grad_(grad)
        loss, res, kld = model.loss(mu, logvar, graphs)
    grads = {}
    if grad:
        loss.backward()
        grads = {"mu": mu.grad, "logvar": logvar.grad}
        sd = model.state_dict()
        for k, p in model.named_parameters():
            grads[k] = p.grad if p.grad is not None else torch.zeros_like(p)
        for k in list(grads):   # aliased encoder GRUs (cells_0 == grue_forward)
            if k in sd:
                for k2, v2 in sd.items():
                    if k2 not in grads and v2.data_ptr() == sd[k].data_ptr():
                        grads[k2] = grads[k]
    return meta, arr, model, loss, res, kld, grads


def _check_values(arr, loss, res, kld, rtol=1e-5):
    for key, got in (("loss", loss), ("res", res), ("kld", kld)):
        ref = float(arr[key])
        assert abs(float(got.detach()) - ref) <= rtol * abs(ref) + 1e-6, (key, float(got), ref)


@pytest.mark.parametrize("name", SMALL)
def test_loss_and_gradients_match_the_reference(device, name):
    meta, arr, model, loss, res, kld, grads = _run(name, device)
    _check_values(arr, loss, res, kld)
    # the query half and the bias of attn_lin cancel inside the soft-max: exact zeros here, rounding noise in the reference
    # (check_grads compares them against the atol)
    Hh.check_grads(meta, arr, grads, rtol=2e-4, atol=2e-7)


HEADS = ("add_vertex.", "add_edge.0.weight", "add_edge.2.")


@pytest.mark.parametrize("name", WIDE)
def test_reference_training_shape_matches_the_reference(device, name):
    """B = 32, hs = 501, L = 2 (scripts/na_train.sh).  Values at rtol 1e-5, the heads' own weight gradients at 2e-4.  The
    gradients that flow back through add_edge's ReLU (its bias, then the states, grud, fc3, mu) are compared at 1e-2: the
    edge head has 0.9 M (NA: 1.8 M) pre-activations, and the few that lie within fp32 rounding of 0 take the other side
    of the ReLU in one implementation or the other - each such flip moves those gradients by |dlogit * w2[c]| (the
    sampled add_edge.0.weight rows happen to hold none)."""
    meta, arr, model, loss, res, kld, grads = _run(name, device)
    _check_values(arr, loss, res, kld)
    heads = {k for k in arr if k.startswith("g::") and k[3:].startswith(HEADS)}
    Hh.check_grads(meta, {k: arr[k] for k in arr if k in heads or k.startswith("gsum::")}, grads, rtol=2e-4, atol=2e-7)
    Hh.check_grads(meta, {k: arr[k] for k in arr if k not in heads}, grads, rtol=1e-2, atol=2e-7)


@pytest.mark.parametrize("name", ["dvae_loss_na_h64_L2", "dvae_loss_bn_h32_L3"])
def test_no_grad_values_equal_grad_values(device, name):
    _, arr, _, loss, res, kld, _ = _run(name, device, grad=True)
    _, _, _, loss2, res2, kld2, _ = _run(name, device, grad=False)
    assert not loss2.requires_grad
    assert torch.equal(loss.detach(), loss2) and torch.equal(res.detach(), res2) and torch.equal(kld.detach(), kld2)


@pytest.mark.parametrize("name", ["dvae_loss_na_h501_L2", "dvae_loss_bn_h32_L3"])
def test_loss_and_gradients_are_bitwise_repeatable(device, name):
    _, _, _, loss, _, _, g1 = _run(name, device)
    _, _, _, loss2, _, _, g2 = _run(name, device)
    assert torch.equal(loss.detach(), loss2.detach())
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_train_mode_loss_is_the_eval_loss_at_the_sampled_z(device):
    meta, arr = Hh.load("dvae_loss_na_h64_L2")
    model, _ = Hh.dvae_model(meta)
    model = model.to(device)
    graphs = Hh.dvae_graphs(meta, arr)
    mu = torch.from_numpy(arr["mu"].copy()).to(device)
    logvar = torch.from_numpy(arr["logvar"].copy()).to(device)
    with torch.no_grad():
        torch.manual_seed(7)
        z = model.train().reparameterize(mu, logvar)
        assert not torch.equal(z, mu)
        torch.manual_seed(7)
        loss_t, res_t, kld_t = model.train().loss(mu, logvar, graphs)
        _, res_e, kld_e = model.eval().loss(z, logvar, graphs)
    assert torch.equal(res_t, res_e)
    assert torch.equal(kld_t, -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp()))


def test_loss_and_backward_do_not_synchronise(device):
    meta, arr = Hh.load("dvae_loss_bn_h32_L3")
    model, _ = Hh.dvae_model(meta)
    model = model.to(device).eval()
    graphs = Hh.dvae_graphs(meta, arr)
    mu = torch.from_numpy(arr["mu"].copy()).to(device).requires_grad_(True)
    logvar = torch.from_numpy(arr["logvar"].copy()).to(device).requires_grad_(True)
    model.loss(mu, logvar, graphs)[0].backward()   # (warm-up: library load, allocator)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, _, _ = model.loss(mu, logvar, graphs)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["na", "bn"])
def test_reference_training_step_runs(device, kind):
    """`dvae/train.py:241-257`'s step - encode, loss, backward, clip 0.25, Adam - for a few steps on a fixed batch: the
    loss stays finite and goes down."""
    from dagnn_amd import DAGNN_BN, DAGNN_NA, synth
    torch.manual_seed(0)
    if kind == "na":
        graphs = [synth.decode_enas_row(r) for r in synth.enas_rows(5, 16)]
        model = DAGNN_NA(8, 32, 32, 8, 8, 0, 1, hs=32, nz=16, num_nodes=8, num_layers=2, bidirectional=False)
    else:
        graphs = [synth.decode_bn_row(r) for r in synth.bn_rows(5, 16)]
        model = DAGNN_BN(10, 32, 32, 10, 10, 0, 1, hs=32, nz=16, num_nodes=10, num_layers=2, bidirectional=True)
    model = model.to(device).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        mu, logvar = model.encode([g.clone() for g in graphs])
        loss, recon, kld = model.loss(mu, logvar, graphs)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 0.25)
        opt.step()
        losses.append(float(loss))
    assert all(torch.isfinite(torch.tensor(losses)))
    assert losses[-1] < losses[0]
    assert model.grud[0].weight_hh.grad.abs().sum() > 0 and model.fc3.weight.grad.abs().sum() > 0
    assert model.add_edge[0].weight.grad.abs().sum() > 0 and model.fc1.weight.grad.abs().sum() > 0


def test_train_step_script_runs(device):
    out = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "dvae_train_step.py"), "--steps", "3", "--warmup", "1",
                          "--batch", "8", "--hs", "64"], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "enas" in out.stdout and "bn" in out.stdout
