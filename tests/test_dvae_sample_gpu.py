"""`DAGNN_NA.decode` / `DAGNN_BN.decode` (the sampling decoder of dvae/models_pyg.py:338-396 in HIP,
csrc/dvae_sample.hip) against the reference's own `decode()` (`dvae_decode_*` fixtures, replayed with their draws),
plus the per-attempt independence, structural invariants and sampling statistics at R >= 16 000 rows."""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dagnn_amd import _lib, dvae
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

FIXTURES = ["dvae_decode_na_h64_L2_argmax", "dvae_decode_bn_h32_L3_argmax", "dvae_decode_na_h64_L2_sample",
            "dvae_decode_bn_h32_L3_sample", "dvae_decode_na_h501_L2_sample", "dvae_decode_bn_h501_L2_sample"]


def _model(meta, device):
    model, _ = Hh.dvae_model(meta)
    return model.to(device).eval()


def _replay(name, device, states=True):
    meta, arr = Hh.load(name)
    model = _model(meta, device)
    z = torch.from_numpy(arr["z"].copy()).to(device)
    draws = None
    if meta["stochastic"]:
        draws = (torch.from_numpy(arr["u_type"].copy()).to(device), torch.from_numpy(arr["u_edge"].copy()).to(device))
    d = model.decode_dense(z, stochastic=meta["stochastic"], draws=draws, states=states)
    return meta, arr, model, z, d


@pytest.mark.parametrize("name", FIXTURES)
def test_decode_matches_the_reference(device, name):
    meta, arr, model, z, d = _replay(name, device)
    nv, types, preds = d.nv[0].cpu().numpy(), d.types[0].cpu().numpy(), d.preds[0].cpu().numpy()
    assert np.array_equal(nv, arr["nv"])
    assert np.array_equal(types, arr["types"])
    assert np.array_equal(preds.view(np.uint32).astype(np.int64), arr["preds"])
    ref = arr["states"]
    err = float(np.abs(d.states[0].cpu().numpy() - ref).max())
    assert err <= 1e-5 * float(np.abs(ref).max()), (name, err)
    if not meta["stochastic"]:   # the public call: host graphs equal to the reference's, edges in its insertion order
        graphs = model.decode(z, stochastic=False)
        assert len(graphs) == meta["B"]
        for b, g in enumerate(graphs):
            assert g.vcount() == arr["nv"][b] and list(g.vs["type"]) == list(arr["types"][b, :arr["nv"][b]])
            assert [list(e) for e in g.get_edgelist()] == meta["edge_order"][b]
            assert g.vs.attributes() == ["type"]


def test_attempts_equal_separate_calls(device):
    """Groups never see each other: k attempts in one call equal k calls on the same draws (bitwise)."""
    meta, arr = Hh.load("dvae_decode_na_h64_L2_sample")
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


@pytest.mark.parametrize("name", ["dvae_decode_na_h64_L2_sample", "dvae_decode_bn_h32_L3_sample"])
def test_structural_invariants_at_16k_rows(device, name):
    meta, arr = Hh.load(name)
    model = _model(meta, device)
    z = torch.from_numpy(arr["z"].copy()).to(device)
    attempts = (16000 + z.shape[0] - 1) // z.shape[0]
    torch.manual_seed(5)
    d = model.decode_dense(z, True, attempts=attempts)
    n = model.max_n
    types = d.types.view(-1, n).cpu().numpy()
    preds = d.preds.view(-1, n).cpu().numpy().view(np.uint32).astype(np.int64)
    nv = d.nv.view(-1).cpu().numpy()
    assert types.shape[0] >= 16000
    assert (nv >= 2).all() and (nv <= n).all()
    assert (types[:, 0] == model.START_TYPE).all()
    ids = np.arange(n)
    inside = ids[None, :] < nv[:, None]
    assert ((types >= 0) == inside).all() and (preds[~inside] == 0).all()
    end = types == model.END_TYPE
    assert (end.sum(1) == 1).all() and end[np.arange(len(nv)), nv - 1].all()
    assert (preds[:, 0] == 0).all()
    assert ((preds >> ids[None, :]) == 0).all()   # edges only from lower to higher ids
    succ = np.bitwise_or.reduce(preds, axis=1)   # bit u: u has an out-edge
    has_succ = (succ[:, None] >> ids[None, :]) & 1
    need = inside & (ids[None, :] < (nv - 1)[:, None])
    assert (has_succ[need] == 1).all()   # every vertex but END has an out-edge
    assert (preds[np.arange(len(nv)), nv - 1] > 0).all()


@pytest.mark.parametrize("name", ["dvae_decode_na_h64_L2_sample", "dvae_decode_bn_h32_L3_sample"])
def test_first_type_frequencies_follow_the_softmax(device, name):
    meta, arr = Hh.load(name)
    model = _model(meta, device)
    z = torch.from_numpy(arr["z"][:1].copy()).to(device)
    N = 20000
    torch.manual_seed(9)
    d = model.decode_dense(z, True, attempts=N)
    t1 = d.types[:, 0, 1].cpu().numpy()
    with torch.no_grad():   # the model's own first step, in torch
        H0 = torch.tanh(model.fc3(z))
        hv = F.one_hot(torch.tensor([model.START_TYPE], device=device), model.nvt).float()
        for cell in list(model.grud)[:model.num_layers]:
            hv = cell(hv, H0)
        p = torch.softmax(model.add_vertex(hv), 1)[0].double().cpu().numpy()
    freq = np.bincount(t1, minlength=model.nvt) / N
    sigma = np.sqrt(p * (1 - p) / N)
    assert (np.abs(freq - p) <= 4 * sigma + 1e-12).all(), (freq, p)


def test_same_seed_gives_bitwise_equal_decodes(device):
    meta, arr = Hh.load("dvae_decode_bn_h501_L2_sample")
    model = _model(meta, device)
    z = torch.from_numpy(arr["z"].copy()).to(device)
    out = []
    for _ in range(2):
        torch.manual_seed(123)
        out.append(model.decode_dense(z, True, attempts=4, states=True))
    for k in ("types", "preds", "nv", "states"):
        assert torch.equal(getattr(out[0], k), getattr(out[1], k)), k
    torch.manual_seed(124)
    other = model.decode_dense(z, True, attempts=4)
    assert not torch.equal(other.preds, out[0].preds)


def test_decode_dense_does_not_synchronise(device):
    meta, arr = Hh.load("dvae_decode_na_h64_L2_sample")
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


def test_decode_returns_host_graphs(device):
    meta, arr = Hh.load("dvae_decode_bn_h32_L3_sample")
    model = _model(meta, device)
    z = torch.from_numpy(arr["z"].copy()).to(device)
    torch.manual_seed(1)
    graphs = model.decode(z)
    assert len(graphs) == z.shape[0]
    for g in graphs:
        assert g.vs[0]["type"] == model.START_TYPE and g.vs[g.vcount() - 1]["type"] == model.END_TYPE
        assert g.is_dag()


def test_decode_raises_for_bad_arguments_on_the_gpu(device):
    meta, arr = Hh.load("dvae_decode_na_h64_L2_argmax")
    model = _model(meta, device)
    z = torch.from_numpy(arr["z"].copy()).to(device)
    with pytest.raises(ValueError, match="nz"):
        model.decode(z[:, :3])
    with pytest.raises(ValueError, match="draws"):
        model.decode_dense(z, True, draws=(torch.rand(1, 3, 3, device=device), torch.rand(1, 3, 3, device=device)))
    with pytest.raises(ValueError, match="attempts"):
        model.decode_dense(z, True, attempts=0)
    model.max_n = 40
    with pytest.raises(ValueError, match="32"):
        model.decode(z)
    model_add, _ = Hh.dvae_model(dict(meta, agg="add"))
    with pytest.raises(NotImplementedError, match="attn_h"):
        model_add.to(device).decode(z)
