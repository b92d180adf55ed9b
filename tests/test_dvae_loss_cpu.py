"""Host side of the teacher-forced D-VAE decoder (`loss()`, csrc/dvae_decode.hip): the schedule, argument checks of the
C entry points, and the errors `loss()` raises - none of it needs a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from dagnn_amd import _lib, dvae
from tests import helpers as Hh

LOSS = ["dvae_loss_na_h64_L2", "dvae_loss_bn_h32_L3", "dvae_loss_na_h501_L2", "dvae_loss_bn_h501_L2",
        "dvae_loss_na_h64_encode"]


@pytest.mark.parametrize("name", LOSS)
def test_schedule_gives_the_reference_padding_width_of_every_update(name):
    """P of every `_update_iv` call, as the reference's `_ipropagate_to` saw it (recorded in the fixture), from the
    host schedule (types, predecessor bitmasks) the device derives its widths from."""
    meta, arr = Hh.load(name)
    n = 8 if meta["kind"] == "na" else 10
    graphs = Hh.dvae_graphs(meta, arr)
    types, preds = dvae.decode_schedule(graphs, n, n)
    assert types.shape == preds.shape == (len(graphs), n) and types.dtype == preds.dtype == np.int32
    assert dvae.update_widths(preds, n) == [int(x) for x in arr["widths"]]
    assert len(arr["widths"]) == (36 if n == 8 else 55)


def _args(**kw):
    a = _lib.DvaeDecodeArgs()
    a.B, a.n, a.hs, a.L, a.nvt, a.start_type, a.bn, a.edge_hidden, a.vertex_hidden = 4, 8, 16, 2, 8, 0, 0, 64, 32
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_decode_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    good = _args()
    assert lib.dagnn_dvae_decode_saved_bytes(C.byref(good)) > 0
    assert lib.dagnn_dvae_decode_work_bytes(C.byref(good)) > 0
    bad = [dict(B=0), dict(n=1), dict(n=33), dict(hs=0), dict(L=0), dict(L=9), dict(nvt=0), dict(start_type=8),
           dict(bn=2), dict(edge_hidden=0), dict(vertex_hidden=-1)]
    for kw in bad:
        a = _args(**kw)
        assert lib.dagnn_dvae_decode_saved_bytes(C.byref(a)) == 0, kw
        assert lib.dagnn_dvae_decode_forward(C.byref(a), None) == -22, kw
        assert lib.dagnn_dvae_decode_backward(C.byref(a), C.byref(_lib.DvaeDecodeGrads()), None) == -22, kw
    # a well-shaped struct with null pointers is refused before any HIP call
    assert lib.dagnn_dvae_decode_forward(C.byref(good), None) == -22
    assert lib.dagnn_dvae_decode_forward(None, None) == -22
    assert lib.dagnn_dvae_decode_backward(C.byref(good), None, None) == -22


def _model_and_graphs(name="dvae_loss_na_h64_L2", **over):
    meta, arr = Hh.load(name)
    model, _ = Hh.dvae_model(dict(meta, **over))
    graphs = Hh.dvae_graphs(meta, arr)
    mu = torch.from_numpy(arr["mu"].copy())
    lv = torch.from_numpy(arr["logvar"].copy())
    return model, graphs, mu, lv


def test_loss_raises_on_graphs_shorter_than_max_n():
    model, graphs, mu, lv = _model_and_graphs()
    g = graphs[3]
    g.x = g.x[:-1]
    with pytest.raises(ValueError, match="max_n"):
        model.loss(mu, lv, graphs)


def test_loss_raises_for_other_aggregators():
    model, graphs, mu, lv = _model_and_graphs(agg="add")
    with pytest.raises(NotImplementedError, match="attn_h"):
        model.loss(mu, lv, graphs)


def test_loss_raises_for_a_model_off_the_gpu():
    model, graphs, mu, lv = _model_and_graphs()
    with pytest.raises(_lib.DagnnHipError, match="GPU"):
        model.loss(mu, lv, graphs)


def test_reparameterize_follows_the_mode():
    model, graphs, mu, lv = _model_and_graphs()
    assert model.eval().reparameterize(mu, lv) is mu
    torch.manual_seed(3)
    z = model.train().reparameterize(mu, lv)
    torch.manual_seed(3)
    eps = torch.randn_like(mu) * 0.01
    assert torch.equal(z, eps.mul(lv.mul(0.5).exp()).add(mu))


def test_schedule_refuses_start_type_after_vertex_0():
    """The reference reads START_TYPE at a vertex >= 1 as padding and does not add that vertex (models_pyg.py:413-414),
    which shifts every later index; the kernel would compute something else, so the schedule refuses it."""
    model, graphs, mu, lv = _model_and_graphs()
    n = model.max_n
    types, _ = dvae.decode_schedule(graphs, n, n, 0)
    assert (types[:, 1:] != 0).all()
    for st in (2, 5):   # another START_TYPE that the graphs do use at a later vertex
        b, v = (int(x[0]) for x in np.nonzero(types[:, 1:] == st))
        with pytest.raises(ValueError, match="vertex %d of graph %d has START_TYPE=%d" % (v + 1, b, st)):
            dvae.decode_schedule(graphs, n, n, st)
    types0 = types[:, 0].copy()   # vertex 0 may carry any type: the decoder sets it to START_TYPE itself
    g = graphs[0]
    g.vs[0]["type"] = 3
    t2, _ = dvae.decode_schedule(graphs, n, n, 0)
    assert t2[0, 0] == 3 and np.array_equal(t2[1:, 0], types0[1:])
    model.START_TYPE = int(types[0, 2])
    with pytest.raises(ValueError, match="START_TYPE"):
        model.loss(mu, lv, graphs)


@pytest.mark.parametrize("kind", ["na", "bn"])
def test_decoders_refuse_attention_keys_of_another_width(kind):
    """attn_h's key half of attn_lin is hidden_dim (+ num_nodes for NA) wide; the decoders read hs (+ max_n) columns of
    it, so a model whose widths differ is refused (the reference fails with a shape error)."""
    from dagnn_amd import DAGNN_BN, DAGNN_NA
    cls, n = (DAGNN_NA, 8) if kind == "na" else (DAGNN_BN, 10)
    bad = [dict(hidden_dim=24)] + ([dict(num_nodes=9)] if kind == "na" else [])
    for kw in bad:
        args = dict(hidden_dim=16, num_nodes=n)
        args.update(kw)
        model = cls(n, args["hidden_dim"], 16, n, n, 0, 1, hs=16, nz=4, num_nodes=args["num_nodes"], num_layers=2)
        z = torch.zeros(2, 4)
        with pytest.raises(ValueError, match="hidden_dim == hs"):
            model.decode(z)
        with pytest.raises(ValueError, match="hidden_dim == hs"):
            model.loss(z, z, [])
    ok = cls(n, 16, 16, n, n, 0, 1, hs=16, nz=4, num_nodes=20 if kind == "bn" else n, num_layers=2)
    with pytest.raises(_lib.DagnnHipError, match="GPU"):   # past the check: only the missing GPU stops it
        ok.decode(torch.zeros(2, 4))
