"""Host side of the gated_sum D-VAE decoder (`agg = 1` of csrc/dvae_decode.hip and csrc/dvae_sample.hip): the appended
C struct fields, the argument checks of the entry points, the errors `loss()` / `decode()` raise, and the coverage of the
`dvae_gated_*` fixtures - none of it needs a GPU."""
from __future__ import annotations

import ctypes as C

import pytest
import torch

from dagnn_amd import DAGNN_NA, _lib, dvae
from tests import helpers as Hh

LOSS = ["dvae_gated_loss_na_h64_L2", "dvae_gated_loss_na_h501_L2", "dvae_gated_loss_na_h64_encode"]
DECODE = ["dvae_gated_decode_na_h64_L2_argmax", "dvae_gated_decode_na_h64_L2_sample", "dvae_gated_decode_na_h501_L2_sample"]
FAKE = 1 << 20   # a non-null pointer for the size queries (never dereferenced: nothing here launches)
GATED = ("agg", "gate_w", "gate_b", "mapper_w")


@pytest.mark.parametrize("cls", [_lib.DvaeDecodeArgs, _lib.DvaeSampleArgs])
def test_gated_fields_are_appended(cls):
    """The gated fields follow the last attn_h field with no padding in front, so a caller's attn_h struct is a prefix, and a
    zero-filled struct means agg = 0 (attn_h).  (Every offset against the header: tests/test_abi_cpu.py.)"""
    names = [f[0] for f in cls._fields_]
    assert tuple(names[-4:]) == GATED
    old = type("Old", (C.Structure,), {"_fields_": cls._fields_[:-4]})
    assert cls.agg.offset == C.sizeof(old)
    assert cls().agg == 0


def test_gated_gradient_fields_are_appended():
    names = [f[0] for f in _lib.DvaeDecodeGrads._fields_]
    assert tuple(names[-3:]) == ("d_gate_w", "d_gate_b", "d_mapper_w")
    old = type("Old", (C.Structure,), {"_fields_": _lib.DvaeDecodeGrads._fields_[:-3]})
    assert _lib.DvaeDecodeGrads.d_gate_w.offset == C.sizeof(old)


def _decode_args(**kw):
    a = _lib.DvaeDecodeArgs()
    a.B, a.n, a.hs, a.L, a.nvt, a.start_type, a.bn, a.edge_hidden, a.vertex_hidden = 4, 8, 16, 2, 8, 0, 0, 64, 32
    a.agg, a.gate_w, a.gate_b, a.mapper_w = 1, FAKE, FAKE, FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _sample_args(**kw):
    a = _lib.DvaeSampleArgs()
    a.G, a.B, a.n, a.hs, a.L, a.nvt, a.start_type, a.end_type = 2, 4, 8, 16, 2, 8, 0, 1
    a.bn, a.stochastic, a.edge_hidden, a.vertex_hidden = 0, 1, 64, 32
    a.agg, a.gate_w, a.gate_b, a.mapper_w = 1, FAKE, FAKE, FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD = [dict(agg=2), dict(agg=-1), dict(bn=1), dict(gate_w=None), dict(gate_b=None), dict(mapper_w=None)]


def test_gated_decode_entry_points_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    gated = _decode_args()
    attn = _decode_args(agg=0, gate_w=None, gate_b=None, mapper_w=None)
    # the size queries account for the message buffers (saved) and their gradients (work)
    assert lib.dagnn_dvae_decode_saved_bytes(C.byref(gated)) > lib.dagnn_dvae_decode_saved_bytes(C.byref(attn)) > 0
    assert lib.dagnn_dvae_decode_work_bytes(C.byref(gated)) > lib.dagnn_dvae_decode_work_bytes(C.byref(attn)) > 0
    for kw in BAD:
        a = _decode_args(**kw)
        assert lib.dagnn_dvae_decode_saved_bytes(C.byref(a)) == 0, kw
        assert lib.dagnn_dvae_decode_work_bytes(C.byref(a)) == 0, kw
        assert lib.dagnn_dvae_decode_forward(C.byref(a), None) == -22, kw
        assert lib.dagnn_dvae_decode_backward(C.byref(a), C.byref(_lib.DvaeDecodeGrads()), None) == -22, kw


def test_gated_sample_entry_point_checks_its_arguments_without_a_gpu():
    lib = _lib.load()
    gated = _sample_args()
    attn = _sample_args(agg=0, gate_w=None, gate_b=None, mapper_w=None)
    assert lib.dagnn_dvae_sample_work_bytes(C.byref(gated)) > lib.dagnn_dvae_sample_work_bytes(C.byref(attn)) > 0
    for kw in BAD:
        a = _sample_args(**kw)
        assert lib.dagnn_dvae_sample_work_bytes(C.byref(a)) == 0, kw
        assert lib.dagnn_dvae_sample(C.byref(a), None) == -22, kw


@pytest.mark.parametrize("name", LOSS)
def test_gated_schedule_gives_the_reference_padding_width_of_every_update(name):
    meta, arr = Hh.load(name)
    assert meta["agg"] == "gated_sum"
    graphs = Hh.dvae_graphs(meta, arr)
    types, preds = dvae.decode_schedule(graphs, 8, 8)
    assert dvae.update_widths(preds, 8) == [int(x) for x in arr["widths"]]


@pytest.mark.parametrize("name", DECODE)
def test_gated_decode_fixtures_cover_the_decoder(name):
    meta, arr = Hh.load(name)
    assert meta["agg"] == "gated_sum" and meta["margin"] >= 1e-4
    cov = meta["coverage"]
    assert cov["early_end"] > 0 and cov["forced_end"] > 0 and cov["end_joins_two"] > 0 and cov["coupled_updates"] > 0


def _gated(**kw):
    args = dict(hs=16, nz=8, num_nodes=8, num_layers=2, bidirectional=False, agg="gated_sum")
    args.update(kw)
    hidden = args.pop("hidden_dim", args["hs"])
    return DAGNN_NA(8, hidden, hidden, 8, 8, 0, 1, **args)


def _inputs(B=3):
    from dagnn_amd import synth
    graphs = [synth.decode_enas_row(r) for r in synth.enas_rows(2, B)]
    return graphs, torch.zeros(B, 8), torch.zeros(B, 8)


def test_gated_decoder_needs_num_nodes_equal_to_max_n():
    model = _gated(num_nodes=9)
    graphs, mu, lv = _inputs()
    with pytest.raises(ValueError, match="num_nodes == max_n"):
        model.loss(mu, lv, graphs)
    with pytest.raises(ValueError, match="num_nodes == max_n"):
        model.decode(mu)


def test_gated_decoder_needs_hidden_dim_equal_to_hs():
    model = _gated(hidden_dim=24)
    graphs, mu, lv = _inputs()
    with pytest.raises(ValueError, match="hidden_dim == hs"):
        model.loss(mu, lv, graphs)


def test_gated_decoder_raises_for_a_model_off_the_gpu():
    model = _gated()
    graphs, mu, lv = _inputs()
    with pytest.raises(_lib.DagnnHipError, match="GPU"):
        model.loss(mu, lv, graphs)
    with pytest.raises(_lib.DagnnHipError, match="GPU"):
        model.decode(mu)


@pytest.mark.parametrize("agg", ["add", "max"])
def test_other_aggregators_still_raise(agg):
    model = _gated(agg=agg)
    graphs, mu, lv = _inputs()
    with pytest.raises(NotImplementedError, match="attn_h"):
        model.loss(mu, lv, graphs)
    with pytest.raises(NotImplementedError, match="attn_h"):
        model.decode(mu)
