"""What the dataflow training path of `agg` = `add` / `max` decides and computes outside its kernels: the route (`route.plain`, a
pure function once the device's two answers are given), the host mirrors of the `max` pull weights and of the edge encoder's
gradient (`variants.plain_pull_host`, `variants.plain_edge_grads_host`) against float64 torch autograd of the reference's conv
on the MIXED batch - whose ties are real -, and the ABI the path added."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from dagnn_amd import _lib, engine, route, variants
from tests import test_variants_bwd_gpu as T

GOOD = dict(backend="dataflow", training=True, agg="max", recurr=True, agg_x=False, schedule="lockstep", wea=True, R=2, H=72, L=2,
            ndirs=2, B=5, N=300, ok=True, groups=3, fits=True)


def _plain(**kw):
    a = dict(GOOD, **kw)
    return route.plain(None, a["backend"], a["training"], a["agg"], a["recurr"], a["agg_x"], a["schedule"], a["wea"], a["R"],
                       a["H"], a["L"], a["ndirs"], a["B"], a["N"], ok=a["ok"], groups=a["groups"], fits=a["fits"])


def test_the_route_takes_both_kernels_or_neither():
    r = _plain()
    assert (r.kind, r.reverse, r.why, r.Hp, r.groups) == ("dataflow", "dataflow", None, 128, 3)
    r = _plain(agg="add", H=256, wea=False, R=0)
    assert (r.kind, r.reverse, r.Hp) == ("dataflow", "dataflow", 256)
    r = _plain(training=False, backend="hip")   # an evaluation pass takes the kernel under either HIP backend
    assert (r.kind, r.reverse, r.why) == ("dataflow", None, None)


@pytest.mark.parametrize("flip", [dict(backend="hip"), dict(agg="gated_sum"), dict(ok=False), dict(recurr=False), dict(agg_x=True),
                                  dict(schedule="pergraph"), dict(R=3), dict(wea=True, R=0), dict(H=257), dict(H=344), dict(N=0),
                                  dict(N=(1 << 31) // (3 * 128) + 1), dict(groups=0), dict(fits=False)])
def test_every_condition_flips_the_route(flip):
    r = _plain(**flip)
    assert (r.kind, r.reverse, r.groups, r.stat_rows) == ("launches", "lockstep", 0, False) and r.why, r


@pytest.mark.parametrize("flag", ["DATAFLOW", "VARIANT_DATAFLOW", "BWD_DATAFLOW"])
def test_every_flag_flips_the_route(flag, monkeypatch):
    monkeypatch.setattr(engine, flag, 0)
    r = _plain()
    assert (r.kind, r.reverse) == ("launches", "lockstep") and r.why
    if flag == "BWD_DATAFLOW":   # (the evaluation pass does not need the reverse sweep)
        assert _plain(training=False).kind == "dataflow"


def test_the_hip_backend_never_trains_on_the_new_path():
    for agg in ("add", "max"):
        for H in (64, 72, 256):
            for L in (1, 2, 3):
                for wea, R in ((True, 2), (False, 0)):
                    r = _plain(backend="hip", agg=agg, H=H, L=L, wea=wea, R=R)
                    assert r.kind == "launches" and r.reverse == "lockstep" and r.why == route.PLAIN_BACKEND
    assert _plain(backend="torch").kind == "launches"


# ------------------------------------------------------------------------------------------------ the host mirrors
def _mixed_states(agg):
    """fp32 states of stacked layer 0, direction 0, of the `agg`-H64 model on the MIXED batch, with everything a conv call needs."""
    c = dict(agg=agg, H=64, E=64, L=2, batch="MIXED", kw={})
    b, model = T._batch("MIXED").clone(), T._model(c)
    b.bi_layer_index = torch.stack([b._bi_layer_idx0, b._bi_layer_index0, b._bi_layer_idx1, b._bi_layer_index1], dim=0).view(2, 2, -1)
    with torch.no_grad():
        x = model.encoder(b.x, b.node_depth.view(-1))
        h = variants.run(model, b, x)[0][0]
    return model, b, h.contiguous()


@pytest.mark.parametrize("agg", ["max", "add"])
def test_host_mirrors_match_float64_autograd_of_the_conv_on_the_mixed_batch(agg):
    """The gradient the conv hands to the states, sum_e weight_e (.) da_dst(e) at src(e), and both edge-encoder formulas,
    sum_e weight_e (.) da_dst(e) f_e[r] and sum_e weight_e (.) da_dst(e) - the mirrors in fp32 weights against torch autograd in
    float64 (`amax` splits a tie evenly, the rule the kernels have).  The MIXED batch ties: a duplicate edge and the twin roots."""
    model, b, h = _mixed_states(agg)
    conv = model.node_aggr_0[0]
    N, H = h.shape
    src, dst = b.edge_index[0], b.edge_index[1]
    ea = b.edge_attr.float().view(src.shape[0], -1)
    W, bias = conv.edge_encoder.weight.detach(), conv.edge_encoder.bias.detach()
    da = torch.from_numpy(np.random.default_rng(5).standard_normal((N, H))).double()
    # float64 autograd of the reference's conv over all edges at once (every node a frontier row)
    conv64 = type("P", (), dict(wea=True, edge_encoder=torch.nn.Linear(ea.shape[1], H).double()))()
    with torch.no_grad():
        conv64.edge_encoder.weight.copy_(W.double())
        conv64.edge_encoder.bias.copy_(bias.double())
    v64 = h.double().requires_grad_(True)
    out = variants._conv(agg, conv64, v64, None, None, src, dst, torch.arange(N), ea.double(), True)
    out.backward(da)
    # the mirrors
    if agg == "max":
        hn, wn, bn, en = h.numpy(), W.numpy(), bias.numpy(), ea.numpy()
        w = variants.plain_pull_host(hn, None, wn, bn, src, dst, en)
        tied = (w > 0) & (w < 1)
        assert tied.any() and set(np.unique(w[tied])) <= {np.float32(0.5)}, "the duplicate edge and the twin roots tie in two"
        assert np.array_equal(np.unique(w), np.array([0, 0.5, 1], dtype=np.float32))
        per_node = np.zeros((N, H))
        np.add.at(per_node, dst.numpy(), w.astype(np.float64))
        has_in = np.bincount(dst.numpy(), minlength=N) > 0
        assert np.allclose(per_node[has_in], 1.0) and not per_node[~has_in].any(), "the weights of a (node, unit) add up to one"
    else:
        w = None
    pulled = np.zeros((N, H))
    np.add.at(pulled, src.numpy(), da.numpy()[dst.numpy()] if w is None else w.astype(np.float64) * da.numpy()[dst.numpy()])
    assert np.abs(pulled - v64.grad.numpy()).max() <= 1e-6 * np.abs(v64.grad.numpy()).max()
    gw, gb = variants.plain_edge_grads_host(w, da.numpy(), dst, ea.numpy())
    for got, ref in ((gw, conv64.edge_encoder.weight.grad.numpy()), (gb, conv64.edge_encoder.bias.grad.numpy())):
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()


# ------------------------------------------------------------------------------------------------ ABI
def test_the_new_abi_is_declared_bound_and_checks_its_arguments():
    lib = _lib.load()   # (declared and bound as the header has it: tests/test_abi_cpu.py)
    # refused before any launch: a width beyond a weight row, rows beyond the plan, a bad direction, a short pitch, a missing buffer
    plan = _lib.Plan(64, 0, 4, 3, 1, 2, 0)   # (data, bytes, N, E, B, R, flags)

    def good():
        pp = _lib.PlainPull()
        pp.h = pp.a = pp.weights = pp.da_granules = pp.esum = 64
        pp.ld_h = pp.ld_a = pp.gld = 64
        return pp

    for fn in (lib.dagnn_plain_max_weights, lib.dagnn_plain_edge_grads):
        assert fn(ctypes.byref(plan), ctypes.byref(good()), 0, _lib.PULL_ROW + 1, 0, 4, None) == -22
        assert fn(ctypes.byref(plan), ctypes.byref(good()), 0, 64, 0, 5, None) == -22
        assert fn(ctypes.byref(plan), ctypes.byref(good()), 2, 64, 0, 4, None) == -22
        assert fn(ctypes.byref(_lib.Plan(0, 0, 4, 3, 1, 2, 0)), ctypes.byref(good()), 0, 64, 0, 4, None) == -22
        pp = good()
        pp.edge_mat = 64   # an edge encoder's weight without its bias
        assert fn(ctypes.byref(plan), ctypes.byref(pp), 0, 64, 0, 4, None) == -22
    for field in ("h", "a", "weights"):
        pp = good()
        setattr(pp, field, None)
        assert lib.dagnn_plain_max_weights(ctypes.byref(plan), ctypes.byref(pp), 0, 64, 0, 4, None) == -22
    for field in ("ld_h", "ld_a"):
        pp = good()
        setattr(pp, field, 63)
        assert lib.dagnn_plain_max_weights(ctypes.byref(plan), ctypes.byref(pp), 0, 64, 0, 4, None) == -22
    for field, bad in (("da_granules", None), ("esum", None), ("gld", 63)):
        pp = good()
        setattr(pp, field, bad)
        assert lib.dagnn_plain_edge_grads(ctypes.byref(plan), ctypes.byref(pp), 0, 64, 0, 4, None) == -22
    # the sweep refuses per-unit pull rows at the wide shape before any launch
    a = _lib.BwdDataflowArgs()
    a.num_stacked, a.dir_mask, a.H, a.ld_h, a.ld_g, a.gld, a.groups, a.epoch, a.pull_rows = 1, 1, 320, 320, 320, 320, 1, 1, 1
    a.schedule = a.records = a.err = 64
    assert lib.dagnn_bwd_dataflow_prepare(ctypes.byref(plan), ctypes.byref(a), None) == -22
    assert lib.dagnn_bwd_dataflow_run(ctypes.byref(plan), ctypes.byref(a), None) == -22
