"""`attention_host` - the written-down definition of `model.attention(G)` - against the reference's recorded attention weights,
and the argument handling that needs no GPU (tests/attention_f64.py holds inputs and bounds)."""
from __future__ import annotations

import ctypes as C

import pytest
import torch

import dagnn_amd
from dagnn_amd import _lib, attention_host, evaluate
from tests import attention_f64 as AF


@pytest.mark.parametrize("name", AF.FIXTURES)
def test_host_definition_matches_the_reference_fixtures(name):
    """`attention_host` in float64, on the float64 oracle's states, against what the reference's conv modules computed: alpha
    and the pre-softmax score of every edge, within the parity bound 1e-4."""
    meta, arr, model, batch = AF.fixture(name)
    G = batch()
    x, h = AF.oracle_states(model, G, AF.F64)
    alpha, logit = attention_host(model, G, h, x, AF.F64)
    D, L, E = len(model.dirs), model.num_layers, G.edge_index.shape[1]
    assert tuple(alpha.shape) == tuple(logit.shape) == (D, L, E) == tuple(arr["alpha"].shape)
    ea = float((alpha - torch.from_numpy(arr["alpha"]).double()).abs().max())
    el = float((logit - torch.from_numpy(arr["logit"]).double()).abs().max())
    print("ATTN-HOST %-26s alpha err %.3e, logit err %.3e (max |logit| %.3e)" % (name, ea, el, float(abs(arr["logit"]).max())))
    assert ea <= AF.PARITY
    assert el <= AF.PARITY
    # float32 restatement: the same numbers within the same bound
    a32, l32 = attention_host(model, G, [[t.float() for t in hd] if hd is not None else None for hd in h], x.float(), torch.float32)
    assert a32.dtype == torch.float32 and float((a32.double() - alpha).abs().max()) <= AF.PARITY


def test_host_definition_is_a_segment_softmax():
    """Every in-edge segment sums to 1, an in-degree of 1 gives exactly 1, parallel edges each get a weight; `logits=False`
    returns None; no edges gives [D, L, 0]."""
    model = AF.code2_model(32)
    G = AF.parallel_batch()
    x, h = AF.oracle_states(model, G, torch.float32)
    alpha, logit = attention_host(model, G, h, x, torch.float32)
    AF.segment_sums(alpha, G.edge_index, x.shape[0], model.dirs)
    seg = alpha[0, :, :4]   # edges 0..3 feed node 3 in direction 0; edges 1 and 2 are parallel with different types
    assert bool((seg > 0).all()) and float((seg.double().sum(1) - 1).abs().max()) <= 1e-6
    assert float((alpha[0, :, 1] - alpha[0, :, 2]).abs().min()) > 0   # (different types: different weights)
    assert attention_host(model, G, h, x, torch.float32, logits=False)[1] is None
    G0 = AF.edgeless_batch()
    x0, h0 = AF.oracle_states(model, G0, torch.float32)
    a0, l0 = attention_host(model, G0, h0, x0, torch.float32)
    assert tuple(a0.shape) == tuple(l0.shape) == (2, 2, 0)


def test_argument_handling():
    model = AF.code2_model(32)
    model.train()
    with pytest.raises(RuntimeError, match="evaluation pass"):
        model.attention(AF.parallel_batch())
    na = AF.dvae_model("na", 32)
    na.train()
    with pytest.raises(RuntimeError, match="evaluation pass"):
        na.attention(AF.dvae_batch(1))
    with pytest.raises(NotImplementedError, match="agg_x"):
        AF.code2_model(32, agg_x=True).attention(AF.parallel_batch())
    for agg in ("add", "max", "gated_sum"):
        with pytest.raises(ValueError, match=agg):
            AF.code2_model(32, agg=agg).attention(AF.parallel_batch())
    with pytest.raises(ValueError, match="gated_sum"):
        AF.dvae_model("na", 32, agg="gated_sum").attention(AF.dvae_batch(1))
    assert evaluate.Attention is dagnn_amd.Attention and evaluate.attention_host is attention_host
    assert dagnn_amd.Attention._fields[:3] == ("out", "alpha", "logit")


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """`dagnn_attention_weights` validates on the host: a null output with E > 0, no cells, too many cells, a pitch below the
    key width, a direction outside {0, 1} - DAGNN_EINVAL each, with no HIP call made (this tier has no GPU)."""
    lib = _lib.load()
    plan = _lib.Plan(1, 1 << 20, 8, 5, 1, 0, 0)   # (a non-null workspace address that is never dereferenced)
    a = _lib.AttnArgs()
    a.num_cells = 1
    c = a.cell[0]
    c.key, c.w_key, c.ld_key, c.key_dim, c.dir = 16, 16, 32, 32, 0
    a.key_score = 16
    assert lib.dagnn_attention_weights(C.byref(plan), C.byref(a), None) == -22          # alpha is NULL, E = 5
    a.alpha = 16
    for field, bad in (("num_cells", 0), ("num_cells", _lib.ATTN_MAX_CELLS + 1), ("mode", 2)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert lib.dagnn_attention_weights(C.byref(plan), C.byref(a), None) == -22, field
        setattr(a, field, keep)
    for field, bad in (("ld_key", 31), ("key_dim", 0), ("dir", 2), ("key", None), ("w_key", None)):
        keep = getattr(c, field)
        setattr(c, field, bad)
        assert lib.dagnn_attention_weights(C.byref(plan), C.byref(a), None) == -22, field
        setattr(c, field, keep)
    a.key_score = None
    assert lib.dagnn_attention_weights(C.byref(plan), C.byref(a), None) == -22          # no scratch for the key scores
    a.key_score = 16
    big = _lib.Plan(1, 1 << 20, 1 << 31, 5, 1, 0, 0)
    assert lib.dagnn_attention_weights(C.byref(big), C.byref(a), None) == -22           # N out of range
    empty = _lib.Plan(1, 1 << 20, 8, 0, 1, 0, 0)
    a.alpha = None
    assert lib.dagnn_attention_weights(C.byref(empty), C.byref(a), None) == 0           # E == 0: nothing to do, no launch
