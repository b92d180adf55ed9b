"""`model.attention(G)` on the GPU: the reference's fixtures, float64 at the kernel's edges, the properties that tie the exported
weights to the pass (tests/attention_f64.py holds inputs, references and bounds).

Measured on one MI355X: the fixtures' alpha within 7.2e-7 and scores within 1.9e-6; over all float64 cases the worst error is
0.52 of its bound (4 x the float32 host restatement's own error + 2e-7; a logit block of the parallel-edge case), typically
0.1-0.3.  Every case prints its figures (ATTN lines)."""
from __future__ import annotations

import copy
import ctypes as C

import pytest
import torch

from dagnn_amd import _lib, engine
from tests import attention_f64 as AF

pytestmark = pytest.mark.gpu

_MODELS = {}


def _code2(device, H, **kw):
    key = ("code2", H, tuple(sorted(kw.items())))
    if key not in _MODELS:
        _MODELS[key] = AF.on_device(lambda: AF.code2_model(H, **kw), device)
    return _MODELS[key]


def _dvae(device, kind, hs, **kw):
    key = ("dvae", kind, hs, tuple(sorted(kw.items())))
    if key not in _MODELS:
        _MODELS[key] = AF.on_device(lambda: AF.dvae_model(kind, hs, **kw), device)
    return _MODELS[key]


def _run(model, batch, device, what, logits=True):
    """One `attention` pass on a copy of `batch`, all checks that hold for every case: shapes, the float64 bound, the segment
    sums and the states that follow from the weights."""
    G = batch.clone().to(device)
    att = model.attention(G, logits=logits)
    D, L, E = len(model.dirs), model.num_layers, batch.edge_index.shape[1]
    assert tuple(att.alpha.shape) == (D, L, E) and att.alpha.is_contiguous() and att.alpha.dtype == torch.float32
    assert att.alpha.device == G.edge_index.device
    assert (att.logit is None) == (not logits)
    x = G.x.float() if AF.is_dvae(model) else G.x
    N = x.shape[0]
    Gc = copy.copy(G)
    Gc.edge_index, Gc.edge_attr = batch.edge_index, getattr(batch, "edge_attr", None)
    AF.check_against_f64(model, Gc, att, x, what)
    AF.segment_sums(att.alpha, batch.edge_index, N, model.dirs)
    AF.states_follow(model, batch.edge_index, att, x)
    return att, G


# ------------------------------------------------------------------ the reference's fixtures
@pytest.mark.parametrize("name", AF.FIXTURES)
def test_matches_the_reference_fixtures(device, name):
    meta, arr, model, batch = AF.fixture(name)
    model = model.to(device)
    att = model.attention(batch(device), logits=True)
    ref_a, ref_l = torch.from_numpy(arr["alpha"]).double(), torch.from_numpy(arr["logit"]).double()
    assert tuple(att.alpha.shape) == tuple(ref_a.shape)
    ea = float((att.alpha.cpu().double() - ref_a).abs().max())
    el = float((att.logit.cpu().double() - ref_l).abs().max())
    bound_l = 1e-4 * float(ref_l.abs().max()) + 2e-7
    print("ATTN-FIXTURE %-26s alpha err %.3e (1e-4), logit err %.3e (%.3e)" % (name, ea, el, bound_l))
    assert ea <= 1e-4
    assert el <= bound_l


# ------------------------------------------------------------------ float64 at the kernel's edges
@pytest.mark.parametrize("twin", (False, True), ids=("forwards", "reversed"))
def test_every_in_degree_class_both_directions(device, twin):
    """In-degrees 1..5, 63, 64, 65, 128, 129 (and the rest of the ladder) in both directions, the edge list forwards and back to
    front; two float edge features."""
    _run(_code2(device, 64), AF.ladder_batch(twin), device, "ladder H=64 twin=%d" % twin)


@pytest.mark.parametrize("H, L", ((32, 2), (72, 2), (256, 2), (320, 2), (64, 3)))
def test_hidden_widths_and_pitches(device, H, L):
    """32, 72 (no multiple of 16), 256, 320 (the 512-wide padded route); L = 3 once.  The kernel reads rows at the pitch of the
    pass's state buffers."""
    model = _code2(device, H, L=L)
    att, _ = _run(model, AF.ladder_batch(), device, "ladder H=%d L=%d" % (H, L))
    if H == 320:
        assert att.h[0][0].stride(0) > H   # (the padded route: a pitch that is not the width)


def test_no_edge_term_and_three_edge_types(device):
    _run(_code2(device, 64, w_edge_attr=False), AF.ladder_batch(), device, "dagnn_wea=0")
    _run(_code2(device, 64, num_rels=3), AF.typed_batch(3), device, "three edge types")


def test_parallel_edges_one_node_and_no_edges(device):
    model = _code2(device, 32)
    b = AF.parallel_batch()
    att, _ = _run(model, b, device, "parallel edges")
    seg = att.alpha[:, :, :4].cpu()   # direction 0: edges 0..3 feed node 3; 1 and 2 are parallel, with different types
    assert bool((seg[0] > 0).all()) and float((seg[0].double().sum(1) - 1).abs().max()) <= 1e-6
    assert float((seg[0, :, 1] - seg[0, :, 2]).abs().min()) > 0
    for bb, E in ((AF.edgeless_batch(), 0), (AF.one_node_batch(), 0)):
        G = bb.clone().to(device)
        a = model.attention(G, logits=True)
        assert tuple(a.alpha.shape) == tuple(a.logit.shape) == (2, 2, E) and a.alpha.device.type == "cuda"
        assert len(a.out) == 2 and a.out[0].shape[0] == bb.num_graphs


def test_scores_of_plus_minus_80_stay_finite(device):
    """The key weights scaled until the largest |score| is about 80: exp() of the raw score would overflow fp32 near 88; the
    result has no inf / NaN and keeps the float64 bound."""
    model = _code2(device, 64, seed=77)   # (a model of its own: its attention weights are rescaled below)
    b = AF.ladder_batch()
    measure = lambda: float(model.attention(b.clone().to(device), logits=True).logit.abs().max())  # noqa: E731
    peak = measure()
    for _ in range(5):   # (the states move with the weights: rescale until the peak sits at 80)
        if abs(peak - 80.0) <= 4.0:
            break
        with torch.no_grad():
            for d in model.dirs:
                for a in getattr(model, "node_aggr_%d" % d):
                    a.attn_lin.weight.mul_(80.0 / peak)
                    a.attn_lin.bias.mul_(80.0 / peak)
        peak = measure()
    assert 72.0 <= peak <= 88.0, peak
    AF.sync_cpu(model)
    att, _ = _run(model, b, device, "scores +-80")
    assert 72.0 <= float(att.logit.abs().max()) <= 88.0
    assert bool(torch.isfinite(att.alpha).all()) and bool(torch.isfinite(att.logit).all())


@pytest.mark.parametrize("agg", ("attn_x", "self_attn_h", "self_attn_x", "mattn_h"))
def test_every_attention_aggregator(device, agg):
    _run(_code2(device, 64, agg=agg), AF.ladder_batch(), device, "agg=%s" % agg)


def test_linear_cells_and_one_direction(device):
    _run(_code2(device, 64, recurr=0), AF.ladder_batch(), device, "recurr=0")
    _run(_code2(device, 64, bidirectional=False), AF.ladder_batch(), device, "unidirectional")


@pytest.mark.parametrize("kind, hs, agg, bidir", (("na", 501, "attn_h", False), ("na", 64, "self_attn_h", True),
                                                  ("bn", 64, "attn_h", True), ("bn", 64, "attn_x", True),
                                                  ("bn", 32, "self_attn_x", True)))
def test_dvae_encoders(device, kind, hs, agg, bidir):
    """`DAGNN_NA` (the one-hot vertex-id columns in keys and queries; hs = 501: row pitch 504) and `DAGNN_BN`, the self-attention
    encoders included; in-degrees 0..13."""
    model = _dvae(device, kind, hs, agg=agg, bidirectional=bidir)
    b = AF.dvae_batch()
    att, G = _run(model, b, device, "%s hs=%d %s" % (kind, hs, agg))
    with torch.no_grad():
        out = model(b.clone().to(device))   # (the fused call where it applies: the same bits as the step-by-step route)
    assert torch.equal(att.out, out)


# ------------------------------------------------------------------ properties
def test_same_bits_and_permutation_invariance(device):
    model = _code2(device, 64)
    b = AF.ladder_batch()
    att, G = _run(model, b, device, "bits")
    h0, x0 = [[t.detach().cpu().clone() for t in hd] for hd in att.h], G.x.detach().cpu().clone()   # (this pass's states, kept)
    with torch.no_grad():
        out = model(b.clone().to(device))
    assert len(out) == len(att.out) and all(torch.equal(o, p) for o, p in zip(out, att.out))
    again = model.attention(b.clone().to(device), logits=True)
    assert torch.equal(att.alpha, again.alpha) and torch.equal(att.logit, again.logit)
    bp, perm = AF.permuted_batch()
    assert torch.equal(bp.edge_index, b.edge_index[:, perm])
    attp, _ = _run(model, bp, device, "permuted")
    undone = torch.empty_like(attp.alpha)
    undone[:, :, perm.to(device)] = attp.alpha          # alpha of the original edge ids
    Gc = AF._cpu_graph(_with_edges(G, b))
    a64, _ = AF.attention_host(AF.model_cpu(model), Gc, h0, x0, AF.F64)
    a32, _ = AF.attention_host(AF.model_cpu(model), Gc, h0, x0, torch.float32)
    for q in range(2):
        for l in range(2):
            bound = AF.FACTOR * float((a32[q, l].double() - a64[q, l]).abs().max()) + AF.FLOOR   # (the float64 bound of the block)
            diff = float((undone[q, l] - att.alpha[q, l]).abs().max())
            print("ATTN permuted vs original         alpha block (%d, %d): diff %.3e, bound %.3e (%.2f)" % (q, l, diff, bound, diff / bound))
            assert diff <= bound


def test_more_cells_than_one_call_takes(device, monkeypatch):
    """More (direction, stacked layer) cells than one call of the entry point takes go in chunks: the same bits."""
    model = _code2(device, 64)
    b = AF.ladder_batch()
    whole = model.attention(b.clone().to(device), logits=True)
    monkeypatch.setattr(_lib, "ATTN_MAX_CELLS", 3)    # (4 cells: 3 + 1)
    parts = model.attention(b.clone().to(device), logits=True)
    assert torch.equal(whole.alpha, parts.alpha) and torch.equal(whole.logit, parts.logit)


def _with_edges(G, b):
    Gc = copy.copy(G)
    Gc.edge_index, Gc.edge_attr = b.edge_index, b.edge_attr
    return Gc


def test_adds_no_synchronisation(device):
    """Where `predict(G)` runs clean under the sync debug mode, `attention(G)` does: the default bidirectional configuration."""
    meta, arr, model, batch = AF.fixture("attention_code2_h32")
    model = model.to(device)
    model.predict(batch(device))
    model.attention(batch(device), logits=True)   # (warm-up: derived weights, allocator)
    G1, G2, G3 = batch(device), batch(device), batch(device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        model.predict(G1)
        a = model.attention(G2)
        b = model.attention(G3, logits=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(a.alpha, b.alpha)
    model.check()


# ------------------------------------------------------------------ arguments
def test_argument_handling(device):
    model = _code2(device, 32)
    b = AF.parallel_batch()
    model.train()
    try:
        with pytest.raises(RuntimeError, match="evaluation pass"):
            model.attention(b.clone().to(device))
    finally:
        model.eval()
    with pytest.raises(NotImplementedError, match="agg_x"):
        AF.code2_model(32, agg_x=True).to(device).attention(b.clone().to(device))
    with pytest.raises(ValueError, match="gated_sum"):
        AF.code2_model(32, agg="gated_sum").to(device).attention(b.clone().to(device))
    # the entry point itself: a null output with E > 0
    G = b.clone().to(device)
    att = model.attention(G)
    plan = engine.build_plan(b.edge_index.to(device), b._bi_layer_idx0.to(device), b._bi_layer_idx1.to(device), b.batch.to(device),
                             b.num_graphs, b.edge_attr.to(device))
    a = _lib.AttnArgs()
    a.num_cells = 1
    c = a.cell[0]
    w = torch.zeros(32, device=device)
    ks = torch.zeros(G.x.shape[0], device=device)
    c.key, c.ld_key, c.key_dim, c.w_key, c.dir = att.h[0][0].data_ptr(), att.h[0][0].stride(0), 32, w.data_ptr(), 0
    a.key_score = ks.data_ptr()
    assert _lib.load().dagnn_attention_weights(C.byref(plan.desc), C.byref(a), engine._stream(w)) == -22
    torch.cuda.synchronize()
