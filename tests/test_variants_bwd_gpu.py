"""The reverse sweep of the constructor-string variants (csrc/variants_bwd.hip: `dagnn_variant_backward_run`,
`dagnn_variant_aggregator_backward`, the prepare kernels) against the float64 oracle at the widths where its code takes another
path than at H = 64: lane loops of several trips and ragged tails (72), the last narrow / first wide additive-attention width
(256 / 260), a second K chunk and a second column block of the rows map (344, 516), 8 cells in a step (L = 4), a grid-stride
wrap of the GRU kernel (2100 rows x 256), `emb_dim != hidden_dim`, no edge features, `agg_x` with a zero-padded aggregate -
and `max` with real ties (a duplicate edge, twin roots), whose gradient the tied messages share evenly.

One training step of a plain `DAGNN` per case, four results: the float64 oracle on the CPU (`Hh.code2_grads64`), the
reference's loop nest on fp32 torch ops on the device (`variant_backend = "torch"`: a second reference, not code under test),
the same torch ops on the CPU (a second summation order; a tensor's baseline error is the larger of the two - several
gradients here are sums with heavy cancellation, where one fp32 order can be ten times luckier than another), the HIP step, and
the HIP step again (bitwise equal except the embedding tables, whose scatter is atomic by default).

Bound (the convention of tests/test_dvae_gated_train_gpu.py): per tensor, with e = largest absolute error
against float64 and scale = max |ref|:  e_hip <= 4 x max(e_torch, 2^-23 scale), e_torch over both torch baselines - one fp32 ulp of the largest entry is the floor
no fp32 result can be held below; entries that are exactly zero in the oracle: |hip| <= 1e-6; tensors with scale <= 2e-5 (the
query half of `attn_lin`, attention biases: rounding noise) e_hip <= 2e-7 = 100 x the `atol` of `Hh.check_grads_full`; the loss
within 1e-5.  Nothing is derived from the HIP result.  `MEASURED`: what `_report` printed on one MI355X.

The GPU tests carry the `gpu` mark one by one: the tests at the bottom run on the CPU and show that the tie cases can
fail - the ties are real and carry gradient, and the two conserving tie conventions (even split / first winner) give the same
parameter gradients on this batch, so the comparison holds whichever of them a kernel takes."""
from __future__ import annotations

import functools
import warnings

import numpy as np
import pytest
import torch

from dagnn_amd import DAGNN, ASTNodeEncoder, GraphData, engine, synth, variants
from dagnn_amd.dag_utils import add_order_info_01
from oracle import dagnn_oracle as O
from oracle.seeding import seeded_fill
from tests import helpers as Hh

FACTOR = 4.0          # x the fp32 torch path's own error (tests/test_dvae_gated_train_gpu.py: 2.9 observed there)
ULP = 2.0 ** -23      # x scale: one fp32 ulp of the tensor's largest entry
ZERO_FLOOR = 1e-6     # absolute, for entries that are exactly zero in the oracle
TINY_SCALE, TINY_ABS = 2e-5, 2e-7   # gradients that are rounding noise: 100 x the atol of Hh.check_grads_full
V, S = 11, 2

# width: (worst relative error of a tensor larger than 2e-5 over the cases of that width - torch baselines, HIP -; the largest ratio of a
# single tensor's HIP error to max(e_torch, ulp), bound 4, and that tensor) - recorded from `_report` on one MI355X, not asserted
MEASURED = {
    64: (4.4e-05, 2.9e-06, 2.55, "node_aggr_0.3.attn_linl.bias of mattn_h-H64-L4"),         # 2 cases
    70: (1.5e-06, 1.1e-06, 1.56, "node_aggr_1.0.gate.0.weight of gated_sum-E32-H70"),       # 1 case
    72: (3.4e-05, 4.7e-05, 3.25, "cells_0.1.bias of mattn_h-recurr0-H72"),                  # 16 cases
    128: (2.9e-06, 2.5e-06, 1.58, "graph_pred_linear_list.1.bias of aggx-gated_sum-E64-H128"),   # 1 case
    256: (3.8e-05, 1.5e-05, 2.92, "node_aggr_0.0.edge_encoder.weight of attn_x-recurr0-H256"),   # 5 cases
    260: (4.4e-06, 9.8e-06, 3.17, "cells_1.0.weight of attn_x-recurr0-E64-H260"),           # 6 cases
    344: (1.8e-04, 5.5e-05, 2.13, "encoder.attribute_encoder.weight of max-H344"),          # 3 cases
    516: (2.7e-06, 2.7e-06, 1.91, "graph_pred_linear_list.1.bias of gated_sum-H516"),       # 1 case
}
# The five `max` cases on the kernel before the tie rule (every tied message kept the whole gradient): errors of 31-84 % of a tensor's
# largest entry - H = 64: cells_0.0.weight_ih 1.3e-2 of 2.4e-2, node_aggr_0.0.edge_encoder.bias 5.0e-3 of 1.5e-2, the embedding
# tables 8.0e-4 / 8.0e-4 / 1.1e-3 of 2.7e-3 / 2.8e-3 / 4.2e-3 (torch path: 7e-10..8e-9); now 1.2-2.1 x the torch path's error.


def _case_of(cid, agg, H, E=None, L=2, batch="MIXED", **kw):
    return cid, dict(agg=agg, H=H, E=H if E is None else E, L=L, batch=batch, kw=kw)


CASES = dict([
    _case_of("mattn_h-H72", "mattn_h", 72), _case_of("mattn_h-H256", "mattn_h", 256),
    _case_of("mattn_h-H344", "mattn_h", 344),                       # 3H = 1032: a second K chunk; J = 344: two column blocks
    _case_of("mattn_h-H64-L4", "mattn_h", 64, L=4),                 # 8 cells in one step
    _case_of("mattn_h-E32-H72", "mattn_h", 72, E=32),
    _case_of("gated_sum-H72", "gated_sum", 72), _case_of("gated_sum-H260", "gated_sum", 260),
    _case_of("gated_sum-H516", "gated_sum", 516),                   # 2H = 1032: the gate / mapper switch inside chunk 0
    _case_of("gated_sum-H72-nomapperbias", "gated_sum", 72, mapper_bias=False),
    _case_of("gated_sum-H72-noedgeattr", "gated_sum", 72, w_edge_attr=False),
    _case_of("gated_sum-H256-widelayer", "gated_sum", 256, batch="WIDE_LAYER"),   # vb_gru_kernel wraps its grid
    _case_of("gated_sum-E32-H70", "gated_sum", 70, E=32),           # row pitch 72 != H, with the R = 2 edge sums
    _case_of("add-H72", "add", 72), _case_of("add-H344", "add", 344),
    _case_of("add-H72-unidir-poolall", "add", 72, bidirectional=False, out_pool_all=True),
    _case_of("max-H64", "max", 64), _case_of("max-H72", "max", 72), _case_of("max-H344", "max", 344),
    _case_of("max-H72-noedgeattr", "max", 72, w_edge_attr=False),
    _case_of("attn_h-recurr0-H256", "attn_h", 256, recurr=0), _case_of("attn_h-recurr0-H260", "attn_h", 260, recurr=0),
    _case_of("attn_x-recurr0-H256", "attn_x", 256, recurr=0), _case_of("attn_x-recurr0-H260", "attn_x", 260, recurr=0),
    _case_of("self_attn_h-recurr0-H256", "self_attn_h", 256, recurr=0),
    _case_of("self_attn_h-recurr0-H260", "self_attn_h", 260, recurr=0),
    _case_of("attn_x-recurr0-E64-H260", "attn_x", 260, E=64, recurr=0),           # key width != H
    _case_of("mattn_h-recurr0-H72", "mattn_h", 72, recurr=0), _case_of("gated_sum-recurr0-H72", "gated_sum", 72, recurr=0),
    _case_of("aggx-attn_h-H72", "attn_h", 72, agg_x=True), _case_of("aggx-add-H72", "add", 72, agg_x=True),
    _case_of("aggx-gated_sum-H72", "gated_sum", 72, agg_x=True), _case_of("aggx-mattn_h-H72", "mattn_h", 72, agg_x=True),
    _case_of("aggx-max-H72", "max", 72, agg_x=True), _case_of("aggx-attn_h-H260", "attn_h", 260, agg_x=True),
    _case_of("aggx-gated_sum-E64-H128", "gated_sum", 128, E=64, agg_x=True),      # zero-padded aggregate
])


# ------------------------------------------------------------------------------------------------ batches and models
def _graph(x, depth, edges, attr=None):
    ei = torch.tensor(edges, dtype=torch.long).t().reshape(2, -1)
    ea = torch.zeros(ei.shape[1], 2) if attr is None else torch.tensor(attr, dtype=torch.float32)
    d = GraphData(x=torch.tensor(x, dtype=torch.long), node_depth=torch.tensor(depth, dtype=torch.long).view(-1, 1),
                  edge_index=ei, edge_attr=ea)
    add_order_info_01(d)
    return d


def _twin_roots():
    """Two roots with identical features feed one node through edges of equal attributes: their messages tie in every column."""
    return _graph([[7, 41], [7, 41], [3, 9]], [0, 0, 1], [(0, 2), (1, 2)])


@functools.lru_cache(maxsize=None)
def _batch(name):
    if name == "MIXED":   # ~570 nodes: the degenerate graphs (duplicate edge = graph 5), six code2-like graphs, the twin roots LAST
        b = Hh._degenerate_batch(extra=synth.code2_graphs(5, 6, 20) + [_twin_roots()])
    else:   # WIDE_LAYER: 2100 single-node graphs in front: layer 0 holds more than 524288 / 256 rows
        single = [_graph([[i % 98, i % 300]], [i % 30], []) for i in range(2100)]
        b = synth.GraphBatch.from_data_list(single + [_twin_roots(), _graph([[1, 2], [3, 4], [5, 6]], [0, 1, 2], [(0, 1), (1, 2)])])
    b.x[:, 1] %= 300
    return b


def _num_graphs(b):
    return int(b.batch.max()) + 1


def _labels(b):
    return torch.from_numpy(np.random.default_rng(2).integers(0, V, size=(_num_graphs(b), S)))


def _ctor(c):
    kw = dict(w_edge_attr=True, num_layers=c["L"], bidirectional=True, agg=c["agg"], out_wx=False, out_pool_all=False,
              out_pool="max", dropout=0.0)
    kw.update(c["kw"])
    return kw


def _model(c):
    E, H = c["E"], c["H"]
    model = DAGNN(num_vocab=V, max_seq_len=S, emb_dim=E, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(E, 98, 300, 20),
                  **_ctor(c))
    seeded_fill(model, 13)
    return model


def _oracle_kw(c):
    kw = _ctor(c)
    return dict(num_layers=kw["num_layers"], bidirectional=kw["bidirectional"], out_wx=False, out_pool_all=kw["out_pool_all"],
                out_pool="max", max_seq_len=S, agg=kw["agg"], agg_x=kw.get("agg_x", False), recurr=kw.get("recurr", 1))


# ------------------------------------------------------------------------------------------------ the four results
def _refuse(*a, **k):
    raise AssertionError("the torch-ops recurrence ran in a HIP step")


class _Spy(object):
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


def _cpu64(loss, grads):
    return float(loss), {k: v.detach().double().cpu() for k, v in grads.items()}


def _torch_step_cpu(model, G, y):
    """The second fp32 baseline: the same torch-ops path (`variants.run` + the torch read-out, what `DAGNN._pass` runs with
    `variant_backend = "torch"`) on the CPU - another summation order of the same loop nest."""
    from dagnn_amd.core import num_graphs_of

    def forward(G):
        G.bi_layer_index = torch.stack([G._bi_layer_idx0, G._bi_layer_index0, G._bi_layer_idx1, G._bi_layer_index1], dim=0).view(2, 2, -1)
        G.x = model.encoder(G.x, G.node_depth.view(-1))
        return model._finish(G, None, G.x, variants.run(model, G, G.x), num_graphs_of(G), None)

    model.forward = forward   # (an instance attribute in front of the method, for this step only)
    try:
        return _cpu64(*Hh._train_step(model, G, y))
    finally:
        del model.forward
        model.zero_grad(set_to_none=True)


@functools.lru_cache(maxsize=None)
def _case(cid):
    """Per tensor (name, scale, e_torch = the larger error of the two fp32 torch baselines (device, CPU), e_hip over the non-zero entries of the oracle, largest |hip| where the oracle is
    exactly zero), the three losses and the names whose two HIP gradients differ in a bit - computed once per case."""
    c = CASES[cid]
    dev = torch.device("cuda:0")
    b, model = _batch(c["batch"]), _model(c)
    y = _labels(b)
    loss_r, g_r = Hh.code2_grads64(None, model, b, y, **_oracle_kw(c))
    _, g_c = _torch_step_cpu(model, b.clone(), y)
    model = model.to(dev)
    model.variant_backend = "torch"
    loss_t, g_t = _cpu64(*Hh._train_step(model, b.clone().to(dev), y.to(dev)))
    model.variant_backend = "hip"
    lib = engine._lib.load()
    spied = ["dagnn_variant_backward_run"] + (["dagnn_variant_aggregator_backward"] if c["kw"].get("agg_x") else [])
    spies = {n: _Spy(getattr(lib, n)) for n in spied}
    seen, run = variants._TORCH_PATH_SEEN, variants.run
    try:
        for n, s in spies.items():
            setattr(lib, n, s)
        variants._TORCH_PATH_SEEN = set()   # `warn_torch_path` speaks once per shape: no earlier test has used this one up
        variants.run = _refuse
        with warnings.catch_warnings():
            warnings.filterwarnings("error", category=RuntimeWarning, message=".*torch ops.*")
            loss_h, g_h = _cpu64(*Hh._train_step(model, b.clone().to(dev), y.to(dev)))
            loss_h2, g_h2 = _cpu64(*Hh._train_step(model, b.clone().to(dev), y.to(dev)))
        torch.cuda.synchronize()
        model.check()
    finally:
        for n, s in spies.items():
            setattr(lib, n, s.fn)
        variants._TORCH_PATH_SEEN, variants.run = seen, run
    for n, s in spies.items():
        assert s.calls >= 2, "%s: %s ran %d times in two training steps" % (cid, n, s.calls)
    assert set(g_h) == set(g_t) and set(g_h) <= set(g_r), set(g_h) ^ set(g_r)
    rows = []
    for k in g_h:
        ref, got, par = g_r[k].double(), g_h[k], g_t[k]
        assert got.shape == ref.shape == par.shape, (k, got.shape, ref.shape)
        zero = ref == 0
        rows.append((k, float(ref.abs().max()), max(float((par - ref).abs().max()), float((g_c[k] - ref).abs().max())),
                     float((got - ref)[~zero].abs().max()) if (~zero).any() else 0.0,
                     float(got[zero].abs().max()) if zero.any() else 0.0))
    differ = [k for k in g_h if not k.startswith("encoder.") and not torch.equal(g_h[k], g_h2[k])]
    if loss_h != loss_h2:
        differ.append("loss")
    return rows, (float(loss_r), loss_t, loss_h), differ


def _base(row):
    return max(row[2], ULP * row[1])


def _report(cid, rows):
    big = [r for r in rows if r[1] > TINY_SCALE]
    worst = max(big, key=lambda r: r[3] / _base(r))
    print("\n%s: worst relative error torch %.3e / hip %.3e; closest to the bound: %s torch %.3e hip %.3e (scale %.3e), ratio %.2f of %.1f"
          % (cid, max(r[2] / r[1] for r in big), max(r[3] / r[1] for r in big), worst[0], worst[2], worst[3], worst[1],
             worst[3] / _base(worst), FACTOR))
    for r in rows:
        print("    %-46s scale %.3e  torch %.3e  hip %.3e  at zeros %.1e" % r)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_training_step_gradients_match_the_float64_oracle(device, cid):
    """Loss and the gradient of every named parameter, HIP sweep against float64 within 4 x the fp32 torch path's own error
    (module docstring); the sweep's entry points ran and nothing fell back to torch ops (`_case` asserts both).

    What the cases found besides the `max` ties: the soft-max Jacobian of the attention aggregators was
    formed against the STORED aggregate (aggx-attn_h-H260: `attn_lin.weight` at 27 x the torch error, six cases over the bound),
    and the logits of the sweep's prepare kernels were float chains (mattn_h-H72 `node_aggr_1.0.attn_linr.weight` 4.4 x,
    aggx-attn_h-H260 `node_aggr_0.0.attn_lin.weight` 12.6 x with the Jacobian alone mended).  Both are formed in double now; those
    two tensors stand at 2.3 x and 2.25 x."""
    rows, (loss_r, loss_t, loss_h), _ = _case(cid)
    _report(cid, rows)
    failures = []
    if abs(loss_h - loss_r) > 1e-5:
        failures.append("loss %.8f, oracle %.8f" % (loss_h, loss_r))
    for name, scale, e_t, e_h, at_zero in rows:
        if scale <= TINY_SCALE:
            if max(e_h, at_zero) > TINY_ABS:
                failures.append("%s: %.3e at scale %.3e (rounding noise: at most %.0e)" % (name, max(e_h, at_zero), scale, TINY_ABS))
            continue
        if at_zero > ZERO_FLOOR:
            failures.append("%s: %.3e where the oracle is exactly zero" % (name, at_zero))
        bound = FACTOR * max(e_t, ULP * scale)
        if e_h > bound:
            failures.append("%s: hip %.3e > %.3e = %.0f x max(torch %.3e, ulp %.3e)" % (name, e_h, bound, FACTOR, e_t, ULP * scale))
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_two_training_steps_are_bitwise_equal(device, cid):
    """Every gradient outside the embedding tables (an atomic scatter unless DAGNN_AMD_TABLE_GRADS=1) and the loss."""
    _, _, differ = _case(cid)
    assert not differ, differ


# ------------------------------------------------------------------------------------------------ the tie cases can fail (CPU)
class _FirstWinner(torch.autograd.Function):
    """`amax` over the messages of a node whose gradient goes, whole, to the first message that attains the maximum."""

    @staticmethod
    def forward(ctx, msg, index, num_nodes):
        idx = index.view(-1, 1).expand_as(msg)
        out = msg.new_zeros(num_nodes, msg.shape[1]).scatter_reduce_(0, idx, msg, "amax", include_self=False)
        n = msg.shape[0]
        pos = torch.arange(n).view(-1, 1).expand_as(msg)
        hit = msg == out[index]
        first = torch.full((num_nodes, msg.shape[1]), n).scatter_reduce_(0, idx, torch.where(hit, pos, n), "amin", include_self=True)
        ctx.save_for_backward(hit & (pos == first[index]), index)
        return out

    @staticmethod
    def backward(ctx, grad):
        win, index = ctx.saved_tensors
        return grad[index] * win.to(grad.dtype), None, None


def _max_oracle_step(propagate=None, monkeypatch=None):
    c = CASES["max-H64"]
    b, model = _batch("MIXED"), _model(c)
    if propagate is not None:
        monkeypatch.setattr(O, "_propagate", propagate)
    return b, Hh.code2_grads64(None, model, b, _labels(b), **_oracle_kw(c))


def test_the_ties_of_the_mixed_batch_are_real_and_carry_gradient(monkeypatch):
    """In the float64 oracle's forward of the `max` model on MIXED, the target of the duplicate edge and the target of the twin
    roots each receive at least two messages that are equal in EVERY column, and the loss gradient at those aggregates is not
    zero: a kernel that hands each tied message the whole gradient computes something else."""
    real = O._propagate
    seen = []

    def spy(msg, index, num_nodes, reduce):
        out = real(msg, index, num_nodes, reduce)
        rec = dict(msg=msg.detach(), index=index, grad=None)
        if reduce == "max" and out.requires_grad:
            out.register_hook(lambda g, rec=rec: rec.__setitem__("grad", g.detach()))
            seen.append(rec)
        return out

    b, _ = _max_oracle_step(spy, monkeypatch)
    dup = int((b.batch == 5).nonzero().max())              # graph 5 = the duplicate edge 0 -> 1, 0 -> 1
    twin = b.x.shape[0] - 1                                # the twin roots are the last graph, their target its last node
    assert int((b.batch == 5).sum()) == 2 and int((b.batch == b.batch[twin]).sum()) == 3
    for node in (dup, twin):
        found = 0
        for rec in seen:
            rows = (rec["index"] == node).nonzero().view(-1)
            if rows.numel() < 2 or rec["grad"] is None:
                continue
            m = rec["msg"][rows]
            if bool((m == m[0]).all()) and float(rec["grad"][node].abs().max()) > 0:
                found += 1
        assert found >= 1, node


def test_max_prepare_checks_its_arguments_before_any_launch():
    """`ties` is the last field of `dagnn_variant_bwd_cell`: the ctypes mirror and the C struct agree on where it lies (the one
    missing value each case plants is refused; an empty row range with everything in place is not)."""
    import ctypes
    from dagnn_amd import _lib
    lib = _lib.load()
    plan = _lib.Plan(64, 0, 4, 3, 1, 0)
    c = _lib.VariantBwdCell()
    c.mode, c.lands, c.h, c.a = _lib.AGG_MAX, 1, 64, 64
    assert _lib.VariantBwdCell._fields_[-1][0] == "ties"
    assert lib.dagnn_variant_max_prepare(ctypes.byref(plan), ctypes.byref(c), 0, 8, 8, 2, 2, None) == -22   # no ties buffer
    c.ties = 64
    assert lib.dagnn_variant_max_prepare(ctypes.byref(plan), ctypes.byref(c), 0, 8, 8, 2, 2, None) == 0     # empty range
    assert lib.dagnn_variant_max_prepare(ctypes.byref(plan), ctypes.byref(c), 0, 8, 7, 2, 2, None) == -22   # pitch < width
    assert lib.dagnn_variant_max_prepare(ctypes.byref(plan), ctypes.byref(c), 0, 8, 8, 0, 5, None) == -22   # beyond N
    c.mode = _lib.AGG_ADD
    assert lib.dagnn_variant_max_prepare(ctypes.byref(plan), ctypes.byref(c), 0, 8, 8, 2, 2, None) == -22   # not a max cell


def test_both_conserving_tie_conventions_give_the_same_parameter_gradients(monkeypatch):
    """The whole gradient to the first tied message instead of an even split: every parameter gradient of the `max` model on
    MIXED within 1e-12 of its largest entry (tied sources have identical states and inputs) - the comparison of the GPU cases
    with the even-split oracle is valid for either convention."""
    _, (loss_even, even) = _max_oracle_step()
    real = O._propagate
    used = []

    def first_winner(msg, index, num_nodes, reduce):
        if reduce != "max":
            return real(msg, index, num_nodes, reduce)
        used.append(1)
        return _FirstWinner.apply(msg, index, num_nodes)

    _, (loss_first, first) = _max_oracle_step(first_winner, monkeypatch)
    assert used and float(loss_even) == float(loss_first)
    assert set(even) == set(first)
    for k, ref in even.items():
        scale = float(ref.abs().max())
        assert float((first[k] - ref).abs().max()) <= 1e-12 * scale, (k, float((first[k] - ref).abs().max()), scale)
