"""Training passes of `agg` = `add` / `max` on the two persistent dataflow kernels (`variant_backend = "dataflow"`:
`variants.PlainRecurrence` - the PLAIN loaders of csrc/dataflow.hip forward, the reverse sweep of csrc/bwd_dataflow.hip with a
plain pull, `dagnn_plain_max_weights` / `dagnn_plain_edge_grads` around it) against the reference's fixtures and the float64
oracle, with the convention of tests/test_variants_bwd_gpu.py unchanged (its helpers, batches and bound are imported):

    per tensor e_hip <= 4 x max(e_torch over the two fp32 torch baselines, 2^-23 x scale); |hip| <= 1e-6 where the oracle is
    exactly zero; tensors with scale <= 2e-5: e_hip <= 2e-7; the loss within 1e-5.

Shapes: one column block (64), a padded row (72 -> 128 wide), all four column blocks of the `max` weights (256), emb width !=
hidden width, L = 2 and 3 (the du chain), with / without the edge encoder, both directions (direction 1 aggregates nothing) and
one with every node pooled, the MIXED batch (real `max` ties; a 200-way fan-out: the loader's overflow trips; sinks) and the
WIDE_LAYER batch (2102 graphs: every group of the schedule has work).

`MEASURED`: per case the largest ratio of a tensor's error to max(e_torch, ulp) (bound 4) that `_report` printed on one MI355X -
recorded, not asserted."""
from __future__ import annotations

import functools
import warnings

import pytest
import torch

from dagnn_amd import engine, variants
from dagnn_amd.train import ClipAdam
from tests import helpers as Hh
from tests import test_variants_bwd_gpu as T

# case: (worst relative error of a tensor larger than 2e-5 - torch baselines, HIP -; the largest ratio of a tensor's HIP error to
# max(e_torch, ulp), bound 4, and that tensor) - recorded from `_report` on one MI355X, not asserted
MEASURED = {
    "add-H64": (4.0e-06, 3.9e-06, 1.70, "graph_pred_linear_list.0.bias"), "max-H64": (4.9e-07, 5.3e-07, 1.54, "cells_1.0.weight_ih"),
    "add-H72": (4.6e-06, 2.5e-06, 2.19, "graph_pred_linear_list.1.bias"), "max-H72": (3.3e-07, 2.8e-07, 1.40, "encoder.attribute_encoder.weight"),
    "add-H256": (6.1e-06, 3.5e-06, 1.44, "cells_1.0.weight_ih"), "max-H256": (4.7e-07, 5.7e-07, 1.25, "node_aggr_0.0.edge_encoder.bias"),
    "add-E32-H72": (1.8e-05, 1.0e-05, 1.21, "cells_1.0.weight_ih"), "max-E32-H72": (3.6e-07, 4.6e-07, 1.39, "graph_pred_linear_list.0.bias"),
    "add-H64-L3": (1.4e-05, 1.0e-05, 1.51, "cells_0.0.weight_hh"), "max-H64-L3": (3.6e-07, 4.0e-07, 1.26, "cells_1.2.weight_ih"),
    "add-H72-noedgeattr": (1.3e-06, 9.7e-07, 1.50, "graph_pred_linear_list.0.bias"), "max-H72-noedgeattr": (3.2e-07, 3.2e-07, 1.51, "cells_0.1.bias_ih"),
    "add-H72-unidir-poolall": (8.8e-06, 1.4e-05, 2.07, "node_aggr_0.0.edge_encoder.weight"),
    "max-H72-unidir-poolall": (4.6e-07, 4.4e-07, 1.22, "node_aggr_0.0.edge_encoder.bias"),
    "add-H64-widelayer": (2.4e-06, 1.5e-06, 1.28, "encoder.depth_encoder.weight"), "max-H64-widelayer": (2.4e-06, 1.5e-06, 1.30, "encoder.depth_encoder.weight"),
}

CASES = dict([
    T._case_of("add-H64", "add", 64), T._case_of("max-H64", "max", 64),
    T._case_of("add-H72", "add", 72), T._case_of("max-H72", "max", 72),
    T._case_of("add-H256", "add", 256), T._case_of("max-H256", "max", 256),
    T._case_of("add-E32-H72", "add", 72, E=32), T._case_of("max-E32-H72", "max", 72, E=32),
    T._case_of("add-H64-L3", "add", 64, L=3), T._case_of("max-H64-L3", "max", 64, L=3),
    T._case_of("add-H72-noedgeattr", "add", 72, w_edge_attr=False), T._case_of("max-H72-noedgeattr", "max", 72, w_edge_attr=False),
    T._case_of("add-H72-unidir-poolall", "add", 72, bidirectional=False, out_pool_all=True),
    T._case_of("max-H72-unidir-poolall", "max", 72, bidirectional=False, out_pool_all=True),
    T._case_of("add-H64-widelayer", "add", 64, batch="WIDE_LAYER"), T._case_of("max-H64-widelayer", "max", 64, batch="WIDE_LAYER"),
])
BOTH_BACKENDS = ("add-H72", "max-H72")   # cases whose lock-step step is held to the same bound (test 4)


def _hip_steps(model, b, y, dev, backend, steps=2):
    """`steps` training steps under `backend` with the sweep's entry points counted and the torch-ops recurrence refused:
    ([(loss, grads)], path of the last pass, {entry point: calls})."""
    model.variant_backend = backend
    lib = engine._lib.load()
    spies = {n: T._Spy(getattr(lib, n)) for n in ("dagnn_variant_backward_run", "dagnn_bwd_dataflow_run", "dagnn_dataflow_run")}
    seen, run = variants._TORCH_PATH_SEEN, variants.run
    out = []
    try:
        for n, s in spies.items():
            setattr(lib, n, s)
        variants._TORCH_PATH_SEEN = set()
        variants.run = T._refuse
        with warnings.catch_warnings():
            warnings.filterwarnings("error", category=RuntimeWarning, message=".*torch ops.*")
            for _ in range(steps):
                out.append(T._cpu64(*Hh._train_step(model, b.clone().to(dev), y.to(dev))))
        torch.cuda.synchronize()
        model.check()
    finally:
        for n, s in spies.items():
            setattr(lib, n, s.fn)
        variants._TORCH_PATH_SEEN, variants.run = seen, run
    return out, model.last_variant_path, {n: s.calls for n, s in spies.items()}


@functools.lru_cache(maxsize=None)
def _baselines(cid):
    """(float64 loss and gradients, the two fp32 torch baselines' gradients) of a case - computed once, shared by every test."""
    c = CASES[cid]
    dev = torch.device("cuda:0")
    b, model = T._batch(c["batch"]), T._model(c)
    y = T._labels(b)
    loss_r, g_r = Hh.code2_grads64(None, model, b, y, **T._oracle_kw(c))
    _, g_c = T._torch_step_cpu(model, b.clone(), y)
    model = model.to(dev)
    model.variant_backend = "torch"
    _, g_t = T._cpu64(*Hh._train_step(model, b.clone().to(dev), y.to(dev)))
    return float(loss_r), g_r, g_c, g_t


@functools.lru_cache(maxsize=None)
def _case(cid, backend="dataflow", stat_fwd=1):
    """Rows (name, scale, e_torch, e_hip, largest |hip| at the oracle's exact zeros) as in tests/test_variants_bwd_gpu.py, the
    losses, the names whose two steps differ in a bit, the path taken and the entry points' call counts."""
    c = CASES[cid]
    dev = torch.device("cuda:0")
    loss_r, g_r, g_c, g_t = _baselines(cid)
    b, model = T._batch(c["batch"]), T._model(c).to(dev)
    keep, engine.STAT_FWD = engine.STAT_FWD, stat_fwd   # (0: the forward launch hands over gh / gi, `bd_stat_kernel` makes the static rows)
    try:
        (s1, s2), path, calls = _hip_steps(model, b, T._labels(b), dev, backend)
    finally:
        engine.STAT_FWD = keep
    (loss_h, g_h), (loss_h2, g_h2) = s1, s2
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
    return rows, (loss_r, loss_h), differ, path, calls


def _failures(rows, loss_r, loss_h):
    failures = []
    if abs(loss_h - loss_r) > 1e-5:
        failures.append("loss %.8f, oracle %.8f" % (loss_h, loss_r))
    for name, scale, e_t, e_h, at_zero in rows:
        if scale <= T.TINY_SCALE:
            if max(e_h, at_zero) > T.TINY_ABS:
                failures.append("%s: %.3e at scale %.3e (rounding noise: at most %.0e)" % (name, max(e_h, at_zero), scale, T.TINY_ABS))
            continue
        if at_zero > T.ZERO_FLOOR:
            failures.append("%s: %.3e where the oracle is exactly zero" % (name, at_zero))
        bound = T.FACTOR * max(e_t, T.ULP * scale)
        if e_h > bound:
            failures.append("%s: hip %.3e > %.3e = %.0f x max(torch %.3e, ulp %.3e)" % (name, e_h, bound, T.FACTOR, e_t, T.ULP * scale))
    return failures


# ------------------------------------------------------------------------------------------------ 1. the reference's fixtures
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grad_var_h64_add", "grad_var_h64_max"])
def test_reference_fixture_gradients_on_the_dataflow_kernels(device, name):
    """Loss and every stored parameter gradient of the reference's own `loss.backward()` at the tolerance of the existing
    fixture test (`Hh.check_grads`, rtol 1e-4 + 2e-7 - `Hh.check_grads_full`'s); the pass ran on the dataflow kernels and the
    lock-step sweep did not run.  (Fails before this path existed: the backend value changes nothing there.)"""
    meta, arr = Hh.load(name)
    model = Hh.code2_model(meta).to(device)
    model.variant_backend = "dataflow"
    lib = engine._lib.load()
    spy = T._Spy(lib.dagnn_variant_backward_run)
    try:
        lib.dagnn_variant_backward_run = spy
        loss, grads = Hh._train_step(model, Hh.code2_batch(arr, device), torch.from_numpy(arr["y"]).to(device))
        torch.cuda.synchronize()
    finally:
        lib.dagnn_variant_backward_run = spy.fn
    model.check()
    assert model.last_variant_path == "dataflow", (model.last_variant_path, getattr(model.last_variant_route, "why", None))
    assert spy.calls == 0, "the lock-step sweep ran %d times" % spy.calls
    assert abs(float(loss) - float(arr["loss"])) < 1e-5
    Hh.check_grads(meta, arr, grads, rtol=1e-4)


# ------------------------------------------------------------------------------------------------ 2. the float64 oracle
@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_training_step_gradients_match_the_float64_oracle(device, cid):
    rows, (loss_r, loss_h), _, path, calls = _case(cid)
    T._report(cid, rows)
    assert path == "dataflow" and calls["dagnn_variant_backward_run"] == 0 and calls["dagnn_bwd_dataflow_run"] >= 2 and \
        calls["dagnn_dataflow_run"] >= 2, (path, calls)
    failures = _failures(rows, loss_r, loss_h)
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["add-H72", "max-H256"])
def test_the_preactivation_handover_meets_the_same_bound(device, cid):
    """`DAGNN_AMD_STAT_FWD=0`: the reverse sweep's static rows come from `bd_stat_kernel` (gi, gh, the recomputed aggregate)
    instead of the forward launch - the other of the two hand-overs the sweep's preparation reads."""
    rows, (loss_r, loss_h), differ, path, calls = _case(cid, "dataflow", 0)
    assert path == "dataflow" and calls["dagnn_variant_backward_run"] == 0, (path, calls)
    failures = _failures(rows, loss_r, loss_h)
    assert not failures and not differ, (failures, differ)


# ------------------------------------------------------------------------------------------------ 3. bitwise repeatability
@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_two_training_steps_are_bitwise_equal(device, cid):
    """The loss and every gradient outside the embedding tables (an atomic scatter unless DAGNN_AMD_TABLE_GRADS=1)."""
    differ = _case(cid)[2]
    assert not differ, differ


# ------------------------------------------------------------------------------------------------ 4. both backends
@pytest.mark.gpu
@pytest.mark.parametrize("cid", BOTH_BACKENDS)
def test_both_backends_are_within_bound_of_the_oracle(device, cid):
    for backend, want in (("dataflow", "dataflow"), ("hip", "lockstep")):
        rows, (loss_r, loss_h), _, path, calls = _case(cid, backend)
        assert path == want, (backend, path)
        assert (calls["dagnn_variant_backward_run"] > 0) == (backend == "hip"), calls
        failures = _failures(rows, loss_r, loss_h)
        assert not failures, (backend, failures)


# ------------------------------------------------------------------------------------------------ 5. fall-backs
FALLBACKS = dict([
    T._case_of("add-H344", "add", 344), T._case_of("max-aggx-H72", "max", 72, agg_x=True),
    T._case_of("add-recurr0-H72", "add", 72, recurr=0), T._case_of("max-H72-flag-off", "max", 72),
])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(FALLBACKS))
def test_passes_that_do_not_qualify_run_the_lockstep_sweep_bit_for_bit(device, cid, monkeypatch):
    c = FALLBACKS[cid]
    if cid.endswith("flag-off"):
        monkeypatch.setattr(engine, "VARIANT_DATAFLOW", 0)
    b = T._batch(c["batch"])
    y = T._labels(b)
    res = {}
    for backend in ("dataflow", "hip"):
        model = T._model(c).to(device)
        (step,), path, calls = _hip_steps(model, b, y, device, backend, steps=1)
        assert path == "lockstep" and calls["dagnn_variant_backward_run"] == 1 and calls["dagnn_bwd_dataflow_run"] == 0, (backend, path, calls)
        if backend == "dataflow":
            assert model.last_variant_route.why, "a fall-back names its reason"
        res[backend] = step
    assert res["dataflow"][0] == res["hip"][0]
    differ = [k for k in res["hip"][1] if not k.startswith("encoder.") and not torch.equal(res["hip"][1][k], res["dataflow"][1][k])]
    assert not differ, differ


# ------------------------------------------------------------------------------------------------ 6. the caches see the updates
@pytest.mark.gpu
@pytest.mark.parametrize("agg", ["add", "max"])
def test_three_optimizer_steps_then_evaluation_reads_the_new_weights(device, agg):
    c = CASES[agg + "-H72"]
    b = T._batch("MIXED")
    y = T._labels(b).to(device)
    model = T._model(c).to(device)
    model.variant_backend = "dataflow"
    opt = ClipAdam(model.parameters(), lr=1e-2, max_norm=0.25)
    for _ in range(3):
        Hh._train_step(model, b.clone().to(device), y)
        assert model.last_variant_path == "dataflow"
        opt.step()
    model.eval()
    with torch.no_grad():
        out = model(b.clone().to(device))
    fresh = T._model(c).to(device)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    with torch.no_grad():
        ref = fresh(b.clone().to(device))
    torch.cuda.synchronize()
    model.check()
    for o, r in zip(out, ref):
        assert torch.equal(o, r)
