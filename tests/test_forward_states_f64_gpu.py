"""Every node's state row of a forward pass against the float64 oracle, class by class of in-degree, on every path the
recurrence can take (inputs, reference and bound: `tests/forward_states_f64.py`, shown able to fail by
`tests/test_forward_states_cpu.py`).

One model, one batch and its edge-reversed twin, one forward pass each per test.  The batches hold every in-degree class of
`FS.DEGS` at layer 2 or deeper in BOTH directions (ladder graphs and their transposes), `GENERAL` beyond the limits of the
one-workgroup plan builds and with the degenerate graphs of the parity tests behind the ladders (single nodes, a chain of 40,
200-way fan-in and fan-out, no edges, a duplicate edge: real ties for `max`), `SMALL` inside those limits.  Every test spies
on the library's entry points and FAILS if the path it names did not run.

Bound: per (direction, stacked layer) block `e <= 4 x max(e_base, 2^-23 max|ref|)` for the rows of every class, `e_base` the
fp32 oracle's own error against float64 over all rows of the block.  Nothing in it is derived from the HIP result.

`MEASURED`: per case the worst ratio e / max(e_base, ulp) over both batches and the class it belongs to, as `FS._report`
printed them on one MI355X - recorded, not asserted."""
from __future__ import annotations

import warnings

import pytest
import torch

from dagnn_amd import DAGNN, ASTNodeEncoder, engine
from oracle.seeding import seeded_fill
from tests import forward_states_f64 as FS
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

# case id: (worst ratio e / max(e_base, ulp) over both batches - bound 4 -, the class and the block it belongs to, that e, the block's
# e_base) - recorded from `FS._report` on one MI355X, not asserted.  Cases that differ in launch shape alone print the same figures.
MEASURED = {
    "dataflow-H64":                          (1.00, 1, "(1, 1)", 1.875e-07, 1.871e-07),
    "dataflow-H100":                         (0.88, 1, "(0, 0)", 7.799e-07, 8.851e-07),
    "dataflow-H256":                         (0.80, 1, "(1, 0)", 1.449e-06, 1.808e-06),
    "dataflow-H256-unidir":                  (1.11, 1, "(0, 0)", 1.756e-06, 1.580e-06),
    "dataflow-H64-noedgeattr":               (1.07, 1, "(1, 1)", 1.769e-07, 1.659e-07),
    "dataflow-wide-H300-L2":                 (1.12, 9, "(0, 0)", 1.462e-06, 1.301e-06),
    "dataflow-wide-H320-L1":                 (1.19, 16, "(1, 0)", 1.539e-06, 1.296e-06),
    "dataflow-attn_x-H64":                   (0.91, 9, "(1, 0)", 5.615e-07, 6.145e-07),
    "dataflow-self_attn_h-H64":              (1.19, 9, "(1, 1)", 1.988e-07, 1.674e-07),
    "dataflow-self_attn_x-H64":              (1.10, 8, "(0, 1)", 2.482e-07, 2.266e-07),
    "add-H72-dataflow":                      (1.37, 129, "(0, 0)", 1.846e-04, 1.350e-04),
    "add-H72-launches":                      (1.14, 129, "(0, 0)", 1.541e-04, 1.350e-04),
    "add-H256-dataflow":                     (2.97, 129, "(0, 0)", 1.717e-04, 5.785e-05),
    "add-H256-launches":                     (3.10, 129, "(0, 0)", 1.794e-04, 5.785e-05),
    "max-H72-dataflow":                      (1.10, 0, "(1, 0)", 4.739e-07, 4.293e-07),
    "max-H72-launches":                      (1.00, 1, "(0, 0)", 1.052e-06, 1.052e-06),
    "max-H256-dataflow":                     (1.40, 9, "(0, 0)", 1.608e-06, 1.147e-06),
    "max-H256-launches":                     (1.10, 128, "(0, 1)", 7.843e-07, 7.143e-07),
    "lockstep-H64-default":                  (0.98, 7, "(1, 0)", 5.613e-07, 5.723e-07),
    "lockstep-H64-mfma_tiles":               (0.98, 7, "(1, 0)", 5.613e-07, 5.723e-07),
    "lockstep-H64-no_tail":                  (0.98, 7, "(1, 0)", 5.613e-07, 5.723e-07),
    "lockstep-H64-mfma_tiles-no_tail":       (0.98, 7, "(1, 0)", 5.613e-07, 5.723e-07),
    "lockstep-H256-default":                 (0.80, 1, "(1, 0)", 1.449e-06, 1.808e-06),
    "lockstep-H256-mfma_tiles":              (0.80, 1, "(1, 0)", 1.449e-06, 1.808e-06),
    "lockstep-H256-no_tail":                 (0.80, 1, "(1, 0)", 1.449e-06, 1.808e-06),
    "lockstep-H256-mfma_tiles-no_tail":      (0.80, 1, "(1, 0)", 1.449e-06, 1.808e-06),
    "pergraph-H64":                          (1.00, 9, "(1, 1)", 1.880e-07, 1.871e-07),
    "tiles-H512":                            (1.03, 0, "(0, 0)", 1.909e-06, 1.849e-06),
    "tiles-H300":                            (1.15, 9, "(0, 0)", 1.499e-06, 1.301e-06),
    "fat-H512-L2-dual":                      (1.03, 0, "(0, 0)", 1.909e-06, 1.849e-06),
    "fat-H512-L2-single":                    (1.03, 0, "(0, 0)", 1.909e-06, 1.849e-06),
    "fat-H384-L1-dual":                      (1.18, 0, "(0, 0)", 1.867e-06, 1.582e-06),
    "fat-H384-L1-single":                    (1.18, 0, "(0, 0)", 1.867e-06, 1.582e-06),
    "plan-small-H64":                        (1.03, 3, "(1, 1)", 1.566e-07, 1.516e-07),
    "plan-general-H64":                      (1.03, 3, "(1, 1)", 1.566e-07, 1.516e-07),
    "plan-small-H256":                       (0.89, 1, "(1, 0)", 1.185e-06, 1.338e-06),
    "plan-general-H256":                     (0.89, 1, "(1, 0)", 1.185e-06, 1.338e-06),
    "train-forward-H256":                    (0.81, 7, "(1, 0)", 1.456e-06, 1.808e-06),
    "dvae-na-hs56-small":                    (1.92, 9, "(0, 0)", 1.094e-07, 5.685e-08),
    "dvae-na-hs56-general":                  (1.92, 9, "(0, 0)", 1.094e-07, 5.685e-08),
    "dvae-na-hs128-small":                   (2.24, 5, "(0, 0)", 1.312e-07, 5.849e-08),
    "dvae-na-hs128-general":                 (2.24, 5, "(0, 0)", 1.312e-07, 5.849e-08),
    "dvae-na-hs501-small":                   (0.83, 3, "(0, 0)", 6.225e-08, 7.510e-08),
    "dvae-na-hs501-general":                 (0.83, 3, "(0, 0)", 6.225e-08, 7.510e-08),
    "dvae-bn-hs56-small":                    (1.12, 4, "(unified,)", 1.476e-07, 1.313e-07),
    "dvae-bn-hs56-general":                  (1.12, 4, "(unified,)", 1.476e-07, 1.313e-07),
    "dvae-bn-hs128-small":                   (2.85, 5, "(unified,)", 2.939e-07, 1.030e-07),
    "dvae-bn-hs128-general":                 (2.85, 5, "(unified,)", 2.939e-07, 1.030e-07),
    "dvae-bn-hs501-small":                   (1.85, 9, "(unified,)", 1.895e-07, 1.027e-07),
    "dvae-bn-hs501-general":                 (1.85, 9, "(unified,)", 1.895e-07, 1.027e-07),
}


# ------------------------------------------------------------------ models, batches, references: built once per session
_batch = FS.build_batch


_MODELS, _REFS = {}, {}


def _code2(device, H, L=2, bidirectional=True, agg="attn_h", w_edge_attr=True):
    key = ("code2", H, L, bidirectional, agg, w_edge_attr)
    if key not in _MODELS:
        enc = ASTNodeEncoder(H, 98, 300, 20)
        model = DAGNN(num_vocab=7, max_seq_len=2, emb_dim=H, hidden_dim=H, out_dim=None, encoder=enc, w_edge_attr=w_edge_attr,
                      num_layers=L, bidirectional=bidirectional, agg=agg, out_wx=False, out_pool_all=True, out_pool="max",
                      dropout=0.0).eval()
        seeded_fill(model, 4000 + H + L)
        _MODELS[key] = model.to(device)
    return key, _MODELS[key]


def _dvae(device, kind, hs):
    key = ("dvae", kind, hs)
    if key not in _MODELS:
        model = Hh.dvae_decoder_model(kind, max_n=14, nvt=6, hs=hs, L=2 if kind == "bn" else 1, seed=7)
        model.output_all = True   # the read-out over all nodes (dvae/dagnn.py:163-172): G.h keeps a row per node
        _MODELS[key] = model.to(device)
    return key, _MODELS[key]


def _reference(key, model, name, twin):
    """One float64 reference per (model, batch): the cases that differ in the path alone share it."""
    if (key, name, twin) not in _REFS:
        _REFS[(key, name, twin)] = FS.reference(model, _batch(name, twin))
    return _REFS[(key, name, twin)]


# ------------------------------------------------------------------ which path ran
def _cell0(args):
    return args.cell[0][0]


_ENTRIES = {
    "dagnn_dataflow_run": lambda a: dict(H=a[1]._obj.H, stat_rows=a[1]._obj.stat_rows, vid_mod=a[1]._obj.vid_mod,
                                         static=bool(_cell0(a[1]._obj).static_score), agg=_cell0(a[1]._obj).agg,
                                         flags=a[0]._obj.flags),
    "dagnn_frontier_run": lambda a: dict(H=a[1]._obj.H, mfma_min_rows=a[1]._obj.mfma_min_rows, vid_mod=a[1]._obj.vid_mod,
                                         tail_replicas=a[1]._obj.tail_replicas, chains=bool(a[1]._obj.side_stream),
                                         flags=a[0]._obj.flags),
    "dagnn_tiles_run": lambda a: dict(H=a[1]._obj.H, vid_mod=a[1]._obj.vid_mod, flags=a[0]._obj.flags),
    "dagnn_recurrence_layer": lambda a: dict(H=a[3], flags=a[0]._obj.flags),
    "dagnn_variant_run": lambda a: dict(H=a[1]._obj.H, flags=a[0]._obj.flags),
}


def _spy(monkeypatch):
    """{C entry point of a recurrence: [what its argument structs said, per call]} (`test_gpu_parity._spy_entries`)."""
    lib = engine._lib.load()
    seen = {}
    for name, read in _ENTRIES.items():
        seen[name] = []
        orig = getattr(lib, name)

        def spy(*a, _name=name, _read=read, _orig=orig):
            seen[_name].append({k: int(v) for k, v in _read(a).items()})
            return _orig(*a)
        monkeypatch.setattr(lib, name, spy, raising=False)
    return seen


def _only(seen, entry, **fields):
    """The pass ran `entry` - with these argument fields, every call - and no other recurrence."""
    others = {k: v for k, v in seen.items() if k != entry and v}
    assert seen[entry] and not others, "expected %s alone, saw %s" % (entry, {k: len(v) for k, v in seen.items()})
    for call in seen[entry]:
        assert all(call[f] == v for f, v in fields.items()), (entry, fields, call)


def _forward(model, batch, device, train=False):
    for c in model._derived.values():
        c.invalidate()
    G = batch.clone().to(device)
    if train:   # a training pass: gradients enabled, module in train() mode (dropout 0)
        model.train()
        try:
            model(G)
        finally:
            model.eval()
    else:
        with torch.no_grad():
            model(G)
    model.check()
    return FS.blocks_of(G.h, model)


def _case(device, monkeypatch, cid, key, model, name, path, train=False):
    """Both batches of `name` through `model`; `path(seen)` asserts the route of each pass; then the bound."""
    seen = _spy(monkeypatch)
    reports, failure = [], None
    for twin in (False, True):
        batch = _batch(name, twin)
        ref = _reference(key, model, name, twin)
        for calls in seen.values():
            calls.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)   # (widths off the dataflow kernel say so once: not this file's subject)
            got = _forward(model, batch, device, train)
        path(seen)
        cls = {d: FS.classes(batch, d) for d in (0, 1)}
        try:
            reports += FS.check(got, ref, cls)
        except FS.StateMismatch as e:
            reports += e.report
            failure = failure or e
    for c in model._derived.values():
        c.invalidate()
    FS._report(cid, reports)   # (printed before the assertion)
    if failure is not None:
        raise failure


def _set(monkeypatch, **flags):
    for k, v in flags.items():
        monkeypatch.setattr(engine, k, v)


# ------------------------------------------------------------------ a, b: the dataflow kernel
_GENERAL_CASES = [("H64", 64, {}), ("H100", 100, {}), ("H256", 256, {}), ("H256-unidir", 256, dict(bidirectional=False)),
                  ("H64-noedgeattr", 64, dict(w_edge_attr=False))]


@pytest.mark.parametrize("tag,H,kw", _GENERAL_CASES, ids=[c[0] for c in _GENERAL_CASES])
def test_dataflow_general_loaders(device, monkeypatch, tag, H, kw):
    key, model = _code2(device, H, **kw)
    Hp = (H + 63) // 64 * 64   # (100 runs padded to 128)
    _case(device, monkeypatch, "dataflow-" + tag, key, model, "GENERAL",
          lambda seen: _only(seen, "dagnn_dataflow_run", H=Hp, static=0, agg=0))


@pytest.mark.parametrize("H,L", [(300, 2), (320, 1)])
def test_dataflow_wide_lean_loaders(device, monkeypatch, H, L):
    assert engine.DF_WIDE == 1
    key, model = _code2(device, H, L=L)
    _case(device, monkeypatch, "dataflow-wide-H%d-L%d" % (H, L), key, model, "GENERAL",
          lambda seen: _only(seen, "dagnn_dataflow_run", H=320, static=0))


# ------------------------------------------------------------------ c: static-score loaders
@pytest.mark.parametrize("agg", ["attn_x", "self_attn_h", "self_attn_x"])
def test_dataflow_static_score_loaders(device, monkeypatch, agg):
    key, model = _code2(device, 64, agg=agg)
    _case(device, monkeypatch, "dataflow-%s-H64" % agg, key, model, "GENERAL",
          lambda seen: _only(seen, "dagnn_dataflow_run", H=64, static=int("_x" in agg)))


# ------------------------------------------------------------------ d: the PLAIN fold and the per-layer variant launches
@pytest.mark.parametrize("on_dataflow", [1, 0], ids=["dataflow", "launches"])
@pytest.mark.parametrize("H", [72, 256])
@pytest.mark.parametrize("agg", ["add", "max"])
def test_plain_fold(device, monkeypatch, agg, H, on_dataflow):
    _set(monkeypatch, VARIANT_DATAFLOW=on_dataflow)
    key, model = _code2(device, H, agg=agg)
    if on_dataflow:
        def path(seen):
            _only(seen, "dagnn_dataflow_run", H=128 if H == 72 else 256, agg=1 if agg == "add" else 2)
    else:
        def path(seen):
            _only(seen, "dagnn_variant_run", H=H)
    _case(device, monkeypatch, "%s-H%d-%s" % (agg, H, "dataflow" if on_dataflow else "launches"), key, model, "GENERAL", path)


# ------------------------------------------------------------------ e, f: lock-step launches, per-graph schedule
@pytest.mark.parametrize("knob", ["default", "mfma_tiles", "no_tail", "mfma_tiles-no_tail"])
@pytest.mark.parametrize("H", [64, 256])
def test_lockstep_launches(device, monkeypatch, H, knob):
    """`DAGNN_AMD_DATAFLOW=0`: the per-layer launches with the persistent tail behind them; 64-row MFMA tiles for every launch
    the tail leaves; every layer a launch of its own; and both (every launch of the pass on MFMA tiles)."""
    _set(monkeypatch, DATAFLOW=0)
    assert engine.TAIL_REPLICAS > 0 and engine.MFMA_MIN_ROWS > 1
    if "mfma_tiles" in knob:
        _set(monkeypatch, MFMA_MIN_ROWS=1)
    if "no_tail" in knob:
        _set(monkeypatch, TAIL_REPLICAS=0)
    want = dict(H=H, mfma_min_rows=engine.MFMA_MIN_ROWS, tail_replicas=engine.TAIL_REPLICAS)
    key, model = _code2(device, H)
    _case(device, monkeypatch, "lockstep-H%d-%s" % (H, knob), key, model, "GENERAL",
          lambda seen: _only(seen, "dagnn_frontier_run", **want))


def test_pergraph_schedule(device, monkeypatch):
    key, model = _code2(device, 64)
    monkeypatch.setattr(model, "schedule", "pergraph")
    _case(device, monkeypatch, "pergraph-H64", key, model, "GENERAL", lambda seen: _only(seen, "dagnn_recurrence_layer", H=64))


# ------------------------------------------------------------------ g, h: the tile kernel, the fat launches
@pytest.mark.parametrize("H", [512, 300])
def test_tile_kernel(device, monkeypatch, H):
    _set(monkeypatch, TILES=2)
    if H == 300:
        _set(monkeypatch, DF_WIDE=0)   # (with it 257..320 run on the dataflow kernel: test_dataflow_wide_lean_loaders)
    key, model = _code2(device, H)
    _case(device, monkeypatch, "tiles-H%d" % H, key, model, "GENERAL", lambda seen: _only(seen, "dagnn_tiles_run", H=512))


@pytest.mark.parametrize("dual", [1, 0], ids=["two-chains", "one-chain"])
@pytest.mark.parametrize("H,L", [(512, 2), (384, 1)])
def test_fat_launches(device, monkeypatch, H, L, dual):
    _set(monkeypatch, TILES=0, MFMA_MIN_ROWS=1, DUAL_CHAINS=dual)
    key, model = _code2(device, H, L=L)
    _case(device, monkeypatch, "fat-H%d-L%d-%s" % (H, L, "dual" if dual else "single"), key, model, "GENERAL",
          lambda seen: _only(seen, "dagnn_frontier_run", H=H, mfma_min_rows=1, tail_replicas=0, chains=dual))


# ------------------------------------------------------------------ i: one-workgroup plan builds against the general ones
@pytest.mark.parametrize("small", [1, 0], ids=["small-build", "general-build"])
@pytest.mark.parametrize("H", [64, 256])
def test_plan_builds(device, monkeypatch, H, small):
    _set(monkeypatch, PLAN_SMALL=small)
    key, model = _code2(device, H)
    _case(device, monkeypatch, "plan-%s-H%d" % ("small" if small else "general", H), key, model, "SMALL",
          lambda seen: _only(seen, "dagnn_dataflow_run", H=H, flags=0 if small else engine.PLAN_GENERAL_BUILD))


# ------------------------------------------------------------------ j: the training-mode forward
def test_training_mode_forward_writes_the_static_rows(device, monkeypatch):
    assert engine.STAT_FWD == 1 and engine.BWD_DATAFLOW == 1
    key, model = _code2(device, 256)
    _case(device, monkeypatch, "train-forward-H256", key, model, "GENERAL",
          lambda seen: _only(seen, "dagnn_dataflow_run", H=256, stat_rows=1), train=True)


# ------------------------------------------------------------------ k: the D-VAE encoders
@pytest.mark.parametrize("small", [1, 0], ids=["small-build", "general-build"])
@pytest.mark.parametrize("hs", [56, 128, 501])
@pytest.mark.parametrize("kind", ["na", "bn"])
def test_dvae_encoders(device, monkeypatch, kind, hs, small):
    """NA: one direction, one layer, keys with the vertex-id bias (the raw states); BN: two directions, two stacked layers (the
    rows behind `hg_unify`, a per-node linear map of the four cells' rows, checked under the classes of both directions)."""
    _set(monkeypatch, PLAN_SMALL=small)
    key, model = _dvae(device, kind, hs)
    vid = 14 if kind == "na" else 0
    flags = 0 if small else engine.PLAN_GENERAL_BUILD

    def path(seen):
        if hs <= 256:
            _only(seen, "dagnn_dataflow_run", H=64 if hs == 56 else 128, vid_mod=vid, flags=flags)
        else:   # 501 runs 512 wide, off the dataflow kernel: on the tile kernel or on the per-layer launches (the policy's choice)
            ran = [k for k in ("dagnn_tiles_run", "dagnn_frontier_run") if seen[k]]
            assert len(ran) == 1, {k: len(v) for k, v in seen.items()}
            _only(seen, ran[0], H=512, vid_mod=vid, flags=flags)
    _case(device, monkeypatch, "dvae-%s-hs%d-%s" % (kind, hs, "small" if small else "general"), key, model, "DVAE", path)
