"""`dagnn_amd.route` without a GPU: the decisions recorded on an MI355X from the commit before the module existed
(`tests/golden/route_cases.json`, written by `scripts/route_cases.py`) replayed case by case, and the thresholds no small
batch reaches on synthetic sizes.  The library's host functions (group counts, record sizes) run here."""
import json
import os

import numpy as np
import pytest

from dagnn_amd import engine, route

with open(os.path.join(os.path.dirname(__file__), "golden", "route_cases.json")) as _f:
    GOLDEN = json.load(_f)
CASES = {c["name"]: c for c in GOLDEN["cases"]}
DEV = "cuda:0"   # (only a key: the CU count and the memory size are patched in)


class Plan(object):
    """What the route reads of a plan: sizes, and the layer row counts where a policy asks for them."""

    def __init__(self, N, R, B=4, rows=None):
        self.N, self.R, self.B, self.rows = N, R, B, rows

    def read_schedule(self):
        assert self.rows is not None, "this pass read no schedule"
        return [np.concatenate([[0], np.cumsum(r)]).astype(np.int32) for r in self.rows]


@pytest.fixture
def mi355x(monkeypatch):
    monkeypatch.setattr(engine, "_num_cus", lambda device: GOLDEN["device"]["cus"])
    monkeypatch.setattr(engine, "_total_memory", lambda device: GOLDEN["device"]["total_memory"])
    for name, v in (("DATAFLOW", 1), ("DF_WIDE", 1), ("DF_GROUPS", 0), ("TILES", 1), ("TILES_PAD", 1), ("TILES_MAX_NODES", 10000),
                    ("TILES_TAIL_ROWS", 32), ("TILES_MAX_MEAN_ROWS", 160), ("RESERVED_CUS", -1), ("STAT_FWD", 1), ("BWD_DATAFLOW", 1),
                    ("BWD_DF_MAX_BYTES", -1)):
        monkeypatch.setattr(engine, name, v)   # (the defaults the record was made with, whatever the environment says)
    return monkeypatch


def _recorded(p):
    """(kind, Hp, groups, tiles, split, stat_rows, reverse, warning) a recorded pass shows; kind None: no recurrence launch
    of the lock-step schedule ran (the per-layer variant kernels did)."""
    calls = p["calls"]
    by = lambda fn: [c for c in calls if c["fn"] == fn]   # noqa: E731
    df, ti, fr, args = by("dataflow_run"), by("tiles_run"), by("frontier_run"), by("dataflow_args")
    kind = "dataflow" if df or args else "launches+tiles" if fr and ti else "tiles" if ti else "launches" if fr else None
    first = (df or args or fr or ti or [{"H": None}])[0]
    tiles = [c["out"] for c in by("tiles_launches")]
    flat = [c["out"] for c in by("tiles_batch_too_flat")]
    reverse = "dataflow" if by("bwd_dataflow_sweep") else "lockstep" if by("backward_sweep") else None
    return dict(kind=kind, Hp=first["H"], groups=(df or args)[0]["groups"] if df or args else 0,
                tiles=tiles[0] if tiles and tiles[0] > 0 and not (flat and flat[0]) else 0,
                split=fr[0]["stop_layer"] if fr else None, stat_rows=bool(df and df[0]["preact"]), reverse=reverse,
                prepared=[c["groups"] for c in by("launch_prepare")], rows=(by("read_schedule") or [{"rows": None}])[0]["rows"],
                fused=bool(args and not df), warning=(p["warnings"] or [None])[0])


def _replay(case, name, p, rec):
    """The route of one recorded pass, asked the way the modules ask it."""
    train = name == "train"
    H, L, B, ndirs = case["H"], case["L"], case["B"], 2 if case["bidirectional"] else 1
    facts = p["facts"] or dict(N=0, R=0, B=B)   # (none: no recorded call was given the plan, and the route needs none)
    assert facts["B"] == B
    plan = Plan(facts["N"], facts["R"], B, rec["rows"])
    dirs = list(range(ndirs))
    if case["kind"] != "code2":   # the D-VAE encoders: no edge encoder, vertex-id key biases (NA)
        vid = 8 if case["kind"] == "na" else 0
        Hp, _ = route.width(H, L, 0, True, vid, False)
        if not train and case.get("encode_fused", 1):   # `_encode_fused`: the dataflow kernel or the general path
            groups = route.dataflow_only(DEV, ndirs, L, Hp, B, plan.N)
            if groups > 0:
                return route.Route(Hp, groups, "dataflow")
        r0 = route.before_plan(DEV, H, L, ndirs, plan.R, B, True, vid, False, train, Hp=Hp)   # `run_stack_lockstep`, from the cells
        return route.with_plan(r0, DEV, plan, dirs, L, plan.N, True, True, train)
    wea, agg = case["w_edge_attr"], case["agg"]
    if agg in ("add", "max"):   # `variants.run_plain_dataflow`: the dataflow kernel or the per-layer variant kernels
        Hp, df_ok = route.width(H, L, 0, True, 0, False)
        groups = route.dataflow_only(DEV, ndirs, L, Hp, B, plan.N) if df_ok else 0
        return route.Route(Hp, groups, "dataflow" if groups else None)
    Hp, _ = route.width(H, L, 2 if wea else 0, True, 0, wea)   # the cells (`derive_cell`: the keys are H wide, emb_dim == hidden_dim)
    keys_hidden = agg != "attn_x"
    r0 = route.before_plan(DEV, H, L, ndirs, plan.R, B, keys_hidden, 0, wea, train)   # `DAGNN._route0`
    if rec["prepared"] != [r0.groups]:
        # the one decision that moved: the recorded commit asked the library for groups at 320 wide before it looked whether
        # the model is one the 320-wide kernel serves, and built a schedule for them that no kernel read
        assert r0 == route.Route(320, 0) and rec["kind"] == "launches" and (not wea or not keys_hidden) and rec["prepared"][0] > 0, (r0, rec)
    if r0.Hp != Hp:   # (`run_stack_lockstep`: the route it was handed is for another width than the cells have)
        r0 = route.before_plan(DEV, H, L, ndirs, plan.R, B, keys_hidden, 0, wea, train, Hp=Hp)
    return route.with_plan(r0, DEV, plan, dirs, L, plan.N, keys_hidden, True, train)


@pytest.mark.parametrize("name", sorted(CASES))
def test_route_equals_the_recorded_decision(mi355x, name):
    case = CASES[name]
    for k, v in case["flags"].items():
        mi355x.setattr(engine, k, v)
    assert set(case["passes"]) == ({"eval", "train"} if case["train"] else {"eval"})
    for pname, p in sorted(case["passes"].items()):
        rec = _recorded(p)
        r = _replay(case, pname, p, rec)
        assert (r.kind, r.groups) == (rec["kind"], rec["groups"]), (pname, r, rec)
        if r.kind is None:
            continue
        assert r.Hp == rec["Hp"], (pname, r, rec)
        if not rec["fused"]:
            assert (r.stat_rows, r.reverse) == (rec["stat_rows"], rec["reverse"]), (pname, r, rec)
        if r.kind == "launches+tiles":
            assert list(r.split) == rec["split"] and r.tiles > 0, (pname, r, rec)
        else:
            assert r.split is None and rec["split"] is None and r.tiles == rec["tiles"], (pname, r, rec)
        assert (r.why is None) == (r.kind == "dataflow")
        if rec["warning"] is None:
            assert r.kind != "launches" or r.why in route.QUIET, (pname, r)
        else:
            assert r.kind == "launches" and r.why not in route.QUIET and (r.why == route.LIB or rec["warning"].endswith(r.why)), (pname, r, rec)


def test_every_kind_and_reverse_is_recorded():
    seen = [_recorded(p) for c in CASES.values() for p in c["passes"].values()]
    assert {s["kind"] for s in seen} == {"dataflow", "tiles", "launches+tiles", "launches", None}
    assert {s["reverse"] for s in seen} == {"dataflow", "lockstep", None} and len(CASES) >= 60


def _route(N, H=256, L=2, R=2, B=128, train=False, plan=None, ndirs=2):
    r0 = route.before_plan(DEV, H, L, ndirs, R, B, keys_hidden=True, edge_enc=R > 0, training=train)
    return route.with_plan(r0, DEV, plan or Plan(N, R, B), list(range(ndirs)), L, N, True, True, train)


def test_dataflow_ends_where_32_bit_row_offsets_end(mi355x):
    for H, N in ((256, 2796202), (64, 11184810)):
        r, over = _route(N, H), _route(N + 1, H)
        assert r.kind == "dataflow" and r.groups > 0 and r.why is None, r
        assert over.kind == "launches" and over.groups == 0 and over.why == route.LIB, over


def test_static_rows_need_32_bit_records(mi355x):
    mi355x.setattr(engine, "_total_memory", lambda device: 1 << 50)
    for H, N in ((256, 524287), (64, 524287), (320, 419430)):
        r, over = _route(N, H, train=True), _route(N + 1, H, train=True)
        assert r.Hp == (H + 63) // 64 * 64 and r.groups > 0
        assert (r.stat_rows, r.reverse) == (True, "dataflow") and (over.stat_rows, over.reverse) == (False, "dataflow"), (r, over)
    assert not _route(1000, 64).stat_rows and _route(1000, 64).reverse is None   # (evaluation)
    mi355x.setattr(engine, "STAT_FWD", 0)
    assert (_route(1000, 64, train=True).stat_rows, _route(1000, 64, train=True).reverse) == (False, "dataflow")


def test_reverse_sweep_follows_the_byte_cap(mi355x):
    mi355x.setattr(engine, "BWD_DF_MAX_BYTES", 8192 * 1000 * 4 * 3)   # 4 cells, three times their records
    r, over = _route(1000, 64, train=True), _route(1001, 64, train=True)
    assert (r.kind, r.reverse, r.stat_rows) == ("dataflow", "dataflow", True), r
    assert (over.kind, over.reverse, over.stat_rows) == ("dataflow", "lockstep", False), over
    mi355x.setattr(engine, "BWD_DATAFLOW", 0)
    assert (_route(10, 64, train=True).reverse, _route(10, 64, train=True).stat_rows) == ("lockstep", False)
    assert _route(10, 512, train=True).reverse == "lockstep"   # (the tile kernel's forward)


def test_tile_kernel_alone_behind_the_launches_or_not_at_all(mi355x):
    N = engine.TILES_MAX_NODES
    thin = [[300] * 30 + [3] * 40, [250] * 36 + [2] * 50]
    r = _route(N, 512, plan=Plan(N, 2, rows=[[100] * 100] * 2))
    assert (r.kind, r.tiles, r.split, r.groups, r.why) == ("tiles", 1, None, 0, route.POLICY), r
    r = _route(N + 1, 512, plan=Plan(N + 1, 2, rows=thin))
    assert (r.kind, r.tiles, list(r.split)) == ("launches+tiles", 1, [30, 36]) and r.why in route.QUIET, r
    r = _route(N + 1, 512, L=5, plan=Plan(N + 1, 2, rows=thin))
    assert (r.kind, r.tiles, list(r.split)) == ("launches+tiles", 2, [30, 36]), r
    r = _route(N + 1, 512, plan=Plan(N + 1, 2, rows=[[400] * 26] * 2))   # no thin tail
    assert (r.kind, r.tiles, r.split) == ("launches", 0, None) and r.why in route.QUIET, r
    r = _route(N, 512, plan=Plan(N, 2, rows=[[500] * 20] * 2))   # too flat for the kernel, and no tail either
    assert (r.kind, r.tiles, r.split) == ("launches", 0, None), r
    # batches of up to 1536 nodes are never too flat, and cost no read of the schedule (`Plan.read_schedule` asserts)
    assert _route(1536, 512).kind == "tiles"
    with pytest.raises(AssertionError, match="read no schedule"):
        _route(1537, 512)
    assert _route(1537, 512, L=1).kind == "launches" and _route(1537, 512, L=1).why.startswith("hidden size 512 > 256")
    mi355x.setattr(engine, "TILES", 0)
    assert _route(1537, 512).kind == "launches" and _route(1537, 512).why.startswith("hidden size 512 > 256")


def test_flags_are_read_when_the_route_is_asked(mi355x):
    assert _route(100, 64).kind == "dataflow"
    mi355x.setattr(engine, "DATAFLOW", 0)
    r = _route(100, 64)
    assert (r.kind, r.groups, r.why) == ("launches", 0, route.OFF)
    mi355x.setattr(engine, "DATAFLOW", 1)
    assert _route(100, 300).Hp == 320 and _route(100, 300).kind == "dataflow"
    mi355x.setattr(engine, "DF_WIDE", 0)
    assert _route(100, 300).Hp == 512 and _route(100, 300).kind == "tiles"
    assert route.width(300, 1, 2, True, 0, True) == (320, False) and route.dataflow_only(DEV, 2, 2, 320, 8, 100) == 0
