"""Which recurrence path a pass takes, recorded from the outside: small models and batches run one evaluation pass (and,
where the case says so, one training step) under spies on the launch, packing and schedule entry points, and the calls
they saw are written as JSON with sorted keys.  Run it on two commits: equal files mean that no decision moved.

    python scripts/route_cases.py OUT.json

Only names both commits have are used; flags are set with `setattr` on `engine`, as the tests do.  The record of the
parent of the commit that introduced `dagnn_amd/route.py` is `tests/golden/route_cases.json`, which
`tests/test_route_cpu.py` replays without a GPU."""
import inspect
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dagnn_amd import DAGNN, DAGNN_BN, DAGNN_NA, ASTNodeEncoder, GraphData, autograd, core, dvae, engine, model, synth, variants  # noqa: E402
from dagnn_amd.dag_utils import add_order_info_01  # noqa: E402

MODULES = (engine, core, model, dvae, variants, autograd)
LOG = []      # the calls of the running pass
FACTS = {}    # what the pass's plans said


def _plan_facts(plan):
    if plan is not None and hasattr(plan, "N"):
        FACTS.update(N=plan.N, E=plan.E, B=plan.B, R=plan.R)


def _ints(v):
    return None if v is None else [int(x) for x in v]


def _df_key(groups):
    return (int(groups), engine.DF_COST_LAYER, engine.DF_COST_ROW)


def _cells_missing(cells, name):
    return sum(1 for c in cells if getattr(c, name, None) is None)


def _before(name, a):
    """What a call was given (`a`: its bound arguments)."""
    rec = {"fn": name}
    _plan_facts(a.get("plan"))
    for k in ("H", "Hp", "groups", "training", "transposed_too", "force", "launch", "num_nodes"):
        if k in a and a[k] is not None:
            rec[k] = int(a[k])
    for k in ("first_layer", "stop_layer"):
        if k in a:
            rec[k] = _ints(a[k])
    if "static_score" in a:
        rec["static_score"] = int(a["static_score"] is not None)
    if name in ("pack_dataflow", "pack_lockstep"):
        cells = list(a["cells"])
        rec.update(cells=len(cells), Hp=cells[0].Hp if cells else 0, df_ok=int(bool(cells and cells[0].df_ok)))
        if name == "pack_dataflow":   # (cells still without the forward / the transposed layout)
            rec["todo"] = [_cells_missing(cells, n) for n in ("w_hh_df", "w_hh_bt")]
    if name in ("pack_dataflow_batch", "pack_batch"):
        rec.update(mats=len(a["mats"]), gains=len(a.get("gains", ())))
    if name == "dataflow_args":
        rec["schedule_cached"] = int(_df_key(a["groups"]) in a["plan"].__dict__.get("_df", {}))
    if name in ("dataflow_schedule", "launch_prepare"):
        _plan_facts(a["self"])
        rec["built"] = int(_df_key(a["groups"]) not in a["self"].__dict__.get("_df", {}))   # (`_after`: and there afterwards)
        if name == "launch_prepare":
            rec.update(enc=int(a["enc"] is not None), stack=int(a["stack"] is not None))
    return rec


def _after(name, a, rec, out):
    if name in ("dataflow_run", "bwd_dataflow_sweep"):
        p = a.get("record")   # (`engine.PassRecord`, read after the call: the forward launch has filled it)
        rec["preact"] = None if p is None else int(p.handover() == "stat")   # (None: no pre-activations kept; 1: static rows)
    if name in ("dataflow_schedule", "launch_prepare"):
        rec["built"] = int(a["groups"] > 0 and rec["built"] and _df_key(a["groups"]) in a["self"].__dict__.get("_df", {}))
    if name == "tiles_launches":
        rec["out"] = int(out)
    if name == "tiles_batch_too_flat":
        rec["out"] = int(out)
    if name == "tiles_tail_split":
        rec["out"] = _ints(out)
    if name == "read_schedule":
        rec["rows"] = [np.diff(s.astype(np.int64)).tolist() for s in out]


def _spy(owner, name):
    orig = getattr(owner, name)
    sig = inspect.signature(orig)

    def wrapper(*args, **kw):
        bound = sig.bind(*args, **kw)
        bound.apply_defaults()
        a = bound.arguments
        rec = _before(name, a)
        LOG.append(rec)
        out = orig(*args, **kw)
        _after(name, a, rec, out)
        return out

    wrapper.__wrapped__ = orig
    return wrapper


def install_spies():
    for name in ("dataflow_run", "dataflow_args", "tiles_run", "frontier_run", "recurrence_layer", "bwd_dataflow_sweep",
                 "backward_sweep", "pack_dataflow_batch", "pack_batch", "tiles_launches", "tiles_batch_too_flat", "tiles_tail_split"):
        setattr(engine, name, _spy(engine, name))
    for name in ("dataflow_schedule", "launch_prepare", "read_schedule"):
        setattr(engine.PlanHandle, name, _spy(engine.PlanHandle, name))
    for name in ("pack_dataflow", "pack_lockstep"):
        orig, w = getattr(core, name), _spy(core, name)
        for m in MODULES:   # (modules that imported the name hold their own reference)
            if getattr(m, name, None) is orig:
                setattr(m, name, w)


# ----------------------------------------------------------------------------- cases
def _chain(n):
    ei = torch.tensor([(i, i + 1) for i in range(n - 1)], dtype=torch.long).t().reshape(2, -1)
    d = GraphData(x=torch.stack([torch.arange(n) % 98, torch.arange(n) % 300], 1), node_depth=(torch.arange(n) % 20).view(-1, 1),
                  edge_index=ei, edge_attr=torch.zeros(ei.shape[1], 2))
    add_order_info_01(d)
    return d


def code2_case(name, H, L=2, bidir=True, wea=True, agg="attn_h", B=4, train=False, flags=None, deep=False):
    return dict(name=name, kind="code2", H=H, L=L, bidirectional=bidir, w_edge_attr=wea, agg=agg, B=B, train=train,
                flags=flags or {}, deep=deep)


def dvae_case(name, kind, hs, fused=1, train=False, B=5, L=2):
    return dict(name=name, kind=kind, H=hs, L=L, bidirectional=kind == "bn", agg="attn_h", B=B, train=train, flags={},
                encode_fused=fused)


def all_cases():
    out = []
    for k, H in enumerate((64, 200, 256, 300, 320, 384, 501, 512)):
        for L in (1, 2):
            out.append(code2_case("code2_h%d_L%d" % (H, L), H, L, B=3 + (k + L) % 6))
    for H, L in ((64, 2), (256, 1), (300, 2), (320, 1), (384, 2), (512, 2), (512, 1)):
        out.append(code2_case("code2_h%d_L%d_train" % (H, L), H, L, train=True))
    for H, train in ((64, True), (300, False), (512, False), (256, False)):
        out.append(code2_case("code2_h%d_one_direction" % H, H, bidir=False, train=train))
    for H, L in ((64, 2), (300, 1), (300, 2), (320, 1), (512, 2)):
        out.append(code2_case("code2_h%d_L%d_no_edge_attr" % (H, L), H, L, wea=False, train=H == 64))
    for agg, H, L in (("attn_x", 64, 2), ("attn_x", 300, 1), ("attn_x", 300, 2), ("attn_x", 512, 2), ("self_attn_h", 64, 2),
                      ("self_attn_h", 200, 1), ("self_attn_h", 320, 2)):
        out.append(code2_case("code2_%s_h%d_L%d" % (agg, H, L), H, L, agg=agg, train=H == 64))
    for agg in ("add", "max"):
        for H in (64, 300):
            out.append(code2_case("code2_%s_h%d" % (agg, H), H, agg=agg))
    out += [code2_case("code2_h256_L5", 256, 5), code2_case("code2_h512_L5", 512, 5), code2_case("code2_h256_L5_train", 256, 5, train=True),
            code2_case("code2_h64_L7_26_cells", 64, 7)]
    for kind in ("na", "bn"):
        for hs in (64, 501):
            out += [dvae_case("%s_hs%d_fused" % (kind, hs), kind, hs, 1), dvae_case("%s_hs%d_steps" % (kind, hs), kind, hs, 0),
                    dvae_case("%s_hs%d_train" % (kind, hs), kind, hs, 1, train=True)]
    f = lambda name, H, flags, **kw: code2_case("flag_%s" % name, H, flags=flags, **kw)   # noqa: E731
    out += [f("dataflow0", 64, {"DATAFLOW": 0}), f("dataflow0_train", 64, {"DATAFLOW": 0}, train=True),
            f("df_wide0", 300, {"DF_WIDE": 0}), f("df_wide0_train", 300, {"DF_WIDE": 0}, train=True),
            f("tiles0", 512, {"TILES": 0}), f("tiles0_h300", 300, {"TILES": 0, "DF_WIDE": 0}),
            f("tiles2", 512, {"TILES": 2}), f("tiles2_L1", 512, {"TILES": 2}, L=1),
            f("tiles_max_nodes_split", 512, {"TILES_MAX_NODES": 10, "TILES_TAIL_ROWS": 2}, deep=True),
            f("tiles_max_nodes_split_L5", 512, {"TILES_MAX_NODES": 10, "TILES_TAIL_ROWS": 2}, deep=True, L=5),
            f("tiles_max_nodes_flat", 512, {"TILES_MAX_NODES": 10}),
            f("reserved_cus64_train", 64, {"RESERVED_CUS": 64}, train=True), f("reserved_cus64", 64, {"RESERVED_CUS": 64}),
            f("stat_fwd0_train", 64, {"STAT_FWD": 0}, train=True), f("stat_fwd0_h300_train", 300, {"STAT_FWD": 0}, train=True),
            f("bwd_dataflow0_train", 64, {"BWD_DATAFLOW": 0}, train=True), f("bwd_dataflow0_h256_train", 256, {"BWD_DATAFLOW": 0}, train=True),
            f("bwd_df_max_bytes0_train", 64, {"BWD_DF_MAX_BYTES": 0}, train=True),
            f("bwd_df_max_bytes0_h300_train", 300, {"BWD_DF_MAX_BYTES": 0}, train=True)]
    assert len({c["name"] for c in out}) == len(out)
    return out


def build(case, seed):
    torch.manual_seed(seed)
    H, L, B = case["H"], case["L"], case["B"]
    if case["kind"] == "code2":
        m = DAGNN(num_vocab=8, max_seq_len=2, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(H, 98, 10030, 20),
                  w_edge_attr=case["w_edge_attr"], num_layers=L, bidirectional=case["bidirectional"], agg=case["agg"], out_wx=False,
                  out_pool_all=False, out_pool="max", dropout=0.0)
        # (`deep`: shallow graphs and one chain, a batch whose last 32 layers and more are one row wide)
        graphs = synth.code2_graphs(seed, B - 1, 8, 12) + [_chain(48)] if case["deep"] else synth.code2_graphs(seed, B, 20, 40)
        return m, synth.GraphBatch.from_data_list(graphs)
    cls, nn_, rows, dec = (DAGNN_NA, 8, synth.enas_rows, synth.decode_enas_row) if case["kind"] == "na" else \
        (DAGNN_BN, 10, synth.bn_rows, synth.decode_bn_row)
    m = cls(nn_, H, H, nn_, nn_, 0, 1, hs=H, nz=56, num_nodes=nn_, num_layers=L, bidirectional=case["bidirectional"])
    return m, synth.dvae_batch([dec(r) for r in rows(seed, B)])


def run_pass(case, m, G, dev, train):
    del LOG[:]
    FACTS.clear()
    core._OFF_DATAFLOW_SEEN.clear()
    G = G.clone().to(dev)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        if train:
            m.train()
            m.zero_grad(set_to_none=True)
            out = m(G)
            loss = out.square().mean() if torch.is_tensor(out) else sum(p.square().mean() for p in out)
            loss.backward()
        else:
            m.eval()
            with torch.no_grad():
                m(G)
    torch.cuda.synchronize()
    m.check()
    calls = list(LOG)
    return {"calls": calls, "facts": dict(FACTS),
            "schedule_builds": [c["groups"] for c in calls if c.get("built")],
            "warnings": sorted(str(w.message) for w in seen if issubclass(w.category, RuntimeWarning))}


def main():
    dev = torch.device("cuda:0")
    install_spies()
    device = {"cus": int(engine._num_cus(dev)), "total_memory": int(engine._total_memory(dev))}
    cases = []
    for seed, case in enumerate(all_cases()):
        saved = {k: getattr(engine, k) for k in case["flags"]}
        fused = dvae.ENCODE_FUSED
        try:
            for k, v in case["flags"].items():
                setattr(engine, k, v)
            dvae.ENCODE_FUSED = case.get("encode_fused", fused)
            m, G = build(case, seed)
            m = m.to(dev)
            rec = dict(case, passes={"eval": run_pass(case, m, G, dev, False)})
            if case["train"]:
                rec["passes"]["train"] = run_pass(case, m, G, dev, True)
        finally:
            for k, v in saved.items():
                setattr(engine, k, v)
            dvae.ENCODE_FUSED = fused
        cases.append(rec)
        print(case["name"], [c["fn"] for p in rec["passes"].values() for c in p["calls"]
                             if c["fn"] in ("dataflow_run", "dataflow_args", "tiles_run", "frontier_run", "bwd_dataflow_sweep", "backward_sweep")],
              flush=True)
    text = '{"cases":[\n' + ",\n".join(json.dumps(c, sort_keys=True, separators=(",", ":")) for c in cases) + \
        '\n],\n"device":' + json.dumps(device, sort_keys=True, separators=(",", ":")) + "}\n"
    with open(sys.argv[1], "w") as f:
        f.write(text)
    print("%d cases, %d bytes" % (len(cases), len(text)))


if __name__ == "__main__":
    main()
