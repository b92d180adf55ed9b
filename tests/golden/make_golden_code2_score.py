#!/usr/bin/env python
"""Generate the fixtures of `DAGNN.score` (`code2_score_*.npz`) from the REAL reference.

Runs only where the reference is present.  The model recipes are those of three `code2_eval_*` fixtures
(`make_golden_code2_eval.py`: same data seeds, same weight seeds, the bias boosts THAT fixture stores), rebuilt here around the
reference's unmodified `ogbg-code/model/dagnn.py`; the reference's own arg-max must reproduce the token matrix that fixture
holds, or nothing is written.  The batch itself stays in the `code2_eval_*` file; this one adds, per (graph, head), from the
reference's own `model(G)` logits:

    lse      float64  log-sum-exp of the fp32 logits, in float64
    y        int64    seeded targets: every other entry the reference's own arg-max (small losses), the rest uniform in [0, V)
    nll      float64  -log_softmax at y, in float64
    top_val  float32  the 8 largest logits, descending          top_col  int32  their columns
    clear    bool     rank r is clear when its logit is more than TAU away from both neighbouring ranks (the 9th included)

Two logits that each move by the project's parity bound (1e-4) can swap if they are within TAU = 2e-4: a rank that is not clear
is ambiguous and a test may skip it.  At most MAX_AMBIGUOUS of a fixture's (graph, head, rank) slots may be.

    python tests/golden/make_golden_code2_score.py
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REPO, _load_file, _np, _save, _setup_paths  # noqa: E402
from make_golden_code2_eval import MAX_AMBIGUOUS, TAU  # noqa: E402
from oracle.seeding import seeded_fill  # noqa: E402
from dagnn_amd import synth  # noqa: E402

sys.path.insert(0, REPO)
from tests import helpers as Hh  # noqa: E402

K = 8


def make_score(ref_dagnn, ref_utils, ref_dagutils, source, name, y_seed):
    meta, arr = Hh.load(source)
    V, S, H, B = meta["V"], meta["S"], meta["H"], meta["B"]
    graphs = synth.code2_graphs(meta["data_seed"], B, meta["mean_n"], meta["max_n"])
    for g in graphs:
        g.x[:, 1] %= meta["n_attr"]
        ns = SimpleNamespace(edge_index=g.edge_index, num_nodes=g.num_nodes)
        ref_dagutils.add_order_info_01(ns)
        for k in ("_bi_layer_idx0", "_bi_layer_index0", "_bi_layer_idx1", "_bi_layer_index1"):
            setattr(g, k, getattr(ns, k))
    b = synth.GraphBatch.from_data_list(graphs)
    assert np.array_equal(_np(b.x), arr["x"]) and np.array_equal(_np(b.edge_index), arr["edge_index"])
    enc = ref_utils.ASTNodeEncoder(H, 98, meta["n_attr"], 20)
    model = ref_dagnn.DAGNN(num_vocab=V, max_seq_len=S, emb_dim=H, hidden_dim=H, out_dim=None, encoder=enc, **meta["ctor"]).eval()
    seeded_fill(model, meta["w_seed"])
    if meta["heads"] > 1:
        with torch.no_grad():
            for s, hd in enumerate(model.graph_pred_linear_list):
                hd.bias[V - 1] += torch.tensor(arr["boost_eos"][s])
            model.graph_pred_linear_list[0].bias[V - 2] += torch.tensor(arr["boost_unk"][0])
    G = SimpleNamespace(x=b.x.clone(), node_depth=b.node_depth.clone(), edge_index=b.edge_index.clone(),
                        edge_attr=b.edge_attr.clone(), batch=b.batch.clone(),
                        _bi_layer_idx0=b._bi_layer_idx0.clone(), _bi_layer_index0=b._bi_layer_index0.clone(),
                        _bi_layer_idx1=b._bi_layer_idx1.clone(), _bi_layer_index1=b._bi_layer_index1.clone())
    with torch.no_grad():
        out = model(G)
    pred = list(out) if isinstance(out, (list, tuple)) else [out]
    logits = torch.stack(pred, dim=1)                                    # [B, heads, width] fp32
    heads, width = logits.shape[1], logits.shape[2]
    argmax = torch.argmax(logits, dim=2)
    assert np.array_equal(_np(argmax), arr["tok"]), "the recipe does not reproduce %s" % source
    x64 = logits.double()
    lse = torch.logsumexp(x64, dim=2)
    rng = np.random.default_rng(y_seed)
    y = rng.integers(0, width, size=(B, heads))
    own = (np.arange(B * heads).reshape(B, heads) + y_seed) % 2 == 0
    y = np.where(own, _np(argmax), y).astype(np.int64)
    nll = -torch.log_softmax(x64, dim=2).gather(2, torch.from_numpy(y).unsqueeze(2)).squeeze(2)
    top = torch.topk(logits, min(K + 1, width), dim=2)
    val = _np(top.values).astype(np.float64)
    gap = val[:, :, :-1] - val[:, :, 1:]                                 # gap[r]: rank r to rank r + 1
    below = gap[:, :, :K]
    above = np.concatenate([np.full(gap.shape[:2] + (1,), np.inf), gap[:, :, :K - 1]], axis=2)
    clear = (below > TAU) & (above > TAU)
    ambiguous = float((~clear).mean())
    print("%-26s ambiguous %.4f  loss %.4f  min nll %.3e" % (name, ambiguous, float(nll.mean()), float(nll.min())))
    assert ambiguous <= MAX_AMBIGUOUS, (name, ambiguous)
    out_meta = dict(kind="code2_score", source=source, y_seed=y_seed, B=B, heads=heads, width=int(width), k=K, tau=TAU,
                    ambiguous=ambiguous)
    _save(name, out_meta, lse=_np(lse), y=y, nll=_np(nll), top_val=_np(top.values[:, :, :K]),
          top_col=_np(top.indices[:, :, :K]).astype(np.int32), clear=clear)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not found at %s - fixtures can only be regenerated where it is present" % REF)
    _setup_paths()
    torch.manual_seed(0)
    import importlib
    ref_dagutils = importlib.import_module("src.utils_dag")
    ref_dagnn = _load_file("ref_ogbg_dagnn", os.path.join(REF, "ogbg-code", "model", "dagnn.py"))
    ref_utils = _load_file("ref_ogbg_utils", os.path.join(REF, "ogbg-code", "utils.py"))
    make_score(ref_dagnn, ref_utils, ref_dagutils, "code2_eval_b64_h64", "code2_score_b64_h64", 81)
    make_score(ref_dagnn, ref_utils, ref_dagutils, "code2_eval_unidir_wx", "code2_score_unidir_wx", 82)
    make_score(ref_dagnn, ref_utils, ref_dagutils, "code2_eval_numclass", "code2_score_numclass", 83)


if __name__ == "__main__":
    main()
