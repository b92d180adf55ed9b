#!/usr/bin/env python
"""Generate the attention fixtures: what the REAL reference's conv modules hand to and get from `softmax` in every conv call
of a forward pass, scattered to original edge ids.

Runs only in the build container (needs the reference).  The reference runs unmodified in eval() mode; the name `softmax`
of each reference module (the function `AttnConv.message` / `SelfAttnConv.message` call, ogbg-code/model/dagnn.py:308,371,
dvae/dagnn.py:337,379, dvae/dagnn_bn.py:331,373) is wrapped at run time to record its first argument (the pre-softmax
score, query part and bias included) and its result.  `forward` makes one conv call per (direction, topological layer >= 1,
stacked layer), in that order, on `edge_index[:, le_idx]`; `le_idx` is recomputed here exactly as `forward` builds it
(dagnn.py:152-156), which gives every recorded row its edge id.  Every edge lies in exactly one frontier per direction, so
`alpha` / `logit` [D, L, E] are filled completely (asserted).

Each fixture holds the inputs, the state dict ("sd::<name>"), `alpha` and `logit`.

    python tests/golden/make_golden_attention.py
"""
from __future__ import annotations

import importlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _load_file, _np, _save, _setup_paths  # noqa: E402
from oracle.seeding import seeded_fill  # noqa: E402
from dagnn_amd import synth  # noqa: E402


class _Recorder(object):
    """Wraps `mod.softmax`: keeps (score, weight) of every call, in call order."""

    def __init__(self, mod):
        self.mod, self.orig, self.calls = mod, mod.softmax, []

    def __enter__(self):
        def wrapped(src, *args, **kw):
            out = self.orig(src, *args, **kw)
            self.calls.append((src.detach().reshape(-1).clone(), out.detach().reshape(-1).clone()))
            return out
        self.mod.softmax = wrapped
        return self

    def __exit__(self, *exc):
        self.mod.softmax = self.orig
        return False


def _scatter(calls, edge_index, layer_index, dirs, L):
    """`alpha`, `logit` [D, L, E] from the recorded calls: the loop nest of `forward` (dagnn.py:144-182) without the cells."""
    E = edge_index.shape[1]
    alpha = torch.full((len(dirs), L, E), float("nan"))
    logit = torch.full((len(dirs), L, E), float("nan"))
    it = iter(calls)
    for q, d in enumerate(dirs):
        T = int(layer_index[d][0].max()) + 1
        for l_idx in range(1, T):
            layer = layer_index[d][1][layer_index[d][0] == l_idx]
            le_idx = torch.cat([(edge_index[1 - d] == n).nonzero().squeeze(-1) for n in layer], dim=-1)
            for i in range(L):
                score, weight = next(it)
                assert score.numel() == le_idx.numel(), (d, l_idx, i, score.numel(), le_idx.numel())
                assert bool(torch.isnan(alpha[q, i, le_idx]).all()), "an edge in two frontiers"
                alpha[q, i, le_idx], logit[q, i, le_idx] = weight, score
    assert next(it, None) is None, "more conv calls than (direction, layer, stacked layer) cells"
    assert not bool(torch.isnan(alpha).any()) and not bool(torch.isnan(logit).any()), "an edge no conv call saw"
    return alpha, logit


ENCODER_KEYS = ("node_aggr_", "grue_", "hg_unify", "out_linear", "fc1", "fc2")


def _state(model, only=None):
    """The state dict as arrays "sd::<name>"; `only`: name prefixes to keep (the D-VAE models: the encoder's entries - the
    decoder's take no part in `forward` and would be ~1 MB; `cells_<d>` are aliases of `grue_*`.  The rest of the model is
    `seeded_fill(model, w_seed)` on both sides)."""
    return {"sd::" + k: _np(v) for k, v in model.state_dict().items() if only is None or k.startswith(only)}


def make_code2(ref_dagnn, ref_utils, ref_dagutils, name, *, data_seed, B, mean_n, H, L, bidir, w_seed, V=8, S=2, n_attr=30, **ctor):
    graphs = synth.code2_graphs(data_seed, B, mean_n, 1000)
    for g in graphs:
        g.x[:, 1] %= n_attr
        ns = SimpleNamespace(edge_index=g.edge_index, num_nodes=g.num_nodes)
        ref_dagutils.add_order_info_01(ns)
        for k in ("_bi_layer_idx0", "_bi_layer_index0", "_bi_layer_idx1", "_bi_layer_index1"):
            setattr(g, k, getattr(ns, k))
    b = synth.GraphBatch.from_data_list(graphs)
    enc = ref_utils.ASTNodeEncoder(H, 98, n_attr, 20)
    kw = dict(w_edge_attr=True, num_layers=L, bidirectional=bidir, agg="attn_h", out_wx=False, out_pool_all=False, out_pool="max",
              dropout=0.0)
    kw.update(ctor)
    model = ref_dagnn.DAGNN(num_vocab=V, max_seq_len=S, emb_dim=H, hidden_dim=H, out_dim=None, encoder=enc, **kw).eval()
    seeded_fill(model, w_seed)
    G = SimpleNamespace(x=b.x.clone(), node_depth=b.node_depth.clone(), edge_index=b.edge_index.clone(),
                        edge_attr=b.edge_attr.clone(), batch=b.batch.clone(),
                        _bi_layer_idx0=b._bi_layer_idx0.clone(), _bi_layer_index0=b._bi_layer_index0.clone(),
                        _bi_layer_idx1=b._bi_layer_idx1.clone(), _bi_layer_index1=b._bi_layer_index1.clone())
    with torch.no_grad(), _Recorder(ref_dagnn) as rec:
        out = model(G)
    alpha, logit = _scatter(rec.calls, b.edge_index, G.bi_layer_index, model.dirs, L)
    meta = dict(kind="code2", data_seed=data_seed, B=B, mean_n=mean_n, H=H, L=L, bidir=bool(bidir), V=V, S=S, n_attr=n_attr,
                w_seed=w_seed, ctor=kw, N=int(b.x.shape[0]), E=int(b.edge_index.shape[1]),
                state_dict={k: list(v.shape) for k, v in model.state_dict().items()})
    _save(name, meta, x=_np(b.x), node_depth=_np(b.node_depth), edge_index=_np(b.edge_index), edge_attr=_np(b.edge_attr),
          batch=_np(b.batch), layer0=_np(b._bi_layer_idx0), layer1=_np(b._bi_layer_idx1), pred=np.stack([_np(o) for o in out]),
          alpha=_np(alpha), logit=_np(logit), **_state(model))


def make_dvae(ref_mod, cls_name, ref_util, ref_batch_mod, name, *, kind, rows, hs, L, bidir, agg, w_seed):
    nvt = 8 if kind == "na" else 10
    decode = ref_util.decode_ENAS_to_pygraph if kind == "na" else ref_util.decode_BN_to_pygraph
    graphs = [decode(r)[0] for r in rows]
    model = getattr(ref_mod, cls_name)(nvt, hs, hs, nvt, nvt, 0, 1, hs=hs, nz=56, num_nodes=nvt, agg=agg, num_layers=L,
                                       bidirectional=bidir, out_wx=False, out_pool_all=False, out_pool="max", dropout=0.0).eval()
    seeded_fill(model, w_seed)
    b = ref_batch_mod.Batch.from_data_list(graphs)
    edge_index, layer_index, batch = b.edge_index.clone(), b.bi_layer_index.clone(), b.batch.clone()
    with torch.no_grad(), _Recorder(ref_mod) as rec:
        Hg = model(b)
    alpha, logit = _scatter(rec.calls, edge_index, layer_index, model.dirs, L)
    meta = dict(kind=kind, hs=hs, L=L, bidir=bool(bidir), agg=agg, w_seed=w_seed, nrows=len(rows),
                state_dict={k: list(v.shape) for k, v in model.state_dict().items()})
    _save(name, meta, rows=np.array([json.dumps(r) for r in rows]), x=_np(b.x), edge_index=_np(edge_index),
          bi_layer_index=_np(layer_index), batch=_np(batch), Hg=_np(Hg), alpha=_np(alpha), logit=_np(logit), **_state(model, ENCODER_KEYS))


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not found at %s - fixtures can only be regenerated in the build container" % REF)
    _setup_paths()
    torch.manual_seed(0)
    ref_dagutils = importlib.import_module("src.utils_dag")
    ref_dagnn = _load_file("ref_ogbg_dagnn", os.path.join(REF, "ogbg-code", "model", "dagnn.py"))
    ref_utils = _load_file("ref_ogbg_utils", os.path.join(REF, "ogbg-code", "utils.py"))
    # 1. code2 attn_h: h = 32, L = 2, bidirectional, with the edge encoder
    make_code2(ref_dagnn, ref_utils, ref_dagutils, "attention_code2_h32", data_seed=71, B=4, mean_n=25, H=32, L=2, bidir=1, w_seed=701)
    ref_util = importlib.import_module("util")
    ref_batch_mod = importlib.import_module("batch")
    ref_na = importlib.import_module("dagnn")
    ref_bn = importlib.import_module("dagnn_bn")
    # 2. NA attn_h: h = 64, unidirectional, 8 nodes (the one-hot vertex-id columns in keys and queries)
    rows = []
    with open(os.path.join(REF, "dvae", "data", "final_structures6.txt")) as f:
        for i, line in enumerate(f):
            if i >= 1000:   # burn_in of load_ENAS_graphs (dvae/util.py:67)
                rows.append(eval(line)[0])
            if len(rows) == 6:
                break
    make_dvae(ref_na, "DAGNN", ref_util, ref_batch_mod, "attention_na_h64", kind="na", rows=rows, hs=64, L=2, bidir=False,
              agg="attn_h", w_seed=702)
    # 2b. NA self_attn_h: h = 32, bidirectional (`SelfAttnConv`: no query half; the vertex-id columns behind the keys)
    make_dvae(ref_na, "DAGNN", ref_util, ref_batch_mod, "attention_na_h32_self_attn_h", kind="na", rows=rows, hs=32, L=2, bidir=True,
              agg="self_attn_h", w_seed=704)
    # 3. BN attn_x: h = 64, bidirectional (keys and queries are the node inputs)
    make_dvae(ref_bn, "DAGNN_BN", ref_util, ref_batch_mod, "attention_bn_h64_attn_x", kind="bn", rows=synth.bn_rows(73, 6), hs=64,
              L=2, bidir=True, agg="attn_x", w_seed=703)


if __name__ == "__main__":
    main()
