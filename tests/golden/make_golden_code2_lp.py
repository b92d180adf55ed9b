#!/usr/bin/env python
"""Generate the fixtures of the ogbg-code2 LP task (`code2_lp_*.npz`) from the REAL reference.

Runs only where the reference is present.  Same pattern as `make_golden_code2_eval.py`: the reference's files are imported
unmodified (`ogbg-code/model/dagnn.py`, `ogbg-code/utils2.py`, `src/utils_dag.py`, `ogb/graphproppred/evaluate.py`), weights
come from `oracle.seeding.seeded_fill` and are never stored, only data goes into this directory.

    python tests/golden/make_golden_code2_lp.py

Model fixtures: one step of the reference's LP loop (ogbg-code/main_pyg_lp.py:43-74) on a seeded batch - the model with
`ASTNodeEncoder2` and one `num_class` head, `len_longest_path` per graph as the reference's reader computes it
(ogb/io/read_graph_pyg.py:51-54: the maximum of `_bi_layer_idx0`, a Python float per graph, a float32 tensor after
collation), `CrossEntropyLoss()(pred, targ.to(torch.long))`, `loss.backward()`, the argmax and `Evaluator._eval_acc` on it.
The data seed is chosen so that every target is below `num_class`, and so that no graph's two best logits are within TAU.

Metric fixture, independent of any model: 3000 (prediction, target) pairs in uneven batches with NaN targets, non-integer
float targets and one batch without a single hit, and `_eval_acc`'s number on all of them.
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _load_file, _np, _save, _setup_paths, sample_grad  # noqa: E402
from oracle.seeding import seeded_fill  # noqa: E402
from dagnn_amd import synth  # noqa: E402

TAU = 2e-4          # two logits that each move by the 1e-4 parity bound can swap if they are this close
MAX_AMBIGUOUS = 0.02
ROW_STRIDE = 4      # the embedding rows a fixture keeps


def make_lp(ref_dagnn, ref_utils2, ref_dagutils, ref_eval, name, *, data_seed, B, mean_n, H, L, bidir, agg, num_class, n_attr,
            w_seed, max_n=1000):
    graphs = synth.code2_graphs(data_seed, B, mean_n, max_n)
    llp = []
    for g in graphs:
        g.x[:, 1] %= n_attr
        ns = SimpleNamespace(edge_index=g.edge_index, num_nodes=g.num_nodes)
        ref_dagutils.add_order_info_01(ns)
        for k in ("_bi_layer_idx0", "_bi_layer_index0", "_bi_layer_idx1", "_bi_layer_index1"):
            setattr(g, k, getattr(ns, k))
        llp.append(float(torch.max(ns._bi_layer_idx0).item()))   # ogb/io/read_graph_pyg.py:54
    b = synth.GraphBatch.from_data_list(graphs)
    targ = torch.tensor(llp)   # (what PyG's collation makes of the per-graph floats)
    assert float(targ.max()) < num_class, (name, float(targ.max()), num_class)
    enc = ref_utils2.ASTNodeEncoder2(H, 98, n_attr, 20)
    # main_pyg_lp.py:140-148, 373-377: the LP script's constructor arguments
    kw = dict(w_edge_attr=0, num_layers=L, bidirectional=bidir, agg=agg, mapper_bias=True, out_wx=False, out_pool_all=0,
              out_pool="max", dropout=0.0, num_class=num_class)
    model = ref_dagnn.DAGNN(num_vocab=None, max_seq_len=None, emb_dim=H, hidden_dim=H, out_dim=None, encoder=enc, **kw).train()
    seeded_fill(model, w_seed)
    G = SimpleNamespace(x=b.x.clone(), node_depth=b.node_depth.clone(), edge_index=b.edge_index.clone(),
                        edge_attr=b.edge_attr.clone(), batch=b.batch.clone(),
                        _bi_layer_idx0=b._bi_layer_idx0.clone(), _bi_layer_index0=b._bi_layer_index0.clone(),
                        _bi_layer_idx1=b._bi_layer_idx1.clone(), _bi_layer_index1=b._bi_layer_index1.clone())
    pred = model(G)
    loss = torch.nn.CrossEntropyLoss()(pred, targ.to(torch.long))   # main_pyg_lp.py:40, 58
    loss.backward()
    tok = torch.argmax(pred.detach(), dim=1).view(-1, 1)             # main_pyg_lp.py:67
    acc = ref_eval.Evaluator._eval_acc(None, targ.view(-1, 1).numpy(), tok.numpy())["acc"]
    top = torch.topk(pred.detach(), min(3, num_class), dim=1)
    margin = _np(top.values[:, 0] - top.values[:, 1])
    ambiguous = float((margin <= TAU).mean())
    print("%-26s ambiguous %.4f  min margin %.3e  max target %d  acc %.4f  loss %.6f"
          % (name, ambiguous, float(margin.min()), int(targ.max()), acc, float(loss.detach())))
    assert ambiguous <= MAX_AMBIGUOUS, (name, ambiguous)
    N = b.x.shape[0]
    rows = np.arange(0, N, ROW_STRIDE)
    arrays = dict(x=_np(b.x), node_depth=_np(b.node_depth), edge_index=_np(b.edge_index), edge_attr=_np(b.edge_attr),
                  batch=_np(b.batch), layer0=_np(b._bi_layer_idx0), layer1=_np(b._bi_layer_idx1),
                  len_longest_path=_np(targ), pred=_np(pred), loss=np.array(float(loss.detach())), tok=_np(tok),
                  top_val=_np(top.values), top_col=_np(top.indices), acc=np.array(acc, dtype=np.float64),
                  rows=rows, x_emb=_np(G.x)[rows], node_depth_after=_np(G.node_depth))
    strides = {}
    for k, p_ in model.named_parameters():
        g = np.zeros(tuple(p_.shape), np.float32) if p_.grad is None else _np(p_.grad)
        arrays["g::" + k], strides[k], arrays["gsum::" + k] = sample_grad(k, g)
    meta = dict(kind="code2_lp", data_seed=data_seed, B=B, mean_n=mean_n, max_n=max_n, H=H, L=L, bidir=bool(bidir), agg=agg,
                num_class=num_class, n_attr=n_attr, w_seed=w_seed, ctor=kw, N=int(N), E=int(b.edge_index.shape[1]), tau=TAU,
                ambiguous=ambiguous, grad_stride=strides,
                state_dict={k_: list(v.shape) for k_, v in model.state_dict().items()})
    _save(name, meta, **arrays)


def make_acc(ref_eval, name, *, seed, n, num_class, splits):
    rng = np.random.default_rng(seed)
    assert sum(splits) == n
    targ = rng.integers(0, num_class, size=n).astype(np.float32)
    tok = np.where(rng.random(n) < 0.6, targ.astype(np.int64), rng.integers(0, num_class, size=n))
    targ[rng.random(n) < 0.05] = np.nan                      # unlabelled: in neither count
    frac = rng.random(n) < 0.05
    targ[frac] += np.float32(0.5)                            # 3.5 matches no class
    lo = sum(splits[:3])                                     # the fourth batch: not one hit
    sl = slice(lo, lo + splits[3])
    tok[sl] = (np.nan_to_num(targ[sl]).astype(np.int64) + 1) % num_class
    res = ref_eval.Evaluator._eval_acc(None, targ.reshape(-1, 1), tok.reshape(-1, 1))
    lab = targ == targ
    hits = int(np.sum(targ[lab] == tok[lab]))
    assert res["acc"] == float(hits) / int(lab.sum())
    assert int(np.sum(targ[sl][lab[sl]] == tok[sl][lab[sl]])) == 0
    meta = dict(kind="code2_lp_acc", seed=seed, n=n, num_class=num_class, splits=list(splits), hits=hits, labelled=int(lab.sum()))
    _save(name, meta, tok=tok.astype(np.int64), targ=targ, acc=np.array(res["acc"], dtype=np.float64))
    print("%-26s acc %.6f  (%d / %d, %d NaN, %d non-integer)" % (name, res["acc"], hits, int(lab.sum()), int((~lab).sum()),
                                                                int(frac.sum())))


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not found at %s - fixtures can only be regenerated where it is present" % REF)
    _setup_paths()
    torch.manual_seed(0)
    import importlib
    ref_dagutils = importlib.import_module("src.utils_dag")
    ref_dagnn = _load_file("ref_ogbg_dagnn", os.path.join(REF, "ogbg-code", "model", "dagnn.py"))
    ref_utils2 = _load_file("ref_ogbg_utils2", os.path.join(REF, "ogbg-code", "utils2.py"))
    ref_eval = _load_file("ref_ogb_evaluate", os.path.join(REF, "ogb", "graphproppred", "evaluate.py"))

    make_lp(ref_dagnn, ref_utils2, ref_dagutils, ref_eval, "code2_lp_gated_h64", data_seed=89, B=12, mean_n=30, H=64, L=1,
            bidir=0, agg="gated_sum", num_class=24, n_attr=300, w_seed=181)
    make_lp(ref_dagnn, ref_utils2, ref_dagutils, ref_eval, "code2_lp_attn_h32_bidir", data_seed=96, B=12, mean_n=30, H=32, L=2,
            bidir=1, agg="attn_h", num_class=24, n_attr=300, w_seed=182)
    make_acc(ref_eval, "code2_lp_acc", seed=91, n=3000, num_class=275, splits=[128, 1, 20, 257, 1025, 3, 640, 77, 849])


if __name__ == "__main__":
    main()
