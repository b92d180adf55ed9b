#!/usr/bin/env python
"""Generate the fixtures of the ogbg-code2 evaluation path (`code2_eval_*.npz`, `code2_f1_*.npz`) from the REAL reference.

Runs only where the reference is present.  Same pattern as `make_golden.py`: the reference's files are imported unmodified
(`ogbg-code/model/dagnn.py`, `ogbg-code/utils.py`, `ogb/graphproppred/evaluate.py`), weights come from
`oracle.seeding.seeded_fill` and are never stored, only data goes into this directory.

    python tests/golden/make_golden_code2_eval.py

Model fixtures: the batch, the token matrix of the reference's own `argmax` + `cat` (ogbg-code/main_pyg.py:106-109), its three
largest logits and their columns per (graph, head), and the bias boosts.  With seeded random weights the reference never
predicts `__EOS__`, so after `seeded_fill` each head's bias at the EOS column (V - 1) is raised by the median over graphs of
(top-1 logit - EOS logit) of that head - about half of its rows then end in EOS - and head 0's bias at the `__UNK__` column
(V - 2) by the 90th percentile likewise.  The tests apply the stored boosts to their own model.  Winners are stored, not
logits (a [5, 128, 5002] fp32 tensor is 12.8 MB).

Metric fixtures, independent of any model: a vocabulary from the reference's `get_vocab_mapping` on a seeded synthetic
corpus, token matrices and label lists built to hit every branch (EOS at every position and absent, repeated ids, `__UNK__`;
labels with repeated words, words outside the vocabulary, more than S words, empty lists, the literals `__UNK__` and
`__EOS__`), and what the reference's `decode_arr_to_seq` and `Evaluator._eval_F1` make of them.
"""
from __future__ import annotations

import contextlib
import io
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

TAU = 2e-4          # two logits that each move by the 1e-4 parity bound can swap if they are this close
MAX_AMBIGUOUS = 0.02


def _words(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


# ------------------------------------------------------------------------------- model fixtures
def make_eval(ref_dagnn, ref_utils, ref_dagutils, name, *, data_seed, B, mean_n, H, L, bidir, V, S, n_attr, w_seed, max_n=1000,
              num_class=0, **ctor):
    graphs = synth.code2_graphs(data_seed, B, mean_n, max_n)
    for g in graphs:
        g.x[:, 1] %= n_attr
        ns = SimpleNamespace(edge_index=g.edge_index, num_nodes=g.num_nodes)
        ref_dagutils.add_order_info_01(ns)
        for k in ("_bi_layer_idx0", "_bi_layer_index0", "_bi_layer_idx1", "_bi_layer_index1"):
            setattr(g, k, getattr(ns, k))
    b = synth.GraphBatch.from_data_list(graphs)
    enc = ref_utils.ASTNodeEncoder(H, 98, n_attr, 20)
    kw = dict(w_edge_attr=True, num_layers=L, bidirectional=bidir, agg="attn_h", out_wx=False, out_pool_all=False,
              out_pool="max", dropout=0.0)
    kw.update(ctor)
    if num_class:
        kw["num_class"] = num_class
    model = ref_dagnn.DAGNN(num_vocab=V, max_seq_len=S, emb_dim=H, hidden_dim=H, out_dim=None, encoder=enc, **kw).eval()
    seeded_fill(model, w_seed)

    def run():
        G = SimpleNamespace(x=b.x.clone(), node_depth=b.node_depth.clone(), edge_index=b.edge_index.clone(),
                            edge_attr=b.edge_attr.clone(), batch=b.batch.clone(),
                            _bi_layer_idx0=b._bi_layer_idx0.clone(), _bi_layer_index0=b._bi_layer_index0.clone(),
                            _bi_layer_idx1=b._bi_layer_idx1.clone(), _bi_layer_index1=b._bi_layer_index1.clone())
        with torch.no_grad():
            out = model(G)
        return list(out) if isinstance(out, (list, tuple)) else [out]

    heads = len(run())
    boost_eos = np.zeros(heads, dtype=np.float32)
    boost_unk = np.zeros(1, dtype=np.float32)
    if not num_class:
        pred = run()
        for s, p in enumerate(pred):
            boost_eos[s] = np.float32(np.median(_np(p.max(dim=1).values - p[:, V - 1])))
        boost_unk[0] = np.float32(np.percentile(_np(pred[0].max(dim=1).values - pred[0][:, V - 2]), 90))
        with torch.no_grad():
            for s, hd in enumerate(model.graph_pred_linear_list):
                hd.bias[V - 1] += torch.tensor(boost_eos[s])
            model.graph_pred_linear_list[0].bias[V - 2] += torch.tensor(boost_unk[0])
    pred_list = run()
    # ogbg-code/main_pyg.py:106-109, verbatim in effect
    mat = []
    for i in range(len(pred_list)):
        mat.append(torch.argmax(pred_list[i], dim=1).view(-1, 1))
    mat = torch.cat(mat, dim=1)
    width = pred_list[0].shape[1]
    k = min(3, width)
    top = [torch.topk(p, k, dim=1) for p in pred_list]
    top_val = torch.stack([t.values for t in top], dim=1)     # [B, S, 3]
    top_col = torch.stack([t.indices for t in top], dim=1)
    margin = _np(top_val[:, :, 0] - top_val[:, :, 1])
    ambiguous = float((margin <= TAU).mean())
    third = float(_np(top_val[:, :, 0] - top_val[:, :, 2]).min())
    eos_share = float((_np(mat) == V - 1).mean()) if not num_class else None
    print("%-26s ambiguous %.4f  min(top1 - top3) %.3e  EOS share %s" % (name, ambiguous, third, eos_share))
    assert ambiguous <= MAX_AMBIGUOUS, (name, ambiguous)
    assert third > TAU, (name, third)
    if not num_class:
        assert 0.10 <= eos_share <= 0.60, (name, eos_share)
    meta = dict(kind="code2_eval", data_seed=data_seed, B=B, mean_n=mean_n, max_n=max_n, H=H, L=L, bidir=bool(bidir), V=V, S=S,
                n_attr=n_attr, w_seed=w_seed, ctor=kw, N=int(b.x.shape[0]), E=int(b.edge_index.shape[1]), heads=heads,
                width=int(width), tau=TAU, ambiguous=ambiguous, eos_share=eos_share,
                state_dict={k_: list(v.shape) for k_, v in model.state_dict().items()})
    _save(name, meta, x=_np(b.x), node_depth=_np(b.node_depth), edge_index=_np(b.edge_index), edge_attr=_np(b.edge_attr),
          batch=_np(b.batch), layer0=_np(b._bi_layer_idx0), layer1=_np(b._bi_layer_idx1), tok=_np(mat),
          top_val=_np(top_val), top_col=_np(top_col), boost_eos=boost_eos, boost_unk=boost_unk)


# ------------------------------------------------------------------------------- metric fixtures
def make_f1(ref_utils, ref_eval, name, *, seed, B, S, num_vocab, splits):
    rng = np.random.default_rng(seed)
    pool = ["w%03d" % i for i in range(3 * num_vocab)]
    zipf = 1.0 / np.arange(1, len(pool) + 1)
    zipf /= zipf.sum()
    corpus = [[pool[i] for i in rng.choice(len(pool), size=int(rng.integers(1, 8)), p=zipf)] for _ in range(2000)]
    with contextlib.redirect_stdout(io.StringIO()):
        vocab2idx, idx2vocab = ref_utils.get_vocab_mapping(corpus, num_vocab)
    V = len(idx2vocab)
    unk, eos = vocab2idx["__UNK__"], vocab2idx["__EOS__"]
    assert (unk, eos) == (V - 2, V - 1)

    tok = rng.integers(0, V - 2, size=(B, S))
    seq_ref = []
    for b in range(B):
        case = (b + seed) % 12
        if case < S + 1:
            tok[b, case:case + 1] = eos                      # EOS at every position 0 .. S-1; case == S: absent
        if case == 6:
            tok[b, :] = tok[b, 0]                            # one id repeated
        if case == 7:
            tok[b, 1] = tok[b, 0]
            tok[b, S - 1] = eos
        if case == 8:
            tok[b, 0] = unk
        if case == 9:
            tok[b, 0], tok[b, 1] = eos, eos                  # two EOS: the first one cuts
        if case == 10:
            tok[b, rng.integers(0, S)] = unk
        # labels: mostly words the row predicts (so that true positives occur), plus the special cases
        n_lab = int(rng.integers(0, S + 4))
        lab = []
        for _ in range(n_lab):
            u = rng.random()
            if u < 0.45:
                lab.append(idx2vocab[int(tok[b, rng.integers(0, S)])])      # (may be the literal __EOS__ / __UNK__)
            elif u < 0.75:
                lab.append(pool[int(rng.choice(len(pool), p=zipf))])         # in or out of the vocabulary
            elif u < 0.85:
                lab.append("rare_%d" % int(rng.integers(0, 5)))              # never in the vocabulary
            elif u < 0.92 and lab:
                lab.append(lab[int(rng.integers(0, len(lab)))])              # a repeated word
            elif u < 0.96:
                lab.append("__UNK__")
            else:
                lab.append("__EOS__")
        if (b + 1) % 41 == 0:
            lab = []
        seq_ref.append(lab)
    tok_t = torch.from_numpy(tok)
    # ogbg-code/main_pyg.py:111, ogb/graphproppred/evaluate.py:231-267
    seq_pred = [ref_utils.decode_arr_to_seq(arr, idx2vocab) for arr in tok_t]
    res = ref_eval.Evaluator._eval_F1(None, seq_ref, seq_pred)
    tpfpfn = np.zeros((B, 3), dtype=np.int64)
    for b, (l, p) in enumerate(zip(seq_ref, seq_pred)):
        label, prediction = set(l), set(p)
        tpfpfn[b] = (len(label & prediction), len(prediction - label), len(label - prediction))
        one = ref_eval.Evaluator._eval_F1(None, [l], [p])    # the per-graph counts reproduce the evaluator's own numbers
        tp, fp, fn = (int(v) for v in tpfpfn[b])
        assert one["precision"] == (tp / (tp + fp) if tp + fp else 0) and one["recall"] == (tp / (tp + fn) if tp + fn else 0)
    assert sum(splits) == B
    meta = dict(kind="code2_f1", seed=seed, B=B, S=S, V=V, num_vocab=num_vocab, splits=list(splits), unk=unk, eos=eos)
    _save(name, meta, tok=tok, idx2vocab=_words(idx2vocab), seq_ref=_words(seq_ref), seq_pred=_words(seq_pred), tpfpfn=tpfpfn,
          f1=np.array([res["precision"], res["recall"], res["F1"]], dtype=np.float64))
    print("%-26s precision %.6f recall %.6f F1 %.6f" % (name, res["precision"], res["recall"], res["F1"]))


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not found at %s - fixtures can only be regenerated where it is present" % REF)
    _setup_paths()
    torch.manual_seed(0)
    import importlib
    ref_dagutils = importlib.import_module("src.utils_dag")
    ref_dagnn = _load_file("ref_ogbg_dagnn", os.path.join(REF, "ogbg-code", "model", "dagnn.py"))
    ref_utils = _load_file("ref_ogbg_utils", os.path.join(REF, "ogbg-code", "utils.py"))
    ref_eval = _load_file("ref_ogb_evaluate", os.path.join(REF, "ogb", "graphproppred", "evaluate.py"))

    code2 = dict(V=5002, S=5, n_attr=300)
    make_eval(ref_dagnn, ref_utils, ref_dagutils, "code2_eval_b64_h64", data_seed=61, B=64, mean_n=30, H=64, L=2, bidir=1,
              w_seed=161, **code2)
    make_eval(ref_dagnn, ref_utils, ref_dagutils, "code2_eval_b128_h128", data_seed=62, B=128, mean_n=30, H=128, L=2, bidir=1,
              w_seed=162, **code2)
    make_eval(ref_dagnn, ref_utils, ref_dagutils, "code2_eval_unidir_wx", data_seed=63, B=48, mean_n=30, H=64, L=2, bidir=0,
              w_seed=163, out_wx=True, **code2)
    make_eval(ref_dagnn, ref_utils, ref_dagutils, "code2_eval_numclass", data_seed=64, B=64, mean_n=30, H=64, L=2, bidir=1,
              w_seed=174, num_class=17, **code2)
    make_eval(ref_dagnn, ref_utils, ref_dagutils, "code2_eval_gated_sum", data_seed=65, B=32, mean_n=25, H=64, L=2, bidir=1,
              w_seed=165, agg="gated_sum", **code2)
    make_f1(ref_utils, ref_eval, "code2_f1_b1", seed=71, B=1, S=5, num_vocab=50, splits=[1])
    make_f1(ref_utils, ref_eval, "code2_f1_b3000", seed=72, B=3000, S=5, num_vocab=200,
            splits=[128, 128, 1, 500, 77, 1024, 3, 640, 499])


if __name__ == "__main__":
    main()
