#!/usr/bin/env python
"""Generate the fixtures of the ogbg-code2 training epoch (`code2_train_*.npz`) from the REAL reference.

Runs only where the reference is present.  Same pattern as `make_golden_code2_lp.py`: the reference's files are imported
unmodified (`ogbg-code/model/dagnn.py`, `ogbg-code/utils.py`, `ogbg-code/utils2.py`, `src/utils_dag.py`,
`ogb/graphproppred/evaluate.py`), weights come from `oracle.seeding.seeded_fill` and are never stored, only data goes into
this directory.

    python tests/golden/make_golden_code2_train.py

Each fixture: THREE consecutive steps of the reference's own loop body - `train()` of ogbg-code/main_pyg.py:39-88 for the TOK
task, of ogbg-code/main_pyg_lp.py:43-74 for the LP task - over 36 seeded graphs in three batches of 12, in order, with
`torch.optim.Adam(lr=1e-3)`: forward, `zero_grad()`, the loss, `backward()`, `step()`, `loss_accum += loss.item()`, the argmax
of the training logits.  Stored: the three batches, `y_arr` and the label words (TOK) / `len_longest_path` (LP), per step the
loss, the tokens and the top-2 margin of every row, the epoch's `loss_accum / (step + 1)` and the evaluator's own F1 / acc on
the three steps' tokens.  The same three steps run a second time with the reference model in float64: `loss64` per step,
`loss_err_ref` = |loss32 - loss64|.  The reference model takes `.double()` only under `torch.set_default_dtype(torch.float64)`
- its state buffers are `torch.zeros(...)` of the default dtype (model/dagnn.py:141, 173), which would round every state to
float32 - so the float64 run sets that default for its duration; the edge attributes are cast with the model.

TOK: H = 32, L = 2, bidirectional, `attn_h`, S = 5, a vocabulary of 12 words + `__UNK__` + `__EOS__` (small, so that seeded
random weights predict label words often enough for a training F1 above zero); `y_arr` is the reference's
`encode_seq_to_arr` of the label words.  As in `make_golden_code2_eval.py` each head's bias at the EOS column is
raised after `seeded_fill` (by the median over the first batch of top-1 logit - EOS logit), so that rows end in EOS; the
tests apply the stored boosts.  LP: the `code2_lp_gated_h64` shape; its 36 graphs are the first of 144 seeded ones whose
longest path is below the 24 classes.

The data seed is the first one from the starting value at which no row's two best logits are within TAU = 2e-4 in any of
the three steps (ambiguous share 0: asserted), and - LP - every target is below `num_class`; the fixture's own F1 / acc can
then be demanded exactly.
"""
from __future__ import annotations

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
STEPS, B = 3, 12
BATCH_KEYS = ("x", "node_depth", "edge_index", "edge_attr", "batch", "layer0", "layer1")


def _words(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def _graphs(ref_dagutils, data_seed, mean_n, n_attr, max_n=1000, max_llp=None):
    """STEPS * B seeded graphs with the reference's layer ids; `max_llp`: the first STEPS * B of four times as many whose
    longest path is below it (one in five synthetic graphs of 30 nodes is deeper than the LP fixtures' 24 classes)."""
    graphs = synth.code2_graphs(data_seed, STEPS * B * (4 if max_llp else 1), mean_n, max_n)
    if max_llp:
        graphs = [g for g in graphs if int(g._bi_layer_idx0.max()) < max_llp][:STEPS * B]
        assert len(graphs) == STEPS * B
    llp = []
    for g in graphs:
        g.x[:, 1] %= n_attr
        ns = SimpleNamespace(edge_index=g.edge_index, num_nodes=g.num_nodes)
        ref_dagutils.add_order_info_01(ns)
        for k in ("_bi_layer_idx0", "_bi_layer_index0", "_bi_layer_idx1", "_bi_layer_index1"):
            setattr(g, k, getattr(ns, k))
        llp.append(float(torch.max(ns._bi_layer_idx0).item()))   # ogb/io/read_graph_pyg.py:54
    return graphs, llp


def _G(b, dtype):
    return SimpleNamespace(x=b.x.clone(), node_depth=b.node_depth.clone(), edge_index=b.edge_index.clone(),
                           edge_attr=b.edge_attr.clone().to(dtype), batch=b.batch.clone(),
                           _bi_layer_idx0=b._bi_layer_idx0.clone(), _bi_layer_index0=b._bi_layer_index0.clone(),
                           _bi_layer_idx1=b._bi_layer_idx1.clone(), _bi_layer_index1=b._bi_layer_index1.clone())


def _in_float64(fn):
    torch.set_default_dtype(torch.float64)
    try:
        return fn()
    finally:
        torch.set_default_dtype(torch.float32)


def _labels(rng, idx2vocab, n):
    """Label word lists: mostly vocabulary words, some outside it, repeats, lists longer than S, an empty one."""
    out = []
    for g in range(n):
        lab = []
        for _ in range(int(rng.integers(0, 8))):
            u = rng.random()
            if u < 0.75:
                lab.append(idx2vocab[int(rng.integers(0, len(idx2vocab) - 2))])
            elif u < 0.9:
                lab.append("rare_%d" % int(rng.integers(0, 5)))
            elif lab:
                lab.append(lab[int(rng.integers(0, len(lab)))])
        out.append([] if g == 7 else lab)
    return out


def _margin(p):
    if p.shape[1] < 2:
        return np.full(p.shape[0], np.inf, dtype=np.float32)
    top = torch.topk(p.detach(), 2, dim=1).values
    return _np(top[:, 0] - top[:, 1])


def run_tok(make_model, batches, y_arrs, dtype):
    """main_pyg.py:52-72 three times: (losses, token matrices, margins [B, S])."""
    model = make_model().to(dtype).train()
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = torch.nn.CrossEntropyLoss()
    losses, toks, margins = [], [], []
    for b, y_arr in zip(batches, y_arrs):
        pred_list = model(_G(b, dtype))
        optimizer.zero_grad()
        loss = 0
        for i in range(len(pred_list)):
            loss += crit(pred_list[i].to(dtype), y_arr[:, i])
        loss = loss / len(pred_list)
        loss.backward()
        optimizer.step()
        losses.append(loss.item())
        mat = []
        for i in range(len(pred_list)):
            mat.append(torch.argmax(pred_list[i], dim=1).view(-1, 1))
        toks.append(torch.cat(mat, dim=1))
        margins.append(np.stack([_margin(p) for p in pred_list], axis=1))
    return losses, toks, margins


def run_lp(make_model, batches, targs, dtype):
    """main_pyg_lp.py:53-67 three times."""
    model = make_model().to(dtype).train()
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = torch.nn.CrossEntropyLoss()
    losses, toks, margins = [], [], []
    for b, targ in zip(batches, targs):
        pred = model(_G(b, dtype))
        optimizer.zero_grad()
        loss = crit(pred, targ.to(torch.long))
        loss.backward()
        optimizer.step()
        losses.append(loss.item())
        toks.append(torch.argmax(pred.detach(), dim=1).view(-1, 1))
        margins.append(_margin(pred))
    return losses, toks, margins


def _batch_arrays(batches):
    arrays = {}
    for s, b in enumerate(batches):
        vals = dict(x=b.x, node_depth=b.node_depth, edge_index=b.edge_index, edge_attr=b.edge_attr, batch=b.batch,
                    layer0=b._bi_layer_idx0, layer1=b._bi_layer_idx1)
        for k in BATCH_KEYS:
            arrays["s%d::%s" % (s, k)] = _np(vals[k])
    return arrays


def _step_arrays(l32, l64, toks, margins):
    arrays = dict(loss=np.asarray(l32, dtype=np.float64), loss64=np.asarray(l64, dtype=np.float64),
                  loss_err_ref=np.abs(np.asarray(l32, dtype=np.float64) - np.asarray(l64, dtype=np.float64)))
    for s in range(STEPS):
        arrays["s%d::tok" % s] = _np(toks[s])
        arrays["s%d::margin" % s] = np.asarray(margins[s], dtype=np.float32)
    return arrays


def make_tok(ref_dagnn, ref_utils, ref_dagutils, ref_eval, name, *, seed0, mean_n, H, L, bidir, S, words, n_attr, w_seed):
    idx2vocab = ["w%02d" % i for i in range(words)] + ["__UNK__", "__EOS__"]
    vocab2idx = {w: i for i, w in enumerate(idx2vocab)}
    V = len(idx2vocab)
    kw = dict(w_edge_attr=True, num_layers=L, bidirectional=bidir, agg="attn_h", out_wx=False, out_pool_all=False,
              out_pool="max", dropout=0.0)
    for data_seed in range(seed0, seed0 + 200):
        graphs, _ = _graphs(ref_dagutils, data_seed, mean_n, n_attr)
        batches = [synth.GraphBatch.from_data_list(graphs[s * B:(s + 1) * B]) for s in range(STEPS)]
        seq_ref = _labels(np.random.default_rng(1000 + data_seed), idx2vocab, STEPS * B)
        y_arr = torch.cat([ref_utils.encode_seq_to_arr(seq, vocab2idx, S) for seq in seq_ref], dim=0)   # utils.py:155-163
        y_arrs = [y_arr[s * B:(s + 1) * B] for s in range(STEPS)]

        def plain():
            enc = ref_utils.ASTNodeEncoder(H, 98, n_attr, 20)
            m = ref_dagnn.DAGNN(num_vocab=V, max_seq_len=S, emb_dim=H, hidden_dim=H, out_dim=None, encoder=enc, **kw)
            seeded_fill(m, w_seed)
            return m

        with torch.no_grad():
            pred = plain().eval()(_G(batches[0], torch.float32))
        boost = np.array([np.float32(np.median(_np(p.max(dim=1).values - p[:, V - 1]))) for p in pred], dtype=np.float32)

        def make_model():
            m = plain()
            with torch.no_grad():
                for s, hd in enumerate(m.graph_pred_linear_list):
                    hd.bias[V - 1] += torch.tensor(boost[s])
            return m

        l32, toks, margins = run_tok(make_model, batches, y_arrs, torch.float32)
        if min(float(m.min()) for m in margins) <= TAU:
            continue
        break
    else:
        raise SystemExit("%s: no data seed without an ambiguous token" % name)
    l64, toks64, _ = _in_float64(lambda: run_tok(make_model, batches, y_arrs, torch.float64))
    assert all(torch.equal(a, b) for a, b in zip(toks, toks64)), name   # (no margin within TAU: both precisions agree)
    ambiguous = float(np.mean([float((m <= TAU).mean()) for m in margins]))
    assert ambiguous == 0.0, (name, ambiguous)
    # main_pyg.py:74-88
    arr_to_seq = lambda arr: ref_utils.decode_arr_to_seq(arr, idx2vocab)   # noqa: E731
    seq_pred = [arr_to_seq(arr) for mat in toks for arr in mat]
    res = ref_eval.Evaluator._eval_F1(None, seq_ref, seq_pred)
    mean_loss = sum(l32) / STEPS        # loss_accum / (step + 1): `loss_accum += loss.item()` in step order
    mean_loss64 = sum(l64) / STEPS
    eos_share = float(np.mean([float((_np(t) == V - 1).mean()) for t in toks]))
    print("%-24s seed %d  ambiguous %.4f  min margin %.3e  EOS share %.3f  losses %s  |32-64| %s  F1 %.6f"
          % (name, data_seed, ambiguous, min(float(m.min()) for m in margins), eos_share, ["%.6f" % v for v in l32],
             ["%.2e" % abs(a - c) for a, c in zip(l32, l64)], res["F1"]))
    assert 0.05 <= eos_share <= 0.7, (name, eos_share)
    arrays = _batch_arrays(batches)
    arrays.update(_step_arrays(l32, l64, toks, margins))
    meta = dict(kind="code2_train_tok", data_seed=data_seed, steps=STEPS, B=B, mean_n=mean_n, max_n=1000, H=H, L=L, bidir=bool(bidir),
                V=V, S=S, n_attr=n_attr, w_seed=w_seed, ctor=kw, lr=1e-3, tau=TAU, ambiguous=ambiguous, eos_share=eos_share,
                float64=True, mean_loss=mean_loss, mean_loss64=mean_loss64,
                state_dict={k_: list(v.shape) for k_, v in make_model().state_dict().items()})
    _save(name, meta, y_arr=_np(y_arr), seq_ref=_words(seq_ref), idx2vocab=_words(idx2vocab), boost_eos=boost,
          f1=np.array([res["precision"], res["recall"], res["F1"]], dtype=np.float64), **arrays)


def make_lp(ref_dagnn, ref_utils2, ref_dagutils, ref_eval, name, *, seed0, mean_n, H, L, bidir, agg, num_class, n_attr, w_seed):
    # main_pyg_lp.py:140-148, 373-377: the LP script's constructor arguments
    kw = dict(w_edge_attr=0, num_layers=L, bidirectional=bidir, agg=agg, mapper_bias=True, out_wx=False, out_pool_all=0,
              out_pool="max", dropout=0.0, num_class=num_class)

    def make_model():
        enc = ref_utils2.ASTNodeEncoder2(H, 98, n_attr, 20)
        m = ref_dagnn.DAGNN(num_vocab=None, max_seq_len=None, emb_dim=H, hidden_dim=H, out_dim=None, encoder=enc, **kw)
        seeded_fill(m, w_seed)
        return m

    for data_seed in range(seed0, seed0 + 200):
        graphs, llp = _graphs(ref_dagutils, data_seed, mean_n, n_attr, max_llp=num_class)
        assert max(llp) < num_class, (name, max(llp))   # (the reference's layer ids, not the ones the graphs were picked by)
        batches = [synth.GraphBatch.from_data_list(graphs[s * B:(s + 1) * B]) for s in range(STEPS)]
        targ = torch.tensor(llp)   # (what PyG's collation makes of the per-graph floats)
        targs = [targ[s * B:(s + 1) * B] for s in range(STEPS)]
        l32, toks, margins = run_lp(make_model, batches, targs, torch.float32)
        if min(float(m.min()) for m in margins) <= TAU:
            continue
        break
    else:
        raise SystemExit("%s: no data seed without an ambiguous token" % name)
    l64, toks64, _ = _in_float64(lambda: run_lp(make_model, batches, targs, torch.float64))
    assert all(torch.equal(a, b) for a, b in zip(toks, toks64)), name
    ambiguous = float(np.mean([float((m <= TAU).mean()) for m in margins]))
    assert ambiguous == 0.0, (name, ambiguous)
    # main_pyg_lp.py:66-74
    y_true = torch.cat([t.view(-1, 1) for t in targs], dim=0).numpy()
    y_pred = torch.cat(toks, dim=0).numpy()
    acc = ref_eval.Evaluator._eval_acc(None, y_true, y_pred)["acc"]
    mean_loss, mean_loss64 = sum(l32) / STEPS, sum(l64) / STEPS
    print("%-24s seed %d  ambiguous %.4f  min margin %.3e  max target %d  losses %s  |32-64| %s  acc %.6f"
          % (name, data_seed, ambiguous, min(float(m.min()) for m in margins), int(targ.max()), ["%.6f" % v for v in l32],
             ["%.2e" % abs(a - c) for a, c in zip(l32, l64)], acc))
    arrays = _batch_arrays(batches)
    arrays.update(_step_arrays(l32, l64, toks, margins))
    meta = dict(kind="code2_train_lp", data_seed=data_seed, steps=STEPS, B=B, mean_n=mean_n, max_n=1000, H=H, L=L, bidir=bool(bidir),
                agg=agg, num_class=num_class, n_attr=n_attr, w_seed=w_seed, ctor=kw, lr=1e-3, tau=TAU, ambiguous=ambiguous,
                float64=True, mean_loss=mean_loss, mean_loss64=mean_loss64,
                state_dict={k_: list(v.shape) for k_, v in make_model().state_dict().items()})
    _save(name, meta, len_longest_path=_np(targ), acc=np.array(acc, dtype=np.float64), **arrays)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not found at %s - fixtures can only be regenerated where it is present" % REF)
    _setup_paths()
    torch.manual_seed(0)
    import importlib
    ref_dagutils = importlib.import_module("src.utils_dag")
    ref_dagnn = _load_file("ref_ogbg_dagnn", os.path.join(REF, "ogbg-code", "model", "dagnn.py"))
    ref_utils = _load_file("ref_ogbg_utils", os.path.join(REF, "ogbg-code", "utils.py"))
    ref_utils2 = _load_file("ref_ogbg_utils2", os.path.join(REF, "ogbg-code", "utils2.py"))
    ref_eval = _load_file("ref_ogb_evaluate", os.path.join(REF, "ogb", "graphproppred", "evaluate.py"))

    make_tok(ref_dagnn, ref_utils, ref_dagutils, ref_eval, "code2_train_tok_h32", seed0=301, mean_n=30, H=32, L=2, bidir=1, S=5,
             words=12, n_attr=300, w_seed=191)
    make_lp(ref_dagnn, ref_utils2, ref_dagutils, ref_eval, "code2_train_lp_gated_h64", seed0=311, mean_n=30, H=64, L=1, bidir=0,
            agg="gated_sum", num_class=24, n_attr=300, w_seed=192)


if __name__ == "__main__":
    main()
