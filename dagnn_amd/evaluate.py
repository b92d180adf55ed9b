"""The evaluation half of the ogbg-code2 loop (ogbg-code/main_pyg.py:91-124) next to the model, on the device.

What the reference does per batch with the S heads' logits - `argmax` per head and a `cat` (main_pyg.py:106-109), a copy to
the host, `decode_arr_to_seq` per row (utils.py:166-179: cut at the first `__EOS__`, ids to words) - and at the end with all
word lists (ogb/graphproppred/evaluate.py:231-267: per graph the SET of label words against the SET of predicted words,
precision / recall / F1 averaged over graphs) is here: `DAGNN.predict` (tokens without logits), `SeqF1.update` (one launch of
integer set arithmetic per batch, counts kept on the device), one copy in `SeqF1.compute()`.

Why integers give the evaluator's numbers bit for bit: `idx2vocab` is injective, so sets of predicted ids and sets of predicted
words have the same sizes and intersections.  A label word outside the vocabulary can never be predicted: it only ever is a
false negative (`ref_extra`).  A predicted `__UNK__` id decodes to the literal word `__UNK__` and matches a label only if the
label holds that literal, which `vocab2idx` maps to the same id.  Labels are not cut to `max_seq_len` (the evaluator sees
`data.y` in full).  With tp, n_pred, n_ref per graph: false_positive = n_pred - tp, false_negative = n_ref - tp, and the three
divisions below are the evaluator's own float64 operations on the same integers.

    metric = evaluate.evaluate(model, batches, vocab2idx)       # {'precision', 'recall', 'F1', 'n'}
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np
import torch

from . import engine
from .train import heads_base

__all__ = ["rows_argmax", "encode_ref_sets", "tokens_to_seqs", "f1_counts_host", "f1_from_counts", "SeqF1", "evaluate"]


def rows_argmax(pred) -> torch.Tensor:
    """`torch.cat([torch.argmax(p, dim=1).view(-1, 1) for p in pred_list], dim=1)` (main_pyg.py:69-72,106-109) -> [B, S] int64.
    `pred`: the list `DAGNN.forward` returns, or one [B, V] tensor (`num_class` models).  When the list is S views of one
    [B, S V] fp32 GPU tensor (how `forward` lays the heads' outputs out; the detection `train.seq_cross_entropy` uses) this is
    ONE launch (`dagnn_rows_argmax`), else the plain loop."""
    if isinstance(pred, torch.Tensor):
        pred = [pred]
    pred = list(pred)
    base = heads_base(pred)
    if base is not None:
        return engine.rows_argmax(base.detach(), len(pred), pred[0].shape[1])
    if len(pred) == 1 and pred[0].is_cuda and pred[0].dtype == torch.float32 and pred[0].dim() == 2 and pred[0].stride(1) == 1:
        return engine.rows_argmax(pred[0].detach(), 1, pred[0].shape[1])
    return torch.cat([torch.argmax(p, dim=1).view(-1, 1) for p in pred], dim=1)


def encode_ref_sets(seq_ref: Sequence[Sequence[str]], vocab2idx: Dict[str, int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host side of the metric: the label word lists of a batch -> (`ref_ids` [B, R] int32: each graph's distinct in-vocabulary
    label ids in order of first appearance, padded with -1; `ref_extra` [B] int32: its number of distinct label words outside
    the vocabulary).  R = the batch's largest distinct in-vocabulary count (at least 1).  CPU tensors."""
    rows, extra = [], []
    for seq in seq_ref:
        words = list(dict.fromkeys(seq))   # distinct, first appearance first
        ids = [vocab2idx[w] for w in words if w in vocab2idx]
        rows.append(ids)
        extra.append(len(words) - len(ids))
    R = max([len(r) for r in rows] + [1])
    ref_ids = np.full((len(rows), R), -1, dtype=np.int32)
    for b, r in enumerate(rows):
        ref_ids[b, :len(r)] = r
    return torch.from_numpy(ref_ids), torch.from_numpy(np.asarray(extra, dtype=np.int32).reshape(len(rows)))


def tokens_to_seqs(tok: torch.Tensor, idx2vocab: Sequence[str]) -> List[List[str]]:
    """`[decode_arr_to_seq(arr, idx2vocab) for arr in tok]` (utils.py:166-179) with one copy to the host: every row cut at its
    first `__EOS__` (the LAST entry of `idx2vocab`), ids mapped to words."""
    rows = tok.detach().cpu().numpy()
    eos = len(idx2vocab) - 1
    out = []
    for r in rows:
        hit = np.flatnonzero(r == eos)
        out.append([idx2vocab[int(i)] for i in (r[:hit[0]] if hit.size else r)])
    return out


def f1_counts_host(tok, eos_id: int, ref_ids, ref_extra) -> np.ndarray:
    """The definition `dagnn_seq_f1_counts` implements, in numpy: counts [B, 4] int32 = (true_positive, n_pred, n_ref, len).
    len = position of the first `eos_id` in tok[b] (S if none); n_pred = distinct ids in tok[b, :len]; n_ref = distinct
    non-negative ids in ref_ids[b] + ref_extra[b]; true_positive = size of the intersection of the two id sets."""
    tok = np.asarray(tok.cpu() if isinstance(tok, torch.Tensor) else tok)
    ref_ids = np.asarray(ref_ids.cpu() if isinstance(ref_ids, torch.Tensor) else ref_ids)
    ref_extra = np.asarray(ref_extra.cpu() if isinstance(ref_extra, torch.Tensor) else ref_extra).reshape(-1)
    B, S = tok.shape
    out = np.zeros((B, 4), dtype=np.int32)
    for b in range(B):
        hit = np.flatnonzero(tok[b] == eos_id)
        n = int(hit[0]) if hit.size else S
        pred = set(tok[b, :n].tolist())
        ref = set(int(v) for v in ref_ids[b] if v >= 0)
        out[b] = (len(pred & ref), len(pred), len(ref) + int(ref_extra[b]), n)
    return out


def f1_from_counts(counts: np.ndarray) -> dict:
    """`Evaluator._eval_F1` (ogb/graphproppred/evaluate.py:231-267) from per-graph integer counts [n, >= 3] = (tp, n_pred,
    n_ref, ..): the evaluator's own operations in its own order - a zero denominator gives 0, `2 * p * r / (p + r)`,
    `np.average` over the per-graph lists."""
    precision_list, recall_list, f1_list = [], [], []
    for row in np.asarray(counts).tolist():
        true_positive, false_positive, false_negative = row[0], row[1] - row[0], row[2] - row[0]
        precision = true_positive / (true_positive + false_positive) if true_positive + false_positive > 0 else 0
        recall = true_positive / (true_positive + false_negative) if true_positive + false_negative > 0 else 0
        f1 = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0
        precision_list.append(precision)
        recall_list.append(recall)
        f1_list.append(f1)
    return {"precision": np.average(precision_list), "recall": np.average(recall_list), "F1": np.average(f1_list),
            "n": len(f1_list)}


class SeqF1(object):
    """The F1 evaluator of ogbg-code2 as an accumulator.  `update(tok, ref_ids, ref_extra)`: one launch of
    `dagnn_seq_f1_counts` for GPU tokens (the numpy mirror `f1_counts_host` for CPU tokens), the counts stay where the tokens
    are, nothing synchronises.  `compute()`: the one copy to the host, then `f1_from_counts` -> {'precision', 'recall', 'F1',
    'n'}.  `eos_id` is the id of `__EOS__`: `len(idx2vocab) - 1`."""

    def __init__(self, eos_id: int):
        self.eos_id = int(eos_id)
        self.reset()

    def reset(self) -> None:
        self._parts = []

    def update(self, tok: torch.Tensor, ref_ids: torch.Tensor, ref_extra: torch.Tensor) -> None:
        if tok.dim() != 2 or ref_ids.dim() != 2 or ref_ids.shape[0] != tok.shape[0] or ref_extra.numel() != tok.shape[0]:
            raise ValueError("SeqF1.update: tok [B, S], ref_ids [B, R], ref_extra [B] needed (got %s, %s, %s)"
                             % (tuple(tok.shape), tuple(ref_ids.shape), tuple(ref_extra.shape)))
        if tok.shape[0] == 0:
            return
        if tok.is_cuda:
            # (host tensors go through pinned memory: the copies are queued behind the pass, the host does not wait)
            ref_ids, ref_extra = (t if t.is_cuda else t.pin_memory().to(tok.device, non_blocking=True) for t in (ref_ids, ref_extra))
            self._parts.append(engine.seq_f1_counts(tok, self.eos_id, ref_ids, ref_extra))
        else:
            self._parts.append(torch.from_numpy(f1_counts_host(tok, self.eos_id, ref_ids, ref_extra)))

    def counts(self) -> np.ndarray:
        """Every graph's (true_positive, n_pred, n_ref, len) so far, in update order, on the host (one blocking copy)."""
        if not self._parts:
            return np.zeros((0, 4), dtype=np.int32)
        return (self._parts[0] if len(self._parts) == 1 else torch.cat(self._parts, dim=0)).cpu().numpy()

    def compute(self) -> dict:
        return f1_from_counts(self.counts())


def evaluate(model, batches: Iterable, vocab2idx: Dict[str, int]) -> dict:
    """The loop of ogbg-code/main_pyg.py:91-124 over batches whose `y` is the list of each graph's label words: `predict`,
    `encode_ref_sets`, `SeqF1.update` per batch and one `compute()` - the loop's only synchronisation besides what the passes
    themselves need - at the end.  `__EOS__` is the last vocabulary entry (utils.py:166-179).  Filtering one-node batches stays
    with the caller, as in the reference; the model's mode is restored."""
    was_training = model.training
    model.eval()
    metric = SeqF1(len(vocab2idx) - 1)
    try:
        for batch in batches:
            tok = model.predict(batch)
            ref_ids, ref_extra = encode_ref_sets(batch.y, vocab2idx)
            metric.update(tok, ref_ids, ref_extra)
    finally:
        if was_training:
            model.train()
    return metric.compute()
