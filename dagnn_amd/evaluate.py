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

Beyond the arg-max: `DAGNN.score` (`dagnn_heads_score`: the k best columns, their log-probabilities, the log-sum-exp and - with
targets - the row losses of `CrossEntropyLoss`, main_pyg.py:37,55-60, still without the logits), `SeqLoss` (the loss of an
evaluation as a float64 sum on the device) and `loss=True` on the loops.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import engine
from .attention import Attention, attention_host   # (what `model.attention(G)` returns, and its definition in torch ops)
from .train import heads_base

__all__ = ["rows_argmax", "encode_ref_sets", "tokens_to_seqs", "f1_counts_host", "f1_from_counts", "SeqF1", "evaluate",
           "heads_score_host", "rows_score", "Score", "SeqLoss", "Attention", "attention_host"]


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


# ----------------------------------------------------------------------------- scores: top-k, log-sum-exp, row losses
def _order_keys(x: np.ndarray) -> np.ndarray:
    """The order of logits of csrc/predict.hip as a float64 sort key: a NaN above every number (+inf included), -0 == +0."""
    return np.where(np.isnan(x), np.inf, np.where(np.isinf(x), np.sign(x) * 1e308, x + 0.0))


def heads_score_host(out, wcat, bcat, S: int, V: int, y=None, k: int = 1) -> dict:
    """The definition `dagnn_heads_score` implements, in numpy on float64 logits of the fp32 inputs (`out` [B, D], `wcat`
    [S V, D], `bcat` [S V]): {'tok' [B, S, k] int64, 'logit' [B, S, k], 'lse' [B, S], 'nll' [B, S] or None, 'logits'
    [B, S, V]}, all float64.  Ranks descend in the order of `predict`: the greatest value first, the lowest column among equals, a
    NaN above every number and the first NaN first, -0 == +0; ranks beyond V hold column -1 and -inf.  `lse` follows
    `torch.logsumexp`: NaN with any NaN in the row, else +inf with any +inf, -inf for a row of -inf alone.  `nll` = lse - the
    logit at y[b, s]; NaN, for that row alone, where the target lies outside [0, V)."""
    def as_np(t):
        return np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t)
    out, wcat, bcat = as_np(out).astype(np.float64), as_np(wcat).astype(np.float64), as_np(bcat).astype(np.float64)
    B = out.shape[0]
    k = int(k)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        logits = (out @ wcat.T + bcat.reshape(1, -1)).reshape(B, S, V)
        order = np.argsort(-_order_keys(logits), axis=2, kind="stable")[:, :, :k]
        tok = np.full((B, S, k), -1, dtype=np.int64)
        logit = np.full((B, S, k), -np.inf)
        tok[:, :, :order.shape[2]] = order
        logit[:, :, :order.shape[2]] = np.take_along_axis(logits, order, axis=2)
        m = np.max(np.where(np.isnan(logits), -np.inf, logits), axis=2)
        mf = np.where(np.isinf(m), 0.0, m)
        lse = mf + np.log(np.sum(np.exp(logits - mf[:, :, None]), axis=2))
        nll = None
        if y is not None:
            t = as_np(y).astype(np.int64).reshape(B, S)
            ok = (t >= 0) & (t < V)
            xy = np.take_along_axis(logits, np.where(ok, t, 0)[:, :, None], axis=2)[:, :, 0]
            nll = np.where(ok, lse - xy, np.nan)
    return {"tok": tok, "logit": logit, "lse": lse, "nll": nll, "logits": logits}


def rows_score(pred, y=None, k: int = 1):
    """(tok [B, S, k], logit [B, S, k] fp32, lse [B, S] fp32, nll or None) from logits that exist - a list of S [B, V] tensors -
    in torch ops, with the ordering and special-value rules of `heads_score_host`: what `DAGNN.score` composes for heads that
    are not plain fp32 GPU `nn.Linear`."""
    x = torch.stack([p.detach().float() for p in pred], dim=1)   # [B, S, V]
    B, S, V = x.shape
    k = int(k)
    x64 = x.double()
    key = torch.where(torch.isnan(x64), torch.full_like(x64, float("inf")),
                      torch.where(torch.isinf(x64), torch.sign(x64) * 1e308, x64 + 0.0))   # (`_order_keys`)
    order = torch.sort(key, dim=2, descending=True, stable=True).indices[:, :, :k]
    tok = torch.full((B, S, k), -1, dtype=torch.int64, device=x.device)
    logit = torch.full((B, S, k), float("-inf"), dtype=torch.float32, device=x.device)
    tok[:, :, :order.shape[2]] = order
    logit[:, :, :order.shape[2]] = torch.gather(x, 2, order)
    logit = logit + 0.0   # (-0 reads as +0, as the kernel's keys return it)
    lse = torch.logsumexp(x, dim=2)
    nll = None
    if y is not None:
        t = y.reshape(B, S).to(x.device).to(torch.int64)
        ok = (t >= 0) & (t < V)
        xy = torch.gather(x, 2, torch.where(ok, t, torch.zeros_like(t)).unsqueeze(2)).squeeze(2)
        nll = torch.where(ok, lse - xy, torch.full_like(lse, float("nan")))
    return tok, logit, lse, nll


class Score(object):
    """What `DAGNN.score` returns: `tok` [B, S, k] int64 and `logit` [B, S, k] (the k best columns of every (graph, head) and
    their logits, best first), `lse` [B, S], `nll` [B, S] (None without targets); `logprob` = logit - lse; `loss` = the mean of
    `nll`, a device scalar (`train.seq_cross_entropy(model(G), y_arr)` by definition)."""
    __slots__ = ("tok", "logit", "lse", "nll")

    def __init__(self, tok, logit, lse, nll=None):
        self.tok, self.logit, self.lse, self.nll = tok, logit, lse, nll

    @property
    def logprob(self) -> torch.Tensor:
        return self.logit - self.lse.unsqueeze(-1)

    @property
    def loss(self) -> torch.Tensor:
        if self.nll is None:
            raise ValueError("Score.loss: scored without targets")
        return self.nll.mean()


class SeqLoss(object):
    """The loss of an evaluation as an accumulator, in the shape of `SeqF1`: a float64 sum of row losses and an int64 row
    count, 16 bytes on the device.  `model.score(G, y_arr, sums=acc)` adds a batch's rows inside its own launch, one by one
    in row order; `update(nll)` adds the rows of a tensor that exists (`torch.sum` in float64).  Nothing synchronises.
    `compute()`: the one read -> {'loss': sum / rows, 'rows'}."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.reset()

    def reset(self) -> None:
        self.sums = torch.zeros(2, dtype=torch.float64, device=self.device)   # [0]: the sum; [1]: the row count as int64 bits

    def update(self, nll: torch.Tensor) -> None:
        if nll.numel() == 0:
            return
        self.sums[0:1] += nll.detach().to(self.device, torch.float64).sum()
        self.sums.view(torch.int64)[1:2] += nll.numel()

    def stage(self) -> torch.Tensor:
        """The two words on their way to pinned host memory, without waiting: valid once a later blocking copy on the same
        stream has returned (`compute(staged)` then reads them without a synchronisation of its own)."""
        if self.device.type != "cuda":
            return self.sums
        host = torch.empty(2, dtype=torch.float64, pin_memory=True)
        host.copy_(self.sums, non_blocking=True)
        return host

    def compute(self, staged: Optional[torch.Tensor] = None) -> dict:
        host = self.sums.cpu() if staged is None else staged
        rows = int(host.view(torch.int64)[1])
        if rows == 0:
            raise ValueError("SeqLoss.compute: no row scored")
        return {"loss": float(host[0]) / rows, "rows": rows}


def evaluate(model, batches: Iterable, vocab2idx: Dict[str, int], loss: bool = False) -> dict:
    """The loop of ogbg-code/main_pyg.py:91-124 over batches whose `y` is the list of each graph's label words: `predict`,
    `encode_ref_sets`, `SeqF1.update` per batch and one `compute()` - the loop's only synchronisation besides what the passes
    themselves need - at the end.  `__EOS__` is the last vocabulary entry (utils.py:166-179).  Filtering one-node batches stays
    with the caller, as in the reference; the model's mode is restored.  `loss=True`: the passes are `score(batch,
    batch.y_arr)` - the same tokens - and the dict gains 'loss', the float64 sum of every row's `CrossEntropyLoss` term
    divided by (graphs * S): the criterion of main_pyg.py:37,55-60 on held-out batches; still one synchronisation."""
    was_training = model.training
    model.eval()
    metric = SeqF1(len(vocab2idx) - 1)
    acc = None
    try:
        for batch in batches:
            if loss:
                y_arr = batch.y_arr   # (before the pass, which may rewrite the batch)
                if acc is None:
                    acc = SeqLoss(y_arr.device)
                tok = model.score(batch, y_arr, sums=acc).tok[:, :, 0]
            else:
                tok = model.predict(batch)
            ref_ids, ref_extra = encode_ref_sets(batch.y, vocab2idx)
            metric.update(tok, ref_ids, ref_extra)
    finally:
        if was_training:
            model.train()
    return _with_loss(metric, acc)


def _with_loss(metric, acc) -> dict:
    """`metric.compute()` with 'loss' from `acc` (a `SeqLoss` or None) and still ONE synchronisation: the accumulator's 16
    bytes are queued into pinned memory in front of the metric's own blocking copy, which completes behind them."""
    if acc is None:
        return metric.compute()
    staged = acc.stage() if metric._parts and all(p.device == acc.device for p in metric._parts) else None
    res = metric.compute()
    res["loss"] = acc.compute(staged)["loss"]
    return res
