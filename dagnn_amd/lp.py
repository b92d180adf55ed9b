"""The longest-path (LP) task of ogbg-code2 (ogbg-code/main_pyg_lp.py) around the model, on the device.

The reference predicts `len_longest_path` of every AST as one of 275 classes: one `[B, num_class]` head, `CrossEntropyLoss`
against `targ.to(torch.long)` (main_pyg_lp.py:56-58), accuracy through `Evaluator("ogbg-ppa")` - `_eval_acc` of
ogb/graphproppred/evaluate.py:221-229 - on the argmax and the targets of every batch, copied to the host batch by batch
(main_pyg_lp.py:66-74, 93-107).  Here: `lp_targets` (the attribute, or the per-graph maximum of `_bi_layer_idx0` in one
launch when the dataset is a stock one), `class_cross_entropy` (loss and d logits in one launch), `ClassAccuracy` (one
launch per batch, one copy to the host at the end), with the model built as `DAGNN(..., encoder=ASTNodeEncoder2(...),
num_class=275)`.  Kernels: csrc/lp.hip; the loss is the one-head instance of csrc/loss.hip's kernel.

    for batch in lp_batches(loader, training=True):
        loss = class_cross_entropy(model(batch), lp_targets(batch)); loss.backward(); optimizer.step()
    metric = evaluate_lp(model, lp_batches(valid_loader, training=False))       # {'acc', 'n'}
"""
from __future__ import annotations

from typing import Iterable, Iterator, Optional

import numpy as np
import torch

from . import engine
from .core import num_graphs_of

__all__ = ["lp_targets", "graph_depth_host", "class_cross_entropy", "class_ce_step", "class_ce_step_host", "class_hits_host",
           "ClassAccuracy", "lp_batches", "evaluate_lp"]


# ----------------------------------------------------------------------------- targets
def graph_depth_host(layer, batch, num_graphs: Optional[int] = None) -> np.ndarray:
    """The definition `dagnn_graph_depth` implements, in numpy: [num_graphs] int64, the largest `layer` value among the nodes
    whose `batch` id is g; 0 for an id without nodes; ids outside [0, num_graphs) are ignored.  `num_graphs` None: the
    largest id + 1."""
    layer = np.asarray(layer.cpu() if isinstance(layer, torch.Tensor) else layer).reshape(-1)
    batch = np.asarray(batch.cpu() if isinstance(batch, torch.Tensor) else batch).reshape(-1)
    if num_graphs is None:
        num_graphs = int(batch.max()) + 1 if batch.size else 0
    out = np.zeros(int(num_graphs), dtype=np.int64)
    keep = (batch >= 0) & (batch < num_graphs)
    np.maximum.at(out, batch[keep], layer[keep].astype(np.int64))
    return out


def lp_targets(batch, num_graphs: Optional[int] = None) -> torch.Tensor:
    """The LP task's targets of a batch, [B] int64 on the batch's device: `batch.len_longest_path` as the reference casts it
    (`.to(torch.long)`, main_pyg_lp.py:56-58) when the batch carries it - the reference's patched reader stores it,
    ogb/io/read_graph_pyg.py:51-54 - else what that reader computes, the maximum of `_bi_layer_idx0` per graph, from the
    layer ids the batch already holds (`dagnn_graph_depth` on the GPU: one launch, no host read when `num_graphs` is given
    or the batch knows its `num_graphs`; `graph_depth_host` for a CPU batch)."""
    llp = getattr(batch, "len_longest_path", None)
    if llp is not None:
        return llp.reshape(-1).to(batch.batch.device).to(torch.long)
    B = int(num_graphs) if num_graphs is not None else num_graphs_of(batch)
    layer = batch._bi_layer_idx0
    if layer.is_cuda:
        return engine.graph_depth(layer, batch.batch, B)
    return torch.from_numpy(graph_depth_host(layer, batch.batch, B))


# ----------------------------------------------------------------------------- loss
class _ClassCE(torch.autograd.Function):
    """Mean cross-entropy of one [B, C] head, loss and gradient in one HIP launch (`dagnn_class_ce`, csrc/loss.hip); the
    backward is one multiplication by the incoming scalar, into rows of the pitch `_HeadsLinear.backward` reads."""

    @staticmethod
    def forward(ctx, pred, targ):
        loss, ctx.dl = engine.class_ce(pred, targ, pred.requires_grad)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        return engine._scale_rows(ctx.dl, g), None


def _fused_ok(pred, targ: torch.Tensor) -> bool:
    """Whether the one-launch loss can take `pred` and `targ` - fp32 GPU logits [B >= 1, C >= 1] with unit column stride,
    one target per row: the predicate of `class_cross_entropy` and `class_ce_step`."""
    return isinstance(pred, torch.Tensor) and pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 2 and \
        pred.shape[0] > 0 and pred.shape[1] > 0 and pred.stride(1) == 1 and (pred.shape[0] == 1 or pred.stride(0) >= pred.shape[1]) \
        and targ.numel() == pred.shape[0]


def class_cross_entropy(pred: torch.Tensor, targ: torch.Tensor) -> torch.Tensor:
    """`torch.nn.CrossEntropyLoss()(pred, targ.to(torch.long))` - the loss of the reference's LP loop (main_pyg_lp.py:56-58), a
    mean over the graphs.  `pred` [B, C] fp32 on the GPU with unit column stride: loss and d logits are ONE launch
    (`dagnn_class_ce`).  `targ` [B] (or [B, 1]) may be int64 or the float tensor the reference concatenates; the kernel
    truncates toward zero as `.to(torch.long)` does.  A target outside [0, C) - a NaN included - makes the loss NaN (the
    contract of `dagnn_seq_ce`; there is no `ignore_index`), where torch raises.  Anything else (CPU, other dtypes, strided
    columns) takes `F.cross_entropy`."""
    if not _fused_ok(pred, targ):
        return torch.nn.functional.cross_entropy(pred, targ.reshape(-1).to(pred.device).to(torch.long))
    return _ClassCE.apply(pred, targ)


class _ClassCEStep(torch.autograd.Function):
    """`_ClassCE` through `dagnn_class_ce_step` (the STEP instance of the same kernel, csrc/loss.hip): the same loss and d
    logits, and in the same launch the step's tokens, its (hits, labelled) pair and the epoch sums on `meter`."""

    @staticmethod
    def forward(ctx, pred, targ, meter):
        loss, ctx.dl, meter.tok = engine.class_ce_step(pred, targ, pred.requires_grad, meter.hits, meter.loss_sum, meter.steps)
        meter.graphs += pred.shape[0]
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        return engine._scale_rows(ctx.dl, g), None, None


def class_ce_step(pred: torch.Tensor, targ: torch.Tensor, meter) -> torch.Tensor:
    """The loss of `class_cross_entropy(pred, targ)` - under autograd, the same bits - with the rest of the reference's LP
    training step (main_pyg_lp.py:64-67) in the SAME launch: `loss_accum += loss.item()` as a float64 sum on the device, the
    argmax (`meter.tok`, [B]) and the batch's (hits, labelled) pair of `Evaluator._eval_acc` added to the epoch's.  `meter`:
    a `train.EpochMeter` made without `eos_id`.  Nothing synchronises; `meter.result()` is the epoch's one read.  The fused
    launch (`dagnn_class_ce_step`) runs under the conditions of `class_cross_entropy` for a meter on the logits' device; anything
    else composes `class_cross_entropy`, the argmax and `class_hits` / `class_hits_host` on the meter."""
    if meter.eos_id is not None:
        raise ValueError("class_ce_step: the meter was made with `eos_id` (a TOK meter)")
    if _fused_ok(pred, targ) and meter.device == pred.device:
        return _ClassCEStep.apply(pred, targ, meter)
    loss = class_cross_entropy(pred, targ)
    from .evaluate import rows_argmax
    tok = rows_argmax(pred.detach()).reshape(-1)
    if tok.is_cuda:
        pair = engine.class_hits(tok, targ)
    else:
        pair = torch.from_numpy(class_hits_host(tok, targ))
    meter.hits.add_(pair.to(meter.device))
    meter.loss_sum.add_(loss.detach().to(torch.float32).to(meter.device, torch.float64))
    meter.steps.add_(1)
    meter.tok = tok
    meter.graphs += pred.shape[0]
    return loss


def class_ce_step_host(logits, targ, epoch_hits=(0, 0), epoch_sum: float = 0.0) -> dict:
    """The definition `dagnn_class_ce_step` implements, in numpy: `train.seq_ce_step_host` with one head - the target
    truncated toward zero as `.to(torch.long)` does, a NaN target outside every class - with `hits` [2] int64 = the incoming
    pair + `class_hits_host(tok, targ)` in place of the counts."""
    from .train import seq_ce_step_host
    t = _as_np(targ).reshape(-1)
    if t.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            cls = np.where(np.isfinite(t), np.trunc(np.where(np.isfinite(t), t, 0.0)), -1).astype(np.int64)
    else:
        cls = t.astype(np.int64)
    x = _as_np(logits)
    out = seq_ce_step_host(x.reshape(x.shape[0], 1, -1), cls.reshape(-1, 1), 0, epoch_sum=epoch_sum)
    tok = out["tok"].reshape(-1)
    return {"row_loss": out["row_loss"], "loss": out["loss"], "tok": tok, "epoch_sum": out["epoch_sum"],
            "hits": np.asarray(epoch_hits, dtype=np.int64) + class_hits_host(tok, t)}


# ----------------------------------------------------------------------------- accuracy
def _as_np(t):
    return np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t)


def class_hits_host(pred, targ) -> np.ndarray:
    """The definition `dagnn_class_hits` implements, in numpy: [2] int64 = (hits, labelled) of one batch.  `pred`: float logits
    [B, C] - argmax with the lowest column among equals, a NaN beating every number (`torch.argmax`) - or integer tokens [B] /
    [B, 1]; `targ` [B] / [B, 1].  `Evaluator._eval_acc`'s own operations: labelled where the target equals itself (not NaN),
    hit where target and prediction are equal as values."""
    pred, targ = _as_np(pred), _as_np(targ).reshape(-1)
    if pred.dtype.kind == "f":
        nan = np.isnan(pred)
        tok = np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, pred).argmax(axis=1)).astype(np.int64)
    else:
        tok = pred.reshape(-1).astype(np.int64)
    is_labeled = targ == targ
    correct = targ[is_labeled] == tok[is_labeled]
    return np.array([int(np.sum(correct)), int(len(correct))], dtype=np.int64)


class ClassAccuracy(object):
    """The accuracy evaluator of the LP task (`Evaluator("ogbg-ppa")`: `_eval_acc`) as an accumulator, in the shape of `SeqF1`.
    `update(pred_or_tok, targ)`: one launch of `dagnn_class_hits` for GPU predictions - [B, C] fp32 logits (argmax fused) or
    the [B] / [B, 1] int64 tokens of `DAGNN.predict` - writing one (hits, labelled) int64 pair into device memory (the numpy
    mirror `class_hits_host` for CPU predictions); nothing synchronises.  `compute()`: the one copy to the host, then
    `float(hits) / labelled` -> {'acc', 'n'}; without a labelled graph the evaluator divides by zero: `ValueError`."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self._parts = []

    def update(self, pred: torch.Tensor, targ: torch.Tensor) -> None:
        B = pred.shape[0] if pred.dim() else 1
        if targ.numel() != B:
            raise ValueError("ClassAccuracy.update: %d targets for %d predictions" % (targ.numel(), B))
        if B == 0:
            return
        if pred.is_cuda:
            self._parts.append(engine.class_hits(pred.detach(), targ))
        else:
            self._parts.append(torch.from_numpy(class_hits_host(pred, targ)))

    def counts(self) -> np.ndarray:
        """(hits, labelled) of every update so far, [updates, 2] int64 on the host (one blocking copy)."""
        if not self._parts:
            return np.zeros((0, 2), dtype=np.int64)
        if len({p.device for p in self._parts}) > 1:
            return np.stack([p.cpu().numpy() for p in self._parts])
        return torch.stack(self._parts).cpu().numpy()

    def compute(self) -> dict:
        hits, labelled = (int(v) for v in self.counts().sum(axis=0)) if self._parts else (0, 0)
        if labelled == 0:
            raise ValueError("ClassAccuracy.compute: no labelled graph (the evaluator's division by zero)")
        return {"acc": float(hits) / labelled, "n": labelled}


# ----------------------------------------------------------------------------- the loops
def lp_batches(batches: Iterable, training: bool) -> Iterator:
    """The reference's filters on its batches (main_pyg_lp.py:51, 84): a batch with ONE node is dropped; a training loop also
    drops a batch with ONE graph (its `batch.batch[-1] == 0`).  The graph count is the batch's host attribute `num_graphs`
    (`core.num_graphs_of`: a batch without it costs the device read the reference's test costs)."""
    for b in batches:
        if b.x.shape[0] == 1:
            continue
        if training and num_graphs_of(b) == 1:
            continue
        yield b


def evaluate_lp(model, batches: Iterable, loss: bool = False) -> dict:
    """The evaluation loop of main_pyg_lp.py:77-107: `predict`, `lp_targets`, `ClassAccuracy.update` per batch and one
    `compute()` - the loop's only synchronisation besides what the passes themselves need - at the end -> {'acc', 'n'}.
    Filtering (`lp_batches`) stays with the caller; the model's mode is restored.  `loss=True`: the passes are
    `score(batch, targets)` - the targets cast as `class_cross_entropy` casts them, `.to(torch.long)` - and the dict gains
    'loss', the float64 sum of every graph's `CrossEntropyLoss` term divided by the number of graphs."""
    from .evaluate import SeqLoss, _with_loss
    was_training = model.training
    model.eval()
    metric = ClassAccuracy()
    acc = None
    try:
        for batch in batches:
            B = num_graphs_of(batch)
            targ = lp_targets(batch, B)   # (before the pass: `forward` may replace `batch.batch`)
            if loss:
                if acc is None:
                    acc = SeqLoss(targ.device)
                metric.update(model.score(batch, _class_targets(targ), sums=acc).tok.reshape(-1), targ)
            else:
                metric.update(model.predict(batch), targ)
    finally:
        if was_training:
            model.train()
    return _with_loss(metric, acc)


def _class_targets(targ: torch.Tensor) -> torch.Tensor:
    """Targets as classes, [B] int64: truncated toward zero as `.to(torch.long)` does; a NaN or infinite target lies outside
    every class (-1), as `dagnn_class_ce` decides."""
    targ = targ.reshape(-1)
    if targ.dtype.is_floating_point:
        return torch.where(torch.isfinite(targ), targ, torch.full_like(targ, -1.0)).to(torch.long)
    return targ.to(torch.long)
