"""Training-side plumbing for one-process-per-GPU data parallelism.

The reference trains with `tg/data_parallel.DataParallel`: one process, k threads, the 29.8 M parameters
re-broadcast and the gradients reduced to device 0 every step (`ogbg-code/tg/data_parallel.py:48-62`).  Here
every rank owns a full replica and its own shard of graphs; the only exchange of a training step is ONE
all-reduce of a flat gradient bucket over RCCL/xGMI.  The reference's loss is the mean over the graphs of the GLOBAL
batch (`main_pyg.py:55-60` on the gathered predictions) and its `Collater` balances shards by nodes, not by graphs
(`tg/dataloader.py:17-27`: 12..18 graphs per shard on the seed-0 batch), so every rank's gradient of its LOCAL mean
loss is weighted by its graph count: grad = sum_k b_k grad_k / sum_k b_k.  The counts travel in the same collective.
"""
from __future__ import annotations

from typing import Iterable, Optional

import torch
import torch.distributed as dist


class GradBucket(object):
    """All gradients of `params` as views of one contiguous fp32 buffer.

    autograd accumulates into an existing `.grad` in place, so after `backward()` the bucket holds the
    step's gradients without any copy; `all_reduce_mean` is then a single collective of `numel` floats
    (119 MB at the headline configuration) instead of one per parameter."""

    def __init__(self, params: Iterable[torch.nn.Parameter]):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("no trainable parameters")
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self._buf = torch.zeros(n + 1, dtype=torch.float32, device=dev)   # one more float: this rank's graph count
        self.flat = self._buf[:n]
        off = 0
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("GradBucket needs fp32 parameters on one device")
            p.grad = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()

    @property
    def numel(self) -> int:
        return self.flat.numel()

    def rebind(self) -> None:
        """Make every `p.grad` alias its view of the flat buffer again.  A gradient that lives elsewhere (the
        optimizer's `zero_grad()` set it to None and `backward()` allocated a fresh one) is copied in first; a
        parameter without a gradient this step contributes zeros."""
        off = 0
        for p in self.params:
            view = self.flat[off:off + p.numel()].view_as(p)
            g = p.grad
            if g is None:
                view.zero_()
                p.grad = view
            elif g.data_ptr() != view.data_ptr() or g.shape != view.shape:
                view.copy_(g)
                p.grad = view
            off += p.numel()

    def zero(self) -> None:
        """Replaces `optimizer.zero_grad()` (which would detach the views when it sets grads to None)."""
        self.flat.zero_()

    def all_reduce_mean(self, local_count: Optional[int] = None, group: Optional[dist.ProcessGroup] = None) -> None:
        """Gradient of the mean loss over the GLOBAL batch from the ranks' gradients of their local mean losses:
        sum_k b_k grad_k / sum_k b_k with b_k = `local_count` (graphs in this rank's shard; 0 for a rank that skipped
        its shard, as `main_pyg.py:47` does for one-graph chunks).  Without `local_count` every rank weighs the same
        (equal shards).  ONE collective of numel + 1 floats."""
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
            return
        self.launch(1.0 if local_count is None else float(local_count), group).wait()
        self.normalise()

    def launch(self, count: float, group: Optional[dist.ProcessGroup] = None):
        """Start the count-weighted sum of this bucket (asynchronous: returns the collective's work handle; the
        backend orders it behind the kernels already queued on the current stream)."""
        if count != 1.0:
            self.flat.mul_(count)
        self._buf[-1] = count
        return dist.all_reduce(self._buf, op=dist.ReduceOp.SUM, group=group, async_op=True)

    def normalise(self) -> None:
        """After the collective: divide by the total count it carried."""
        self.flat.div_(self._buf[-1].clamp(min=1.0))


def clip_flat_grad_norm_(flats, max_norm: float, eps: float = 1e-6) -> torch.Tensor:
    """`torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)` (`ogbg-code/main_pyg.py:63-64`, `--clip`, 0.25 in
    `scripts/ogb_tok.sh:16`) over flat gradient buffers: the global 2-norm of ALL gradients, every buffer scaled by
    `min(1, max_norm / (norm + eps))`.  One norm kernel per buffer instead of one per parameter, no device->host read
    (the scale stays on the device).  Under data parallelism it must see the REDUCED gradients - the mean over the
    global batch, identical on every rank - so it sits behind the last collective of the step and in front of
    `optimizer.step()`; every rank then applies the same scale without another exchange.  Returns the norm."""
    flats = [f for f in flats if f is not None and f.numel() > 0]
    if not flats:
        return torch.zeros(())
    sq = torch.stack([torch.linalg.vector_norm(f, 2.0) for f in flats])
    total = torch.linalg.vector_norm(sq, 2.0)
    coef = torch.clamp(float(max_norm) / (total + eps), max=1.0)
    for f in flats:
        f.mul_(coef)
    return total


class OverlappedGradReducer(object):
    """Gradient exchange of one training step in TWO buckets so that most of it hides behind the reverse sweep.

    The 29.8 M parameters of the headline model are 25.6 M in the vocabulary heads (`graph_pred_linear_list`,
    `dagnn.py:106-112`) and 4.2 M in the DAGNN core + encoder.  `loss.backward()` finishes the heads first - their
    gradients are final before the recurrence's reverse sweep (the longest kernel of the step) even starts - so the
    heads' bucket (113 MB at cfg 2) is all-reduced ASYNCHRONOUSLY from a post-accumulate hook on the last head
    parameter, on the communication backend's own stream, while the sweep and its epilogue run; only the small core
    bucket (6.3 MB) is exchanged after `backward()` returns.  Same arithmetic as `GradBucket.all_reduce_mean`
    (count-weighted sum / total count), bucket by bucket: the result is identical to the single-bucket exchange.

        red = OverlappedGradReducer(model.parameters(), early=model.graph_pred_linear_list.parameters())
        red.zero(local_count=b_k); loss.backward(); red.finish(); optimizer.step()
    """

    def __init__(self, params: Iterable[torch.nn.Parameter], early: Iterable[torch.nn.Parameter],
                 group: Optional[dist.ProcessGroup] = None):
        early = [p for p in early if p.requires_grad]
        ids = {id(p) for p in early}
        rest = [p for p in params if p.requires_grad and id(p) not in ids]
        self.group = group
        from . import engine
        engine.register_collective(group)   # (the co-residency rule of the persistent kernels looks at THIS group: engine.reserved_cus)
        self.early = GradBucket(early) if early else None
        self.late = GradBucket(rest) if rest else None
        self._count = 1.0
        self._pending = 0
        self._work = None
        self.exposed_ms = None
        self._hooks = []
        if self.early is not None:
            for p in self.early.params:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_early_grad))

    def _active(self) -> bool:
        return dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1

    def zero(self, local_count: Optional[int] = None) -> None:
        """Start of a step.  `local_count` (graphs of this rank's shard) must be known here: the early bucket leaves
        in the middle of `backward()`."""
        for b in (self.early, self.late):
            if b is not None:
                b.zero()
        self._count = 1.0 if local_count is None else float(local_count)
        self._pending = len(self.early.params) if self.early is not None else 0
        self._work = None

    def _on_early_grad(self, p) -> None:
        self._pending -= 1
        if self._pending == 0 and self._active():
            self.early.rebind()   # (a gradient autograd allocated outside the bucket is copied in first)
            self._work = self.early.launch(self._count, self.group)

    def finish(self, clip: float = 0.0) -> Optional[torch.Tensor]:
        """After `backward()`: exchange the late bucket, wait for the early one, normalise both - and, with `clip` > 0, the
        reference's `clip_grad_norm(model.parameters(), clip)` (`main_pyg.py:63-64`) on the reduced gradients of BOTH
        buckets (it needs the global norm, so it cannot start before the last collective has landed); then
        `optimizer.step()`.  Returns the gradient norm when clipping."""
        self._exchange()
        if clip and clip > 0:
            for b in (self.early, self.late):   # (single process: the gradients may live outside the buckets)
                if b is not None and not self._active():
                    b.rebind()
            return clip_flat_grad_norm_([b.flat for b in (self.early, self.late) if b is not None], clip)
        return None

    def _exchange(self) -> None:
        if not self._active():
            return
        if self.early is not None and self._work is None:   # no hook fired (a head without gradient): exchange it now
            self.early.rebind()
            self._work = self.early.launch(self._count, self.group)
        if self.late is not None:
            self.late.rebind()
            w = self.late.launch(self._count, self.group)
            w.wait()
            self.late.normalise()
        if self._work is not None:
            self._work.wait()
            self.early.normalise()
            self._work = None

    def remove(self) -> None:
        for h in self._hooks:
            h.remove()
        self._hooks = []


# ----------------------------------------------------------------------------- the TOK task's loss (main_pyg.py:55-60)
class _SeqCE(torch.autograd.Function):
    """Mean cross-entropy over the S heads' logits laid side by side in ONE [B, S * V] tensor, loss and gradient in one HIP
    launch (`engine.seq_ce`: `dagnn_seq_ce`, csrc/loss.hip); the backward is one multiplication by the incoming scalar."""

    @staticmethod
    def forward(ctx, base, y, S, V):
        from . import engine
        loss, ctx.dl = engine.seq_ce(base, y, S, V, base.requires_grad)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        from . import engine
        return engine._scale_rows(ctx.dl, g), None, None, None


def heads_base(pred_list):
    """The ONE [B, S * V] fp32 GPU tensor `pred_list` is S views of - what `DAGNN.forward` returns on a GPU: the heads' outputs
    side by side, head i at column i * V - or None for any other list."""
    S = len(pred_list)
    if S == 0:
        return None
    p0 = pred_list[0]
    base = getattr(p0, "_base", None)
    if base is None or not base.is_cuda or base.dtype != torch.float32 or base.dim() != 2 or base.stride(1) != 1 or p0.dim() != 2:
        return None
    V = p0.shape[1]
    for i, p in enumerate(pred_list):
        if getattr(p, "_base", None) is not base or p.shape != p0.shape or p.stride() != base.stride() or \
                p.data_ptr() != base.data_ptr() + 4 * i * V:
            return None
    return base if base.shape[1] == S * V else None


def _fused_ok(pred_list, y_arr: torch.Tensor):
    """`heads_base(pred_list)` when the one-launch loss can take it with the targets `y_arr` - contiguous int64 [B, S] on a
    GPU - else None: the predicate of `seq_cross_entropy` and `seq_ce_step`."""
    base = heads_base(pred_list)
    ok = base is not None and y_arr.is_cuda and y_arr.dtype == torch.int64 and y_arr.dim() == 2 \
        and y_arr.shape[1] == len(pred_list) and y_arr.is_contiguous() and y_arr.shape[0] == base.shape[0]
    return base if ok else None


def seq_cross_entropy(pred_list, y_arr: torch.Tensor) -> torch.Tensor:
    """`sum_i CrossEntropyLoss()(pred_list[i], y_arr[:, i]) / len(pred_list)` - the loss of the reference's training loop
    (ogbg-code/main_pyg.py:55-60).  When the list is what `DAGNN.forward` returns on a GPU - views of one [B, S * V] tensor, the
    heads' outputs side by side - loss and gradient are ONE launch (`dagnn_seq_ce`) and the backward pass meets the heads as
    one matrix; any other list takes the plain loop.  Targets must lie in [0, V) (no `ignore_index`)."""
    S = len(pred_list)
    base = _fused_ok(pred_list, y_arr)
    if base is None:
        loss = 0
        for i in range(S):
            loss = loss + torch.nn.functional.cross_entropy(pred_list[i].to(torch.float32), y_arr[:, i])
        return loss / S
    V = pred_list[0].shape[1]
    return _SeqCE.apply(base, y_arr, S, V)


# ----------------------------------------------------------------------------- an epoch of `train()` (main_pyg.py:39-88)
class EpochMeter(object):
    """The device state of one epoch of the reference's `train()` (ogbg-code/main_pyg.py:39-88, main_pyg_lp.py:43-74): the
    float64 sum of the steps' losses (`loss_accum += loss.item()`), the step counter and what the training metric is made
    of - for the TOK task (`eos_id` given: the id of `__EOS__`) the `[capacity_graphs, 4]` int32 F1 counts of every graph
    seen, for the LP task (`eos_id` None) the (hits, labelled) int64 pair.  `seq_ce_step` / `lp.class_ce_step` update it
    inside the loss launch; nothing synchronises until `result()`.  One buffer holds all of it, so the read is one copy.

    `tok`: the predicted tokens of the last step ([B, S] / [B] int64).  `graphs`: graphs counted so far (host)."""

    _HEAD = 8   # int32 words in front of the counts: sum (float64) | steps (int64) | hits, labelled (int64)

    def __init__(self, device, capacity_graphs: int, eos_id: Optional[int] = None):
        self.capacity = int(capacity_graphs)
        if self.capacity < 0:
            raise ValueError("EpochMeter: capacity_graphs must not be negative")
        self.eos_id = None if eos_id is None else int(eos_id)
        rows = self.capacity if self.eos_id is not None else 0
        self._buf = torch.zeros(self._HEAD + 4 * rows, dtype=torch.int32, device=torch.device(device))
        self.device = self._buf.device   # (with its index, as every tensor's: 'cuda' and 'cuda:0' name one device and compare unequal)
        self.loss_sum = self._buf[0:2].view(torch.float64)
        self.steps = self._buf[2:4].view(torch.int64)
        self.hits = self._buf[4:8].view(torch.int64)
        self.counts = self._buf[self._HEAD:].view(rows, 4)
        self.graphs = 0
        self.tok = None

    def reset(self) -> None:
        self._buf.zero_()
        self.graphs = 0
        self.tok = None

    def room(self, B: int) -> int:
        """The row of `counts` the next step's first graph goes to; `ValueError` when its B graphs do not fit."""
        if self.eos_id is not None and self.graphs + B > self.capacity:
            raise ValueError("EpochMeter: %d graphs counted, %d more do not fit capacity_graphs=%d" % (self.graphs, B, self.capacity))
        return self.graphs

    def result(self, num_batches: int):
        """(`loss_sum / num_batches`, metric) after the epoch's ONE blocking read.  `num_batches` is the reference's
        `step + 1`: every batch of its loader, skipped ones included.  TOK: `evaluate.f1_from_counts` on the rows written
        -> {'precision', 'recall', 'F1', 'n'}; LP: {'acc', 'n'} as `ClassAccuracy.compute` gives it."""
        from .evaluate import f1_from_counts
        if int(num_batches) < 1:
            raise ValueError("EpochMeter.result: num_batches must be positive")
        rows = self.graphs if self.eos_id is not None else 0
        host = self._buf[:self._HEAD + 4 * rows].cpu()
        loss_sum = float(host[0:2].view(torch.float64)[0])
        if self.eos_id is not None:
            if rows == 0:
                raise ValueError("EpochMeter.result: no graph was counted")
            metric = f1_from_counts(host[self._HEAD:].view(rows, 4).numpy())
        else:
            hits, labelled = (int(v) for v in host[4:8].view(torch.int64))
            if labelled == 0:
                raise ValueError("EpochMeter.result: no labelled graph (the evaluator's division by zero)")
            metric = {"acc": float(hits) / labelled, "n": labelled}
        return loss_sum / int(num_batches), metric


def seq_ce_step_host(logits, y, eos_id: int, ref_ids=None, ref_extra=None, epoch_sum: float = 0.0) -> dict:
    """The definition `dagnn_seq_ce_step` implements, in numpy.  `logits` [B, S, V] (or [B, S V] with `y` [B, S]) fp32.
    `row_loss` [B S] fp32: log-sum-exp minus the target's logit per (graph, head) row, NaN for a target outside [0, V);
    `loss`: their fp32 sum in index order / (B S); `tok` [B, S] int64: lowest column among equals, a NaN beats every number,
    -0 == +0; `counts` [B, 4] int32 = `evaluate.f1_counts_host` of `tok` (None without `ref_ids`); `epoch_sum`: the incoming
    float64 + float64(loss), `loss_accum += loss.item()`."""
    import numpy as np
    from .evaluate import f1_counts_host
    y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).astype(np.int64)
    x = np.asarray(logits.detach().cpu() if isinstance(logits, torch.Tensor) else logits, dtype=np.float32)
    B, S = y.shape
    x = x.reshape(B, S, -1)
    V = x.shape[2]
    nan = np.isnan(x)
    tok = np.where(nan.any(axis=2), nan.argmax(axis=2), np.where(nan, -np.inf, x).argmax(axis=2)).astype(np.int64)
    x64 = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = x64.max(axis=2, keepdims=True)
        lse = m[..., 0] + np.log(np.exp(x64 - m).sum(axis=2))
    ok = (y >= 0) & (y < V)
    picked = np.take_along_axis(x64, np.where(ok, y, 0)[..., None], axis=2)[..., 0]
    row_loss = np.where(ok, lse - picked, np.nan).astype(np.float32).reshape(-1)
    acc = np.float32(0.0)
    for v in row_loss:
        acc = np.float32(acc + v)
    loss = np.float32(acc / np.float32(B * S))
    counts = None if ref_ids is None else f1_counts_host(tok, eos_id, ref_ids, np.zeros(B, np.int32) if ref_extra is None else ref_extra)
    return {"row_loss": row_loss, "loss": loss, "tok": tok, "counts": counts, "epoch_sum": float(epoch_sum) + float(loss)}


class _SeqCEStep(torch.autograd.Function):
    """`_SeqCE` through `dagnn_seq_ce_step` (the STEP instance of the same kernel, csrc/loss.hip): the same loss and d logits,
    and in the same launch the step's tokens, its F1 counts and the epoch sums on `meter`."""

    @staticmethod
    def forward(ctx, base, y, S, V, meter, ref_ids, ref_extra):
        from . import engine
        B = base.shape[0]
        off = meter.room(B) if ref_ids is not None else 0   # (a step without label sets counts no graph: nothing has to fit)
        loss, ctx.dl, tok = engine.seq_ce_step(base, y, S, V, base.requires_grad, meter.eos_id, ref_ids, ref_extra, meter.counts,
                                               off, meter.loss_sum, meter.steps)
        meter.tok = tok
        if ref_ids is not None:
            meter.graphs = off + B
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        from . import engine
        return engine._scale_rows(ctx.dl, g), None, None, None, None, None, None


def seq_ce_step(pred_list, y_arr: torch.Tensor, meter: EpochMeter, ref_ids: Optional[torch.Tensor] = None,
                ref_extra: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The loss of `seq_cross_entropy(pred_list, y_arr)` - under autograd, the same bits - with the rest of the reference's
    training step (main_pyg.py:67-83) in the SAME launch: `loss_accum += loss.item()` as a float64 sum on the device, the
    argmax of every head (`meter.tok`, [B, S]) and, with the batch's label id sets `ref_ids` [B, R] / `ref_extra` [B] (int32:
    `evaluate.encode_ref_sets`, or a `GraphStore` batch's own), the F1 counts of its graphs at their place in `meter.counts`.
    Nothing synchronises; `meter.result()` is the epoch's one read.

    The fused launch (`dagnn_seq_ce_step`) runs when `heads_base(pred_list)` is not None, under the conditions
    `seq_cross_entropy` checks, for a TOK meter on the logits' device; any other list composes `seq_cross_entropy`,
    `evaluate.rows_argmax` and the `SeqF1` arithmetic on the meter.  Without `ref_ids` the step counts no graph."""
    from . import engine
    from .evaluate import f1_counts_host, rows_argmax
    if meter.eos_id is None:
        raise ValueError("seq_ce_step: the meter was made without `eos_id` (an LP meter)")
    if (ref_ids is None) != (ref_extra is None):
        raise ValueError("seq_ce_step: `ref_ids` and `ref_extra` go together")
    S = len(pred_list)
    if S == 0:
        raise ValueError("seq_ce_step: empty `pred_list`")
    B = pred_list[0].shape[0]
    if ref_ids is not None:
        if ref_ids.dim() != 2 or ref_ids.shape[0] != B or ref_ids.shape[1] < 1 or ref_extra.numel() != B:
            raise ValueError("seq_ce_step: ref_ids [B, R >= 1] and ref_extra [B] needed (got %s, %s)"
                             % (tuple(ref_ids.shape), tuple(ref_extra.shape)))
        dev = pred_list[0].device
        # (host tensors go through pinned memory: the copies are queued behind the pass, the host does not wait)
        ref_ids, ref_extra = ((t if t.device == dev else t.pin_memory().to(dev, non_blocking=True)) if dev.type == "cuda" else t
                              for t in (ref_ids, ref_extra))
        ref_ids, ref_extra = ref_ids.to(torch.int32).contiguous(), ref_extra.reshape(B).to(torch.int32).contiguous()
    base = _fused_ok(pred_list, y_arr)
    if base is not None and meter.device == base.device:
        return _SeqCEStep.apply(base, y_arr, S, pred_list[0].shape[1], meter, ref_ids, ref_extra)
    off = meter.room(B) if ref_ids is not None else 0
    loss = seq_cross_entropy(pred_list, y_arr)
    tok = rows_argmax([p.detach() for p in pred_list])
    meter.loss_sum.add_(loss.detach().to(torch.float32).to(meter.device, torch.float64))
    meter.steps.add_(1)
    meter.tok = tok
    if ref_ids is not None:
        rows = meter.counts[off:off + B]
        if tok.is_cuda and meter.device == tok.device:
            engine.seq_f1_counts(tok, meter.eos_id, ref_ids, ref_extra, out=rows)
        else:
            rows.copy_(torch.from_numpy(f1_counts_host(tok, meter.eos_id, ref_ids, ref_extra)))
        meter.graphs = off + B
    return loss


# ----------------------------------------------------------------------------- clip_grad_norm_ + Adam (main_pyg.py:63-65)
class ClipAdam(torch.optim.Optimizer):
    """`torch.nn.utils.clip_grad_norm_(params, max_norm)` followed by `torch.optim.Adam(params, ...).step()` - the tail of the
    reference's training step (ogbg-code/main_pyg.py:63-65, optimizer at :179) - as three launches (csrc/optim.hip): the global
    gradient 2-norm as a device float (fixed summation order), then Adam's update with the clip coefficient applied to the
    gradient as it is read.  Every tensor crosses the memory bus once; torch's pair is ~12 launches that move the gradients
    three times and walk the small tensors at a fraction of the memory rate (0.36 -> 0.2 ms at the headline shape).

    Same update as `torch.optim.Adam` (no amsgrad, no maximize; `weight_decay` is Adam's L2 term) and the same `state_dict`
    layout (`step`, `exp_avg`, `exp_avg_sq` per parameter), so checkpoints move between the two.  `max_norm=None` (or <= 0)
    leaves the gradients unclipped.  Gradients themselves are NOT scaled in place (unlike `clip_grad_norm_`): the coefficient
    only enters the update.  `last_norm` is the device float of the last step's total norm (what `clip_grad_norm_` returns).
    The updated parameters' version counters move as under torch's Adam, so caches keyed on them see every step.
    fp32 parameters on one ROCm device."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_norm: Optional[float] = None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.max_norm = max_norm
        self.last_norm = None
        self._scratch = None

    @torch.no_grad()
    def step(self, closure=None):
        import ctypes as C
        from . import engine
        from ._lib import OptTensor
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = engine._lib.load()
        work = []   # (group, [params with a gradient])
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if ps:
                work.append((group, ps))
        if not work:
            return loss
        allp = [p for _, ps in work for p in ps]
        dev = allp[0].device
        for p in allp:
            if not p.is_cuda or p.device != dev or p.dtype != torch.float32 or p.grad.dtype != torch.float32 or p.grad.is_sparse:
                raise engine.DagnnHipError("ClipAdam needs dense fp32 parameters and gradients on one ROCm device")
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in allp]
        st = engine._stream(allp[0])
        cap = 48
        clip = self.max_norm is not None and self.max_norm > 0
        if clip:
            numel = (C.c_int64 * len(allp))(*[g.numel() for g in grads])
            chunks = int(lib.dagnn_opt_chunks(numel, len(allp)))
            sc = self._scratch
            if sc is None or sc[0].device != dev or sc[0].numel() < chunks:
                sc = self._scratch = (torch.empty(max(chunks, 1), dtype=torch.float32, device=dev),
                                      torch.empty(2, dtype=torch.float32, device=dev))
            for o in range(0, len(grads), cap):
                part = grads[o:o + cap]
                ptrs = (C.c_void_p * len(part))(*[g.data_ptr() for g in part])
                nn_ = (C.c_int64 * len(part))(*[g.numel() for g in part])
                engine.check(lib.dagnn_grad_norm(ptrs, nn_, len(part), sc[0].data_ptr(), sc[0].numel(), sc[1].data_ptr(),
                                                 1 if o > 0 else 0, sc[1].data_ptr() + 4, st), "dagnn_grad_norm")
            self.last_norm = sc[1][1]
        k = 0
        for group, ps in work:
            b1, b2 = group["betas"]
            gs = grads[k:k + len(ps)]
            k += len(ps)
            for p in ps:
                state = self.state[p]
                if not state:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            # (one step counter per group, as torch keeps them in lock-step; parameters that joined later start their own)
            steps = {}
            for p, g in zip(ps, gs):
                state = self.state[p]
                if state["step"].is_cuda:   # (a checkpoint written by torch's fused Adam keeps its counters on the device)
                    state["step"] = state["step"].cpu()
                state["step"] += 1
                steps.setdefault(int(state["step"]), []).append((p, g, state))
            for stepno, items in steps.items():
                for o in range(0, len(items), cap):
                    part = items[o:o + cap]
                    arr = (OptTensor * len(part))()
                    for j, (p, g, state) in enumerate(part):
                        m, v = state["exp_avg"], state["exp_avg_sq"]
                        if not (p.is_contiguous() and m.is_contiguous() and v.is_contiguous()):
                            raise engine.DagnnHipError("ClipAdam needs contiguous parameters")
                        arr[j].param, arr[j].grad, arr[j].exp_avg, arr[j].exp_avg_sq, arr[j].numel = \
                            p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
                    engine.check(lib.dagnn_clip_adam(arr, len(part), float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                                     float(group["weight_decay"]), stepno, float(self.max_norm) if clip else 0.0,
                                                     self._scratch[1].data_ptr() + 4 if clip else None, st), "dagnn_clip_adam")
        # the kernel wrote the parameters through raw pointers: bump their version counters as an in-place torch op would, so
        # that the derived-weight caches (keyed on data_ptr, _version) rebuild and autograd sees the modification
        torch.autograd.graph.increment_version(allp)
        return loss
