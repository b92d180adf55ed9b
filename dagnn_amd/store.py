"""A device-resident store of an ogbg-code2 style dataset: batches collated by one HIP launch.

What the reference does per batch in its loader workers - `augment_edge2` (ogbg-code/utils2.py:31-79) and `add_order_info_01`
(src/utils_dag.py:39-52) per graph, the collation of ogbg-code/tg/dataloader.py:13-35, eleven copies to the device, and in
the evaluation loop the label words of every batch - depends on nothing but the dataset.  `GraphStore` packs all of it once
(vectorised numpy on the host, the layerings by `engine.topo_layers` on the device) and keeps it in device memory as int32
arrays; `store.batch(idx)` is then one small host-to-device copy and one launch of `dagnn_store_gather` (csrc/store.hip), with
no synchronisation, and gives exactly

    GraphBatch.from_data_list([prep(g) for g in idx]).to(device)        prep = clone, augment_edge2, add_order_info_01

plus `len_longest_path`, `y_arr` and the label id sets where the dataset has them.  `gather_host` is the definition the kernel
implements, in numpy; a store on the CPU runs it.

    store = GraphStore.from_graphs(raw_graphs, "cuda", vocab2idx)
    for batch in store.loader(train_ids, 128, shuffle=True, seed=epoch, training=True): ...
    metric = store.evaluate_tok(model, valid_ids, 128)                    # {'precision', 'recall', 'F1', 'n'}
"""
from __future__ import annotations

from typing import Dict, Iterator, Optional, Sequence

import numpy as np
import torch

from . import engine
from .dag_utils import longest_path_layers
from .data import GraphBatch
from .evaluate import SeqF1, encode_ref_sets

__all__ = ["GraphStore", "gather_host"]

REQUIRED = ("x", "node_depth", "edge_index", "node_is_attributed")
PACK_NODE_BUDGET = 1 << 20      # nodes per chunk of the pack step's layering pass (about 100 MB of temporaries)
_I32_MAX = 2 ** 31 - 1


def _get(obj, key):
    return obj.get(key) if isinstance(obj, dict) else getattr(obj, key, None)


def _np64(t, what: str) -> np.ndarray:
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if a.dtype.kind not in "iub":
        raise ValueError("GraphStore: %s must hold integers (got %s)" % (what, a.dtype))
    return a.astype(np.int64, copy=False)


def _i32(a: np.ndarray, what: str) -> np.ndarray:
    if a.size and (int(a.max()) > _I32_MAX or int(a.min()) < -_I32_MAX - 1):
        raise ValueError("GraphStore: a value of %s does not fit int32" % what)
    return np.ascontiguousarray(a, dtype=np.int32)


def _offsets(slices, key: str) -> np.ndarray:
    s = _get(slices, key)
    if s is None:
        raise ValueError("GraphStore: `slices` has no entry for %s" % key)
    return _np64(s, "slices[%s]" % key).reshape(-1)


def _ranges(counts: np.ndarray):
    """(slot of every element, position inside its slot) for consecutive runs of `counts` elements."""
    total = int(counts.sum())
    slot = np.repeat(np.arange(counts.size, dtype=np.int64), counts)
    start = np.cumsum(counts) - counts
    return slot, np.arange(total, dtype=np.int64) - start[slot]


def gather_host(packed: Dict[str, np.ndarray], idx, layers: bool = True) -> Dict[str, np.ndarray]:
    """The definition `dagnn_store_gather` implements, in numpy: the batch of the graphs `idx` (any order, repeats allowed)
    of a packed store, as a dict of arrays under the batch's attribute names (`num_graphs` excepted).  Per graph slot: its
    node rows; its AST edges in stored order, then next-token edge k = (tok[k], tok[k+1]), both shifted by the slot's node
    offset; `edge_attr` rows [0, 0] / [1, 0]; `len_longest_path` = depth_max as float32.  `layers` False leaves the layer
    ids (and `len_longest_path`) out - the pack step gathers before they exist."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    B = idx.size
    node_ptr, edge_ptr, tok_ptr = packed["node_ptr"], packed["edge_ptr"], packed["tok_ptr"]
    n = node_ptr[idx + 1] - node_ptr[idx]
    n_ast = edge_ptr[idx + 1] - edge_ptr[idx]
    n_nxt = np.maximum(tok_ptr[idx + 1] - tok_ptr[idx] - 1, 0)
    ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    slot, local = _ranges(n)
    v = node_ptr[idx][slot] + local
    N = int(ptr[-1])
    out = {"x": packed["x"][v].astype(np.int64).reshape(N, 2), "node_depth": packed["depth"][v].astype(np.int64).reshape(N, 1),
           "batch": slot, "ptr": ptr, "_bi_layer_index0": np.arange(N, dtype=np.int64), "_bi_layer_index1": np.arange(N, dtype=np.int64)}
    eslot, k = _ranges(n_ast + n_nxt)
    is_ast = k < n_ast[eslot]
    u, w = np.empty(k.size, dtype=np.int64), np.empty(k.size, dtype=np.int64)
    e = edge_ptr[idx][eslot[is_ast]] + k[is_ast]
    u[is_ast], w[is_ast] = packed["src"][e], packed["dst"][e]
    nxt = ~is_ast
    p = tok_ptr[idx][eslot[nxt]] + k[nxt] - n_ast[eslot[nxt]]
    u[nxt], w[nxt] = packed["tok"][p], packed["tok"][p + 1]
    out["edge_index"] = np.stack([u, w]).reshape(2, -1) + ptr[eslot][None, :]
    out["edge_attr"] = np.stack([(~is_ast).astype(np.float32), np.zeros(k.size, np.float32)], axis=1)
    if layers:
        out["_bi_layer_idx0"] = packed["layer_f"][v].astype(np.int64)
        out["_bi_layer_idx1"] = packed["layer_b"][v].astype(np.int64)
        out["len_longest_path"] = packed["depth_max"][idx].astype(np.float32)
    if packed.get("y_arr") is not None:
        out["y_arr"] = packed["y_arr"][idx].astype(np.int64)
    if packed.get("ref_ids") is not None:
        out["ref_ids"], out["ref_extra"] = packed["ref_ids"][idx].copy(), packed["ref_extra"][idx].copy()
    return out


class GraphStore(object):
    """The packed dataset (see the module docstring).  `counts`: host int64 [3, G] - nodes, AST edges and attributed nodes per
    graph; `arrays`: the packed arrays on `device` under the names of `dagnn_store_gather_args`."""

    def __init__(self, packed: Dict[str, np.ndarray], device):
        self.device = torch.device(device)
        self.num_graphs = int(packed["node_ptr"].size - 1)
        self.counts = np.stack([np.diff(packed[k]) for k in ("node_ptr", "edge_ptr", "tok_ptr")]).astype(np.int64)
        self._n = self.counts[0]
        self._n_ast = self.counts[1]
        self._n_nxt = np.maximum(self.counts[2] - 1, 0)
        self._extents = np.stack([self._n, self._n_ast, self._n_nxt])   # what a graph adds to a batch: nodes, AST / next-token edges
        self.eos_id: Optional[int] = None
        if self.device.type == "cuda":
            # (arrays the kernel indexes keep at least one element: an empty tensor has no address)
            pad = lambda k, a: np.concatenate([a, np.zeros(1, a.dtype)]) if k in ("src", "dst", "tok") and a.size == 0 else a  # noqa: E731
            self.arrays = {k: torch.from_numpy(pad(k, a)).to(self.device) for k, a in packed.items() if a is not None}
            self._layer_device()
        else:
            self._layer_host(packed)
            self.arrays = {k: torch.from_numpy(a) for k, a in packed.items() if a is not None}
        self._host = packed if self.device.type != "cuda" else None

    # ------------------------------------------------------------------------- construction
    @classmethod
    def from_graphs(cls, graphs: Sequence, device, vocab2idx: Optional[Dict[str, int]] = None) -> "GraphStore":
        """Pack a list of raw graphs (as they are BEFORE `augment_edge2`): `x` [n, 2], `node_depth` [n, 1], `edge_index`
        [2, a] (the AST edges), `node_is_attributed` [n, 1], optionally `y_arr` [1, S] and `y` (label words; needs
        `vocab2idx`)."""
        graphs = list(graphs)
        if not graphs:
            raise ValueError("GraphStore.from_graphs: no graph")
        keys = list(REQUIRED) + (["y_arr"] if _get(graphs[0], "y_arr") is not None else [])
        cols = {k: [] for k in keys}
        for i, g in enumerate(graphs):
            for k in keys:
                t = _get(g, k)
                if t is None:
                    raise ValueError("GraphStore.from_graphs: graph %d has no attribute %s" % (i, k))
                cols[k].append(t)
        has_y = _get(graphs[0], "y") is not None
        if has_y and any(_get(g, "y") is None for g in graphs):
            raise ValueError("GraphStore.from_graphs: some graphs carry label words `y`, others do not")
        data = {k: torch.cat([torch.as_tensor(t) for t in v], dim=1 if k == "edge_index" else 0) for k, v in cols.items()}
        nodes = np.array([0] + [int(torch.as_tensor(t).shape[0]) for t in cols["x"]], dtype=np.int64).cumsum()
        slices = {k: torch.from_numpy(nodes) for k in ("x", "node_depth", "node_is_attributed")}
        slices["edge_index"] = torch.from_numpy(
            np.array([0] + [int(torch.as_tensor(t).shape[1]) for t in cols["edge_index"]], dtype=np.int64).cumsum())
        if has_y:
            data["y"] = [_get(g, "y") for g in graphs]
        return cls.from_slices(data, slices, device, vocab2idx)

    @classmethod
    def from_slices(cls, data, slices, device, vocab2idx: Optional[Dict[str, int]] = None) -> "GraphStore":
        """Pack the PyG in-memory form: `data` holds the graphs' tensors concatenated (`edge_index` along dim 1 with node ids
        inside each graph, `y_arr` [G, S], `y` a list of G word lists), `slices` the [G + 1] offsets of `x` and
        `edge_index`."""
        for k in REQUIRED:
            if _get(data, k) is None:
                raise ValueError("GraphStore: the dataset has no attribute %s" % k)
        node_ptr, edge_ptr = _offsets(slices, "x"), _offsets(slices, "edge_index")
        G = node_ptr.size - 1
        x = _np64(_get(data, "x"), "x")
        ei = _np64(_get(data, "edge_index"), "edge_index")
        depth = _np64(_get(data, "node_depth"), "node_depth").reshape(-1)
        attributed = _np64(_get(data, "node_is_attributed"), "node_is_attributed").reshape(-1)
        n, n_ast = np.diff(node_ptr), np.diff(edge_ptr)
        if G < 1 or edge_ptr.size != G + 1 or node_ptr[0] != 0 or edge_ptr[0] != 0 or (n < 0).any() or (n_ast < 0).any():
            raise ValueError("GraphStore: `slices` must hold G + 1 ascending offsets from 0 for x and edge_index")
        Nt, Et = int(node_ptr[-1]), int(edge_ptr[-1])
        if x.ndim != 2 or x.shape != (Nt, 2) or depth.size != Nt or attributed.size != Nt or ei.ndim != 2 or ei.shape != (2, Et):
            raise ValueError("GraphStore: x [N, 2], node_depth [N, 1], node_is_attributed [N, 1], edge_index [2, E] needed "
                             "for N = %d, E = %d (got %s, %s, %s, %s)" % (Nt, Et, x.shape, depth.shape, attributed.shape, ei.shape))
        if max(int(n.max()), int(n_ast.max())) > _I32_MAX:
            raise ValueError("GraphStore: a graph's node or edge count does not fit int32")
        egraph = np.repeat(np.arange(G, dtype=np.int64), n_ast)
        if Et and ((ei < 0).any() or (ei >= n[egraph][None, :]).any()):
            raise ValueError("GraphStore: edge_index must hold node ids inside each graph, 0 .. n - 1")
        pos = np.flatnonzero(attributed == 1)
        tgraph = np.searchsorted(node_ptr, pos, side="right") - 1
        tok_ptr = np.concatenate([[0], np.cumsum(np.bincount(tgraph, minlength=G))]).astype(np.int64)
        packed = {"node_ptr": node_ptr, "edge_ptr": edge_ptr, "tok_ptr": tok_ptr, "x": _i32(x, "x"),
                  "depth": _i32(depth, "node_depth"), "layer_f": np.zeros(Nt, np.int32), "layer_b": np.zeros(Nt, np.int32),
                  "src": _i32(ei[0], "edge_index"), "dst": _i32(ei[1], "edge_index"),
                  "tok": (pos - node_ptr[tgraph]).astype(np.int32), "depth_max": np.zeros(G, np.int32),
                  "y_arr": None, "ref_ids": None, "ref_extra": None}
        y_arr, y = _get(data, "y_arr"), _get(data, "y")
        if y_arr is not None:
            y_arr = _np64(y_arr, "y_arr")
            if y_arr.ndim != 2 or y_arr.shape[0] != G or y_arr.shape[1] < 1:
                raise ValueError("GraphStore: y_arr [G, S] needed for G = %d (got %s)" % (G, y_arr.shape))
            packed["y_arr"] = _i32(y_arr, "y_arr")
        if y is not None:
            if vocab2idx is None:
                raise ValueError("GraphStore: label words `y` need `vocab2idx`")
            if len(y) != G:
                raise ValueError("GraphStore: %d label word lists for %d graphs" % (len(y), G))
            ref_ids, ref_extra = encode_ref_sets(y, vocab2idx)   # (the evaluation loop's host work, once for the dataset)
            packed["ref_ids"], packed["ref_extra"] = ref_ids.numpy(), ref_extra.numpy()
        store = cls(packed, device)
        store.eos_id = len(vocab2idx) - 1 if vocab2idx is not None else None
        return store

    # ------------------------------------------------------------------------- layerings of the augmented graphs
    def _layer_host(self, packed) -> None:
        node_ptr, edge_ptr, tok_ptr = packed["node_ptr"], packed["edge_ptr"], packed["tok_ptr"]
        for g in range(self.num_graphs):
            tok = packed["tok"][tok_ptr[g]:tok_ptr[g + 1]]
            e0, e1 = edge_ptr[g], edge_ptr[g + 1]
            ei = np.stack([np.concatenate([packed["src"][e0:e1], tok[:-1]]), np.concatenate([packed["dst"][e0:e1], tok[1:]])])
            n = int(self._n[g])
            v0 = node_ptr[g]
            try:
                packed["layer_f"][v0:v0 + n] = longest_path_layers(ei, n)
                packed["layer_b"][v0:v0 + n] = longest_path_layers(ei[::-1], n)
            except ValueError as exc:
                raise ValueError("GraphStore: graph %d: %s" % (g, exc)) from exc
            packed["depth_max"][g] = packed["layer_f"][v0:v0 + n].max() if n else 0

    def _layer_device(self) -> None:
        """Chunks of the store (consecutive graphs, at most PACK_NODE_BUDGET nodes unless one graph alone has more) are
        gathered without layer outputs and layered by `engine.topo_layers`; the cycle status is read ONCE, at the end."""
        node_ptr = np.concatenate([[0], np.cumsum(self._n)])
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        g0 = 0
        while g0 < self.num_graphs:
            g1 = int(np.searchsorted(node_ptr, node_ptr[g0] + PACK_NODE_BUDGET, side="right")) - 1
            g1 = min(max(g1, g0 + 1), self.num_graphs)
            out = self._gather(np.arange(g0, g1, dtype=np.int64), layers=False)
            lf, lb, st = engine.topo_layers(out["edge_index"], out["batch"], g1 - g0)
            v0, v1 = int(node_ptr[g0]), int(node_ptr[g1])
            self.arrays["layer_f"][v0:v1] = lf
            self.arrays["layer_b"][v0:v1] = lb
            self.arrays["depth_max"][g0:g1] = engine.graph_depth(lf, out["batch"], g1 - g0)
            status |= st
            g0 = g1
        if int(status):
            raise ValueError("GraphStore: a graph of the dataset has a cycle")

    # ------------------------------------------------------------------------- batches
    def _ids(self, idx) -> np.ndarray:
        if isinstance(idx, torch.Tensor):
            if idx.is_cuda:
                raise ValueError("GraphStore.batch: graph ids must be on the host (a list, a numpy array or a CPU tensor)")
            idx = idx.numpy()
        idx = np.asarray(idx)
        if idx.size == 0:
            raise ValueError("GraphStore.batch: no graph ids")
        if idx.dtype.kind not in "iu":
            raise ValueError("GraphStore.batch: graph ids must be integers (got %s)" % idx.dtype)
        idx = idx.reshape(-1).astype(np.int64, copy=False)
        if int(idx.min()) < 0 or int(idx.max()) >= self.num_graphs:
            raise ValueError("GraphStore.batch: graph id outside [0, %d)" % self.num_graphs)
        return idx

    def _gather(self, idx: np.ndarray, layers: bool = True) -> Dict[str, torch.Tensor]:
        """The GPU path: ids and the [3, B + 1] offsets in one fresh pinned buffer (torch's caching host allocator keeps a
        block away from reuse until the copy that reads it has run), one non-blocking copy, one launch."""
        B = idx.size
        stage = torch.empty((4, B + 1), dtype=torch.int64, pin_memory=True)
        tab = stage.numpy()
        tab[0, :B] = idx
        tab[0, B] = 0
        tab[1:, 0] = 0
        np.cumsum(self._extents[:, idx], axis=1, out=tab[1:, 1:])
        N, E = int(tab[1, B]), int(tab[2, B] + tab[3, B])
        table = stage.to(self.device, non_blocking=True)
        return engine.store_gather(self.arrays, table, B, N, E, layers=layers, llp=layers, labels=layers, refs=layers)

    def batch(self, idx) -> GraphBatch:
        """The batch of the graphs `idx` (a list, a numpy array or a CPU tensor of ids; any order, repeats allowed), every
        tensor freshly allocated on the store's device.  `ValueError` for no id or an id outside the store, before anything
        is launched."""
        idx = self._ids(idx)
        if self.device.type == "cuda":
            out = self._gather(idx)
        else:
            out = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in gather_host(self._host, idx).items()}
        b = GraphBatch()
        for k, v in out.items():
            b[k] = v
        b.num_graphs = int(idx.size)
        return b

    def loader(self, idx, batch_size: int, shuffle: bool = False, seed: int = 0, training: bool = False) -> Iterator[GraphBatch]:
        """One pass over the graphs `idx` in batches of `batch_size` (the last one may be short), in the reference's loader
        order: as given, or - `shuffle` - permuted by `torch.randperm` of a host generator seeded with `seed`.  The
        reference's filters, from the host counts: a batch with ONE node is skipped; `training` also skips a batch with ONE
        graph (main_pyg.py:47,99; `lp.lp_batches`)."""
        ids = self._ids(idx)
        if int(batch_size) < 1:
            raise ValueError("GraphStore.loader: batch_size must be positive")
        if shuffle:
            ids = ids[torch.randperm(ids.size, generator=torch.Generator().manual_seed(int(seed))).numpy()]
        for i in range(0, ids.size, int(batch_size)):
            chunk = ids[i:i + int(batch_size)]
            if int(self._n[chunk].sum()) == 1 or (training and chunk.size == 1):
                continue
            yield self.batch(chunk)

    def evaluate_tok(self, model, idx, batch_size: int, loss: bool = False) -> dict:
        """The loop of `evaluate.evaluate` (ogbg-code/main_pyg.py:91-124) over the graphs `idx`, fed by the store: `predict`
        and `SeqF1.update` on the batch's own `ref_ids` / `ref_extra` - no host string work and no copy of reference sets
        per batch - and one synchronisation, in `compute()`.  One-node batches are skipped as the reference skips them.
        `loss=True`: the passes are `score(batch, batch.y_arr)` and the dict gains 'loss', the float64 sum of all row losses
        divided by (graphs * S), as in `evaluate.evaluate`."""
        if "ref_ids" not in self.arrays or self.eos_id is None:
            raise ValueError("GraphStore.evaluate_tok: the store was packed without label words and vocab2idx")
        if loss and "y_arr" not in self.arrays:
            raise ValueError("GraphStore.evaluate_tok: the store was packed without y_arr")
        from .evaluate import SeqLoss, _with_loss
        was_training = model.training
        model.eval()
        metric = SeqF1(self.eos_id)
        acc = SeqLoss(self.device) if loss else None
        try:
            for batch in self.loader(idx, batch_size):
                ref_ids, ref_extra = batch.ref_ids, batch.ref_extra   # (before the pass, which may rewrite the batch)
                if loss:
                    metric.update(model.score(batch, batch.y_arr, sums=acc).tok[:, :, 0], ref_ids, ref_extra)
                else:
                    metric.update(model.predict(batch), ref_ids, ref_extra)
        finally:
            if was_training:
                model.train()
        return _with_loss(metric, acc)

    # ------------------------------------------------------------------------- the training epoch
    def _train_epoch(self, what: str, model, optimizer, idx, batch_size: int, clip: float, seed: Optional[int], eos_id: Optional[int],
                     step):
        from .train import ClipAdam, EpochMeter
        clip = float(clip or 0.0)
        if clip > 0 and isinstance(optimizer, ClipAdam):
            raise ValueError("GraphStore.%s: a ClipAdam optimizer clips through its own `max_norm`; pass clip=0" % what)
        ids = self._ids(idx)
        if int(batch_size) < 1:
            raise ValueError("GraphStore.%s: batch_size must be positive" % what)
        chunks = -(-ids.size // int(batch_size))   # every chunk of the loader, skipped ones included: the reference's `step + 1`
        meter = EpochMeter(self.device, ids.size, eos_id)
        model.train()
        for batch in self.loader(ids, batch_size, shuffle=seed is not None, seed=0 if seed is None else int(seed), training=True):
            loss = step(batch, meter)   # (forward, `optimizer.zero_grad()`, the fused loss: the reference's order)
            loss.backward()
            if clip > 0:
                torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
            optimizer.step()
        return meter.result(chunks)

    def train_tok(self, model, optimizer, idx, batch_size: int, clip: float = 0.0, seed: Optional[int] = None):
        """One epoch of the reference's `train()` for the TOK task (ogbg-code/main_pyg.py:39-88) over the graphs `idx`, fed by
        the store -> (mean loss, {'precision', 'recall', 'F1', 'n'} of the training predictions).  `model.train()`; batches of
        `self.loader(idx, batch_size, shuffle=seed is not None, seed=seed, training=True)`; per batch forward,
        `optimizer.zero_grad()`, `train.seq_ce_step` on the batch's own `y_arr` / `ref_ids` / `ref_extra`, `backward()`,
        `clip_grad_norm_(model.parameters(), clip)` when `clip` > 0, `optimizer.step()`.  The loss launch also leaves the step's
        tokens, F1 counts and `loss_accum += loss.item()` on the device, so nothing synchronises inside the loop; the epoch
        ends with one read.  The mean loss is the sum / the number of chunks of the loader, skipped one-graph and one-node
        chunks included (the reference's `loss_accum / (step + 1)`).  With a `train.ClipAdam` optimizer clip through its
        `max_norm`: `clip` > 0 then raises `ValueError`.  The model is left in training mode, as the reference leaves it."""
        from .train import seq_ce_step
        if "y_arr" not in self.arrays:
            raise ValueError("GraphStore.train_tok: the store was packed without y_arr")
        if "ref_ids" not in self.arrays or self.eos_id is None:
            raise ValueError("GraphStore.train_tok: the store was packed without label words and vocab2idx")

        def step(batch, meter):
            y_arr, ref_ids, ref_extra = batch.y_arr, batch.ref_ids, batch.ref_extra   # (before the pass, which may rewrite the batch)
            pred_list = model(batch)
            optimizer.zero_grad()
            return seq_ce_step(pred_list, y_arr, meter, ref_ids, ref_extra)

        return self._train_epoch("train_tok", model, optimizer, idx, batch_size, clip, seed, self.eos_id, step)

    def train_lp(self, model, optimizer, idx, batch_size: int, clip: float = 0.0, seed: Optional[int] = None):
        """`train_tok` for the LP task (ogbg-code/main_pyg_lp.py:43-74) -> (mean loss, {'acc', 'n'}): the targets are the
        batch's `len_longest_path`, the loss launch is `lp.class_ce_step`."""
        from .lp import class_ce_step
        if "y_arr" not in self.arrays:
            raise ValueError("GraphStore.train_lp: the store was packed without y_arr")

        def step(batch, meter):
            targ = batch.len_longest_path   # (before the pass, which may rewrite the batch)
            pred = model(batch)
            optimizer.zero_grad()
            return class_ce_step(pred, targ, meter)

        return self._train_epoch("train_lp", model, optimizer, idx, batch_size, clip, seed, None, step)
