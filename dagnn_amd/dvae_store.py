"""A device-resident store of a D-VAE data set (ENAS / BN graphs): batches collated by one HIP launch.

What the reference does per batch on the host - `_collate_fn`'s deep copies (models_pyg.py:114-115), `Batch.from_data_list`
(dvae/batch.py:26-146) over the graphs that `decode_ENAS_to_pygraph` / `decode_BN_to_pygraph` (dvae/util.py:290-385) made,
the copies of the batch to the device, and in `loss()` the walk over every vertex of every graph for the decoder's schedule
(models_pyg.py:405-420) - depends on nothing but the data set.  The graphs are dense by construction: exactly n vertices
each (8 ENAS, 10 BN), every edge from a lower to a higher vertex.  `DagStore` packs them once (vectorised numpy on the
host, the layerings by `dagnn_dag_store_layers` on the device) into int32 [M, n] arrays in device memory - types,
predecessor masks, successor masks, the two layerings; `store.batch(idx)` is then one small host-to-device copy and one
launch of `dagnn_dag_store_gather` (csrc/dvae_store.hip), with no synchronisation, and gives exactly

    GraphBatch.from_data_list([g_i.clone() for i in idx]).to(device)        g_i = the decoded graph of row i, without `vs`

plus the decoder's schedule `types` / `preds` [B, n] int32 (what `decode_schedule` builds per call) and `y` [B] where the
store has it.  `gather_host` is the definition the kernel implements, in numpy; a store on the CPU runs it.

    store = DagStore.from_rows(rows, "ENAS", nvt=8, device="cuda", y=accuracies)
    for epoch in range(E):
        loss, recon, kld = train_epoch(model, optimizer, store, train_ids, 32, seed=epoch)
    nll = test_nll(model, store, test_ids, 64)
    # with `predictor.attach_predictor(model)`: train_epoch(..., predictor=True) -> (loss, recon, kld, pred); test_predictor(...)
    Z = extract_latent(model, (store, train_ids), 64)
"""
from __future__ import annotations

import ast
import itertools
from typing import Dict, Iterator, Optional, Sequence

import numpy as np
import torch

from . import engine
from .data import GraphBatch
from .dvae import GraphSet, dense_rows

__all__ = ["DagStore", "gather_host", "layers_host", "train_epoch", "test_nll", "test_predictor"]

MAX_N = 32
BATCH_KEYS = ("x", "edge_index", "bi_layer_index", "batch", "ptr", "types", "preds")


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint32)


def _popcount_rows(masks: np.ndarray) -> np.ndarray:
    """Set bits per row of a [M, n] array of 32-bit words, int64 [M]."""
    m = _u32(masks)
    return np.unpackbits(m.view(np.uint8).reshape(m.shape[0], -1), axis=1).sum(axis=1, dtype=np.int64)


def transpose_masks(preds: np.ndarray) -> np.ndarray:
    """succs [M, n] of preds [M, n] (words taken as unsigned): bit v of succs[:, u] = bit u of preds[:, v]."""
    p = _u32(preds)
    M, n = p.shape
    s = np.zeros((M, n), dtype=np.uint32)
    for v in range(n):
        for u in range(n):
            s[:, u] |= ((p[:, v] >> np.uint32(u)) & np.uint32(1)) << np.uint32(v)
    return s.view(np.int32)


def layers_host(preds: np.ndarray, succs: np.ndarray):
    """The numpy mirror of `dagnn_dag_store_layers`: layer_f[v] = 1 + max(layer_f[u]) over the predecessors u < v of v (0
    without one), walking v ascending; layer_b the same over succs, descending.  int32 [M, n] each."""
    p, s = _u32(preds), _u32(succs)
    M, n = p.shape
    lf, lb = np.zeros((M, n), dtype=np.int32), np.zeros((M, n), dtype=np.int32)
    for v in range(n):
        for u in range(v):
            bit = ((p[:, v] >> np.uint32(u)) & np.uint32(1)).astype(bool)
            lf[:, v] = np.maximum(lf[:, v], np.where(bit, lf[:, u] + 1, 0))
    for u in range(n - 1, -1, -1):
        for v in range(u + 1, n):
            bit = ((s[:, u] >> np.uint32(v)) & np.uint32(1)).astype(bool)
            lb[:, u] = np.maximum(lb[:, u], np.where(bit, lb[:, v] + 1, 0))
    return lf, lb


def gather_host(packed: Dict[str, np.ndarray], idx, nvt: int) -> Dict[str, np.ndarray]:
    """The definition `dagnn_dag_store_gather` implements, in numpy: the batch of the graphs `idx` (any order, repeats
    allowed) of a packed store, as a dict of arrays under the batch's attribute names (`num_graphs` excepted).  Graph slot
    b owns nodes [b n, (b + 1) n); its edges come source-major - source ascending, then target ascending, the order
    `networkx.DiGraph(adj).edges` gives the reference's decoders - shifted by b n."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    B, n = idx.size, packed["types"].shape[1]
    N = B * n
    types = packed["types"][idx]
    x = np.zeros((N, int(nvt)), dtype=np.float32)
    x[np.arange(N), types.reshape(-1)] = 1.0
    bits = (_u32(packed["succs"][idx])[:, :, None] >> np.arange(n, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    b, u, v = np.nonzero(bits)     # (row-major: slot, then source, then target)
    ids = np.arange(N, dtype=np.int64)
    out = {"x": x, "edge_index": np.stack([b * n + u, b * n + v]).astype(np.int64).reshape(2, -1),
           "bi_layer_index": np.stack([np.stack([packed["layer_f"][idx].reshape(-1).astype(np.int64), ids]),
                                       np.stack([packed["layer_b"][idx].reshape(-1).astype(np.int64), ids])]),
           "batch": np.repeat(np.arange(B, dtype=np.int64), n), "ptr": np.arange(B + 1, dtype=np.int64) * n,
           "types": types.copy(), "preds": packed["preds"][idx].copy()}
    if packed.get("y") is not None:
        out["y"] = packed["y"][idx].astype(np.float32)
    return out


# --------------------------------------------------------------------------------- rows -> dense graphs
def _parse_rows(rows) -> list:
    rows = list(rows)
    if rows and all(isinstance(r, str) for r in rows):   # (one parse of the whole file's lines)
        rows = ast.literal_eval("[" + ",".join(rows) + "]")
    elif any(isinstance(r, str) for r in rows):
        rows = [ast.literal_eval(r) if isinstance(r, str) else r for r in rows]
    return rows


def rows_to_dense(rows, kind: str, start_type: int = 0, end_type: int = 1):
    """(types, preds) int32 [M, n] of rows in the reference's format - row = [[type, c_0 .. c_{i-1}] for node i = 0 .. n-3],
    lists or their strings - as `decode_ENAS_to_pygraph` / `decode_BN_to_pygraph` (dvae/util.py:290-385) decode them, in
    numpy over all rows at once: vertex 0 has `start_type`, vertex i + 1 type row[i][0] + 2, the last vertex `end_type`.
    ENAS: the chain i -> i + 1 and the edge j -> i + 1 where c_j == 1.  BN: c_j == 1 is the edge j + 1 -> i + 1, a node
    whose c sum to 0 hangs off vertex 0, and every middle vertex that is nobody's parent feeds the last vertex."""
    if kind not in ("ENAS", "BN"):
        raise ValueError("DagStore.from_rows: kind must be 'ENAS' or 'BN' (got %r)" % (kind,))
    rows = _parse_rows(rows)
    M = len(rows)
    if M == 0:
        raise ValueError("DagStore.from_rows: no row")
    try:
        k = len(rows[0])
        row_len = np.fromiter(map(len, rows), dtype=np.int64, count=M)
        node_len = np.fromiter(map(len, itertools.chain.from_iterable(rows)), dtype=np.int64)
    except TypeError as exc:
        raise ValueError("DagStore.from_rows: a row must be a list of per-node lists (%s)" % exc) from exc
    n = k + 2
    if k < 1 or n > MAX_N:
        raise ValueError("DagStore.from_rows: rows of 1 .. %d nodes are possible (n = nodes + 2 <= %d; got %d)" % (MAX_N - 2, MAX_N, k))
    if (row_len != k).any():
        raise ValueError("DagStore.from_rows: every graph must have exactly n = %d vertices (row %d has %d nodes, row 0 has %d)"
                         % (n, int(np.flatnonzero(row_len != k)[0]), int(row_len[np.flatnonzero(row_len != k)[0]]), k))
    if node_len.size != M * k or (node_len.reshape(M, k) != 1 + np.arange(k)[None, :]).any():
        raise ValueError("DagStore.from_rows: node i of a row must be [type, c_0 .. c_{i-1}] (1 + i entries)")
    flat = np.fromiter(itertools.chain.from_iterable(itertools.chain.from_iterable(rows)), dtype=np.int64,
                       count=M * (k * (k + 1) // 2)).reshape(M, -1)
    first = np.arange(k) * (np.arange(k) + 1) // 2          # where node i starts: sum of 1 + j over j < i
    types = np.empty((M, n), dtype=np.int64)
    types[:, 0], types[:, n - 1] = start_type, end_type
    types[:, 1:n - 1] = flat[:, first] + 2
    preds = np.zeros((M, n), dtype=np.uint32)
    one = np.uint32(1)
    if kind == "ENAS":
        for i in range(k):
            preds[:, i + 1] |= one << np.uint32(i)
            for j in range(i):
                preds[:, i + 1] |= (flat[:, first[i] + 1 + j] == 1).astype(np.uint32) << np.uint32(j)
        preds[:, n - 1] |= one << np.uint32(k)
    else:
        loose = np.ones((M, k), dtype=bool)
        for i in range(k):
            c = flat[:, first[i] + 1:first[i] + 1 + i]
            orphan = c.sum(axis=1) == 0
            preds[:, i + 1] |= orphan.astype(np.uint32)
            for j in range(i):
                e = (c[:, j] == 1) & ~orphan
                preds[:, i + 1] |= e.astype(np.uint32) << np.uint32(j + 1)
                loose[:, j] &= ~e
        for j in range(k):
            preds[:, n - 1] |= loose[:, j].astype(np.uint32) << np.uint32(j + 1)
    if int(types.max()) > np.iinfo(np.int32).max or int(types.min()) < np.iinfo(np.int32).min:
        raise ValueError("DagStore.from_rows: a vertex type does not fit int32")
    return types.astype(np.int32), preds.view(np.int32)


class DagStore(object):
    """The packed data set (see the module docstring).  `arrays`: types / preds / succs / layer_f / layer_b int32 [M, n] and
    - when given - y fp32 [M], on `device`; `edge_count`: host int64 [M]: every size a batch needs comes from the host."""

    def __init__(self, types, preds, nvt: int, device, y=None, start_type: int = 0):
        types, preds = np.asarray(types), np.asarray(preds)
        if types.ndim != 2 or types.shape != preds.shape or types.shape[0] < 1 or types.shape[1] < 1:
            raise ValueError("DagStore: types and preds [M >= 1, n >= 1] needed (got %s, %s)" % (types.shape, preds.shape))
        M, n = types.shape
        if n > MAX_N:
            raise ValueError("DagStore: at most %d vertices per graph (got n=%d)" % (MAX_N, n))
        if types.dtype.kind not in "iu" or preds.dtype.kind not in "iu":
            raise ValueError("DagStore: types and preds must hold integers (got %s, %s)" % (types.dtype, preds.dtype))
        nvt = int(nvt)
        if nvt < 1:
            raise ValueError("DagStore: nvt must be positive (got %d)" % nvt)
        if int(types.min()) < 0 or int(types.max()) >= nvt:
            g, v = (int(a[0]) for a in np.nonzero((types < 0) | (types >= nvt)))
            raise ValueError("DagStore: vertex types must lie in [0, nvt=%d) (vertex %d of graph %d has %d; a graph of fewer "
                             "than n=%d vertices cannot be packed: every graph must have exactly n vertices)"
                             % (nvt, v, g, int(types[g, v]), n))
        if (types[:, 1:] == start_type).any():
            g, v = (int(a[0]) for a in np.nonzero(types[:, 1:] == start_type))
            raise ValueError("DagStore: vertex %d of graph %d has START_TYPE=%d, which only vertex 0 may have (the reference "
                             "treats it as padding and skips the vertex)" % (v + 1, g, start_type))
        if preds.dtype.itemsize != 4:   # (wider words: the value must be a 32-bit mask)
            wide = preds.astype(np.int64)
            if int(wide.min()) < -(1 << 31) or int(wide.max()) >= (1 << 32):
                raise ValueError("DagStore: predecessor masks must be 32-bit words")
            preds = (wide & 0xFFFFFFFF).astype(np.uint32)
        preds = _u32(preds)
        below = np.array([(1 << v) - 1 for v in range(n)], dtype=np.uint32)   # word v may hold bits u < v only
        if (preds & ~below[None, :]).any():
            g, v = (int(a[0]) for a in np.nonzero(preds & ~below[None, :]))
            raise ValueError("DagStore: vertex %d of graph %d has a predecessor u >= v (mask 0x%x): edges must go from a lower "
                             "to a higher vertex" % (v, g, int(preds[g, v])))
        self.device = torch.device(device)
        self.num_graphs, self.n, self.nvt, self.start_type = M, n, nvt, int(start_type)
        self.edge_count = _popcount_rows(preds)
        packed = {"types": np.ascontiguousarray(types, dtype=np.int32), "preds": preds.view(np.int32).copy(),
                  "succs": transpose_masks(preds), "y": None}
        if y is not None:
            y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
            if y.reshape(-1).size != M:
                raise ValueError("DagStore: y must hold one value per graph (got %s for %d graphs)" % (y.shape, M))
            packed["y"] = np.ascontiguousarray(y.reshape(-1), dtype=np.float32)
        if self.device.type == "cuda":
            self.arrays = {k: torch.from_numpy(a).to(self.device) for k, a in packed.items() if a is not None}
            self.arrays["layer_f"], self.arrays["layer_b"] = engine.dag_store_layers(self.arrays["preds"], self.arrays["succs"])
            self._host = None
        else:
            packed["layer_f"], packed["layer_b"] = layers_host(packed["preds"], packed["succs"])
            self.arrays = {k: torch.from_numpy(a) for k, a in packed.items() if a is not None}
            self._host = packed

    # ------------------------------------------------------------------------- construction
    @classmethod
    def from_dense(cls, types, preds, nvt: int, device, y=None, start_type: int = 0) -> "DagStore":
        """From dense rows as `decode_schedule` / `dense_rows` describe them: types [M, n] and predecessor masks [M, n]
        (bit u of preds[g, v]: the edge u -> v), numpy arrays or tensors."""
        h = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)   # noqa: E731
        return cls(h(types), h(preds), nvt, device, y, start_type)

    @classmethod
    def from_rows(cls, rows, kind: str, nvt: int, device, y=None, start_type: int = 0, end_type: int = 1) -> "DagStore":
        """From rows of the reference's data files (`kind` 'ENAS' or 'BN'; lists, or the strings of such lists, which are
        parsed as literals, never evaluated).  `nvt` counts the start and end types."""
        types, preds = rows_to_dense(rows, kind, start_type, end_type)
        return cls(types, preds, nvt, device, y, start_type)

    @classmethod
    def from_graphs(cls, graphs: Sequence, max_n: int, nvt: int, device, y=None, start_type: int = 0) -> "DagStore":
        """From graph objects (what `encode` / `loss` take: `x`, `edge_index`, `vs`), every one of exactly max_n vertices.
        A batch lists a graph's edges source-major whatever order its `edge_index` had."""
        graphs = list(graphs)
        if not graphs:
            raise ValueError("DagStore.from_graphs: no graph")
        types, preds, nv = dense_rows(graphs, max_n, nvt)
        if (nv != max_n).any():
            g = int(np.flatnonzero(nv != max_n)[0])
            raise ValueError("DagStore.from_graphs: every graph must have exactly max_n=%d vertices (graph %d has %d)"
                             % (max_n, g, int(nv[g])))
        edges = np.array([int(g.edge_index.shape[1]) for g in graphs], dtype=np.int64)
        if (edges != _popcount_rows(preds)).any():   # (`dense_rows` keeps the edges u < v only, each once)
            g = int(np.flatnonzero(edges != _popcount_rows(preds))[0])
            raise ValueError("DagStore.from_graphs: graph %d has an edge u -> v with u >= v, or one edge twice" % g)
        return cls(types, preds, nvt, device, y, start_type)

    # ------------------------------------------------------------------------- batches
    def _ids(self, idx) -> np.ndarray:
        if isinstance(idx, torch.Tensor):
            if idx.is_cuda:
                raise ValueError("DagStore.batch: graph ids must be on the host (a list, a numpy array or a CPU tensor)")
            idx = idx.numpy()
        idx = np.asarray(idx)
        if idx.size == 0:
            raise ValueError("DagStore.batch: no graph ids")
        if idx.dtype.kind not in "iu":
            raise ValueError("DagStore.batch: graph ids must be integers (got %s)" % idx.dtype)
        idx = idx.reshape(-1).astype(np.int64, copy=False)
        if int(idx.min()) < 0 or int(idx.max()) >= self.num_graphs:
            raise ValueError("DagStore.batch: graph id outside [0, %d)" % self.num_graphs)
        return idx

    def _gather(self, idx: np.ndarray) -> Dict[str, torch.Tensor]:
        """The GPU path: ids and edge offsets in one fresh pinned [2, B + 1] table (torch's caching host allocator keeps a
        block away from reuse until the copy that reads it has run), one non-blocking copy, one launch."""
        B = idx.size
        stage = torch.empty((2, B + 1), dtype=torch.int64, pin_memory=True)
        tab = stage.numpy()
        tab[0, :B] = idx
        tab[0, B] = 0
        tab[1, 0] = 0
        np.cumsum(self.edge_count[idx], out=tab[1, 1:])
        E = int(tab[1, B])
        table = stage.to(self.device, non_blocking=True)
        return engine.dag_store_gather(self.arrays, table, B, E, self.nvt)

    def batch(self, idx) -> GraphBatch:
        """The batch of the graphs `idx` (a list, a numpy array or a CPU tensor of ids; any order, repeats allowed), every
        tensor freshly allocated on the store's device: x, edge_index, bi_layer_index, batch, ptr, num_graphs, and the
        decoder's schedule types / preds (and y).  `ValueError` for no id or an id outside the store, before anything is
        launched."""
        idx = self._ids(idx)
        if self.device.type == "cuda":
            out = self._gather(idx)
        else:
            out = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in gather_host(self._host, idx, self.nvt).items()}
        b = GraphBatch()
        for k, v in out.items():
            b[k] = v
        b.num_graphs = int(idx.size)
        return b

    def loader(self, idx, batch_size: int, shuffle: bool = False, seed: int = 0) -> Iterator[GraphBatch]:
        """One pass over the graphs `idx` in batches of `batch_size`, the last one short when they do not divide
        (dvae/train.py:233), in the order given or - `shuffle` - permuted by `torch.randperm` of a host generator seeded
        with `seed` (the rule of `GraphStore.loader`)."""
        ids = self._ids(idx)
        if int(batch_size) < 1:
            raise ValueError("DagStore.loader: batch_size must be positive")
        if shuffle:
            ids = ids[torch.randperm(ids.size, generator=torch.Generator().manual_seed(int(seed))).numpy()]
        for i in range(0, ids.size, int(batch_size)):
            yield self.batch(ids[i:i + int(batch_size)])

    def graph_set(self) -> GraphSet:
        """The GraphSet of the packed rows (`prior_validity`'s training set), on the store's device."""
        return GraphSet.from_dense(self.arrays["types"], self.arrays["preds"])


# --------------------------------------------------------------------------------- the loops of dvae/train.py
def train_epoch(model, optimizer, store: DagStore, idx, batch_size: int, clip: float = 0.0, beta: float = 0.005,
                seed: Optional[int] = None, predictor: bool = False):
    """`train()` of dvae/train.py:218-273 over the graphs `idx` of a store: per batch zero_grad, `encode_batch`, `loss_dense`,
    backward, `clip_grad_norm_` when clip > 0, step.  `seed` None keeps the order of `idx`; a number shuffles it as
    `store.loader` does (the reference shuffles its list every epoch).  Returns the sums (loss, recon, kld) over the batches
    as floats - added up on the device and read once, at the end.

    `predictor` True is the reference's `--predictor` branch (train.py:243-250, 262-263): every batch adds
    `predictor_mse(model, mu, b.y)[0]` - the summed squared error of `model.predictor` (see `predictor.attach_predictor`)
    against the graphs' scores - to the loss before backward, and the call returns the four sums (loss, recon, kld, pred)
    of train.py:272.  A store without `y` raises ValueError."""
    if predictor:
        from .predictor import _predictor_of, predictor_mse
        if "y" not in store.arrays:
            raise ValueError("train_epoch(predictor=True): the store holds no y (pass y= to DagStore)")
        _predictor_of(model, "train_epoch(predictor=True)")
    model.train()
    sums = None
    for b in store.loader(idx, batch_size, shuffle=seed is not None, seed=0 if seed is None else seed):
        optimizer.zero_grad()
        types, preds = b.types, b.preds
        mu, logvar = model.encode_batch(b)
        loss, recon, kld = model.loss_dense(mu, logvar, types, preds, beta)
        parts = [recon, kld]
        if predictor:
            pred = predictor_mse(model, mu, b.y)[0]
            loss = loss + pred
            parts.append(pred)
        loss.backward()
        if clip > 0:
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
        part = torch.stack([t.detach().reshape(()) for t in [loss] + parts])
        sums = part if sums is None else sums + part
        optimizer.step()
    return tuple(float(v) for v in sums.tolist())   # the one read


def test_nll(model, store: DagStore, idx, batch_size: int) -> float:
    """The `Nll` of `test()` (dvae/train.py:276-301): in evaluation mode and without gradients, the reconstruction loss of
    every batch summed and divided by len(idx) - added up on the device and read once.  The mode the model came in is
    restored."""
    ids = store._ids(idx)
    was_training = model.training
    model.eval()
    total = None
    try:
        with torch.no_grad():
            for b in store.loader(ids, batch_size):
                types, preds = b.types, b.preds
                mu, logvar = model.encode_batch(b)
                nll = model.loss_dense(mu, logvar, types, preds)[1].reshape(())
                total = nll if total is None else total + nll
    finally:
        model.train(was_training)
    return float(total) / ids.size


def test_predictor(model, store: DagStore, idx, batch_size: int) -> float:
    """The `pred rmse` of `test()` (dvae/train.py:276-308) as that line is plainly meant: in evaluation mode and without
    gradients, sqrt(sum (y_pred - y)^2 / len(idx)) over the graphs `idx`, the batches' squared errors added up on the device
    and read once.  The reference prints it from a `pred_loss` that its loop never accumulates (train.py:282, 302-303): there
    the figure is always 0.  The mode the model came in is restored; a store without `y` raises ValueError."""
    from .predictor import _predictor_of, predictor_mse
    if "y" not in store.arrays:
        raise ValueError("test_predictor: the store holds no y (pass y= to DagStore)")
    _predictor_of(model, "test_predictor")
    ids = store._ids(idx)
    was_training = model.training
    model.eval()
    total = None
    try:
        with torch.no_grad():
            for b in store.loader(ids, batch_size):
                y = b.y
                mu, _ = model.encode_batch(b)
                se = predictor_mse(model, mu, y)[0].reshape(())
                total = se if total is None else total + se
    finally:
        model.train(was_training)
    return float(np.sqrt(float(total) / ids.size))


test_nll.__test__ = False   # (loops of the library, not tests for pytest to collect)
test_predictor.__test__ = False
