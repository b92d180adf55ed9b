"""Every node's forward state against float64, class by class of in-degree: inputs, reference and
bound of `tests/test_forward_states_cpu.py` and `tests/test_forward_states_f64_gpu.py`.  Nothing here needs a GPU.

Which code a row of the forward recurrence runs through depends on its in-degree (0, 1, 2, 3, 4 straight-line, chunks of four
under an online soft-max above that, one edge per lane up to 64, a strided loop beyond): `DEGS` holds both sides of every
such boundary, and a node's CLASS is the largest entry of `DEGS` that its in-degree reaches.

* `ladder_graph(seed)`  - sources, a middle tier (1-3 source predecessors each), then per class k > 0 `PER_CLASS` targets with
                          exactly k distinct predecessors out of both tiers (so a target sits at layer 2), each feeding a
                          one-node tail; two float edge features drawn per edge;
* `transposed(g)`       - the same graph with every edge turned round: the reverse direction meets the same classes;
* `SMALL` / `GENERAL`   - a ladder and its transpose (inside the limits of the one-workgroup builds) / five ladders and their
                          transposes, then the degenerate graphs of the parity tests (outside those limits);
* `edge_reversed(gs)`   - the twin: every graph's edge list back to front, so every node's in-edge list is reversed - the
                          same mathematics, the maximum score at the other end of the online soft-max;
* `dvae_graph_list`     - complete DAGs on 14 vertices (in-degrees 0..13) and random ones at density 0.5;
* `classes`             - (class, layer) of every node in a direction; `assert_classes` is the condition on the input: every
                          class k > 0 of a batch has two nodes at layer 2 or deeper, in each direction (`build_batch` asserts it);
* `reference`           - float64 state rows per (direction, stacked layer) and the fp32 oracle's own error against them;
* `check`               - the bound: per block `4 x max(e_base, 2^-23 max|ref|)`, asserted for the rows of every class.

Bound (the convention of DESIGN.md section 9c): `e_base` is the larger error, over ALL rows of the block, of the oracle's two fp32
restatements (`mode="csr"` / `"faithful"`; one run where the oracle has one loop nest only); one fp32 ulp of the block's
largest entry is the floor.  Nothing in it comes from the result under test."""
from __future__ import annotations

import bisect
import copy
import functools
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from dagnn_amd import GraphData, GraphBatch
from dagnn_amd.dag_utils import add_order_info, add_order_info_01
from oracle import dagnn_oracle as O

DEGS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 32, 33, 63, 64, 65, 128, 129)
PER_CLASS = 2
N_SRC, N_MID = 100, 40      # N_SRC + N_MID >= 129 distinct predecessors
FACTOR = 4.0
ULP = 2.0 ** -23
SMALL_LIMITS = (2048, 4096, 512)   # nodes, edges, graphs of the one-workgroup builds (csrc/small.hip)
F64 = torch.float64


def deg_class(k: int) -> int:
    """The largest entry of `DEGS` that is <= k."""
    return DEGS[bisect.bisect_right(DEGS, int(k)) - 1]


# ------------------------------------------------------------------ graphs
def _code2_graph(n: int, edges: np.ndarray, attr: np.ndarray, rng) -> GraphData:
    g = GraphData(x=torch.from_numpy(np.stack([rng.integers(0, 98, n), rng.integers(0, 300, n)], 1)).long(),
                  node_depth=torch.from_numpy(rng.integers(0, 30, n)).long().view(-1, 1),
                  edge_index=torch.from_numpy(np.ascontiguousarray(edges)).long().reshape(2, -1),
                  edge_attr=torch.from_numpy(np.ascontiguousarray(attr, dtype=np.float32)).reshape(-1, 2))
    add_order_info_01(g)
    return g


def ladder_graph(seed: int) -> GraphData:
    """Node ids: sources [0, N_SRC), middle tier, then (target, tail) pairs in ascending class order."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    mids = list(range(N_SRC, N_SRC + N_MID))
    for m in mids:
        for s in rng.choice(N_SRC, size=int(rng.integers(1, 4)), replace=False):
            src.append(int(s))
            dst.append(m)
    n = N_SRC + N_MID
    for k in DEGS[1:]:
        for _ in range(PER_CLASS):
            if k == 1:
                preds = [int(rng.choice(mids))]
            else:   # at least one of each tier, the rest from both
                n_mid = int(rng.integers(1, min(k - 1, N_MID) + 1))
                n_mid = max(n_mid, k - N_SRC)
                preds = [int(p) for p in rng.choice(mids, size=n_mid, replace=False)] + \
                        [int(p) for p in rng.choice(N_SRC, size=k - n_mid, replace=False)]
                preds = [preds[j] for j in rng.permutation(k)]
            assert len(set(preds)) == k
            src += preds + [n]
            dst += [n] * k + [n + 1]
            n += 2
    edges = np.stack([np.asarray(src), np.asarray(dst)])
    return _code2_graph(n, edges, rng.standard_normal((edges.shape[1], 2)), rng)


def _rebuilt(g: GraphData, edge_index, edge_attr=None) -> GraphData:
    """`g` with another edge list; layers recomputed."""
    out = g.clone()
    out.edge_index = edge_index.contiguous()
    if edge_attr is not None:
        out.edge_attr = edge_attr.contiguous()
    if getattr(g, "bi_layer_index", None) is not None:
        add_order_info(out)
    else:
        add_order_info_01(out)
    return out


def transposed(g: GraphData) -> GraphData:
    return _rebuilt(g, g.edge_index.flip(0), getattr(g, "edge_attr", None))


def edge_reversed(graphs: Sequence[GraphData]) -> List[GraphData]:
    """Every graph's edge list back to front: the in-edge (and out-edge) list of every node is reversed."""
    ea = lambda g: getattr(g, "edge_attr", None)  # noqa: E731
    return [_rebuilt(g, g.edge_index.flip(1), None if ea(g) is None else ea(g).flip(0)) for g in graphs]


def small_graphs(seed: int = 11) -> List[GraphData]:
    g = ladder_graph(seed)
    return [g, transposed(g)]


def _degenerate_graphs() -> List[GraphData]:
    """The graphs of `tests.helpers._degenerate_batch` (single nodes, a chain, 200-way fan-in / fan-out, no edges, a duplicate
    edge), taken back out of the batch it collates."""
    from tests.helpers import _degenerate_batch
    b = _degenerate_batch()
    out = []
    for i in range(b.num_graphs):
        n0, n1 = int(b.ptr[i]), int(b.ptr[i + 1])
        e = (b.batch[b.edge_index[0]] == i) if b.edge_index.shape[1] else torch.zeros(0, dtype=torch.bool)
        g = GraphData(x=b.x[n0:n1].clone(), node_depth=b.node_depth[n0:n1].clone(), edge_index=b.edge_index[:, e] - n0,
                      edge_attr=b.edge_attr[e].clone())
        add_order_info_01(g)
        out.append(g)
    return out


def general_graphs(seeds: Sequence[int] = (21, 22, 23, 24, 25)) -> List[GraphData]:
    out = []
    for s in seeds:
        g = ladder_graph(s)
        out += [g, transposed(g)]
    return out + _degenerate_graphs()


def dvae_graph_list(kind: str, B: int = 6, n: int = 14, nvt: int = 6, seed: int = 3) -> List[GraphData]:
    """B complete DAGs (vertex v has in-degree v at layer v) and B random ones (density 0.5; they hold the small in-degrees at
    deep layers) on n vertices, as graph objects of the D-VAE encoders (`kind`: 'na' | 'bn' - the same graphs for both)."""
    from tests import helpers as Hh
    out = []
    for j, family in enumerate(("complete", "random0.5")):
        types, preds = Hh.dvae_dense_graphs(family, B, n, nvt, 0, seed + j)
        out += Hh.dvae_graphs_from_dense(types, preds, nvt)
    return out


def collate(graphs: Sequence[GraphData]) -> GraphBatch:
    return GraphBatch.from_data_list([g.clone() for g in graphs])


# ------------------------------------------------------------------ classes
def _layers(batch, d: int) -> torch.Tensor:
    if getattr(batch, "bi_layer_index", None) is not None:
        return batch.bi_layer_index[d][0]
    return batch._bi_layer_idx0 if d == 0 else batch._bi_layer_idx1


def classes(batch, direction: int) -> Tuple[np.ndarray, np.ndarray]:
    """(class [N], layer [N]) of every node in `direction`: in-degree counts in-edges for 0, out-edges for 1 (duplicates count,
    as they do in the kernels' edge lists)."""
    N = int(batch.x.shape[0])
    deg = np.bincount(batch.edge_index[1 - direction].cpu().numpy(), minlength=N)
    cls = np.asarray([deg_class(k) for k in deg], np.int64)
    return cls, _layers(batch, direction).cpu().numpy().astype(np.int64)


def assert_classes(batch, dirs=(0, 1), want: Sequence[int] = ()) -> None:
    """The condition on the input: every class k > 0 that occurs (and every class of `want`) has `PER_CLASS` nodes at layer 2
    or deeper, in each direction - a row whose predecessors are layer-0 rows only reads no recurrent state."""
    for d in dirs:
        cls, lay = classes(batch, d)
        for k in sorted(set(cls.tolist()) | set(want)):
            if k > 0:
                deep = int(((cls == k) & (lay >= 2)).sum())
                assert deep >= PER_CLASS, "direction %d: class %d has %d node(s) at layer >= 2" % (d, k, deep)


def within_small_limits(batch) -> bool:
    return int(batch.x.shape[0]) <= SMALL_LIMITS[0] and int(batch.edge_index.shape[1]) <= SMALL_LIMITS[1] and \
        int(batch.num_graphs) <= SMALL_LIMITS[2]


@functools.lru_cache(maxsize=None)
def graphs_of(name: str, twin: bool = False) -> List[GraphData]:
    """The graphs of batch `name` ("SMALL" | "GENERAL" | "DVAE"), or of its edge-reversed twin."""
    gs = {"SMALL": small_graphs, "GENERAL": general_graphs, "DVAE": lambda: dvae_graph_list("bn")}[name]()
    return edge_reversed(gs) if twin else gs


@functools.lru_cache(maxsize=None)
def build_batch(name: str, twin: bool = False) -> GraphBatch:
    """Batch `name` (or its twin), built once: asserts the class condition - every class of `DEGS` (up to 13 for the D-VAE
    graphs) - and the side of the one-workgroup limits the batch is meant for.  Callers clone it before a pass."""
    b = collate(graphs_of(name, twin))
    assert_classes(b, want=[k for k in DEGS if k <= 13] if name == "DVAE" else DEGS)
    assert within_small_limits(b) == (name != "GENERAL"), name
    return b


# ------------------------------------------------------------------ reference
def _is_dvae(model) -> bool:
    return hasattr(model, "grue_forward")


def _cpu_state(model) -> Dict[str, torch.Tensor]:
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


def oracle_kw(model) -> dict:
    """The oracle's keyword arguments for `model` (a `DAGNN`, `DAGNN_NA` or `DAGNN_BN`), read-out over all nodes."""
    if _is_dvae(model):
        return dict(num_layers=model.num_layers, bidirectional=model.bidirectional, num_nodes=model.num_nodes,
                    vids=bool(model._use_vids), out_pool_all=True, out_pool="max", agg=model.agg)
    return dict(num_layers=model.num_layers, bidirectional=model.bidirectional, out_wx=False, out_pool_all=True,
                out_pool="max", max_seq_len=model.max_seq_len, agg=model.agg)


def blocks_of(rows: torch.Tensor, model) -> Dict[tuple, torch.Tensor]:
    """`G.h` of a pass over all nodes, cut into its blocks: `(direction, stacked layer)` -> [N, H] for the raw states (the
    concatenation of `dagnn.py:195`), or the one block `("unified",)` where a D-VAE encoder leaves the rows behind `hg_unify` /
    `out_linear` only (a per-node linear map of the same rows)."""
    rows = rows.detach().cpu()
    H, L, dirs = model.hidden_dim, model.num_layers, list(model.dirs)
    if _is_dvae(model) and (model.bidirectional or L > 1):
        return {("unified",): rows}
    assert rows.shape[1] == len(dirs) * L * H, (tuple(rows.shape), len(dirs), L, H)
    return {(d, l): rows[:, (q * L + l) * H:(q * L + l + 1) * H] for q, d in enumerate(dirs) for l in range(L)}


def oracle_rows(sd, batch, kw: dict, dtype, mode: str = "csr") -> torch.Tensor:
    """`G.h` of the oracle's pass over all nodes (the oracle mutates its batch: it gets a copy)."""
    G = copy.deepcopy(batch)
    if "num_nodes" in kw:
        O.dvae_forward(sd, G, dtype=dtype, mode=mode, **kw)
    else:
        O.code2_forward(sd, G, dtype=dtype, mode=mode, **kw)
    return G.h


def _two_modes(kw: dict) -> bool:
    """The additive attentions have two restatements in the oracle (`recurrence_csr`, `recurrence_faithful`); the other
    aggregators one loop nest, whatever `mode` says."""
    return kw["agg"] in O.ADDITIVE_ATTN


def reference(model, batch, **kw) -> dict:
    """{"rows": block -> float64 [N, H], "e_base": block -> the fp32 oracle's largest error over all rows of the block}.
    `kw` overrides `oracle_kw(model)`."""
    kw = dict(oracle_kw(model), **kw)
    sd = _cpu_state(model)
    r64 = blocks_of(oracle_rows(sd, batch, kw, F64), model)
    e_base = {b: 0.0 for b in r64}
    for mode in (("csr", "faithful") if _two_modes(kw) else ("csr",)):
        r32 = blocks_of(oracle_rows(sd, batch, kw, torch.float32, mode), model)
        for b in r64:
            e_base[b] = max(e_base[b], float((r32[b].double() - r64[b]).abs().max()))
    return dict(rows=r64, e_base=e_base)


# ------------------------------------------------------------------ the bound
class StateMismatch(AssertionError):
    """A class of rows beyond the bound: `.block`, `.cls`, `.node`, `.layer`, `.ratio` (error / e_base) of the finding and the
    `.report` of every block (what `check` would have returned)."""

    def __init__(self, msg, block, cls, node, layer, ratio, report):
        super().__init__(msg)
        self.block, self.cls, self.node, self.layer, self.ratio, self.report = block, cls, node, layer, ratio, report


def _block_dirs(block, cls_by_dir) -> List[int]:
    return [block[0]] if block[0] != "unified" else sorted(cls_by_dir)


def check(got: Dict[tuple, torch.Tensor], ref: dict, cls_by_dir: Dict[int, Tuple[np.ndarray, np.ndarray]]) -> list:
    """For every block and every in-degree class of its direction: `max |got - ref|` over the class's rows (the H real columns)
    <= 4 x max(e_base, 2^-23 max|ref|).  Every node is in exactly one class, so every row is compared.  Raises `StateMismatch`
    for the first block that misses, naming the class whose failing row lies in the EARLIEST layer (an error travels downstream
    only, so that row is where it began; the worst such row on a tie).  Returns the report rows
    (block, direction, class, rows, e_got, e_base, ulp, ratio = e_got / max(e_base, ulp))."""
    assert set(got) == set(ref["rows"]), (sorted(got, key=str), sorted(ref["rows"], key=str))
    report, failure = [], None
    for block in sorted(ref["rows"], key=str):
        r = ref["rows"][block]
        g = got[block].detach().cpu().double()
        assert g.shape == r.shape, (block, tuple(g.shape), tuple(r.shape))   # (H real columns: no padding reaches here)
        assert bool(torch.isfinite(g).all()), "block %s: non-finite rows" % (block,)
        scale = float(r.abs().max())
        e_base, ulp = ref["e_base"][block], ULP * scale
        bound = FACTOR * max(e_base, ulp)
        err = (g - r).abs().max(1).values.numpy()
        for d in _block_dirs(block, cls_by_dir):
            cls, lay = cls_by_dir[d]
            assert cls.shape[0] == err.shape[0]
            failing = []
            for k in sorted(set(cls.tolist())):
                rows = np.flatnonzero(cls == k)
                e = float(err[rows].max())
                report.append((block, d, k, len(rows), e, e_base, ulp, e / max(e_base, ulp)))
                if not e <= bound:
                    bad = rows[~(err[rows] <= bound)]
                    first = bad[lay[bad] == lay[bad].min()]
                    node = int(first[np.argmax(err[first])])
                    failing.append((int(lay[node]), -float(err[node]), k, node))
            if failing and failure is None:
                layer, e, k, node = min(failing)
                ratio = -e / max(e_base, 1e-300)
                failure = ("block %s, direction %d: class %d misses the bound at node %d (layer %d): |got - ref| %.3e > %.3e = "
                           "%.0f x max(e_base %.3e, ulp %.3e), %.1f x e_base; classes of this block beyond the bound: %s"
                           % (block, d, k, node, layer, -e, bound, FACTOR, e_base, ulp, ratio, sorted(f[2] for f in failing)),
                           block, k, node, layer, ratio)
    if failure is not None:
        raise StateMismatch(*failure, report)
    return report


def _report(cid: str, report: list) -> Tuple[float, int]:
    """Print the worst ratio e / max(e_base, ulp) of a case and the class (and block) it belongs to."""
    block, d, k, n, e, e_base, ulp, ratio = max(report, key=lambda t: t[-1])
    print("STATES %-40s worst %.2f x (bound %.0f): class %d of block %s, direction %d (%d rows): e %.3e, e_base %.3e, ulp %.3e"
          % (cid, ratio, FACTOR, k, block, d, n, e, e_base, ulp))
    return ratio, k
