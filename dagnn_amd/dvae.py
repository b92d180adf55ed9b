"""D-VAE encoder variants of the same hot path: `DAGNN_NA` (= `dvae/dagnn.py:18-184`, class `DAGNN`
there) for ENAS neural-architecture DAGs and `DAGNN_BN` (`dvae/dagnn_bn.py:19-177`) for
Bayesian-network DAGs.

Constructor arguments, parameter names and shapes follow the reference (including the decoder-side
parameters of `DVAE_PYG` / `DVAE_BN_PYG`, `dvae/models_pyg.py:18-85,539-560`: `loss()` trains
fc3 / grud / add_vertex / add_edge; the rest is kept so that `state_dict`s are interchangeable).  `forward(G)` / `encode(list)`
run the layer-by-layer message passing in HIP; `loss(mu, logvar, G_true)` runs the teacher-forced decoder of
`DVAE_PYG.loss()` (`dvae/models_pyg.py:398-456`) and its reverse pass in HIP (csrc/dvae_decode.hip); `decode(z)`
samples graphs from latent vectors as `DVAE_PYG.decode()` (`dvae/models_pyg.py:338-396`) does, the whole decode in one
HIP call (csrc/dvae_sample.hip).
"""
from __future__ import annotations

import collections
import copy
from collections import namedtuple
from typing import List, NamedTuple, Optional

import numpy as np

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import constants as K
from . import engine
from .core import HipModule, default_schedule, derive_cell, pack_lockstep, run_stack
from .data import GraphBatch
from .route import dataflow_only

ENCODE_FUSED = int(__import__("os").environ.get("DAGNN_AMD_ENCODE_FUSED", "1"))   # 1: evaluation passes of the encoders as ONE library call (csrc/encode.hip)
OWN_LINEAR_MAX = 1 << 22   # multiply-adds up to which the final Linear of an evaluation pass runs on dagnn_gemm_nt_bias (see forward)
from .model import _EdgeAttnParams, _SelfAttnParams


class _NoParams(object):
    wea = False   # no edge encoder (num_rels = 1 in the D-VAE models)


class _GatedParams(object):
    wea = False

    def __init__(self, gate, mapper):
        self.gate, self.mapper = gate, mapper   # gate: Sequential(Linear, Sigmoid); mapper: Linear(bias=False)


class _AggView(object):
    """What `dagnn_amd.variants` reads from a model, for a D-VAE encoder with agg in {add, max}: GRU cells, values = the
    cell's own states, no edge features, and - unlike the ogbg model - one AggConv PER direction (`reverse=True` for the
    second, dvae/dagnn.py:66-70), so the messages land on the frontier in both."""
    agg_x = False
    recurr = 1
    agg_attn = False
    agg_attn_x = False
    shared_agg_flow = False

    vid_nodes = 0

    def __init__(self, m):
        self._m = m
        self.agg, self.hidden_dim, self.num_layers, self.dirs = m.agg, m.hidden_dim, m.num_layers, m.dirs
        self.emb_dim = m.cells_0[0].weight_ih.shape[1]   # the node inputs are the one-hot vertex types (nvt wide)
        if m.agg == K.NA_GATED_SUM:
            # GatedSumConv over hs_j = [state ; one-hot vertex id] (dvae/dagnn.py:124-137,269-299): gate / mapper are Linear(hs +
            # num_nodes, hs); csrc/variants.hip takes the one-hot columns as a per-vertex-id bias of the per-node projections
            self.vid_nodes = m.num_nodes
            self.node_aggr_0 = [_GatedParams(m.gate_forward[l], m.mapper_forward[l][0]) for l in range(m.num_layers)]
            self.node_aggr_1 = [_GatedParams(m.gate_backward[l], m.mapper_backward[l][0]) for l in range(m.num_layers)]
            return
        self.node_aggr_0 = [_NoParams() for _ in range(m.num_layers)]
        self.node_aggr_1 = [_NoParams() for _ in range(m.num_layers)]

    def __getattr__(self, name):   # cells_0 / cells_1, training, _cache (the caches land in the module's `_derived`), ...
        return getattr(self.__dict__["_m"], name)

    def parameters(self):
        return self._m.parameters()


class _CellView:
    """The four GRUCell tensors `engine.iprop_step` reads, without the module around them."""
    __slots__ = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")

    def __init__(self, w_ih, w_hh, b_ih, b_hh):
        self.weight_ih, self.weight_hh, self.bias_ih, self.bias_hh = w_ih, w_hh, b_ih, b_hh


def _iprop_dense(values, pred_vid, w_key, vid_bias, H, X, cells):
    """The decoder-side step as dense device-side torch ops, the form its reverse pass differentiates (`dvae/dagnn.py:187-239`):
    padded slots score 0 (their key is a zero row, and the query term `w_q.q + b` is common to every slot of a soft-max
    row, so it cancels - the query half of `attn_lin` and its bias get exact zero gradients), the aggregate of the
    layer-0 states feeds every stacked layer.  `w_key` None: the type-keyed form (`attn_x` on the BN model,
    dvae/dagnn_bn.py:203-225) - `pred_vid` holds the predecessors' vertex TYPES, `vid_bias` the table key_type [nvt], and a
    real slot scores its table entry alone."""
    B = X.shape[0]
    if H is None:
        if values is None or values.shape[1] == 0:
            H = X.new_zeros(B, cells[0].weight_hh.shape[1])
        else:
            scores = values @ w_key if w_key is not None else values.new_zeros(values.shape[:2])
            if vid_bias is not None:
                real = pred_vid >= 0
                scores = scores + torch.where(real, vid_bias[pred_vid.clamp(min=0).long()], torch.zeros_like(scores))
            H = torch.einsum("bp,bpj->bj", torch.softmax(scores, dim=-1), values)
    Hv, out = X, []
    for c in cells:
        gi = F.linear(Hv, c.weight_ih, c.bias_ih)
        gh = F.linear(H, c.weight_hh, c.bias_hh)
        i_r, i_z, i_n = gi.chunk(3, 1)
        h_r, h_z, h_n = gh.chunk(3, 1)
        r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        Hv = n + z * (H - n)
        out.append(Hv)
    return torch.stack(out, 0)


class _IpropStep(torch.autograd.Function):
    """`_ipropagate_to` under autograd: forward = the ONE HIP launch (`dagnn_iprop_step`), backward = the reverse pass of
    the same step on the device (the step is a handful of [B, hs] products: recomputed densely from the saved inputs and
    differentiated there - no state of the forward launch is kept besides its inputs)."""

    @staticmethod
    def forward(ctx, values, pred_vid, w_key, vid_bias, H, X, L, *flat):
        cells = [_CellView(*flat[4 * l:4 * l + 4]) for l in range(L)]
        ctx.save_for_backward(*[t for t in (values, pred_vid, w_key, vid_bias, H, X) if t is not None], *flat)
        ctx.have = [t is not None for t in (values, pred_vid, w_key, vid_bias, H, X)]
        ctx.L = L
        if w_key is None and vid_bias is not None:   # type-keyed: `pred_vid` are types, `vid_bias` is key_type
            return engine.iprop_step(values, pred_vid, None, None, H, X, cells, key_type=vid_bias)
        return engine.iprop_step(values, pred_vid, w_key, vid_bias, H, X, cells)

    @staticmethod
    def backward(ctx, g_states):
        saved = list(ctx.saved_tensors)
        head = [saved.pop(0) if h else None for h in ctx.have]
        values, pred_vid, w_key, vid_bias, H, X = head
        flat = saved
        need = list(ctx.needs_input_grad)
        leaves, slots = [], []

        def leaf(t, slot):
            if t is None or not t.is_floating_point():
                return t
            t = t.detach().requires_grad_(need[slot])
            if need[slot]:
                leaves.append(t)
                slots.append(slot)
            return t

        values, w_key, vid_bias, H = leaf(values, 0), leaf(w_key, 2), leaf(vid_bias, 3), leaf(H, 4)
        flat = [leaf(t, 7 + k) for k, t in enumerate(flat)]
        grads = [None] * (7 + len(flat))
        if leaves:
            with torch.enable_grad():
                cells = [_CellView(*flat[4 * l:4 * l + 4]) for l in range(ctx.L)]
                out = _iprop_dense(values, pred_vid, w_key, vid_bias, H, X, cells)
            for slot, g in zip(slots, torch.autograd.grad(out, leaves, g_states.contiguous(), allow_unused=True)):
                grads[slot] = g
        return tuple(grads)


def decode_schedule(G_true, max_n: int, nvt: int, start_type: int = 0):
    """What the teacher-forced decoder reads of the true graphs: types [B, max_n] (`g.vs[v]['type']`, as
    `models_pyg.py:405-406` reads them) and predecessor bitmasks [B, max_n] (bit u of preds[b, v]: the edge u -> v,
    from `g.edge_index` as `:417-420`), both int32.  Every graph must have exactly max_n vertices, and no vertex but
    vertex 0 may have type `start_type`: the reference reads START_TYPE there as padding and does not add the vertex
    (`:413-414`), which shifts every later index - a different computation from the one the kernel runs."""
    B = len(G_true)
    if max_n > 32:
        raise ValueError("loss(): at most 32 vertices per graph (got max_n=%d)" % max_n)
    types = np.empty((B, max_n), dtype=np.int64)
    preds = np.zeros((B, max_n), dtype=np.uint32)
    for b, g in enumerate(G_true):
        if int(g.x.shape[0]) != max_n:
            raise ValueError("loss(): every graph must have exactly max_n=%d vertices (graph %d has %d)"
                             % (max_n, b, int(g.x.shape[0])))
        types[b] = [int(g.vs[v]["type"]) for v in range(max_n)]
        ei = g.edge_index
        ei = ei.cpu().numpy() if isinstance(ei, torch.Tensor) else np.asarray(ei)
        src, dst = ei[0].astype(np.int64), ei[1].astype(np.int64)
        keep = (src < dst) & (dst < max_n) & (src >= 0)
        np.bitwise_or.at(preds[b], dst[keep], (np.uint32(1) << src[keep].astype(np.uint32)))
    if B and (types[:, 1:].min() < 0 or types.max() >= nvt):
        raise ValueError("loss(): vertex types must lie in [0, nvt=%d)" % nvt)
    if B and (types[:, 1:] == start_type).any():
        b, v = (int(x[0]) for x in np.nonzero(types[:, 1:] == start_type))
        raise ValueError("loss(): vertex %d of graph %d has START_TYPE=%d, which only vertex 0 may have (the reference "
                         "treats it as padding and skips the vertex)" % (v + 1, b, start_type))
    return types.astype(np.int32), preds.view(np.int32)


def update_widths(preds: np.ndarray, max_n: int) -> List[int]:
    """The padding width P of every `_update_iv` call of the teacher-forced decoder, in the reference's call order
    (vertex 0 with H0 given: 0; then per vertex v: the fresh update, then one per earlier vertex vi = v-1 .. 0): the
    largest number of true predecessors >= vi over the batch - the same numbers the device derives from the masks."""
    m = preds.view(np.uint32)
    out = [0]
    for v in range(1, max_n):
        for k in range(v, -1, -1):
            sel = m[:, v] & np.uint32(((1 << v) - 1) & ~((1 << k) - 1))
            out.append(int(max(bin(int(x)).count("1") for x in sel)) if len(sel) else 0)
    return out


# ------------------------------------------------------------------ sampling decoder: draws and decoded graphs
def edge_draw_index(idx: int, vi: int) -> int:
    """Row of `u_edge` that serves the edge step (idx, vi): the reference's call order, idx ascending, vi = idx-1 .. 0."""
    if not 0 <= vi < idx:
        raise ValueError("edge_draw_index: need 0 <= vi < idx (got idx=%d, vi=%d)" % (idx, vi))
    return idx * (idx - 1) // 2 + (idx - 1 - vi)


def draw_shapes(max_n: int, B: int, attempts: int = 1):
    """Shapes of (u_type, u_edge) for `decode_dense(..., draws=...)`: [attempts, max_n, B] (row idx serves the type draw
    of vertex idx = 1 .. max_n-2, the other rows are unused) and [attempts, max_n(max_n-1)/2, B]."""
    return (attempts, max_n, B), (attempts, max_n * (max_n - 1) // 2, B)


IGRAPH_OUT, IGRAPH_IN, IGRAPH_ALL = 1, 2, 3   # igraph.OUT / IN / ALL


def _neighbor_mode(mode):
    if isinstance(mode, str):
        m = {"out": IGRAPH_OUT, "in": IGRAPH_IN, "all": IGRAPH_ALL}.get(mode.lower())
    else:
        m = int(mode) if int(mode) in (IGRAPH_OUT, IGRAPH_IN, IGRAPH_ALL) else None
    if m is None:
        raise ValueError("neighbour mode must be 'out', 'in', 'all' or igraph's OUT / IN / ALL (got %r)" % (mode,))
    return m


class _Vertex(dict):
    """`g.vs[v]`: a dict of the vertex's attributes ('type') with igraph's `index`, `indegree()` and `outdegree()`."""

    def __init__(self, graph, index, t):
        dict.__init__(self, type=t)
        self._graph, self.index = graph, index

    def indegree(self):
        return len(self._graph._pred[self.index])

    def outdegree(self):
        return len(self._graph._succ[self.index])


class _VertexSeq(object):
    def __init__(self, graph):
        self._graph = graph
        self._types = graph._types

    def __len__(self):
        return len(self._types)

    def __iter__(self):
        return (_Vertex(self._graph, v, t) for v, t in enumerate(self._types))

    def attributes(self):
        return ["type"]

    def __getitem__(self, key):
        if isinstance(key, str):
            if key != "type":
                raise KeyError(key)
            return list(self._types)
        v = range(len(self._types))[key]
        return _Vertex(self._graph, v, self._types[v])


class _Matrix(object):
    """What `get_adjacency()` returns: igraph's Matrix, read through `.data` (a list of rows)."""

    def __init__(self, data):
        self.data = data

    def __getitem__(self, key):
        return self.data[key]


class DecodedGraph(object):
    """A decoded DAG when python-igraph is not installed: the parts of `igraph.Graph` that D-VAE code reads of a decoded
    graph (`vcount`, `ecount`, `vs[v]['type']`, `vs['type']`, `vs.attributes()`, `predecessors`, `successors`, `get_edgelist`, `indegree`,
    `outdegree`, `is_dag`), and what dvae/util.py's checks and string forms call: iteration over `vs` (vertices with
    `.index`, `['type']`, `.indegree()`, `.outdegree()`), `are_connected`, `get_adjlist(mode)`, `get_adjacency().data`
    and `neighbors(v, mode)`.  Edges are listed in the order the reference's `decode()` adds them."""

    def __init__(self, types, edges):
        self._types = [int(t) for t in types]
        self._edges = [(int(u), int(v)) for u, v in edges]
        n = len(self._types)
        self._pred, self._succ = [[] for _ in range(n)], [[] for _ in range(n)]
        for u, v in self._edges:
            self._pred[v].append(u)
            self._succ[u].append(v)
        self.vs = _VertexSeq(self)

    def vcount(self):
        return len(self._types)

    def ecount(self):
        return len(self._edges)

    def get_edgelist(self):
        return list(self._edges)

    def predecessors(self, v):
        return sorted(self._pred[v])

    def successors(self, v):
        return sorted(self._succ[v])

    def indegree(self, vertices=None):
        deg = [len(p) for p in self._pred]
        return deg if vertices is None else (deg[vertices] if isinstance(vertices, int) else [deg[v] for v in vertices])

    def outdegree(self, vertices=None):
        deg = [len(s) for s in self._succ]
        return deg if vertices is None else (deg[vertices] if isinstance(vertices, int) else [deg[v] for v in vertices])

    def are_connected(self, u, v):
        return int(v) in self._succ[int(u)]

    def neighbors(self, vertex, mode="all"):
        m = _neighbor_mode(mode)
        v = int(vertex)
        return sorted((self._pred[v] if m != IGRAPH_OUT else []) + (self._succ[v] if m != IGRAPH_IN else []))

    def get_adjlist(self, mode="out"):
        return [self.neighbors(v, mode) for v in range(self.vcount())]

    def get_adjacency(self):
        n = self.vcount()
        data = [[0] * n for _ in range(n)]
        for u, v in self._edges:
            data[u][v] += 1
        return _Matrix(data)

    def is_dag(self):
        indeg = self.indegree()
        ready = [v for v in range(self.vcount()) if indeg[v] == 0]
        seen = 0
        while ready:
            u = ready.pop()
            seen += 1
            for w in self.successors(u):
                indeg[w] -= 1
                if indeg[w] == 0:
                    ready.append(w)
        return seen == self.vcount()


def decoded_edges(types, preds, nv, end_type):
    """The edge list of one decoded graph in the reference's insertion order: per vertex v ascending, its predecessors
    descending (one per edge step vi = v-1 .. 0), except the END vertex, whose loose ends are added at once in the
    iteration order of a python set of them.  types / preds: the graph's rows of decode_dense (preds as bitmasks), nv its vertex count."""
    out = []
    for v in range(1, int(nv)):
        m = int(preds[v]) & 0xFFFFFFFF
        us = [u for u in range(v) if m >> u & 1]
        # (the END vertex: the reference iterates a python set of the loose ends, built in ascending order)
        out += [(u, v) for u in (list(set(us)) if int(types[v]) == end_type else us[::-1])]
    return out


def graphs_from_dense(types, preds, nv, end_type, use_igraph=None):
    """Host graphs from the dense rows of decode_dense (numpy arrays [B, n], [B, n], [B]): `igraph.Graph` objects built
    as the reference builds them (a 'type' vertex attribute, nothing else) when igraph imports, else DecodedGraph."""
    ig = None
    if use_igraph is None or use_igraph:
        try:
            import igraph as ig
        except ImportError:
            if use_igraph:
                raise
            ig = None
    out = []
    for b in range(len(nv)):
        k = int(nv[b])
        ts = [int(t) for t in types[b][:k]]
        edges = decoded_edges(types[b], preds[b], k, end_type)
        if ig is None:
            out.append(DecodedGraph(ts, edges))
        else:
            g = ig.Graph(directed=True)
            for t in ts:
                g.add_vertex(type=t)
            for u, v in edges:
                g.add_edge(u, v)
            out.append(g)
    return out


DecodedDense = namedtuple("DecodedDense", ["types", "preds", "nv", "states"])


# ------------------------------------------------------------------ validity, strings and selection (dvae/util.py)
SelectedDense = namedtuple("SelectedDense", ["valid", "pick", "n_valid", "n_same", "keys"])
_KINDS = {"ENAS": 0, "BN": 1}            # DAGNN_DVAE_ENAS / DAGNN_DVAE_BN
_SELECTS = {"first": 0, "most_common": 1}  # DAGNN_DVAE_FIRST_VALID / DAGNN_DVAE_MOST_FREQUENT
SELECT_ROWS = 1 << 15   # rows (attempts x points) per decode_dense call of decode_from_latent_space by default


def _kind(data_type):
    if data_type not in _KINDS:
        raise ValueError("data_type must be 'ENAS' or 'BN' (got %r)" % (data_type,))
    return _KINDS[data_type]


def _select_mode(select):
    if select not in _SELECTS:
        raise ValueError("select must be 'first' (the reference's pick) or 'most_common' (got %r)" % (select,))
    return _SELECTS[select]


def _n_nodes(n_nodes):
    """0 for any vertex count ('variable' as the reference spells it, or None), else the required count."""
    if n_nodes is None or (isinstance(n_nodes, str) and n_nodes == "variable"):
        return 0
    if isinstance(n_nodes, str) or int(n_nodes) < 1 or int(n_nodes) > 32:
        raise ValueError("n_nodes must be 'variable' or a vertex count in 1..32 (got %r)" % (n_nodes,))
    return int(n_nodes)


def _row_edges(preds, k):
    return [(u, v) for v in range(k) for u in range(v) if int(preds[v]) >> u & 1]


def enas_string(types, preds, nv):
    """`decode_igraph_to_ENAS` (dvae/util.py:168-180) of one dense row: per middle vertex i, type-2 then the i-1 bits
    j -> i for j < i-1."""
    res = []
    for i in range(1, int(nv) - 1):
        m = int(preds[i]) & 0xFFFFFFFF
        res.append(int(types[i]) - 2)
        res += [m >> j & 1 for j in range(i - 1)]
    return " ".join(str(x) for x in res)


def bn_adj_string(types, preds, nv):
    """`decode_igraph_to_BN_adj` (dvae/util.py:388-394) of one dense row: the middle vertices' adjacency, rows and
    columns permuted by the argsort of their types."""
    k = int(nv)
    order = np.argsort([int(t) for t in types[:k]][1:-1]).tolist()
    adj = np.zeros((k, k), dtype=np.int64)
    for u, v in _row_edges(preds, k):
        adj[u, v] += 1
    adj = adj[1:-1, 1:-1][order][:, order]
    return " ".join(str(x) for x in adj.reshape(-1))


def row_valid(types, preds, nv, data_type, nvt, start_type, end_type, n_nodes=None):
    """The reference's rules on one dense row, restated over its edge list: `is_valid_ENAS` (dvae/util.py:599-631;
    with n_nodes, also exactly n_nodes vertices) or `is_valid_BN` (:634-649).  A vertex count outside [1, len(types)] or
    a type outside [0, nvt) is invalid (the decoder writes neither), as in dagnn_dvae_select."""
    k, kind, nn_ = int(nv), _kind(data_type), _n_nodes(n_nodes)
    if not 1 <= k <= len(types):
        return False
    ts = [int(t) for t in types[:k]]
    if any(t < 0 or t >= nvt for t in ts):
        return False
    edges = _row_edges(preds, k)
    indeg, outdeg = [0] * k, [0] * k
    for u, v in edges:
        outdeg[u] += 1
        indeg[v] += 1
    n_start = sum(t == start_type for t in ts)
    n_end = sum(t == end_type and t != start_type for t in ts)
    if kind == 1:
        return n_start == 1 and n_end == 1 and len(set(ts)) == nvt and k == nvt
    res = n_start == 1 and n_end == 1
    for v in range(k):
        if (indeg[v] == 0 and ts[v] != start_type) or (outdeg[v] == 0 and ts[v] != end_type):
            return False
    res = res and all((i, i + 1) in edges for i in range(k - 2)) and indeg[k - 1] == 1
    return res and (nn_ == 0 or k == nn_)


def select_key_words(data_type, n, nvt):
    """W: 64-bit words of a canonical key (dagnn_dvae_select_key_words)."""
    if _kind(data_type) == 0:
        bits = 6 + (n - 2) * max(1, int(nvt - 1).bit_length()) + (n - 2) * (n - 3) // 2
    else:
        bits = max(min(nvt, n) - 2, 0) ** 2
    return max(1, (bits + 63) // 64)


def select_key(types, preds, nv, data_type, n, nvt):
    """The canonical key dagnn_dvae_select writes for a valid row (W signed 64-bit words, bit fields appended low bit
    first): ENAS the vertex count (6 bits), the middle types, then the row bits j < i-1 of vertices i = 2 .. nv-2; BN the
    type-ordered adjacency of the middle vertices, row by row."""
    k, acc, pos = int(nv), 0, 0
    fields = []
    if _kind(data_type) == 0:
        tb = max(1, int(nvt - 1).bit_length())
        fields = [(k, 6)] + [(int(types[v]), tb) for v in range(1, k - 1)]
        fields += [(int(preds[v]) & ((1 << (v - 1)) - 1), v - 1) for v in range(2, k - 1)]
    else:
        mid = [int(t) for t in types[1:k - 1]]
        rank = {t: r for r, t in enumerate(sorted(mid))}
        by_rank = sorted(range(1, k - 1), key=lambda v: rank[int(types[v])])
        for u in by_rank:
            fields.append((sum(1 << rank[int(types[v])] for v in range(u + 1, k - 1) if int(preds[v]) >> u & 1), k - 2))
    for val, width in fields:
        acc |= val << pos
        pos += width
    W = select_key_words(data_type, n, nvt)
    return [int(np.int64(np.uint64((acc >> (64 * w)) & 0xFFFFFFFFFFFFFFFF))) for w in range(W)]


def select_host(types, preds, nv, data_type, nvt, start_type, end_type, n_nodes=None, select="first"):
    """Host mirror of dagnn_dvae_select on numpy rows types / preds [A,B,n], nv [A,B], written as the reference's loop
    (dvae/util.py:430-461): validity per attempt, the string of every valid one, then per point the first valid string
    (select='first') or Counter.most_common(1) ('most_common').  Returns (valid [A,B] bool, pick [B], n_valid [B],
    n_same [B], strings: per point the list of (attempt, string) of its valid attempts)."""
    types, preds, nv = np.asarray(types), np.asarray(preds), np.asarray(nv)
    A, B = nv.shape
    form = enas_string if _kind(data_type) == 0 else bn_adj_string
    mode = _select_mode(select)
    valid = np.zeros((A, B), dtype=bool)
    pick, n_valid, n_same = (np.zeros(B, dtype=np.int32) for _ in range(3))
    strings = []
    for b in range(B):
        cur = []
        for a in range(A):
            if row_valid(types[a, b], preds[a, b], nv[a, b], data_type, nvt, start_type, end_type, n_nodes):
                valid[a, b] = True
                cur.append((a, form(types[a, b], preds[a, b], nv[a, b])))
        strings.append(cur)
        n_valid[b] = len(cur)
        if not cur:
            pick[b] = -1
            continue
        counts = collections.Counter(s for _, s in cur)
        best = cur[0][1] if mode == 0 else counts.most_common(1)[0][0]
        pick[b] = next(a for a, s in cur if s == best)
        n_same[b] = counts[best]
    return valid, pick, n_valid, n_same, strings


def select_decoded(decoded, data_type, nvt, start_type, end_type, n_nodes=None, select="first"):
    """Validity of every attempt of a DecodedDense [A,B,...] and the pick per point: SelectedDense(valid [A,B], pick [B]
    (-1: no valid attempt), n_valid [B], n_same [B], keys [B,A,W]), int32 but the int64 keys.  On the GPU one call of
    dagnn_dvae_select, without synchronising; rows already on the host go through the host mirror."""
    kind, mode = _kind(data_type), _select_mode(select)
    nn_ = _n_nodes(n_nodes) if kind == 0 else 0
    if decoded.types.is_cuda:
        return SelectedDense(*engine.dvae_select(decoded.types, decoded.preds, decoded.nv, nvt, start_type, end_type, kind, nn_,
                                                 mode))
    types, preds, nv = (t.cpu().numpy() for t in (decoded.types, decoded.preds, decoded.nv))
    A, B, n = types.shape
    valid, pick, n_valid, n_same, _ = select_host(types, preds, nv, data_type, nvt, start_type, end_type, nn_ or None, select)
    keys = np.zeros((B, A, select_key_words(data_type, n, nvt)), dtype=np.int64)
    for a, b in zip(*np.nonzero(valid)):
        keys[b, a] = select_key(types[a, b], preds[a, b], nv[a, b], data_type, n, nvt)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32))  # noqa: E731
    return SelectedDense(t(valid), t(pick), t(n_valid), t(n_same), torch.from_numpy(keys))


class _Decoder(NamedTuple):
    """What the D-VAE decoder reads, stated once per call by `_DvaeDagnn._decoder` for its HIP consumers: the teacher-forced
    loss (`engine.DvaeDecode`), the sampling decode (`engine.dvae_sample`) and the single-vertex step
    (`engine.iprop_step`).  `engine._marshal_decoder` checks every shape against the dimensions here."""
    n: int                # max_n
    nvt: int
    hs: int
    L: int                # stacked grud cells
    start_type: int
    end_type: int
    bn: bool
    agg: int              # _lib.DVAE_AGG_*
    # the differentiable parameters, in the order `_DecodeLoss` takes them and returns their gradients: the aggregator's
    # (attn_h / attn_x: attn_lin.weight; gated_sum: gate_forward.0.0.{weight,bias}, mapper_forward.0.0.weight), 4 per
    # grud cell, add_vertex.{0,2}.{weight,bias}, add_edge.{0,2}.{weight,bias}
    params: list
    cells: list           # per layer (w_ih, w_hh, b_ih, b_hh)
    av: list              # add_vertex (w1, b1, w2, b2)
    ae: list              # add_edge (w1, b1, w2, b2)
    # what the library reads of the aggregator - views, no copies: attn_h w_key [hs] and (NA) vid_bias [n]; attn_x key_type
    # [nvt]; gated_sum gate = (gate_w, gate_b, mapper_w); the others None
    w_key: Optional[torch.Tensor]
    vid_bias: Optional[torch.Tensor]
    key_type: Optional[torch.Tensor]
    gate: Optional[list]
    # columns of the attn_lin.weight gradient where the key (attn_x: the type table) and the vertex-id gradients land
    key_off: int
    vid_off: Optional[int]


class _DecodeLoss(torch.autograd.Function):
    """`res` of `DVAE_PYG.loss()` (the negative log-likelihood of the true graphs under teacher forcing) as ONE call of
    `dagnn_dvae_decode_forward`; its gradients as ONE call of `dagnn_dvae_decode_backward`.  Inputs after the fixed
    ones: `dec.params`."""

    @staticmethod
    def forward(ctx, dec, types, preds, h0, *params):
        run = _make_decode(dec, types, preds, h0, params)
        ll = run.forward()
        ctx.run, ctx.dec = run, dec
        ctx.save_for_backward(h0, *params)   # (version checks: backward reads these through the saved pointers)
        return ll[2 * h0.shape[0]].clone()

    @staticmethod
    def backward(ctx, g_res):
        saved = ctx.saved_tensors   # raises if a parameter was modified in place since the forward call
        dec, run = ctx.dec, ctx.run
        if dec.agg == _lib.DVAE_AGG_GATED_SUM:
            d_h0, d_cells, d_av, d_ae, d_agg = run.backward(g_res, None, 0, None)
        else:
            d_attn = torch.zeros_like(saved[1])   # (the query half stays zero: it cancels in the soft-max)
            d_h0, d_cells, d_av, d_ae = run.backward(g_res, d_attn, dec.key_off, dec.vid_off)
            d_agg = [d_attn]
        ctx.run = None
        flat = [t for c in d_cells for t in c] + d_av + d_ae
        return (None, None, None, d_h0) + tuple(d_agg) + tuple(flat)


def _make_decode(dec, types, preds, h0, params=None):
    """The teacher-forced decode of the description `dec` on (types, preds, h0).  `params` are `dec.params`, as
    `_decode_loss_inputs` returns them beside it; the description already holds what is read of them."""
    return engine.DvaeDecode(dec, types, preds, h0.detach())


_LOSS_NEEDS_GPU = ("loss(): the model must live on a ROCm GPU - the teacher-forced decoder is HIP "
                   "(csrc/dvae_decode.hip) and has no CPU path")


class _DvaeBase(HipModule):
    """Parameters of `DVAE_PYG.__init__` (`dvae/models_pyg.py:18-85`), same names and order."""

    def __init__(self, max_n, nvt, START_TYPE, END_TYPE, hs=501, nz=56, bidirectional=False, vid=True,
                 num_layers=1):
        super().__init__()
        self.max_n, self.nvt, self.START_TYPE, self.END_TYPE = max_n, nvt, START_TYPE, END_TYPE
        self.hs, self.nz, self.gs = hs, nz, hs
        self.bidir, self.vid = bidirectional, vid
        self.vs = hs + max_n if vid else hs
        self.num_layers = num_layers
        gru = lambda: nn.ModuleList([nn.GRUCell(nvt if l == 0 else hs, hs) for l in range(num_layers)])  # noqa: E731
        self.grue_forward = gru()
        self.grue_backward = gru()
        self.fc1 = nn.Linear(self.gs, nz)
        self.fc2 = nn.Linear(self.gs, nz)
        self.grud = gru()
        self.fc3 = nn.Linear(nz, hs)
        self.add_vertex = nn.Sequential(nn.Linear(hs, hs * 2), nn.ReLU(), nn.Linear(hs * 2, nvt))
        self.add_edge = nn.Sequential(nn.Linear(hs * 2, hs * 4), nn.ReLU(), nn.Linear(hs * 4, 1))
        self.gate_forward = nn.ModuleList([nn.Sequential(nn.Linear(self.vs, hs), nn.Sigmoid())
                                           for _ in range(num_layers)])
        self.gate_backward = nn.ModuleList([nn.Sequential(nn.Linear(self.vs, hs), nn.Sigmoid())
                                            for _ in range(num_layers)])
        self.mapper_forward = nn.ModuleList([nn.Sequential(nn.Linear(self.vs, hs, bias=False))
                                             for _ in range(num_layers)])
        self.mapper_backward = nn.ModuleList([nn.Sequential(nn.Linear(self.vs, hs, bias=False))
                                              for _ in range(num_layers)])
        if self.bidir:
            self.hv_unify = nn.Sequential(nn.Linear(hs * 2, hs))
            self.hg_unify = nn.Sequential(nn.Linear(self.gs * 2 * num_layers, self.gs))
        self.relu, self.sigmoid, self.tanh = nn.ReLU(), nn.Sigmoid(), nn.Tanh()
        self.logsoftmax1 = nn.LogSoftmax(1)
        self.device = None

    def get_device(self):
        if self.device is None:
            self.device = next(self.parameters()).device
        return self.device

    def _collate_fn(self, G):
        return [copy.deepcopy(g) for g in G]

    def select_dense(self, decoded, data_type="ENAS", n_nodes=None, select="first"):
        """Validity and the pick per latent point of a `decode_dense(z, attempts=A)` result, as the reference's
        `decode_from_latent_space` (dvae/util.py:430-461) applies them: SelectedDense(valid [A,B], pick [B], n_valid [B],
        n_same [B], keys [B,A,W]) - see `select_decoded`.  ONE HIP call (csrc/dvae_select.hip), no synchronisation."""
        return select_decoded(decoded, data_type, self.nvt, self.START_TYPE, self.END_TYPE, n_nodes, select)


class _DvaeDagnn(_DvaeBase):
    _use_vids = True

    def _setup(self, emb_dim, hidden_dim, out_dim, num_layers, bidirectional, agg, out_wx, out_pool_all, out_pool,
               dropout, num_nodes):
        self.num_nodes = num_nodes
        self.agg = agg
        self.agg_attn = "attn" in agg
        self.agg_attn_x = "_x" in agg
        self.bidirectional = bidirectional
        self.dirs = [0, 1] if bidirectional else [0]
        self.out_wx = out_wx
        self.output_all = out_pool_all
        self.out_pool = out_pool
        self.emb_dim = emb_dim
        self.hidden_dim = hidden_dim
        self.out_hidden_dim = emb_dim + hidden_dim * num_layers if out_wx else hidden_dim * num_layers
        self._agg_plain = agg in (K.NA_GATED_SUM, K.NA_SUM, K.NA_MAX)
        if self.agg_attn and self.agg_attn_x and self._use_vids:
            raise NotImplementedError("DAGNN_NA with agg=%r: the reference forbids input-keyed attention on this model "
                                      "(`assert not (\"_x\" in agg and \"attn\" in agg)`, dvae/dagnn.py:28); DAGNN_BN takes it" % (agg,))
        if not self._agg_plain and agg not in (K.NA_ATTN_H, K.NA_SELF_ATTN_H, K.NA_ATTN_X, K.NA_SELF_ATTN_X):
            raise NotImplementedError("D-VAE encoders: agg=%r (attn_h - the reference's default, dvae/train.py:86 -, self_attn_h, "
                                      "gated_sum, add, max; DAGNN_BN also attn_x, self_attn_x)" % (agg,))
        if agg == K.NA_GATED_SUM and not self._use_vids:
            raise NotImplementedError("DAGNN_BN with agg='gated_sum': the reference itself cannot run it - DVAE_BN_PYG re-creates the "
                                      "first layer's mapper / gate with nvt inputs (dvae/models_pyg.py:539-560) and GatedSumConv feeds "
                                      "them hs-wide states (dvae/dagnn_bn.py:289): a shape error in its first message")
        extra = num_nodes if self._use_vids else 0
        pred_dim = hidden_dim + extra
        # (`_x`, BN only: keys and queries are the node inputs G.x, dvae/dagnn_bn.py:48,129-131 - AttnConv's Linear(2 emb_dim, 1)
        # for every stacked layer, SelfAttnConv's Linear(emb_dim, 1))
        attn_dim = emb_dim if self.agg_attn_x else hidden_dim + extra
        if self._agg_plain:
            # GatedSumConv / AggConv own no parameters of their own here: gated_sum uses the base class's mapper / gate
            # (dvae/dagnn.py:60-65), add / max have none (num_rels = 1: no edge encoder)
            def conv(mapper, gate):   # (same `state_dict` names as the reference's GatedSumConv: it registers the shared modules)
                m = nn.Module()
                if agg == K.NA_GATED_SUM:
                    m.mapper, m.gate = mapper, gate
                return m
            self.node_aggr_0 = nn.ModuleList([conv(self.mapper_forward[l], self.gate_forward[l]) for l in range(num_layers)])
            self.node_aggr_1 = nn.ModuleList([conv(self.mapper_backward[l], self.gate_backward[l]) for l in range(num_layers)])
        elif agg in (K.NA_SELF_ATTN_H, K.NA_SELF_ATTN_X):   # keys scored alone: `attn_lin` has no query half (dvae/dagnn.py:49-54, 301-312)
            self.node_aggr_0 = nn.ModuleList([_SelfAttnParams(attn_dim, num_relations=1) for _ in range(num_layers)])
            self.node_aggr_1 = nn.ModuleList([_SelfAttnParams(attn_dim, num_relations=1, reverse=True)
                                              for _ in range(num_layers)])
        else:
            self.node_aggr_0 = nn.ModuleList([
                _EdgeAttnParams(emb_dim if l == 0 else attn_dim, pred_dim, num_relations=1, attn_dim=attn_dim)
                for l in range(num_layers)])
            self.node_aggr_1 = nn.ModuleList([
                _EdgeAttnParams(emb_dim if l == 0 else attn_dim, pred_dim, num_relations=1, attn_dim=attn_dim,
                                reverse=True) for l in range(num_layers)])
        # the cells ARE the base class's encoder GRUs (aliased names, dvae/dagnn.py:73-75)
        self.cells_0 = self.grue_forward
        if bidirectional:
            self.cells_1 = self.grue_backward
        self.dropout = nn.Dropout(dropout)
        self.out_linear = nn.Linear(self.out_hidden_dim, out_dim) if num_layers > 1 else None
        self.schedule = default_schedule()  # 'lockstep' (frontier launches) or 'pergraph' (persistent workgroups)

    def _cells(self, fresh: bool = False):
        # (the registries are read directly: `getattr(self, "cells_0")[i].weight_ih` is three trips through
        # nn.Module.__getattr__ - 15 us for the ten tensors of cfg 1, whose forward is host-bound; same objects, always current)
        srcs: List[torch.Tensor] = []
        mods = self._modules
        for d in self.dirs:
            cells, aggrs = mods["cells_%d" % d]._modules, mods["node_aggr_%d" % d]._modules
            for i in range(self.num_layers):
                c, a = cells[str(i)], aggrs[str(i)]._modules["attn_lin"]
                cp = c._parameters
                for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    t = cp.get(name)
                    srcs.append(t if t is not None else getattr(c, name))   # (a re-parametrised weight is a plain attribute)
                t = a._parameters.get("weight")
                srcs.append(t if t is not None else a.weight)
        extra = self.num_nodes if self._use_vids else 0

        def make():
            out = {}
            for d in self.dirs:
                for i in range(self.num_layers):
                    c = getattr(self, "cells_%d" % d)[i]
                    a = getattr(self, "node_aggr_%d" % d)[i]
                    dq = self._key_offset(i)
                    out[(d, i)] = derive_cell(c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh, a.attn_lin.weight,
                                              self.hidden_dim, dq, i > 0, None, extra, schedule=self.schedule,
                                              key_dim=self.emb_dim if self.agg_attn_x else None, pack=False,
                                              stacked=self.num_layers)
            if self.schedule == "lockstep":
                pack_lockstep(out.values())
            return out

        return self._cache(self.schedule).get(srcs, make, fresh=fresh or self.training)

    # ---- hooks of autograd.Recurrence
    @property
    def _vid_nodes(self) -> int:
        return self.num_nodes if self._use_vids else 0

    def _key_offset(self, i: int) -> int:
        """Where the key half of `attn_lin.weight` starts: behind the query half - which `self_attn_{h,x}` do not have.  The
        `_x` aggregators (BN) query with the inputs in every stacked layer: emb_dim for every i."""
        if self.agg in (K.NA_SELF_ATTN_H, K.NA_SELF_ATTN_X):
            return 0
        return self.emb_dim if i == 0 or self.agg_attn_x else self.hidden_dim + self._vid_nodes

    def _static_scores(self, x, cells):
        """`*_x` aggregators: the keys are the node inputs, one score per node and cell (dvae/dagnn_bn.py:129-131) - the
        query part and the bias are common to all in-edges of a node and cancel in the segment soft-max."""
        if not self.agg_attn_x:
            return None
        return {k: torch.mv(x.detach(), c.key_raw) for k, c in cells.items()}

    def _readout(self, plan, B, x, h):
        """End vertex of every graph for d = 0, start vertex for d = 1 (dvae/dagnn.py:147-161, dagnn_bn.py:138-152)."""
        L, H, nn_ = self.num_layers, self.hidden_dim, self.num_nodes
        hcat = torch.empty(B, len(self.dirs) * L * H, dtype=torch.float32, device=x.device)
        jobs = [(h[0][i], nn_ - 1, i * H) for i in range(L)]
        if self.bidirectional:
            jobs += [(h[1][i], 0, (L + i) * H) for i in range(L)]
        if len(jobs) <= 16:
            engine.gather_rows_batch(jobs, B, nn_, hcat)   # one launch for every (direction, stacked layer)
        else:
            for t, off, col in jobs:
                engine.gather_rows(t, B, nn_, off, hcat, col)
        return hcat

    def _readout_backward(self, plan, x, h, gout, g_ext, dx):
        L, H, nn_ = self.num_layers, self.hidden_dim, self.num_nodes
        for i in range(L):
            g_ext[0][i][nn_ - 1::nn_, :H] = gout[:, i * H:(i + 1) * H]
            if self.bidirectional:
                g_ext[1][i][0::nn_, :H] = gout[:, (L + i) * H:(L + i + 1) * H]

    def _training_pass(self) -> bool:
        if not (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            return False
        if self.schedule != "lockstep":
            raise NotImplementedError("the HIP backward pass needs the lock-step schedule")
        return True

    def forward(self, G):
        """`dvae/dagnn.py:99-175` / `dvae/dagnn_bn.py:98-168`."""
        out = self._forward(G)
        self._guard_params(next(self.parameters()))
        return out

    def attention(self, G, logits: bool = False):
        """The attention weights of an evaluation pass, as `DAGNN.attention`: an `evaluate.Attention` with `out` = what
        `forward(G)` returns (from the same pass, on the step-by-step route: the fused call returns no states), `alpha`
        [len(dirs), num_layers, E], `logit` with `logits=True` - NA: the one-hot vertex-id columns of keys and queries
        included - and `h`, the states the weights weigh (`G.h` keeps the read-out rows only).  `gated_sum`, `add`, `max`
        raise ValueError."""
        from .attention import run
        return run(self, G, logits)

    def _forward(self, G):
        if self.output_all and self.out_pool not in (K.P_MAX, K.P_MEAN, K.P_ADD):
            raise NotImplementedError("out_pool=%r over all nodes: the reference's own self-attention pooling of the "
                                      "D-VAE models references an undefined layer (dvae/dagnn.py:85-88)" % self.out_pool)
        train = self._training_pass()
        device = self.get_device()
        G = G.to(device)
        x = G.x.float().contiguous()
        N = x.shape[0]
        L, H, nn_ = self.num_layers, self.hidden_dim, self.num_nodes
        if N % nn_ != 0:
            raise ValueError("every graph must have exactly num_nodes=%d nodes (dvae/dagnn.py:150-158)" % nn_)
        B = N // nn_
        bl = G.bi_layer_index
        cap = self.__dict__.get("_attn_capture")   # (`attention`: wants the states, which the fused call does not return)
        if not train and not self._agg_plain and not self.agg_attn_x and not self.output_all and ENCODE_FUSED \
                and self.schedule == "lockstep" and engine.TIMER is None and cap is None:
            out = self._encode_fused(G, x, B)
            if out is not None:
                return out
        plan = engine.build_plan(G.edge_index, bl[0][0], bl[1][0], G.batch, B, None)
        if self._agg_plain:
            return self._forward_plain_agg(G, plan, x, B, train)
        if self.output_all:
            if train:
                from .autograd import Recurrence
                flat = Recurrence.apply(self, plan, B, False, x, *self._train_params())
            else:
                cells = self._cells()
                hh = run_stack(plan, x, cells, self.dirs, L, H, vid_nodes=self._vid_nodes, schedule=self.schedule,
                               arena=self._arena_for(x), static_score=self._static_scores(x, cells))
                if cap is not None:
                    cap.update(plan=plan, x=x, h=hh, E=G.edge_index.shape[1])
                flat = [hh[d][i] for d in self.dirs for i in range(L)]
            return self._pool_all(G, plan, x, flat, B)
        if train:
            from .autograd import Recurrence
            hcat = Recurrence.apply(self, plan, B, True, x, *self._train_params())[0]
        else:
            cells = self._cells()
            h = run_stack(plan, x, cells, self.dirs, L, H, vid_nodes=self._vid_nodes, schedule=self.schedule,
                          arena=self._arena_for(x), static_score=self._static_scores(x, cells))
            if cap is not None:
                cap.update(plan=plan, x=x, h=h, E=G.edge_index.shape[1])
            hcat = self._readout(plan, B, x, h)
        G.h = hcat
        G.batch = G.batch[0::nn_] if self.bidirectional else G.batch[nn_ - 1::nn_]
        lin = self.hg_unify if self.bidirectional else (self.out_linear if L > 1 else None)
        if lin is None:
            return G.h
        if isinstance(lin, nn.Sequential) and len(lin) == 1:   # (`hg_unify` is a Sequential of one Linear: dvae/dagnn.py:66-68)
            lin = lin[0]
        if train or not isinstance(lin, nn.Linear) or G.h.shape[0] * lin.weight.numel() > OWN_LINEAR_MAX:
            return lin(G.h)
        # evaluation, small product (cfg 1: 64 x 256 x 128): on the path's own GEMM - nn.Linear costs the host ~27 us of
        # library dispatch and cfg 1 is host-bound (scripts/small_host_profile.py: 155 -> 134 us per forward); cfg 4's
        # 128 x 1024 x 256 stays with the library (its split-K kernel is the faster one there: 196 vs 285 us)
        return engine.gemm_nt_bias([G.h], [lin.weight.detach()], [None if lin.bias is None else lin.bias.detach()])[0]

    def _pool_all(self, G, plan, x, flat, B):
        """Pool over ALL nodes (dvae/dagnn.py:163-172) of the flat states: per-node projection, then HIP pooling over the
        nodes of every graph (`plan` given: `dagnn_readout_pool_batch`, or `autograd.PoolNodes` where a gradient is wanted - every
        graph has `num_nodes` nodes, so the kernel's mean factor is the reference's) or torch pooling."""
        G.h = torch.cat(([x] if self.out_wx else []) + list(flat), dim=-1)
        if self.bidirectional:
            G.h = self.hg_unify(G.h)
        elif self.num_layers > 1:
            G.h = self.out_linear(G.h)
        if plan is not None and not (torch.is_grad_enabled() and G.h.requires_grad):
            out = torch.empty(B, G.h.shape[1], dtype=torch.float32, device=G.h.device)
            engine.readout_pool_batch(plan, [(G.h, 2, self.out_pool, 0)], out)
            return out
        if plan is not None and G.h.is_cuda and G.h.dtype == torch.float32:
            from .autograd import PoolNodes
            return PoolNodes.apply(plan, G.h, 2, self.out_pool)
        idx = G.batch.view(-1, 1).expand_as(G.h)
        out = G.h.new_zeros(B, G.h.shape[1])
        if self.out_pool == K.P_MAX:
            return out.scatter_reduce(0, idx, G.h, "amax", include_self=False)
        out = out.scatter_add(0, idx, G.h)
        return out / self.num_nodes if self.out_pool == K.P_MEAN else out

    # ------------------------------------------------------------------ agg in {gated_sum, add, max} (dvae/dagnn.py:60-70)
    def _agg_view(self):
        v = self.__dict__.get("_agg_view_obj")
        if v is None:
            v = self.__dict__["_agg_view_obj"] = _AggView(self)
        return v

    def _gated_hip_ok(self) -> bool:
        """`gated_sum` through csrc/variants.hip: the states must be as wide as the gate / mapper inputs say (hs + num_nodes)."""
        w = self.gate_forward[0][0].weight
        return w.shape[1] == self.hidden_dim + self.num_nodes and w.shape[0] == self.hidden_dim

    def _gated_sum_states(self, G, x):
        """`gated_sum` on the NA encoder: the messages are gate(hs_j) * mapper(hs_j) with hs_j = [state ; one-hot vertex id]
        (dvae/dagnn.py:124-137, 269-299), i.e. per NODE P_j = W_g[:, :H] h_j + W_g[:, H + j mod n] + b_g (likewise the
        mapper) - the vertex-id columns are a per-node bias.  Layer by layer on differentiable torch ops, on whatever device
        and precision `x` has: the fall-back of `_forward_plain_agg` where the HIP paths do not apply, and the restatement
        the tests tie their float64 oracle to."""
        N, H, L, nn_ = x.shape[0], self.hidden_dim, self.num_layers, self.num_nodes
        dev = x.device
        vid = torch.arange(N, device=dev) % nn_
        ei = G.edge_index
        h = [[None] * L for _ in range(2)]
        for d in self.dirs:
            layer_of = G.bi_layer_index[d][0]
            T = int(layer_of.max()) + 1 if N else 0
            feed, other = ei[1 - d], ei[d]          # an edge feeds node `feed` from node `other`
            order = torch.argsort(layer_of[feed] * N + feed, stable=True)
            counts = torch.bincount(layer_of[feed], minlength=T).cumsum(0).cpu().tolist()
            gates = self.gate_forward if d == 0 else self.gate_backward
            maps = self.mapper_forward if d == 0 else self.mapper_backward
            cells = getattr(self, "cells_%d" % d)
            hs = [x.new_zeros(N, H) for _ in range(L)]
            ids = torch.arange(N, device=dev)
            for t in range(T):
                rows = ids[layer_of == t]
                inp = x[rows]
                if t > 0:
                    eids = order[(counts[t - 1]):(counts[t])]
                    src, dst = other[eids], feed[eids]
                for i in range(L):
                    ps = None
                    if t > 0:
                        wg, bg, wm = gates[i][0].weight, gates[i][0].bias, maps[i][0].weight
                        hj = hs[i][src]
                        g = torch.sigmoid(hj @ wg[:, :H].t() + wg[:, H + vid[src]].t() + bg)
                        m = hj @ wm[:, :H].t() + wm[:, H + vid[src]].t()
                        ps = x.new_zeros(N, H).index_add_(0, dst, g * m)[rows]
                    inp = cells[i](inp, ps)
                    hs[i] = hs[i].index_add(0, rows, inp)   # `G.h[d][i][layer] += inp` (dvae/dagnn.py:145)
            h[d] = hs
        return h

    def _forward_plain_agg(self, G, plan, x, B, train):
        """`forward` for agg in {gated_sum, add, max}: the generic HIP kernels of csrc/variants.hip (`dagnn_variant_run`;
        `gated_sum` (NA): the one-hot vertex-id columns of gate / mapper as a per-vertex-id bias), in training with the
        reverse sweep of csrc/variants_bwd.hip behind them (`variants.VariantRecurrence`, any hidden width); then the
        read-outs of `dvae/dagnn.py:147-172`.  Torch ops only where the sweep does not apply (`variants.hip_backward_
        supported`, or a gate that is not hs + num_nodes wide): one `warn_torch_path` warning per model shape."""
        from . import variants
        L, H, nn_ = self.num_layers, self.hidden_dim, self.num_nodes
        view = self._agg_view()
        gated = self.agg == K.NA_GATED_SUM
        if gated and not self._gated_hip_ok():
            if train:
                variants.warn_torch_path(view, G)
                h = self._gated_sum_states(G, x)
            else:
                with torch.no_grad():
                    h = self._gated_sum_states(G, x)
        elif not train:
            h = variants.run_hip(view, G, x, plan)
        elif variants.hip_backward_supported(view, G):
            # (gated_sum: the view hands out gate / mapper at their full width [hs, hs + num_nodes] - the parameters themselves,
            # so these gradients and the decoder's add up in one .grad)
            flat_params = [p for d in self.dirs for i in range(L) for _, p in variants._cell_params(view, d, i)]
            h = self._unflatten(variants.VariantRecurrence.apply(view, G, plan, x, *flat_params))
        else:
            variants.warn_torch_path(view, G)
            h = self._gated_sum_states(G, x) if gated else variants.run(view, G, x)
        N = x.shape[0]
        if self.output_all:
            return self._pool_all(G, plan, x, [h[d][i] for d in self.dirs for i in range(L)], B)
        first = torch.arange(0, N, nn_, device=x.device)
        last = first + (nn_ - 1)
        parts = [h[0][i][last] for i in range(L)]
        if self.bidirectional:
            parts += [h[1][i][first] for i in range(L)]
        G.h = torch.cat(parts, dim=-1)
        G.batch = G.batch[first] if self.bidirectional else G.batch[last]
        if self.bidirectional:
            return self.hg_unify(G.h)
        return self.out_linear(G.h) if L > 1 else G.h

    def _encode_fused(self, G, x, B):
        """The evaluation pass up to (and including, when it is small) the final Linear as ONE call into the library
        (`dagnn_encode_forward`, csrc/encode.hip): the same launches as the step-by-step path below, without the Python
        between them - these batches (64 x 8 / 128 x 10 nodes) are host-bound.  None: the shape is not one the dataflow
        kernel serves (the caller takes the general path).  Not for the `_x` aggregators: `dagnn_encode_forward` has no
        static-score input, so `_forward` never calls this for them (they take the step-by-step path)."""
        import ctypes as C
        from . import _lib
        from .core import pack_dataflow
        L, H, nn_, dirs = self.num_layers, self.hidden_dim, self.num_nodes, self.dirs
        cells = self._cells()
        Hp = cells[(dirs[0], 0)].Hp
        N, dev = x.shape[0], x.device
        groups = dataflow_only(dev, len(dirs), L, Hp, B, N)
        if groups <= 0:
            return None
        lib = _lib.load()
        arena = self._arena_for(x)
        arena.poll()   # a failure an earlier pass reported (no synchronisation)
        pack_dataflow(cells.values())
        ei = engine._dev(G.edge_index, "edge_index", torch.int64)
        bl = G.bi_layer_index
        lf, lb = engine._dev(bl[0][0], "layer ids", torch.int64), engine._dev(bl[1][0], "layer ids", torch.int64)
        batch = engine._dev(G.batch, "batch", torch.int64)
        plan = engine.PlanHandle(N, ei.shape[1], B, 0, dev)
        a = _lib.EncodeArgs()
        a.plan = plan.desc
        a.edge_index, a.layer_fwd, a.layer_bwd, a.batch = ei.data_ptr(), lf.data_ptr(), lb.data_ptr(), batch.data_ptr()
        a.plan_status = plan.status.data_ptr()
        f32 = dict(dtype=torch.float32, device=dev)
        gi = [None, None]
        for q, d in enumerate(dirs):
            c = cells[(d, 0)]
            gi[d] = torch.empty(N, 3 * Hp, **f32)
            a.gemm[q] = _lib.GemmGroup(x.data_ptr(), c.w_ih.data_ptr(), c.b_ih.data_ptr(), gi[d].data_ptr())
        a.num_gemm, a.gemm_cols, a.in_dim, a.ld_x = len(dirs), 3 * Hp, x.shape[1], x.stride(0)
        sbytes = lib.dagnn_dataflow_bytes(N, B, groups)
        sched = torch.empty((sbytes + 3) // 4, dtype=torch.int32, device=dev)
        plan.__dict__["_df"] = {(int(groups), engine.DF_COST_LAYER, engine.DF_COST_ROW): sched}   # (built inside the call)
        a.schedule, a.schedule_bytes = sched.data_ptr(), sbytes
        a.cost_layer, a.cost_row = engine.DF_COST_LAYER, engine.DF_COST_ROW
        ld = engine.frontier_ld(Hp)
        h = [[torch.empty(N, ld, **f32) if d in dirs else None for _ in range(L)] for d in range(2)]
        engine.dataflow_args(plan, dirs, L, Hp, cells, gi, h, groups, vid_mod=self._vid_nodes, arena=arena, args=a.df)
        hcat = torch.empty(B, len(dirs) * L * H, **f32)
        jobs = [(h[0][i], nn_ - 1, i * H) for i in range(L)]
        if self.bidirectional:
            jobs += [(h[1][i], 0, (L + i) * H) for i in range(L)]
        if len(jobs) > 16:
            return None
        for k, (t, off, col) in enumerate(jobs):
            a.jobs[k] = _lib.GatherJob(t.data_ptr(), t.stride(0), H, int(off), int(col))
        a.num_jobs, a.stride, a.hcat, a.ld_hcat = len(jobs), nn_, hcat.data_ptr(), hcat.shape[1]
        lin = self.hg_unify if self.bidirectional else (self.out_linear if L > 1 else None)
        if isinstance(lin, nn.Sequential) and len(lin) == 1:
            lin = lin[0]
        out = None
        fused_lin = isinstance(lin, nn.Linear) and hcat.shape[0] * lin.weight.numel() <= OWN_LINEAR_MAX and \
            lin.weight.shape[1] == hcat.shape[1] and hcat.shape[1] % 4 == 0
        if fused_lin:
            w = lin.weight.detach()
            out = torch.empty(B, w.shape[0], **f32)
            a.w_out, a.b_out = w.data_ptr(), (None if lin.bias is None else lin.bias.detach().data_ptr())
            a.out, a.out_dim = out.data_ptr(), w.shape[0]
        with engine.persistent_launch(x):
            engine.check(lib.dagnn_encode_forward(C.byref(a), engine._stream(x)), "dagnn_encode_forward")
        arena.watch(None, folded=True)
        G.h = hcat
        G.batch = G.batch[0::nn_] if self.bidirectional else G.batch[nn_ - 1::nn_]
        if lin is None:
            return hcat
        return out if fused_lin else lin(hcat)

    def encode(self, G):
        """(mu, logvar) of a list of graphs (`dvae/dagnn.py:177-184`)."""
        if type(G) != list:
            G = [G]
        b = GraphBatch.from_data_list(G)
        Hg = self(b)
        return self.fc1(Hg), self.fc2(Hg)

    def encode_batch(self, b):
        """(mu, logvar) of an already collated batch - `DagStore.batch(idx)`, or `GraphBatch.from_data_list` of D-VAE graphs:
        what `encode` does after its collation.  The pass may rewrite attributes of `b` (`batch`, `h`)."""
        Hg = self(b)
        return self.fc1(Hg), self.fc2(Hg)


    # ------------------------------------------------------------------ teacher-forced decoder loss (dvae/models_pyg.py:324-456)
    def reparameterize(self, mu, logvar, eps_scale=0.01):
        """z ~ N(mu, std) in training mode, mu in evaluation mode (`models_pyg.py:324-331`)."""
        if self.training:
            std = logvar.mul(0.5).exp_()
            eps = torch.randn_like(std) * eps_scale
            return eps.mul(std).add_(mu)
        return mu

    def loss(self, mu, logvar, G_true, beta=0.005):
        """`(res + beta * kld, res, kld)` of `DVAE_PYG.loss()` (`models_pyg.py:398-456`): the negative log-likelihood of
        the true graphs under the teacher-forced decoder plus the KL term.  The decoder and its reverse pass are HIP
        (csrc/dvae_decode.hip: one library call each); the schedule (types, predecessor masks) is built once on the host
        and copied once.  Gradients reach mu / logvar, fc3, grud, attn_lin (key / vertex-id part), add_vertex and
        add_edge.  Graphs must have exactly max_n vertices; agg must be attn_h, (DAGNN_BN) attn_x - the gradient reaches the
        key half of attn_lin through the type table - or (DAGNN_NA) gated_sum, whose gradients reach gate_forward.0.0 /
        mapper_forward.0.0 (the encoder's layer-0 gate and mapper: both add up in .grad)."""
        self._check_decoder_agg("loss(): the teacher-forced decoder")
        if type(G_true) != list:
            G_true = [G_true]
        types, preds = decode_schedule(G_true, self.max_n, self.nvt, int(self.START_TYPE))
        if len(G_true) != mu.shape[0]:
            raise ValueError("loss(): %d graphs for %d latent rows" % (len(G_true), mu.shape[0]))
        if not (mu.is_cuda and self.fc3.weight.is_cuda):
            raise engine.DagnnHipError(_LOSS_NEEDS_GPU)
        t_types = torch.from_numpy(types).pin_memory().to(mu.device, non_blocking=True)
        t_preds = torch.from_numpy(preds).pin_memory().to(mu.device, non_blocking=True)
        return self.loss_dense(mu, logvar, t_types, t_preds, beta)

    def loss_dense(self, mu, logvar, types, preds, beta=0.005):
        """`loss()` on a schedule that is on the device already: types / preds int32 [B, max_n] as `decode_schedule`
        describes them (`DagStore.batch(idx).types` / `.preds`).  The rows are taken as they are - a DagStore checked them
        when it packed them; `loss()` checks its graphs per call - and nothing is built on or copied from the host."""
        self._check_decoder_agg("loss(): the teacher-forced decoder")
        B = mu.shape[0]
        for t, what in ((types, "types"), (preds, "preds")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (B, self.max_n):
                raise ValueError("loss_dense(): %s must be an int32 tensor [%d, max_n=%d] (got %s)"
                                 % (what, B, self.max_n, getattr(t, "shape", type(t))))
        z = self.reparameterize(mu, logvar)
        H0 = self.tanh(self.fc3(z))
        if not H0.is_cuda:
            raise engine.DagnnHipError(_LOSS_NEEDS_GPU)
        if types.device != H0.device or preds.device != H0.device:
            raise ValueError("loss_dense(): types and preds must be on the model's device %s" % H0.device)
        types, preds = types.contiguous(), preds.contiguous()
        dec, params = self._decode_loss_inputs()
        if torch.is_grad_enabled() and any(t.requires_grad for t in [H0] + params):
            res = _DecodeLoss.apply(dec, types, preds, H0, *params)
        else:   # (no autograd record: the saved activations die with this call)
            res = _make_decode(dec, types, preds, H0, params).forward()[2 * H0.shape[0]].clone()
        kld = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
        return res + beta * kld, res, kld

    def _decode_loss_inputs(self):
        """(description, its differentiable parameters) of `_DecodeLoss` / `_make_decode`."""
        dec = self._decoder()
        return dec, dec.params

    def _decoder(self, attached=False):
        """The `_Decoder` of this model (behind `_check_decoder_agg`).  The one place that cuts attn_lin.weight up: its row
        holds the query half up to `_key_offset(0)`, then the key half - hs state columns and (NA) max_n vertex-id columns,
        or with attn_x, whose keys are the one-hot types, a table over the nvt types.  `attached`: the views stay in the
        autograd graph (`_ipropagate_to` under autograd backpropagates through them); otherwise they are detached, as the
        loss - whose gradients come from the library - and the sampling decode want them."""
        cells = [(c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh) for c in list(self.grud)[:self.num_layers]]
        av = [self.add_vertex[0].weight, self.add_vertex[0].bias, self.add_vertex[2].weight, self.add_vertex[2].bias]
        ae = [self.add_edge[0].weight, self.add_edge[0].bias, self.add_edge[2].weight, self.add_edge[2].bias]
        w_key = vid_bias = key_type = gate = vid_off = None
        dq = self._key_offset(0)
        if self.agg == K.NA_GATED_SUM:   # the layer-0 gate and mapper that node_aggr_0[0] shares with the encoder
            agg = _lib.DVAE_AGG_GATED_SUM
            own = [self.gate_forward[0][0].weight, self.gate_forward[0][0].bias, self.mapper_forward[0][0].weight]
            gate = own if attached else [t.detach() for t in own]
        else:
            own = [self.node_aggr_0[0].attn_lin.weight]   # AttnConv.forward with edge_index=None (`dagnn.py:391-399`), stacked layer 0
            w = (own[0] if attached else own[0].detach())[0]
            if self.agg == K.NA_ATTN_X:
                agg, key_type = _lib.DVAE_AGG_ATTN_X, w[dq:dq + self.nvt]
            else:
                agg, w_key = _lib.DVAE_AGG_ATTN_H, w[dq:dq + self.hs]
                if self._use_vids:
                    vid_off = dq + self.hs
                    vid_bias = w[vid_off:vid_off + self.max_n]
        return _Decoder(n=self.max_n, nvt=self.nvt, hs=self.hs, L=len(cells), start_type=int(self.START_TYPE),
                        end_type=int(self.END_TYPE), bn=not self._use_vids, agg=agg,
                        params=own + [t for c in cells for t in c] + av + ae, cells=cells, av=av, ae=ae, w_key=w_key,
                        vid_bias=vid_bias, key_type=key_type, gate=gate, key_off=dq, vid_off=vid_off)

    def _check_decoder_agg(self, what):
        """The decoders serve attn_h, (NA) gated_sum and (BN) attn_x.  The first two read the predecessors' hs-wide states
        (NA: with a one-hot(u, max_n) vertex id) through the encoder's layer-0 module: gated_sum's gate / mapper, attn_h's
        key half of attn_lin, which is hidden_dim (+ num_nodes) wide.  So the reference itself needs hidden_dim == hs and
        (NA) num_nodes == max_n - a shape error otherwise - and the kernels would read the wrong columns.  attn_x keys
        with the predecessors' one-hot types (dvae/dagnn_bn.py:203-225: `_one_hot(type, nvt)` against an emb_dim-wide key
        half), so it needs emb_dim == nvt; the aggregated values are still the hs-wide states."""
        if self.agg == K.NA_SELF_ATTN_X:
            raise NotImplementedError("%s with agg='self_attn_x': the reference's own SelfAttnConv calls an undefined `attn_linear` "
                                      "on this path (dvae/dagnn_bn.py:311-315); the decoders serve attn_h, gated_sum and (DAGNN_BN) "
                                      "attn_x" % (what,))
        if self.agg not in (K.NA_ATTN_H, K.NA_GATED_SUM, K.NA_ATTN_X):
            raise NotImplementedError("%s is built for agg='attn_h' (the reference's D-VAE default, dvae/train.py:86), "
                                      "agg='gated_sum' and (DAGNN_BN) agg='attn_x', not %r" % (what, self.agg))
        if self.agg == K.NA_ATTN_X and self.emb_dim != self.nvt:
            raise ValueError("%s with agg='attn_x' needs emb_dim == nvt: the keys are the one-hot vertex types "
                             "(got emb_dim=%d, nvt=%d)" % (what, self.emb_dim, self.nvt))
        if self.hidden_dim != self.hs or (self._use_vids and self.num_nodes != self.max_n):
            raise ValueError("%s with agg=%r needs hidden_dim == hs%s (got hidden_dim=%d, hs=%d, num_nodes=%d, max_n=%d)"
                             % (what, self.agg, " and num_nodes == max_n" if self._use_vids else "", self.hidden_dim,
                                self.hs, self.num_nodes, self.max_n))

    # ------------------------------------------------------------------ sampling decoder (dvae/models_pyg.py:338-396)
    def decode_dense(self, z, stochastic=True, attempts=1, draws=None, states=False):
        """`decode(z, stochastic)` for `attempts` independent attempts on the same B latent rows, as dense device tensors,
        without synchronising: DecodedDense(types [attempts, B, max_n] int32 (-1 past the end), preds [attempts, B, max_n]
        int32 predecessor bitmasks (bit u: the edge u -> v), nv [attempts, B] int32 vertex counts, states
        [attempts, B, max_n, hs] final top-layer states or None).  Each attempt is decoded exactly as one reference call on
        its B rows.  Sampled draws come from ONE torch.rand call on z's device (so torch.manual_seed makes decoding
        reproducible) unless `draws = (u_type, u_edge)` is given, shaped as `draw_shapes(max_n, B, attempts)`."""
        if self.max_n > 32:
            raise ValueError("decode(): at most 32 vertices per graph (got max_n=%d)" % self.max_n)
        self._check_decoder_agg("decode(): the decoder step")
        if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.shape[1] != self.nz or z.shape[0] == 0:
            raise ValueError("decode(): z must be [B, nz=%d] with B >= 1 (got %s)"
                             % (self.nz, tuple(z.shape) if isinstance(z, torch.Tensor) else type(z)))
        attempts = int(attempts)
        if attempts < 1:
            raise ValueError("decode(): attempts must be >= 1 (got %d)" % attempts)
        with torch.no_grad():
            H0 = self.tanh(self.fc3(z))
            if not H0.is_cuda:
                raise engine.DagnnHipError("decode(): the model must live on a ROCm GPU - the decoder is HIP "
                                           "(csrc/dvae_sample.hip) and has no CPU path")
            B, n = z.shape[0], self.max_n
            h0 = H0.float().repeat(attempts, 1)
            u_type = u_edge = None
            if stochastic:
                st, se = draw_shapes(n, B, attempts)
                if draws is None:
                    u = torch.rand(int(np.prod(st)) + int(np.prod(se)), device=H0.device)
                    u_type, u_edge = u[:int(np.prod(st))].view(st), u[int(np.prod(st)):].view(se)
                else:
                    u_type, u_edge = draws
                    if tuple(u_type.shape) != st or tuple(u_edge.shape) != se:
                        raise ValueError("decode(): draws must be shaped %s and %s" % (st, se))
            types, preds, nv, hs = engine.dvae_sample(h0, attempts, self._decoder(), u_type, u_edge, states)
        return DecodedDense(types.view(attempts, B, n), preds.view(attempts, B, n), nv.view(attempts, B),
                            None if hs is None else hs.view(attempts, B, n, self.hs))

    def decode(self, z, stochastic=True):
        """Graphs decoded from latent vectors z [B, nz] (`DVAE_PYG.decode`, `dvae/models_pyg.py:338-396`): a list of B
        `igraph.Graph`s with a 'type' vertex attribute, or `DecodedGraph`s when igraph is not installed.
        stochastic=True samples every type and edge, False takes the argmax / score > 0.5.  The decode is one HIP call;
        the result reaches the host with one synchronisation."""
        d = self.decode_dense(z, stochastic)
        B, n = d.nv.shape[1], self.max_n
        host = torch.cat([d.types.view(B, n), d.preds.view(B, n), d.nv.view(B, 1)], 1).cpu().numpy()
        return graphs_from_dense(host[:, :n], host[:, n:2 * n], host[:, 2 * n], self.END_TYPE)

    # ------------------------------------------------------------------ decoder-side single-vertex step
    def _get_zeros(self, n, length):
        return torch.zeros(n, length, device=self.get_device())

    def _get_zero_hidden(self, n=1):
        return self._get_zeros(n, self.hs)

    def _one_hot(self, idx, length):
        """`models_pyg.py:98-107`: a list gives one row per entry (None for an empty list), an int one row."""
        if type(idx) in (list, range):
            if len(idx) == 0:
                return None
            ids = torch.tensor(list(idx), dtype=torch.long).view(-1, 1)
        else:
            ids = torch.tensor([[int(idx)]], dtype=torch.long)
        return torch.zeros(ids.shape[0], length).scatter_(1, ids, 1).to(self.get_device())

    def _ipropagate_to(self, G, v, propagator, H=None, reverse=False):
        """New states at vertex `v` of every graph in `G` that has one, from the states of its predecessors
        (`dvae/dagnn.py:187-239`, `dvae/dagnn_bn.py:179-238`; called by the decoder as `_update_iv`,
        `models_pyg.py:247-250`, with `propagator = self.grud`).  `G` holds igraph-style graphs: `g.vcount()`,
        `g.predecessors(v)`, `g.vs[x]['type']`, `g.vs[x]['H_forward<l>']` ([1, hs] tensors, written for `v`).

        ONE HIP launch per call (`dagnn_iprop_step`, csrc/misc.hip) for the padded soft-max aggregate and the L
        stacked GRU cells of all graphs; there is no CPU path (the model must live on the GPU).  Reproduced as the
        reference computes it, quirks included: the predecessor lists are padded to the longest one with zero rows and
        the attention soft-max runs over the padding as well (a zero key scores `w_q.q + b`; that term is common to all
        slots and cancels, so padded slots score 0 and take weight away from the real predecessors - which is why this
        is NOT the encoder's aggregate); and the aggregate is computed from the layer-0 states only and reused by every
        layer above (`H` is no longer None in the later iterations of the reference's loop).  The host side only
        gathers the igraph-style inputs into dense tensors and writes the new states back into the vertices."""
        assert not reverse
        if self.agg in (K.NA_SELF_ATTN_H, K.NA_SELF_ATTN_X):
            raise NotImplementedError("the decoder-side step with agg=%r: the reference's own SelfAttnConv calls an "
                                      "undefined `attn_linear` on this path (dvae/dagnn.py:317-321, dvae/dagnn_bn.py:311-315)"
                                      % (self.agg,))
        typed = self.agg == K.NA_ATTN_X   # keys = the predecessors' one-hot types: a slot scores key_type[type] (dagnn_bn.py:203-225)
        if typed and self.emb_dim != self.nvt:
            raise ValueError("the decoder-side step with agg='attn_x' needs emb_dim == nvt (got emb_dim=%d, nvt=%d)"
                             % (self.emb_dim, self.nvt))
        G = [g for g in G if g.vcount() > v]
        if len(G) == 0:
            return None
        dev = self.get_device()
        if H is not None:
            H = H[list(range(len(G)))].to(dev)   # the reference indexes with the positions of the already filtered list
        X = self._one_hot([g.vs[v]["type"] for g in G], self.nvt)
        values = pred_vid = None
        dec = self._decoder(attached=True)   # (the training caller `loss()` -> `_update_iv` backpropagates through this step)
        if H is None:
            preds = [g.predecessors(v) for g in G]
            P = max(len(p) for p in preds)
            if P > 0:
                rows, ids = [], []
                zero = self._get_zeros(1, self.hs)
                for g, p in zip(G, preds):
                    rows += [g.vs[x]["H_forward0"].to(dev) for x in p] + [zero] * (P - len(p))
                    ids += ([int(g.vs[x]["type"]) for x in p] if typed else list(p)) + [-1] * (P - len(p))
                if typed and not all(-1 <= t < self.nvt for t in ids):
                    raise ValueError("_ipropagate_to: a predecessor's type is not in [0, nvt=%d)" % self.nvt)
                values = torch.cat(rows, 0).view(len(G), P, self.hs)
                pred_vid = torch.tensor(ids, dtype=torch.int32).view(len(G), P).to(dev)
        cells = list(propagator)[:self.num_layers]
        # (`_iprop_dense`, typed: w_key None, the table in vid_bias' place)
        w_key, vid_bias = (None, dec.key_type) if typed else (dec.w_key, dec.vid_bias)
        flat = [t for c in cells for t in (c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh)]
        diff = [t for t in [values, H, w_key, vid_bias] + flat if t is not None]
        if torch.is_grad_enabled() and any(t.requires_grad for t in diff):
            # training (`models_pyg.py:398-442`: the reconstruction loss reaches `grud`, `attn_lin` and `H0 = tanh(fc3(z))`
            # through these states): the same HIP launch forward, its reverse pass behind an autograd.Function
            states = _IpropStep.apply(values, pred_vid, w_key, vid_bias, H, X, len(cells), *flat)
        elif typed:
            states = engine.iprop_step(values, pred_vid, None, None, H, X, cells, key_type=vid_bias)
        else:
            states = engine.iprop_step(values, pred_vid, w_key, vid_bias, H, X, cells)
        for l in range(self.num_layers):
            for i, g in enumerate(G):
                g.vs[v]["H_forward%d" % l] = states[l, i:i + 1]
        return states[self.num_layers - 1]


class DAGNN_NA(_DvaeDagnn):
    """The reference's `dvae/dagnn.py::DAGNN` (keys carry a one-hot vertex id, `:130-134`)."""
    _use_vids = True

    def __init__(self, emb_dim, hidden_dim, out_dim, max_n, nvt, START_TYPE, END_TYPE, hs, nz,
                 num_layers=2, bidirectional=False, agg=K.NA_ATTN_H, out_wx=False, out_pool_all=False,
                 out_pool=K.P_MAX, dropout=0.0, num_nodes=8):
        super().__init__(max_n, nvt, START_TYPE, END_TYPE, hs, nz, bidirectional=bidirectional, num_layers=num_layers)
        self._setup(emb_dim, hidden_dim, out_dim, num_layers, bidirectional, agg, out_wx, out_pool_all, out_pool,
                    dropout, num_nodes)


class DAGNN_BN(_DvaeDagnn):
    """The reference's `dvae/dagnn_bn.py::DAGNN_BN` on `DVAE_BN_PYG` (`models_pyg.py:539-560`)."""
    _use_vids = False

    def __init__(self, emb_dim, hidden_dim, out_dim, max_n, nvt, START_TYPE, END_TYPE, hs, nz, num_layers=2,
                 bidirectional=True, agg=K.NA_ATTN_H, out_wx=False, out_pool_all=False, out_pool=K.P_MAX,
                 dropout=0.0, num_nodes=8):
        super().__init__(max_n, nvt, START_TYPE, END_TYPE, hs, nz, bidirectional=bidirectional, vid=False,
                         num_layers=num_layers)
        # DVAE_BN_PYG (aggx=0) re-creates these with the first layer reading node types
        lin = lambda l, bias: nn.Linear(self.nvt if l == 0 else hs, hs, bias=bias)  # noqa: E731
        self.mapper_forward = nn.ModuleList([nn.Sequential(lin(l, False)) for l in range(num_layers)])
        self.mapper_backward = nn.ModuleList([nn.Sequential(lin(l, False)) for l in range(num_layers)])
        self.gate_forward = nn.ModuleList([nn.Sequential(lin(l, True), nn.Sigmoid()) for l in range(num_layers)])
        self.gate_backward = nn.ModuleList([nn.Sequential(lin(l, True), nn.Sigmoid()) for l in range(num_layers)])
        self.add_edge = nn.Sequential(nn.Linear(hs * 3, hs), nn.ReLU(), nn.Linear(hs, 1))
        self._setup(emb_dim, hidden_dim, out_dim, num_layers, bidirectional, agg, out_wx, out_pool_all, out_pool,
                    dropout, num_nodes)


def _gather_rows(d, a, b):
    """types / preds / nv of the rows (a[i], b[i]) of a DecodedDense, as one int32 matrix [len(a), 2n+1]."""
    return torch.cat([d.types[a, b], d.preds[a, b], d.nv[a, b].view(-1, 1)], 1)


def _last_occurrence(sel, pick, B, A):
    """Per point: the flat index b' * A + a' of the LAST valid attempt of the whole call whose key equals the picked one
    (point-major, attempt-minor - the order in which the reference overwrites `str2igraph`)."""
    W = sel.keys.shape[2]
    keys = sel.keys.reshape(B * A, W)
    ok = sel.valid.t().reshape(B * A) != 0
    idx = torch.arange(B * A, device=keys.device)
    want = sel.keys[torch.arange(B, device=keys.device), pick]
    out = []
    step = max(1, (1 << 24) // (B * A * W))
    for b0 in range(0, B, step):
        eq = (keys.unsqueeze(0) == want[b0:b0 + step].unsqueeze(1)).all(2) & ok
        out.append(torch.where(eq, idx, torch.full_like(idx, -1)).max(1).values)
    return torch.cat(out).clamp(min=0)


def decode_from_latent_space(latent_points, model, decode_attempts=500, n_nodes="variable", return_igraph=False,
                             data_type="ENAS", select="first", chunk=None, draws=None):
    """`decode_from_latent_space` of dvae/util.py:408-466 on the HIP decoder: `decode_attempts` stochastic decodes of
    every latent point, the reference's validity rules, and one string per point - the first valid one in attempt order
    (what the reference returns), or None when no attempt is valid.  Returns the strings, or (graphs, strings) with
    return_igraph: per point the graph of the last attempt of the whole call with the same string (the reference's
    shared `str2igraph` dict), an igraph.Graph or DecodedGraph.  select='most_common' takes the most frequent valid
    string instead (Counter.most_common(1)).

    All attempts' uniforms are drawn at once, laid out as one `decode_dense(attempts=decode_attempts)` call (so
    torch.manual_seed reproduces the result), or given as `draws` shaped as `draw_shapes(max_n, B, decode_attempts)`;
    the decode runs in chunks of `chunk` attempts (default: about SELECT_ROWS rows per call), which does not change the
    result.  Validity, keys and selection are one HIP call; the result reaches the host with one synchronisation."""
    return _decode_and_pick(latent_points, model, decode_attempts, n_nodes, return_igraph, data_type, select, chunk, draws)[0]


def _decode_and_pick(latent_points, model, decode_attempts, n_nodes, return_igraph, data_type, select, chunk, draws, extra=None):
    """The body of `decode_from_latent_space`.  `extra(d, sel, pick)` - d the DecodedDense [A, B, ...] of all attempts, sel
    the SelectedDense, pick [B] int64 the picked attempt per point (0 where none is valid) - may return an int32 [B, E]
    device tensor that rides to the host in the call's one copy.  Returns (result, extra columns on the host or None)."""
    kind = _kind(data_type)
    if n_nodes != "variable" and kind == 0:
        _n_nodes(n_nodes)
    _select_mode(select)
    z = latent_points
    if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.shape[0] == 0:
        raise ValueError("decode_from_latent_space(): latent_points must be a [B, nz] tensor with B >= 1")
    A, B, n = int(decode_attempts), int(z.shape[0]), model.max_n
    if A < 1:
        raise ValueError("decode_from_latent_space(): decode_attempts must be >= 1 (got %d)" % A)
    st, se = draw_shapes(n, B, A)
    if draws is None:
        u = torch.rand(int(np.prod(st)) + int(np.prod(se)), device=z.device)
        u_type, u_edge = u[:int(np.prod(st))].view(st), u[int(np.prod(st)):].view(se)
    else:
        u_type, u_edge = draws
        if tuple(u_type.shape) != st or tuple(u_edge.shape) != se:
            raise ValueError("decode_from_latent_space(): draws must be shaped %s and %s" % (st, se))
    step = max(1, SELECT_ROWS // B) if chunk is None else int(chunk)
    if step < 1:
        raise ValueError("decode_from_latent_space(): chunk must be >= 1 (got %d)" % step)
    parts = [model.decode_dense(z, True, min(A, a0 + step) - a0, (u_type[a0:a0 + step], u_edge[a0:a0 + step]))
             for a0 in range(0, A, step)]
    d = DecodedDense(*(torch.cat([getattr(p, f) for p in parts]) if len(parts) > 1 else getattr(parts[0], f)
                       for f in ("types", "preds", "nv")), None)
    sel = model.select_dense(d, data_type, None if n_nodes == "variable" else n_nodes, select)
    ar = torch.arange(B, device=d.types.device)
    pick = sel.pick.long().clamp(min=0)
    cols = [sel.pick.view(B, 1), _gather_rows(d, pick, ar)]
    if return_igraph:
        last = _last_occurrence(sel, pick, B, A)
        cols.append(_gather_rows(d, last % A, last // A))
    more = None if extra is None else extra(d, sel, pick)
    if more is not None:
        cols.append(more)
    host = torch.cat(cols, 1).cpu().numpy()   # the one synchronisation
    if more is not None:
        host, more = host[:, :host.shape[1] - more.shape[1]], np.ascontiguousarray(host[:, host.shape[1] - more.shape[1]:])
    form = enas_string if kind == 0 else bn_adj_string
    w = 2 * n + 1
    strings = [None if host[b, 0] < 0 else form(host[b, 1:1 + n], host[b, 1 + n:1 + 2 * n], host[b, 2 * n + 1])
               for b in range(B)]
    if not return_igraph:
        return strings, more
    rows = host[:, 1 + w:]
    keep = [b for b in range(B) if host[b, 0] >= 0]
    built = graphs_from_dense(rows[keep, :n], rows[keep, n:2 * n], rows[keep, 2 * n], model.END_TYPE) if keep else []
    graphs = [None] * B
    for b, g in zip(keep, built):
        graphs[b] = g
    return (graphs, strings), more


# ------------------------------------------------------------------ evaluation metrics (dvae/train.py:276-311, prior_validity)
SameDag = namedtuple("SameDag", ["same", "per_graph", "total"])
PriorValidity = namedtuple("PriorValidity", ["r_valid", "r_unique", "r_novel", "n_valid", "n_total", "n_unique", "n_in_train"])


def dense_rows(G, max_n: int, nvt: int):
    """Graphs as dense rows (types [N, max_n] int32, -1 past the end; preds [N, max_n] int32 predecessor bitmasks; nv [N]
    int32 vertex counts): what `decode_schedule` reads of a graph, for graphs of up to max_n vertices - `is_same_DAG`
    compares graphs of any size."""
    if max_n > 32:
        raise ValueError("dense_rows(): at most 32 vertices per graph (got max_n=%d)" % max_n)
    N = len(G)
    types = np.full((N, max_n), -1, dtype=np.int32)
    preds = np.zeros((N, max_n), dtype=np.uint32)
    nv = np.zeros(N, dtype=np.int32)
    for b, g in enumerate(G):
        k = int(g.x.shape[0])
        if not 1 <= k <= max_n:
            raise ValueError("dense_rows(): graph %d has %d vertices, 1..max_n=%d are possible" % (b, k, max_n))
        nv[b] = k
        types[b, :k] = [int(g.vs[v]["type"]) for v in range(k)]
        ei = g.edge_index
        ei = ei.cpu().numpy() if isinstance(ei, torch.Tensor) else np.asarray(ei)
        src, dst = ei[0].astype(np.int64), ei[1].astype(np.int64)
        keep = (src < dst) & (dst < k) & (src >= 0)
        np.bitwise_or.at(preds[b], dst[keep], (np.uint32(1) << src[keep].astype(np.uint32)))
        if types[b, :k].min() < 0 or types[b, :k].max() >= nvt:
            raise ValueError("dense_rows(): vertex types must lie in [0, nvt=%d) (graph %d)" % (nvt, b))
    return types, preds.view(np.int32), nv


def _record(types, preds, nv):
    """What identifies a dense row under `is_same_DAG`: the vertex count, then type and predecessors below v of every
    vertex v < nv (the record csrc/dvae_match.hip compares)."""
    k = max(int(nv), 0)
    return (int(nv),) + tuple(int(t) for t in types[:k]) + tuple(int(p) & ((1 << v) - 1) for v, p in enumerate(preds[:k]))


def is_same_dag_rows(t0, p0, k0, t1, p1, k1):
    """`is_same_DAG` (dvae/util.py:576-585) of two dense rows: it does not check isomorphism."""
    if int(k0) != int(k1):
        return False
    for vi in range(int(k0)):
        if int(t0[vi]) != int(t1[vi]):
            return False
        if int(p0[vi]) & ((1 << vi) - 1) != int(p1[vi]) & ((1 << vi) - 1):
            return False
    return True


def same_dag_host(types, preds, nv, types_true, preds_true, nv_true=None):
    """Host mirror of dagnn_dvae_same_dag on numpy rows, written as the reference's loop: (same [A,B] bool, per_graph
    [B] int32, total)."""
    types, preds, nv = np.asarray(types), np.asarray(preds), np.asarray(nv)
    A, B = nv.shape
    n = types.shape[-1]
    same = np.zeros((A, B), dtype=bool)
    for b in range(B):
        kt = n if nv_true is None else nv_true[b]
        for a in range(A):
            same[a, b] = is_same_dag_rows(types[a, b], preds[a, b], nv[a, b], types_true[b], preds_true[b], kt)
    return same, same.sum(0).astype(np.int32), int(same.sum())


def same_dag_dense(decoded, types_true, preds_true, nv_true=None):
    """`is_same_DAG` of every attempt of a DecodedDense [A,B,...] against true graph b (types_true / preds_true [B,n],
    nv_true [B] or None: max_n vertices each): SameDag(same [A,B], per_graph [B], total [1]), int32.  On the GPU one call
    of dagnn_dvae_same_dag, without synchronising; rows on the host go through the host mirror."""
    if decoded.types.is_cuda:
        return SameDag(*engine.dvae_same_dag(decoded.types, decoded.preds, decoded.nv, types_true, preds_true, nv_true))
    h = lambda x: None if x is None else (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x))  # noqa: E731
    same, per, total = same_dag_host(h(decoded.types), h(decoded.preds), h(decoded.nv), h(types_true), h(preds_true), h(nv_true))
    return SameDag(torch.from_numpy(same.astype(np.int32)), torch.from_numpy(per), torch.tensor([total], dtype=torch.int32))


def _raise_set_error(err: int, what: str):
    if err & _lib.DVAE_SET_ERR_HEADER:
        raise engine.DagnnHipError("%s: the set's storage does not hold the set it was queried as (results are invalid)" % what)
    if err:
        raise engine.DagnnHipError("%s: a bounded probe of the set ran out - the table is full or damaged (results are "
                                   "invalid, device-side error word %d)" % (what, err))


class _DeviceSet(object):
    """Storage and bookkeeping of one set of csrc/dvae_match.hip: the caller-owned buffer, the rows added so far (known
    on the host, so adding needs no read-back) and the device words {distinct count, error}."""

    def __init__(self, form, width, max_rows, device):
        self.form, self.width, self.max_rows, self.rows = form, int(width), int(max_rows), 0
        self.storage = torch.empty(engine.dvae_set_words(form, width, max_rows), dtype=torch.int32, device=device)
        engine.dvae_set_init(self.storage, form, width, max_rows)

    def add(self, rows, mask, count):
        engine.dvae_set_add(self.storage, self.form, self.width, self.max_rows, self.rows, rows, mask)
        self.rows += count

    def status(self):
        """Device view [2] int32: the distinct rows added so far and the error word (no synchronisation)."""
        return self.storage[_lib.DVAE_SET_COUNT:_lib.DVAE_SET_ERR + 1]


def _rows_of(decoded):
    return (decoded.types, decoded.preds, decoded.nv) if hasattr(decoded, "types") else tuple(decoded)


class GraphSet(object):
    """A set of graphs for `ratio_same_DAG(G_train, .)` (dvae/util.py:588-596): built once from the training set,
    queried with decoded rows.  Membership is `is_same_DAG` against any stored graph, exactly (csrc/dvae_match.hip: the
    hash only picks the bucket).  Rows on a GPU make a device set; rows on the host a Python set of the same records,
    the host mirror.  len() is the number of graphs given, duplicates included, as len(G_train)."""

    def __init__(self, n, rows, device_set=None, records=None):
        self.n, self.rows, self._dev, self._records = int(n), int(rows), device_set, records

    @classmethod
    def from_dense(cls, types, preds, nv=None):
        """types / preds [N, n] int32 and nv [N] (None: n vertices each), torch tensors on the GPU (device set) or on
        the host / numpy arrays (host mirror)."""
        if isinstance(types, torch.Tensor) and types.is_cuda:
            N, n = types.shape
            ds = _DeviceSet(_lib.DVAE_SET_GRAPHS, n, N, types.device)
            ds.add((types, preds, nv), None, N)
            return cls(n, N, device_set=ds)
        h = lambda x: None if x is None else (x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x))  # noqa: E731
        types, preds, nv = h(types), h(preds), h(nv)
        N, n = types.shape
        return cls(n, N, records={_record(types[i], preds[i], n if nv is None else nv[i]) for i in range(N)})

    @classmethod
    def from_graphs(cls, G, max_n, nvt, device=None):
        """From graph objects (what `encode` / `loss` take), of up to max_n vertices each; device None: the host mirror."""
        rows = tuple(torch.from_numpy(x) for x in dense_rows(G, max_n, nvt))
        return cls.from_dense(*(rows if device is None else (t.to(device) for t in rows)))

    def __len__(self):
        return self.rows

    def contains(self, decoded, mask=None):
        """(member, count [1]) int32 for a DecodedDense [A,B,...] or a (types, preds, nv) triple: member = 1 where the
        row is in the set and mask (int32, None: all rows) is not 0; count = the number of such rows.  A device set does
        not synchronise."""
        types, preds, nv = _rows_of(decoded)
        if self._dev is not None:
            return engine.dvae_set_query(self._dev.storage, self.n, self._dev.max_rows, types, preds, nv, mask)
        t, p, k = (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (types, preds, nv))
        if t.shape[-1] != self.n:
            raise ValueError("GraphSet.contains(): rows of %d vertices needed (got %s)" % (self.n, t.shape))
        m = np.ones(k.shape, dtype=bool) if mask is None else \
            (mask.cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)).reshape(k.shape) != 0
        member = np.zeros(k.shape, dtype=np.int32)
        for i in zip(*np.nonzero(m)):
            member[i] = _record(t[i], p[i], k[i]) in self._records
        return torch.from_numpy(member), torch.tensor([int(member.sum())], dtype=torch.int32)

    def status(self):
        """Device set: the device words [distinct graphs, error word] (no synchronisation); host mirror: the same on the host."""
        if self._dev is not None:
            return self._dev.status()
        return torch.tensor([len(self._records), 0], dtype=torch.int32)

    def distinct(self):
        """The number of different graphs in the set (one synchronisation on a device set; raises DagnnHipError if the
        build reported a device-side error)."""
        count, err = self.status().tolist()
        _raise_set_error(err, "GraphSet")
        return count


class DistinctKeys(object):
    """`len(set(G_valid_str))` over several `select_dense` results: the distinct canonical keys among the valid rows of
    every call added (equal keys <=> equal strings).  A device set of csrc/dvae_match.hip sized for max_rows rows in all,
    or, with device None or a CPU device, a Python set (the host mirror)."""

    def __init__(self, W, max_rows, device=None):
        self.W = int(W)
        host = device is None or torch.device(device).type == "cpu"
        self._dev = None if host else _DeviceSet(_lib.DVAE_SET_KEYS, W, max_rows, device)
        self._keys = set() if host else None

    def add(self, keys, valid):
        """keys [B,A,W] int64 and valid [A,B] of one SelectedDense."""
        if self._dev is not None:
            self._dev.add(keys, valid, valid.numel())
            return
        k, v = keys.cpu().numpy(), valid.cpu().numpy() != 0
        for a, b in zip(*np.nonzero(v)):
            self._keys.add(tuple(int(x) for x in k[b, a]))

    def status(self):
        """[distinct keys, error word] int32, on the device for a device set (no synchronisation)."""
        if self._dev is not None:
            return self._dev.status()
        return torch.tensor([len(self._keys), 0], dtype=torch.int32)

    def count(self):
        """The distinct count (one synchronisation on a device set)."""
        count, err = self.status().tolist()
        _raise_set_error(err, "DistinctKeys")
        return count


def _take_draws(draws, n, B, attempts, device, what):
    st, se = draw_shapes(n, B, attempts)
    if draws is None:
        u = torch.rand(int(np.prod(st)) + int(np.prod(se)), device=device)
        return u[:int(np.prod(st))].view(st), u[int(np.prod(st)):].view(se)
    if tuple(draws[0].shape) != st or tuple(draws[1].shape) != se:
        raise ValueError("%s: draws must be shaped %s and %s" % (what, st, se))
    return draws


def _store_pair(G):
    """(store, ids) when `G` is the pair that stands for a list of graphs - a DagStore (dagnn_amd/dvae_store.py) and the
    ids of its graphs - else None."""
    if isinstance(G, tuple) and len(G) == 2 and hasattr(G[0], "batch") and hasattr(G[0], "loader") and hasattr(G[0], "arrays"):
        return G[0], G[0]._ids(G[1])
    return None


def extract_latent(model, graphs, batch_size=64):
    """`extract_latent` of dvae/train.py:314-335 without the host round trip: mu [len(graphs), nz] of a data set (a list
    of graphs, or the pair `(store, ids)` of a DagStore and graph ids, which takes every batch from the store),
    encoded in batches of batch_size in evaluation mode, on the model's device.  The reference leaves the model in
    evaluation mode; here the mode the model came in is restored, so a later `reparameterize` is not changed by the call."""
    if int(batch_size) < 1:
        raise ValueError("extract_latent(): batch_size must be >= 1 (got %d)" % batch_size)
    pair = _store_pair(graphs)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            if pair is not None:   # (the per-batch host work is `store.batch`: one small copy, one launch)
                return torch.cat([model.encode_batch(b)[0] for b in pair[0].loader(pair[1], int(batch_size))])
            return torch.cat([model.encode(list(graphs[i:i + batch_size]))[0] for i in range(0, len(graphs), int(batch_size))])
    finally:
        model.train(was_training)


def recon_accuracy(model, G, encode_times=10, decode_times=10, stochastic=True, draws=None, batch_size=None):
    """The reconstruction accuracy `test()` of dvae/train.py:276-311 reports (its counting loop is gone there): per batch
    of graphs (`G`: a list, or the pair `(store, ids)` of a DagStore and graph ids) `mu, logvar = model.encode(batch)`, encode_times times `z = model.reparameterize(mu, logvar)` (mu in
    evaluation mode, a fresh sample in training mode, as the reference's), per z decode_times decodes - one
    `decode_dense(attempts=decode_times)` call - and the count of decodes that are `is_same_DAG` to their input.
    Returns (n_perfect, n_total, per_graph): per_graph [len(G)] int32 on the host, the perfect decodes of each graph out
    of encode_times * decode_times; accuracy = n_perfect / n_total.

    The uniforms of all decodes are drawn at once as `draw_shapes(max_n, len(G), encode_times * decode_times)` (attempt
    e * decode_times + d is decode d of encode e), or given as `draws` in that shape; batches take their columns, so
    batch_size (None: one batch) does not change the draws a graph gets, and torch.manual_seed reproduces a run.  With
    agg='gated_sum' the result does not depend on batch_size at all.  With 'attn_h' it can, as it does on the reference's
    infer_batch_size: that decoder's padded soft-max couples the rows of one decode call (the padding takes weight, and its
    width is the call's largest predecessor count), so a graph's decode depends on the batch it is decoded in.
    Comparing and counting run in HIP (dagnn_dvae_same_dag); the counts reach the host with one synchronisation."""
    pair = _store_pair(G)
    E, D, N, n = int(encode_times), int(decode_times), len(G) if pair is None else int(pair[1].size), model.max_n
    if E < 1 or D < 1 or N < 1:
        raise ValueError("recon_accuracy(): encode_times, decode_times and len(G) must be >= 1 (got %d, %d, %d)" % (E, D, N))
    step = N if batch_size is None else int(batch_size)
    if step < 1:
        raise ValueError("recon_accuracy(): batch_size must be >= 1 (got %d)" % step)
    rows = dense_rows(G, n, model.nvt) if pair is None else None
    dev = model.get_device()
    if dev.type != "cuda":
        raise engine.DagnnHipError("recon_accuracy(): the model must live on a ROCm GPU - the decoder is HIP and has no CPU path")
    if pair is not None and (pair[0].n != n or pair[0].arrays["types"].device != dev):
        raise ValueError("recon_accuracy(): the store must hold max_n=%d-vertex graphs on the model's device %s" % (n, dev))
    true = [torch.from_numpy(x).pin_memory().to(dev, non_blocking=True) for x in rows] if pair is None else None
    u_type = u_edge = None
    if stochastic:
        u_type, u_edge = _take_draws(draws, n, N, E * D, dev, "recon_accuracy()")
    per = []
    with torch.no_grad():
        for g0 in range(0, N, step):
            g1 = min(N, g0 + step)
            if pair is None:
                mu, logvar = model.encode(list(G[g0:g1]))
                tt, pt, nt = (t[g0:g1] for t in true)
            else:   # (the true rows are the batch's own schedule: n vertices each)
                b = pair[0].batch(pair[1][g0:g1])
                tt, pt, nt = b.types, b.preds, None
                mu, logvar = model.encode_batch(b)
            count = None
            for e in range(E):
                z = model.reparameterize(mu, logvar)
                dr = (u_type[e * D:(e + 1) * D, :, g0:g1], u_edge[e * D:(e + 1) * D, :, g0:g1]) if stochastic else None
                res = same_dag_dense(model.decode_dense(z, stochastic, D, dr), tt, pt, nt)
                count = res.per_graph if count is None else count + res.per_graph
            per.append(count)
    per_graph = torch.cat(per).cpu()   # the one synchronisation
    return int(per_graph.sum()), N * E * D, per_graph


def prior_validity(model, train_set, n_latent_points=1000, decode_times=10, data_type="ENAS", z_mean=None, z_std=None,
                   batch_size=None, z=None, draws=None):
    """`prior_validity` of the D-VAE training script (the call dvae/train.py:411 comments out): decode_times decodes of
    n_latent_points points z ~ N(0, I) - times z_std plus z_mean when given (`scale_to_train_range`: mean and std of
    `extract_latent(model, train_graphs)`), or the rows of `z` - and from all of them
        r_valid  = valid decodes (is_valid_ENAS / is_valid_BN) / all decodes,
        r_unique = distinct strings (decode_igraph_to_ENAS / _BN_adj) among the valid decodes / valid decodes,
        r_novel  = 1 - valid decodes that are `is_same_DAG` to a graph of `train_set` / valid decodes; `train_set` is a
               GraphSet on the device the decodes live on (a host mirror with a GPU model is a ValueError).
    Without a valid decode r_unique is 0.0 (the script's rule) and so is r_novel, where the script would divide by zero.
    Returns PriorValidity(r_valid, r_unique, r_novel, n_valid, n_total, n_unique, n_in_train).

    Points are decoded batch_size at a time (None: about SELECT_ROWS rows per call), each batch one
    `decode_dense(attempts=decode_times)`; uniforms are drawn once as `draw_shapes(max_n, points, decode_times)`, or given
    as `draws`, and batches take their columns, so batch_size does not change the draws a point gets; the decodes
    themselves depend on it the way `recon_accuracy` describes (not for gated_sum; for attn_h through the batch's padding
    width, as with the reference's infer_batch_size).  Validity and keys
    (dagnn_dvae_select), the distinct count and the training-set lookup (csrc/dvae_match.hip) stay on the device; the four
    counts reach the host with one synchronisation per call."""
    kind, D = _kind(data_type), int(decode_times)
    dev = model.get_device()
    if z is None:
        P = int(n_latent_points)
        if P < 1:
            raise ValueError("prior_validity(): n_latent_points must be >= 1 (got %d)" % P)
        z = torch.randn(P, model.nz, device=dev)
        if z_std is not None:
            z = z * z_std
        if z_mean is not None:
            z = z + z_mean
    elif not isinstance(z, torch.Tensor) or z.dim() != 2 or z.shape[0] == 0:
        raise ValueError("prior_validity(): z must be a [points, nz] tensor with at least one row")
    P, n = int(z.shape[0]), model.max_n
    if D < 1:
        raise ValueError("prior_validity(): decode_times must be >= 1 (got %d)" % D)
    if P * D > _lib.DVAE_SET_MAX_ROWS:
        raise ValueError("prior_validity(): at most %d decodes per call (got %d x %d)" % (_lib.DVAE_SET_MAX_ROWS, P, D))
    if not isinstance(train_set, GraphSet) or train_set.n != n:
        raise ValueError("prior_validity(): train_set must be a GraphSet of max_n=%d-vertex rows" % n)
    if train_set.status().device != z.device:
        raise ValueError("prior_validity(): train_set lives on %s, the decodes on %s - build it with "
                         "GraphSet.from_graphs(..., device) / from_dense on the model's device"
                         % (train_set.status().device, z.device))
    step = max(1, SELECT_ROWS // D) if batch_size is None else int(batch_size)
    if step < 1:
        raise ValueError("prior_validity(): batch_size must be >= 1 (got %d)" % step)
    u_type, u_edge = _take_draws(draws, n, P, D, z.device, "prior_validity()")
    distinct = DistinctKeys(select_key_words(data_type, n, model.nvt), P * D, z.device)
    n_valid = n_in = None
    for p0 in range(0, P, step):
        p1 = min(P, p0 + step)
        d = model.decode_dense(z[p0:p1], True, D, (u_type[:, :, p0:p1], u_edge[:, :, p0:p1]))
        sel = model.select_dense(d, data_type)
        distinct.add(sel.keys, sel.valid)
        _, hit = train_set.contains(d, sel.valid)
        nv_, ni_ = sel.valid.sum().view(1).to(torch.int32), hit.view(1)
        n_valid, n_in = (nv_, ni_) if n_valid is None else (n_valid + nv_, n_in + ni_)
    host = torch.cat([n_valid, n_in, distinct.status(), train_set.status()[1:]]).cpu()   # the one synchronisation
    n_valid, n_in, n_unique, err_keys, err_train = (int(x) for x in host)
    _raise_set_error(err_keys, "prior_validity(): distinct keys")
    _raise_set_error(err_train, "prior_validity(): training set")
    total = P * D
    return PriorValidity(n_valid / total, n_unique / n_valid if n_valid else 0.0, 1.0 - n_in / n_valid if n_valid else 0.0,
                         n_valid, total, n_unique, n_in)
