"""Synthetic inputs of the benchmark configurations.

The real datasets are not available offline (`ogbg-code2` downloads at first use,
`ogb/graphproppred/dataset_pyg.py:106-118`; `asia_200k.txt` is missing from the checkout), so
every measured figure uses these generators:

* code2-like AST batches (cfg 2/3/5): random DFS-preorder trees + next-token edges between
  consecutive leaves, exactly the edge layout `augment_edge2` produces
  (`ogbg-code/utils2.py:30-78`);
* ENAS rows -> 8-node DAGs (cfg 1), decoded as `decode_ENAS_to_pygraph` (`dvae/util.py:343-385`);
* Bayesian-network rows -> 10-node DAGs (cfg 4), decoded as `decode_BN_to_pygraph`
  (`dvae/util.py:290-339`).
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

from .dag_utils import add_order_info, add_order_info_01
from .data import GraphBatch, GraphData


# --------------------------------------------------------------------------- code2-like ASTs
def gen_ast(rng: np.random.Generator, n: int) -> dict:
    """One random AST in DFS pre-order with next-token edges (Appendix E, verbatim draw order)."""
    parent = np.full(n, -1)
    depth = np.zeros(n, dtype=np.int64)
    stack = [0]
    for i in range(1, n):
        k = min(len(stack) - 1, rng.geometric(0.45) - 1)
        for _ in range(k):
            stack.pop()
        parent[i] = stack[-1]
        depth[i] = depth[stack[-1]] + 1
        stack.append(i)
    haschild = np.zeros(n, bool)
    haschild[parent[1:]] = True
    leaves = np.where(~haschild)[0]
    ast = np.stack([parent[1:], np.arange(1, n)])  # parent -> child
    nt = np.stack([leaves[:-1], leaves[1:]])  # next-token
    ei = np.concatenate([ast, nt], 1)
    ea = np.concatenate([np.zeros((ast.shape[1], 2)),
                         np.stack([np.ones(nt.shape[1]), np.zeros(nt.shape[1])], 1)], 0).astype(np.float32)
    x = np.stack([rng.integers(0, 98, n), rng.integers(0, 10030, n)], 1)
    return dict(n=n, ei=ei, ea=ea, x=x, depth=depth)


def code2_graphs(seed: int, num_graphs: int, mean_n: int = 125, max_n: int = 1000) -> List[GraphData]:
    """`num_graphs` code2-like graphs drawn one after another from `default_rng(seed)`."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(num_graphs):
        n = int(np.clip(rng.lognormal(np.log(mean_n) - 0.18, 0.6), 11, max_n))
        g = gen_ast(rng, n)
        d = GraphData(
            x=torch.from_numpy(g["x"]).long(),
            node_depth=torch.from_numpy(g["depth"]).long().view(-1, 1),
            edge_index=torch.from_numpy(g["ei"]).long(),
            edge_attr=torch.from_numpy(g["ea"]),
        )
        add_order_info_01(d)
        out.append(d)
    return out


def code2_batch(seed: int = 0, num_graphs: int = 128, mean_n: int = 125, max_n: int = 1000) -> GraphBatch:
    """The headline batch: seed 0, B=128 -> N=16 561, E=25 377, T=374."""
    return GraphBatch.from_data_list(code2_graphs(seed, num_graphs, mean_n, max_n))


# --------------------------------------------------------------------------- D-VAE graphs
def _adj_to_graph(adj: np.ndarray, types: Sequence[int], n_types: int) -> GraphData:
    # networkx.DiGraph(adj).edges enumerates the non-zeros row by row (source-major), which
    # is what the reference's decoders hand to torch (util.py:325,372)
    src, dst = np.nonzero(adj)
    x = torch.zeros(len(types), n_types)
    x[torch.arange(len(types)), torch.tensor(list(types))] = 1.0
    g = GraphData(x=x, edge_index=torch.from_numpy(np.stack([src, dst])).long())
    add_order_info(g)
    g.vs = [{"type": int(t)} for t in types]
    return g


def decode_enas_row(row, n_types: int = 6) -> GraphData:
    """ENAS row [[type, conn_0..conn_{i-1}], ...] -> 8-node DAG with start(0)/end(1) vertices:
    chain i -> i+1 plus the listed skip connections (`dvae/util.py:343-385`)."""
    n_types += 2
    n = len(row)
    adj = np.zeros((n_types, n_types))
    types = [0]
    for i, node in enumerate(row):
        types.append(node[0] + 2)
        adj[i, i + 1] = 1
        for j, e in enumerate(node[1:]):
            if e == 1:
                adj[j, i + 1] = 1
    types.append(1)
    adj[n, n + 1] = 1
    return _adj_to_graph(adj, types, n_types)


def decode_bn_row(row, n_types: int = 8) -> GraphData:
    """BN row -> 10-node DAG: parentless nodes hang off the start vertex, loose ends feed the end
    vertex (`dvae/util.py:290-339`)."""
    n_types += 2
    n = len(row)
    adj = np.zeros((n_types, n_types))
    loose = [True] * n
    types = [0]
    for i, node in enumerate(row):
        types.append(node[0] + 2)
        if sum(node[1:]) == 0:
            adj[0, i + 1] = 1
        else:
            for j, e in enumerate(node[1:]):
                if e == 1:
                    adj[j + 1, i + 1] = 1
                    loose[j] = False
    types.append(1)
    for j, flag in enumerate(loose):
        if flag:
            adj[j + 1, n + 1] = 1
    return _adj_to_graph(adj, types, n_types)


def enas_rows(seed: int, num_graphs: int) -> list:
    """ENAS-shaped rows (6 op types, 6 layers, random skips) when the real file is not at hand."""
    rng = np.random.default_rng(seed)
    return [[[int(rng.integers(0, 6))] + [int(rng.random() < 0.4) for _ in range(i)] for i in range(6)]
            for _ in range(num_graphs)]


def bn_rows(seed: int, num_graphs: int) -> list:
    """Synthetic Bayesian-network rows (Appendix E): permutation of 8 types, parent w.p. 0.3."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(num_graphs):
        perm = rng.permutation(8)
        out.append([[int(perm[i])] + [int(rng.random() < 0.3) for _ in range(i)] for i in range(8)])
    return out


def asia_samples(seed: int, S: int) -> np.ndarray:
    """S samples int64 [S, 8] of the textbook Asia network (Lauritzen and Spiegelhalter 1988), columns A, S, T, L, B, E, X, D,
    1 = yes: a workload for `bn_score` where bnlearn's `data(asia)` - the table the reference scores on - is not at hand.
    It is drawn here from the network's published probabilities, so scores on it are NOT the reference's numbers."""
    rng = np.random.default_rng(seed)
    u = rng.random((int(S), 8))
    a = u[:, 0] < 0.01
    s = u[:, 1] < 0.5
    t = u[:, 2] < np.where(a, 0.05, 0.01)
    l = u[:, 3] < np.where(s, 0.1, 0.01)   # noqa: E741
    b = u[:, 4] < np.where(s, 0.6, 0.3)
    e = t | l
    x = u[:, 6] < np.where(e, 0.98, 0.05)
    d = u[:, 7] < np.where(b, np.where(e, 0.9, 0.8), np.where(e, 0.7, 0.1))
    return np.stack([a, s, t, l, b, e, x, d], axis=1).astype(np.int64)


def dvae_batch(graphs: Sequence[GraphData]) -> GraphBatch:
    """Collate D-VAE graphs the way `dvae/batch.py:26-146` does (`bi_layer_index` row 1 shifted)."""
    return GraphBatch.from_data_list([g for g in graphs])


# --------------------------------------------------------------------------- decoded graphs (decode_from_latent_space)
def _loose_ends(preds: np.ndarray, k: int) -> int:
    """END's predecessor mask as the decoder sets it: every vertex 0..k-2 without a successor."""
    has_succ = 0
    for v in range(k - 1):
        has_succ |= int(preds[v])
    return sum(1 << u for u in range(k - 1) if not has_succ >> u & 1)


def _template(rng, kind: str, n: int, nvt: int, start: int, end: int):
    if kind == "ENAS":
        k = n if rng.random() < 0.5 else int(rng.integers(3, n + 1))
        types = [start] + [int(t) for t in rng.integers(2, nvt, size=k - 2)] + [end]
    else:
        k = min(nvt, n)
        mid = [t for t in range(nvt) if t not in (start, end)][:k - 2]
        types = [start] + [int(t) for t in rng.permutation(mid)] + [end]
    preds = np.zeros(n, dtype=np.int64)
    for v in range(1, k - 1):
        if kind == "ENAS":
            preds[v] = 1 << (v - 1)
        for u in range(v):
            if rng.random() < 0.3:
                preds[v] |= 1 << u
        if preds[v] == 0:
            preds[v] = 1 << int(rng.integers(0, v))
    preds[k - 1] = _loose_ends(preds, k)
    return k, types, preds


def _reorder(rng, k: int, types, preds):
    """The same graph in another topological order of its middle vertices: equal BN string, different rows."""
    succ = {v: [w for w in range(1, k - 1) if preds[w] >> v & 1] for v in range(1, k - 1)}
    indeg = {v: sum(1 for u in range(1, k - 1) if preds[v] >> u & 1) for v in range(1, k - 1)}
    ready, order = [v for v in range(1, k - 1) if indeg[v] == 0], []
    while ready:
        v = ready.pop(int(rng.integers(0, len(ready))))
        order.append(v)
        for w in succ[v]:
            indeg[w] -= 1
            if indeg[w] == 0:
                ready.append(w)
    pos = {0: 0, k - 1: k - 1}
    pos.update({v: i + 1 for i, v in enumerate(order)})
    t2, p2 = list(types), np.zeros_like(preds)
    for v in range(k):
        t2[pos[v]] = types[v]
        for u in range(v):
            if preds[v] >> u & 1:
                p2[pos[v]] |= 1 << pos[u]
    return t2, p2


def decoded_rows(seed: int, kind: str, A: int, B: int, n: int, nvt: int, start: int = 0, end: int = 1):
    """Decoder-shaped dense rows (types [A,B,n] int32, -1 past the end; preds [A,B,n] int32 bitmasks; nv [A,B] int32) for
    the validity and selection checks of `decode_from_latent_space`.  Each point draws its attempts from three graphs
    with uneven odds (so the first valid string is often not the most frequent one; for BN each graph also comes in a
    second vertex order with the same string), and spoils some: a middle vertex of START type, a middle vertex without
    predecessors, a missing chain edge (END then joins two loose ends), an early END, duplicate BN types.  A few points
    spoil every attempt, and some rows carry stray bits at or above the vertex and past the end, which the rules ignore."""
    rng = np.random.default_rng(seed)
    types = np.full((A, B, n), -1, dtype=np.int32)
    preds = np.zeros((A, B, n), dtype=np.int64)
    nv = np.zeros((A, B), dtype=np.int32)
    for b in range(B):
        pool = []
        for _ in range(3):
            k, t, p = _template(rng, kind, n, nvt, start, end)
            pool.append([(k, t, p), (k,) + _reorder(rng, k, t, p)] if kind == "BN" else [(k, t, p)])
        odds = rng.permutation([0.15, 0.5, 0.35])
        hopeless = rng.random() < 0.1
        for a in range(A):
            forms = pool[int(rng.choice(3, p=odds))]
            k, t, p = forms[int(rng.integers(0, len(forms)))]
            t, p = list(t), p.copy()
            if hopeless or rng.random() < 0.4:
                how = int(rng.integers(0, 5))
                v = int(rng.integers(1, max(2, k - 1)))
                if how == 0 and k > 2:
                    t[v] = start
                elif how == 1 and k > 2:
                    p[v] = 0
                    p[k - 1] = _loose_ends(p, k)
                elif how == 2 and k > 3 and kind == "ENAS":
                    v = int(rng.integers(2, k - 1))
                    p[v] &= ~(1 << (v - 1))
                    if p[v] == 0:
                        p[v] = 1
                    p[k - 1] = _loose_ends(p, k)
                elif how == 3 and k > 3:
                    k2 = int(rng.integers(2, k))
                    t = t[:k2 - 1] + [end]
                    p = p.copy()
                    p[k2:] = 0
                    p[k2 - 1] = _loose_ends(p, k2)
                    k = k2
                elif k > 3:
                    w = int(rng.integers(1, k - 1))
                    t[v] = t[w] if w != v else t[v % (k - 2) + 1]
                    if kind == "ENAS":
                        t[v] = nvt - 1 - (t[v] - 2) % (nvt - 2)
                if hopeless:
                    t[1 if k >= 3 else 0] = start if k >= 3 else end
            types[a, b, :k] = t
            preds[a, b] = p
            nv[a, b] = k
            if rng.random() < 0.1:   # stray bits the rules must ignore
                for v in range(n):
                    preds[a, b, v] |= int(rng.integers(0, 1 << 31)) & ~((1 << v) - 1 if v < k else 0)
                if k < n:
                    types[a, b, k] = int(rng.integers(0, nvt))
    return types, (preds & 0xFFFFFFFF).astype(np.uint32).view(np.int32), nv


# --------------------------------------------------------------------------- decoded graphs against true / training graphs
def match_rows(seed: int, kind: str, A: int, B: int, n: int, nvt: int, n_train: int = 300, start: int = 0, end: int = 1,
               all_invalid: bool = False):
    """Rows for the evaluation metrics (`is_same_DAG`, `ratio_same_DAG`, uniqueness) on top of `decoded_rows`: a dict of
    decoded rows types / preds [A,B,n], nv [A,B]; true rows types_true / preds_true [B,n], nv_true [B]; training rows
    types_train / preds_train [n_train,n], nv_train [n_train].  By construction (A >= 5, B >= 2):
    true row b equals decode (b % A, b); the next four attempts of point b are that row with one middle type changed,
    with one edge bit flipped, cut to one vertex less (equal in all vertices it keeps), and - when it has room - grown by
    one vertex (equal in the first nv).  True and training rows carry junk past their end that must not take part.
    Point 0 has no valid attempt (a second START); with all_invalid every point is spoiled that way (an empty valid
    set).  The training set holds decoded rows of every kind - valid ones, invalid ones (in the set, but never counted:
    novelty only looks at valid decodes), each BN graph in at most the vertex order it was drawn in (its other order
    has the same string and is not the same DAG) - then rows of another seed that match nothing, and its second half
    repeats rows of the first (duplicates)."""
    if A < 5 or B < 2:
        raise ValueError("match_rows: needs A >= 5 and B >= 2")
    rng = np.random.default_rng(seed + 7919)
    types, preds, nv = decoded_rows(seed, kind, A, B, n, nvt, start, end)
    types, preds, nv = types.copy(), preds.view(np.uint32).astype(np.int64), nv.copy()
    types_true = np.empty((B, n), dtype=np.int32)
    preds_true = np.zeros((B, n), dtype=np.int64)
    nv_true = np.empty(B, dtype=np.int32)

    def junk(t, p, k):   # what the rules must ignore: entries past the end, bits at or above the vertex
        for v in range(n):
            p[v] |= int(rng.integers(0, 1 << 31)) & ~((1 << v) - 1) & 0xFFFFFFFF
            if v >= k:
                t[v] = int(rng.integers(0, nvt))
                p[v] = int(rng.integers(0, 1 << 31))

    for b in range(B):
        a0 = b % A
        k = int(nv[a0, b])
        types_true[b], preds_true[b], nv_true[b] = types[a0, b], preds[a0, b], k
        clean_t = types[a0, b].copy()
        clean_t[k:] = -1
        clean_p = preds[a0, b] & [((1 << v) - 1) if v < k else 0 for v in range(n)]
        for j, how in enumerate(("type", "edge", "shorter", "longer")):
            a = (a0 + 1 + j) % A
            t, p, kk = clean_t.copy(), clean_p.copy(), k
            v = int(rng.integers(1, max(2, k - 1))) if k > 2 else 0
            if how == "type":
                others = [x for x in range(nvt) if x != t[v]]
                t[v] = others[int(rng.integers(0, len(others)))]
            elif how == "edge":
                v = max(v, 1) if k > 1 else 0
                if v:
                    p[v] ^= 1 << int(rng.integers(0, v))
                else:
                    t[0] = (t[0] + 1) % nvt
            elif how == "shorter" and k > 1:
                kk = k - 1
                t[kk:], p[kk:] = -1, 0
            elif how == "longer" and k < n:
                kk = k + 1
                t[k], p[k] = end, int(rng.integers(0, 1 << k))
            else:
                t[0] = (t[0] + 1) % nvt
            types[a, b], preds[a, b], nv[a, b] = t, p, kk
        junk(types_true[b], preds_true[b], k)
    spoil = range(B) if all_invalid else [0]
    for b in spoil:
        for a in range(A):
            if nv[a, b] >= 2:
                types[a, b, 1] = start
            else:
                types[a, b, 0] = end
    flat_t, flat_p, flat_k = types.reshape(A * B, n), preds.reshape(A * B, n), nv.reshape(A * B)
    other = decoded_rows(seed + 100003, kind, 1, max(n_train, 1), n, nvt, start, end)
    half = (n_train + 1) // 2
    types_train = np.empty((n_train, n), dtype=np.int32)
    preds_train = np.zeros((n_train, n), dtype=np.int64)
    nv_train = np.empty(n_train, dtype=np.int32)
    for i in range(n_train):
        if i >= half:
            src = int(rng.integers(0, half))
            types_train[i], preds_train[i], nv_train[i] = types_train[src], preds_train[src], nv_train[src]
        elif i % 3 != 2:
            r = int(rng.integers(0, A * B))
            types_train[i], preds_train[i], nv_train[i] = flat_t[r], flat_p[r], flat_k[r]
        else:
            types_train[i], preds_train[i], nv_train[i] = other[0][0, i], other[1].view(np.uint32)[0, i], other[2][0, i]
        if i < half:
            junk(types_train[i], preds_train[i], int(nv_train[i]))
    as_i32 = lambda p: (p & 0xFFFFFFFF).astype(np.uint32).view(np.int32)  # noqa: E731
    return dict(types=types, preds=as_i32(preds), nv=nv, types_true=types_true, preds_true=as_i32(preds_true), nv_true=nv_true,
                types_train=types_train, preds_train=as_i32(preds_train), nv_train=nv_train)
