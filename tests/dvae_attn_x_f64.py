"""Float64 restatement of the BN D-VAE with the input-keyed aggregators (`agg` = attn_x / self_attn_x,
dvae/dagnn_bn.py:48-59,129-131,203-225): the checker of the new paths of `dagnn_amd.DAGNN_BN`, never the thing measured.
`tests/test_dvae_bn_attn_x_cpu.py` pins every function here to the fixtures the unmodified reference wrote.

* `encode`        - `DAGNN_BN.forward` / `.encode` (dagnn_bn.py:98-177) on `oracle.dagnn_oracle._Cfg(..., agg)` with
                    `recurrence_csr` / `recurrence_faithful` (which handle `keys_from_x`), plus the BN read-outs;
* `decoder_loss`  - the teacher-forced `loss()` (models_pyg.py:398-456) with `_ipropagate_to`'s type-keyed aggregate
                    (dagnn_bn.py:203-228), at any dtype: float64 is the reference, float32 the yardstick of the GPU bounds;
* `type_keyed`    - a context in which `oracle.dvae_decoder_oracle` (imported, not edited) takes agg='attn_x': its `_Model`
                    is replaced by a subclass with the type-keyed aggregate, so `decoder_loss` / `replay_decode` there run
                    the BN decoder with it;
* `iprop_step`    - one `_ipropagate_to` call on dense inputs.

The full logit is kept everywhere - query half, key half and bias of `attn_lin` - as the reference computes it; that the
query part and the bias cancel in the soft-max is what the kernels rely on and what these functions check."""
from __future__ import annotations

import contextlib
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dagnn_oracle as O
from oracle import dvae_decoder_oracle as DO

Tensor = torch.Tensor
F64 = torch.float64
ATTN = "node_aggr_0.0.attn_lin."


def leaves(sd: Dict[str, Tensor], dtype=F64) -> Dict[str, Tensor]:
    """One leaf per storage of the state dict, under every name of that storage (cells_0 == grue_forward): the
    reference's .grad of a shared module is the sum over its uses."""
    by_ptr, out = {}, {}
    for k, v in sd.items():
        key = (v.data_ptr(), tuple(v.shape), tuple(v.stride()))
        if key not in by_ptr:
            by_ptr[key] = v.detach().to(dtype).clone().requires_grad_(True) if v.is_floating_point() else v
        out[k] = by_ptr[key]
    return out


def leaf_grads(lv: Dict[str, Tensor]) -> Dict[str, Tensor]:
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in lv.items() if v.is_floating_point()}


# ------------------------------------------------------------------ encoder
def encode(sd: Dict[str, Tensor], G, *, L: int, bidirectional: bool, num_nodes: int, agg: str, out_pool_all: bool = False,
           out_pool: str = "max", mode: str = "csr", dtype=F64):
    """(Hg, mu, logvar) of `DAGNN_BN` on a collated batch; differentiable in the tensors of `sd`."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    dirs = [0, 1] if bidirectional else [0]
    H = sd["cells_0.0.weight_hh"].shape[1]
    x = G.x.to(dtype)
    layers = [G.bi_layer_index[0][0], G.bi_layer_index[1][0]]
    cfg = O._Cfg(sd, dirs, L, H, "cells_", False, 0, agg)
    h = (O.recurrence_faithful if mode == "faithful" else O.recurrence_csr)(cfg, x, G.edge_index, None, layers)
    N = x.shape[0]
    if out_pool_all:   # dagnn_bn.py:153-165: per-node projection, then pooling over all nodes of a graph
        hn = torch.cat([h[q][l] for q in range(len(dirs)) for l in range(L)], -1)
        if bidirectional:
            hn = hn @ sd["hg_unify.0.weight"].t() + sd["hg_unify.0.bias"]
        elif L > 1:
            hn = hn @ sd["out_linear.weight"].t() + sd["out_linear.bias"]
        Hg = O._pool(hn, G.batch, out_pool)
    else:              # dagnn_bn.py:138-152: the end vertex of every graph for d = 0, the start vertex for d = 1
        first = torch.arange(0, N, num_nodes)
        last = first + (num_nodes - 1)
        hc = torch.cat([h[0][l][last] for l in range(L)] + ([h[1][l][first] for l in range(L)] if bidirectional else []), -1)
        if bidirectional:
            Hg = hc @ sd["hg_unify.0.weight"].t() + sd["hg_unify.0.bias"]
        else:
            Hg = hc @ sd["out_linear.weight"].t() + sd["out_linear.bias"] if L > 1 else hc
    return Hg, Hg @ sd["fc1.weight"].t() + sd["fc1.bias"], Hg @ sd["fc2.weight"].t() + sd["fc2.bias"]


# ------------------------------------------------------------------ the type-keyed aggregate
def _padded_softmax_aggregate(base: Tensor, key: Tensor, sel: Tensor, P: int, vals: Tensor) -> Tensor:
    """`AttnConv.forward(edge_index=None)` over P slots: base [R] = w_q . x_v + b, key [R, v] = the key score of every
    earlier vertex, sel [R, v] the real predecessors, vals [R, v, hs] their layer-0 states.  The P - count zero padding
    rows score `base` alone (multiplicity m enters as + log m) and carry zero values."""
    s = base.unsqueeze(1) + key
    pad = (P - sel.sum(1)).to(base.dtype)
    s = torch.where(sel, s, s.new_full((), float("-inf")))
    logpad = torch.where(pad > 0, base + torch.log(pad.clamp(min=1)), base.new_full((), float("-inf")))
    alpha = torch.softmax(torch.cat([s, logpad.unsqueeze(1)], 1), 1)[:, :-1]
    return torch.einsum("rv,rvh->rh", alpha, vals)


def _attn_x_halves(sd, nvt, cast):
    w = cast(sd[ATTN + "weight"])[0]
    assert w.shape[0] == 2 * nvt, "attn_x on the BN model: attn_lin is Linear(2 nvt, 1)"
    return w[:nvt], w[nvt:], cast(sd[ATTN + "bias"])[0]


def decoder_loss(sd: Dict[str, Tensor], types, preds, H0: Tensor, *, L: int, start_type: int = 0, dtype=F64):
    """`(res, vertex_ll [B], edge_ll [B])` of the teacher-forced BN decoder with agg='attn_x', in `dtype`.  Vertex v is
    updated v+1 times, update k reading v's true predecessors >= k with the padding width of the batch in that call; the
    edge probability is the float32 sigmoid of `oracle.dvae_decoder_oracle._Sigmoid32` at every dtype (the reference's
    binary_cross_entropy sees a float32 p)."""
    cast = lambda t: t.to(dtype)  # noqa: E731
    types = torch.as_tensor(np.asarray(types)).long().clone()
    types[:, 0] = start_type
    bits = DO._bits(preds)
    B, n = types.shape
    nvt, hs = sd["add_vertex.2.weight"].shape[0], sd["fc3.weight"].shape[0]
    cells = [tuple(cast(sd["grud.%d.%s" % (l, w)]) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for l in range(L)]
    av = [cast(sd["add_vertex.%s" % k]) for k in ("0.weight", "0.bias", "2.weight", "2.bias")]
    ae = [cast(sd["add_edge.%s" % k]) for k in ("0.weight", "0.bias", "2.weight", "2.bias")]
    wq, wk, ab = _attn_x_halves(sd, nvt, cast)
    onehot = lambda t: F.one_hot(t, nvt).to(dtype)  # noqa: E731
    H0 = H0.to(dtype)
    key = onehot(types) @ wk           # [B, n]: the key score of every vertex
    h0s, tops, edge_rows = [], [], []
    for v in range(n):
        X = onehot(types[:, v])
        if v == 0:
            ks, H = [0], H0
        else:
            ks, aggs = list(range(v, -1, -1)), []
            base, vals = X @ wq + ab, torch.stack(h0s, 1)
            for k in ks:
                sel = bits[:, v, :v] & (torch.arange(v) >= k)
                P = int(sel.sum(1).max())
                aggs.append(X.new_zeros(B, hs) if P == 0 else _padded_softmax_aggregate(base, key[:, :v], sel, P, vals))
            H, X = torch.cat(aggs, 0), X.repeat(len(ks), 1)
        st, x = [], X
        for c in cells:
            x = O.gru_cell(x, H, *c)
            st.append(x)
        if v > 0:
            for i, k in enumerate(ks[:-1]):
                edge_rows.append((v, k - 1, st[-1][i * B:(i + 1) * B]))
            st = [s[v * B:] for s in st]   # the final update (k = 0)
        h0s.append(st[0])
        tops.append(st[-1])
    Hg = torch.stack([sum(tops[:v]) for v in range(1, n)], 0)                 # BN: the sum of the top states
    logits = torch.relu(Hg @ av[0].t() + av[1]) @ av[2].t() + av[3]
    vll = torch.log_softmax(logits, -1).gather(2, types[:, 1:].t().unsqueeze(-1))[..., 0].sum(0)
    Hvi = torch.stack([tops[vi] for _, vi, _ in edge_rows], 0)
    Hv = torch.stack([h for _, _, h in edge_rows], 0)
    y = torch.stack([bits[:, v, vi] for v, vi, _ in edge_rows], 0).to(F64)
    xe = torch.cat([Hvi, Hv, H0.expand(len(edge_rows), B, hs)], -1)
    logit = (torch.relu(xe @ ae[0].t() + ae[1]) @ ae[2].t() + ae[3])[..., 0]
    ell = -F.binary_cross_entropy(DO._Sigmoid32.apply(logit.double()), y, reduction="none").sum(0)
    return -(vll.sum() + ell.sum()), vll, ell


def loss_grads(sd: Dict[str, Tensor], types, preds, mu: Tensor, logvar: Tensor, *, L: int, start_type: int = 0, beta=0.005,
               dtype=F64):
    """`loss()` in evaluation mode (z = mu) and its gradients in `dtype`: (loss, res, kld, vertex_ll, edge_ll,
    {name: gradient}) for mu, logvar and every floating tensor of `sd` (zeros where it takes no part)."""
    lv = leaves(sd, dtype)
    mu = mu.detach().to(dtype).clone().requires_grad_(True)
    logvar = logvar.detach().to(dtype).clone().requires_grad_(True)
    H0 = torch.tanh(mu @ lv["fc3.weight"].t() + lv["fc3.bias"])
    res, vll, ell = decoder_loss(lv, types, preds, H0, L=L, start_type=start_type, dtype=dtype)
    kld = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
    loss = res + beta * kld
    loss.backward()
    grads = dict(leaf_grads(lv), mu=mu.grad, logvar=logvar.grad)
    return loss.detach(), res.detach(), kld.detach(), vll.detach(), ell.detach(), grads


# ------------------------------------------------------------------ oracle.dvae_decoder_oracle with agg='attn_x'
@contextlib.contextmanager
def type_keyed(types, nv, start_type: int = 0):
    """Within the context `DO.decoder_loss` / `DO.replay_decode` accept kind='bn', agg='attn_x' for the graphs (types
    [B, n], nv [B] vertex counts).  Their `_Model.aggregate` gets the rows of one `_ipropagate_to` call without the
    predecessors' types, so the model is bound to the graphs: the rows of a call for vertex v are the graphs with nv > v
    in ascending order - all of them under teacher forcing, the rows still alive in `replay_decode`."""
    tt = torch.as_tensor(np.asarray(types)).long().clone()
    tt[:, 0] = start_type
    counts = np.asarray(nv).astype(np.int64)

    class TypeKeyed(DO._Model):
        def __init__(self, sd, kind, agg, L, max_n):
            if agg != "attn_x":
                super().__init__(sd, kind, agg, L, max_n)
                return
            if kind != "bn":
                raise NotImplementedError((kind, agg))   # dvae/dagnn.py:28
            g = lambda k: sd[k].to(F64)  # noqa: E731
            self.bn, self.agg, self.L, self.n = True, agg, L, max_n
            self.hs, self.nvt = sd["fc3.weight"].shape[0], sd["add_vertex.2.weight"].shape[0]
            self.cells = [tuple(g("grud.%d.%s" % (l, w)) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                          for l in range(L)]
            self.av = [g("add_vertex.%s" % k) for k in ("0.weight", "0.bias", "2.weight", "2.bias")]
            self.ae = [g("add_edge.%s" % k) for k in ("0.weight", "0.bias", "2.weight", "2.bias")]
            self.wq, self.wk, self.ab = _attn_x_halves(sd, self.nvt, lambda t: t.to(F64))

        def aggregate(self, X, sel, P, h0s, msgs):
            if self.agg != "attn_x":
                return super().aggregate(X, sel, P, h0s, msgs)
            R, v = sel.shape
            if P == 0:
                return X.new_zeros(R, self.hs)
            rows = torch.from_numpy(np.nonzero(counts > v)[0])
            assert len(rows) == R, (len(rows), R, v)
            key = self.onehot(tt[rows, :v].clamp(min=0)) @ self.wk
            return _padded_softmax_aggregate(X @ self.wq + self.ab, key, sel, P, torch.stack(h0s, 1))

    saved = DO._Model
    DO._Model = TypeKeyed
    try:
        yield
    finally:
        DO._Model = saved


# ------------------------------------------------------------------ single-vertex step
def iprop_step(sd: Dict[str, Tensor], x_type, pred_types: Optional[List[List[int]]], values: Optional[Tensor], *, L: int,
               H: Optional[Tensor] = None, dtype=F64):
    """One `_ipropagate_to(G, v, grud)` call with agg='attn_x' (dagnn_bn.py:179-233) for the graphs that have the vertex:
    x_type [B] its types, pred_types[b] the types of graph b's predecessors in ascending vertex order, values[b] their
    layer-0 states ([len, hs]); `H` [B, hs] given: the aggregate is skipped.  Returns the states [L, B, hs]."""
    cast = lambda t: t.to(dtype)  # noqa: E731
    nvt, hs = sd["add_vertex.2.weight"].shape[0], sd["fc3.weight"].shape[0]
    wq, wk, ab = _attn_x_halves(sd, nvt, cast)
    X = F.one_hot(torch.as_tensor(x_type).long(), nvt).to(dtype)
    B = X.shape[0]
    if H is None:
        P = max(len(p) for p in pred_types)
        if P == 0:
            H = X.new_zeros(B, hs)
        else:   # the reference's own form: zero key rows and zero value rows up to P, the full logit in the soft-max
            keys, vals = X.new_zeros(B, P, nvt), X.new_zeros(B, P, hs)
            for b, p in enumerate(pred_types):
                for j, t in enumerate(p):
                    keys[b, j, t] = 1
                    vals[b, j] = cast(values[b][j])
            s = (X @ wq + ab).unsqueeze(1) + keys @ wk
            H = torch.einsum("bp,bph->bh", torch.softmax(s, 1), vals)
    else:
        H = cast(H)
    out, x = [], X
    for l in range(L):
        x = O.gru_cell(x, H, *(cast(sd["grud.%d.%s" % (l, w)]) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
        out.append(x)
    return torch.stack(out, 0)
