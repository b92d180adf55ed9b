"""Per-edge attention weights of an evaluation pass: `DAGNN.attention(G)` (and the D-VAE encoders'), `attention_host`.

What a hook on the reference's conv modules would record (`AttnConv.message` / `SelfAttnConv.message` / `MultAttnConv.message`,
ogbg-code/model/dagnn.py:297-310, 366-373, 399-406; the D-VAE twins dvae/dagnn.py:109-145, dvae/dagnn_bn.py): for direction d
and stacked layer l, edge e with target t and source s (d = 0: t = edge_index[1, e], s = edge_index[0, e]; d = 1: swapped),

    score_e = attn_lin(cat[q_t, key_s + enc(ea_e)])                              attn_h, attn_x  (self_attn_*: no q)
    score_e = sum_k (W_l q_t + b_l)_k (W_r (key_s + enc(ea_e)) + b_r)_k          mattn_h
    alpha_e = exp(score_e - max_seg) / (sum_seg exp(score - max_seg) + 1e-16)    PyG's softmax over the in-edges of t

with key = the states h[d][l] (`*_h`; NA: [state ; one-hot vertex id]) or the node inputs x (`*_x`), q = x for l = 0 and for
the `*_x` kinds, else h[d][l-1] (NA: with the vertex-id columns).  Every state is written exactly once by the recurrence, so
the final states of a pass are the states its aggregations saw: the weights are computed AFTER the pass from the states, the
plan's CSR (`eidx_d`: the original edge id of every slot) and the parameters - `dagnn_attention_weights`, csrc/attention.hip:
two launches for all cells (mattn_h: two projection GEMMs per cell and one launch).

`attention_host` is the same definition in torch ops on any device and precision (it gathers [E, H] rows: the yardstick of
the tests, not a path of the model).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import torch

from . import constants as K
from . import engine

__all__ = ["Attention", "attention_host", "attention_cells", "forward_with_states", "weights_of", "run"]

_ADDITIVE = (K.NA_ATTN_H, K.NA_ATTN_X, K.NA_SELF_ATTN_H, K.NA_SELF_ATTN_X)


class Attention(NamedTuple):
    """What `model.attention(G)` returns.  `out`: what `forward(G)` returns, from the same pass; `alpha` [D, L, E] fp32: the
    weight the aggregation of direction d (index into `model.dirs`), stacked layer l gave edge e (column of `G.edge_index`);
    `logit` [D, L, E]: the pre-softmax scores, or None.  `h`: the pass's states h[d][l] [N, hidden] (views of the kernels' row
    buffers), the rows `alpha` weighs - the D-VAE encoders keep only the read-out rows on `G`.  The row buffers are tensors the
    pass allocated for itself (not arena scratch): they stay valid as long as this record holds them, but they are views
    ([:, :hidden] of wider rows) - `.clone()` what must outlive the record or be changed."""
    out: object
    alpha: torch.Tensor
    logit: Optional[torch.Tensor]
    h: Optional[list] = None


def _is_dvae(model) -> bool:
    return hasattr(model, "grue_forward")


def check_supported(model) -> None:
    """`agg_x=True`: NotImplementedError; an aggregator without attention: ValueError."""
    if getattr(model, "agg_x", False):
        raise NotImplementedError("attention(): agg_x=True (the aggregator runs on the inputs once per direction, not per stacked "
                                  "layer: there is no [D, L, E] weight tensor for it)")
    if model.agg not in _ADDITIVE and model.agg != "mattn_h":
        raise ValueError("attention(): agg=%r has no attention weights (attn_h, attn_x, self_attn_h, self_attn_x, mattn_h do)" % (model.agg,))
    if _is_dvae(model) and model.agg == "mattn_h":
        raise ValueError("attention(): the D-VAE encoders have no mattn_h")


def attention_cells(model) -> List[dict]:
    """The terms of the definition per (direction, stacked layer), in `alpha`'s order, as views of the PARAMETERS: `d`, `l`,
    `key_src` / `query_src` ('h' = h[d][l], 'below' = h[d][l-1], 'x', None), `w_key`, `w_query`, `vid_key`, `vid_query` (NA: the
    weights of the one-hot vertex-id columns), `edge_w` / `edge_b` (edge encoder or None), `bias` (attn_lin.bias);
    mattn_h: `wl`, `bl`, `wr`, `br` instead of the vectors."""
    check_supported(model)
    H, E = model.hidden_dim, model.emb_dim
    self_attn = "self_attn" in model.agg
    keys_x = "_x" in model.agg
    nn_ = int(model._vid_nodes) if _is_dvae(model) else 0
    out = []
    for d in model.dirs:
        for l in range(model.num_layers):
            a = getattr(model, "node_aggr_%d" % d)[l]
            c = dict(d=d, l=l, key_src="x" if keys_x else "h",
                     query_src=None if self_attn else ("x" if (l == 0 or keys_x) else "below"),
                     edge_w=a.edge_encoder.weight if getattr(a, "wea", False) else None,
                     edge_b=a.edge_encoder.bias if getattr(a, "wea", False) else None,
                     vid_key=None, vid_query=None, w_query=None)
            if model.agg == "mattn_h":
                c.update(wl=a.attn_linl.weight, bl=a.attn_linl.bias, wr=a.attn_linr.weight, br=a.attn_linr.bias)
                out.append(c)
                continue
            w = a.attn_lin.weight[0]
            kd = E if keys_x else H
            qd = 0 if self_attn else (E if (l == 0 or keys_x) else H)
            q_vid = nn_ if (c["query_src"] == "below") else 0          # (NA: the query of l > 0 is [h[d][l-1] ; vertex id])
            dq = 0 if self_attn else qd + q_vid
            if qd:
                c["w_query"] = w[:qd]
                if q_vid:
                    c["vid_query"] = w[qd:qd + q_vid]
            c["w_key"] = w[dq:dq + kd]
            if nn_ and not keys_x:
                c["vid_key"] = w[dq + kd:dq + kd + nn_]
            assert dq + kd + (nn_ if (nn_ and not keys_x) else 0) == w.shape[0], (model.agg, d, l, tuple(w.shape))
            c["bias"] = a.attn_lin.bias
            out.append(c)
    return out


def attention_host(model, G, h, x=None, dtype=torch.float64, logits: bool = True):
    """The definition in torch ops: (alpha [D, L, E], logit [D, L, E] or None) in `dtype` on the device of `G.edge_index`, from
    the states `h[d][l]` ([N, >= hidden] each) and the node inputs `x` (default `G.x`: what the pass left there - the
    embedding for `DAGNN`, the one-hot types for the D-VAE encoders) of a pass of `model` on `G`."""
    ei = G.edge_index
    dev = ei.device
    Ecount = int(ei.shape[1])
    cells = attention_cells(model)
    D, L, H = len(model.dirs), model.num_layers, model.hidden_dim
    x = (G.x if x is None else x).to(dev, dtype)
    N = x.shape[0]
    nn_ = int(model._vid_nodes) if _is_dvae(model) else 0
    alpha = torch.zeros(D, L, Ecount, dtype=dtype, device=dev)
    logit = torch.zeros(D, L, Ecount, dtype=dtype, device=dev)
    if Ecount == 0:
        return alpha, (logit if logits else None)
    P = lambda t: None if t is None else t.detach().to(dev, dtype)  # noqa: E731
    ea = None
    if cells[0]["edge_w"] is not None:
        ea = G.edge_attr.to(dev, torch.float32).view(Ecount, -1).to(dtype)   # (the plan carries fp32 features)
    vid = torch.arange(N, device=dev) % nn_ if nn_ else None
    for c in cells:
        d, l = c["d"], c["l"]
        q = model.dirs.index(d)
        tgt, src = (ei[1], ei[0]) if d == 0 else (ei[0], ei[1])
        rows = lambda name: x if name == "x" else h[d][l if name == "h" else l - 1][:, :H].to(dev, dtype)  # noqa: E731
        key = rows(c["key_src"])[src]
        if ea is not None:
            key = key + ea @ P(c["edge_w"]).t() + P(c["edge_b"])
        if "wl" in c:
            qq = rows(c["query_src"])[tgt] @ P(c["wl"]).t() + P(c["bl"])
            score = (qq * (key @ P(c["wr"]).t() + P(c["br"]))).sum(1)
        else:
            score = key @ P(c["w_key"]) + P(c["bias"])
            if c["vid_key"] is not None:
                score = score + P(c["vid_key"])[vid[src]]
            if c["query_src"] is not None:
                score = score + rows(c["query_src"])[tgt] @ P(c["w_query"])
                if c["vid_query"] is not None:
                    score = score + P(c["vid_query"])[vid[tgt]]
        m = torch.full((N,), float("-inf"), dtype=dtype, device=dev).scatter_reduce(0, tgt, score, "amax", include_self=True)
        ex = torch.exp(score - m[tgt])
        s = torch.zeros(N, dtype=dtype, device=dev).index_add_(0, tgt, ex)
        alpha[q, l] = ex / (s[tgt] + 1e-16)
        logit[q, l] = score
    return alpha, (logit if logits else None)


def _derived(model):
    """Kernel-ready terms of every cell, cached per parameter version like the pass's own derived weights (evaluation only)."""
    cells = attention_cells(model)
    srcs = [t for c in cells for t in c.values() if isinstance(t, torch.Tensor)]
    srcs = [t._base if t._base is not None else t for t in srcs]

    def make():
        out = []
        for c in cells:
            k = dict(dir=c["d"])
            We, be = c["edge_w"], c["edge_b"]
            f = lambda t: None if t is None else t.detach().float().contiguous()  # noqa: E731
            if "wl" in c:
                k.update(wl=f(c["wl"]), bl=f(c["bl"]), wr=f(c["wr"]), br=f(c["br"]))
                if We is not None:
                    k["edge_gain"] = (k["wr"] @ We.detach().float()).contiguous()     # [q_dim, R]
                    k["edge_vec"] = (k["wr"] @ be.detach().float()).contiguous()
            else:
                k.update(w_key=f(c["w_key"]), w_query=f(c["w_query"]), vid_key=f(c["vid_key"]), vid_query=f(c["vid_query"]))
                bias = c["bias"].detach().float().reshape(1)
                if We is not None:
                    k["edge_gain"] = (We.detach().float().t() @ k["w_key"]).contiguous()   # [R]: as `core.derive_cell` folds it
                    bias = bias + (be.detach().float() @ k["w_key"]).reshape(1)
                k["bias"] = bias.contiguous()
            out.append(k)
        return out

    return cells, model._cache("attention").get(srcs, make, fresh=model.training)


def weights_of(model, plan, x: torch.Tensor, h, E: int, logits: bool):
    """(alpha [D, L, E], logit or None) of a finished pass: its plan, node inputs `x` [N, emb] and states h[d][l]."""
    D, L = len(model.dirs), model.num_layers
    cells, derived = _derived(model)
    mult = model.agg == "mattn_h"
    if E == 0 or x.shape[0] == 0:
        z = torch.zeros(D, L, E, dtype=torch.float32, device=x.device)
        return z, (z.clone() if logits else None)
    rows = lambda c, name: x if name == "x" else h[c["d"]][c["l"] if name == "h" else c["l"] - 1]  # noqa: E731
    jobs = []
    for c, k in zip(cells, derived):
        job = dict(k)
        if mult:
            pq = engine.gemm_nt_bias([rows(c, c["query_src"])], [k["wl"]], [k["bl"]])[0]
            pk = engine.gemm_nt_bias([rows(c, c["key_src"])], [k["wr"]], [k["br"]])[0]
            job.update(key=pk, key_dim=pk.shape[1], query=pq, query_dim=pq.shape[1])
        else:
            key = rows(c, c["key_src"])
            job.update(key=key, key_dim=k["w_key"].numel())
            if c["query_src"] is not None:
                job.update(query=rows(c, c["query_src"]), query_dim=k["w_query"].numel())
        jobs.append(job)
    nn_ = int(model._vid_nodes) if _is_dvae(model) else 0
    cap = engine._lib.ATTN_MAX_CELLS   # (cells per call of the entry point: more than 16 go in chunks, two launches each)
    parts = [engine.attention_weights(plan, jobs[o:o + cap], E, mode=1 if mult else 0, vid_mod=nn_, logits=logits)
             for o in range(0, len(jobs), cap)]
    alpha, logit = parts[0] if len(parts) == 1 else (torch.cat([p[0] for p in parts]),
                                                     torch.cat([p[1] for p in parts]) if logits else None)
    return alpha.view(D, L, E), (None if logit is None else logit.view(D, L, E))


def forward_with_states(model, G):
    """(`model.forward(G)`, {'plan', 'x', 'h', 'E'}): one pass that also hands out its plan, node inputs and states h[d][l].  The
    pass finds the dict under `model.__dict__['_attn_capture']` (`DAGNN._finish`, `_DvaeDagnn._forward`) - the one place that
    key is set; like the rest of a module's pass state (arenas, caches) it is per model, not for two threads on one model."""
    if "_attn_capture" in model.__dict__:
        raise RuntimeError("attention(): a pass of this model is already collecting its states (one model, two threads?)")
    cap = model.__dict__["_attn_capture"] = {}
    try:
        out = model.forward(G)
    finally:
        model.__dict__.pop("_attn_capture", None)
    if cap.get("plan") is None:
        raise engine.DagnnHipError("attention(): the pass ran without a plan (variant_backend = 'torch'): no HIP states to weigh")
    return out, cap


def run(model, G, logits: bool = False) -> Attention:
    """`model.attention(G, logits)`: one evaluation pass (`forward`'s side effects on `G`), then the weights of its cells."""
    if model.training:
        raise RuntimeError("%s.attention is an evaluation pass: call model.eval() first" % type(model).__name__)
    check_supported(model)
    with torch.no_grad():
        out, cap = forward_with_states(model, G)
        h = cap["h"]
        alpha, logit = weights_of(model, cap["plan"], cap["x"], h, int(cap["E"]), bool(logits))
    return Attention(out, alpha, logit, [[h[d][l] for l in range(model.num_layers)] for d in model.dirs])
