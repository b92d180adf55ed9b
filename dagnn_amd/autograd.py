"""Training path: `torch.autograd.Function`s around the HIP kernels.

The reference trains through torch autograd over its Python loops (`loss.backward()`,
ogbg-code/main_pyg.py:62): one autograd node per (direction, topological layer, stacked layer)
micro-step.  Here the forward pass is the same HIP path as inference and keeps only the states
h[d][i]; `Recurrence.backward` recomputes aggregates / pre-activations in parallel, walks the dependent
chain once in reverse lock-step (csrc/backward.hip) and finishes with library GEMMs for the weight
gradients.  Everything around it (dropout, the vocabulary heads, the loss, the optimizer) stays
ordinary torch autograd, as in the reference.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib, engine
from .core import run_stack_lockstep


class EncodeAST(torch.autograd.Function):
    """`ASTNodeEncoder.forward` (ogbg-code/utils.py:26-28) on the HIP kernel; backward = the three
    embedding-table gradients (row sums of the incoming gradient by index).  `depth_w` None: `ASTNodeEncoder2`
    (ogbg-code/utils2.py:26-28), two tables and two gradients."""

    @staticmethod
    def forward(ctx, x, depth, type_w, attr_w, depth_w, max_depth):
        out = engine.encode_ast(x, depth, type_w, attr_w, depth_w, max_depth)  # clamps `depth` in place
        if depth_w is None:
            ctx.save_for_backward(x)
            ctx.rows = (type_w.shape[0], attr_w.shape[0])
        else:
            ctx.save_for_backward(x, depth.clone())
            ctx.rows = (type_w.shape[0], attr_w.shape[0], depth_w.shape[0])
        return out

    @staticmethod
    def backward(ctx, g):
        x = ctx.saved_tensors[0]
        if engine.TABLE_GRADS:   # one fixed summation order (`table_grads_host` below), all tables in one call
            grads = engine.table_grads(g, (x[:, 0], x[:, 1]) + tuple(ctx.saved_tensors[1:]), ctx.rows)
            return (None, None, grads[0], grads[1], grads[2] if len(grads) > 2 else None, None)
        g = g.contiguous()
        grads = []
        for rows, idx in zip(ctx.rows, (x[:, 0], x[:, 1]) + tuple(ctx.saved_tensors[1:])):
            grads.append(torch.zeros(rows, g.shape[1], dtype=g.dtype, device=g.device).index_add_(0, idx, g))
        return (None, None, grads[0], grads[1], grads[2] if len(grads) > 2 else None, None)


TABLE_GRADS_CHUNK = _lib.TABLE_GRADS_CHUNK   # DAGNN_TABLE_GRADS_CHUNK: members per chunk of a row's list


def table_grads_host(g, keys, rows):
    """Host mirror of `engine.table_grads` (`dagnn_table_grads`) in numpy fp32: the same bits, and the definition of the order.

    For table t and row r, list the nodes v with keys[t][v] == r in ascending v and cut the list into chunks of
    TABLE_GRADS_CHUNK consecutive members by position in the list (the last chunk may be short).  A chunk's partial is
    ((g[v0] + g[v1]) + g[v2]) + ..., left to right from its first member; out[r] = ((+0.0 + p0) + p1) + ..., left to right
    over the row's chunks; a row without members is +0.0.  Keys outside [0, rows[t]) contribute nothing.  Every add is
    one IEEE fp32 add (numpy adds whole arrays of independent sums at a time: step j adds the j-th member of every chunk).

    g [N, H] (tensor or array), keys: integer tensors / arrays of N entries (strided views allowed), rows: row counts.
    Returns a list of float32 arrays [rows[t], H]."""
    import numpy as np
    as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)   # noqa: E731
    g = np.ascontiguousarray(as_np(g), dtype=np.float32)
    C = TABLE_GRADS_CHUNK
    outs = []
    for k, R in zip(keys, rows):
        k, R = as_np(k).astype(np.int64).reshape(-1), int(R)
        assert k.shape[0] == g.shape[0], (k.shape, g.shape)
        v = np.nonzero((k >= 0) & (k < R))[0]
        members = v[np.argsort(k[v], kind="stable")]          # grouped by key, ascending v inside a group
        row = k[members]
        count = np.bincount(row, minlength=R)
        off = np.concatenate([[0], np.cumsum(count)])
        pos = np.arange(members.shape[0]) - off[row]          # position inside the row's list
        chunks = (count + C - 1) // C
        coff = np.concatenate([[0], np.cumsum(chunks)])
        chunk = coff[row] + pos // C                          # chunk of each member; pos % C is its place in the chunk
        partial = np.zeros((int(coff[-1]), g.shape[1]), dtype=np.float32)
        for j in range(C):
            sel = pos % C == j
            if not sel.any():
                break
            partial[chunk[sel]] = g[members[sel]] if j == 0 else partial[chunk[sel]] + g[members[sel]]
        out = np.zeros((R, g.shape[1]), dtype=np.float32)     # +0.0
        chunk_row = np.repeat(np.arange(R), chunks)
        chunk_at = np.arange(chunk_row.shape[0]) - coff[chunk_row]
        for c in range(int(chunks.max()) if R > 0 else 0):
            sel = chunk_at == c
            out[chunk_row[sel]] = out[chunk_row[sel]] + partial[sel]
        outs.append(out)
    return outs


def _wgrad(dg: torch.Tensor, u: torch.Tensor, splits: int = 32) -> torch.Tensor:
    """dg^T @ u for [N, J] x [N, K] with N >> J, K (a weight gradient): the reduction dimension is the long one,
    so it is split into `splits` batches (one library bmm fills the GPU; a plain GEMM here has J*K/128^2 = 12
    output tiles for 256 CUs) and the partial products are summed in a fixed order."""
    N = dg.shape[0]
    n = N // splits * splits
    if n == 0:
        return dg.t() @ u
    out = torch.bmm(dg[:n].view(splits, n // splits, dg.shape[1]).transpose(1, 2),
                    u[:n].reshape(splits, n // splits, u.shape[1])).sum(0)
    if n < N:
        out = out + dg[n:].t() @ u[n:]
    return out


class PoolNodes(torch.autograd.Function):
    """`(plan, h [N, W], scope, how) -> [B, W]`: max / add / mean pool of the rows of an ordinary autograd tensor over the
    output nodes of direction 0 / 1 (scope 0 / 1) or over all nodes of every graph (scope 2) - `global_{max,add,mean}_pool`
    of dagnn.py:194-202 and dvae/dagnn.py:163-172 - in HIP, forward (`dagnn_readout_pool_batch`) and backward
    (`dagnn_readout_pool_backward_batch` into a zero-filled [N, W]): no mask index, no scatter, no atomics.  The mean
    divides by the number of nodes in scope.  `h` may be a row-pitched view (`engine._rows`); once differentiable.  The
    recurrence states of a `Recurrence` pass do not come here: their read-out seeds the reverse sweep directly."""

    @staticmethod
    def forward(ctx, plan, h, scope, how):
        h = engine._rows(h, "pooled rows")
        out = torch.empty(plan.B, h.shape[1], dtype=torch.float32, device=h.device)   # (every element is written)
        if h.shape[1] > 0:
            engine.readout_pool_batch(plan, [(h, scope, how, 0)], out)
        ctx.plan, ctx.scope, ctx.how, ctx.shape = plan, int(scope), how, tuple(h.shape)
        ctx.save_for_backward(*([h] if how == "max" else []))   # (only the arg-max needs the values again)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[1]:
            return None, None, None, None
        gh = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        if ctx.shape[1] > 0:
            h = ctx.saved_tensors[0] if ctx.how == "max" else None
            engine.readout_pool_backward_batch(ctx.plan, [(h, ctx.scope, ctx.how, 0, gh)], g.contiguous().float())
        return None, gh, None, None


def seed_state_grads(gouts, dirs, L: int, N: int, H: int, Hp: int, device):
    """g_ext[d][i] [N, Hp], the gradients reaching the states h[d][i] from outside: views of ONE zero fill, the first H columns
    copied from `gouts` (one per (d, i); None: nobody differentiates that state; no `gouts`: the caller's read-out adds them)."""
    g_all = torch.zeros(len(dirs) * L, N, Hp, dtype=torch.float32, device=device)
    g_ext = [[g_all[dirs.index(d) * L + i] if d in dirs else None for i in range(L)] for d in range(2)]
    for q, go in enumerate(gouts or ()):
        if go is not None:
            g_ext[dirs[q // L]][q % L][:, :H] = go
    return g_ext


def unflatten_params(mod, params):
    """Flat parameters in `variants._cell_params` order -> (names [(d, i, name)], cellp {(d, i): {name: tensor}})."""
    from .variants import _cell_params
    it, names, cellp = iter(params), [], {}
    for d in mod.dirs:
        for i in range(mod.num_layers):
            cellp[(d, i)] = {n: next(it) for n, _ in _cell_params(mod, d, i)}
            names += [(d, i, n) for n in cellp[(d, i)]]
    return names, cellp


def wgrad_jobs(res, inp, dirs, L: int, H: int):
    """Jobs of `engine.wgrad` for the GRU cells in (d, i) order: (dgi, the cell's input `inp(d, i)`), then (dgh, the aggregate)."""
    jobs = []
    for d in dirs:
        for i in range(L):
            r = res[(d, i)]
            jobs += [(r["dgi"], inp(d, i), True), (r["dgh"], r["a"][:, :H], True)]
    return jobs


def gru_grads(jobs, like, N: int, Hp: int, H: int):
    """(g_wih, g_bih, g_whh, g_bhh) per cell of `wgrad_jobs`; an empty batch: zeros like `like`, (w_ih, b_ih, w_hh, b_hh) per cell."""
    if N == 0 or not jobs:
        return [tuple(torch.zeros_like(t) for t in cell) for cell in like]
    wg = engine.wgrad(jobs, N, Hp, H)
    return [wg[k] + wg[k + 1] for k in range(0, len(wg), 2)]


def add_input_grad(dx, dgi, w_ih, H: int, Hp: int) -> None:
    """dx += dgi ([N, 3Hp] in gate blocks of Hp -> [N, 3H]) @ w_ih, in place (dx is the caller's own buffer: no add kernel)."""
    N = dgi.shape[0]
    dx.addmm_(dgi if Hp == H else dgi.view(N, 3, Hp)[:, :, :H].reshape(N, 3 * H), w_ih)


class Recurrence(torch.autograd.Function):
    """Plan + node inputs -> graph read-out, differentiable (dagnn.py:144-193; dvae/dagnn.py:99-175).

    `mod` is the calling module, a `core.HipModule` (its docstring lists the hooks this reads).
    Inputs after `x` are the cells' parameters (`mod._train_params()`), 8 per (direction, stacked layer): weight_ih,
    weight_hh, bias_ih, bias_hh, attn_lin.weight, attn_lin.bias, edge_encoder.weight, edge_encoder.bias (the last two
    None without edge features)."""

    PER_CELL = 8

    @staticmethod
    def forward(ctx, mod, plan, B, fused, x, *params):
        """fused: returns (read-out [B, .], states...) with the read-out done by the module's HIP hooks and the states
        not differentiable; otherwise returns the states h[d][i] ([N, H] each, d over `dirs`, i over layers) as
        differentiable outputs - what follows is ordinary autograd (the D-VAE encoders' all-node read-out projects every node
        first, dvae/dagnn.py:163-172, and pools the projection through `PoolNodes`)."""
        L, H, dirs = mod.num_layers, mod.hidden_dim, mod.dirs
        ctx.set_materialize_grads(False)   # (outputs nobody differentiates arrive as None in backward, not as [N, H] zero fills)
        cells = mod._cells(fresh=True)   # a differentiable pass: the optimizer changes the parameters every step
        rec = engine.PassRecord()
        sscore = mod._static_scores(x, cells)   # keys from the inputs (`*_x` aggregators): one score per node and cell
        h = run_stack_lockstep(plan, x, cells, dirs, L, H, vid_nodes=mod._vid_nodes, arena=mod._arena_for(x), record=rec,
                               static_score=sscore, route=plan.route)
        ctx.mod, ctx.plan, ctx.cells, ctx.rec, ctx.h, ctx.fused = mod, plan, cells, rec, h, bool(fused)
        ctx.sscore = sscore
        ctx.save_for_backward(x, *[p for p in params if p is not None])
        ctx.present = [p is not None for p in params]
        flat = [h[d][i] for d in dirs for i in range(L)]
        if not fused:
            return tuple(flat)
        out = mod._readout(plan, B, x, h)
        ctx.mark_non_differentiable(*flat)
        return (out,) + tuple(flat)

    @staticmethod
    def backward(ctx, *gouts):
        mod, plan, cells, rec, h = ctx.mod, ctx.plan, ctx.cells, ctx.rec, ctx.h
        saved = list(ctx.saved_tensors)
        x, it = saved[0], iter(saved[1:])
        params = [next(it) if present else None for present in ctx.present]
        L, H, dirs, Hp = mod.num_layers, mod.hidden_dim, mod.dirs, rec.Hp
        N = x.shape[0]
        # (not fused: the gradients of the states themselves, from whatever autograd ops followed)
        g_ext = seed_state_grads(None if ctx.fused else gouts, dirs, L, N, H, Hp, x.device)
        dx = torch.zeros_like(x)
        if ctx.fused and gouts[0] is not None:
            mod._readout_backward(plan, x, h, gouts[0].contiguous().float(), g_ext, dx)
        kw = dict(arena=mod._arena_for(x, "backward"), vid_mod=mod._vid_nodes, static_score=ctx.sscore)
        # (decided with the forward's path: it runs on the forward's schedule; `held`: what its launch reads, alive until this returns)
        if rec.route.reverse == "dataflow":
            res, held = engine.bwd_dataflow_sweep(plan, dirs, L, Hp, cells, rec.h_buf, rec.gi0, g_ext, rec.route.groups, record=rec, **kw)
        else:
            res = engine.backward_sweep(plan, dirs, L, Hp, cells, rec.h_buf, rec.gi0, g_ext, **kw)
        with engine._span("backward_epilogue", x):
            # weight / bias gradients of every cell: ONE batch of split transposed products in HIP (csrc/wgrad.hip)
            P, order = Recurrence.PER_CELL, [(d, i) for d in dirs for i in range(L)]
            wg = gru_grads(wgrad_jobs(res, lambda d, i: x if i == 0 else h[d][i - 1], dirs, L, H),
                           [[params[k + q] for q in (0, 2, 1, 3)] for k in range(0, len(params), P)], N, Hp, H)
            # the small reductions of the attention / edge-encoder gradients, all cells in one batch (csrc/wgrad.hip):
            # sum_v sigma_v keys_v, sum_v (edge-feature sums)_v, sum_v sigma_v
            cs_jobs, cs_at = [], {}
            for d, i in (order if N > 0 else ()):
                r = res[(d, i)]
                keys = x if ctx.sscore is not None else h[d][i]
                cs_at[(d, i)] = len(cs_jobs)
                cs_jobs.append((keys, r["sigma"]))
                if r["edge_feat_grad"] is not None:
                    cs_jobs += [(r["edge_feat_grad"], None), (r["sigma"], None)]
            cs = engine.colsums(cs_jobs, N) if cs_jobs else None
            # gradients of attn_lin.weight and of the edge encoder, every cell in ONE launch (csrc/wgrad.hip).  The attention logit is
            # s_e = w_key . (h_p + W_e feat_e + b_e) [+ w_vid[p mod n]] (+ query and bias terms that cancel in the segment
            # softmax: their gradients are exact zeros)
            ag = None
            if cs is not None:
                ag_jobs = []
                for k, (d, i) in enumerate(order):
                    w_ih, w_hh, b_ih, b_hh, attn_w, attn_b, edge_w, edge_b = params[k * P:(k + 1) * P]
                    at = cs_at[(d, i)]
                    has_e = edge_w is not None and res[(d, i)]["edge_feat_grad"] is not None
                    ag_jobs.append({"key_sum": cs[at], "feat_sum": cs[at + 1] if has_e else None,
                                    "sigma_sum": cs[at + 2] if has_e else None, "edge_w": edge_w if has_e else None, "edge_b": edge_b,
                                    "attn_w": attn_w, "dq": mod._key_offset(i)})
                ag = engine.attn_grads(ag_jobs)
            grads = []
            for ci, (d, i) in enumerate(order):
                w_ih, w_hh, b_ih, b_hh, attn_w, attn_b, edge_w, edge_b = params[ci * P:(ci + 1) * P]
                r = res[(d, i)]
                g_wih, g_bih, g_whh, g_bhh = wg[ci]
                if i == 0 and x.requires_grad:
                    add_input_grad(dx, r["dgi"], w_ih, H, Hp)
                dq = mod._key_offset(i)
                sigma = r["sigma"]
                kd = attn_w.shape[1] - dq - mod._vid_nodes     # key width: H, or the input width for the `*_x` aggregators
                if ctx.sscore is not None and x.requires_grad:   # the score of node v is w_key . x_v
                    dx = dx + sigma[:, None] * attn_w[0, dq:dq + kd][None, :]
                if ag is not None:
                    g_attn, g_edge_w, g_edge_b = ag[ci]
                    if edge_w is not None and g_edge_w is None:
                        g_edge_w, g_edge_b = torch.zeros_like(edge_w), torch.zeros_like(edge_b)
                else:   # an empty batch
                    g_attn = torch.zeros_like(attn_w)
                    g_edge_w = None if edge_w is None else torch.zeros_like(edge_w)
                    g_edge_b = None if edge_w is None else torch.zeros_like(edge_b)
                if mod._vid_nodes:   # node v carries the one-hot of (v mod n): d w_vid[j] = sum of sigma over those nodes
                    g_attn[0, dq + kd:dq + kd + mod._vid_nodes] = sigma.view(-1, mod._vid_nodes).sum(0)
                grads += [g_wih, g_whh, g_bih, g_bhh, g_attn, None if attn_b is None else torch.zeros_like(attn_b),
                          g_edge_w, g_edge_b]
        return (None, None, None, None, dx if x.requires_grad else None) + tuple(grads)
