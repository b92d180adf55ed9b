"""CPU restatement of the reference's D-VAE decoders in float64.

TEST INFRASTRUCTURE.  Only `tests/` may import this module; nothing under `dagnn_amd/` does.  It is the checker of
csrc/dvae_decode.hip (`loss()`) and csrc/dvae_sample.hip (`decode()` / `decode_dense()`), never the thing measured.

Parity status: **pinned**.  `tests/test_dvae_decoder_oracle_cpu.py` checks every function here against the 17 decoder
fixtures the unmodified reference wrote (`dvae_loss_*`, `dvae_gated_loss_*`, `dvae_decode_*`, `dvae_gated_decode_*`);
the GPU tests then trust it at the shapes no fixture reaches.

What is restated (plain torch on CPU, no custom kernels), with the reference lines each function follows:

* `decoder_loss`    - `DVAE_PYG.loss()` `dvae/models_pyg.py:398-456` with `_update_iv` (`:247-250`) calling
                      `_ipropagate_to` (`dvae/dagnn.py:187-239` NA, `dvae/dagnn_bn.py:179-238` BN), the attention of
                      `AttnConv.forward` with `edge_index=None` (`dagnn.py:360-369`), `GatedSumConv.forward`
                      (`dagnn.py:284-288`), the graph state of `_get_igraph_state` (`models_pyg.py:294-309` NA,
                      `:591-613` BN) and the edge head of `_get_edge_score` (`:333-336` NA, `:733-737` BN)
* `padding_widths`  - the padding width of every `_ipropagate_to` call of `loss()`, in call order
* `replay_decode`   - `DVAE_PYG.decode()` `models_pyg.py:338-396` along a given decoded result

Inputs are dense, as `dagnn_amd.dvae.decode_schedule` produces them: types [B, n] and predecessor bitmasks preds [B, n]
(bit u of preds[b, v]: the edge u -> v), H0 [B, hs] and a state dict (names of `DAGNN_NA` / `DAGNN_BN`).

NA attn_h at max_n != 8: the reference pads the attention VALUES with rows `vs - 8` wide (`dagnn.py:219-220`), which
is hs wide only when max_n == 8; at any other max_n its own decoder stops with a shape error.  Here the padding rows are
zero states of width hs at every max_n - the intended semantics, and the only definition the kernels can be checked
against there (no fixture can reach that case).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle.dagnn_oracle import gru_cell

Tensor = torch.Tensor
F64 = torch.float64


class _Sigmoid32(torch.autograd.Function):
    """The reference's float32 `torch.sigmoid` (returned in float64): 1 / (1 + exp(-s)) with every step rounded to
    float32 - so p is exactly 1 from s = 16.64 on (1 + exp(-s) rounds to 1), where the rounded exact sigmoid waits until 17.33 -
    and its derivative p (1 - p) taken at that float32 p."""

    @staticmethod
    def forward(ctx, s):
        p = (1.0 / (1.0 + torch.exp(-s).float())).double()
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, g):
        p, = ctx.saved_tensors
        return g * p * (1.0 - p)


def _bits(preds) -> Tensor:
    """[B, n] int32 (or int64) bitmasks -> [B, n, n] bool, [b, v, u] = edge u -> v."""
    m = torch.as_tensor(np.asarray(preds)).to(torch.int64) & 0xFFFFFFFF
    u = torch.arange(m.shape[1], dtype=torch.int64)
    return (m.unsqueeze(-1) >> u) & 1 == 1


def padding_widths(preds) -> List[int]:
    """P of every `_ipropagate_to` call of the teacher-forced decoder, in call order: vertex 0 (H0 given) 0, then per
    vertex v the fresh update (k = v) and one update per edge step vi = v-1 .. 0 (k = vi): the largest number of true
    predecessors u with k <= u < v over the batch."""
    bits = _bits(preds)
    n = bits.shape[1]
    out = [0]
    for v in range(1, n):
        for k in range(v, -1, -1):
            out.append(int(bits[:, v, k:v].sum(1).max()) if bits.shape[0] else 0)
    return out


class _Model(object):
    """The decoder's tensors out of a state dict, in float64 (a differentiable cast: leaves stay leaves' ancestors)."""

    def __init__(self, sd: Dict[str, Tensor], kind: str, agg: str, L: int, max_n: int):
        g = lambda k: sd[k].to(F64)  # noqa: E731
        self.bn, self.agg, self.L, self.n = kind == "bn", agg, L, max_n
        if kind not in ("na", "bn") or agg not in ("attn_h", "gated_sum") or (self.bn and agg != "attn_h"):
            raise NotImplementedError((kind, agg))
        self.hs = sd["fc3.weight"].shape[0]
        self.nvt = sd["add_vertex.2.weight"].shape[0]
        self.cells = [tuple(g("grud.%d.%s" % (l, w)) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                      for l in range(L)]
        self.av = [g("add_vertex.0.weight"), g("add_vertex.0.bias"), g("add_vertex.2.weight"), g("add_vertex.2.bias")]
        self.ae = [g("add_edge.0.weight"), g("add_edge.0.bias"), g("add_edge.2.weight"), g("add_edge.2.bias")]
        if agg == "attn_h":
            w = g("node_aggr_0.0.attn_lin.weight")[0]
            q = w.shape[0] - (self.hs if self.bn else self.hs + max_n)   # query half: emb_dim (= nvt) columns
            self.wq, self.wk = w[:q], w[q:q + self.hs]
            self.wid = None if self.bn else w[q + self.hs:]
            self.ab = g("node_aggr_0.0.attn_lin.bias")[0]
        else:
            self.gw, self.gb, self.mw = g("gate_forward.0.0.weight"), g("gate_forward.0.0.bias"), g("mapper_forward.0.0.weight")

    def onehot(self, t: Tensor) -> Tensor:
        return F.one_hot(t.long(), self.nvt).to(F64)

    def message(self, h: Tensor, u: int) -> Tensor:
        """gated_sum: sigmoid(Wg [h; e_u] + bg) * Wm [h; e_u] of vertex u's final layer-0 states h [B, hs]."""
        x = torch.cat([h, h.new_zeros(h.shape[0], self.n).index_fill_(1, torch.tensor([u]), 1.0)], 1)
        return torch.sigmoid(x @ self.gw.t() + self.gb) * (x @ self.mw.t())

    def aggregate(self, X: Tensor, sel: Tensor, P: int, h0s: List[Tensor], msgs: List[Tensor]) -> Tensor:
        """The hidden input of one `_ipropagate_to` call: X [R, nvt] the updated vertices' one-hot types, sel [R, v] bool
        their predecessors of this call, P the padding width of the call, h0s / msgs the final layer-0 states / gated
        messages of vertices 0..v-1 ([R, hs] each, row-aligned with X)."""
        R, v = sel.shape
        if P == 0:
            return X.new_zeros(R, self.hs)
        if self.agg == "gated_sum":   # padding rows: gate(0) * mapper(0) = 0 (the mapper has no bias)
            return sum(torch.where(sel[:, u:u + 1], msgs[u], msgs[u].new_zeros(())) for u in range(v))
        # attn_lin([query ; key]) of every real slot and of a zero padding row, then a soft-max over the real slots
        # plus (P - count) padding slots (a padding slot of multiplicity m enters as logit + log m)
        base = X @ self.wq + self.ab                                                # [R]
        keys = torch.stack(h0s, 1)                                                  # [R, v, hs]
        s = base.unsqueeze(1) + keys @ self.wk
        if self.wid is not None:
            s = s + self.wid[:v]
        cnt = sel.sum(1)
        pad = (P - cnt).to(F64)
        s = torch.where(sel, s, s.new_full((), float("-inf")))
        logpad = torch.where(pad > 0, base + torch.log(pad.clamp(min=1)), base.new_full((), float("-inf")))
        z = torch.cat([s, logpad.unsqueeze(1)], 1)
        alpha = torch.softmax(z, 1)[:, :v]
        return torch.einsum("rv,rvh->rh", alpha, keys)

    def stack(self, X: Tensor, H: Tensor) -> List[Tensor]:
        """The L stacked cells: layer 0 reads X, layer l > 0 the state below; every layer's hidden input is H."""
        out, x = [], X
        for c in self.cells:
            x = gru_cell(x, H, *c)
            out.append(x)
        return out

    def vertex_pre(self, Hg: Tensor) -> Tensor:
        return Hg @ self.av[0].t() + self.av[1]

    def vertex_logits(self, pre: Tensor) -> Tensor:
        return torch.relu(pre) @ self.av[2].t() + self.av[3]

    def edge_pre(self, Hvi: Tensor, Hv: Tensor, H0: Tensor) -> Tensor:
        x = torch.cat([Hvi, Hv, H0] if self.bn else [Hvi, Hv], -1)
        return x @ self.ae[0].t() + self.ae[1]

    def edge_logit(self, pre: Tensor) -> Tensor:
        return (torch.relu(pre) @ self.ae[2].t() + self.ae[3])[..., 0]


def _kinks(pre: Tensor, rel: float = 1e-5):
    a = pre.detach().abs()
    if a.numel() == 0:
        return 0, float("inf")
    return int((a <= rel * float(a.max())).sum()), float(a.min())


def decoder_loss(sd: Dict[str, Tensor], types, preds, H0: Tensor, *, kind: str = "na", agg: str = "attn_h", L: int = 2,
                 start_type: int = 0, diag: Optional[dict] = None):
    """`(res, vertex_ll [B], edge_ll [B])` of the teacher-forced decoder, differentiable in H0 and every decoder tensor
    of `sd` (pass float64 leaves to get their gradients).  res = -(sum vertex_ll + sum edge_ll).

    Float64 throughout with one deliberate exception: the reference's `F.binary_cross_entropy` sees a FLOAT32
    probability and clamps its logs at -100, so a logit beyond about +16.6 gives p = 1 exactly and a loss of 100 for a
    missing edge, and its backward, (p - y) / max(p (1 - p), 1e-12) times p (1 - p) at the float32 p, vanishes there.
    p is therefore the float32 sigmoid (`_Sigmoid32`), fed to a float64 BCE with the same clamp and backward rule - that
    is the reference's saturation behaviour, which dd_edge_head_kernel mirrors; in float64 those terms would differ by
    orders of magnitude.

    The quirks of the reference are kept: vertex 0 is START_TYPE whatever the true type, and H0 is the hidden input of
    each of its stacked layers; vertex v is updated v+1 times, update k reading v's true predecessors >= k; the hidden
    input of every layer is the aggregate of the FINAL layer-0 states of the predecessors; attn_h's soft-max also runs
    over P - count zero padding rows (P: the widest list of the batch in that call), with query and bias in every score.
    `diag` (a dict, optional) receives the ReLU pre-activations of add_vertex.0 / add_edge.0 within 1e-5 x max|.| of
    zero (`vertex_kinks`, `edge_kinks`: count, smallest |.|), the largest |edge logit| (`max_logit`) and the number of
    edge logits beyond +-30 (`saturated`)."""
    types = torch.as_tensor(np.asarray(types)).long()
    bits = _bits(preds)
    B, n = types.shape
    M = _Model(sd, kind, agg, L, n)
    H0 = H0.to(F64)
    h0s, tops, msgs = [], [], []      # final layer-0 / top states and gated messages of vertex 0..v-1, [B, hs]
    edge_rows = []                    # (v, vi, top state of the update that scores vi)
    for v in range(n):
        t = torch.full((B,), start_type, dtype=torch.long) if v == 0 else types[:, v]
        X = M.onehot(t)
        if v == 0:
            st = M.stack(X, H0)
        else:
            ks = list(range(v, -1, -1))   # call order: the fresh update, then edge steps vi = v-1 .. 0
            sel = torch.cat([bits[:, v, :v] & (torch.arange(v) >= k) for k in ks], 0)          # [(v+1) B, v]
            Ps = [int(bits[:, v, k:v].sum(1).max()) for k in ks]
            Xr = X.repeat(len(ks), 1)
            hagg = torch.cat([M.aggregate(Xr[i * B:(i + 1) * B], sel[i * B:(i + 1) * B], P,
                                          h0s, msgs) for i, P in enumerate(Ps)], 0)
            st = M.stack(Xr, hagg)
            for i, k in enumerate(ks[:-1]):
                edge_rows.append((v, k - 1, st[-1][i * B:(i + 1) * B]))
            st = [s[v * B:] for s in st]    # the final update (k = 0)
        h0s.append(st[0])
        tops.append(st[-1])
        if M.agg == "gated_sum":
            msgs.append(M.message(st[0], v))
    # vertex heads: graph state NA top of v-1, BN sum of the tops of 0..v-1
    Hg = torch.stack([sum(tops[:v]) if M.bn else tops[v - 1] for v in range(1, n)], 0)          # [n-1, B, hs]
    vpre = M.vertex_pre(Hg)
    vll = torch.log_softmax(M.vertex_logits(vpre), -1).gather(2, types[:, 1:].t().unsqueeze(-1))[..., 0].sum(0)
    # edge heads over every (v, vi)
    Hvi = torch.stack([tops[vi] for _, vi, _ in edge_rows], 0)
    Hv = torch.stack([h for _, _, h in edge_rows], 0)
    y = torch.stack([bits[:, v, vi] for v, vi, _ in edge_rows], 0).to(F64)
    epre = M.edge_pre(Hvi, Hv, H0.expand(len(edge_rows), B, M.hs))
    logit = M.edge_logit(epre)
    p = _Sigmoid32.apply(logit)
    ell = -F.binary_cross_entropy(p, y, reduction="none").sum(0)
    res = -(vll.sum() + ell.sum())
    if diag is not None:
        diag["vertex_kinks"] = _kinks(vpre)
        diag["edge_kinks"] = _kinks(epre)
        diag["max_logit"] = float(logit.detach().abs().max()) if logit.numel() else 0.0
        diag["saturated"] = int((logit.detach().abs() > 30).sum())
    return res, vll, ell


def decoder_loss_grads(sd: Dict[str, Tensor], types, preds, mu: Tensor, logvar: Tensor, *, beta: float = 0.005,
                       diag: Optional[dict] = None, **kw):
    """`loss()` in evaluation mode (z = mu) and its gradients in float64: returns (loss, res, kld, vertex_ll, edge_ll,
    {name: gradient}) for mu, logvar and every floating tensor of `sd` that takes part."""
    leaves = {k: v.detach().to(F64).clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    mu = mu.detach().to(F64).clone().requires_grad_(True)
    logvar = logvar.detach().to(F64).clone().requires_grad_(True)
    H0 = torch.tanh(mu @ leaves["fc3.weight"].t() + leaves["fc3.bias"])
    res, vll, ell = decoder_loss(leaves, types, preds, H0, diag=diag, **kw)
    kld = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
    loss = res + beta * kld
    names = list(leaves)
    gs = torch.autograd.grad(loss, [mu, logvar] + [leaves[k] for k in names], allow_unused=True)
    out = {"mu": gs[0], "logvar": gs[1]}
    out.update({k: g for k, g in zip(names, gs[2:]) if g is not None})
    return loss.detach(), res.detach(), kld.detach(), vll.detach(), ell.detach(), out


@torch.no_grad()
def replay_decode(sd: Dict[str, Tensor], H0: Tensor, types, preds, nv, *, kind: str = "na", agg: str = "attn_h",
                  L: int = 2, start_type: int = 0, end_type: int = 1, u_type=None, u_edge=None, tol: float = 0.0):
    """`decode()` of B rows along a given decoded result (types [B, n] with -1 past the end, preds [B, n] bitmasks,
    nv [B], which the caller compares with the returned nv), in the reference's call order.  u_type [n, B] /
    u_edge [n(n-1)/2, B] are the draws of a sampled decode (layout `dagnn_amd.dvae.draw_shapes` / `edge_draw_index`),
    None for argmax.

    At every decision the float64 probabilities and the decision they imply are recorded with its margin: a type draw
    picks the first type whose normalised cumulative probability exceeds u (margin: distance of u to the nearest inner
    CDF boundary); argmax types take the first largest logit (margin: top-two logit gap); a sampled edge is u < p
    (margin |u - p|), an argmax edge p > 0.5 (margin |p - 0.5|).  The decode then FOLLOWS the given result.  An END
    vertex connects every loose end (vertices without successors), finishes its row and is still updated by the
    remaining edge steps of that vertex; each update's padding width is taken over the rows still alive in that call
    (vcount > v).

    Returns a dict: type_p [n, B, nvt], type_dec / type_margin [n, B] (-1 / inf where the row takes no type decision),
    edge_p / edge_dec / edge_margin [n(n-1)/2, B] (likewise), the result the oracle implies - types, preds (int64
    bitmasks), nv - where a decision of margin <= tol takes the given value, the final top-layer states [B, n, hs]
    (zeros past the end) and the padding widths of every call."""
    types_g = np.asarray(types).astype(np.int64)
    preds_g = np.asarray(preds).astype(np.int64) & 0xFFFFFFFF
    B, n = types_g.shape
    M = _Model(sd, kind, agg, L, n)
    H0 = H0.detach().to(F64)
    stochastic = u_type is not None
    u_type = None if u_type is None else torch.as_tensor(np.asarray(u_type, dtype=np.float32)).to(F64)
    u_edge = None if u_edge is None else torch.as_tensor(np.asarray(u_edge, dtype=np.float32)).to(F64)
    NE = n * (n - 1) // 2
    out = dict(type_p=torch.zeros(n, B, M.nvt, dtype=F64), type_dec=np.full((n, B), -1, np.int64),
               type_margin=np.full((n, B), np.inf), edge_p=torch.zeros(NE, B, dtype=F64),
               edge_dec=np.full((NE, B), -1, np.int64), edge_margin=np.full((NE, B), np.inf), widths=[])
    itypes = np.full((B, n), -1, np.int64)
    ipreds = np.zeros((B, n), np.int64)
    itypes[:, 0] = start_type
    cur_t = np.full((B, n), -1, np.int64)      # the followed graph: types, predecessor masks, vertex counts
    cur_p = np.zeros((B, n), np.int64)
    vcount = np.ones(B, np.int64)
    cur_t[:, 0] = start_type
    layers = [[torch.zeros(B, M.hs, dtype=F64) for _ in range(n)] for _ in range(L)]   # [l][v] states [B, hs]
    msgs = [torch.zeros(B, M.hs, dtype=F64) for _ in range(n)]

    def update(v, H=None):
        alive = np.nonzero(vcount > v)[0]
        if len(alive) == 0:
            out["widths"].append(0)
            return
        rows = torch.from_numpy(alive)
        X = M.onehot(torch.from_numpy(cur_t[alive, v]))
        if H is None:
            m = torch.from_numpy(cur_p[alive, v])
            sel = (m.unsqueeze(1) >> torch.arange(v)) & 1 == 1
            P = int(sel.sum(1).max()) if v else 0
            out["widths"].append(P)
            H = M.aggregate(X, sel, P, [layers[0][u][rows] for u in range(v)], [msgs[u][rows] for u in range(v)])
        else:
            out["widths"].append(0)
            H = H[rows]
        for l, s in enumerate(M.stack(X, H)):
            layers[l][v][rows] = s
        if M.agg == "gated_sum":
            msgs[v][rows] = M.message(layers[0][v][rows], v)

    def top(v):
        return layers[L - 1][v] * torch.from_numpy(vcount > v).to(F64).unsqueeze(1)

    update(0, H0)
    finished = np.zeros(B, bool)
    for idx in range(1, n):
        live = ~finished
        if idx < n - 1:
            last = torch.from_numpy(vcount - 1)
            if M.bn:
                Hg = sum(top(u) for u in range(idx))
            else:
                Hg = torch.stack([layers[L - 1][u] for u in range(idx)], 0)[last, torch.arange(B)]
            logits = M.vertex_logits(M.vertex_pre(Hg))
            p = torch.softmax(logits, 1)
            out["type_p"][idx] = p
            if stochastic:
                cdf = p.cumsum(1)
                cdf = cdf / cdf[:, -1:]
                u = u_type[idx]
                dec = (cdf <= u.unsqueeze(1)).sum(1).clamp(max=M.nvt - 1).numpy()
                gap = (cdf[:, :-1] - u.unsqueeze(1)).abs().min(1).values.numpy() if M.nvt > 1 else np.full(B, np.inf)
            else:
                dec = logits.argmax(1).numpy()
                two = torch.topk(logits, 2, 1).values if M.nvt > 1 else None
                gap = (two[:, 0] - two[:, 1]).numpy() if M.nvt > 1 else np.full(B, np.inf)
            out["type_dec"][idx, live] = dec[live]
            out["type_margin"][idx, live] = gap[live]
            itypes[live, idx] = np.where(gap <= tol, types_g[:, idx], dec)[live]
        else:
            itypes[live, idx] = end_type
        cur_t[live, idx] = types_g[live, idx] if idx < n - 1 else end_type   # the decode follows the given result
        vcount[live] += 1
        update(idx)
        is_end = live & (cur_t[:, idx] == end_type)
        for vi in range(idx - 1, -1, -1):
            e = idx * (idx - 1) // 2 + (idx - 1 - vi)
            pre = M.edge_pre(top(vi), top(idx), H0)
            pe = torch.sigmoid(M.edge_logit(pre))
            out["edge_p"][e] = pe
            if stochastic:
                u = u_edge[e]
                dec, gap = (u < pe).numpy(), (u - pe).abs().numpy()
            else:
                dec, gap = (pe > 0.5).numpy(), (pe - 0.5).abs().numpy()
            take = live & ~finished & ~is_end
            out["edge_dec"][e, take] = dec[take]
            out["edge_margin"][e, take] = gap[take]
            given = (preds_g[:, idx] >> vi) & 1
            ibit = np.where(gap <= tol, given, dec.astype(np.int64))
            ipreds[take, idx] |= ibit[take] << vi
            cur_p[take, idx] |= given[take] << vi
            ends = is_end & ~finished
            if ends.any():   # END: every loose end (no successor yet, the new vertex excluded) joins it
                for b in np.nonzero(ends)[0]:
                    succ = int(np.bitwise_or.reduce(cur_p[b, :idx])) if idx else 0
                    loose = sum(1 << u for u in range(idx) if not succ >> u & 1)
                    cur_p[b, idx] = loose
                    ipreds[b, idx] = loose
                finished |= ends
            update(idx)
    out["types"], out["preds"] = itypes, ipreds
    inside = itypes >= 0
    out["nv"] = inside.sum(1)
    out["states"] = torch.stack([top(v) for v in range(n)], 1)
    return out
