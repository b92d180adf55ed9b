"""`DAGNN` - drop-in for the reference's `ogbg-code/model/dagnn.py:16-215` on MI355X.

Same constructor signature, same `state_dict` keys and shapes (checkpoints written by the
reference's `utils2.create_checkpoint` load unchanged), same `forward(G)` contract on a PyG-style
batch including its side effects on `G` (`G.bi_layer_index`, `G.x` replaced by the embedding,
`G.node_depth` clamped, `G.h`).  The layer-by-layer gather -> attention-aggregate -> GRU path
runs in hand-written HIP (libdagnn_hip.so); there is no CPU or eager-PyTorch fallback for it.

Aggregators: the additive-attention family (`attn_h` - every BASELINE config - `attn_x`, `self_attn_h`,
`self_attn_x`) runs in HIP, forward and backward.  The reference's other constructor strings (`mattn_h`,
`gated_sum`, `add`, `max`, `agg_x=True`, `recurr=0`; SURVEY.md §8(a) row a12: exercised by no BASELINE
configuration) keep the same contract on the generic HIP kernels of `csrc/variants.hip` (forward) and
`csrc/variants_bwd.hip` (the reverse sweep of a training step), marshalled by `dagnn_amd/variants.py`; only what those
kernels do not take (more than 8 cells, an input width that is no multiple of 4 - or a hidden width with `mattn_h` / additive
attention -, more than two edge features behind an edge encoder) trains on torch-ROCm ops, and says so once (`variants.warn_torch_path`).
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import constants as K
from . import engine, route
from .core import HipModule, built_marker, default_schedule, derive_cell, meet_built, num_graphs_of, pack_lockstep, run_stack


class ASTNodeEncoder(nn.Module):
    """Node embedding of `ogbg-code/utils.py:6-28` (same parameter names)."""

    def __init__(self, emb_dim, num_nodetypes, num_nodeattributes, max_depth):
        super().__init__()
        self.max_depth = max_depth
        self.type_encoder = nn.Embedding(num_nodetypes, emb_dim)
        self.attribute_encoder = nn.Embedding(num_nodeattributes, emb_dim)
        self.depth_encoder = nn.Embedding(self.max_depth + 1, emb_dim)

    def forward(self, x, depth):
        if x.is_cuda and self.type_encoder.weight.shape[1] % 4 == 0 and depth.dtype == torch.int64 \
                and depth.is_contiguous():
            tables = (self.type_encoder.weight, self.attribute_encoder.weight, self.depth_encoder.weight)
            if torch.is_grad_enabled() and any(t.requires_grad for t in tables):
                from .autograd import EncodeAST
                return EncodeAST.apply(x, depth, *tables, self.max_depth)
            return engine.encode_ast(x, depth, *tables, self.max_depth)
        # generic torch path (odd widths): same math as utils.py:26-28
        depth[depth > self.max_depth] = self.max_depth
        return self.type_encoder(x[:, 0]) + self.attribute_encoder(x[:, 1]) + self.depth_encoder(depth)


class ASTNodeEncoder2(nn.Module):
    """Node embedding of the LP task, `ogbg-code/utils2.py:6-28` (same parameter names): type + attribute and NO depth table
    - the depth would leak `len_longest_path`.  `depth` is still clamped in place (utils2.py:27)."""

    def __init__(self, emb_dim, num_nodetypes, num_nodeattributes, max_depth):
        super().__init__()
        self.max_depth = max_depth
        self.type_encoder = nn.Embedding(num_nodetypes, emb_dim)
        self.attribute_encoder = nn.Embedding(num_nodeattributes, emb_dim)

    def forward(self, x, depth):
        if x.is_cuda and self.type_encoder.weight.shape[1] % 4 == 0 and depth.dtype == torch.int64 \
                and depth.is_contiguous():
            tables = (self.type_encoder.weight, self.attribute_encoder.weight)
            if torch.is_grad_enabled() and any(t.requires_grad for t in tables):
                from .autograd import EncodeAST
                return EncodeAST.apply(x, depth, *tables, None, self.max_depth)
            return engine.encode_ast(x, depth, *tables, None, self.max_depth)
        # generic torch path (odd widths): same math as utils2.py:27-28
        depth[depth > self.max_depth] = self.max_depth
        return self.type_encoder(x[:, 0]) + self.attribute_encoder(x[:, 1])


def _ast_tables(enc):
    """(type, attribute, depth) tables of the two encoders the row kernels know - depth None for `ASTNodeEncoder2` - or None
    for an encoder of any other class (a user's own module, a subclass included: its `forward` may do anything)."""
    if type(enc) is ASTNodeEncoder:
        return enc.type_encoder.weight, enc.attribute_encoder.weight, enc.depth_encoder.weight
    if type(enc) is ASTNodeEncoder2:
        return enc.type_encoder.weight, enc.attribute_encoder.weight, None
    return None


class _EdgeAttnParams(nn.Module):
    """Parameter holder with the names of the reference's `AttnConv` (`dagnn.py:347-359`)."""

    def __init__(self, attn_q_dim, emb_dim, attn_dim=0, num_relations=1, reverse=False):
        super().__init__()
        attn_dim = attn_dim if attn_dim > 0 else emb_dim
        self.wea = num_relations > 1
        if self.wea:
            self.edge_encoder = nn.Linear(num_relations, attn_dim)
        self.attn_lin = nn.Linear(attn_q_dim + attn_dim, 1)
        self.reverse = reverse


class _SelfAttnParams(nn.Module):  # dagnn.py:279-290
    def __init__(self, emb_dim, attn_dim=0, num_relations=1, reverse=False):
        super().__init__()
        attn_dim = attn_dim if attn_dim > 0 else emb_dim
        self.wea = num_relations > 1
        if self.wea:
            self.edge_encoder = nn.Linear(num_relations, attn_dim)
        self.attn_lin = nn.Linear(attn_dim, 1)


class _MultAttnParams(nn.Module):  # dagnn.py:379-392
    def __init__(self, attn_q_dim, emb_dim, attn_dim=0, num_relations=1, reverse=False):
        super().__init__()
        attn_dim = attn_dim if attn_dim > 0 else emb_dim
        self.wea = num_relations > 1
        if self.wea:
            self.edge_encoder = nn.Linear(num_relations, attn_dim)
        self.attn_linl = nn.Linear(attn_q_dim, attn_q_dim)
        self.attn_linr = nn.Linear(attn_dim, attn_q_dim)


class _GatedSumParams(nn.Module):  # dagnn.py:254-265
    def __init__(self, emb_dim, num_relations=1, mapper_bias=True, reverse=False):
        super().__init__()
        self.wea = num_relations > 1
        if self.wea:
            self.edge_encoder = nn.Linear(num_relations, emb_dim)
        self.mapper = nn.Linear(emb_dim, emb_dim, bias=mapper_bias)
        self.gate = nn.Sequential(nn.Linear(emb_dim, emb_dim), nn.Sigmoid())


class _AggParams(nn.Module):  # dagnn.py:232-241
    def __init__(self, agg, num_relations=1, emb_dim=0):
        super().__init__()
        self.wea = num_relations > 1
        if self.wea:
            self.edge_encoder = nn.Linear(num_relations, emb_dim)


def _init_encoder(word_vectors, emb_dims):  # dagnn.py:218-223
    if word_vectors is not None:
        return nn.EmbeddingBag.from_pretrained(word_vectors, freeze=True, mode="sum")
    if len(emb_dims) > 0:
        return nn.EmbeddingBag(emb_dims[0], emb_dims[1], mode="sum")
    return None


class _HeadsLinear(torch.autograd.Function):
    """`out @ Wcat^T + bcat` for the S heads at once (their parameters are views of `wcat` / `bcat`: `DAGNN._head_storage`)
    with the gradients of the S weights and biases as views of ONE product."""

    @staticmethod
    def forward(ctx, out, wcat, bcat, V, *params):
        ctx.save_for_backward(out)
        ctx.wcat, ctx.V, ctx.S = wcat, V, len(params) // 2
        ctx.needs = (out.requires_grad, any(p.requires_grad for p in params))
        return torch.addmm(bcat, out, wcat.t())

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        wcat, V, S = ctx.wcat, ctx.V, ctx.S
        if g.stride(1) != 1:
            g = g.contiguous()
        d_out = g @ wcat if ctx.needs_input_grad[0] else None
        if ctx.needs[1]:
            D = out.shape[1]
            if g.stride(0) % 4 == 0 and g.data_ptr() % 16 == 0 and D % 2 == 0 and out.is_contiguous() and g.dtype == torch.float32:
                # (rows pitched to a multiple of 4 floats - what train.seq_cross_entropy hands back: csrc/wgrad.hip's own tiles
                # for a product that reduces 128 rows into 25 010 x 1 024 outputs, bias sums on the way)
                dw = torch.empty(S * V, D, dtype=torch.float32, device=g.device)
                db = torch.empty(S * V, dtype=torch.float32, device=g.device)
                engine.check(engine._lib.load().dagnn_tn_product(g.data_ptr(), g.stride(0), out.data_ptr(), out.stride(0), g.shape[0],
                                                                S * V, D, dw.data_ptr(), db.data_ptr(), engine._stream(g)),
                             "dagnn_tn_product")
            else:
                dw = g.t() @ out            # [S V, D]: the S weight gradients, one product
                db = g.sum(0)
            gw, gb = list(dw.split(V, 0)), list(db.split(V, 0))
        else:
            gw, gb = [None] * S, [None] * S
        return (d_out, None, None, None, *gw, *gb)


class DAGNN(HipModule):
    """See module docstring.  Constructor mirrors `dagnn.py:18-112` argument for argument."""

    _plain_dataflow_ok = True   # (variants.run_plain_dataflow: `add` / `max` of THIS class - one shared AggConv - on the dataflow kernel)

    def __init__(self, num_vocab, max_seq_len, emb_dim, hidden_dim, out_dim,
                 num_rels=2, w_edge_attr=True, num_layers=2, bidirectional=True, mapper_bias=True,
                 agg_x=False, agg=K.NA_ATTN_H, out_wx=True, out_pool_all=True, out_pool=K.P_MAX, encoder=None,
                 dropout=0.0, word_vectors=None, emb_dims=[], activation=None, num_class=0, recurr=1):
        super().__init__()
        self.num_class = num_class
        self.num_vocab = num_vocab
        self.max_seq_len = max_seq_len
        if agg_x and hidden_dim < emb_dim:
            raise ValueError('Hidden dimension too small for input.')

        self.agg = agg
        self.agg_x = agg_x
        self.agg_attn = "attn" in agg
        self.agg_attn_x = "_x" in agg
        self.bidirectional = bidirectional
        self.dirs = [0, 1] if bidirectional else [0]
        self.num_layers = num_layers
        self.out_wx = out_wx
        self.output_all = out_pool_all
        self.out_pool = out_pool
        self.recurr = recurr
        self.emb_dim = emb_dim
        self.hidden_dim = hidden_dim
        nd = len(self.dirs)
        self.out_hidden_dim = emb_dim * nd + hidden_dim * nd * num_layers if out_wx else hidden_dim * nd * num_layers

        self.encoder = encoder if encoder is not None else _init_encoder(word_vectors, emb_dims)

        # parameter creation order follows the reference so that seeded default inits coincide
        num_rels = num_rels if w_edge_attr else 1
        self.num_rels = num_rels
        pred_dim = emb_dim if agg_x else hidden_dim
        attn_dim = emb_dim if "_x" in agg else hidden_dim
        if "self_attn" in agg:
            self.node_aggr_0 = nn.ModuleList([_SelfAttnParams(attn_dim, num_relations=num_rels)
                                              for _ in range(num_layers)])
            self.node_aggr_1 = nn.ModuleList([_SelfAttnParams(attn_dim, num_relations=num_rels, reverse=True)
                                              for _ in range(num_layers)])
        elif "attn" in agg:
            op = _MultAttnParams if "mattn" in agg else _EdgeAttnParams
            self.node_aggr_0 = nn.ModuleList([
                op(emb_dim if l == 0 else attn_dim, pred_dim, num_relations=num_rels, attn_dim=attn_dim)
                for l in range(num_layers)])
            self.node_aggr_1 = nn.ModuleList([
                op(emb_dim if l == 0 else attn_dim, pred_dim, num_relations=num_rels, attn_dim=attn_dim, reverse=True)
                for l in range(num_layers)])
        elif agg == K.NA_GATED_SUM:
            self.node_aggr_0 = nn.ModuleList([_GatedSumParams(pred_dim, num_rels, mapper_bias=mapper_bias)
                                              for _ in range(num_layers)])
            self.node_aggr_1 = nn.ModuleList([_GatedSumParams(pred_dim, num_rels, mapper_bias=mapper_bias,
                                                              reverse=True) for _ in range(num_layers)])
        else:
            node_aggr = _AggParams(agg, num_rels, pred_dim)
            self.node_aggr_0 = self.node_aggr_1 = nn.ModuleList([node_aggr for _ in range(num_layers)])

        for d in self.dirs:
            if recurr:
                cells = [nn.GRUCell(emb_dim if l == 0 else hidden_dim, hidden_dim) for l in range(num_layers)]
            else:
                cells = [nn.Linear((emb_dim if l == 0 else hidden_dim) + hidden_dim, hidden_dim)
                         for l in range(num_layers)]
            setattr(self, "cells_{}".format(d), nn.ModuleList(cells))

        if out_pool == K.P_ATTN:
            dd = int(self.out_hidden_dim / 2) if self.bidirectional and not self.output_all else self.out_hidden_dim
            self.self_attn_linear_out = nn.Linear(dd, 1)

        self.dropout = nn.Dropout(dropout)
        if self.num_class > 0:
            self.graph_pred_linear = nn.Linear(self.out_hidden_dim, self.num_class)
        else:
            self.graph_pred_linear_list = nn.ModuleList()
            if self.num_vocab == 1:
                self.graph_pred_linear_list.append(nn.Sequential(nn.Linear(self.out_hidden_dim, self.num_vocab),
                                                                 nn.ReLU()))
            else:
                for _ in range(max_seq_len):
                    self.graph_pred_linear_list.append(nn.Linear(self.out_hidden_dim, self.num_vocab))

        self.schedule = default_schedule()  # 'lockstep' (frontier launches) or 'pergraph' (persistent workgroups)
        self.variant_backend = "hip"       # constructor-string variants (a12): 'hip' = csrc/variants.hip forward and
                                            # csrc/variants_bwd.hip reverse sweep; 'torch' = always the differentiable
                                            # torch-ROCm ops (the checker of the HIP sweep in the GPU tests)
                                            # 'dataflow' = as 'hip', but training passes of add / max run on the two
                                            # persistent dataflow kernels where `route.plain` allows (else exactly 'hip')
        self.last_variant_path = None      # what the last differentiable variant pass ran on: 'dataflow' | 'lockstep' | 'torch'
        self.last_variant_route = None     # ... and its `route.plain` (`.why`: the reason it stayed off the dataflow kernels)

    # ------------------------------------------------------------------------------ helpers
    # additive-attention aggregators: the logit is w . [query ; key (+ edge)] (+ b); query and bias cancel
    # inside the segment softmax, so all four reduce to "score of the key + edge gain"
    _HIP_AGGS = (K.NA_ATTN_H, K.NA_ATTN_X, K.NA_SELF_ATTN_H, K.NA_SELF_ATTN_X)

    def _hip_supported(self) -> bool:
        return self.agg in self._HIP_AGGS and not self.agg_x and bool(self.recurr)

    def _attn_geometry(self, i: int):
        """(offset of the key weights inside attn_lin.weight, key width) for stacked layer i."""
        key_dim = self.emb_dim if self.agg_attn_x else self.hidden_dim
        if "self_attn" in self.agg:
            return 0, key_dim                                   # SelfAttnConv: Linear(attn_dim, 1), no query
        attn_dim = self.emb_dim if self.agg_attn_x else self.hidden_dim
        return (self.emb_dim if i == 0 else attn_dim), key_dim  # AttnConv: Linear(attn_q_dim + attn_dim, 1)

    def _cells(self, fresh: bool = False):
        srcs: List[torch.Tensor] = []
        for d in self.dirs:
            for i in range(self.num_layers):
                c = getattr(self, "cells_%d" % d)[i]
                a = getattr(self, "node_aggr_%d" % d)[i]
                srcs += [c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh, a.attn_lin.weight]
                if a.wea:
                    srcs.append(a.edge_encoder.weight)

        def make():
            out = {}
            for d in self.dirs:
                for i in range(self.num_layers):
                    c = getattr(self, "cells_%d" % d)[i]
                    a = getattr(self, "node_aggr_%d" % d)[i]
                    dq, kd = self._attn_geometry(i)
                    out[(d, i)] = derive_cell(c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh, a.attn_lin.weight,
                                              self.hidden_dim, dq, i > 0, a.edge_encoder.weight if a.wea else None, 0,
                                              schedule=self.schedule, key_dim=kd, pack=False, stacked=self.num_layers)
            if self.schedule == "lockstep":
                pack_lockstep(out.values())
            return out

        return self._cache(self.schedule).get(srcs, make, fresh=fresh or self.training)

    def _folded_tables(self, cells):
        """Input side of stacked layer 0 by constant folding (evaluation only).  The node embedding is a sum of three table
        rows (utils.py:26-28) and nothing non-linear sits between it and `GRUCell`'s `W_ih x + b_ih` (dagnn.py:139,148,181), so
        `W_ih x_v + b_ih = (T W_ih^T)[type_v] + (A W_ih^T)[attr_v] + (D W_ih^T + b_ih)[depth_v]`: the three products depend on
        the PARAMETERS only and are made once per weight version (kept on the derived cell, like the packed matrices); per batch the
        [N, emb] x [emb, 3H] GEMM of every direction becomes the encoder's own row kernel on the folded tables.  Per
        direction (type, attribute, depth) tables of width 3Hp - depth None for `ASTNodeEncoder2`, whose two products are
        `T W_ih^T` and `A W_ih^T + b_ih` -, or None where it does not apply (other encoders, odd widths; training passes never ask)."""
        tabs = _ast_tables(self.encoder)
        if not engine.FOLD_INPUT or tabs is None or self.schedule != "lockstep" or self.agg_x:
            return None
        if self.training:
            # a no-grad pass on a module left in train() mode (validation without eval(), MC dropout): the derived cells are
            # rebuilt on every pass there, and re-folding three tables per direction each time costs what the fold saves
            return None
        if tabs[0].shape[1] % 4 or not tabs[0].is_cuda:
            return None
        # (every node takes exactly one row of the LAST table - depth, or attribute for `ASTNodeEncoder2`: the bias rides on it)
        last = 2 if tabs[2] is not None else 1
        key = tuple((p.data_ptr(), p._version) for p in tabs[:last + 1])
        out = []
        with torch.no_grad():
            for d in self.dirs:
                c = cells[(d, 0)]   # (the folded tables live and die with the derived cell: same invalidation rules, same width)
                if c.fold is None or c.fold[0] != key:
                    t, a, dp = (None if tab is None else engine.gemm_nt_bias([tab.detach()], [c.w_ih], [c.b_ih if j == last else None])[0]
                                for j, tab in enumerate(tabs))
                    c.fold = (key, (t, a, dp), built_marker(t))
                else:
                    meet_built(c.fold[2])   # (built by a pass on another stream, perhaps still in flight)
                out.append(c.fold[1])
        self.__dict__["fold_passes"] = self.__dict__.get("fold_passes", 0) + 1   # (tests assert the path a pass took)
        return out

    @staticmethod
    def _rows_ok(x_idx, depth) -> bool:
        return bool(x_idx.is_cuda and x_idx.dtype == torch.int64 and x_idx.dim() == 2 and x_idx.shape[1] == 2
                    and x_idx.is_contiguous() and depth.is_cuda and depth.dtype == torch.int64 and depth.is_contiguous())

    def _folded_gi0(self, x_idx, depth, cells):
        """gi0 of every direction from the folded tables (`_folded_tables`), or None."""
        if not self._rows_ok(x_idx, depth):
            return None
        folded = self._folded_tables(cells)
        if folded is None:
            return None
        return [engine.encode_ast(x_idx, depth, t, a, dp, self.encoder.max_depth) for (t, a, dp) in folded]

    def _prepare_fused(self, G, B, cells):
        """Evaluation passes: plan + dataflow schedule + encoder rows (+ folded gi0 rows) + side effect 1 as ONE pipeline of 7
        launches (`dagnn_prepare`, csrc/prepare.hip).  Returns (plan, gi0 or None) with `G.x` / `G.bi_layer_index` set, or None
        where the pipeline does not apply (the caller then takes the separate calls)."""
        tabs = _ast_tables(self.encoder)
        if not engine.PREPARE_FUSED or self.schedule != "lockstep" or tabs is None or \
                getattr(G, "_dagnn_plan", None) is not None:
            return None
        x_idx, depth = G.x, G.node_depth.view(-1, )
        enc = self.encoder
        if not (self._rows_ok(x_idx, depth) and tabs[0].shape[1] % 4 == 0 and G.edge_index.is_cuda):
            return None
        dev, N = x_idx.device, x_idx.shape[0]
        ea, r = self._route0(G, B, training=False)
        tables = [(*tabs, torch.empty(N, tabs[0].shape[1], dtype=torch.float32, device=dev))]
        folded = self._folded_tables(cells)
        gi0 = None
        if folded is not None:
            gi0 = [torch.empty(N, t.shape[1], dtype=torch.float32, device=dev) for (t, _, _) in folded]
            tables += [(t, a, dp, o) for (t, a, dp), o in zip(folded, gi0)]
        lidx = torch.empty(4, N, dtype=torch.int64, device=dev)
        plan = engine.build_plan(G.edge_index, G._bi_layer_idx0, G._bi_layer_idx1, G.batch, B, ea, launch=False)
        plan.route = r
        plan.launch_prepare(r.groups, enc=(x_idx, depth, enc.max_depth, tables), stack=(self._layer_index_srcs(G), lidx))
        G.bi_layer_index = lidx.view(2, 2, -1)   # side effect 1 (dagnn.py:130-133)
        G.x = tables[0][3]                       # side effects 2 + 3 (dagnn.py:139, utils.py:27)
        return plan, gi0

    def _route0(self, G, B, training: bool):
        """(the edge features the batch's plan carries, `route.before_plan` of this model on this batch): the padded width
        and the dataflow kernel's group count, which the plan's schedule is built for and the recurrence goes on from."""
        has_edge_enc = getattr(self.node_aggr_0[0], "wea", False)
        ea = G.edge_attr if has_edge_enc else None
        R = 0 if ea is None else int(ea.numel() // max(1, G.edge_index.shape[1]))
        return ea, route.before_plan(G.edge_index.device, self.hidden_dim, self.num_layers, len(self.dirs), R, B,
                                     keys_hidden=not (self.agg_x or self.agg_attn_x), edge_enc=has_edge_enc, training=training)

    def _training_pass(self) -> bool:
        """True when this call must be differentiable.  The HIP backward (csrc/backward.hip) covers the additive-attention
        aggregators with GRU cells on the lock-step schedule, with every read-out the constructor offers (`_readout`);
        other combinations raise instead of silently detaching."""
        if not (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            return False
        ok = self._hip_supported() and self.schedule == "lockstep" and self.emb_dim % 4 == 0
        if not ok:
            raise NotImplementedError(
                "the HIP backward pass covers the aggregators %s (any read-out) with the lock-step schedule; call "
                "this configuration under torch.no_grad() (evaluation) or freeze its parameters" % (self._HIP_AGGS,))
        return True

    # hooks of autograd.Recurrence
    _vid_nodes = 0

    def _key_offset(self, i: int) -> int:
        return self._attn_geometry(i)[0]

    def _static_scores(self, x, cells):
        """`*_x` aggregators: the keys are the node inputs, one score per node and cell (dagnn.py:175-177)."""
        if not self.agg_attn_x:
            return None
        return {k: torch.mv(x.detach(), c.key_raw) for k, c in cells.items()}

    def _pool_how(self) -> str:
        """The pool the kernels run.  P_ATTN (dagnn.py:114-117) is a softmax over a size-1 dimension: weights of exactly 1,
        i.e. add-pooling - and the exact derivative with respect to `self_attn_linear_out.{weight, bias}` is zero: a
        training step through the HIP read-out leaves their `.grad` at None (`train.ClipAdam`, like `torch.optim.Adam`,
        skips a parameter without a gradient)."""
        return K.P_ADD if self.out_pool in (K.P_ATTN, K.P_SUM) else self.out_pool

    def _readout_jobs(self, x, h):
        """The column blocks of the pooled vector, left to right, as (matrix, (d, i) - None for `x` -, scope, column):
        [d][x?, layer 0 .. L-1] over the output nodes of direction d (dagnn.py:184-193), or [x?, [d][layer 0 .. L-1]]
        over all nodes / over the output nodes of direction 0 (dagnn.py:194-202) - there `x` appears once."""
        L = self.num_layers
        xs = [(x, None)] if self.out_wx else []
        if self.bidirectional and not self.output_all:
            blocks = [(d, xs + [(h[d][i], (d, i)) for i in range(L)]) for d in (0, 1)]
        else:
            blocks = [(2 if self.output_all else 0, xs + [(h[d][i], (d, i)) for d in self.dirs for i in range(L)])]
        jobs, col = [], 0
        for scope, ts in blocks:
            for t, key in ts:
                jobs.append((t, key, scope, col))
                col += t.shape[1]
        return jobs

    def _readout(self, plan, B, x, h):
        """The read-out, for every (bidirectional, out_pool_all, out_pool, out_wx): the pooled graph vectors
        [B, out_hidden_dim] from the states in ONE launch (`_readout_jobs`; P_ATTN pools as add: `_pool_how`)."""
        how = self._pool_how()
        jobs = [(t, scope, how, col) for t, _, scope, col in self._readout_jobs(x, h)]
        out = torch.empty(B, jobs[-1][3] + jobs[-1][0].shape[1], dtype=torch.float32, device=x.device)   # (the blocks tile it)
        engine.readout_pool_batch(plan, jobs, out)
        return out

    def _readout_backward(self, plan, x, h, gout, g_ext, dx):
        """`gout` [B, out_hidden_dim] straight into the reverse sweep's seeds `g_ext[d][i]` and into `dx`: no [N, H]
        gradient tensors in between.  Jobs of one launch add into distinct buffers, so the second `x` block of the
        bidirectional output-node read-out with `out_wx` goes in a launch of its own: `dx` takes direction 0's share in
        the first launch and direction 1's in the second, always in that order, which fixes its bits."""
        how = self._pool_how()
        first, second = [], []
        for t, key, scope, col in self._readout_jobs(x, h):
            job = (t, scope, how, col, dx if key is None else g_ext[key[0]][key[1]])
            (second if key is None and any(j[4] is dx for j in first) else first).append(job)
        engine.readout_pool_backward_batch(plan, first, gout)
        engine.readout_pool_backward_batch(plan, second, gout)

    def _state_side_effects(self, G, x, h):
        """Side effect 4 (dagnn.py:141-142,182) and those of the read-out branch (dagnn.py:124-126,194-202) after a training
        step whose read-out ran in HIP: `G.h` - and `G.batch` - as `_finish` leaves them, from the non-differentiable states.
        Unidirectional without `out_pool_all` narrows both to the output nodes, which needs a row count: that one mask
        index (a host synchronisation, as the evaluation path has it) stays; the pooling itself does not use it."""
        L, dirs = self.num_layers, self.dirs
        if self.bidirectional and not self.output_all:
            G.h = [[h[d][i] for i in range(L)] for d in dirs]
            return
        G.h = torch.cat(([x.detach()] if self.out_wx else []) + [h[d][i] for d in dirs for i in range(L)], dim=-1)
        if not self.output_all:
            idx = G.bi_layer_index[1][1][G.bi_layer_index[1][0] == 0]  # dagnn.py:124-126
            G.h, G.batch = G.h[idx], G.batch[idx]

    def _pool(self, h, batch, B):
        """`global_{max,mean,add}_pool` / P_ATTN read-outs on torch (variants outside BASELINE)."""
        how = self.out_pool
        if how == K.P_ATTN:  # dagnn.py:114-117: softmax over a size-1 dim == 1 -> sum pooling
            w = F.softmax(self.self_attn_linear_out(h), dim=-1)
            h, how = w * h, K.P_ADD
        idx = batch.view(-1, 1).expand_as(h)
        out = h.new_zeros(B, h.shape[1])
        if how == K.P_MAX:
            return out.scatter_reduce_(0, idx, h, "amax", include_self=False)
        out.scatter_add_(0, idx, h)
        if how == K.P_MEAN:
            cnt = torch.bincount(batch, minlength=B).clamp(min=1).to(h.dtype).view(-1, 1)
            out = out / cnt
        return out

    def _plan_of(self, G, B, overlap: bool = False):
        """The batch's plan.  With `overlap` the plan kernels (and the dataflow schedule's) run on a side stream next
        to the encoder and the batched input GEMM, which do not depend on them; the recurrence waits for `plan.ready`."""
        has_edge_enc = getattr(self.node_aggr_0[0], "wea", False)
        if getattr(G, "_dagnn_plan", None) is not None:  # built by the loader (dagnn_amd.host_plan.attach_plan)
            if has_edge_enc or int(G._dagnn_plan_meta.get("R", 0)) == 0:
                if overlap:
                    self._set_layer_index(G)
                return engine.PlanHandle.from_words(G._dagnn_plan, G._dagnn_plan_meta, getattr(G, "_dagnn_df", None))
            # the loader packed edge features this model has no encoder for (w_edge_attr=False): the kernels would
            # want an edge gain per feature - build the plan without them here instead
        if not (overlap and G.edge_index.is_cuda and self.schedule == "lockstep"):
            if overlap:
                self._set_layer_index(G)
            return engine.build_plan(G.edge_index, G._bi_layer_idx0, G._bi_layer_idx1, G.batch, B, G.edge_attr if has_edge_enc else None)
        dev = G.edge_index.device
        ea, r = self._route0(G, B, self._training_pass())   # (`plan.route`: the recurrence goes on from it)
        groups = r.groups
        # every buffer comes from the CALLER's pool (no `record_stream`, no foreign-pool blocks that cannot be reused: a forward
        # that allocated under a side stream cost seven hipMalloc calls per batch); only the launches may go to a side stream
        plan = engine.build_plan(G.edge_index, G._bi_layer_idx0, G._bi_layer_idx1, G.batch, B, ea, launch=False)
        plan.route = r
        if groups > 0:
            plan.dataflow_schedule(groups, launch=False)
        srcs = self._layer_index_srcs(G)
        stack = None
        if engine.PREPARE_FUSED and all(t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() for t in srcs):
            stack = (srcs, torch.empty(4, srcs[0].shape[0], dtype=torch.int64, device=dev))

        def launch():
            if engine.PREPARE_FUSED:   # plan + schedule (+ side effect 1 on its second launch) as one pipeline (csrc/prepare.hip)
                plan.launch_prepare(groups, stack=stack)
            else:
                plan.launch_build()
                if groups > 0:
                    plan.dataflow_schedule(groups)

        if engine.PLAN_OVERLAP:
            # ... on the arena's side stream, next to the encoder and the input GEMM of a training pass, which do not depend on
            # them; the side stream forks here and joins at `plan.wait_ready()`
            cur = torch.cuda.current_stream(dev)
            side = self._arena_for(G.edge_index).side_stream(dev)
            side.wait_stream(cur)
            with engine.launch_on(side):
                launch()
            plan.ready = torch.cuda.Event()
            plan.ready.record(side)
        else:
            launch()
        if stack is not None:
            G.bi_layer_index = stack[1].view(2, 2, -1)   # side effect 1 (dagnn.py:130-133); on the caller's stream after `plan.wait_ready()`
        else:
            self._set_layer_index(G)
        return plan

    @staticmethod
    def _layer_index_srcs(G):
        return [G._bi_layer_idx0, G._bi_layer_index0, G._bi_layer_idx1, G._bi_layer_index1]

    @classmethod
    def _set_layer_index(cls, G):
        """side effect 1 (dagnn.py:130-133): `G.bi_layer_index` [2, 2, N] (one copy kernel instead of three)"""
        G.bi_layer_index = torch.stack(cls._layer_index_srcs(G), dim=0).view(2, 2, -1)

    # ------------------------------------------------------------------------------ forward
    def forward(self, G):
        return self._pass(G, self._heads)

    def predict(self, G, return_top: bool = False):
        """Evaluation passes of the TOK task (ogbg-code/main_pyg.py:101-109): the predicted token matrix [B, S] (int64) -
        equal by contract to `torch.cat([torch.argmax(p, dim=1).view(-1, 1) for p in model(G)], dim=1)` under
        `torch.no_grad()`, with `forward`'s side effects on `G` - from ONE pass over the heads that never writes the
        [B, S V] logits (`dagnn_heads_argmax`, csrc/predict.hip; `num_class` models: [B, 1]).  Among equal logits the lowest
        column wins and a NaN beats every number, as `torch.argmax` decides.  `return_top=True` also returns [B, S, 2]: the
        winning logit and the runner-up.  Evaluation mode only (a training step has its logits: `evaluate.rows_argmax`)."""
        if self.training:
            raise RuntimeError("DAGNN.predict is an evaluation pass: call model.eval() first (the argmax of a training step's "
                               "logits is dagnn_amd.evaluate.rows_argmax)")
        with torch.no_grad():
            tok, top = self._pass(G, self._heads_argmax)
        return (tok, top) if return_top else tok

    def score(self, G, y_arr=None, topk: int = 1, sums=None):
        """An evaluation pass that says more than `predict` and still never writes the [B, S V] logits (`dagnn_heads_score`,
        csrc/predict.hip): an `evaluate.Score` with `tok` / `logit` [B, S, topk] - the `topk` (1..8) best columns of every
        (graph, head) and their logits, best first in `predict`'s order, so `tok[:, :, 0]` IS `predict(G)` - `lse` [B, S], and
        with targets `y_arr` [B, S] (`num_class` models: [B] or [B, 1]) `nll` [B, S], the row terms of the reference's
        criterion `CrossEntropyLoss` (ogbg-code/main_pyg.py:37,55-60): `.loss` is `train.seq_cross_entropy(model(G), y_arr)` by
        definition, `.logprob` the log-probabilities of the candidates.  A target outside [0, V) makes its row's `nll` NaN.
        `sums`: an `evaluate.SeqLoss` the pass adds its row losses to, inside its own launch.  `forward`'s side effects on
        `G`; evaluation mode only, under `torch.no_grad()` (a training step has its logits and `train.seq_ce_step`)."""
        from .evaluate import Score
        if self.training:
            raise RuntimeError("DAGNN.score is an evaluation pass: call model.eval() first (a training step has its logits: "
                               "dagnn_amd.train.seq_ce_step)")
        topk = int(topk)
        if not 1 <= topk <= 8:
            raise ValueError("DAGNN.score: topk must lie in 1..8 (got %d)" % topk)
        if sums is not None and y_arr is None:
            raise ValueError("DAGNN.score: `sums` accumulates row losses: targets needed")
        with torch.no_grad():
            return Score(*self._pass(G, lambda out: self._heads_score(out, y_arr, topk, sums)))

    def attention(self, G, logits: bool = False):
        """The attention weights of an evaluation pass (PyG's `return_attention_weights`; a hook on `AttnConv.message` in the
        reference): an `evaluate.Attention` with `out` = what `forward(G)` returns, from the same pass and with its side effects
        on `G`; `alpha` [len(dirs), num_layers, E] fp32, the weight direction d, stacked layer l gave edge e (column of
        `G.edge_index`; parallel edges each their own); `logit` (with `logits=True`) the pre-softmax scores, query part and
        biases included.  Two launches behind the pass for all cells (`dagnn_attention_weights`, csrc/attention.hip; mattn_h:
        its projection GEMMs and one; more than 16 cells go in chunks of 16), no synchronisation of its own.  Evaluation mode only, under `torch.no_grad()`;
        `agg_x=True` raises NotImplementedError, an aggregator without attention ValueError."""
        from .attention import run
        return run(self, G, logits)

    def _heads_score(self, out, y_arr, topk, sums):
        """(tok, logit, lse, nll) of the heads on the pooled graph vectors: the head step of `score`, routed as
        `_heads_argmax` routes `predict`'s."""
        single = self.num_class > 0
        heads = [self.graph_pred_linear] if single else list(self.graph_pred_linear_list)
        S = len(heads)
        if y_arr is not None:
            if y_arr.numel() != out.shape[0] * S:
                raise ValueError("DAGNN.score: targets [%d, %d] needed (got %s)" % (out.shape[0], S, tuple(y_arr.shape)))
            y_arr = y_arr.reshape(out.shape[0], S).to(out.device)
            if y_arr.dtype != torch.int64:
                y_arr = y_arr.to(torch.int64)
        if out.is_cuda and out.dtype == torch.float32 and all(
                isinstance(hd, nn.Linear) and hd.bias is not None and hd.weight.dtype == torch.float32 and hd.weight.is_cuda
                for hd in heads):
            wcat, bcat = (heads[0].weight, heads[0].bias) if single else self._head_storage()
            return engine.heads_score(out, wcat.detach(), bcat.detach(), S, heads[0].weight.shape[0], y=y_arr, k=topk,
                                      sums=None if sums is None else sums.sums, arena=self._arena_for(out))
        from .evaluate import rows_score
        pred = self._heads(out)
        res = rows_score([pred] if single else pred, y_arr, topk)
        if sums is not None:
            sums.update(res[3])
        return res

    def _pass(self, G, head):
        """`forward` up to the pooled graph vectors, then `head` on them (`_heads`: the logits; `_heads_argmax`: `predict`;
        `_heads_score`: `score`)."""
        L, H, dirs = self.num_layers, self.hidden_dim, self.dirs
        if not self._hip_supported():
            # constructor strings outside every BASELINE configuration: same contract, torch-ROCm ops
            if not G.x.is_cuda:
                raise engine.DagnnHipError("DAGNN.forward needs its batch on a ROCm GPU (there is no CPU path)")
            from . import variants
            self._set_layer_index(G)
            B = num_graphs_of(G)
            G.x = self.encoder(G.x, G.node_depth.view(-1, ))
            if self.variant_backend == "torch" or (torch.is_grad_enabled()
                                                    and any(p.requires_grad for p in self.parameters())):
                variants.drop_caches(self)
                if self.variant_backend != "torch" and variants.hip_backward_supported(self, G):
                    # gated_sum / mattn_h / add with GRU cells: forward AND reverse sweep in HIP (csrc/variants_bwd.hip)
                    plan = self._plan_of(G, B)
                    flat_params = [p for d in self.dirs for i in range(L) for _, p in variants._cell_params(self, d, i)]
                    # add / max under variant_backend = 'dataflow': both persistent kernels where `route.plain` says so
                    r = self.last_variant_route = variants.plain_route(self, plan, G.x.shape[0], G.x.device, training=True)
                    if r.kind == "dataflow":
                        self.last_variant_path = "dataflow"
                        flat = variants.PlainRecurrence.apply(self, plan, r, G.x, *flat_params)
                    else:
                        self.last_variant_path = "lockstep"
                        flat = variants.VariantRecurrence.apply(self, G, plan, G.x, *flat_params)
                    return self._finish(G, plan, G.x, self._unflatten(flat), B, head)   # (the plan: HIP read-out, `PoolNodes`)
                if self.variant_backend != "torch":   # (an explicit 'torch' backend is a choice, not a cliff)
                    variants.warn_torch_path(self, G)
                self.last_variant_path = "torch"
                return self._finish(G, None, G.x, variants.run(self, G, G.x), B, head)   # training: differentiable torch ops
            plan = self._plan_of(G, B)
            h = variants.run_hip(self, G, G.x, plan)
            self._guard_params(G.x)
            return self._finish(G, plan, G.x, h, B, head)
        train = self._training_pass()

        B = num_graphs_of(G)
        if not train:
            cells = self._cells()
            fused = self._prepare_fused(G, B, cells)   # (plan + schedule + encoder + side effect 1: one pipeline, csrc/prepare.hip)
            if fused is not None:
                plan, gi0 = fused
                x = G.x
                sscore = self._static_scores(x, cells)
                h = run_stack(plan, x, cells, dirs, L, H, schedule=self.schedule, static_score=sscore,
                              arena=self._arena_for(x), gi0=gi0, route=plan.route)
                self._guard_params(x)
                return self._finish(G, plan, x, h, B, head)
        # side effect 1 (dagnn.py:130-133) + the plan: on a side stream next to the encoder and the input GEMM, which do not
        # depend on them (`engine.PLAN_OVERLAP`); the caller's stream meets it again in front of the recurrence
        plan = self._plan_of(G, B, overlap=True)
        # side effects 2+3 (dagnn.py:139, utils.py:27): embedding replaces G.x, depth clamped in place
        x_idx, depth = G.x, G.node_depth.view(-1, )
        G.x = self.encoder(x_idx, depth)
        x = G.x
        if train:
            # differentiable call: the read-out and its backward in HIP for every (bidirectional, out_pool_all, out_pool,
            # out_wx) (`_readout` / `_readout_backward`: hooks of autograd.Recurrence); the states come back non-differentiable
            from .autograd import Recurrence
            res = Recurrence.apply(self, plan, B, True, x, *self._train_params())
            self._state_side_effects(G, x, self._unflatten(res[1:]))
            self.__dict__["readout_hip_passes"] = self.__dict__.get("readout_hip_passes", 0) + 1   # (tests assert the path a pass took)
            return head(self.dropout(res[0]))
        cells = self._cells()
        sscore = self._static_scores(x, cells)
        h = run_stack(plan, x, cells, dirs, L, H, schedule=self.schedule, static_score=sscore,
                      arena=self._arena_for(x), gi0=self._folded_gi0(x_idx, depth, cells), route=plan.route)
        self._guard_params(x)
        return self._finish(G, plan, x, h, B, head)

    def _head_storage(self):
        """The S vocabulary heads' weights and biases as ONE [S V, D] / [S V] pair: each head's parameter is (made) a VIEW of
        it - same names, shapes and values in `state_dict`, same `Parameter` objects for the optimizer - so the heads are one
        matrix for the library GEMMs without a concatenation per pass (102 MB at the headline shape) and without a cache that
        could go stale: an in-place update of a head IS an update of the matrix.  Re-established when something re-seated the
        parameters' storage (`module.to()`, `deepcopy`)."""
        heads = list(self.graph_pred_linear_list)
        V, D = heads[0].weight.shape
        st = self.__dict__.get("_heads_flat")
        w0 = heads[0].weight
        ok = st is not None and st[0].device == w0.device and st[0].dtype == w0.dtype
        if ok:
            for i, hd in enumerate(heads):
                if hd.weight.data_ptr() != st[0].data_ptr() + i * V * D * st[0].element_size() or \
                        hd.bias.data_ptr() != st[1].data_ptr() + i * V * st[1].element_size():
                    ok = False
                    break
        if not ok:
            with torch.no_grad():
                w = torch.cat([hd.weight.data for hd in heads], 0)
                b = torch.cat([hd.bias.data for hd in heads], 0)
                for i, hd in enumerate(heads):
                    hd.weight.data = w[i * V:(i + 1) * V]
                    hd.bias.data = b[i * V:(i + 1) * V]
            st = self.__dict__["_heads_flat"] = (w, b)
        return st

    def _heads(self, out):
        """The prediction heads on the pooled graph vectors (dagnn.py:204-215)."""
        if self.num_class > 0:
            return self.graph_pred_linear(out)
        if self.num_vocab > 1 and self.max_seq_len > 1 and out.is_cuda and out.dtype == torch.float32 and \
                all(isinstance(hd, nn.Linear) for hd in self.graph_pred_linear_list):
            # the S vocabulary heads as ONE library GEMM (dagnn.py:212-215 runs S): their parameters are views of one matrix
            # (`_head_storage`), the list entries are views of its output.  Under autograd the GEMM and its two backward
            # products are one node (`_HeadsLinear`); a caller that takes the loss through `train.seq_cross_entropy` meets
            # the logits as ONE tensor there too (fifteen 25-us GEMMs + ~50 loss launches -> 3 + 2).
            wcat, bcat = self._head_storage()
            if torch.is_grad_enabled() and (out.requires_grad or any(p.requires_grad for p in self.graph_pred_linear_list.parameters())):
                heads = list(self.graph_pred_linear_list)
                logits = _HeadsLinear.apply(out, wcat, bcat, self.num_vocab, *[hd.weight for hd in heads], *[hd.bias for hd in heads])
            else:
                logits = torch.addmm(bcat, out, wcat.t())
            return list(logits.split(self.num_vocab, dim=1))
        return [self.graph_pred_linear_list[i](out) for i in range(self.max_seq_len)]

    def _heads_argmax(self, out):
        """(tok [B, S], top [B, S, 2]) of the heads on the pooled graph vectors: the head step of `predict`.  Plain `nn.Linear`
        heads on an fp32 GPU `out` are one pass of `dagnn_heads_argmax`; anything else takes `_heads` + torch, as `_heads`
        itself falls back."""
        single = self.num_class > 0
        heads = [self.graph_pred_linear] if single else list(self.graph_pred_linear_list)
        if out.is_cuda and out.dtype == torch.float32 and all(
                isinstance(hd, nn.Linear) and hd.bias is not None and hd.weight.dtype == torch.float32 and hd.weight.is_cuda
                for hd in heads):
            wcat, bcat = (heads[0].weight, heads[0].bias) if single else self._head_storage()
            return engine.heads_argmax(out, wcat.detach(), bcat.detach(), len(heads), heads[0].weight.shape[0],
                                       arena=self._arena_for(out))
        pred = self._heads(out)
        pred = [pred] if single else pred
        tok = torch.cat([torch.argmax(p, dim=1).view(-1, 1) for p in pred], dim=1)
        top = torch.stack([torch.cat([p.float(), p.new_full((p.shape[0], 1), float("-inf")).float()], 1).topk(2, dim=1).values
                           for p in pred], dim=1)
        return tok, top

    def _finish(self, G, plan, x, h, B, head=None):
        """Read-out + `head` (default `_heads`: dagnn.py:184-215) on the states h[d][i]: of an evaluation pass, and of the
        constructor-string variants' training passes (the additive-attention path trains through `_readout`).  With a plan the
        pooling is HIP - `autograd.PoolNodes` where a gradient is wanted -, without one (`variant_backend = "torch"`, the
        variants' torch fall-back) torch ops."""
        L, dirs = self.num_layers, self.dirs
        cap = self.__dict__.get("_attn_capture")
        if cap is not None:   # (`attention`: the pass's plan, inputs and states, before the read-out narrows `G`)
            cap.update(plan=plan, x=x, h=h, E=G.edge_index.shape[1])
        G.h = [[h[d][i] for i in range(L)] for d in dirs]  # side effect 4 (dagnn.py:141-142,182)

        differentiable = torch.is_grad_enabled() and (x.requires_grad or any(h[d][i].requires_grad
                                                                             for d in dirs for i in range(L)))
        hip_pool = plan is not None and not differentiable
        # a differentiable read-out of ordinary autograd tensors (the constructor-string variants' HIP training branch): HIP
        # pool and HIP backward as one autograd node per matrix (`autograd.PoolNodes`) - no mask index, no scatter
        node_pool = plan is not None and differentiable and all(
            t.is_cuda and t.dtype == torch.float32 for t in [x] + [h[d][i] for d in dirs for i in range(L)])
        if node_pool:
            from .autograd import PoolNodes
            self.__dict__["readout_hip_passes"] = self.__dict__.get("readout_hip_passes", 0) + 1   # (tests assert the path a pass took)
        how = self._pool_how()   # (P_ATTN pools as add)
        if self.bidirectional and not self.output_all:
            if hip_pool:
                out = self._readout(plan, B, x, h)   # one launch for all (direction, stacked layer) columns
            elif node_pool:
                out = torch.cat([PoolNodes.apply(plan, t, d, how) for d in (0, 1)
                                 for t in ([x] if self.out_wx else []) + [h[d][i] for i in range(L)]], dim=-1)
            else:
                outs = []
                for d in (0, 1):
                    idx = G.bi_layer_index[1 - d][1][G.bi_layer_index[1 - d][0] == 0]
                    hd = torch.cat(([x] if self.out_wx else []) + [h[d][i] for i in range(L)], dim=-1)
                    outs.append(self._pool(hd[idx], G.batch[idx], B))
                out = torch.cat(outs, dim=-1)
        else:
            G.h = torch.cat(([x] if self.out_wx else []) + [h[d][i] for d in dirs for i in range(L)], dim=-1)
            if hip_pool:   # over all nodes, or over the output nodes of direction 0 (dagnn.py:124-126,194-202)
                out = self._readout(plan, B, x, h)
            elif node_pool:
                out = PoolNodes.apply(plan, G.h, 2 if self.output_all else 0, how)
            if not self.output_all:
                idx = G.bi_layer_index[1][1][G.bi_layer_index[1][0] == 0]  # dagnn.py:124-126
                G.h, G.batch = G.h[idx], G.batch[idx]
            if not (hip_pool or node_pool):
                out = self._pool(G.h, G.batch, B)

        return (head or self._heads)(self.dropout(out))
