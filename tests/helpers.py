"""Fixture loading and model construction shared by the CPU and GPU test tiers."""
from __future__ import annotations

import json
import os
from types import SimpleNamespace

import numpy as np
import torch

import dagnn_amd
from dagnn_amd import DAGNN, DAGNN_BN, DAGNN_NA, ASTNodeEncoder
from oracle.seeding import seeded_fill

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CODE2 = ["code2_h32_bidir", "code2_h256_bidir", "code2_h512_L5", "code2_h300_L3", "code2_h64_unidir",
         "code2_h64_numclass", "code2_h128_deep", "code2_h64_attn_x", "code2_h64_self_attn_h",
         "code2_h64_self_attn_x"]
VARIANTS = ["var_h64_" + t for t in ("gated_sum", "gated_nobias", "mattn_h", "add", "max", "aggx_attn_h", "aggx_add",
                                        "recurr0", "recurr0_gated")]
GRAD = ["grad_h32_bidir", "grad_h256_bidir", "grad_h128_deep", "grad_h64_L3_wx", "grad_h300_bidir", "grad_h64_unidir",
        "grad_h64_mean_all"]
GRAD_VAR = ["grad_var_h64_" + t for t in ("gated_sum", "gated_nobias", "mattn_h", "add", "mattn_h_L3", "max", "recurr0_gated",
                                           "recurr0_mattn", "recurr0_attn_h", "recurr0_attn_x", "recurr0_self_attn_h",
                                           "aggx_attn_h", "aggx_add", "aggx_gated", "aggx_mattn", "aggx_max_recurr0")]
DVAE_GRAD = ["grad_na_h64_unidir", "grad_bn_h64_bidir", "grad_na_h501_unidir", "grad_bn_h501_bidir",
             "grad_na_h64_self_attn_h", "grad_bn_h64_self_attn_h",
             "grad_na_h64_gated_sum", "grad_na_h64_add", "grad_na_h64_max", "grad_bn_h64_add", "grad_bn_h64_max"]
DVAE = ["na_h128_unidir", "na_h64_bidir", "bn_h256_bidir", "bn_h64_unidir", "na_h64_poolall_max", "bn_h64_poolall_mean",
        "na_h501_unidir", "bn_h501_bidir",   # the reference's default width (dvae/train.py:55)
        "na_h64_self_attn_h", "bn_h128_self_attn_h",   # agg='self_attn_h' (dvae/dagnn.py:49-54)
        "na_h64_gated_sum", "na_h64_add", "na_h64_max", "bn_h64_add", "bn_h64_max"]   # dvae/dagnn.py:60-70


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k: z[k] for k in z.files if k != "meta"}


def code2_model(meta):
    H = meta["H"]
    enc = ASTNodeEncoder(H, 98, meta["n_attr"], 20)
    model = DAGNN(num_vocab=meta["V"], max_seq_len=meta["S"], emb_dim=H, hidden_dim=H, out_dim=None, encoder=enc,
                  **meta["ctor"]).eval()
    seeded_fill(model, meta["w_seed"])
    return model


def code2_batch(arr, device="cpu"):
    t = lambda k, dt=None: torch.from_numpy(arr[k].copy()).to(device)  # noqa: E731
    N = arr["x"].shape[0]
    ids = torch.arange(N, device=device)
    return SimpleNamespace(x=t("x"), node_depth=t("node_depth"), edge_index=t("edge_index"), edge_attr=t("edge_attr"),
                           batch=t("batch"), _bi_layer_idx0=t("layer0"), _bi_layer_index0=ids,
                           _bi_layer_idx1=t("layer1"), _bi_layer_index1=ids.clone(),
                           num_graphs=int(arr["batch"].max()) + 1)


def dvae_graphs(meta, arr):
    """The fixture's graphs, decoded from its stored rows (ENAS / BN encodings) by our own decoders."""
    import json as _json
    from dagnn_amd import synth
    rows = [_json.loads(r) for r in arr["rows"]]
    return [(synth.decode_enas_row if meta["kind"] == "na" else synth.decode_bn_row)(r) for r in rows]


def dvae_model(meta):
    cls, nn_ = (DAGNN_NA, 8) if meta["kind"] == "na" else (DAGNN_BN, 10)
    hs = meta["hs"]
    model = cls(nn_, hs, hs, nn_, nn_, 0, 1, hs=hs, nz=56, num_nodes=nn_, agg=meta.get("agg", "attn_h"), num_layers=meta["L"],
                bidirectional=meta["bidir"], out_wx=False, out_pool_all=meta.get("out_pool_all", False),
                out_pool=meta.get("out_pool", "max"), dropout=0.0).eval()
    seeded_fill(model, meta["w_seed"])
    return model, nn_


def dvae_batch(arr, device="cpu"):
    t = lambda k: torch.from_numpy(arr[k].copy()).to(device)  # noqa: E731
    return dagnn_amd.GraphBatch(x=t("x"), edge_index=t("edge_index"), bi_layer_index=t("bi_layer_index"),
                                batch=t("batch"))


def maxdiff(a, b):
    a = a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.as_tensor(a).double()
    b = b.detach().cpu().double() if isinstance(b, torch.Tensor) else torch.as_tensor(b).double()
    return float((a - b).abs().max()) if a.numel() else 0.0


def grad_view(meta, name, g):
    """The rows of a full gradient that a gradient fixture stores (tests/golden/make_golden.sample_grad)."""
    return g[::meta["grad_stride"][name]]


def check_grads(meta, arr, grads, rtol=2e-4, atol=2e-7, verbose=False):
    """Compare {name: gradient} with a gradient fixture: stored rows and the float64 sum of every parameter,
    relative to the largest entry of that gradient (+ `atol`: the gradients of the attention query weights,
    attention bias and edge-encoder bias are mathematically zero - they cancel inside the segment softmax - and
    come out of the reference's autograd as ~1e-9 rounding noise).  Returns the worst relative error."""
    worst = 0.0
    for key in arr:
        if not key.startswith("g::"):
            continue
        name = key[3:]
        ref = torch.from_numpy(arr[key]).double()
        got = grad_view(meta, name, grads[name].detach().cpu()).double()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        scale = float(ref.abs().max())
        aerr = float((got - ref).abs().max())
        abs_sum = float(arr["gsum::" + name][1])
        serr = abs(float(grads[name].detach().cpu().double().sum()) - float(arr["gsum::" + name][0]))
        if verbose:
            print("%-44s max|g| %.3e  err %.3e  sum err %.3e / %.3e" % (name, scale, aerr, serr, abs_sum))
        assert aerr <= rtol * scale + atol, "%s: max abs err %.3g at scale %.3g" % (name, aerr, scale)
        assert serr <= rtol * abs_sum + atol * got.numel() ** 0.5 * 10, "%s: sum err %.3g of %.3g" % (name, serr, abs_sum)
        worst = max(worst, aerr / max(scale, 1e-30) if scale > 100 * atol else 0.0)
    return worst


# ------------------------------------------------------------------ decoder-side single-vertex step
class VertexGraph(object):
    """The igraph surface `_ipropagate_to` touches: `vcount()`, `predecessors(v)` (ascending), `vs[x][attr]`."""

    def __init__(self, n):
        self.vs = [dict() for _ in range(n)]
        self._pred = [[] for _ in range(n)]

    def vcount(self):
        return len(self.vs)

    def predecessors(self, v):
        return sorted(self._pred[v])


def iprop_graphs(meta, arr, device):
    gs = []
    for k in range(meta["K"]):
        g = VertexGraph(int(arr["counts"][k]))
        for v in range(g.vcount()):
            g.vs[v]["type"] = int(arr["types"][k, v])
            for l in range(meta["L"]):
                g.vs[v]["H_forward%d" % l] = torch.from_numpy(arr["states"][k, v, l][None].copy()).to(device)
            g._pred[v] = [u for u in range(v) if arr["adj"][k, u, v]]
        gs.append(g)
    return gs


def check_ipropagate(name, step, device, tol):
    """`step(model, G, v, H=None)` against the `iprop_*` fixture generated from the reference's `_ipropagate_to`."""
    meta, arr = load(name)
    meta = dict(meta, bidir=False)
    model, nvt = dvae_model(meta)
    model = model.to(device)
    K, n, L = meta["K"], meta["n"], meta["L"]
    with torch.no_grad():
        for v in meta["vs"]:
            G = iprop_graphs(meta, arr, device)
            Hv = step(model, G, v)
            alive = [k for k in range(K) if arr["counts"][k] > v]
            assert alive == list(arr["v%d_alive" % v])
            assert maxdiff(Hv, arr["v%d_Hv" % v]) < tol
            got = np.stack([np.stack([G[k].vs[v]["H_forward%d" % l][0].cpu().numpy() for l in range(L)]) for k in alive])
            assert np.abs(got - arr["v%d_states" % v]).max() < tol
            Hg = step(model, iprop_graphs(meta, arr, device), v, H=torch.from_numpy(arr["H_given"].copy()).to(device))
            assert maxdiff(Hg, arr["v%d_Hv_given" % v]) < tol
        assert step(model, iprop_graphs(meta, arr, device), n + 3) is None   # no graph has that vertex


# ------------------------------------------------------------------ float64 references (the oracle's autograd at any size)
_REF64 = {}


def _cpu_state(model):
    """`state_dict` on the CPU with its aliases kept (the D-VAE encoders register their GRUs under two names; the oracle
    reports a gradient under every name of one storage)."""
    seen, out = {}, {}
    for k, v in model.state_dict().items():
        key = (v.data_ptr(), tuple(v.shape), tuple(v.stride()))
        if key not in seen:
            seen[key] = v.detach().cpu()
        out[k] = seen[key]
    return out


def code2_grads64(key, model, b, y, **kw):
    """`(loss, {name: gradient})` of `O.code2_grads` in float64 for (model, batch, y): computed once per session and `key` (the
    full-size cases cost ~30-60 s of CPU each; several GPU paths compare against the SAME reference).  `key=None`: not cached.
    The oracle mutates its batch: it gets a deep copy."""
    import copy
    from oracle import dagnn_oracle as O
    if key is None or key not in _REF64:
        sd = _cpu_state(model)
        loss, grads = O.code2_grads(sd, copy.deepcopy(b), y.cpu(), dtype=torch.float64, **kw)
        # one module under several names (`agg` = add / max: ONE AggConv for every cell, dagnn.py:74-75) takes the sum of
        # the gradients the oracle's separate leaves received, under each of its names
        groups = {}
        for k, v in sd.items():
            if k in grads:
                groups.setdefault((v.data_ptr(), tuple(v.shape), tuple(v.stride())), []).append(k)
        for ks in groups.values():
            if len(ks) > 1:
                tot = sum(grads[k] for k in ks)
                grads.update({k: tot for k in ks})
        val = (loss, grads)
        if key is None:
            return val
        _REF64[key] = val
    return _REF64[key]


def dvae_grads64(key, model, G, r1, r2, **kw):
    """`(loss, {name: gradient})` of `O.dvae_grads` in float64 (loss <mu, r1> + <logvar, r2>), cached like `code2_grads64`."""
    import copy
    from oracle import dagnn_oracle as O
    if key is None or key not in _REF64:
        val = O.dvae_grads(_cpu_state(model), copy.deepcopy(G), r1.cpu(), r2.cpu(), dtype=torch.float64, **kw)
        if key is None:
            return val
        _REF64[key] = val
    return _REF64[key]


def check_grads_full(model, ref, rtol=1e-4, atol=2e-7):
    """Every named parameter's `.grad` (zeros where there is none) against the full reference gradient: max abs error
    <= rtol x its largest entry + atol (`atol`: the mathematically zero gradients of the attention and edge-encoder biases
    come out as rounding noise).  Returns (worst error relative to the largest entry, its parameter) over the gradients
    larger than 100 x atol - the baseline a later change can be compared with."""
    worst = (0.0, None)
    for k, p in model.named_parameters():
        r = ref[k] if k in ref else torch.zeros(p.shape, dtype=torch.float64)   # (the oracle omits what takes no part)
        g = torch.zeros_like(p) if p.grad is None else p.grad
        assert g.shape == r.shape, (k, g.shape, r.shape)
        scale = float(r.abs().max())
        err = maxdiff(g, r)
        assert err <= rtol * scale + atol, "%s: max abs err %.3g at scale %.3g" % (k, err, scale)
        if scale > 100 * atol:
            worst = max(worst, (err / scale, k))
    return worst


def grad_norm64(model, ref):
    """The float64 global 2-norm of the reference gradients of `model`'s parameters (what clip_grad_norm_ sees)."""
    return float(torch.sqrt(sum((ref[k].double() ** 2).sum() for k, _ in model.named_parameters() if k in ref)))


# ------------------------------------------------------------------ D-VAE decoders at free shapes (test_dvae_decoder_f64_gpu)
def dvae_decoder_model(kind, *, max_n, nvt, hs, L, nz=8, start_type=0, end_type=1, agg="attn_h", seed=0):
    """DAGNN_NA (kind 'na') or DAGNN_BN ('bn') with free max_n / nvt / hs / L / nz / START_TYPE / END_TYPE: emb_dim = nvt,
    hidden_dim = hs, num_nodes = max_n (the widths the reference's decoder needs), weights from `seeded_fill`."""
    cls = DAGNN_NA if kind == "na" else DAGNN_BN
    model = cls(nvt, hs, hs, max_n, nvt, start_type, end_type, hs=hs, nz=nz, num_nodes=max_n, agg=agg, num_layers=L,
                bidirectional=kind == "bn", out_wx=False, out_pool_all=False, out_pool="max", dropout=0.0).eval()
    seeded_fill(model, seed)
    return model


GRAPH_FAMILIES = ("none", "chain", "star", "complete", "random0.2", "random0.5", "random0.8", "one_complete")


def dvae_dense_graphs(family, B, n, nvt, start_type, seed):
    """(types [B, n], preds [B, n]) int32 of B graphs of one family: no edges, a chain, a star out of vertex 0, the
    complete DAG (P = v at every vertex), random at density 0.2 / 0.5 / 0.8, or one complete graph among edgeless ones
    (that row alone sets every padding width).  Types at vertices >= 1 avoid start_type; vertex 0 has start_type."""
    rng = np.random.default_rng(seed)
    others = [t for t in range(nvt) if t != start_type]
    types = np.asarray(others, np.int64)[rng.integers(0, len(others), size=(B, n))]
    types[:, 0] = start_type
    adj = np.zeros((B, n, n), bool)   # [b, v, u]: edge u -> v
    lower = np.tril(np.ones((n, n), bool), -1)
    if family == "chain":
        adj[:, np.arange(1, n), np.arange(n - 1)] = True
    elif family == "star":
        adj[:, 1:, 0] = True
    elif family == "complete":
        adj[:] = lower
    elif family.startswith("random"):
        adj = (rng.random((B, n, n)) < float(family[6:])) & lower
    elif family == "one_complete":
        adj[int(rng.integers(0, B))] = lower
    elif family != "none":
        raise ValueError(family)
    preds = (adj.astype(np.int64) << np.arange(n)).sum(2)
    return types.astype(np.int32), preds.astype(np.uint32).view(np.int32)


def dvae_graphs_from_dense(types, preds, nvt):
    """Graph objects `loss()` / `encode()` take, from dense types and predecessor masks."""
    from dagnn_amd import synth
    out = []
    for t, p in zip(np.asarray(types), np.asarray(preds).view(np.uint32)):
        n = len(t)
        adj = np.zeros((n, n))
        for v in range(n):
            for u in range(v):
                if int(p[v]) >> u & 1:
                    adj[u, v] = 1
        out.append(synth._adj_to_graph(adj, [int(x) for x in t], nvt))
    return out


def dvae_decoder64(key, model, types, preds, mu, logvar, graphs=None, diag=None):
    """The float64 teacher-forced `loss()` of `oracle.dvae_decoder_oracle` for (model, types, preds, mu, logvar):
    (loss, res, kld, vertex_ll, edge_ll, {name: gradient}, diag), cached per `key` like `code2_grads64`.  With `graphs`,
    mu / logvar come from the float64 encoder oracle on those graphs (one leaf per shared storage, so the layer-0
    gate / mapper get the encoder's and the decoder's gradients added)."""
    from oracle import dagnn_oracle as O
    from oracle import dvae_decoder_oracle as DO
    if key is not None and key in _REF64:
        return _REF64[key]
    sd = _cpu_state(model)
    kind = "bn" if isinstance(model, DAGNN_BN) else "na"
    kw = dict(kind=kind, agg=model.agg, L=model.num_layers, start_type=int(model.START_TYPE))
    d = {}
    if graphs is None:
        loss, res, kld, vll, ell, grads = DO.decoder_loss_grads(sd, types, preds, mu.cpu(), logvar.cpu(), diag=d, **kw)
    else:
        by_ptr, leaves = {}, {}
        for k, v in sd.items():
            if v.is_floating_point():
                pk = (v.data_ptr(), tuple(v.shape), tuple(v.stride()))
                by_ptr.setdefault(pk, v.detach().double().clone().requires_grad_(True))
                leaves[k] = by_ptr[pk]
        b = dagnn_amd.GraphBatch.from_data_list([g.clone() for g in graphs])
        mu64, lv64 = O.dvae_encode(leaves, b, num_layers=model.num_layers, bidirectional=model.bidirectional,
                                   num_nodes=model.num_nodes, vids=kind == "na", agg=model.agg, dtype=torch.float64,
                                   keep_graph=True)
        H0 = torch.tanh(mu64 @ leaves["fc3.weight"].t() + leaves["fc3.bias"])
        res, vll, ell = DO.decoder_loss(leaves, types, preds, H0, diag=d, **kw)
        kld = -0.5 * torch.sum(1 + lv64 - mu64.pow(2) - lv64.exp())
        loss = res + 0.005 * kld
        names = list(leaves)
        gs = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
        grads = {k: g for k, g in zip(names, gs) if g is not None}
        loss, res, kld, vll, ell = (t.detach() for t in (loss, res, kld, vll, ell))
    val = (loss, res, kld, vll, ell, grads, d)
    if key is not None:
        _REF64[key] = val
    return val


# ------------------------------------------------------------------ shared by the GPU gradient tests
def _degenerate_batch(extra=()):
    """Single-node graphs, a chain, stars with a 200-way fan-in / fan-out, a graph with no edges, a duplicate edge
    (`extra`: more graphs behind them)."""
    from dagnn_amd import GraphData
    from dagnn_amd.dag_utils import add_order_info_01

    def g(n, edges, attr=None):
        ei = torch.tensor(edges, dtype=torch.long).t().reshape(2, -1)
        ea = torch.zeros(ei.shape[1], 2) if attr is None else torch.tensor(attr, dtype=torch.float32)
        d = GraphData(x=torch.stack([torch.arange(n) % 98, torch.arange(n) % 300], 1),
                      node_depth=(torch.arange(n) % 30).view(-1, 1), edge_index=ei, edge_attr=ea)
        add_order_info_01(d)
        return d

    graphs = [g(1, []), g(5, []), g(40, [(i, i + 1) for i in range(39)]),
              g(201, [(i, 200) for i in range(200)], [[i % 2, 0] for i in range(200)]),
              g(201, [(0, i) for i in range(1, 201)]), g(2, [(0, 1), (0, 1)])]
    from dagnn_amd import synth
    return synth.GraphBatch.from_data_list(graphs + list(extra))


def _train_step(model, G, y, fused_loss=False):
    model.train()
    model.zero_grad(set_to_none=True)
    pred = model(G)
    if fused_loss:   # the same loss through the library's one-launch entry (train.seq_cross_entropy, csrc/loss.hip)
        from dagnn_amd.train import seq_cross_entropy
        loss = seq_cross_entropy(pred, y)
    else:
        loss = sum(torch.nn.functional.cross_entropy(p, y[:, s]) for s, p in enumerate(pred)) / len(pred)  # main_pyg.py:55-60
    loss.backward()
    return loss.detach(), {k: (torch.zeros_like(p) if p.grad is None else p.grad) for k, p in model.named_parameters()}
