"""A float64 oracle of `DAGNN_NA(agg='gated_sum').encode` - the reference's loop (`dvae/dagnn.py:99-184` with `GatedSumConv`,
`:271-298`) vertex by vertex under torch autograd - and its tie to the layer-wise restatement `_gated_sum_states`, which the
reference fixture `dvae_gated_loss_na_h64_encode` pins (tests/test_dvae_gated_gpu.py).  No GPU: the GPU tests of
tests/test_dvae_gated_train_gpu.py import the oracle and `torch_path_encode` from here."""
from __future__ import annotations

import pytest
import torch

from dagnn_amd import DAGNN_NA, synth
from dagnn_amd.data import GraphBatch

N_NODES = 8   # vertices per graph = num_nodes = max_n (synth.decode_enas_row)


def make_model(hs, L, bidir, pool_all=False, seed=0, nz=16):
    torch.manual_seed(seed)
    return DAGNN_NA(N_NODES, hs, hs, N_NODES, N_NODES, 0, 1, hs=hs, nz=nz, num_nodes=N_NODES, num_layers=L, bidirectional=bidir,
                    agg="gated_sum", out_pool_all=pool_all)


def make_graphs(B, seed=5):
    return [synth.decode_enas_row(r) for r in synth.enas_rows(seed, B)]


def cotangent(B, nz, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, nz, generator=g, dtype=torch.float64), torch.randn(B, nz, generator=g, dtype=torch.float64)


def _gru(x, h, w_ih, w_hh, b_ih, b_hh):
    """nn.GRUCell on one vertex (gate order r, z, n)."""
    H = h.shape[0]
    gi, gh = w_ih @ x + b_ih, w_hh @ h + b_hh
    r = torch.sigmoid(gi[:H] + gh[:H])
    z = torch.sigmoid(gi[H:2 * H] + gh[H:2 * H])
    n = torch.tanh(gi[2 * H:] + r * gh[2 * H:])
    return (1 - z) * n + z * h


def oracle_encode(state_dict, graphs, hs, L, bidir, pool_all=False, out_pool="max"):
    """(mu, logvar, {canonical parameter name: float64 leaf}) of the reference's encoder, one vertex at a time: vertex v of
    direction d reads, per stacked layer i, the messages gate(hs_j) * mapper(hs_j) of its predecessors j in edge order with
    hs_j = [h_j ; one-hot(j mod num_nodes)] (dagnn.py:130-141,293-295), their sum is the hidden state of GRUCell(input, .)
    (None -> zeros at layer 0), and the cell's output is the next stacked layer's input (dagnn.py:144-145)."""
    b = GraphBatch.from_data_list([g.clone() for g in graphs])
    x = b.x.double()
    N = x.shape[0]
    ei = b.edge_index
    P = {k: v.detach().double().clone().requires_grad_(True) for k, v in state_dict.items()
         if k.split(".")[0] in ("grue_forward", "grue_backward", "gate_forward", "gate_backward", "mapper_forward",
                                "mapper_backward", "hg_unify", "out_linear", "fc1", "fc2")}
    dirs = [0, 1] if bidir else [0]
    eye = torch.eye(N_NODES, dtype=torch.float64)
    h = {}
    for d in dirs:
        sfx = "forward" if d == 0 else "backward"
        layer_of = b.bi_layer_index[d][0]
        order = sorted(range(N), key=lambda v: (int(layer_of[v]), v))
        hd = [[None] * N for _ in range(L)]
        for v in order:
            preds = [int(ei[d][e]) for e in range(ei.shape[1]) if int(ei[1 - d][e]) == v]
            assert all(int(layer_of[j]) < int(layer_of[v]) for j in preds)
            assert (len(preds) == 0) == (int(layer_of[v]) == 0)
            inp = x[v]
            for i in range(L):
                wg, bg = P["gate_%s.%d.0.weight" % (sfx, i)], P["gate_%s.%d.0.bias" % (sfx, i)]
                wm = P["mapper_%s.%d.0.weight" % (sfx, i)]
                a = torch.zeros(hs, dtype=torch.float64)
                for j in preds:
                    hj = torch.cat([hd[i][j], eye[j % N_NODES]])
                    a = a + torch.sigmoid(wg @ hj + bg) * (wm @ hj)
                inp = _gru(inp, a, *(P["grue_%s.%d.%s" % (sfx, i, n)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
                hd[i][v] = inp
        h[d] = [torch.stack(hd[i]) for i in range(L)]
    B = N // N_NODES
    if pool_all:
        hg = torch.cat([h[d][i] for d in dirs for i in range(L)], dim=-1)
        if bidir:
            hg = hg @ P["hg_unify.0.weight"].t() + P["hg_unify.0.bias"]
        elif L > 1:
            hg = hg @ P["out_linear.weight"].t() + P["out_linear.bias"]
        hg = hg.view(B, N_NODES, -1)
        Hg = {"max": hg.max(1)[0], "mean": hg.mean(1), "add": hg.sum(1)}[out_pool]
    else:
        last = torch.arange(N_NODES - 1, N, N_NODES)
        parts = [h[0][i][last] for i in range(L)]
        if bidir:
            parts += [h[1][i][last - (N_NODES - 1)] for i in range(L)]
        Hg = torch.cat(parts, dim=-1)
        if bidir:
            Hg = Hg @ P["hg_unify.0.weight"].t() + P["hg_unify.0.bias"]
        elif L > 1:
            Hg = Hg @ P["out_linear.weight"].t() + P["out_linear.bias"]
    mu = Hg @ P["fc1.weight"].t() + P["fc1.bias"]
    logvar = Hg @ P["fc2.weight"].t() + P["fc2.bias"]
    return mu, logvar, P


def oracle_grads(state_dict, graphs, hs, L, bidir, cot, pool_all=False):
    """(mu, logvar, {name: gradient of sum(mu * cot[0] + logvar * cot[1])}), all float64; a parameter the encoder does not
    reach has a zero gradient."""
    mu, logvar, P = oracle_encode(state_dict, graphs, hs, L, bidir, pool_all)
    ((mu * cot[0]).sum() + (logvar * cot[1]).sum()).backward()
    return mu.detach(), logvar.detach(), {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in P.items()}


def torch_path_encode(model, graphs):
    """(mu, logvar) through `_gated_sum_states` and the read-outs of `_forward_plain_agg` (dvae/dagnn.py:147-184), in the
    model's own device and precision: the differentiable torch-ops path training used before the HIP reverse sweep took
    the vertex-id columns, and still the fall-back."""
    p0 = next(model.parameters())
    b = GraphBatch.from_data_list([g.clone() for g in graphs]).to(p0.device)
    x = b.x.to(p0.dtype).contiguous()
    N, L, nn_ = x.shape[0], model.num_layers, model.num_nodes
    h = model._gated_sum_states(b, x)
    if model.output_all:
        Hg = model._pool_all(b, None, x, [h[d][i] for d in model.dirs for i in range(L)], N // nn_)
    else:
        first = torch.arange(0, N, nn_, device=x.device)
        parts = [h[0][i][first + (nn_ - 1)] for i in range(L)]
        if model.bidirectional:
            parts += [h[1][i][first] for i in range(L)]
        Hg = torch.cat(parts, dim=-1)
        Hg = model.hg_unify(Hg) if model.bidirectional else (model.out_linear(Hg) if L > 1 else Hg)
    return model.fc1(Hg), model.fc2(Hg)


def path_grads(model, encode, cot):
    """(mu, logvar, {name: gradient}) of `encode()` -> (mu, logvar) under the fixed cotangent, as float64 CPU tensors."""
    model.zero_grad(set_to_none=True)
    mu, logvar = encode()
    c0, c1 = (c.to(mu.device, mu.dtype) for c in cot)
    ((mu * c0).sum() + (logvar * c1).sum()).backward()
    grads = {k: (p.grad.detach().double().cpu() if p.grad is not None else torch.zeros(p.shape, dtype=torch.float64))
             for k, p in model.named_parameters()}
    return mu.detach().double().cpu(), logvar.detach().double().cpu(), grads


def rel_err(got, ref):
    """max |got - ref| / max |ref| of one tensor (0 for a tensor that is zero in exact arithmetic and in `got`)."""
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


@pytest.mark.parametrize("bidir", [False, True])
@pytest.mark.parametrize("pool_all", [False, True])
def test_oracle_equals_the_layerwise_torch_path_in_float64(bidir, pool_all):
    """hs = 8, L = 2: mu, logvar and every parameter gradient of the per-vertex oracle and of `_gated_sum_states` + read-out,
    both float64 on the CPU on the same weights, agree to 1e-9 relative - two orders of summation of the same expression."""
    hs, L, B = 8, 2, 5
    model = make_model(hs, L, bidir, pool_all).double()
    graphs = make_graphs(B)
    cot = cotangent(B, 16)
    mu_o, lv_o, g_o = oracle_grads(model.state_dict(), graphs, hs, L, bidir, cot, pool_all)
    mu_t, lv_t, g_t = path_grads(model, lambda: torch_path_encode(model, graphs), cot)
    assert rel_err(mu_t, mu_o) <= 1e-9 and rel_err(lv_t, lv_o) <= 1e-9
    reached = 0
    for k, _ in model.named_parameters():
        if k not in g_o:   # the decoder's parameters: the encoder does not reach them
            assert float(g_t[k].abs().max()) == 0, k
            continue
        assert rel_err(g_t[k], g_o[k]) <= 1e-9, (k, rel_err(g_t[k], g_o[k]))
        reached += float(g_o[k].abs().max()) > 0
    sfx = ["forward", "backward"] if bidir else ["forward"]
    for s in sfx:   # the vertex-id columns carry gradient of their own
        for i in range(L):
            for k in ("gate_%s.%d.0.weight" % (s, i), "mapper_%s.%d.0.weight" % (s, i)):
                assert float(g_o[k][:, hs:].abs().max()) > 0, k
    assert reached >= (8 if bidir else 6) * L


def test_the_sweep_takes_any_hidden_width_for_gated_add_max():
    """`hip_backward_supported`: hidden widths that are no multiple of 4 pass for gated_sum / add / max (D-VAE views and plain
    DAGNN alike) and still not for mattn_h; emb_dim % 4 and the 8-cell cap stay."""
    from dagnn_amd import DAGNN, variants
    for agg, ok in (("gated_sum", True), ("add", True), ("max", True), ("mattn_h", False)):
        m = DAGNN(3, 1, emb_dim=8, hidden_dim=38, out_dim=None, w_edge_attr=False, num_layers=2, bidirectional=True, agg=agg)
        assert variants.hip_backward_supported(m, None) is ok, agg
    assert not variants.hip_backward_supported(DAGNN(3, 1, emb_dim=6, hidden_dim=38, out_dim=None, w_edge_attr=False, agg="add"), None)
    assert not variants.hip_backward_supported(DAGNN(3, 1, emb_dim=8, hidden_dim=38, out_dim=None, w_edge_attr=False, num_layers=5, agg="add"), None)
    view = make_model(501, 2, True)._agg_view()
    assert variants.hip_backward_supported(view, None)
    assert variants.row_pitch(501) == 504 and variants.row_pitch(37) == 40 and variants.row_pitch(32) == 32
