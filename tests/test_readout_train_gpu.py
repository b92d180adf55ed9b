"""The training read-out on the GPU (-m gpu): `dagnn_readout_pool_batch` / `dagnn_readout_pool_backward_batch`
(csrc/readout.hip) at kernel level on one hand-made batch, then `DAGNN`, the constructor-string variants and the D-VAE
encoders through them for one training step each against float64 autograd through the oracle.

Bounds.  The forward is a float32 host replay's arithmetic (`_replay`: the first node's value, then `np.maximum` or one
fp32 `+` per node in the plan's visiting order, then one fp32 multiply by 1 / count for mean): bit for bit.  Backward, ADD and MAX from a zero `grad_h`:
every element receives ONE addend, an fp32 number of `grad_out` itself, so the float64 reference cast to fp32 is hit
exactly.  MEAN: the factor 1.f / count and its product with `grad_out` are two fp32 roundings, (1 + 2^-24)^2 - 1 < 2.4e-7
relative.  Accumulation into a pre-filled `grad_h` is one fp32 addition of that addend: bit for bit.  Model level:
`helpers.check_grads_full` at its defaults, the project's bound for a training step against float64 autograd, and the loss
within 1e-5 of the oracle's (the bound of the training-step tests of tests/test_gpu_parity.py; the D-VAE loss, a sum over
B x 112 terms, within 1e-4 of its size as `test_full_size_dvae_training_step` there has it)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from dagnn_amd import ASTNodeEncoder, DAGNN, GraphBatch, GraphData, dag_utils, engine, synth
from dagnn_amd import _lib
from dagnn_amd.autograd import PoolNodes
from oracle.seeding import seeded_fill
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

MODES = {"max": _lib.POOL_MAX, "add": _lib.POOL_ADD, "mean": _lib.POOL_MEAN}
CASES = [(scope, how) for scope in (0, 1, 2) for how in ("max", "add", "mean")]
WIDTHS = [1, 4, 255, 257]   # (257: a thread's second trip at 256 threads)
COL0 = 5                    # a nonzero column offset; the output rows are wider than the columns used
EINVAL = -22


def bits(t):
    return t.contiguous().view(torch.int32)


# ============================================================================= the hand-made batch
def _hand_batch():
    """5 graphs, 18 nodes: a single node; two nodes joined by a double edge; a 5-chain; a 6-way fan-in star; three nodes
    without edges (each both source and sink)."""
    shapes = [(1, []), (2, [(0, 1), (0, 1)]), (5, [(i, i + 1) for i in range(4)]), (7, [(i, 6) for i in range(6)]), (3, [])]
    graphs = []
    for n, edges in shapes:
        ei = torch.tensor(edges, dtype=torch.long).reshape(len(edges), 2).t().contiguous()
        g = GraphData(x=torch.zeros(n, 1), edge_index=ei)
        dag_utils.add_order_info_01(g)
        graphs.append(g)
    return GraphBatch.from_data_list(graphs)


@pytest.fixture(scope="module")
def hand(device):
    b = _hand_batch()
    plan = engine.build_plan(b.edge_index.to(device), b._bi_layer_idx0.to(device), b._bi_layer_idx1.to(device), b.batch.to(device),
                             b.num_graphs, None)
    plan.check_status()
    # the node sets from the LAYER IDS, not from the plan: output nodes of direction d = layer 0 of the other direction
    masks = [b._bi_layer_idx1 == 0, b._bi_layer_idx0 == 0, torch.ones_like(b.batch, dtype=torch.bool)]
    return b, plan, masks


@pytest.fixture(scope="module")
def visits(hand):
    """`_visits` of the hand batch; the SET of nodes per (scope, graph) is the one the layer ids describe - only the order
    is the plan's."""
    b, plan, masks = hand
    visit = _visits(plan, b)
    for scope in range(3):
        for g in range(b.num_graphs):
            want = torch.nonzero(masks[scope] & (b.batch == g)).view(-1).tolist()
            assert sorted(visit[scope][g].tolist()) == want and len(set(visit[scope][g].tolist())) == len(want), (scope, g)
    return visit


def _pitched(N, W, gen, device, ints=False):
    """[N, W] view of a [N, W + 3] buffer (ld = W + 3: rows that are neither contiguous nor aligned)."""
    buf = (torch.randint(0, 3, (N, W + 3), generator=gen).float() if ints else torch.randn(N, W + 3, generator=gen)).to(device)
    return buf, buf[:, :W]


def _pool64(h, mask, batch, B, how):
    """The pool of dagnn.py:119-126,194-202 on index ops in float64 (differentiable)."""
    idx = torch.nonzero(mask).view(-1)
    rows, seg = h[idx], batch[idx]
    out = torch.zeros(B, h.shape[1], dtype=h.dtype)
    if how == "max":
        return out.scatter_reduce(0, seg.view(-1, 1).expand_as(rows), rows, "amax", include_self=False)
    out = out.index_add(0, seg, rows)
    if how == "mean":
        out = out / torch.bincount(seg, minlength=B).clamp(min=1).to(h.dtype).view(-1, 1)
    return out


def _visits(plan, b):
    """visit[scope][g]: the node ids the kernels read for graph g, in their visiting order - scope 0 / 1 from the plan's
    own words (`depth`, `lstart`, `order` of direction 1 - scope, ONE copy of `plan.ws`), scope 2 ascending node ids."""
    lay, ws, B = plan.layout(), plan.ws.cpu().numpy(), b.num_graphs
    node_ptr = ws[lay["node_ptr"]:lay["node_ptr"] + B + 1]
    visit = []
    for scope in (0, 1):
        od = 1 - scope
        per = []
        for g in range(B):
            ls = ws[lay["lstart%d" % od] + node_ptr[g] + g:][:2]
            p0, p1 = (int(ls[0]), int(ls[1])) if ws[lay["depth%d" % od] + g] > 0 else (0, 0)
            per.append(ws[lay["order%d" % od] + p0:lay["order%d" % od] + p1].copy())
        visit.append(per)
    visit.append([np.arange(node_ptr[g], node_ptr[g + 1]) for g in range(B)])
    return visit


def _replay(h, nodes_of, how):
    """The forward on the host in numpy float32.  h [N, W] float32; nodes_of[g]: graph g's nodes in visiting order."""
    out = np.zeros((len(nodes_of), h.shape[1]), dtype=np.float32)
    for g, nodes in enumerate(nodes_of):
        if len(nodes) == 0:
            continue   # nothing in scope: 0
        m = h[nodes[0]].copy()
        for v in nodes[1:]:
            m = np.maximum(m, h[v]) if how == "max" else m + h[v]
        out[g] = m * (np.float32(1) / np.float32(len(nodes))) if how == "mean" else m
    assert out.dtype == np.float32
    return out


def _replay_backward(h, go, nodes_of, how):
    """The backward from a zero `grad_h` on the host: go [B, W] float32 -> [N, W] float32 (one addend per element; max: to
    the first node in visiting order attaining the column maximum)."""
    gh = np.zeros_like(h)
    cols = np.arange(h.shape[1])
    for g, nodes in enumerate(nodes_of):
        if len(nodes) == 0:
            continue
        if how == "max":
            rows = h[nodes]
            gh[np.asarray(nodes)[np.argmax(rows, axis=0)], cols] = go[g]   # (numpy: the FIRST of equal maxima, in `nodes` order)
        else:
            gh[nodes] = go[g] * (np.float32(1) / np.float32(len(nodes))) if how == "mean" else go[g]
    return gh


def _forward_jobs(views):
    arr = (_lib.PoolJob * len(CASES))()
    W = views[0].shape[1]
    for k, ((scope, how), h) in enumerate(zip(CASES, views)):
        arr[k] = _lib.PoolJob(h.data_ptr(), h.stride(0), W, scope, MODES[how], COL0 + k * W)
    return arr


def _backward(plan, views, gout, grads, h_null_unless_max=True):
    """One launch of the nine (scope, mode) jobs; grads[k]: the [N, W] view job k adds into."""
    arr = (_lib.PoolBwdJob * len(CASES))()
    W = views[0].shape[1]
    for k, ((scope, how), h, gh) in enumerate(zip(CASES, views, grads)):
        hp = h.data_ptr() if (how == "max" or not h_null_unless_max) else None
        arr[k] = _lib.PoolBwdJob(hp, gh.data_ptr(), h.stride(0), gh.stride(0), W, scope, MODES[how], COL0 + k * W)
    rc = _lib.load().dagnn_readout_pool_backward_batch(C.byref(plan.desc), arr, len(CASES), gout.data_ptr(), gout.stride(0),
                                                       engine._stream(gout))
    assert rc == 0
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def kernel_runs(hand, device):
    """Per width: inputs, the batch forward, the backward from zero (twice) and from a pre-filled `grad_h`, computed once."""
    b, plan, masks = hand
    N, B = b.batch.shape[0], b.num_graphs
    runs = {}
    for W in WIDTHS:
        gen = torch.Generator().manual_seed(100 + W)
        hs = [_pitched(N, W, gen, device) for _ in CASES]
        views = [v for _, v in hs]
        ld_out = COL0 + len(CASES) * W + 2
        out = torch.full((B, ld_out), -7.0, device=device)
        rc = _lib.load().dagnn_readout_pool_batch(C.byref(plan.desc), _forward_jobs(views), len(CASES), out.data_ptr(), ld_out,
                                                  engine._stream(out))
        assert rc == 0
        gout = torch.randn(B, ld_out, generator=gen).to(device)
        zero = [torch.zeros(N, W + 1, device=device) for _ in CASES]            # (ld_g = W + 1)
        zero2 = [torch.zeros(N, W + 1, device=device) for _ in CASES]
        init = [torch.randn(N, W + 1, generator=gen).to(device) for _ in CASES]
        acc = [t.clone() for t in init]
        _backward(plan, views, gout, [t[:, :W] for t in zero])
        _backward(plan, views, gout, [t[:, :W] for t in zero2], h_null_unless_max=False)
        _backward(plan, views, gout, [t[:, :W] for t in acc])
        runs[W] = dict(views=views, out=out, ld_out=ld_out, gout=gout, zero=zero, zero2=zero2, init=init, acc=acc)
    return runs


# ============================================================================= kernel level
@pytest.mark.parametrize("W", WIDTHS)
def test_forward_batch_is_the_single_job_kernel_bit_for_bit(hand, visits, kernel_runs, device, W):
    """Nine (scope, mode) jobs in one launch against `_replay`, which shares no source with the kernel."""
    b, plan, masks = hand
    r = kernel_runs[W]
    host = np.full((b.num_graphs, r["ld_out"]), -7.0, dtype=np.float32)
    for k, ((scope, how), h) in enumerate(zip(CASES, r["views"])):
        host[:, COL0 + k * W:COL0 + (k + 1) * W] = _replay(h.cpu().numpy(), visits[scope], how)
    assert np.array_equal(r["out"].cpu().numpy().view(np.int32), host.view(np.int32))   # (the columns no job owns still hold the sentinel)
    assert bool((r["out"][:, :COL0] == -7.0).all()) and bool((r["out"][:, COL0 + len(CASES) * W:] == -7.0).all())
    for k, ((scope, how), h) in enumerate(zip(CASES, r["views"])):   # ... and it is the pool the layer ids describe
        ref = _pool64(h.double().cpu(), masks[scope], b.batch, b.num_graphs, how)
        # (at most 7 nodes: 6 fp32 additions, each within 2^-24 of a partial sum <= sum |v|, + the mean's two roundings)
        bound = 9 * 2.0 ** -24 * _pool64(h.double().cpu().abs(), masks[scope], b.batch, b.num_graphs, "add")
        for got in (r["out"][:, COL0 + k * W:COL0 + (k + 1) * W].double().cpu(),
                    torch.from_numpy(host[:, COL0 + k * W:COL0 + (k + 1) * W]).double()):   # (the kernel's, the replay's on its own)
            assert bool(((got - ref).abs() <= bound).all()), (scope, how)


@pytest.mark.parametrize("W", WIDTHS)
def test_backward_against_float64_autograd_of_an_index_built_pool(hand, kernel_runs, W):
    b, plan, masks = hand
    r = kernel_runs[W]
    for k, ((scope, how), h) in enumerate(zip(CASES, r["views"])):
        h64 = h.double().cpu().requires_grad_(True)
        g64 = r["gout"][:, COL0 + k * W:COL0 + (k + 1) * W].double().cpu()
        (_pool64(h64, masks[scope], b.batch, b.num_graphs, how) * g64).sum().backward()
        ref = h64.grad
        got = r["zero"][k][:, :W].cpu()
        err = (got.double() - ref).abs()
        worst = float((err / ref.abs().clamp(min=1e-300)).max()) if how == "mean" else float(err.max())
        print("W=%d scope=%d %s: %s %.3g" % (W, scope, how, "max rel err" if how == "mean" else "max abs err vs fp32(ref)", worst))
        if how == "mean":
            assert bool((err <= 2.4e-7 * ref.abs()).all()), (scope, how, worst)
        else:
            assert torch.equal(bits(got), bits(ref.float())), (scope, how)
        assert bool((r["zero"][k][:, W:] == 0).all())      # (the pitch column behind the rows stays untouched)


@pytest.mark.parametrize("W", WIDTHS)
def test_backward_adds_into_a_prefilled_grad_h_and_repeats_bit_for_bit(kernel_runs, W):
    r = kernel_runs[W]
    for k, (scope, how) in enumerate(CASES):
        addend, init, acc = r["zero"][k], r["init"][k], r["acc"][k]
        assert torch.equal(bits(acc), bits(init + addend)), (scope, how)    # fp32 init + addend (+ 0 leaves a value as it is)
        assert torch.equal(bits(r["zero2"][k]), bits(addend)), (scope, how)  # a second run (h given where it is not read)


def test_max_ties(hand, visits, device):
    """Rows with equal entries: scope 0 / 1 give the first node in the plan's visiting order that attains the maximum,
    scope 2 the lowest node id."""
    b, plan, masks = hand
    N, B, W = b.batch.shape[0], b.num_graphs, 257
    gen = torch.Generator().manual_seed(9)
    _, h = _pitched(N, W, gen, device, ints=True)        # values in {0, 1, 2}: ties in nearly every (graph, column)
    gout = torch.randn(B, W + COL0, generator=gen).to(device)
    lib = _lib.load()
    new = [torch.zeros(N, W, device=device) for _ in range(3)]
    arr = (_lib.PoolBwdJob * 3)(*[_lib.PoolBwdJob(h.data_ptr(), new[s].data_ptr(), h.stride(0), W, W, s, _lib.POOL_MAX, COL0)
                                  for s in range(3)])
    assert lib.dagnn_readout_pool_backward_batch(C.byref(plan.desc), arr, 3, gout.data_ptr(), gout.stride(0), engine._stream(h)) == 0
    torch.cuda.synchronize()
    hc, gc = h.cpu().numpy(), gout.cpu().numpy()
    for d in range(2):
        want = _replay_backward(hc, gc[:, COL0:COL0 + W], visits[d], "max")
        assert np.array_equal(new[d].cpu().numpy().view(np.int32), want.view(np.int32)), d
        assert int((new[d] != 0).sum()) > 0
    want = np.zeros((N, W), dtype=np.float32)
    ptr = b.ptr.tolist()
    for g in range(B):
        first = ptr[g] + np.argmax(hc[ptr[g]:ptr[g + 1]], axis=0)     # (numpy: the FIRST of equal maxima)
        want[first, np.arange(W)] = gc[g, COL0:COL0 + W]
    assert np.array_equal(new[2].cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("n_jobs", [17, 24, 25])
def test_job_count_edges_against_the_host_replay(hand, visits, device, n_jobs):
    """17 jobs (more than 16), 24 (a full `MAX_READOUT_JOBS` launch) in one library call; 25 through the engine wrapper,
    which takes two chunks: forward and backward from zero, every job against the host replay bit for bit."""
    b, plan, masks = hand
    N, B, W = b.batch.shape[0], b.num_graphs, 4
    assert _lib.MAX_READOUT_JOBS == 24
    gen = torch.Generator().manual_seed(200 + n_jobs)
    cases = [CASES[k % len(CASES)] for k in range(n_jobs)]
    views = [_pitched(N, W, gen, device)[1] for _ in cases]
    ld_out = COL0 + n_jobs * W + 2
    out = torch.full((B, ld_out), -7.0, device=device)
    gout = torch.randn(B, ld_out, generator=gen).to(device)
    grads = [torch.zeros(N, W + 1, device=device) for _ in cases]
    if n_jobs > _lib.MAX_READOUT_JOBS:
        engine.readout_pool_batch(plan, [(h, scope, how, COL0 + k * W) for k, ((scope, how), h) in enumerate(zip(cases, views))], out)
        engine.readout_pool_backward_batch(plan, [(h, scope, how, COL0 + k * W, gh[:, :W])
                                                  for k, ((scope, how), h, gh) in enumerate(zip(cases, views, grads))], gout)
    else:
        fwd, bwd = (_lib.PoolJob * n_jobs)(), (_lib.PoolBwdJob * n_jobs)()
        for k, ((scope, how), h, gh) in enumerate(zip(cases, views, grads)):
            fwd[k] = _lib.PoolJob(h.data_ptr(), h.stride(0), W, scope, MODES[how], COL0 + k * W)
            bwd[k] = _lib.PoolBwdJob(h.data_ptr(), gh.data_ptr(), h.stride(0), gh.stride(0), W, scope, MODES[how], COL0 + k * W)
        lib = _lib.load()
        assert lib.dagnn_readout_pool_batch(C.byref(plan.desc), fwd, n_jobs, out.data_ptr(), ld_out, engine._stream(out)) == 0
        assert lib.dagnn_readout_pool_backward_batch(C.byref(plan.desc), bwd, n_jobs, gout.data_ptr(), ld_out, engine._stream(out)) == 0
    torch.cuda.synchronize()
    host, gc = np.full((B, ld_out), -7.0, dtype=np.float32), gout.cpu().numpy()
    for k, ((scope, how), h, gh) in enumerate(zip(cases, views, grads)):
        cols = slice(COL0 + k * W, COL0 + (k + 1) * W)
        host[:, cols] = _replay(h.cpu().numpy(), visits[scope], how)
        want = _replay_backward(h.cpu().numpy(), gc[:, cols], visits[scope], how)
        assert np.array_equal(gh[:, :W].cpu().numpy().view(np.int32), want.view(np.int32)), (k, scope, how)
        assert bool((gh[:, W:] == 0).all())
    assert np.array_equal(out.cpu().numpy().view(np.int32), host.view(np.int32))


def test_equal_grad_h_in_two_jobs_is_refused(hand, device):
    b, plan, masks = hand
    N, W = b.batch.shape[0], 4
    gh, gout = torch.zeros(N, W, device=device), torch.ones(b.num_graphs, 2 * W, device=device)
    arr = (_lib.PoolBwdJob * 2)(_lib.PoolBwdJob(None, gh.data_ptr(), 0, W, W, 0, _lib.POOL_ADD, 0),
                                _lib.PoolBwdJob(None, gh.data_ptr(), 0, W, W, 1, _lib.POOL_ADD, W))
    rc = _lib.load().dagnn_readout_pool_backward_batch(C.byref(plan.desc), arr, 2, gout.data_ptr(), 2 * W, engine._stream(gh))
    torch.cuda.synchronize()
    assert rc == EINVAL and not bool(gh.any())
    with pytest.raises(engine.DagnnHipError):
        engine.readout_pool_backward_batch(plan, [(None, 0, "add", 0, gh), (None, 1, "add", W, gh)], gout)


@pytest.mark.parametrize("how", ["max", "add", "mean"])
def test_pool_nodes_takes_row_pitched_views(hand, device, how):
    """`autograd.PoolNodes` on a [:, :8] view of a [N, 12] buffer (kept, not copied: `engine._rows`) and on an unaligned one
    (copied) against the float64 index pool: values and the gradient of a linear loss."""
    b, plan, masks = hand
    N, B = b.batch.shape[0], b.num_graphs
    gen = torch.Generator().manual_seed(3)
    for pitch, W in ((12, 8), (10, 7)):
        buf = torch.randn(N, pitch, generator=gen).to(device).requires_grad_(True)
        w = torch.randn(B, W, generator=gen)
        out = PoolNodes.apply(plan, buf[:, :W], 2, how)
        (out * w.to(device)).sum().backward()
        ref_in = buf.detach().double().cpu().requires_grad_(True)
        ref = _pool64(ref_in[:, :W], masks[2], b.batch, B, how)
        (ref * w.double()).sum().backward()
        bound = 9 * 2.0 ** -24 * _pool64(ref_in.detach()[:, :W].abs(), masks[2], b.batch, B, "add")   # (as in the forward test above)
        assert bool(((out.detach().double().cpu() - ref.detach()).abs() <= bound).all())
        assert float((buf.grad.double().cpu() - ref_in.grad).abs().max()) <= 2.4e-7 * float(ref_in.grad.abs().max())


# ============================================================================= model level
CONFIGS = [dict(out_wx=False, out_pool="mean"), dict(out_wx=False, out_pool="add", out_pool_all=True),
           dict(out_wx=False, out_pool="attn"), dict(out_wx=False, out_pool="mean", out_pool_all=True),
           dict(out_pool="attn", out_pool_all=True), dict(bidirectional=False, out_pool="mean"),
           dict(bidirectional=False, out_pool="add", out_wx=True), dict(bidirectional=False, out_pool="max", out_pool_all=True)]
FUSED_MAX = dict(out_wx=True, out_pool="max")   # (the configuration whose read-out was in HIP all along: the control)


def _code2_case(kw, agg="attn_h"):
    args = dict(w_edge_attr=True, num_layers=2, bidirectional=True, agg=agg, out_wx=False, out_pool_all=False, out_pool="max",
                dropout=0.0)
    args.update(kw)
    m = DAGNN(num_vocab=12, max_seq_len=3, emb_dim=32, hidden_dim=32, out_dim=None, encoder=ASTNodeEncoder(32, 98, 10030, 20),
              **args).eval()
    seeded_fill(m, 77)
    okw = dict(num_layers=2, bidirectional=args["bidirectional"], out_wx=args["out_wx"], out_pool_all=args["out_pool_all"],
               out_pool=args["out_pool"], max_seq_len=3)
    if agg != "attn_h":
        okw["agg"] = agg
    return m, args, okw


@pytest.fixture(scope="module")
def code2_data():
    b = synth.code2_batch(31, 9, 30)
    y = torch.randint(0, 12, (9, 3), generator=torch.Generator().manual_seed(31))
    return b, y


def _step(model, G, y):
    model.train()
    model.zero_grad(set_to_none=True)
    pred = model(G)
    loss = sum(torch.nn.functional.cross_entropy(p, y[:, s]) for s, p in enumerate(pred)) / len(pred)   # main_pyg.py:55-60
    loss.backward()
    return loss.detach()


def _no_sync_step(model, b, y, device):
    """forward + backward of one training step with every host synchronisation an error (batch and targets on the device
    beforehand; one warm-up step outside: library load, allocator, derived-weight caches)."""
    yd = y.to(device)
    _step(model, copy.deepcopy(b).to(device), yd)
    G = copy.deepcopy(b).to(device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = _step(model, G, yd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return loss


@pytest.mark.parametrize("kw", CONFIGS, ids=lambda kw: "-".join("%s=%s" % kv for kv in sorted(kw.items())))
def test_training_step_of_every_readout(device, code2_data, kw):
    """One training step per non-fused configuration of `test_out_wx_and_other_pools`: loss and every parameter gradient
    against float64 autograd through the oracle (a None gradient - `self_attn_linear_out` under P_ATTN, whose exact
    derivative is zero - counts as zeros), the read-out took the HIP path, the side effects on `G` have `_finish`'s
    shapes; and, for the bidirectional and the all-node configurations, forward + backward synchronise nowhere (the
    already-fused max configuration runs first under the same guard, as the control)."""
    b, y = code2_data
    model, args, okw = _code2_case(kw)
    loss_ref, ref = Hh.code2_grads64(None, model, b, y, **okw)
    model = model.to(device)
    G = copy.deepcopy(b).to(device)
    before = model.__dict__.get("readout_hip_passes", 0)
    loss = _step(model, G, y.to(device))
    model.check()
    assert model.__dict__.get("readout_hip_passes", 0) == before + 1
    assert abs(float(loss) - float(loss_ref)) < 1e-5, (float(loss), float(loss_ref))
    worst = Hh.check_grads_full(model, ref)
    print("%s: loss err %.3g, worst gradient error %.3g of its scale (%s)" % (kw, abs(float(loss) - float(loss_ref)), *worst))
    if args["out_pool"] == "attn":
        assert model.self_attn_linear_out.weight.grad is None and model.self_attn_linear_out.bias.grad is None
    if args["bidirectional"] and not args["out_pool_all"]:
        assert isinstance(G.h, list) and G.h[1][1].shape == (b.x.shape[0], 32) and not G.h[0][0].requires_grad
    else:
        rows = b.x.shape[0] if args["out_pool_all"] else int((b._bi_layer_idx1 == 0).sum())
        assert G.h.shape == (rows, model.out_hidden_dim) and G.batch.shape[0] == rows and not G.h.requires_grad
    if args["bidirectional"] or args["out_pool_all"]:
        control = _code2_case(FUSED_MAX)[0].to(device)
        _no_sync_step(control, b, y, device)
        again = _no_sync_step(model, b, y, device)
        assert torch.equal(again, loss)    # (the same step: no atomics anywhere in it)


def test_variant_trains_through_pool_nodes(device, code2_data):
    """`gated_sum` (csrc/variants_bwd.hip) with mean-pooling over all nodes: the HIP training branch hands its plan to
    `_finish`, which pools through `PoolNodes`; the torch backend stays on torch ops."""
    b, y = code2_data
    kw = dict(out_pool="mean", out_pool_all=True)
    model, args, okw = _code2_case(kw, agg="gated_sum")
    loss_ref, ref = Hh.code2_grads64(None, model, b, y, **okw)
    model = model.to(device)
    loss = _step(model, copy.deepcopy(b).to(device), y.to(device))
    assert model.__dict__.get("readout_hip_passes", 0) == 1
    assert abs(float(loss) - float(loss_ref)) < 1e-5, (float(loss), float(loss_ref))
    print("gated_sum mean all: worst gradient error %.3g of its scale (%s)" % Hh.check_grads_full(model, ref))
    model.variant_backend = "torch"
    _step(model, copy.deepcopy(b).to(device), y.to(device))
    assert model.__dict__.get("readout_hip_passes", 0) == 1


@pytest.mark.parametrize("pool", ["max", "mean", "add"])
@pytest.mark.parametrize("kind", ["na", "bn"])
def test_dvae_encoders_pool_all_nodes_through_pool_nodes(device, monkeypatch, kind, pool):
    """`DAGNN_NA` / `DAGNN_BN` with `out_pool_all`: gradients of <mu, r1> + <logvar, r2> against float64 autograd through
    the oracle, pooled by `PoolNodes` (counted here: the class has no path counter of its own)."""
    bidir = kind == "bn"
    model, nn_ = Hh.dvae_model(dict(kind=kind, hs=32, L=2, bidir=bidir, out_pool_all=True, out_pool=pool, w_seed=900))
    B = 4
    rows = synth.enas_rows(11, B) if kind == "na" else synth.bn_rows(12, B)
    G = synth.dvae_batch([(synth.decode_enas_row if kind == "na" else synth.decode_bn_row)(r) for r in rows])
    gen = torch.Generator().manual_seed(B)
    r1, r2 = torch.randn(B, 56, generator=gen), torch.randn(B, 56, generator=gen)
    loss_ref, ref = Hh.dvae_grads64(None, model, G, r1, r2, num_layers=2, bidirectional=bidir, num_nodes=nn_, vids=kind == "na",
                                    out_pool_all=True, out_pool=pool)
    calls = []
    real = PoolNodes.apply
    monkeypatch.setattr(PoolNodes, "apply", lambda *a: (calls.append(a[2:]), real(*a))[1])
    model = model.to(device).train()
    model.zero_grad(set_to_none=True)
    Hg = model(G.clone().to(device))
    loss = (model.fc1(Hg) * r1.to(device)).sum() + (model.fc2(Hg) * r2.to(device)).sum()
    loss.backward()
    loss = loss.detach()
    assert calls == [(2, pool)]
    assert abs(float(loss) - float(loss_ref)) < 1e-4 * max(1.0, abs(float(loss_ref))), (float(loss), float(loss_ref))
    print("%s %s: worst gradient error %.3g of its scale (%s)" % ((kind, pool) + Hh.check_grads_full(model, ref)))
