"""The ogbg-code2 LP task on the GPU (-m gpu): the two-table node encoder through every path of `DAGNN`, the three kernels of
csrc/lp.hip against their numpy mirrors / float64, and `evaluate_lp`, against fixtures generated from the reference
(tests/golden/make_golden_code2_lp.py).

Bounds.  Encoder: one fp32 add, 1 ulp.  Table gradients: a sum of `count` fp32 terms in any order, (count - 1) u / (1 - (count -
1) u) x sum |terms| with u = 2^-24.  Class loss: the units of DESIGN.md 4i (`dagnn_class_ce` is `dagnn_seq_ce`'s arithmetic
with S = 1), 4 x the error torch's own fp32 kernels show against float64 on the same GPU over all cases of this file.  Logits
1e-4, tokens outside the TAU = 2e-4 margin, gradients as the existing gradient-fixture tests of the same code path."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dagnn_amd import ASTNodeEncoder, ASTNodeEncoder2, ClassAccuracy, engine, lp, variants
from dagnn_amd import _lib as L
from tests import helpers as Hh
from tests.test_code2_lp_cpu import MODELS, lp_model, row_lse_loss64

pytestmark = pytest.mark.gpu
TAU, TOL = 2e-4, 1e-4
U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
EINVAL = -22
NAN = float("nan")


def _sync_count(fn):
    """Synchronisations torch reports while fn runs (blocking copies and reads of device values)."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, sum("synchroniz" in str(x.message) for x in w)


# ============================================================================= 1. the node encoder
def _enc_case(N, H, device, seed=0):
    g = torch.Generator().manual_seed(1000 * N + H + seed)
    tabs = [torch.randn(r, H, generator=g) for r in (9, 31, 6)]
    x = torch.stack([torch.randint(0, 9, (N,), generator=g), torch.randint(0, 31, (N,), generator=g)], 1)
    depth = torch.randint(0, 11, (N,), generator=g)   # max_depth 5: about half are clamped
    return tabs, x, depth


@pytest.mark.parametrize("H", [8, 300])
@pytest.mark.parametrize("N", [1, 63, 257])
def test_two_table_encoder_kernel(device, N, H):
    """Raw `dagnn_encode_ast` with a NULL depth table into NaN-filled rows of pitch H + 4 followed by sentinel words."""
    (tw, aw, _), x, depth = _enc_case(N, H, device)
    ld = H + 4
    whole = torch.full((N * ld + 64,), NAN, device=device)
    whole[N * ld:] = -7.0
    d_dev, x_dev, tw_d, aw_d = depth.to(device), x.to(device), tw.to(device), aw.to(device)
    rc = L.load().dagnn_encode_ast(x_dev.data_ptr(), d_dev.data_ptr(), tw_d.data_ptr(), aw_d.data_ptr(), None, 5,
                                   whole.data_ptr(), ld, N, H, engine._stream(whole))
    assert rc == 0
    out = whole[:N * ld].view(N, ld).cpu()
    want = tw.double()[x[:, 0]] + aw.double()[x[:, 1]]
    err = (out[:, :H].double() - want).abs()
    assert bool((err <= 2 * U * want.abs() + FLT_MIN).all()), float(err.max())     # 1 ulp of the result
    assert torch.equal(out[:, :H], tw[x[:, 0]] + aw[x[:, 1]])                      # ... in fact the one fp32 add, bit for bit
    assert bool(torch.isnan(out[:, H:]).all()) and bool((whole[N * ld:] == -7.0).all())
    assert torch.equal(d_dev.cpu(), depth.clamp(max=5))
    # the module's paths: no-grad kernel, and the kernel under autograd
    enc = ASTNodeEncoder2(H, 9, 31, 5).to(device)
    with torch.no_grad():
        enc.type_encoder.weight.copy_(tw)
        enc.attribute_encoder.weight.copy_(aw)
        d2 = depth.to(device)
        assert torch.equal(enc(x_dev, d2).cpu(), out[:, :H]) and torch.equal(d2.cpu(), depth.clamp(max=5))
    d3 = depth.to(device)
    y = enc(x_dev, d3)
    assert y.requires_grad and torch.equal(y.detach().cpu(), out[:, :H]) and torch.equal(d3.cpu(), depth.clamp(max=5))


@pytest.mark.parametrize("H", [8, 300])
@pytest.mark.parametrize("N", [1, 63, 257])
def test_two_table_encoder_gradients(device, N, H):
    (tw, aw, _), x, depth = _enc_case(N, H, device, seed=7)
    enc = ASTNodeEncoder2(H, 9, 31, 5).to(device)
    g = torch.randn(N, H, generator=torch.Generator().manual_seed(N + H))
    enc(x.to(device), depth.to(device)).backward(g.to(device))
    assert sorted(k for k, p in enc.named_parameters() if p.grad is not None) == ["attribute_encoder.weight", "type_encoder.weight"]
    for col, p, rows in ((0, enc.type_encoder.weight, 9), (1, enc.attribute_encoder.weight, 31)):
        want = torch.zeros(rows, H, dtype=torch.float64).index_add_(0, x[:, col], g.double())
        sumabs = torch.zeros(rows, H, dtype=torch.float64).index_add_(0, x[:, col], g.double().abs())
        count = torch.bincount(x[:, col], minlength=rows).double().view(-1, 1)
        n1 = (count - 1).clamp(min=0)
        bound = n1 * U / (1 - n1 * U) * sumabs
        err = (p.grad.cpu().double() - want).abs()
        assert bool((err <= bound + FLT_MIN).all()), (col, float((err - bound).max()))


@pytest.mark.parametrize("H", [8, 300])
@pytest.mark.parametrize("N", [1, 63, 257])
def test_three_table_encoder_is_bitwise_what_it_was(device, N, H):
    """(type + attr) + depth in fp32, in that order: the kernel's bits are those of the same two IEEE adds on the host."""
    (tw, aw, dw), x, depth = _enc_case(N, H, device, seed=3)
    enc = ASTNodeEncoder(H, 9, 31, 5).to(device)
    with torch.no_grad():
        for p, w in zip((enc.type_encoder.weight, enc.attribute_encoder.weight, enc.depth_encoder.weight), (tw, aw, dw)):
            p.copy_(w)
        d_dev = depth.to(device)
        out = enc(x.to(device), d_dev)
    dc = depth.clamp(max=5)
    assert torch.equal(out.cpu(), (tw[x[:, 0]] + aw[x[:, 1]]) + dw[dc]) and torch.equal(d_dev.cpu(), dc)
    d_dev = depth.to(device)
    out2 = enc(x.to(device), d_dev)    # under autograd
    assert torch.equal(out2.detach(), out)
    out2.sum().backward()
    assert enc.depth_encoder.weight.grad is not None
    assert torch.equal(enc.depth_encoder.weight.grad.cpu(), torch.bincount(dc, minlength=6).float().view(-1, 1).expand(6, H))


@pytest.mark.parametrize("B,mean_n,groups", [(20, 30, 0), (128, 125, 4)])   # a small batch's separate calls / the fused launches
def test_fused_prepare_two_tables_equals_the_encoder_kernel(device, B, mean_n, groups):
    """The `enc=` stage of `dagnn_prepare` with one two-table set and one three-table set against `dagnn_encode_ast`."""
    from dagnn_amd import synth
    b = synth.code2_batch(3, B, mean_n)
    N = b.x.shape[0]
    dev = lambda t: t.to(device)   # noqa: E731
    gen = torch.Generator().manual_seed(5)
    t2 = [dev(torch.randn(r, 64, generator=gen)) for r in (98, 300)] + [None]
    t3 = [dev(torch.randn(r, 192, generator=gen)) for r in (98, 300, 21)]
    x = dev(torch.stack([torch.randint(0, 98, (N,), generator=gen), torch.randint(0, 300, (N,), generator=gen)], 1))
    depth0 = torch.randint(0, 40, (N,), generator=gen)
    plan = engine.build_plan(dev(b.edge_index), dev(b._bi_layer_idx0), dev(b._bi_layer_idx1), dev(b.batch), B, dev(b.edge_attr),
                             launch=False)
    outs = [torch.full((N, 64), NAN, device=device), torch.full((N, 192), NAN, device=device)]
    d1 = dev(depth0.clone())
    plan.launch_prepare(groups, enc=(x, d1, 20, [(*t2, outs[0]), (*t3, outs[1])]))
    d2 = dev(depth0.clone())
    assert torch.equal(outs[0], engine.encode_ast(x, d2, *t2, 20)) and torch.equal(outs[1], engine.encode_ast(x, d2, *t3, 20))
    assert torch.equal(d1, d2) and int(d1.max()) == 20


# ============================================================================= 2. the model
def _no_torch_path(monkeypatch):
    calls = []
    monkeypatch.setattr(variants, "warn_torch_path", lambda *a, **k: calls.append(1))
    return calls


@pytest.mark.parametrize("name", MODELS)
def test_lp_model_evaluation_matches_the_reference(device, name, monkeypatch):
    monkeypatch.setenv("DAGNN_AMD_SCHEDULE", "lockstep")
    torch_path = _no_torch_path(monkeypatch)
    prepared = []
    orig = engine.PlanHandle.launch_prepare

    def spy(self, groups=0, enc=None, stack=None):
        prepared.append(None if enc is None else [t[2] is None for t in enc[3]])
        return orig(self, groups, enc=enc, stack=stack)
    monkeypatch.setattr(engine.PlanHandle, "launch_prepare", spy)
    meta, arr = Hh.load(name)
    model = lp_model(meta).to(device)
    G = Hh.code2_batch(arr, device)
    with torch.no_grad():
        out = model(G)
    assert tuple(out.shape) == arr["pred"].shape and Hh.maxdiff(out, arr["pred"]) < TOL
    assert Hh.maxdiff(G.x[arr["rows"]], arr["x_emb"]) < 1e-6
    assert np.array_equal(G.node_depth.cpu().numpy(), arr["node_depth_after"])
    assert tuple(G.bi_layer_index.shape) == (2, 2, arr["x"].shape[0])
    if name == "code2_lp_attn_h32_bidir":
        # the tuned main path: ONE fused front carrying the embedding rows and the folded gi0 rows of both directions,
        # every set without a depth table; the fold ran (what the existing fused-path tests observe)
        assert model._hip_supported() and engine.PREPARE_FUSED and engine.FOLD_INPUT
        assert prepared == [[True, True, True]] and model.__dict__.get("fold_passes", 0) == 1
    else:
        assert not model._hip_supported()   # the constructor-string variants' route (variants.run_hip)
    tok, top = model.predict(Hh.code2_batch(arr, device), return_top=True)
    tok = tok.cpu().numpy()
    assert tok.shape == (meta["B"], 1) and tok.dtype == np.int64
    clear = arr["top_val"][:, 0] - arr["top_val"][:, 1] > TAU
    assert int((~clear).sum()) <= 0.02 * meta["B"]
    assert np.array_equal(tok[clear], arr["tok"][clear])
    stray = (tok[:, 0] != arr["top_col"][:, 0]) & (tok[:, 0] != arr["top_col"][:, 1])
    assert not stray[~clear].any()
    assert Hh.maxdiff(top[:, 0, :], arr["top_val"][:, :2]) < TOL
    assert not torch_path
    model.check()


@pytest.mark.parametrize("name", MODELS)
def test_lp_training_step_gradients_match_the_reference(device, name, monkeypatch):
    """forward + `class_cross_entropy` + `loss.backward()` against the reference's own autograd on the same seeded step, with the
    tolerances of the existing gradient-fixture tests of the same code path (tests/test_gpu_parity.py: the variants'
    fixtures for `gated_sum`, the main path's for `attn_h`)."""
    torch_path = _no_torch_path(monkeypatch)
    lib = engine._lib.load()
    swept = []
    orig = lib.dagnn_variant_backward_run

    class _Spy(object):
        def __call__(self, *a):
            swept.append(1)
            return orig(*a)
    monkeypatch.setattr(lib, "dagnn_variant_backward_run", _Spy(), raising=False)
    meta, arr = Hh.load(name)
    model = lp_model(meta).to(device).train()
    G = Hh.code2_batch(arr, device)
    targ = lp.lp_targets(G)
    assert np.array_equal(targ.cpu().numpy(), arr["len_longest_path"].astype(np.int64))
    model.zero_grad(set_to_none=True)
    pred = model(G)
    loss = lp.class_cross_entropy(pred, torch.from_numpy(arr["len_longest_path"]).to(device))   # (float, as the reference holds it)
    loss.backward()
    grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad) for k, p in model.named_parameters()}
    assert not torch_path
    assert Hh.maxdiff(pred, arr["pred"]) < TOL
    print("%s: loss %.7f reference %.7f" % (name, float(loss.detach()), float(arr["loss"])))
    loss = loss.detach()
    assert abs(float(loss) - float(arr["loss"])) < 1e-5
    assert abs(float(loss) - row_lse_loss64(pred.detach().cpu().numpy(), arr["len_longest_path"])) < 1e-5   # (the float64 oracle on OUR logits)
    worst = Hh.check_grads(meta, arr, grads, rtol=1e-4)
    print("%s: worst relative gradient error %.3e" % (name, worst))
    if meta["agg"] == "gated_sum":
        assert swept, "the variant's training step did not go through the HIP reverse sweep"
        assert worst < 5e-3
    else:
        assert not swept and worst < 1e-4


# ============================================================================= 3. dagnn_graph_depth
def _chains(sizes):
    layer = torch.cat([torch.arange(n) for n in sizes]) if sizes else torch.zeros(0, dtype=torch.int64)
    batch = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(sizes)]) if sizes else torch.zeros(0, dtype=torch.int64)
    return layer, batch


def _depth_cases():
    big_first = torch.randint(0, 500, (1100,), generator=torch.Generator().manual_seed(1))
    big_first[0] = 900
    big_last = big_first.clone()
    big_last[0], big_last[-1] = 3, 901
    zeros = torch.zeros(1100, dtype=torch.int64)
    return {"one_node": (*_chains([1]), 1, [0]),
            "chains": (*_chains([1, 2, 70]), 3, [0, 1, 69]),
            "max_first": (big_first, zeros, 1, [900]),
            "max_last": (big_last, zeros, 1, [901]),
            "many_graphs": (torch.zeros(300, dtype=torch.int64), torch.arange(300), 300, [0] * 300),
            "trailing_empty": (*_chains([3, 5]), 4, [2, 4, 0, 0]),
            "middle_empty": (torch.tensor([4, 1, 7]), torch.tensor([0, 0, 2]), 3, [4, 0, 7])}


@pytest.mark.parametrize("case", sorted(_depth_cases()))
def test_graph_depth(device, case):
    layer, batch, B, want = _depth_cases()[case]
    host = lp.graph_depth_host(layer, batch, B)
    assert host.tolist() == want
    G = SimpleNamespace(_bi_layer_idx0=layer.to(device), batch=batch.to(device))
    (a, b), syncs = _sync_count(lambda: (engine.graph_depth(G._bi_layer_idx0, G.batch, B), lp.lp_targets(G, B)))
    assert syncs == 0                                  # no host read of B, nothing waits
    assert a.dtype == torch.int64 and a.device.type == "cuda"
    assert np.array_equal(a.cpu().numpy(), host) and torch.equal(a, b)


def test_graph_depth_refuses_bad_arguments(device):
    lib = L.load()
    t = torch.zeros(8, dtype=torch.int64, device=device)
    p, st = t.data_ptr(), engine._stream(t)
    assert lib.dagnn_graph_depth(p, p, -1, 1, p, st) == EINVAL and lib.dagnn_graph_depth(p, p, 4, 1, None, st) == EINVAL
    assert lib.dagnn_graph_depth(None, p, 4, 1, p, st) == EINVAL and lib.dagnn_graph_depth(None, None, 0, 0, None, st) == 0


# ============================================================================= 4. class_cross_entropy
CE_C = [1, 2, 24, 275, 1030]
CE_B = [1, 5, 257]


def _ce_case(B, C, device):
    g = torch.Generator().manual_seed(1000 * B + C)
    x = torch.randn(B, C, generator=g) * (1.0 if C % 2 else 8.0)   # (even widths: peaked rows)
    y = torch.randint(0, C, (B,), generator=g)
    return x.to(device), y.to(device)


class _Ce64(object):
    """float64 softmax / log-softmax per row of fp32 logits and the error units of DESIGN.md 4i for the kernel's arithmetic:
    an entry of softmax - onehot carries u (|x_j - max| + c) p_j (+ u on the target, + the smallest normal in units of
    B x d logits), a row loss u (|loss| + c), with c = ceil(C / 256) + 6 + 2 + 5 (the thread's chain, the shuffle levels,
    the adds across waves, exp / reciprocal / two products / the scale)."""

    def __init__(self, x, y):
        B, C = x.shape
        x64 = x.double()
        self.p = torch.softmax(x64, -1)
        self.onehot = torch.zeros_like(self.p).scatter_(1, y[:, None], 1.0)
        self.loss = -torch.log_softmax(x64, -1).gather(1, y[:, None])[:, 0]
        self.c = (C + 255) // 256 + 6 + 2 + 5
        spread = x64.amax(-1, keepdim=True) - x64
        self.d_unit = U * ((spread + self.c) * self.p + self.onehot) + FLT_MIN * B
        self.mean_unit = U * (float(self.loss.abs().mean()) + self.c)

    def d_ratio(self, d_times_b):
        return float(((d_times_b.double() - (self.p - self.onehot)).abs() / self.d_unit).max())

    def mean_ratio(self, loss):
        return abs(float(loss) - float(self.loss.mean())) / self.mean_unit


@pytest.fixture(scope="module")
def ce_torch_ratios(device):
    """The error of torch's own fp32 `softmax` / `cross_entropy` on this GPU against float64 in `_Ce64`'s units, the largest
    over every case of this file (the reasons for the largest and not case by case: tests/test_train_tail_gpu.py)."""
    worst = {"d": 0.0, "mean": 0.0}
    for B in CE_B:
        for C in CE_C:
            x, y = _ce_case(B, C, device)
            ref = _Ce64(x, y)
            worst["d"] = max(worst["d"], ref.d_ratio(torch.softmax(x, -1) - ref.onehot.float()))
            worst["mean"] = max(worst["mean"], ref.mean_ratio(torch.nn.functional.cross_entropy(x, y)))
    print("torch fp32 against float64: softmax - onehot %.3f, mean loss %.3f units" % (worst["d"], worst["mean"]))
    assert all(0.0 < v < float("inf") for v in worst.values()), worst
    return worst


def _float_targets(y, kind):
    """Targets as the reference holds them: floats that truncate TOWARD ZERO to y (class 0 from -0.5 as well)."""
    t = y.to(kind) + 0.75
    t[y == 0] = -0.5
    return t


@pytest.mark.parametrize("C", CE_C)
@pytest.mark.parametrize("B", CE_B)
def test_class_cross_entropy_matches_float64(device, ce_torch_ratios, B, C):
    x, y = _ce_case(B, C, device)
    ref = _Ce64(x, y)
    seen = {}
    for kind, targ in (("int64", y), ("float32", _float_targets(y, torch.float32)), ("float64", _float_targets(y, torch.float64)),
                       ("column", y.view(-1, 1))):
        leaf = x.clone().requires_grad_(True)
        pred = leaf * 1.0
        grads = []
        pred.register_hook(grads.append)
        loss = lp.class_cross_entropy(pred, targ)
        loss.backward()
        g, = grads
        rd, rm = ref.d_ratio(g * float(B)), ref.mean_ratio(loss.detach())
        print("B %d C %d %s: d %.3f mean %.3f units (torch's worst: %.3f, %.3f)" % (B, C, kind, rd, rm, ce_torch_ratios["d"], ce_torch_ratios["mean"]))
        assert rd <= 4 * ce_torch_ratios["d"] and rm <= 4 * ce_torch_ratios["mean"]
        assert g.shape == (B, C) and g.stride(1) == 1 and g.stride(0) % 4 == 0 and g.stride(0) >= C   # `_HeadsLinear.backward`'s pitch
        seen[kind] = (loss.detach().clone(), g.clone())
        with torch.no_grad():
            assert torch.equal(lp.class_cross_entropy(x, targ), loss.detach())    # without d logits: the same bits
    for kind in seen:   # every target form, and a second run: bitwise equal
        assert torch.equal(seen[kind][0], seen["int64"][0]) and torch.equal(seen[kind][1], seen["int64"][1]), kind
    if C == 1:
        assert float(seen["int64"][0]) == 0.0 and bool((seen["int64"][1] == 0).all())


@pytest.mark.parametrize("B,C", [(5, 24), (257, 275), (3, 1030)])
def test_class_ce_raw_padding_and_bad_targets(device, ce_torch_ratios, B, C):
    """Raw `dagnn_class_ce`: logits in rows of pitch C + 5, d logits into NaN-filled rows of pitch C + 3 (a 4-float pitch when
    the wrapper allocates: above) with sentinel words behind; then one target outside [0, C) of every kind."""
    lib = L.load()
    x, y = _ce_case(B, C, device)
    ref = _Ce64(x, y)
    xp = torch.full((B, C + 5), 1e30, device=device)
    xp[:, :C] = x
    st = engine._stream(x)
    counter = torch.zeros(1, dtype=torch.int32, device=device)

    def call(targ, kind):
        whole = torch.full((B * (C + 3) + 64,), NAN, device=device)
        whole[B * (C + 3):] = -7.0
        row = torch.full((B + 16,), -7.0, device=device)
        loss = torch.full((17,), -7.0, device=device)
        rc = lib.dagnn_class_ce(xp.data_ptr(), C + 5, targ.data_ptr(), kind, B, C, whole.data_ptr(), C + 3, row.data_ptr(),
                                loss.data_ptr(), counter.data_ptr(), st)
        assert rc == 0
        d = whole[:B * (C + 3)].view(B, C + 3)
        assert bool(torch.isnan(d[:, C:]).all()) and bool((whole[B * (C + 3):] == -7.0).all())
        assert bool((row[B:] == -7.0).all()) and bool((loss[1:] == -7.0).all())
        assert int(counter[0]) == 0
        return d[:, :C], row[:B], loss[0]
    d, row, loss = call(y, L.LP_INT64)
    assert ref.d_ratio(d * float(B)) <= 4 * ce_torch_ratios["d"] and ref.mean_ratio(loss) <= 4 * ce_torch_ratios["mean"]
    bad_row = B // 2
    for kind, dtype, bad in ((L.LP_INT64, torch.int64, -1), (L.LP_INT64, torch.int64, C), (L.LP_FLOAT32, torch.float32, float(C)),
                             (L.LP_FLOAT32, torch.float32, NAN), (L.LP_FLOAT64, torch.float64, -1.0), (L.LP_FLOAT64, torch.float64, 1e300)):
        t = y.to(dtype)
        t[bad_row] = bad
        d2, row2, loss2 = call(t, kind)
        others = torch.arange(B, device=device) != bad_row
        assert bool(torch.isnan(loss2)) and bool(torch.isnan(row2[bad_row])), (kind, bad)
        assert torch.equal(row2[others], row[others]) and torch.equal(d2[others], d[others])
    assert bool(torch.isnan(lp.class_cross_entropy(x, torch.full_like(y, C))))          # the documented contract, through the wrapper
    p = x.data_ptr()
    assert lib.dagnn_class_ce(p, C - 1, y.data_ptr(), 0, B, C, None, 0, p, p, counter.data_ptr(), st) == EINVAL
    assert lib.dagnn_class_ce(p, C, y.data_ptr(), 3, B, C, None, 0, p, p, counter.data_ptr(), st) == EINVAL
    assert lib.dagnn_class_ce(p, C, y.data_ptr(), 0, 0, C, None, 0, p, p, counter.data_ptr(), st) == EINVAL
    assert lib.dagnn_class_ce(p, C, None, 0, B, C, None, 0, p, p, counter.data_ptr(), st) == EINVAL


@pytest.mark.parametrize("B,C,D", [(5, 24, 64), (257, 275, 300)])
def test_class_cross_entropy_backward_through_the_head(device, B, C, D):
    """`loss.backward()` through `graph_pred_linear` against float64 autograd of the torch expression: each gradient within 4 x the
    error the same expression shows in fp32 on this GPU (`F.cross_entropy`), and `(3 loss).backward()` twice on one graph."""
    g = torch.Generator().manual_seed(B + C)
    out = torch.randn(B, D, generator=g).to(device)
    y = torch.randint(0, C, (B,), generator=g).to(device)
    lin = torch.nn.Linear(D, C).to(device)

    def grads(fn, dtype):
        m = torch.nn.Linear(D, C).to(device).to(dtype)
        m.load_state_dict({k: v.to(dtype) for k, v in lin.state_dict().items()})
        o = out.to(dtype).clone().requires_grad_(True)   # (a leaf of its own: `.to` of the same dtype is the same tensor)
        fn(m(o)).backward()
        return [t.double() for t in (m.weight.grad, m.bias.grad, o.grad)]
    ref = grads(lambda p: torch.nn.functional.cross_entropy(p, y), torch.float64)
    t32 = grads(lambda p: torch.nn.functional.cross_entropy(p, y), torch.float32)
    ours = grads(lambda p: lp.class_cross_entropy(p, _float_targets(y, torch.float32)), torch.float32)
    for r, t, o, what in zip(ref, t32, ours, ("weight", "bias", "input")):
        e_t, e_o = float((t - r).abs().max()), float((o - r).abs().max())
        print("B %d C %d d %s: ours %.3e torch fp32 %.3e (scale %.3e)" % (B, C, what, e_o, e_t, float(r.abs().max())))
        assert e_o <= 4 * e_t + FLT_MIN
    o = out.clone().requires_grad_(True)
    loss = 3.0 * lp.class_cross_entropy(lin(o), y)
    g1, = torch.autograd.grad(loss, o, retain_graph=True)
    g2, = torch.autograd.grad(loss, o)
    assert torch.equal(g1, g2)
    assert float((g1.double() - 3.0 * ref[2]).abs().max()) <= 3 * (4 * float((t32[2] - ref[2]).abs().max()) + U * float(ref[2].abs().max()))


def test_class_cross_entropy_takes_torch_for_anything_else(device):
    x, y = _ce_case(5, 24, device)
    want = torch.nn.functional.cross_entropy(x.double(), y)
    assert torch.equal(lp.class_cross_entropy(x.double(), y), want)                                      # not fp32
    assert torch.equal(lp.class_cross_entropy(x.cpu(), y.cpu().float() + 0.5), torch.nn.functional.cross_entropy(x.cpu(), y.cpu()))
    xt = x.t().contiguous().t()                                                                          # strided columns
    assert abs(float(lp.class_cross_entropy(xt, y)) - float(want)) < 1e-5


# ============================================================================= 5. dagnn_class_hits / ClassAccuracy
def _hits_case(B, C, device):
    g = torch.Generator().manual_seed(100 * B + C)
    logits = torch.randn(B, C, generator=g)
    targ = torch.randint(0, max(C, 2), (B,), generator=g).float()
    for b in range(0, B, 3):                      # ties: the maximum planted twice, the lowest column wins
        c0, c1 = sorted(torch.randint(0, C, (2,), generator=g).tolist())
        logits[b, c0] = logits[b, c1] = 50.0
        targ[b] = c0 if b % 2 == 0 else c1        # ... a target on the HIGHER column is a miss
    for b in range(1, B, 7):                      # a NaN logit beats everything, the first NaN wins
        c0, c1 = sorted(torch.randint(0, C, (2,), generator=g).tolist())
        logits[b, c0] = logits[b, c1] = NAN
        targ[b] = c0
    targ[2::11] = NAN                             # unlabelled
    targ[5::13] += 0.5                            # matches nothing
    return logits.to(device), targ.to(device)


@pytest.mark.parametrize("C", [1, 275])
@pytest.mark.parametrize("B", [1, 65, 1025])
def test_class_hits_forms_agree(device, B, C):
    logits, targ = _hits_case(B, C, device)
    host = lp.class_hits_host(logits, targ)
    tok = torch.from_numpy(np.where(np.isnan(logits.cpu().numpy()).any(1), np.isnan(logits.cpu().numpy()).argmax(1),
                                    np.nan_to_num(logits.cpu().numpy(), nan=-np.inf).argmax(1))).to(device)
    assert torch.equal(tok, engine.rows_argmax(logits, 1, C)[:, 0])      # (predict.hip's order is the mirror's order)
    got = {}
    for form, pred, t in (("logits", logits, targ), ("tok", tok, targ), ("tok_col", tok.view(-1, 1), targ.view(-1, 1)),
                          ("f64", logits, targ.double()), ("pitched", torch.cat([logits, logits], 1)[:, :C], targ)):
        out, syncs = _sync_count(lambda: engine.class_hits(pred, t))
        assert syncs == 0 and out.dtype == torch.int64 and tuple(out.shape) == (2,)
        got[form] = out.cpu().numpy()
        assert np.array_equal(got[form], host), (form, got[form], host)
        assert np.array_equal(lp.class_hits_host(pred, t), host), form
        assert torch.equal(engine.class_hits(pred, t), out)               # a second run
    lab = ~torch.isnan(targ)
    ti = targ[lab].long()                          # integer targets: every graph labelled, compared as integers
    want = np.array([int((tok[lab] == ti).sum()), int(lab.sum())])
    if int(lab.sum()):
        assert np.array_equal(engine.class_hits(tok[lab], ti).cpu().numpy(), want)
        assert np.array_equal(engine.class_hits(logits[lab], ti).cpu().numpy(), want)


def test_class_hits_refuses_bad_arguments(device):
    lib = L.load()
    t = torch.zeros(64, dtype=torch.int64, device=device)
    cnt = torch.zeros(1, dtype=torch.int32, device=device)
    p, st = t.data_ptr(), engine._stream(t)
    call = lambda logits=p, ld=4, tok=None, B=2, C=4, kind=0, work=p + 256, nbytes=16: lib.dagnn_class_hits(   # noqa: E731
        logits, ld, tok, B, C, p + 64, kind, work, nbytes, cnt.data_ptr(), p + 128, st)
    assert call() == 0 and call(logits=None, tok=p) == 0
    assert call(tok=p) == EINVAL and call(logits=None) == EINVAL and call(ld=3) == EINVAL and call(B=0) == EINVAL
    assert call(kind=5) == EINVAL and call(work=p + 260) == EINVAL and call(nbytes=8) == -28
    assert lib.dagnn_class_hits_bytes(1025, 1) == 17 * 16 and lib.dagnn_class_hits_bytes(1025, 0) == 5 * 16
    assert lib.dagnn_class_hits_bytes(-1, 1) == 0
    torch.cuda.synchronize(device)
    assert int(cnt[0]) == 0


@pytest.mark.parametrize("form", ["tok", "logits"])
def test_class_accuracy_is_the_evaluators_number_exactly(device, form):
    meta, arr = Hh.load("code2_lp_acc")
    tok, targ = torch.from_numpy(arr["tok"]).to(device), torch.from_numpy(arr["targ"]).to(device)
    C = meta["num_class"]
    if form == "logits":
        pred = torch.rand(tok.shape[0], C, generator=torch.Generator().manual_seed(1)).to(device)
        pred[torch.arange(tok.shape[0], device=device), tok] = 2.0
    else:
        pred = tok
    metric = ClassAccuracy()

    def run():
        o = 0
        for n in meta["splits"]:
            metric.update(pred[o:o + n], targ[o:o + n])
            o += n
    _, syncs = _sync_count(run)
    assert syncs == 0                                  # nothing synchronises in `update`
    counts = metric.counts()
    assert counts.shape == (len(meta["splits"]), 2) and counts[3].tolist()[0] == 0 and counts[3, 1] > 0
    res = metric.compute()
    assert res["n"] == meta["labelled"] and int(counts[:, 0].sum()) == meta["hits"]
    assert res["acc"] == float(arr["acc"])
    metric.reset()
    with pytest.raises(ValueError):
        metric.compute()


# ============================================================================= 6. evaluate_lp
def _graph_range(arr, g0, g1, device):
    """The graphs [g0, g1) of a fixture's batch as a batch of their own."""
    batch = arr["batch"]
    nodes = np.flatnonzero((batch >= g0) & (batch < g1))
    n0 = int(nodes[0])
    edges = np.flatnonzero((batch[arr["edge_index"][0]] >= g0) & (batch[arr["edge_index"][0]] < g1))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    ids = torch.arange(len(nodes), device=device)
    return SimpleNamespace(x=t(arr["x"][nodes]), node_depth=t(arr["node_depth"][nodes]), edge_index=t(arr["edge_index"][:, edges] - n0),
                           edge_attr=t(arr["edge_attr"][edges]), batch=t(batch[nodes] - g0), _bi_layer_idx0=t(arr["layer0"][nodes]),
                           _bi_layer_index0=ids, _bi_layer_idx1=t(arr["layer1"][nodes]), _bi_layer_index1=ids.clone(),
                           num_graphs=g1 - g0)


def test_evaluate_lp_on_a_split_batch(device):
    meta, arr = Hh.load("code2_lp_gated_h64")
    model = lp_model(meta).to(device).train()
    batches = [_graph_range(arr, 0, 5, device), _graph_range(arr, 5, 12, device)]
    res = lp.evaluate_lp(model, lp.lp_batches(batches, training=False))
    assert model.training                                                    # the mode is restored
    ambiguous = int((arr["top_val"][:, 0] - arr["top_val"][:, 1] <= TAU).sum())
    assert res["n"] == meta["B"] and abs(res["acc"] - float(arr["acc"])) <= ambiguous / meta["B"]
    model.eval()
    with_attr = [_graph_range(arr, 0, 5, device), _graph_range(arr, 5, 12, device)]
    with_attr[0].len_longest_path = torch.from_numpy(arr["len_longest_path"][:5]).to(device)   # the attribute, as the reader stores it
    with_attr[1].len_longest_path = torch.from_numpy(arr["len_longest_path"][5:])               # ... and still on the host
    assert lp.evaluate_lp(model, with_attr) == res and not model.training
    # every prediction wrong by construction: accuracy 0, not an error
    for b, lo in zip(with_attr, (0, 5)):
        b.__dict__.update(_graph_range(arr, lo, lo + b.num_graphs, device).__dict__)
        b.len_longest_path = torch.full((b.num_graphs,), 1000.0)
    assert lp.evaluate_lp(model, with_attr) == {"acc": 0.0, "n": meta["B"]}
