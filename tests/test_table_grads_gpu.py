"""`dagnn_table_grads` on the GPU (-m gpu): the kernels' bits against the host mirror of their summation order
(`autograd.table_grads_host`), the node encoders' backward with `engine.TABLE_GRADS` on, and whole training steps that are
then bitwise repeatable - `encoder.*` included - without torch's deterministic mode.

Bounds.  Kernel against mirror: `torch.equal`.  Against float64: the bound of the order (tests/test_table_grads.py).  Knob off:
the any-order bound of tests/test_code2_lp_gpu.py, (count - 1) u / (1 - (count - 1) u) x sum |terms|.  The gradient fixture: the
tolerance of `test_training_step_gradients_match_reference_golden`."""
import ctypes as C

import numpy as np
import pytest
import torch

from dagnn_amd import ASTNodeEncoder, ASTNodeEncoder2, engine, synth
from dagnn_amd import _lib as L
from dagnn_amd.autograd import table_grads_host
from tests import helpers as Hh
from tests.test_table_grads import FLT_MIN, U, order_bound, raw_call, refused_calls, skewed_keys, spread_gradients

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = -7.0
ROWS = (98, 10030, 21)


def _patterns(N, seed):
    """Key patterns of one call over the three tables of ROWS: name -> list of three int64 [N] host tensors (views allowed)."""
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64))   # noqa: E731
    pats = {
        "one key": [torch.full((N,), r, dtype=torch.int64) for r in (97, 4000, 0)],     # one row of N members
        "distinct": [t(np.arange(N) % R) if N > R else t(rng.permutation(R)[:N]) for R in ROWS],
        "skewed": [t(skewed_keys(N, R, seed + q)) for q, R in enumerate(ROWS)],
    }
    x = torch.stack([t(skewed_keys(N, ROWS[0], seed + 5, 0.3)), t(skewed_keys(N, ROWS[1], seed + 6))], 1)
    pats["columns"] = [x[:, 0], x[:, 1], t(rng.integers(0, ROWS[2], N))]                # two columns of one [N, 2] tensor
    foreign = [t(rng.integers(0, R, N)) for R in ROWS]
    for k, R in zip(foreign, ROWS):
        for at, bad in zip(rng.permutation(N)[:6], (-1, R, R + 5, -(1 << 40), 1 << 40, (1 << 32) + 3)):
            k[at] = bad
    pats["foreign"] = foreign
    return pats


def _run_raw(device, g_host, keys_host, rows, pad=4):
    """One raw call: g with row pitch H + pad, NaN-filled outputs of pitch H + pad whose pitch columns and tail hold GUARD.
    Returns the [R, H] outputs on the host after checking that the guards survived."""
    lib = L.load()
    N, H = g_host.shape
    gbuf = torch.full((max(N, 1), H + pad), NAN, device=device)
    g = gbuf[:N, :H]
    g.copy_(torch.from_numpy(g_host))
    keys = []
    for k in keys_host:   # a strided host view stays a strided device view
        base = k._base if k._base is not None else k
        keys.append(base.to(device).as_strided(k.shape, k.stride(), k.storage_offset()))
    wholes, tables = [], []
    for k, R in zip(keys, rows):
        whole = torch.full((R * (H + pad) + 64,), NAN, device=device)
        whole[:R * (H + pad)].view(R, H + pad)[:, H:] = GUARD
        whole[R * (H + pad):] = GUARD
        wholes.append(whole)
        tables.append((k.data_ptr() if N else None, k.stride(0) if N > 1 else 1, R, whole.data_ptr(), H + pad))
    nbytes = lib.dagnn_table_grads_workspace_bytes(N, H, (C.c_int64 * len(rows))(*rows), len(rows))
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=device)   # "any contents"
    rc = raw_call(g.data_ptr() if N else None, H + pad, N, H, tables, ws.data_ptr(), nbytes, stream=engine._stream(gbuf))
    assert rc == 0, rc
    outs = []
    for whole, R in zip(wholes, rows):
        body = whole[:R * (H + pad)].view(R, H + pad).cpu()
        assert bool((body[:, H:] == GUARD).all()) and bool((whole[R * (H + pad):] == GUARD).all())
        outs.append(body[:, :H].contiguous())
    return outs, keys, g


@pytest.mark.parametrize("H", [4, 64, 300])
@pytest.mark.parametrize("N", [0, 1, 31, 32, 33, 1025, 5000])
def test_kernels_equal_the_mirror_bit_for_bit(device, N, H):
    g_host = spread_gradients(N, H, 100 * N + H)
    for name, keys_host in _patterns(N, N + H).items():
        want = table_grads_host(g_host, keys_host, ROWS)
        got, keys, g = _run_raw(device, g_host, keys_host, ROWS)
        for t, (o, w, k, R) in enumerate(zip(got, want, keys_host, ROWS)):
            assert not bool(torch.isnan(o).any()), (name, t)
            assert torch.equal(o, torch.from_numpy(w)), (name, t, float((o - torch.from_numpy(w)).abs().max()))
            assert not bool(np.signbit(o.numpy()[np.bincount(k.numpy()[(k.numpy() >= 0) & (k.numpy() < R)], minlength=R) == 0]).any())
            exact, bound = order_bound(g_host, k.numpy(), R)
            err = np.abs(o.numpy().astype(np.float64) - exact)
            assert (err <= bound + FLT_MIN).all(), (name, t, float((err - bound).max()))
        if name in ("columns", "skewed"):   # the public wrapper: the same bits
            again = engine.table_grads(g, keys, ROWS)
            assert all(torch.equal(a.cpu(), o) for a, o in zip(again, got)), name
    # a table of one row
    one = [torch.zeros(N, dtype=torch.int64)]
    got, _, _ = _run_raw(device, g_host, one, (1,))
    assert torch.equal(got[0], torch.from_numpy(table_grads_host(g_host, one, (1,))[0]))


def test_the_kernels_order_is_the_chunked_one(device):
    """34 members 2^24, 31 zeros, 1, 1 give 2^24 + 2 (a strict sequential fp32 sum gives 2^24); 32 members give 2^24."""
    col = np.array([2.0 ** 24] + [0.0] * 31 + [1.0, 1.0], dtype=np.float32)
    out, _, _ = _run_raw(device, np.repeat(col[:, None], 8, 1), [torch.zeros(34, dtype=torch.int64)], (1,))
    assert bool((out[0] == 2.0 ** 24 + 2).all())
    col32 = np.array([2.0 ** 24] + [0.0] * 29 + [1.0, 1.0], dtype=np.float32)
    out, _, _ = _run_raw(device, np.repeat(col32[:, None], 8, 1), [torch.zeros(32, dtype=torch.int64)], (1,))
    assert bool((out[0] == 2.0 ** 24).all())


def test_stages_split_the_call_and_repeat_its_bits(device):
    """Index and sum launches apart over a kept workspace (what scripts/bench_table_grads.py times) give the bits of the whole
    call; more than three tables go in several calls."""
    N, H = 3000, 64
    g = torch.from_numpy(spread_gradients(N, H, 1)).to(device)
    keys = [torch.from_numpy(skewed_keys(N, R, 3 + q)).to(device) for q, R in enumerate(ROWS)]
    whole = engine.table_grads(g, keys, ROWS)
    nbytes = L.load().dagnn_table_grads_workspace_bytes(N, H, (C.c_int64 * 3)(*ROWS), 3)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    assert engine.table_grads(g, keys, ROWS, stages=L.TABLE_GRADS_INDEX, workspace=ws) is not None
    split = engine.table_grads(g, keys, ROWS, stages=L.TABLE_GRADS_SUM, workspace=ws)
    assert all(torch.equal(a, b) for a, b in zip(whole, split))
    five = engine.table_grads(g, keys + keys[:2], ROWS + ROWS[:2])
    assert len(five) == 5 and all(torch.equal(a, b) for a, b in zip(five, whole + whole[:2]))


def test_argument_errors_with_real_pointers(device):
    g = torch.zeros(100, 8, device=device)
    keys = torch.zeros(100, dtype=torch.int64, device=device)
    out = torch.zeros(9, 8, device=device)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=device)
    refused_calls(g.data_ptr(), keys.data_ptr(), out.data_ptr(), ws.data_ptr(), 1 << 20)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0   # nothing ran


# ============================================================================= the module path
def _enc_case(N, H, seed=0):
    gen = torch.Generator().manual_seed(1000 * N + H + seed)
    x = torch.stack([torch.randint(0, 9, (N,), generator=gen), torch.randint(0, 31, (N,), generator=gen)], 1)
    depth = torch.randint(0, 11, (N,), generator=gen)   # max_depth 5: about half are clamped
    g = torch.from_numpy(spread_gradients(N, H, 7 * N + H + seed))
    return x, depth, g


@pytest.mark.parametrize("three", [False, True])
@pytest.mark.parametrize("H", [8, 300])
@pytest.mark.parametrize("N", [1, 63, 257])
def test_encoder_gradients_equal_the_mirror_with_the_knob_on(device, monkeypatch, N, H, three):
    x, depth, g = _enc_case(N, H)
    enc = (ASTNodeEncoder if three else ASTNodeEncoder2)(H, 9, 31, 5).to(device)
    params = [enc.type_encoder.weight, enc.attribute_encoder.weight] + ([enc.depth_encoder.weight] if three else [])
    keys = [x[:, 0], x[:, 1]] + ([depth.clamp(max=5)] if three else [])
    rows = (9, 31, 6)[:len(keys)]
    calls = []
    orig = engine.table_grads
    monkeypatch.setattr(engine, "table_grads", lambda *a, **k: (calls.append(len(a[1])), orig(*a, **k))[1])
    monkeypatch.setattr(engine, "TABLE_GRADS", 1)
    enc(x.to(device), depth.to(device)).backward(g.to(device))
    assert calls == [len(keys)]                                       # one call for all tables
    want = table_grads_host(g, keys, rows)
    for p, w in zip(params, want):
        assert torch.equal(p.grad.cpu(), torch.from_numpy(w))
    # knob off: what it was - torch's index_add_, any order
    monkeypatch.setattr(engine, "TABLE_GRADS", 0)
    enc.zero_grad(set_to_none=True)
    enc(x.to(device), depth.to(device)).backward(g.to(device))
    assert calls == [len(keys)]
    for p, k, R in zip(params, keys, rows):
        exact = torch.zeros(R, H, dtype=torch.float64).index_add_(0, k, g.double())
        sumabs = torch.zeros(R, H, dtype=torch.float64).index_add_(0, k, g.double().abs())
        n1 = (torch.bincount(k, minlength=R).double().view(-1, 1) - 1).clamp(min=0)
        bound = n1 * U / (1 - n1 * U) * sumabs
        err = (p.grad.cpu().double() - exact).abs()
        assert bool((err <= bound + FLT_MIN).all()), float((err - bound).max())


# ============================================================================= the training step
@pytest.mark.parametrize("H,L_,B,mean_n", [(64, 3, 6, 30), (256, 2, 128, 125)])
def test_training_step_is_bitwise_repeatable_with_the_knob_on(device, monkeypatch, H, L_, B, mean_n):
    """Two steps from the same state, then the same with the other workgroup placement of the dataflow kernels: the loss and
    every gradient, `encoder.*` included, bit for bit.  torch's deterministic mode stays off: this is the library's own order."""
    from tests.test_gpu_parity import _headline_model, _train_step
    assert not torch.are_deterministic_algorithms_enabled()
    monkeypatch.setattr(engine, "TABLE_GRADS", 1)
    model = _headline_model(H=H, L=L_, V=32, seed=4).to(device)
    b = synth.code2_batch(11, B, mean_n)
    y = torch.randint(0, 32, (B, 5), generator=torch.Generator().manual_seed(3)).to(device)
    runs = []
    for mode in (1, 1, 0, 0):
        monkeypatch.setattr(engine, "DF_XCD", mode)
        loss, grads = _train_step(model, b.clone().to(device), y)
        model.check()
        runs.append((loss.clone(), {k: v.clone() for k, v in grads.items()}))
    assert any("encoder." in k for k in runs[0][1])
    for loss, grads in runs[1:]:
        assert torch.equal(loss, runs[0][0])
        for k, v in grads.items():
            assert torch.equal(v, runs[0][1][k]), k
    # ... and the tables' gradients are the mirror's bits of what reached the encoder (the headline shape is checked on the
    # small batch's terms only: the order does not depend on the shape)
    if B == 6:
        enc = model.encoder
        G = b.clone().to(device)
        depth = G.node_depth.view(-1).clone()
        out = enc(G.x, depth)
        gin = torch.from_numpy(spread_gradients(out.shape[0], H, 2)).to(device)
        enc.zero_grad(set_to_none=True)
        out.backward(gin)
        want = table_grads_host(gin, [G.x[:, 0], G.x[:, 1], depth], (98, 10030, 21))
        for p, w in zip((enc.type_encoder.weight, enc.attribute_encoder.weight, enc.depth_encoder.weight), want):
            assert torch.equal(p.grad.cpu(), torch.from_numpy(w))


def test_reference_gradient_fixture_with_the_knob_on(device, monkeypatch):
    """`grad_h32_bidir` (the reference's own autograd on a seeded step) through the knob-on path, at the tolerance of
    `test_training_step_gradients_match_reference_golden`."""
    from tests.test_gpu_parity import TOL, _train_step
    monkeypatch.setattr(engine, "TABLE_GRADS", 1)
    calls = []
    orig = engine.table_grads
    monkeypatch.setattr(engine, "table_grads", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    meta, arr = Hh.load("grad_h32_bidir")
    model = Hh.code2_model(meta).to(device)
    loss, grads = _train_step(model, Hh.code2_batch(arr, device), torch.from_numpy(arr["y"]).to(device))
    assert calls == [1]
    assert abs(float(loss) - float(arr["loss"])) < 1e-5
    with torch.no_grad():
        assert Hh.maxdiff(torch.stack(model(Hh.code2_batch(arr, device))), arr["pred"]) < TOL
    assert Hh.check_grads(meta, arr, grads, rtol=1e-4) < 1e-4
