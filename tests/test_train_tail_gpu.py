"""The tail of a training step, kernel by kernel, against float64: `dagnn_tn_product`, `dagnn_wgrad_run`, `dagnn_colsum_run`,
`dagnn_attn_grads_run` (csrc/wgrad.hip), `dagnn_seq_ce` (csrc/loss.hip), `dagnn_grad_norm` and `dagnn_clip_adam` (csrc/optim.hip).

Every comparison is element by element against a float64 torch expression of the same operation on the same fp32 inputs.  The
tolerances are of two kinds only:
  * sums and products: the forward bound of fp32 summation in any order, |got - ref| <= (n + c) u sum|terms| with u = 2^-24
    (gamma_n = n u / (1 - n u) <= (n + 1) u for n < 4096), n the longest chain of roundings a term passes through - counted from
    the kernel's code in a comment next to each use;
  * transcendental paths (softmax / log, Adam's sqrt and divisions): the error of torch's own fp32 kernels against float64 on
    the same inputs, measured by the test itself in the same units, times 4 (fast intrinsics and fused multiply-adds carry
    about one ulp more than libm, the summation order differs).  DESIGN.md §4i records the ratios measured on an MI355X.
No element is masked out; buffers are pre-filled with NaN or a sentinel, so an element the kernel does not write, or a word it
writes past its output, fails the comparison."""
import ctypes as C
import math

import pytest
import torch

from dagnn_amd import _lib as L
from dagnn_amd import engine
from dagnn_amd.train import ClipAdam, seq_cross_entropy

from tests import helpers as Hh

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # unit roundoff of fp32
FLT_MIN = 2.0 ** -126     # smallest normal fp32 (the GPU's fast exp flushes below it)
SENT = 12345.0            # what the slack behind an output holds
EINVAL = -22


def _randn(shape, seed, device, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(device)


def _pitched(mat, ld, fill=float("nan"), extra_rows=0):
    """`mat` [n, k] as a view of rows of pitch `ld`; the padding words (and `extra_rows` more rows behind) hold `fill`."""
    n, k = mat.shape
    buf = torch.full((n + extra_rows, ld), fill, dtype=torch.float32, device=mat.device)
    buf[:n, :k] = mat
    return buf[:n, :k]


def _with_slack(n, device, fill=float("nan"), extra=64):
    """fp32 output of n words (pre-filled with `fill`) and the sentinel words right behind it."""
    whole = torch.full((n + extra,), SENT, dtype=torch.float32, device=device)
    whole[:n] = fill
    return whole[:n], whole[n:]


def _untouched(slack):
    return bool((slack == SENT).all())


def _within(got, ref, bound):
    """Every element: |got - ref| <= bound (a NaN on either side fails)."""
    err = (got.double() - ref).abs()
    return bool((err <= bound).all())


def _worst(got, ref, bound):
    err = (got.double() - ref).abs()
    return "worst err %.3g at bound %.3g" % (float(err.nan_to_num(float("inf")).max()), float(bound.max()) if bound.numel() else 0.0)


def _ceil4(n):
    return (n + 3) // 4 * 4


# =========================================================================== 1. dagnn_tn_product, dagnn_wgrad_run, engine.wgrad
def _tn_ref(A, Bm):
    """(ref, sum of |terms|) of A^T B in float64 and the same for the column sums of A."""
    A64, B64 = A.double(), Bm.double()
    return A64.t() @ B64, A64.abs().t() @ B64.abs(), A64.sum(0), A64.abs().sum(0)


def _tn_call(lib, A, Bm, N, M, K2, out, colsum):
    return lib.dagnn_tn_product(A.data_ptr(), A.stride(0), Bm.data_ptr(), Bm.stride(0), N, M, K2, out.data_ptr(),
                                None if colsum is None else colsum.data_ptr(), engine._stream(A))


@pytest.mark.parametrize("K2", [2, 66, 258])
@pytest.mark.parametrize("M", [4, 130, 301])
def test_tn_product_matches_float64(device, M, K2):
    """out = A^T B and colsum = sum_n A, N in {1, 2, 15, 16, 17, 33} (the pipeline's groups of 4 UN = 16 rows, an odd last pair),
    both pitches tight and loose, with and without the column sums.
    Rounding chain (wgrad_partial_kernel, splits = 1): an MFMA step adds the products of two rows to the accumulator, at most one
    rounding for a product and one per add.  The first row's product meets an accumulator of 0 (exact) and then the adds of
    the N - 1 later rows; a later row's passes its own add and fewer later ones: at most N roundings per term.  The rows
    >= N of the last group are zeros (exact).  Column sums: a lane adds every second row (N / 2 adds), one more add joins the two
    half-waves.  So the bound is gamma_N <= (N + 1) u: c = 1, the second-order term alone."""
    lib = L.load()
    c = 1
    for N in (1, 2, 15, 16, 17, 33):
        A0, B0 = _randn((N, M), 1000 + N, device), _randn((N, K2), 2000 + N, device)
        ref, mag, cref, cmag = _tn_ref(A0, B0)
        for lda in (_ceil4(M), _ceil4(M) + 8):
            for ldb in (K2, K2 + 6):
                A, Bm = _pitched(A0, lda), _pitched(B0, ldb)   # (NaN in the padding words: none may reach a stored element)
                for want_cs in (False, True):
                    out, out_slack = _with_slack(M * K2, device)
                    cs, cs_slack = _with_slack(M, device)
                    rc = _tn_call(lib, A, Bm, N, M, K2, out, cs if want_cs else None)
                    assert rc == 0, (rc, N, lda, ldb)
                    tag = (N, lda, ldb, want_cs)
                    g = (N + c) * U
                    assert _within(out.view(M, K2), ref, g * mag), (tag, _worst(out.view(M, K2), ref, g * mag))
                    assert _untouched(out_slack) and _untouched(cs_slack), tag
                    if want_cs:
                        assert _within(cs, cref, g * cmag), (tag, _worst(cs, cref, g * cmag))
                    else:
                        assert bool(torch.isnan(cs).all()), tag   # (not asked for: not written)


def test_tn_product_refuses_bad_arguments(device):
    """Odd K2, a pitch of A that is no multiple of 4 or shorter than ceil4(M), an odd or short pitch of B, pointers off their
    alignment (A: 16 bytes, B and out: 8), N = 0: DAGNN_EINVAL before anything is launched."""
    lib = L.load()
    A = torch.zeros(8, 16, device=device)
    Bm = torch.zeros(8, 16, device=device)
    out = torch.full((16 * 16 + 8,), SENT, device=device)
    st = engine._stream(A)
    a, b, o = A.data_ptr(), Bm.data_ptr(), out.data_ptr()
    ok = lambda *args: lib.dagnn_tn_product(*args, None, st)   # noqa: E731
    assert ok(a, 16, b, 16, 8, 6, 4, o) == 0
    assert ok(a, 16, b, 16, 8, 6, 3, o) == EINVAL      # odd K2
    assert ok(a, 6, b, 16, 8, 6, 4, o) == EINVAL       # lda % 4
    assert ok(a, 4, b, 16, 8, 6, 4, o) == EINVAL       # lda < ceil4(M)
    assert ok(a, 4, b, 16, 8, 5, 4, o) == EINVAL       # lda < M
    assert ok(a, 16, b, 2, 8, 6, 4, o) == EINVAL       # ldb < K2
    assert ok(a, 16, b, 5, 8, 6, 4, o) == EINVAL       # ldb odd
    assert ok(a + 4, 16, b, 16, 4, 6, 4, o) == EINVAL  # A not 16-byte aligned
    assert ok(a + 8, 16, b, 16, 4, 6, 4, o) == EINVAL
    assert ok(a, 16, b + 4, 16, 4, 6, 4, o) == EINVAL  # B not 8-byte aligned
    assert ok(a, 16, b, 16, 4, 6, 4, o + 4) == EINVAL  # out not 8-byte aligned
    assert ok(a, 16, b, 16, 0, 6, 4, o) == EINVAL      # nothing to reduce
    assert ok(None, 16, b, 16, 8, 6, 4, o) == EINVAL
    torch.cuda.synchronize(device)
    assert bool((out[24:] == SENT).all())


@pytest.mark.parametrize("splits", [1, 3, 64])
@pytest.mark.parametrize("Hp,H", [(32, 32), (36, 32), (36, 33)])
def test_wgrad_run_splits_padding_and_mixed_widths(device, Hp, H, splits):
    """The raw batch call with chosen `splits`: three jobs of input width 2, 66 and 320 in one launch (one partial pitch K2max for
    all), one of them without a bias; gate blocks of Hp columns whose columns >= H hold DATA that must be dropped; N = 0 (exact
    zeros), N = 5 (most of 64 splits are empty), N = 130.  The workspace starts as NaN: a partial tile nobody wrote would show.
    Rounding chain: inside a split as in `dagnn_tn_product` (<= rows of the split <= N roundings), then wgrad_reduce_kernel adds
    the `splits` partials in order (the first add is to 0: splits - 1 roundings): <= N + splits - 1 roundings, and gamma of that
    is below (N + c) u with c = splits + 1 (one for the second-order term, (N + splits)^2 u < 1 for every N here)."""
    lib = L.load()
    dims, pitch_extra, want_bias = (2, 66, 320), (0, 4, 0), (True, False, True)
    c = splits + 1
    nbytes = lib.dagnn_wgrad_workspace_bytes(3, Hp, max(dims), splits)
    for N in (0, 5, 130):
        ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=device)
        arr = (L.WgradJob * 3)()
        keep, outs = [], []
        for q, K2 in enumerate(dims):
            # one more row behind the N the call names, full of NaN: a row index past n_end would show
            dg = _pitched(_randn((N, 3 * Hp), 31 * N + q, device), 3 * Hp + 4 * (q == 1), extra_rows=1)
            inp = _pitched(_randn((N, K2), 57 * N + q, device), K2 + pitch_extra[q], extra_rows=1)
            dW, dW_slack = _with_slack(3 * H * K2, device)
            db, db_slack = _with_slack(3 * H, device)
            keep += [dg, inp]
            outs.append((dg, inp, dW.view(3 * H, K2), dW_slack, db, db_slack))
            base_dg, base_in = dg._base, inp._base
            arr[q] = L.WgradJob(base_dg.data_ptr(), base_in.data_ptr(), dW.data_ptr(), db.data_ptr() if want_bias[q] else None,
                                base_dg.stride(0), base_in.stride(0), K2)
        rc = lib.dagnn_wgrad_run(arr, 3, N, Hp, H, splits, ws.data_ptr(), nbytes, engine._stream(ws))
        assert rc == 0, (rc, N)
        for q, (dg, inp, dW, dW_slack, db, db_slack) in enumerate(outs):
            A = dg.view(N, 3, Hp)[:, :, :H].reshape(N, 3 * H)
            ref, mag, cref, cmag = _tn_ref(A, inp)
            g = (N + c) * U if N else 0.0
            assert _within(dW, ref, g * mag), (N, q, _worst(dW, ref, g * mag))
            assert _untouched(dW_slack) and _untouched(db_slack), (N, q)
            if want_bias[q]:
                assert _within(db, cref, g * cmag), (N, q, _worst(db, cref, g * cmag))
            else:
                assert bool(torch.isnan(db).all()), (N, q)
            if N == 0:
                assert Hh.maxdiff(dW, torch.zeros_like(dW)) == 0.0 and (not want_bias[q] or Hh.maxdiff(db, torch.zeros_like(db)) == 0.0)


def test_wgrad_run_refuses_bad_arguments(device):
    lib = L.load()
    t, ws = torch.zeros(4096, device=device), torch.zeros(4096, device=device)
    job = lambda **kw: (L.WgradJob * 1)(L.WgradJob(**dict(dict(dg=t.data_ptr(), inp=t.data_ptr() + 4096, d_weight=t.data_ptr() + 8192,   # noqa: E731
                                                               d_bias=None, ld_dg=96, ld_in=4, in_dim=4), **kw)))
    run = lambda arr, N=4, Hp=32, H=32, splits=1, nb=4 * 4096: lib.dagnn_wgrad_run(arr, 1, N, Hp, H, splits, ws.data_ptr(), nb, engine._stream(t))   # noqa: E731
    assert run(job(), N=0) == 0
    assert run(job(in_dim=3)) == EINVAL            # odd width
    assert run(job(ld_dg=92)) == EINVAL            # pitch below 3 Hp
    assert run(job(ld_dg=98)) == EINVAL            # pitch % 4
    assert run(job(ld_in=2)) == EINVAL             # pitch below the width
    assert run(job(), Hp=34, H=32) == EINVAL       # Hp % 4
    assert run(job(), Hp=32, H=33) == EINVAL       # H > Hp
    assert run(job(), splits=65) == EINVAL
    assert run(job(), splits=0) == EINVAL
    assert run(job(), N=-1) == EINVAL
    assert run(job(), splits=64, nb=1024) == -28   # DAGNN_ENOSPC
    torch.cuda.synchronize(device)


def test_engine_wgrad_odd_width_many_jobs_repeatable(device):
    """`engine.wgrad`: an odd input width as a view of wider rows (the wrapper takes the row's next word along as a column it
    drops: that word is NaN here and must not reach a returned column) and as a contiguous matrix (zero-padded copy); 33 jobs
    of mixed widths = two launches; Hp > H; a second call is bitwise equal.  The wrapper picks the splits (at most 64):
    c = 64 + 1 by the chain of `test_wgrad_run_splits_padding_and_mixed_widths`."""
    N, Hp, H = 130, 36, 33
    c = 64 + 1
    widths = [33, 33, 2, 66, 7, 320, 64, 1, 34, 5, 12]
    jobs, refs = [], []
    for q in range(33):
        K = widths[q % len(widths)]
        dg = _randn((N, 3 * Hp), 400 + q, device)
        x = _randn((N, K), 500 + q, device)
        if q % 2 == 0:
            pitch = _ceil4(K + 1) if K % 2 else K + 4
            inp = _pitched(x, pitch)          # strided view, NaN behind column K - 1
        else:
            inp = x                           # contiguous
        jobs.append((dg, inp, q % 3 != 1))
        refs.append(_tn_ref(dg.view(N, 3, Hp)[:, :, :H].reshape(N, 3 * H), x))
    got = engine.wgrad(jobs, N, Hp, H)
    again = engine.wgrad(jobs, N, Hp, H)
    assert len(got) == 33
    g = (N + c) * U
    for q, ((dW, db), (ref, mag, cref, cmag)) in enumerate(zip(got, refs)):
        assert dW.shape == ref.shape and dW.is_contiguous(), q
        assert _within(dW, ref, g * mag), (q, widths[q % len(widths)], _worst(dW, ref, g * mag))
        if jobs[q][2]:
            assert _within(db, cref, g * cmag), (q, _worst(db, cref, g * cmag))
        else:
            assert db is None
        assert torch.equal(dW, again[q][0]) and (db is None or torch.equal(db, again[q][1])), q


# =========================================================================== 2. engine.colsums, engine.attn_grads
def _colsum_g(N):
    """colsum_partial_kernel: 256 chunks of per = ceil(N / 256) rows; in a chunk a thread's fma chain is at most ceil(per / phases)
    <= per long (one rounding per fused multiply-add); two adds join its four accumulators (none when the chunk has one row:
    adds of exact zeros do not round); the row phases that hold a row, at most min(per, 256), meet in LDS (the first add is
    to 0); colsum_reduce_kernel adds the chunk sums in order, of which at most min(N, 256) are not zero:
    <= per + min(2, per - 1) + (min(per, 256) - 1) + (min(N, 256) - 1) roundings; + 1 for the second-order term of gamma."""
    per = (N + 255) // 256
    return (per + min(2, per - 1) + (min(per, 256) - 1) + (min(N, 256) - 1) + 1) * U


def _colsum_job(N, K, weighted, seed, device, pitch=None, one_d=False):
    """(x, w) for `engine.colsums` with N rows named in the call and one more row / weight of NaN behind them, and the float64
    reference with its sum of |terms|."""
    x0 = _randn((N, K), seed, device)
    w0 = _randn((N,), seed + 1, device) if weighted else None
    rows = max(N, 1)   # (an empty tensor has no address: N = 0 is a call that names no rows of a one-row buffer)
    xb = torch.full((rows + 1, pitch or K), float("nan"), dtype=torch.float32, device=device)
    xb[:N, :K] = x0
    x = xb[:rows, :K]
    if one_d:
        assert K == 1 and pitch is None
        x = xb[:rows, 0]
    w = None
    if weighted:
        wb = torch.full((rows + 1,), float("nan"), dtype=torch.float32, device=device)
        wb[:N] = w0
        w = wb[:rows]
    t = x0.double() if w0 is None else w0.double()[:, None] * x0.double()
    return (x, w), t.sum(0), t.abs().sum(0)


@pytest.mark.parametrize("N", [0, 1, 255, 257, 1030])
def test_colsums_match_float64(device, N):
    """K in {1, 3, 256, 257, 600} (one pass, a width that is no power of two, the second pass of the column loop), with and
    without weights, a row pitch above K, a 1-d input; N from nothing over fewer rows than chunks to several rows per chunk.
    Reference (w[:, None] * X).double().sum(0); bitwise repeatable."""
    jobs, refs = [], []
    for q, K in enumerate((1, 3, 256, 257, 600)):
        for weighted in (False, True):
            j, ref, mag = _colsum_job(N, K, weighted, 10 * N + 2 * q + weighted, device)
            jobs.append(j)
            refs.append((ref, mag))
    for K, pitch, weighted in ((3, 8, True), (257, 259, False), (600, 1024, True)):
        j, ref, mag = _colsum_job(N, K, weighted, 7 * N + K, device, pitch=pitch)
        jobs.append(j)
        refs.append((ref, mag))
    for weighted in (False, True):
        j, ref, mag = _colsum_job(N, 1, weighted, 3 * N + weighted, device, one_d=True)
        jobs.append(j)
        refs.append((ref, mag))
    got = engine.colsums(jobs, N)
    again = engine.colsums(jobs, N)
    g = _colsum_g(N) if N else 0.0
    for q, (o, (ref, mag)) in enumerate(zip(got, refs)):
        assert o.shape == ref.shape, q
        assert _within(o, ref, g * mag), (q, _worst(o, ref, g * mag))
        assert torch.equal(o, again[q]), q


def test_colsums_33_jobs_of_mixed_width(device):
    """33 jobs = two launches; the widths differ inside a launch (one partial pitch Kmax for all of them)."""
    N = 257
    Ks = [1, 600, 3, 257, 256, 2, 31]
    jobs, refs = [], []
    for q in range(33):
        j, ref, mag = _colsum_job(N, Ks[q % len(Ks)], q % 2 == 1, 900 + 2 * q, device, pitch=None if q % 3 else Ks[q % len(Ks)] + 5)
        jobs.append(j)
        refs.append((ref, mag))
    got = engine.colsums(jobs, N)
    assert len(got) == 33
    g = _colsum_g(N)
    for q, (o, (ref, mag)) in enumerate(zip(got, refs)):
        assert _within(o, ref, g * mag), (q, _worst(o, ref, g * mag))


def test_attn_grads_match_float64_autograd(device):
    """`engine.attn_grads`, 17 jobs = two launches: with edge features (R = 1, 3) and without, dq in {0, 7}, attn_len > dq + kd
    in some jobs.  The three sums stand for the score  s = attn_w . [query ; key + edge_encoder(features)]  summed over the
    nodes with their sigmas:  L = attn_w[dq : dq + kd] . (key_sum + W_e feat_sum + b_e sigma_sum); the reference is float64
    autograd of L in attn_w, W_e and b_e on the same fp32 sums (the columns outside [dq, dq + kd) take no part: exact zeros).
    Rounding: g_attn[dq + k] adds R + 2 terms - key_sum[k], R fused multiply-adds, the ROUNDED product b_e[k] sigma_sum - and a
    term passes at most R + 2 roundings (R - 1 fmas behind the first, two adds; the product's own); gamma_(R + 2) <= (R + 3) u.
    The edge encoder's gradients are single products: one rounding, inside the same bound."""
    jobs, refs = [], []
    for q in range(17):
        R = (0, 1, 3)[q % 3]
        dq = (0, 7)[q % 2]
        kd = (5, 64, 33, 300)[q % 4]
        tail = (0, 0, 6)[(q // 2) % 3]
        alen = dq + kd + tail
        j = {"key_sum": _randn((kd,), 40 * q, device), "attn_w": _randn((1, alen), 40 * q + 1, device), "dq": dq,
             "feat_sum": None, "sigma_sum": None, "edge_w": None, "edge_b": _randn((kd,), 40 * q + 2, device)}
        if R:
            j.update(feat_sum=_randn((R,), 40 * q + 3, device), sigma_sum=_randn((1,), 40 * q + 4, device),
                     edge_w=_randn((kd, R), 40 * q + 5, device))
        jobs.append(j)
        aw = j["attn_w"].double().requires_grad_(True)
        key = j["key_sum"].double()
        mag_attn = torch.zeros(1, alen, dtype=torch.float64, device=device)
        if R:
            ew, eb = j["edge_w"].double().requires_grad_(True), j["edge_b"].double().requires_grad_(True)
            fs, ss = j["feat_sum"].double(), j["sigma_sum"].double()
            Lq = (aw[0, dq:dq + kd] * (key + ew @ fs + eb * ss)).sum()
            ga, gw, gb = torch.autograd.grad(Lq, [aw, ew, eb])
            mag_attn[0, dq:dq + kd] = key.abs() + ew.detach().abs() @ fs.abs() + (eb.detach() * ss).abs()
            wk = aw.detach()[0, dq:dq + kd]
            refs.append((ga, mag_attn, gw, wk.abs()[:, None] * fs.abs()[None, :], gb, (wk * ss).abs()))
        else:
            Lq = (aw[0, dq:dq + kd] * key).sum()
            ga, = torch.autograd.grad(Lq, [aw])
            mag_attn[0, dq:dq + kd] = key.abs()
            refs.append((ga, mag_attn, None, None, None, None))
    got = engine.attn_grads(jobs)
    again = engine.attn_grads(jobs)
    assert len(got) == 17
    for q, ((g_attn, g_ew, g_eb), (ga, mag_attn, gw, mag_w, gb, mag_b)) in enumerate(zip(got, refs)):
        j = jobs[q]
        R = 0 if j["edge_w"] is None else j["edge_w"].shape[1]
        g = (R + 3) * U
        dq, kd = j["dq"], j["key_sum"].numel()
        assert g_attn.shape == ga.shape, q
        assert _within(g_attn, ga, g * mag_attn), (q, _worst(g_attn, ga, g * mag_attn))
        outside = torch.ones(g_attn.shape[1], dtype=torch.bool, device=device)
        outside[dq:dq + kd] = False
        assert bool((g_attn[0, outside] == 0).all()), q
        assert torch.equal(g_attn, again[q][0]), q
        if R:
            assert g_ew.shape == gw.shape and g_eb.shape == gb.shape, q
            assert _within(g_ew, gw, g * mag_w), (q, _worst(g_ew, gw, g * mag_w))
            assert _within(g_eb, gb, g * mag_b), (q, _worst(g_eb, gb, g * mag_b))
        else:
            assert g_ew is None and g_eb is None, q


# =========================================================================== 3. dagnn_seq_ce
CE_SHAPES = [(1, 1), (3, 5), (51, 5), (65, 4)]          # B S = 1, 15, 255, 260
CE_VOCABS = [1, 2, 17, 255, 256, 257, 1000]
CE_REGIMES = ["normal", "peaked", "constant", "far_target", "neg_inf"]


def _ce_case(B, S, V, regime, device):
    """Seeded logits [B, S, V] and targets [B, S] of one regime: N(0, 1); N(0, 1) x 30 (peaked rows); every row constant; the
    target 80 below the row's maximum (loss ~ 80); -inf in about half of the non-target columns."""
    seed = 100000 * CE_REGIMES.index(regime) + 1000 * (B * S) + V
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, V, generator=gen)
    y = torch.randint(0, V, (B, S), generator=gen)
    onehot = torch.zeros(B, S, V, dtype=torch.bool).scatter_(2, y[..., None], True)
    if regime == "peaked":
        x = x * 30.0
    elif regime == "constant":
        x = x[..., :1].expand(B, S, V).contiguous()
    elif regime == "far_target" and V > 1:
        others = x.masked_fill(onehot, float("-inf")).amax(-1, keepdim=True)
        x = torch.where(onehot, others - 80.0, x)
    elif regime == "neg_inf":
        drop = (torch.rand(B, S, V, generator=gen) < 0.5) & ~onehot
        x = x.masked_fill(drop, float("-inf"))
    return x.to(device), y.to(device)


def _ce_c(V):
    """The relative errors of a softmax entry that do not scale with |x - max| (seq_ce_kernel): exp's own (1), the sum z - a
    thread's chain of ceil(V / 256) adds, 6 shuffle levels, 2 adds across the waves -, the reciprocal (1), the two products
    by it and by the scale (2), the scale 1 / (B S) itself (1)."""
    return (V + 255) // 256 + 6 + 2 + 5


class _Ce64(object):
    """float64 log_softmax / softmax per (graph, head) row of fp32 logits [R, V] with targets [R], and the error units."""

    def __init__(self, x, y, BS):
        x64 = x.double()
        V = x.shape[1]
        self.ls = torch.log_softmax(x64, -1)
        self.p = torch.softmax(x64, -1)
        self.onehot = torch.zeros_like(self.p).scatter_(1, y.clamp(0, V - 1)[:, None], 1.0)
        self.onehot[(y < 0) | (y >= V)] = 0.0
        self.good = (y >= 0) & (y < V)
        self.loss = -self.ls.gather(1, y.clamp(0, V - 1)[:, None])[:, 0]
        spread = x64.amax(-1, keepdim=True) - x64
        spread = torch.where(self.p > 0, spread, torch.zeros_like(spread))   # (-inf columns: p = 0 exactly, no error allowed)
        c = _ce_c(V)
        # unit of an entry of softmax - onehot: u (|x_j - max| + c) p_j, + u on the target (the subtraction from 1), + the smallest
        # normal fp32 in units of B S x d logits (an entry below it may be flushed to zero)
        self.d_unit = U * ((spread + c) * self.p + self.onehot) + FLT_MIN * BS
        self.row_unit = U * (self.loss.abs() + c)
        self.c = c

    def d_ratio(self, d_times_bs, rows=None):
        r = (d_times_bs.double() - (self.p - self.onehot)).abs() / self.d_unit
        r = r if rows is None else r[rows]
        return float(r.max()) if r.numel() else 0.0

    def row_ratio(self, row_loss, rows=None):
        r = (row_loss.double() - self.loss).abs() / self.row_unit
        r = r if rows is None else r[rows]
        return float(r.max()) if r.numel() else 0.0

    def mean_ratio(self, loss):
        return abs(float(loss) - float(self.loss.mean())) / (U * (float(self.loss.abs().mean()) + self.c))


@pytest.fixture(scope="module")
def ce_torch_ratios(device):
    """The error of torch's own fp32 `softmax` / `cross_entropy` on the GPU against float64 in the units of `_Ce64`, the largest
    over every (shape, vocabulary, regime) case of this file: computed once, the kernel gets 4 x each.  The largest over all
    cases and not case by case: torch's figure holds no scaling by 1 / (B S), which costs d logits up to 1.5 u of the target
    entry (the rounding of the scale, of the product, and a p - 1 that torch's own subtraction also rounds) whatever the
    regime, and where torch's arithmetic happens to be nearly exact (constant rows: 0.2 units) 4 x its figure would leave no
    fp32 kernel room for that product.  Measured: DESIGN.md §4i."""
    worst = {"d": 0.0, "row": 0.0, "mean": 0.0}
    for B, S in CE_SHAPES:
        for V in CE_VOCABS:
            for regime in CE_REGIMES:
                x, y = _ce_case(B, S, V, regime, device)
                x, y = x.view(B * S, V), y.view(B * S)
                ref = _Ce64(x, y, B * S)
                d32 = torch.softmax(x, -1) - ref.onehot.float()
                row32 = torch.nn.functional.cross_entropy(x, y, reduction="none")
                mean32 = torch.nn.functional.cross_entropy(x, y)
                worst["d"] = max(worst["d"], ref.d_ratio(d32))
                worst["row"] = max(worst["row"], ref.row_ratio(row32))
                worst["mean"] = max(worst["mean"], ref.mean_ratio(mean32))
    print("torch fp32 against float64: softmax - onehot %.3f, row loss %.3f, mean loss %.3f units" % (worst["d"], worst["row"], worst["mean"]))
    assert all(0.0 < v < float("inf") for v in worst.values()), worst
    return worst


class _CeCall(object):
    """One raw `dagnn_seq_ce` call on logits [B, S, V] copied into rows of pitch `ld`; d logits in rows of pitch `ld_d`."""

    def __init__(self, lib, x, y, counter, ld_extra=5, ld_d_extra=3, want_d=True):
        B, S, V = x.shape
        dev = x.device
        self.B, self.S, self.V = B, S, V
        self.x = _pitched(x.reshape(B, S * V), S * V + ld_extra)
        self.y = y.contiguous()
        self.row, self.row_slack = _with_slack(B * S, dev)
        self.loss, self.loss_slack = _with_slack(1, dev)
        self.d_buf = self.d_slack = None
        if want_d:
            whole = torch.full((B * (S * V + ld_d_extra) + 64,), SENT, dtype=torch.float32, device=dev)
            self.d_buf = whole[:B * (S * V + ld_d_extra)].view(B, S * V + ld_d_extra)
            self.d_slack = whole[B * (S * V + ld_d_extra):]
        base = self.x._base
        self.rc = lib.dagnn_seq_ce(base.data_ptr(), base.stride(0), self.y.data_ptr(), B, S, V,
                                   None if not want_d else self.d_buf.data_ptr(), 0 if not want_d else self.d_buf.stride(0),
                                   self.row.data_ptr(), self.loss.data_ptr(), counter.data_ptr(), engine._stream(x))

    @property
    def d(self):   # [B S, V]
        return self.d_buf[:, :self.S * self.V].reshape(self.B * self.S, self.V)

    def pads_untouched(self):
        ok = _untouched(self.row_slack) and _untouched(self.loss_slack)
        if self.d_buf is not None:
            ok = ok and _untouched(self.d_slack) and bool((self.d_buf[:, self.S * self.V:] == SENT).all())
        return ok


@pytest.mark.parametrize("V", CE_VOCABS)
@pytest.mark.parametrize("B,S", CE_SHAPES)
def test_seq_ce_matches_float64(device, ce_torch_ratios, B, S, V):
    """Raw `dagnn_seq_ce` in every logit regime: d logits x (B S) against softmax64 - onehot and the row / mean losses against
    float64 log_softmax, each within 4 x the error torch's fp32 kernels show in the same units (`ce_torch_ratios`); -inf
    columns and V = 1 exactly 0; `ld != ld_d`, both above S V, padding and slack untouched; the counter back at 0; a second
    call and the call without d logits bitwise equal."""
    lib = L.load()
    counter = torch.zeros(1, dtype=torch.int32, device=device)
    for regime in CE_REGIMES:
        x, y = _ce_case(B, S, V, regime, device)
        ref = _Ce64(x.view(B * S, V), y.view(B * S), B * S)
        a = _CeCall(lib, x, y, counter)
        assert a.rc == 0
        assert int(counter[0]) == 0, regime
        b = _CeCall(lib, x, y, counter)
        n = _CeCall(lib, x, y, counter, want_d=False)
        assert b.rc == 0 and n.rc == 0
        rd, rr, rm = ref.d_ratio(a.d * float(B * S)), ref.row_ratio(a.row), ref.mean_ratio(a.loss[0])
        print("%s B S %d V %d: d %.3f row %.3f mean %.3f units" % (regime, B * S, V, rd, rr, rm))
        assert rd <= 4 * ce_torch_ratios["d"], (regime, rd, ce_torch_ratios["d"])
        assert rr <= 4 * ce_torch_ratios["row"], (regime, rr, ce_torch_ratios["row"])
        assert rm <= 4 * ce_torch_ratios["mean"], (regime, rm, ce_torch_ratios["mean"])
        assert a.pads_untouched() and n.pads_untouched(), regime
        assert int(counter[0]) == 0, regime
        assert torch.equal(a.d, b.d) and torch.equal(a.row, b.row) and torch.equal(a.loss, b.loss), regime
        assert torch.equal(a.row, n.row) and torch.equal(a.loss, n.loss), regime
        if V == 1:
            assert bool((a.d == 0).all()) and bool((a.row == 0).all()) and float(a.loss[0]) == 0.0, regime
        if regime == "neg_inf":
            gone = torch.isinf(x.view(B * S, V))
            assert bool((a.d[gone] == 0).all())
        if regime == "far_target" and V > 1:
            # (the target is `max - 80` rounded to fp32: a value in [64, 128) moves by half an ulp = 2^-18 at most)
            assert float(ref.loss.min()) >= 80.0 - 64 * U


def test_seq_ce_refuses_bad_arguments(device):
    lib = L.load()
    t = torch.zeros(64, device=device)
    y = torch.zeros(4, dtype=torch.int64, device=device)
    cnt = torch.zeros(1, dtype=torch.int32, device=device)
    p, st = t.data_ptr(), engine._stream(t)
    call = lambda ld=6, B=2, S=2, V=3, d=p + 128, ld_d=6, x=p: lib.dagnn_seq_ce(x, ld, y.data_ptr(), B, S, V, d, ld_d, p + 192, p + 224, cnt.data_ptr(), st)   # noqa: E731
    assert call() == 0
    assert call(ld=5) == EINVAL and call(ld_d=5) == EINVAL and call(B=0) == EINVAL and call(V=0) == EINVAL and call(x=None) == EINVAL
    assert call(d=None, ld_d=0) == 0
    torch.cuda.synchronize(device)
    assert int(cnt[0]) == 0


@pytest.mark.parametrize("bad", [-1, 17])
def test_seq_ce_bad_target_is_nan_in_its_row_only(device, ce_torch_ratios, bad):
    """A target outside [0, V) in one row: NaN in that row's loss and in the total; every other row of `row_loss` and of
    d logits still meets the bound."""
    lib = L.load()
    B, S, V = 3, 5, 17
    x, y = _ce_case(B, S, V, "normal", device)
    y[1, 2] = bad
    counter = torch.zeros(1, dtype=torch.int32, device=device)
    a = _CeCall(lib, x, y, counter)
    assert a.rc == 0
    ref = _Ce64(x.view(B * S, V), y.view(B * S), B * S)
    row = 1 * S + 2
    others = torch.arange(B * S, device=device) != row
    assert bool(torch.isnan(a.row[row])) and bool(torch.isnan(a.loss[0]))
    assert not bool(torch.isnan(a.row[others]).any())
    assert ref.row_ratio(a.row, others) <= 4 * ce_torch_ratios["row"]
    assert ref.d_ratio(a.d * float(B * S), others) <= 4 * ce_torch_ratios["d"]
    assert int(counter[0]) == 0 and a.pads_untouched()


def test_seq_ce_shared_counter_across_sizes(device, ce_torch_ratios):
    """Calls of different (B, S) back to back on ONE counter, nothing waited for in between: every one is right and the counter
    reads 0 behind them."""
    lib = L.load()
    counter = torch.zeros(1, dtype=torch.int32, device=device)
    V = 257
    order = [(65, 4), (1, 1), (51, 5), (3, 5), (1, 1), (65, 4)]
    cases = [_ce_case(B, S, V, "normal", device) for B, S in order]
    torch.cuda.synchronize(device)
    calls = [_CeCall(lib, x, y, counter) for x, y in cases]
    assert int(counter[0]) == 0
    for (B, S), (x, y), a in zip(order, cases, calls):
        ref = _Ce64(x.view(B * S, V), y.view(B * S), B * S)
        assert a.rc == 0
        assert ref.d_ratio(a.d * float(B * S)) <= 4 * ce_torch_ratios["d"], (B, S)
        assert ref.row_ratio(a.row) <= 4 * ce_torch_ratios["row"], (B, S)
        assert ref.mean_ratio(a.loss[0]) <= 4 * ce_torch_ratios["mean"], (B, S)


@pytest.mark.parametrize("B,S,V", [(3, 5, 17), (65, 4, 257)])
def test_seq_cross_entropy_autograd(device, ce_torch_ratios, B, S, V):
    """`train.seq_cross_entropy` on views of one [B, S V] tensor: loss and gradient within the bound, `(3 loss).backward()` gives 3 x
    the gradient, the gradient's row pitch is a multiple of 4 floats (what the heads' weight-gradient product reads), and the
    call without a gradient gives the same loss bit for bit."""
    x, y = _ce_case(B, S, V, "normal", device)
    leaf = x.reshape(B, S * V).clone().requires_grad_(True)
    base = leaf * 1.0
    seen = []
    base.register_hook(seen.append)
    loss = seq_cross_entropy([base[:, i * V:(i + 1) * V] for i in range(S)], y)
    (3.0 * loss).backward()
    ref = _Ce64(x.view(B * S, V), y.view(B * S), B * S)
    assert ref.mean_ratio(loss.detach()) <= 4 * ce_torch_ratios["mean"]
    g, = seen
    assert g.shape == (B, S * V) and g.stride(1) == 1 and g.stride(0) % 4 == 0 and g.stride(0) >= S * V
    # (the product by 3 rounds every entry once more: one u of the entry on top of its unit)
    d = g.double().reshape(B * S, V) * float(B * S) / 3.0
    err = (d - (ref.p - ref.onehot)).abs()
    unit = ref.d_unit + U * (ref.p - ref.onehot).abs()   # + one rounding of the product by 3
    assert bool((err <= 4 * ce_torch_ratios["d"] * unit).all()), float((err / unit).max())
    assert torch.equal(leaf.grad, g)
    with torch.no_grad():
        base2 = leaf.detach() * 1.0
        loss2 = seq_cross_entropy([base2[:, i * V:(i + 1) * V] for i in range(S)], y)
    assert torch.equal(loss2, loss.detach())


# =========================================================================== 4. dagnn_grad_norm, ClipAdam
OPT_SIZES = [1, 3, 16383, 16384, 16385, 40001]


def _norm_g(calls):
    """grad_sq_kernel, one 16 K chunk per workgroup: a thread adds 64 squares in a row on the scalar path (unaligned tensors; the
    float4 path's chain is shorter: 3 adds inside a vector, 16 across) - the first square passes its own product's rounding
    and 63 adds -, 6 shuffle levels and 2 adds across the waves: 72 roundings, 73 with the second-order term.  The finish
    adds the chunk sums in double (exact at this scale) and keeps the running sum of squares as a float between the calls
    of one step: one more rounding per call.  All terms are positive, so the bound is relative to the sum itself; the square
    root halves it and the result is rounded to fp32 once more."""
    return (0.5 * (73 + calls) + 1) * U


def _opt_tensor(n, seed, device, unaligned=False, scale=1.0):
    """fp32 vector of n elements; `unaligned`: a slice of a larger buffer at a 4-byte, not 16-byte, aligned address."""
    v = _randn((n,), seed, device, scale)
    if not unaligned:
        assert v.data_ptr() % 16 == 0
        return v
    buf = torch.zeros(n + 4, device=device)
    buf[1:n + 1] = v
    out = buf[1:n + 1]
    assert out.data_ptr() % 16 == 4
    return out


def _opt_mix(count, seed, device, scale=1.0):
    """`count` (parameter, gradient) pairs over OPT_SIZES; the 40001-element ones sit at unaligned addresses: the parameter
    with an aligned gradient, the gradient with an aligned parameter, and both, in turn."""
    ps, gs = [], []
    for i in range(count):
        n = OPT_SIZES[(i + 5) % len(OPT_SIZES)]   # (a single tensor is the 40001-element one)
        how = (i // len(OPT_SIZES)) % 3 if n == 40001 else -1
        p = torch.nn.Parameter(_opt_tensor(n, seed + 2 * i, device, unaligned=how in (0, 2)))
        ps.append(p)
        gs.append(_opt_tensor(n, seed + 2 * i + 1, device, unaligned=how in (1, 2), scale=scale))
    return ps, gs


@pytest.mark.parametrize("count", [1, 48, 49, 100])
def test_grad_norm_matches_float64(device, count):
    """`ClipAdam.last_norm` over 1, 48, 49 and 100 tensors (more than 48 take further `dagnn_grad_norm` calls that accumulate)
    against float64 sqrt(sum g^2); bitwise repeatable."""
    ps, gs = _opt_mix(count, 77 * count, device, scale=0.5)
    for p, g in zip(ps, gs):
        p.grad = g
    ref = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))
    opt = ClipAdam(ps, lr=1e-3, max_norm=0.25)
    opt.step()
    first = opt.last_norm.clone()
    calls = (count + 47) // 48
    assert abs(float(first) - ref) <= _norm_g(calls) * ref, (float(first), ref)
    opt.step()
    assert torch.equal(opt.last_norm, first)
    for g0, p in zip(gs, ps):
        assert p.grad is g0   # (not replaced, not scaled)


def test_grad_norm_raw_sizes_and_bad_arguments(device):
    """One tensor of every size through the raw call, aligned and not; more than 48 tensors, a short partial buffer, an empty
    tensor: refused."""
    lib = L.load()
    partial = torch.zeros(8, device=device)
    res = torch.zeros(2, device=device)
    st = engine._stream(res)
    def run(ts, accumulate=0, plen=8):
        ptrs = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        nn_ = (C.c_int64 * len(ts))(*[t.numel() for t in ts])
        return lib.dagnn_grad_norm(ptrs, nn_, len(ts), partial.data_ptr(), plen, res.data_ptr(), accumulate, res.data_ptr() + 4, st)
    for n in OPT_SIZES:
        for unaligned in (False, True):
            g = _opt_tensor(n, 5 * n + unaligned, device, unaligned=unaligned)
            assert run([g]) == 0
            ref = float(g.double().norm())
            assert abs(float(res[1]) - ref) <= _norm_g(1) * ref, (n, unaligned)
            assert abs(float(res[0]) - ref * ref) <= 2 * _norm_g(1) * ref * ref
    g = _opt_tensor(16385, 3, device)
    assert run([g] * 49) == EINVAL
    assert run([g], plen=1) == -28
    assert int(lib.dagnn_opt_chunks((C.c_int64 * 3)(1, 16384, 16385), 3)) == 4
    ptrs, nn_ = (C.c_void_p * 1)(g.data_ptr()), (C.c_int64 * 1)(0)
    assert lib.dagnn_grad_norm(ptrs, nn_, 1, partial.data_ptr(), 8, res.data_ptr(), 0, res.data_ptr() + 4, st) == EINVAL
    torch.cuda.synchronize(device)


ADAM_GROUPS = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
               dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.02)]
ADAM_STEPS = 3
ADAM_SKIP = (1, 4)      # (step, parameter): no gradient in that step - its counter falls behind its group's
ADAM_ZEROS = 100        # leading elements of parameter 0 (group 0, no weight decay) whose gradient is 0 in every step


def _adam_inputs(device):
    """Two copies of 13 parameters (the size mix of `_opt_mix`, the first 7 in group 0) and their gradients of 3 steps."""
    def params():
        return _opt_mix(13, 4242, device)[0]
    grads = []
    for it in range(ADAM_STEPS):
        gs = _opt_mix(13, 9000 + 100 * it, device, scale=(0.01, 3.0, 0.2)[it])[1]
        gs[0][:ADAM_ZEROS] = 0.0
        if it == ADAM_SKIP[0]:
            gs[ADAM_SKIP[1]] = None
        grads.append(gs)
    return params, grads


def _adam_groups(ps):
    return [dict(ADAM_GROUPS[0], params=ps[:7]), dict(ADAM_GROUPS[1], params=ps[7:])]


def _ratio(err, unit):
    """max err / unit; an element whose unit is 0 (zero gradient, zero state) must be exact."""
    r = torch.where(unit > 0, err / unit, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max())


class _Adam64(object):
    """Adam with the clip coefficient of `clip_grad_norm_`, written out in float64: clip coefficient, L2 term, both moments,
    bias corrections; from the fp32 start state.  Next to every value runs its error unit (in multiples of u): what one
    rounding of each term of this step is worth plus the units inherited from the step before, carried through the update to
    first order.  Adam is ill-conditioned where a gradient cancels against its L2 term or a moment passes through zero
    (m / (sqrt(v) + eps) then turns a rounding of g into a visible change of p); the units grow there, for torch's kernels
    and for ours alike, so the ratio error / unit compares implementations and not the luck of single elements."""

    def __init__(self, ps):
        self.p = [p.detach().double().clone() for p in ps]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.up = [torch.zeros_like(p) for p in self.p]
        self.um = [torch.zeros_like(p) for p in self.p]
        self.uv = [torch.zeros_like(p) for p in self.p]
        self.t = [0] * len(ps)
        self.hyp = [ADAM_GROUPS[0 if i < 7 else 1] for i in range(len(ps))]
        self.norm = None

    def step(self, grads, max_norm):
        live = [i for i, g in enumerate(grads) if g is not None]
        coef = 1.0
        if max_norm is not None:
            self.norm = math.sqrt(sum(float((grads[i].double() ** 2).sum()) for i in live))
            coef = min(1.0, max_norm / (self.norm + 1e-6))
        for i in live:
            h = self.hyp[i]
            b1, b2 = h["betas"]
            wd = h["weight_decay"]
            self.t[i] += 1
            t = self.t[i]
            g = grads[i].double() * coef + wd * self.p[i]
            gmag = (grads[i].double() * coef).abs() + wd * self.p[i].abs()   # (the two terms may cancel: sum of magnitudes)
            ug = gmag + wd * self.up[i]
            self.m[i] = self.m[i] + (1.0 - b1) * (g - self.m[i])
            self.v[i] = b2 * self.v[i] + (1.0 - b2) * g * g
            self.um[i] = b1 * self.um[i] + (1.0 - b1) * ug + self.m[i].abs() + gmag
            self.uv[i] = b2 * self.uv[i] + (1.0 - b2) * 2.0 * g.abs() * ug + self.v[i] + gmag * gmag
            c2 = math.sqrt(1.0 - b2 ** t)
            denom = self.v[i].sqrt() / c2 + h["eps"]
            step_size = h["lr"] / (1.0 - b1 ** t)
            inf = torch.full_like(denom, float("inf"))
            dden = torch.where(self.uv[i] == 0, torch.zeros_like(denom), torch.where(self.v[i] > 0, self.uv[i] / (2.0 * self.v[i].sqrt() * c2), inf))
            self.p[i] = self.p[i] - step_size * (self.m[i] / denom)
            self.up[i] = self.up[i] + self.p[i].abs() + step_size * ((self.um[i] + self.m[i].abs()) / denom + self.m[i].abs() * dden / (denom * denom))

    def ratios(self, i, p, m, v):
        """Errors of one parameter and its two moments in their units."""
        return (_ratio((p.double() - self.p[i]).abs(), U * self.up[i]),
                _ratio((m.double() - self.m[i]).abs(), U * self.um[i]),
                _ratio((v.double() - self.v[i]).abs(), U * self.uv[i]))


def _adam_run(device, max_norm, fused):
    """Three steps of torch's single-tensor Adam behind `clip_grad_norm_` (fused = False) or of `ClipAdam` (True) next to the
    float64 reference: the largest error ratios of parameters and moments over all steps, and the final parameters."""
    params, grads = _adam_inputs(device)
    ps = params()
    start = [p.detach().clone() for p in ps]
    ref = _Adam64(ps)
    if fused:
        opt = ClipAdam(_adam_groups(ps), max_norm=max_norm)
    else:
        opt = torch.optim.Adam(_adam_groups(ps), foreach=False, fused=False)
    worst = [0.0, 0.0, 0.0]
    for it in range(ADAM_STEPS):
        for p, g in zip(ps, grads[it]):
            p.grad = None if g is None else (g if fused else g.clone())   # (clip_grad_norm_ scales in place)
        if not fused and max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        opt.step()
        ref.step(grads[it], max_norm)
        if fused and max_norm is not None:
            assert abs(float(opt.last_norm) - ref.norm) <= _norm_g(1) * ref.norm
        for i, p in enumerate(ps):
            if ref.t[i] == 0:
                continue
            st = opt.state[p]
            assert int(st["step"]) == ref.t[i], (it, i)
            r = ref.ratios(i, p.detach(), st["exp_avg"], st["exp_avg_sq"])
            worst = [max(a, b) for a, b in zip(worst, r)]
    return worst, ps, start, ref


ADAM_CLIPS = [0.25, 1e4, None]   # below the norm of every step (about 5, 1400 and 90), above it, no clipping


@pytest.fixture(scope="module")
def adam_torch_ratios(device):
    """The elementwise error of torch's single-tensor fp32 Adam against `_Adam64` on the inputs of `_adam_run`, per clip setting."""
    out = {}
    for mn in ADAM_CLIPS:
        out[mn] = _adam_run(device, mn, fused=False)[0]
        print("torch Adam against float64, max_norm %s: p %.3f m %.3f v %.3f units" % ((mn,) + tuple(out[mn])))
        assert all(0.0 < v < float("inf") for v in out[mn]), out[mn]
    return out


@pytest.mark.parametrize("max_norm", ADAM_CLIPS)
def test_clip_adam_matches_float64_adam(device, adam_torch_ratios, max_norm):
    """`ClipAdam` over three steps against Adam written out in float64: two parameter groups with different lr, betas and
    weight decay; `max_norm` below and above the norm, and None; a parameter that skips a step (another `step` inside its
    group); unaligned parameters with aligned gradients and the reverse.  Parameters and both moments, element by element,
    within 4 x the error of torch's own fp32 Adam in the same units (fused multiply-adds, another rounding of lr / bias1).
    Elements whose gradient and state are zero stay bit-identical where weight_decay = 0."""
    worst, ps, start, ref = _adam_run(device, max_norm, fused=True)
    print("ClipAdam against float64, max_norm %s: p %.3f m %.3f v %.3f units" % ((max_norm,) + tuple(worst)))
    for got, base, what in zip(worst, adam_torch_ratios[max_norm], ("p", "exp_avg", "exp_avg_sq")):
        assert got <= 4 * base, (what, got, base)
    assert torch.equal(ps[0].detach()[:ADAM_ZEROS], start[0][:ADAM_ZEROS])
    assert not torch.equal(ps[0].detach()[ADAM_ZEROS:], start[0][ADAM_ZEROS:])
    assert ref.t[ADAM_SKIP[1]] == ADAM_STEPS - 1 and ref.t[0] == ADAM_STEPS


@pytest.mark.parametrize("poison,max_norm", [(float("nan"), 0.25), (float("inf"), 0.25), (float("inf"), None), (float("nan"), None)])
def test_clip_adam_non_finite_pattern_is_torchs(device, poison, max_norm):
    """A NaN or inf in one gradient: the pattern of non-finite parameters and moments equals what `clip_grad_norm_` + torch's
    Adam leave (clipped: the coefficient is NaN for a NaN norm and 0 for an infinite one; unclipped: that element alone)."""
    params, grads = _adam_inputs(device)
    pa, pb = params(), params()
    opt_a = torch.optim.Adam(_adam_groups(pa), foreach=False, fused=False)
    opt_b = ClipAdam(_adam_groups(pb), max_norm=max_norm)
    for p, q, g in zip(pa, pb, grads[0]):
        p.grad, q.grad = g.clone(), g.clone()
    pa[3].grad[5] = poison
    pb[3].grad[5] = poison
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(pa, max_norm, foreach=False)
    opt_a.step()
    opt_b.step()
    some = False
    for i, (p, q) in enumerate(zip(pa, pb)):
        assert torch.equal(torch.isfinite(p), torch.isfinite(q)), i
        some = some or not bool(torch.isfinite(q).all())
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(torch.isfinite(opt_a.state[p][k]), torch.isfinite(opt_b.state[q][k])), (i, k)
    assert some
