"""`DAGNN.score` on the GPU (-m gpu): `dagnn_heads_score` against the reference's own logits (fixtures of
tests/golden/make_golden_code2_score.py) on the three schedules, against `predict` bit for bit, against the float64 definition
`evaluate.heads_score_host` at the smallest shapes at which each code path starts, the tie / special-value rules exactly, and
the `loss=True` evaluation loops.

Bounds.  Fixtures: the project's parity bound on logits is 1e-4; log-sum-exp is 1-Lipschitz in the sup norm, so `lse` is held
to 1e-4 and `nll` - a difference of two such terms - to 2e-4; a rank whose logit lies within TAU = 2e-4 of a neighbouring rank
may swap with it and is skipped (`clear`).  Free shapes: |out| <= 1, |w| <= D^-1/2, |b| <= 1, so an fp32 logit of D fused
products, D additions and one bias addition differs from float64 by at most EPS (D + 2) (sqrt(D) + 1) (`_logit_bound`); two ranks further
apart than twice that cannot swap.  `lse` / `nll` get 4 x the error torch's own fp32 `addmm` + `logsumexp` /
`cross_entropy` show against the same float64 over the same cases in the same run (`score_torch_ratios`)."""
import copy
import math

import numpy as np
import pytest
import torch

from dagnn_amd import engine, evaluate, lp
from dagnn_amd import _lib as L
from tests import helpers as Hh
from tests.test_code2_eval_gpu import _exact_case, _labelled_batches, _sync_count, eval_model

pytestmark = pytest.mark.gpu
TAU = 2e-4
EPS = 2.0 ** -24
SENT_F, SENT_I = -7.25, -77
FIXTURES = {"code2_score_b64_h64": "code2_eval_b64_h64", "code2_score_unidir_wx": "code2_eval_unidir_wx",
            "code2_score_numclass": "code2_eval_numclass"}


@pytest.fixture(params=["dataflow", "lockstep", "pergraph"])
def schedule(request, monkeypatch):
    """The three HIP schedules of the recurrence, as the golden parity tests parametrise them."""
    monkeypatch.setenv("DAGNN_AMD_SCHEDULE", "pergraph" if request.param == "pergraph" else "lockstep")
    monkeypatch.setattr(engine, "DATAFLOW", 1 if request.param == "dataflow" else 0)
    return request.param


# ----------------------------------------------------------------------------- against the reference's logits
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_score_matches_the_reference(device, name, schedule):
    meta, arr, model = eval_model(FIXTURES[name], device)
    _, ref = Hh.load(name)
    B, S = meta["B"], meta["heads"]
    y = torch.from_numpy(ref["y"]).to(device)
    s = model.score(Hh.code2_batch(arr, device), y if S > 1 else y.view(-1), topk=8)
    assert tuple(s.tok.shape) == (B, S, 8) and tuple(s.logit.shape) == (B, S, 8) and s.tok.dtype == torch.int64
    assert tuple(s.lse.shape) == (B, S) and tuple(s.nll.shape) == (B, S)
    tok, logit = s.tok.cpu().numpy(), s.logit.cpu().numpy().astype(np.float64)
    clear = ref["clear"]
    wrong = int((tok[clear] != ref["top_col"][clear]).sum())
    e_top = float(np.abs(logit - ref["top_val"]).max())
    e_lse = float(np.abs(s.lse.cpu().numpy() - ref["lse"]).max())
    e_nll = float(np.abs(s.nll.cpu().numpy() - ref["nll"]).max())
    e_loss = abs(float(s.loss) - float(ref["nll"].mean()))
    print("%s %s: slots %d ambiguous %d wrong %d, max error: top %.3e lse %.3e nll %.3e loss %.3e"
          % (name, schedule, clear.size, int((~clear).sum()), wrong, e_top, e_lse, e_nll, e_loss))
    assert wrong == 0
    assert e_top < 1e-4 and e_lse < 1e-4 and e_nll < 2e-4 and e_loss < 2e-4
    assert torch.equal(s.logprob, s.logit - s.lse.unsqueeze(-1))
    # `predict` on the same batch: bit for bit
    ptok, ptop = model.predict(Hh.code2_batch(arr, device), return_top=True)
    assert torch.equal(s.tok[:, :, 0], ptok) and torch.equal(s.logit[:, :, 0], ptop[:, :, 0])
    assert torch.equal(s.logit[:, :, 1], ptop[:, :, 1])
    # without targets, and one candidate: the same bits, no losses
    s1 = model.score(Hh.code2_batch(arr, device))
    assert s1.nll is None and torch.equal(s1.tok, s.tok[:, :, :1]) and torch.equal(s1.logit, s.logit[:, :, :1])
    assert torch.equal(s1.lse, s.lse)


# ----------------------------------------------------------------------------- raw calls with guarded outputs
def _guarded(n, dtype, device):
    sent = SENT_I if dtype == torch.int64 else SENT_F
    whole = torch.full((n + 32,), sent, dtype=dtype, device=device)
    return whole[16:16 + n], whole


def _untouched(whole, n):
    sent = SENT_I if whole.dtype == torch.int64 else SENT_F
    return bool((whole[:16] == sent).all()) and bool((whole[16 + n:] == sent).all())


def _pitched(t, pitch):
    """`t` [R, D] as a view of rows `pitch` floats apart (an odd pitch: rows that are not 16-byte aligned)."""
    buf = torch.full((t.shape[0], pitch), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


class _Call(object):
    """One raw `dagnn_heads_score` call; every output sits between sentinels, `sums` starts at (0.5, 3)."""

    def __init__(self, out, w, b, S, V, y=None, k=1, sums=False):
        lib, dev = L.load(), out.device
        B, D = out.shape
        self.n = B * S
        self.tok, self._tok = _guarded(B * S * k, torch.int64, dev)
        self.logit, self._logit = _guarded(B * S * k, torch.float32, dev)
        self.lse, self._lse = _guarded(B * S, torch.float32, dev)
        self.nll, self._nll = _guarded(B * S, torch.float32, dev) if y is not None else (None, None)
        self.sums = None
        if sums:
            self.sums = torch.full((6,), SENT_F, dtype=torch.float64, device=dev)
            self.sums[2] = 0.5
            self.sums.view(torch.int64)[3] = 3
        nbytes = lib.dagnn_heads_score_bytes(B, S, V, k)
        work, self._work = _guarded(nbytes // 8, torch.int64, dev)
        self.rc = lib.dagnn_heads_score(out.data_ptr(), out.stride(0), w.data_ptr(), w.stride(0), b.data_ptr(), B, D, S, V,
                                        None if y is None else y.data_ptr(), k, self.tok.data_ptr(), self.logit.data_ptr(),
                                        self.lse.data_ptr(), None if y is None else self.nll.data_ptr(),
                                        None if self.sums is None else self.sums[2:].data_ptr(), work.data_ptr(), nbytes,
                                        engine._stream(out))
        self.tok, self.logit = self.tok.view(B, S, k), self.logit.view(B, S, k)
        self.lse = self.lse.view(B, S)
        self.nll = None if y is None else self.nll.view(B, S)
        self.k, self.nwork = k, nbytes // 8

    def pads_untouched(self):
        ok = _untouched(self._tok, self.n * self.k) and _untouched(self._logit, self.n * self.k) and _untouched(self._lse, self.n)
        ok = ok and _untouched(self._work, self.nwork) and (self.nll is None or _untouched(self._nll, self.n))
        if self.sums is not None:
            ok = ok and bool((self.sums[:2] == SENT_F).all()) and bool((self.sums[4:] == SENT_F).all())
        return ok

    def sum_rows(self):
        host = self.sums.cpu()
        return float(host[2]), int(host.view(torch.int64)[3])


def _raw_argmax(out, w, b, S, V):
    lib = L.load()
    B, D = out.shape
    tok = torch.empty(B, S, dtype=torch.int64, device=out.device)
    top = torch.empty(B, S, 2, dtype=torch.float32, device=out.device)
    work = torch.empty(lib.dagnn_heads_argmax_bytes(B, S, V) // 8, dtype=torch.int64, device=out.device)
    engine.check(lib.dagnn_heads_argmax(out.data_ptr(), out.stride(0), w.data_ptr(), w.stride(0), b.data_ptr(), B, D, S, V,
                                        tok.data_ptr(), top.data_ptr(), work.data_ptr(), work.numel() * 8, engine._stream(out)),
                 "heads_argmax")
    return tok, top


def _seq_sum(start, rows):
    """`start` + the rows one by one in row order, in float64: what the summing thread computes."""
    acc = float(start)
    for v in rows.reshape(-1).tolist():
        acc += v
    return acc


# ----------------------------------------------------------------------------- free shapes against the float64 definition
FREE_D = [64, 20, 6]            # the 32-wide stage / float4 tiles / scalar loads (rows 7 floats apart)
FREE_V = [1, 3, 128, 129, 301, 5002]
FREE_B = [1, 127, 129]
FREE_S = [1, 5]
FREE_K = [1, 3, 8]
_CASES = {}


def _logit_bound(D):
    return EPS * (D + 2) * (math.sqrt(D) + 1.0)


def _free_case(D, V, B, S, device):
    """Operands, targets and the float64 definition of one shape: built once, shared, never changed."""
    key = (D, V, B, S)
    if key not in _CASES:
        g = torch.Generator().manual_seed(((D * 7919 + V) * 131 + B) * 7 + S)
        out = torch.rand(B, D, generator=g) * 2 - 1
        w = (torch.rand(S * V, D, generator=g) * 2 - 1) / D ** 0.5
        b = torch.rand(S * V, generator=g) * 2 - 1
        y = torch.randint(0, V, (B, S), generator=g)
        y[0::3] = 0                    # the first column, the last live column (V = 301, 5002: in the partial tile)
        y[1::3] = V - 1
        host = evaluate.heads_score_host(out, w, b, S, V, y=y, k=9)   # (the 9th value: whether rank 8 is clear)
        del host["logits"]
        pitch = 7 if D == 6 else D
        _CASES[key] = dict(out=_pitched(out.to(device), pitch), w=_pitched(w.to(device), pitch), b=b.to(device), y=y.to(device),
                           host=host)
    return _CASES[key]


def _units(got, want):
    """max |got - want| in units of EPS max(1, |want|)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / (EPS * np.maximum(1.0, np.abs(want)))).max())


@pytest.fixture(scope="module")
def score_torch_ratios(device):
    """The error of torch's own fp32 `addmm` + `logsumexp` / `cross_entropy` on the GPU against the float64 definition, in
    `_units`, the largest over every free shape of this file: computed once, the kernel gets 4 x each."""
    worst = {"lse": 0.0, "nll": 0.0}
    for D in FREE_D:
        for V in FREE_V:
            for B in FREE_B:
                for S in FREE_S:
                    c = _free_case(D, V, B, S, device)
                    x = torch.addmm(c["b"], c["out"], c["w"].t()).view(B * S, V)
                    worst["lse"] = max(worst["lse"], _units(torch.logsumexp(x, dim=1).cpu().numpy().reshape(B, S), c["host"]["lse"]))
                    nll = torch.nn.functional.cross_entropy(x, c["y"].view(-1), reduction="none")
                    worst["nll"] = max(worst["nll"], _units(nll.cpu().numpy().reshape(B, S), c["host"]["nll"]))
    print("torch fp32 against float64: lse %.3f, nll %.3f units" % (worst["lse"], worst["nll"]))
    assert all(0.0 < v < float("inf") for v in worst.values()), worst
    return worst


@pytest.mark.parametrize("V", FREE_V)
@pytest.mark.parametrize("D", FREE_D)
def test_heads_score_shapes_against_float64(device, score_torch_ratios, D, V):
    bound = _logit_bound(D)
    worst = {"lse": 0.0, "nll": 0.0, "logit": 0.0}
    for B in FREE_B:
        for S in FREE_S:
            c = _free_case(D, V, B, S, device)
            host = c["host"]
            atok, atop = _raw_argmax(c["out"], c["w"], c["b"], S, V)
            calls = {k: _Call(c["out"], c["w"], c["b"], S, V, y=c["y"], k=k, sums=(k == 8)) for k in FREE_K}
            again = _Call(c["out"], c["w"], c["b"], S, V, y=c["y"], k=8, sums=True)
            bare = _Call(c["out"], c["w"], c["b"], S, V, k=3)
            for call in list(calls.values()) + [again, bare]:
                assert call.rc == 0 and call.pads_untouched(), (B, S, call.k)
            a = calls[8]
            # two runs, the list lengths and the call without targets: the same bits
            assert torch.equal(a.tok, again.tok) and torch.equal(a.logit, again.logit) and torch.equal(a.lse, again.lse)
            assert torch.equal(a.nll, again.nll) and torch.equal(a.sums, again.sums)
            for k in (1, 3):
                assert torch.equal(calls[k].tok, a.tok[:, :, :k]) and torch.equal(calls[k].logit, a.logit[:, :, :k])
                assert torch.equal(calls[k].lse, a.lse) and torch.equal(calls[k].nll, a.nll)
            assert torch.equal(bare.tok, a.tok[:, :, :3]) and torch.equal(bare.lse, a.lse)
            # `predict`'s token and winning logit, bit for bit (and its runner-up)
            assert torch.equal(a.tok[:, :, 0], atok) and torch.equal(a.logit[:, :, 0], atop[:, :, 0])
            assert torch.equal(a.logit[:, :, 1], atop[:, :, 1])
            # the sum: row by row in row order on top of what was there, the row count beside it
            total, rows = a.sum_rows()
            assert rows == 3 + B * S and total == _seq_sum(0.5, a.nll.cpu().double().numpy())
            # columns: exact where float64 separates a rank from its neighbours by more than twice the fp32 error
            tok, logit = a.tok.cpu().numpy(), a.logit.cpu().numpy().astype(np.float64)
            n = min(8, V)
            hv9 = host["logit"][:, :, :min(9, V)]
            hv = hv9[:, :, :n]
            gap = hv9[:, :, :-1] - hv9[:, :, 1:]
            inf = np.full(gap.shape[:2] + (1,), np.inf)
            clear = ((np.concatenate([inf, gap], axis=2) > 2 * bound) & (np.concatenate([gap, inf], axis=2) > 2 * bound))[:, :, :n]
            assert np.array_equal(tok[:, :, :n][clear], host["tok"][:, :, :n][clear])
            assert (tok[:, :, n:] == -1).all() and np.isneginf(logit[:, :, n:]).all()
            assert float(np.abs(logit[:, :, :n] - hv).max()) <= bound
            assert all(len(set(r)) == n for r in tok[:, :, :n].reshape(-1, n).tolist())
            worst["logit"] = max(worst["logit"], float(np.abs(logit[:, :, :n] - hv).max()) / bound)
            worst["lse"] = max(worst["lse"], _units(a.lse.cpu().numpy(), host["lse"]))
            worst["nll"] = max(worst["nll"], _units(a.nll.cpu().numpy(), host["nll"]))
    print("D %d V %d: lse %.3f (torch %.3f) nll %.3f (torch %.3f) units, logits %.3f of their bound"
          % (D, V, worst["lse"], score_torch_ratios["lse"], worst["nll"], score_torch_ratios["nll"], worst["logit"]))
    assert worst["lse"] <= 4 * score_torch_ratios["lse"], (worst["lse"], score_torch_ratios["lse"])
    assert worst["nll"] <= 4 * score_torch_ratios["nll"], (worst["nll"], score_torch_ratios["nll"])


@pytest.mark.parametrize("D", [64, 20, 6])
def test_rows_of_a_batch_equal_the_rows_scored_alone(device, D):
    S, V = 5, 301
    c = _free_case(D, V, 129, S, device)
    whole = _Call(c["out"], c["w"], c["b"], S, V, y=c["y"], k=8)
    assert whole.rc == 0
    for r in (0, 63, 127, 128):
        one = _Call(c["out"][r:r + 1], c["w"], c["b"], S, V, y=c["y"][r:r + 1].contiguous(), k=8)
        assert one.rc == 0 and one.pads_untouched()
        assert torch.equal(one.tok[0], whole.tok[r]) and torch.equal(one.logit[0], whole.logit[r]), r
        assert torch.equal(one.lse[0], whole.lse[r]) and torch.equal(one.nll[0], whole.nll[r]), r


def test_engine_binding_and_b_zero(device):
    c = _free_case(20, 129, 127, 5, device)
    raw = _Call(c["out"], c["w"], c["b"], 5, 129, y=c["y"], k=3)
    acc = evaluate.SeqLoss(device)
    tok, logit, lse, nll = engine.heads_score(c["out"], c["w"], c["b"], 5, 129, y=c["y"], k=3, sums=acc.sums)
    assert torch.equal(tok, raw.tok) and torch.equal(logit, raw.logit) and torch.equal(lse, raw.lse) and torch.equal(nll, raw.nll)
    res = acc.compute()
    assert res["rows"] == 127 * 5 and res["loss"] == _seq_sum(0.0, nll.cpu().double().numpy()) / (127 * 5)
    tok, logit, lse, nll = engine.heads_score(c["out"][:0], c["w"], c["b"], 5, 129, k=2)
    assert tuple(tok.shape) == (0, 5, 2) and tuple(lse.shape) == (0, 5) and nll is None
    with pytest.raises(engine.DagnnHipError, match="1..8"):
        engine.heads_score(c["out"], c["w"], c["b"], 5, 129, k=9)
    with pytest.raises(engine.DagnnHipError, match="targets needed"):
        engine.heads_score(c["out"], c["w"], c["b"], 5, 129, sums=acc.sums)


# ----------------------------------------------------------------------------- ties and special values, exactly
@pytest.mark.parametrize("D", [8, 32, 6])   # float4 tiles / the 32-wide stage / scalar loads
def test_ties_go_to_the_lowest_column_at_every_rank(device, D):
    """Small-integer operands: every logit is exact in fp32, whole groups of columns are equal at every rank.  Planted equal
    pairs: inside one lane's 32 columns, across tiles, in the partial last tile (`_exact_case`), across the two column halves
    of a wave (20, 50) and across the two waves of a tile (10, 100)."""
    S, V, out, w, b, pairs = _exact_case(D, 11 + D)
    for s, (c0, c1) in ((0, (20, 50)), (1, (10, 100))):
        w[s * V + c1] = w[s * V + c0]
        b[s * V + c0] = b[s * V + c1] = 500.0   # (|out . w| <= 4 D <= 128: between the 1000s and the rest)
    y = torch.randint(0, V, (out.shape[0], S), generator=torch.Generator().manual_seed(D))
    pitch = 7 if D == 6 else D
    a = _Call(_pitched(out.to(device), pitch), _pitched(w.to(device), pitch), b.to(device), S, V, y=y.to(device), k=8)
    assert a.rc == 0 and a.pads_untouched()
    x = (out.double() @ w.double().t() + b.double()).view(-1, S, V)
    srt = torch.sort(x, dim=2, descending=True, stable=True)
    assert torch.equal(a.tok.cpu(), srt.indices[:, :, :8])
    assert torch.equal(a.logit.cpu().double(), srt.values[:, :, :8])   # bit-equal: the values are exact in fp32
    assert a.tok[:, 0, :4].cpu().tolist() == [[5, 9, 20, 50]] * out.shape[0]
    assert a.tok[:, 1, :4].cpu().tolist() == [[130, 270, 10, 100]] * out.shape[0]
    assert a.tok[:, 2, :2].cpu().tolist() == [[0, V - 1]] * out.shape[0] and a.tok[:, 3, :2].cpu().tolist() == [[290, 295]] * out.shape[0]
    ties = (srt.values[:, :, :7] == srt.values[:, :, 1:8]).sum()
    assert int(ties) > 6 * out.shape[0]                                 # equal neighbours beyond the 6 planted pairs of a graph
    host = evaluate.heads_score_host(out, w, b, S, V, y=y, k=8)
    assert np.array_equal(a.tok.cpu().numpy(), host["tok"])
    np.testing.assert_allclose(a.lse.cpu().numpy(), host["lse"], rtol=0, atol=1e-4)   # lse is about 1000: an ulp is 6e-5
    np.testing.assert_allclose(a.nll.cpu().numpy(), host["nll"], rtol=0, atol=2e-4)


@pytest.mark.parametrize("D", [64, 20, 6])
def test_special_values(device, D):
    """Zero weights, the logits planted through the biases; one scenario per head, V = 300 (two full tiles and a partial one)."""
    NAN, INF = float("nan"), float("inf")
    S, V, B = 6, 300, 3
    g = torch.Generator().manual_seed(D)
    out = torch.rand(B, D, generator=g) * 2 - 1
    w = torch.zeros(S * V, D)
    b = (torch.rand(S, V, generator=g) * 2 - 1)
    b[0, 200] = b[0, 40] = b[0, 299] = NAN                   # NaN first, ordered by column; +inf behind them
    b[0, 10] = INF
    b[1, 150] = b[1, 7] = INF                                 # +inf: lse +inf; a -inf column is last
    b[1, 0] = -INF
    b[2, :] = -INF                                            # a row of -inf alone
    b[3, :] = -1.0                                            # -0 == +0: by column
    b[3, 5] = b[3, 299] = 0.0
    b[3, 3] = b[3, 140] = -0.0
    b[4, 131:] = -INF                                         # a tile of -inf alone behind live ones; the maximum in the first
    b[5, :290] = -INF                                         # ... and in front of them; the maximum in the partial tile
    y = torch.randint(0, V, (B, S), generator=g)
    y[:, 0], y[:, 1], y[:, 2], y[:, 4], y[:, 5] = 5, 150, 17, 130, 295
    y[0, 3], y[1, 3] = -1, V                                  # outside [0, V): that row's nll alone
    pitch = 7 if D == 6 else D
    a = _Call(_pitched(out.to(device), pitch), _pitched(w.to(device), pitch), b.view(-1).to(device), S, V, y=y.to(device), k=8, sums=True)
    assert a.rc == 0 and a.pads_untouched()
    host = evaluate.heads_score_host(out, w, b.view(-1), S, V, y=y, k=8)
    tok, logit, lse, nll = a.tok.cpu().numpy(), a.logit.cpu().numpy(), a.lse.cpu().numpy(), a.nll.cpu().numpy()
    assert np.array_equal(tok, host["tok"])
    assert tok[0, 0, :4].tolist() == [40, 200, 299, 10] and tok[0, 1, :2].tolist() == [7, 150] and tok[0, 2].tolist() == list(range(8))
    assert tok[0, 3, :5].tolist() == [3, 5, 140, 299, 0]
    np.testing.assert_array_equal(logit.astype(np.float64), host["logit"])      # the logits ARE the biases
    assert not np.signbit(logit[:, 3, :4]).any()
    assert np.isnan(lse[:, 0]).all() and np.isposinf(lse[:, 1]).all() and np.isneginf(lse[:, 2]).all()
    assert np.isfinite(lse[:, 3:]).all()
    np.testing.assert_allclose(lse[:, 3:], host["lse"][:, 3:], rtol=0, atol=4e-6)   # (8 ulps of a value below 8)
    assert np.isnan(nll[:, 0]).all() and np.isnan(nll[:, 1]).all() and np.isnan(nll[:, 2]).all()   # NaN; inf - inf twice
    assert np.array_equal(np.isnan(nll), np.isnan(host["nll"]))
    assert np.isnan(nll[:2, 3]).all() and np.isfinite(nll[2, 3]) and np.isfinite(nll[:, 4:]).all()
    ok = np.isfinite(host["nll"])
    np.testing.assert_allclose(nll[ok], host["nll"][ok], rtol=0, atol=4e-6)   # (8 ulps of a value below 8)
    total, rows = a.sum_rows()
    assert math.isnan(total) and rows == 3 + B * S
    # fewer columns than candidates
    few = _Call(_pitched(out.to(device), pitch), _pitched(w[:S * 3].to(device), pitch), b[:, :3].reshape(-1).to(device), S, 3, k=8)
    assert few.rc == 0 and few.pads_untouched()
    assert (few.tok[:, :, 3:] == -1).all() and torch.isneginf(few.logit[:, :, 3:]).all()
    assert few.tok[:, 2].cpu().tolist() == [[0, 1, 2, -1, -1, -1, -1, -1]] * B


# ----------------------------------------------------------------------------- the loops
def _seq_loss_of(model, batches, targets):
    rows = [model.score(b, t).nll.cpu().double().numpy() for b, t in zip(batches, targets)]
    n = sum(r.size for r in rows)
    return _seq_sum(0.0, np.concatenate([r.reshape(-1) for r in rows])) / n, n


def test_evaluate_with_loss(device):
    meta, arr, model = eval_model("code2_eval_b64_h64", device)
    vocab2idx, batches = _labelled_batches(device, meta["V"])
    g = torch.Generator().manual_seed(12)
    for b in batches:
        b.y_arr = torch.randint(0, meta["V"], (b.num_graphs, meta["S"]), generator=g).to(device)
    fresh = lambda: [copy.deepcopy(b) for b in batches]   # noqa: E731  (a pass replaces G.x: every run gets its own copies)
    model.train()
    plain = evaluate.evaluate(model, fresh(), vocab2idx)
    res = evaluate.evaluate(model, fresh(), vocab2idx, loss=True)     # (also the warm-up: caches, arenas, pinned pools)
    assert model.training                                              # the mode is restored
    model.eval()
    assert set(plain) == {"precision", "recall", "F1", "n"} and set(res) == set(plain) | {"loss"}
    assert all(res[k] == plain[k] for k in plain)
    want, n = _seq_loss_of(model, fresh(), [b.y_arr for b in batches])
    assert res["loss"] == want and n == res["n"] * meta["S"]
    with torch.no_grad():
        from dagnn_amd.train import seq_cross_entropy
        per_batch = [float(seq_cross_entropy(model(b), b.y_arr)) * b.num_graphs for b in fresh()]
    assert abs(res["loss"] - sum(per_batch) / res["n"]) < 2e-4   # (logits within the parity bound: a loss within twice it)
    bs = fresh()
    _, base = _sync_count(lambda: [model.score(b, b.y_arr) for b in bs])
    bs = fresh()
    again, syncs = _sync_count(lambda: evaluate.evaluate(model, bs, vocab2idx, loss=True))
    assert syncs == base + 1, (syncs, base)
    assert again == res


def test_evaluate_tok_with_loss(device):
    from dagnn_amd import DAGNN, ASTNodeEncoder
    from oracle.seeding import seeded_fill
    from tests.test_store_gpu import N_ATTR, S, sweep_graphs, sweep_store
    raw, vocab = sweep_graphs()
    st = sweep_store(device)
    H = 32
    model = DAGNN(num_vocab=len(vocab), max_seq_len=S, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(H, 98, N_ATTR, 20),
                  w_edge_attr=True, num_layers=2, bidirectional=1, agg="attn_h", out_wx=False, out_pool_all=False, out_pool="max",
                  dropout=0.0).train()
    seeded_fill(model, 6)
    model = model.to(device)
    ids = [int(i) for i in np.random.default_rng(8).permutation(43)]
    plain = st.evaluate_tok(model, ids, 16)
    res = st.evaluate_tok(model, ids, 16, loss=True)
    assert model.training
    model.eval()
    assert set(res) == set(plain) | {"loss"} and all(res[k] == plain[k] for k in plain) and res["n"] == 43
    bs = list(st.loader(ids, 16))
    want, n = _seq_loss_of(model, bs, [b.y_arr for b in bs])
    assert res["loss"] == want and n == 43 * S and math.isfinite(want)
    bs = list(st.loader(ids, 16))
    torch.cuda.synchronize()
    _, base = _sync_count(lambda: [model.score(b, b.y_arr) for b in bs])
    again, syncs = _sync_count(lambda: st.evaluate_tok(model, ids, 16, loss=True))
    assert syncs == base + 1 and again == res, (syncs, base)


def test_evaluate_lp_with_loss(device):
    from tests.test_code2_lp_gpu import _graph_range, lp_model
    meta, arr = Hh.load("code2_lp_gated_h64")
    model = lp_model(meta).to(device).train()
    make = lambda: [_graph_range(arr, 0, 5, device), _graph_range(arr, 5, meta["B"], device)]   # noqa: E731
    plain = lp.evaluate_lp(model, make())
    res = lp.evaluate_lp(model, make(), loss=True)
    assert model.training
    model.eval()
    assert set(res) == {"acc", "n", "loss"} and res["acc"] == plain["acc"] and res["n"] == plain["n"] == meta["B"]
    # the criterion of the training loop (main_pyg_lp.py:56-58) on `forward`'s logits, batch by batch
    total = 0.0
    with torch.no_grad():
        for b in make():
            targ = lp.lp_targets(b, b.num_graphs)
            total += float(lp.class_cross_entropy(model(b), targ)) * b.num_graphs
    assert abs(res["loss"] - total / meta["B"]) < 2e-4   # (logits within the parity bound: a loss within twice it)
    bs = make()
    targs = [lp.lp_targets(b, b.num_graphs) for b in bs]
    want, n = _seq_loss_of(model, bs, targs)
    assert res["loss"] == want and n == meta["B"]
    # float targets, as the reference's reader stores them: truncated as `.to(torch.long)` does
    fl = make()
    for b, t in zip(fl, targs):
        b.len_longest_path = t.double() + 0.75
    assert lp.evaluate_lp(model, fl, loss=True)["loss"] == res["loss"]
