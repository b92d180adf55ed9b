"""`DAGNN.score`, host tier: the numpy definition `evaluate.heads_score_host` against torch float64 `logsumexp` /
`cross_entropy` / a stable descending sort, its special-value table, the torch composition `score` falls back to, the
accumulator, the argument checks of `dagnn_heads_score` that need no device, and the fixtures made by the reference
(tests/golden/make_golden_code2_score.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dagnn_amd import _lib, evaluate
from tests import helpers as Hh

SCORE_FIXTURES = {"code2_score_b64_h64": "code2_eval_b64_h64", "code2_score_unidir_wx": "code2_eval_unidir_wx",
                  "code2_score_numclass": "code2_eval_numclass"}
TAU = 2e-4
NAN, INF = float("nan"), float("inf")


def _case(B, D, S, V, seed):
    g = torch.Generator().manual_seed(seed)
    out = torch.rand(B, D, generator=g) * 2 - 1
    w = (torch.rand(S * V, D, generator=g) * 2 - 1) / D ** 0.5
    b = torch.rand(S * V, generator=g) * 2 - 1
    y = torch.randint(0, V, (B, S), generator=g)
    return out, w, b, y


@pytest.mark.parametrize("B,D,S,V,k", [(3, 7, 1, 1, 1), (5, 6, 2, 3, 8), (9, 20, 5, 129, 3), (4, 64, 3, 301, 8)])
def test_host_mirror_against_torch_float64(B, D, S, V, k):
    out, w, b, y = _case(B, D, S, V, 100 * V + k)
    got = evaluate.heads_score_host(out, w, b, S, V, y=y, k=k)
    x = (out.double() @ w.double().t() + b.double()).view(B, S, V)
    np.testing.assert_allclose(got["logits"], x.numpy(), rtol=0, atol=1e-14)   # (two float64 GEMMs: the last bit may differ)
    x = torch.from_numpy(got["logits"])
    np.testing.assert_allclose(got["lse"], torch.logsumexp(x, dim=2).numpy(), rtol=0, atol=1e-13)
    ce = torch.nn.functional.cross_entropy(x.reshape(B * S, V), y.reshape(-1), reduction="none").view(B, S)
    np.testing.assert_allclose(got["nll"], ce.numpy(), rtol=0, atol=1e-13)
    srt = torch.sort(x, dim=2, descending=True, stable=True)
    n = min(k, V)
    np.testing.assert_array_equal(got["tok"][:, :, :n], srt.indices[:, :, :n].numpy())
    np.testing.assert_array_equal(got["logit"][:, :, :n], srt.values[:, :, :n].numpy())
    assert (got["tok"][:, :, n:] == -1).all() and np.isneginf(got["logit"][:, :, n:]).all()
    assert got["tok"].shape == (B, S, k) and got["tok"].dtype == np.int64
    assert evaluate.heads_score_host(out, w, b, S, V, k=k)["nll"] is None


def _table():
    """One head of V = 6 per row, logits planted through the bias (zero weights): (bias row, lse, columns by rank)."""
    return [
        ([1.0, NAN, 3.0, NAN, INF, 2.0], NAN, [1, 3, 4, 2, 5, 0]),           # NaN first, by column; then +inf
        ([1.0, INF, 3.0, INF, -INF, 2.0], INF, [1, 3, 2, 5, 0, 4]),          # +inf wins the sum; -inf last
        ([-INF] * 6, -INF, [0, 1, 2, 3, 4, 5]),                              # a row of -inf alone
        ([0.0, -0.0, -1.0, 0.0, -0.0, -2.0], math.log(4 + math.exp(-1) + math.exp(-2)), [0, 1, 3, 4, 2, 5]),   # -0 == +0
        ([5.0, 5.0, 5.0, 5.0, 5.0, 5.0], 5.0 + math.log(6.0), [0, 1, 2, 3, 4, 5]),   # ties: the lowest column at every rank
        ([-INF, 2.0, -INF, 2.0, -INF, -INF], 2.0 + math.log(2.0), [1, 3, 0, 2, 4, 5]),
    ]


def test_host_mirror_special_values():
    rows = _table()
    V, B = 6, len(rows)
    out = torch.zeros(B, 4)
    w = torch.zeros(V, 4)
    y = np.array([[0], [5], [2], [1], [3], [1]])
    for r, (bias, lse, cols) in enumerate(rows):
        got = evaluate.heads_score_host(out[r:r + 1], w, torch.tensor(bias), 1, V, y=y[r:r + 1], k=8)
        assert got["tok"][0, 0].tolist() == cols + [-1, -1], r
        assert np.isneginf(got["logit"][0, 0, 6:]).all()
        want = torch.logsumexp(torch.tensor(bias, dtype=torch.float64), dim=0).item()
        for v in (got["lse"][0, 0], want):
            assert (math.isnan(lse) and math.isnan(v)) or v == pytest.approx(lse, abs=1e-14), (r, v, lse)
        with np.errstate(invalid="ignore"):
            nll = lse - np.float64(np.float32(bias[int(y[r, 0])]))
        assert (np.isnan(nll) and np.isnan(got["nll"][0, 0])) or got["nll"][0, 0] == pytest.approx(nll, abs=1e-14), r
    # a target outside [0, V) poisons its own row and nothing else
    out, w, b, y = _case(4, 5, 2, 6, 3)
    y[1, 0], y[2, 1] = -1, 6
    got = evaluate.heads_score_host(out, w, b, 2, 6, y=y, k=2)
    bad = np.zeros((4, 2), dtype=bool)
    bad[1, 0] = bad[2, 1] = True
    assert np.array_equal(np.isnan(got["nll"]), bad) and np.isfinite(got["lse"]).all()


def test_torch_composition_follows_the_same_rules():
    """`evaluate.rows_score`: what `score` composes where the heads are not plain fp32 GPU `nn.Linear`."""
    rows = _table()
    x = torch.tensor([r[0] for r in rows])
    tok, logit, lse, nll = evaluate.rows_score([x], torch.tensor([0, 5, 2, 1, 3, 9]), 8)
    assert tok[:, 0, :6].tolist() == [r[2] for r in rows] and (tok[:, 0, 6:] == -1).all()
    assert torch.isneginf(logit[:, 0, 6:]).all() and torch.isnan(logit[0, 0, :2]).all() and logit[0, 0, 2] == INF
    for r, (_, want, _) in enumerate(rows):
        assert (math.isnan(want) and math.isnan(float(lse[r, 0]))) or float(lse[r, 0]) == pytest.approx(want, abs=1e-5)
    assert math.isnan(float(nll[5, 0])) and float(nll[4, 0]) == pytest.approx(math.log(6.0), abs=1e-6)
    out, w, b, y = _case(7, 12, 3, 40, 8)
    pred = list(torch.addmm(b, out, w.t()).split(40, dim=1))
    host = evaluate.heads_score_host(out, w, b, 3, 40, y=y, k=3)
    tok, logit, lse, nll = evaluate.rows_score(pred, y, 3)
    np.testing.assert_array_equal(tok.numpy(), host["tok"])
    np.testing.assert_allclose(logit.numpy(), host["logit"], atol=1e-5)
    np.testing.assert_allclose(lse.numpy(), host["lse"], atol=1e-5)
    np.testing.assert_allclose(nll.numpy(), host["nll"], atol=1e-5)
    s = evaluate.Score(tok, logit, lse, nll)
    assert torch.equal(s.logprob, logit - lse.unsqueeze(-1)) and float(s.loss) == pytest.approx(float(nll.mean()))
    want = sum(torch.nn.functional.cross_entropy(p, y[:, i]) for i, p in enumerate(pred)) / 3
    assert float(s.loss) == pytest.approx(float(want), abs=1e-5)
    with pytest.raises(ValueError, match="without targets"):
        evaluate.Score(tok, logit, lse).loss


class _Head(torch.nn.Module):
    """A head that is no `nn.Linear`: `score` must take `_heads` + torch ops."""

    def __init__(self, lin):
        super().__init__()
        self.lin = lin

    def forward(self, x):
        return self.lin(x)


def test_score_fallback_on_the_pooled_vectors_and_its_refusals():
    meta, _ = Hh.load("code2_eval_numclass")
    model = Hh.code2_model(meta)
    model.graph_pred_linear = _Head(model.graph_pred_linear)
    g = torch.Generator().manual_seed(5)
    out = torch.rand(9, model.graph_pred_linear.lin.weight.shape[1], generator=g)
    y = torch.randint(0, 17, (9,), generator=g)
    acc = evaluate.SeqLoss("cpu")
    tok, logit, lse, nll = model._heads_score(out, y, 3, acc)
    lin = model.graph_pred_linear.lin
    host = evaluate.heads_score_host(out, lin.weight, lin.bias, 1, 17, y=y.view(-1, 1), k=3)
    assert tuple(tok.shape) == (9, 1, 3) and tuple(nll.shape) == (9, 1)
    np.testing.assert_array_equal(tok.numpy(), host["tok"])
    np.testing.assert_allclose(nll.numpy(), host["nll"], atol=1e-5)
    res = acc.compute()
    assert res["rows"] == 9 and res["loss"] == pytest.approx(float(nll.double().mean()), abs=1e-12)
    with pytest.raises(ValueError, match="targets"):
        model._heads_score(out, y[:5], 1, None)
    with pytest.raises(ValueError, match="topk"):
        model.score(object(), topk=9)
    with pytest.raises(ValueError, match="targets needed"):
        model.score(object(), sums=acc)
    model.train()
    with pytest.raises(RuntimeError, match="evaluation pass"):
        model.score(object())
    with pytest.raises(ValueError, match="no row"):
        evaluate.SeqLoss("cpu").compute()


# ----------------------------------------------------------------------------- the C entry point's argument checks
def test_heads_score_refuses_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    EINVAL, ENOSPC = -22, -28
    nbytes = lib.dagnn_heads_score_bytes
    per = lambda kt: 8 * kt + 16   # noqa: E731  (a partial: kt packed keys, maximum, sum, target logit, pad)
    assert nbytes(128, 5, 5002, 1) == 16 + 128 * 5 * 40 * per(1) and nbytes(128, 5, 5002, 8) == 16 + 128 * 5 * 40 * per(8)
    assert nbytes(1, 1, 1, 3) == 16 + per(4) and nbytes(1, 1, 1, 5) == 16 + per(8) and nbytes(0, 5, 48, 2) > 0
    assert nbytes(4, 5, 48, 0) == 0 and nbytes(4, 5, 48, 9) == 0 and nbytes(-1, 5, 48, 1) == 0 and nbytes(4, 0, 48, 1) == 0
    assert nbytes(4, 5, 0, 1) == 0 and nbytes(4, 1 << 16, 1 << 16, 1) == 0
    p = C.c_void_p(4096)   # a non-null, 16-byte aligned address nothing dereferences: every call below returns before a launch
    h = lib.dagnn_heads_score
    big = 1 << 20
    assert h(p, 64, p, 64, p, 0, 64, 5, 48, p, 3, p, p, p, p, p, p, big, None) == 0                  # B = 0 returns at once
    assert h(None, 64, None, 64, None, 0, 64, 5, 48, None, 1, None, None, None, None, None, None, 0, None) == 0
    assert h(p, 64, p, 64, p, 4, 64, 5, 48, p, 0, p, p, p, p, None, p, big, None) == EINVAL           # k outside 1..8
    assert h(p, 64, p, 64, p, 4, 64, 5, 48, p, 9, p, p, p, p, None, p, big, None) == EINVAL
    assert h(p, 64, p, 64, p, 0, 64, 5, 48, p, 9, p, p, p, p, None, p, big, None) == EINVAL
    assert h(p, 64, p, 64, p, 4, 64, 5, 48, p, 1, p, p, p, None, None, p, big, None) == EINVAL        # y without nll
    assert h(p, 64, p, 64, p, 4, 64, 5, 48, None, 1, p, p, p, p, None, p, big, None) == EINVAL        # nll without y
    assert h(p, 64, p, 64, p, 4, 64, 5, 48, None, 1, p, p, p, None, p, p, big, None) == EINVAL        # sums without y
    assert h(p, 64, p, 64, p, 4, 64, 5, 48, p, 1, p, p, p, p, C.c_void_p(4100), p, big, None) == EINVAL   # misaligned sums
    assert h(p, 64, p, 64, p, 4, 64, 5, 48, p, 1, p, p, p, p, None, C.c_void_p(4104), big, None) == EINVAL   # misaligned scratch
    for hole in (0, 2, 4, 11, 12, 13, 16):                                                             # null pointers
        args = [p, 64, p, 64, p, 4, 64, 5, 48, None, 1, p, p, p, None, None, p, big, None]
        args[hole] = None
        assert h(*args) == EINVAL, hole
    assert h(p, 63, p, 64, p, 4, 64, 5, 48, None, 1, p, p, p, None, None, p, big, None) == EINVAL     # row pitch below D
    assert h(p, 64, p, 60, p, 4, 64, 5, 48, None, 1, p, p, p, None, None, p, big, None) == EINVAL
    assert h(p, 64, p, 64, p, 4, 0, 5, 48, None, 1, p, p, p, None, None, p, big, None) == EINVAL
    assert h(p, 64, p, 64, p, -1, 64, 5, 48, None, 1, p, p, p, None, None, p, big, None) == EINVAL
    assert h(p, 64, p, 64, p, 4, 64, 0, 48, None, 1, p, p, p, None, None, p, big, None) == EINVAL
    assert h(p, 64, p, 64, p, 4, 64, 5, 0, None, 1, p, p, p, None, None, p, big, None) == EINVAL
    assert h(p, 64, p, 64, p, 4, 64, 5, 48, None, 3, p, p, p, None, None, p, nbytes(4, 5, 48, 3) - 1, None) == ENOSPC


# ----------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", sorted(SCORE_FIXTURES))
def test_score_fixture_integrity(name):
    meta, arr = Hh.load(name)
    src_meta, src = Hh.load(SCORE_FIXTURES[name])
    assert meta["source"] == SCORE_FIXTURES[name] and meta["tau"] == TAU and meta["k"] == 8
    B, S, V = src_meta["B"], src_meta["heads"], src_meta["width"]
    assert (meta["B"], meta["heads"], meta["width"]) == (B, S, V)
    val, col, clear = arr["top_val"].astype(np.float64), arr["top_col"], arr["clear"]
    assert val.shape == col.shape == clear.shape == (B, S, 8) and arr["lse"].shape == arr["nll"].shape == arr["y"].shape == (B, S)
    assert arr["lse"].dtype == np.float64 and arr["nll"].dtype == np.float64 and clear.dtype == np.bool_
    # the same reference run as the evaluation fixture: its winners and its three best logits
    np.testing.assert_array_equal(col[:, :, 0][clear[:, :, 0]], src["tok"][clear[:, :, 0]])
    np.testing.assert_array_equal(val[:, :, :3], src["top_val"].astype(np.float64))
    assert (np.diff(val, axis=2) <= 0).all() and (col >= 0).all() and (col < V).all()
    assert all(len(set(c)) == 8 for c in col.reshape(-1, 8).tolist())
    gap = val[:, :, :-1] - val[:, :, 1:]
    assert not (clear[:, :, :-1] & (gap <= TAU)).any() and not (clear[:, :, 1:] & (gap <= TAU)).any()
    assert float((~clear).mean()) <= 0.02 and float((~clear).mean()) == pytest.approx(meta["ambiguous"])
    # lse bounds every logit from above and the 8 best from their own sum; nll is lse minus a logit no greater than the best
    assert (arr["lse"] >= val[:, :, 0]).all()
    assert (arr["lse"] >= np.log(np.exp(val - val[:, :, :1]).sum(axis=2)) + val[:, :, 0] - 1e-12).all()
    assert (arr["lse"] <= val[:, :, 0] + np.log(V)).all()
    y, nll = arr["y"], arr["nll"]
    assert (y >= 0).all() and (y < V).all() and (nll >= arr["lse"] - val[:, :, 0] - 1e-12).all()
    own = y == col[:, :, 0]
    assert 0.4 <= own.mean() <= 0.7
    np.testing.assert_allclose(nll[own], (arr["lse"] - val[:, :, 0])[own], rtol=0, atol=1e-12)
