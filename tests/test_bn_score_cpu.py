"""BIC scoring of Bayesian networks (dagnn_amd/bn_score.py), the tier that needs no GPU: the module's numpy mirror against
an independent float64 restatement written here, mathematical properties of the score, the string interface on the
reference's own `decode_igraph_to_BN_adj` strings (the `dvae_select_bn_*` fixtures), the pack-time checks and the C ABI.

The oracle below is the anchor of this file and of tests/test_bn_score_gpu.py.  It is not imported from the package and
is worded differently from both the kernel and the mirror: it takes an adjacency matrix (not masks), codes a parent
configuration with `np.ravel_multi_index`, and computes the log-likelihood as  sum N_ijk log N_ijk - sum N_ij log N_ij
from two `np.bincount`s per family instead of  sum N_ijk (log N_ijk - log N_ij).

Tolerance |diff| <= 1e-9 |score| everywhere: a score is a sum of at most 30 * capacity terms, each rounded to a few ulp of
float64 (1.1e-16 relative); even if every rounding error had the same sign that is about 1e-11 relative, two orders below
the bound.
"""
import math

import numpy as np
import pytest
import torch

from dagnn_amd import _lib, bn_score, dvae
from dagnn_amd.bn_score import BnData, BnEvaluator, scores_host, score_strings

from . import helpers as Hh

MIXED = [2, 3, 4, 2, 5, 3, 2, 2]
RTOL = 1e-9


# ------------------------------------------------------------------------------------------------ the oracle
def _xlogx_sum(counts):
    c = counts[counts > 0].astype(np.float64)
    return float(np.sum(c * np.log(c)))


def oracle_adj(samples, cards, adj):
    """BIC of the structure adj (adj[j, i] == 1: arc j -> i) on samples [S, n_var], float64."""
    X = np.asarray(samples, dtype=np.int64)
    cards = np.asarray(cards, dtype=np.int64)
    S, n = X.shape
    score = 0.0
    for i in range(n):
        pa = np.flatnonzero(np.asarray(adj)[:, i])
        if pa.size:
            q = int(np.prod(cards[pa]))
            code = np.ravel_multi_index(tuple(X[:, j] for j in pa), tuple(int(cards[j]) for j in pa))
        else:
            q, code = 1, np.zeros(S, dtype=np.int64)
        joint = np.bincount(code * cards[i] + X[:, i], minlength=q * int(cards[i]))
        marg = np.bincount(code, minlength=q)
        score += _xlogx_sum(joint) - _xlogx_sum(marg) - 0.5 * math.log(S) * q * (int(cards[i]) - 1)
    return score


def adj_of_masks(masks):
    n = len(masks)
    adj = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            adj[j, i] = int(masks[i]) >> j & 1
    return adj


def oracle_masks(samples, cards, parents):
    return np.array([oracle_adj(samples, cards, adj_of_masks(p)) for p in np.asarray(parents)])


def random_dags(rng, n_var, M, max_parents):
    """Parent masks uint32 [M, n_var] of random DAGs: arcs only from earlier to later in a random order."""
    out = np.zeros((M, n_var), dtype=np.uint32)
    for m in range(M):
        order = rng.permutation(n_var)
        for pos in range(1, n_var):
            k = int(rng.integers(0, min(pos, max_parents) + 1))
            for j in rng.choice(order[:pos], size=k, replace=False):
                out[m, order[pos]] |= np.uint32(1 << int(j))
    return out


def random_samples(rng, S, cards):
    return np.stack([rng.integers(0, r, size=S) for r in cards], axis=1).astype(np.int64)


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.isfinite(want).all()
    diff = np.abs(got - want)
    assert (diff <= RTOL * np.abs(want)).all(), (float(diff.max()), got[np.argmax(diff)], want[np.argmax(diff)])


def cases():
    rng = np.random.default_rng(7)
    out = {}
    out["mixed"] = (random_samples(rng, 500, MIXED), MIXED)
    X = random_samples(rng, 300, MIXED)
    X[:, 2] = np.minimum(X[:, 2], 2)                       # level 3 of x_2 never occurs but counts in r_2 = 4
    out["unobserved_level"] = (X, MIXED)
    X = random_samples(rng, 400, [2] * 8)
    X[:, 5] = X[:, 2] | X[:, 3]
    out["deterministic"] = (X, [2] * 8)
    out["one_variable"] = (random_samples(rng, 200, [3]), [3])
    out["one_sample"] = (random_samples(rng, 1, MIXED), MIXED)
    return out


CASES = cases()


# ------------------------------------------------------------------------------------------------ mirror against oracle
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_mirror_matches_the_oracle(name):
    X, cards = CASES[name]
    rng = np.random.default_rng(11)
    P = random_dags(rng, X.shape[1], 12, 4)
    P[0] = 0
    close(scores_host(X, cards, P), oracle_masks(X, cards, P))


def test_host_mirror_counts_every_level_and_configuration():
    X, cards = CASES["unobserved_level"]
    P = np.zeros((2, 8), dtype=np.uint32)
    P[1, 0] = 1 << 2                                       # x_2 (4 levels, 3 seen) as a parent: q counts all 4
    got = scores_host(X, cards, P)
    close(got, oracle_masks(X, cards, P))
    seen = BnData.from_samples(X, device="cpu")            # cards from the data: r_2 = 3
    assert seen.cards[2] == 3
    assert got[0] < scores_host(X, seen.cards, P[:1])[0]   # the unseen level costs penalty


def test_covered_arc_reversal_leaves_the_score_unchanged():
    rng = np.random.default_rng(3)
    for cards in ([2] * 8, MIXED):
        X = random_samples(rng, 5000, cards)
        X[:, 3] = (X[:, 3] + X[:, 0]) % cards[3]           # (some dependence, so the arcs matter)
        a, b = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
        a[3], b[0] = 1 << 0, 1 << 3                        # 0 -> 3 against 3 -> 0
        c, d = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
        for m in (c, d):                                   # common parent 0 and common child 4 of vertices 1 and 2
            m[1] |= 1 << 0
            m[2] |= 1 << 0
            m[4] |= (1 << 1) | (1 << 2)
        c[1] |= 1 << 2                                     # 2 -> 1
        d[2] |= 1 << 1                                     # 1 -> 2
        s = scores_host(X, cards, np.stack([a, b, c, d]))
        assert abs(s[0] - s[1]) <= RTOL * abs(s[0]) and abs(s[2] - s[3]) <= RTOL * abs(s[2])
        assert s[0] != scores_host(X, cards, np.zeros((1, 8), dtype=np.uint32))[0]


def test_empty_graph_has_the_closed_form():
    X, cards = CASES["mixed"]
    S = X.shape[0]
    want = 0.0
    for i, r in enumerate(cards):
        n = np.bincount(X[:, i], minlength=r).astype(np.float64)
        want += float(np.sum(n[n > 0] * np.log(n[n > 0] / S))) - 0.5 * math.log(S) * (r - 1)
    close(scores_host(X, cards, np.zeros((1, 8), dtype=np.uint32)), [want])


def test_over_capacity_is_nan_in_the_mirror():
    k = int(math.log2(bn_score.TABLE_CELLS // 2))
    X = random_samples(np.random.default_rng(0), 50, [2] * (k + 2))
    P = np.zeros((2, k + 2), dtype=np.uint32)
    P[0, k + 1] = (1 << k) - 1                             # k binary parents of a binary node: exactly the capacity
    P[1, k + 1] = (1 << (k + 1)) - 1
    got = scores_host(X, [2] * (k + 2), P)
    close(got[:1], oracle_masks(X, [2] * (k + 2), P[:1]))
    assert np.isnan(got[1])
    s, n_over = bn_score.bn_scores(BnData.from_samples(X, [2] * (k + 2), device="cpu"), P)
    assert s.dtype == torch.float64 and n_over.dtype == torch.int32 and n_over.tolist() == [1]


# ------------------------------------------------------------------------------------------------ strings
def _fixture_strings():
    out = []
    for name in ("dvae_select_bn_a12", "dvae_select_bn_a500"):
        meta, _ = Hh.load(name)
        assert meta["nvt"] == 10
        for run in meta["runs"]:
            out += [s for s in run["strings"] if s is not None]
    return sorted(set(out))


def test_evaluator_on_the_reference_strings():
    strings = _fixture_strings()
    assert len(strings) >= 8
    X = random_samples(np.random.default_rng(5), 700, MIXED)
    data = BnData.from_samples(X, MIXED, device="cpu")
    ev = BnEvaluator(data)
    want = [oracle_adj(X, MIXED, np.array(s.split(), dtype=np.int64).reshape(8, 8)) for s in strings]
    assert len(set(np.round(want, 6))) > 1
    got = [ev.eval(s) for s in strings[:16]]
    assert all(isinstance(v, float) for v in got)
    close(got, want[:16])
    close(score_strings(data, strings), want)
    mixed = score_strings(data, [None, strings[0], None])
    assert math.isnan(mixed[0]) and math.isnan(mixed[2]) and mixed[1] == got[0]
    assert score_strings(data, []) == []


def test_string_errors():
    X = random_samples(np.random.default_rng(5), 40, [2, 2, 2])
    ev = BnEvaluator(BnData.from_samples(X, device="cpu"))
    assert isinstance(ev.eval("0 1 0 0 0 1 0 0 0"), float)
    for bad in ("0 1 0 0", "0 1 0 0 0 1 0 0 0 0", "0 2 0 0 0 1 0 0 0", "0 -1 0 0 0 1 0 0 0", "0 x 0 0 0 1 0 0 0",
                "0 1 0 1 0 0 0 0 0", "1 0 0 0 0 0 0 0 0", "0 1 0 0 0 1 1 0 0"):   # length, entries, 2-cycle, loop, 3-cycle
        with pytest.raises(ValueError):
            ev.eval(bad)
    k = int(math.log2(bn_score.TABLE_CELLS // 2)) + 1      # one binary parent too many
    n = k + 1
    big = BnEvaluator(BnData.from_samples(random_samples(np.random.default_rng(1), 20, [2] * n), [2] * n, device="cpu"))
    adj = np.zeros((n, n), dtype=np.int64)
    adj[:k, k] = 1
    with pytest.raises(ValueError, match="capacity"):
        big.eval(" ".join(str(v) for v in adj.reshape(-1)))
    adj[0, k] = 0
    assert math.isfinite(big.eval(" ".join(str(v) for v in adj.reshape(-1))))


# ------------------------------------------------------------------------------------------------ packing
def test_pack_time_checks():
    X = random_samples(np.random.default_rng(2), 30, MIXED)
    d = BnData.from_samples(X, device="cpu")
    assert d.cards.tolist() == (X.max(axis=0) + 1).tolist() and (d.S, d.n_var, d.ld) == (30, 8, 32)
    cols = d.cols.numpy()
    assert cols.dtype == np.uint8 and cols.shape == (8, 32)
    np.testing.assert_array_equal(cols[:, :30], X.T)
    assert not cols[:, 30:].any()
    assert BnData.from_samples(torch.from_numpy(X), MIXED, device="cpu").cards.tolist() == MIXED
    with pytest.raises(ValueError):
        BnData.from_samples(X.astype(np.float64), device="cpu")
    with pytest.raises(ValueError):
        BnData.from_samples(X - 1, device="cpu")
    with pytest.raises(ValueError):
        BnData.from_samples(X, [2, 3, 4, 2, 5, 3, 2, 1], device="cpu")          # a value beyond its cardinality
    with pytest.raises(ValueError):
        BnData.from_samples(X, MIXED[:7], device="cpu")
    with pytest.raises(ValueError):
        BnData.from_samples(np.zeros((5, 31), dtype=np.int64), device="cpu")    # n_var <= 30
    with pytest.raises(ValueError):
        BnData.from_samples(np.full((5, 2), 255, dtype=np.int64), device="cpu")  # r_i <= 255
    with pytest.raises(ValueError):
        BnData.from_samples(X, [256] + MIXED[1:], device="cpu")
    with pytest.raises(ValueError):
        BnData.from_samples(np.zeros((0, 3), dtype=np.int64), device="cpu")
    assert BnData.from_samples(np.full((5, 2), 254, dtype=np.int64), device="cpu").cards.tolist() == [255, 255]
    with pytest.raises(ValueError):
        bn_score.bn_scores(d, np.zeros((2, 7), dtype=np.uint32))
    with pytest.raises(ValueError):
        bn_score.bn_scores(d, np.zeros((2, 8), dtype=np.float32))
    with pytest.raises(ValueError):
        bn_score.bn_scores(d, np.zeros((2, 8), dtype=np.uint32), stage="registers")
    with pytest.raises(ValueError):
        bn_score.score_dense(d, np.zeros((1, 10), np.int32), np.zeros((1, 10), np.int32), np.full(1, 10, np.int32), nvt=9)


def test_dense_rows_on_the_host_follow_the_strings():
    """The CPU path of score_dense (rows -> masks by the numpy mirror of the rows kernel) against the strings."""
    meta, arr = Hh.load("dvae_select_bn_a12")
    types, preds, nv = (arr[k].reshape((-1,) + arr[k].shape[2:]) for k in ("types", "preds", "nv"))
    X = random_samples(np.random.default_rng(9), 200, MIXED)
    data = BnData.from_samples(X, MIXED, device="cpu")
    scores, n_over = bn_score.score_dense(data, types, preds, nv, 10)
    valid = np.array([dvae.row_valid(types[g], preds[g], nv[g], "BN", 10, 0, 1) for g in range(len(nv))])
    assert valid.any() and not valid.all() and n_over.tolist() == [0]
    np.testing.assert_array_equal(np.isnan(scores.numpy()), ~valid)
    want = score_strings(data, [dvae.bn_adj_string(types[g], preds[g], nv[g]) if valid[g] else None for g in range(len(nv))])
    np.testing.assert_array_equal(scores.numpy()[valid], np.array(want)[valid])


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_mirror_and_argument_checks():
    lib = _lib.load()
    for name in ("dagnn_bn_stage_fits", "dagnn_bn_score", "dagnn_bn_rows_to_parents"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert (_lib.BN_TABLE_CELLS, _lib.BN_MAX_VARS) == (bn_score.TABLE_CELLS, bn_score.MAX_VARS)

    a = 4096   # (never dereferenced: every call below is refused on the host, before any HIP call)

    def desc(n_var=8, S=100, ld=112, cols=a, card=2):
        d = _lib.BnData()
        d.cols, d.ld, d.S, d.n_var = cols, ld, S, n_var
        for i in range(min(max(n_var, 0), _lib.BN_MAX_VARS)):
            d.cards[i] = card
        return d

    good = desc()
    assert lib.dagnn_bn_stage_fits(good) == 1
    assert lib.dagnn_bn_stage_fits(desc(n_var=30, S=8000, ld=8000)) == 0
    assert lib.dagnn_bn_stage_fits(None) == -22
    bad = [desc(n_var=0), desc(n_var=31), desc(S=0), desc(S=1 << 31, ld=1 << 31), desc(ld=96), desc(ld=120), desc(cols=None),
           desc(cols=a + 8), desc(card=0), desc(card=256)]
    for d in bad:
        assert lib.dagnn_bn_stage_fits(d) == -22
        assert lib.dagnn_bn_score(d, a, None, 1, 0, a, a, None) == -22
    score = lambda d=good, p=a, M=1, stage=0, s=a, o=a: lib.dagnn_bn_score(d, p, None, M, stage, s, o, None)   # noqa: E731
    assert score(d=None) == -22 and score(p=None) == -22 and score(s=None) == -22 and score(o=None) == -22
    assert score(M=-1) == -22 and score(M=1 << 31) == -22 and score(stage=3) == -22 and score(stage=-1) == -22
    assert score(d=desc(n_var=30, S=8000, ld=8000), stage=_lib.BN_STAGE_LDS) == -22     # forced staging of a table that does not fit
    assert score(M=0, p=None, s=None, o=None) == 0                                      # nothing to do, nothing launched
    rows = lambda t=a, p=a, k=a, R=1, n=10, nvt=10, st=0, en=1, out=a, v=a: lib.dagnn_bn_rows_to_parents(   # noqa: E731
        t, p, k, R, n, nvt, st, en, out, v, None)
    assert rows(t=None) == -22 and rows(p=None) == -22 and rows(k=None) == -22 and rows(out=None) == -22 and rows(v=None) == -22
    assert rows(R=-1) == -22 and rows(n=33) == -22 and rows(n=2, nvt=2) == -22 and rows(nvt=11) == -22 and rows(nvt=2) == -22
    assert rows(st=-1) == -22 and rows(en=10) == -22 and rows(st=1, en=1) == -22
    assert rows(R=0, t=None, p=None, k=None, out=None, v=None) == 0
