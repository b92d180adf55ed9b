"""BIC scoring of Bayesian networks on the GPU (csrc/bn_score.hip) against the float64 oracle of tests/test_bn_score_cpu.py
(an independent restatement, see there; tolerance 1e-9 relative, justified there), the capacity rule, bitwise determinism
(run to run, under a permutation of the samples, across the two staging paths), score equivalence, dense decoder rows, a
BN `DagStore`, and `decode_and_score`.  Shapes are the smallest at which each path can go wrong: S = 1, S below / above one
pass of the 256 threads x 4 samples, S = 5000; 1, 8 and 30 variables; more structures than workgroups."""
import math
import warnings

import numpy as np
import pytest
import torch

from dagnn_amd import DagStore, bn_score, dvae, synth
from dagnn_amd.bn_score import BnData, bn_scores, decode_and_score, score_dense, score_strings, store_scores

from . import helpers as Hh
from .test_bn_score_cpu import MIXED, RTOL, close, oracle_adj, oracle_masks, random_dags, random_samples

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def same_bits(got, want):
    """Equal float64 bit patterns where finite, NaN in the same places."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.int64), want[ok].view(np.int64))


def _cards(n_var):
    return (MIXED * 4)[:n_var]


@pytest.mark.parametrize("S", [1, 63, 257, 5000])
@pytest.mark.parametrize("n_var", [1, 8, 30])
def test_scores_match_the_oracle(device, S, n_var):
    rng = np.random.default_rng(1000 * n_var + S)
    cards = _cards(n_var)
    X = random_samples(rng, S, cards)
    if n_var >= 8:
        X[:, 2] = np.minimum(X[:, 2], 2)        # a level that never occurs
        X[:, 5] = (X[:, 1] + X[:, 3]) % 3       # a deterministic column
    data = BnData.from_samples(X, cards, device=device)
    P = random_dags(rng, n_var, 3, 4)
    P[0] = 0
    want = oracle_masks(X, cards, P)
    assert data.fits_lds() == (n_var * data.ld <= 160 * 1024 - 4 * bn_score.TABLE_CELLS - 960)   # (30 x 5008 bytes do not fit)
    for stage in (None, "lds", "global") if data.fits_lds() else (None, "global"):
        scores, n_over = bn_scores(data, P, stage=stage)
        assert scores.dtype == torch.float64 and scores.device.type == "cuda" and n_over.dtype == torch.int32
        assert n_over.tolist() == [0]
        close(scores.cpu().numpy(), want)


@pytest.mark.parametrize("M", [1, 3, 5000])
def test_many_structures(device, M):
    """5000 structures are more than the grid's workgroups: every workgroup walks several."""
    rng = np.random.default_rng(M)
    X = random_samples(rng, 64, MIXED)
    data = BnData.from_samples(X, MIXED, device=device)
    P = random_dags(rng, 8, M, 3)
    scores, n_over = bn_scores(data, torch.from_numpy(P.view(np.int32)).to(device))
    close(scores.cpu().numpy(), oracle_masks(X, MIXED, P))
    assert n_over.tolist() == [0]


def test_seven_binary_parents(device):
    rng = np.random.default_rng(2)
    X = random_samples(rng, 5000, [2] * 8)
    X[:, 7] = (X[:, :7].sum(axis=1) + (rng.random(5000) < 0.2)) % 2
    data = BnData.from_samples(X, device=device)
    P = np.zeros((2, 8), dtype=np.uint32)
    P[0, 7] = 0x7F
    P[1, 3] = 0x7F & ~(1 << 3) | (1 << 7)
    for stage in ("lds", "global"):
        close(bn_scores(data, P, stage=stage)[0].cpu().numpy(), oracle_masks(X, [2] * 8, P))


def test_capacity_edge(device):
    k = int(math.log2(bn_score.TABLE_CELLS // 2))   # binary parents of a binary node that fill the table exactly (12)
    n_var = k + 2
    rng = np.random.default_rng(4)
    X = random_samples(rng, 257, [2] * n_var)
    data = BnData.from_samples(X, [2] * n_var, device=device)
    P = random_dags(rng, n_var, 4, 3)
    P[1] = 0
    P[1, n_var - 1] = (1 << k) - 1                  # exactly the capacity
    P[2] = 0
    P[2, n_var - 1] = (1 << (k + 1)) - 1            # one parent over
    want = oracle_masks(X, [2] * n_var, P[[0, 1, 3]])
    for stage in ("lds", "global"):
        scores, n_over = bn_scores(data, P, stage=stage)
        s = scores.cpu().numpy()
        assert n_over.tolist() == [1] and np.isnan(s[2])
        close(s[[0, 1, 3]], want)


def test_bitwise_determinism(device):
    rng = np.random.default_rng(6)
    S = 5000
    X = random_samples(rng, S, MIXED)
    X[:, 4] = (X[:, 4] + X[:, 0] * X[:, 1]) % 5
    P = random_dags(rng, 8, 300, 5)
    data = BnData.from_samples(X, MIXED, device=device)
    assert data.fits_lds()                          # (so 'global' below is forced at a size that would have fitted LDS)
    first = bn_scores(data, P)[0]
    again = bn_scores(data, P)[0]
    perm = BnData.from_samples(X[rng.permutation(S)], MIXED, device=device)
    lds, glob = bn_scores(data, P, stage="lds")[0], bn_scores(data, P, stage="global")[0]
    permuted = [bn_scores(perm, P, stage=st)[0] for st in ("lds", "global")]
    assert np.isfinite(first.cpu().numpy()).all()
    for other in [again, lds, glob] + permuted:
        np.testing.assert_array_equal(_bits(first), _bits(other))
    close(first.cpu().numpy()[:20], oracle_masks(X, MIXED, P[:20]))


def test_streaming_path_when_the_table_does_not_fit(device):
    rng = np.random.default_rng(8)
    cards = _cards(30)
    X = random_samples(rng, 6000, cards)            # 30 columns of 6000 bytes: beyond the LDS beside the count table
    data = BnData.from_samples(X, cards, device=device)
    assert not data.fits_lds()
    P = random_dags(rng, 30, 2, 3)
    close(bn_scores(data, P)[0].cpu().numpy(), oracle_masks(X, cards, P))
    with pytest.raises(Exception):
        bn_scores(data, P, stage="lds")


def test_covered_arc_reversal_on_the_device(device):
    rng = np.random.default_rng(3)
    for cards in ([2] * 8, MIXED):
        X = random_samples(rng, 5000, cards)
        X[:, 3] = (X[:, 3] + X[:, 0]) % cards[3]
        a, b, c, d = (np.zeros(8, dtype=np.uint32) for _ in range(4))
        a[3], b[0] = 1 << 0, 1 << 3                 # 0 -> 3 against 3 -> 0
        for m in (c, d):                            # common parent 0, common child 4
            m[1] |= 1 << 0
            m[2] |= 1 << 0
            m[4] |= (1 << 1) | (1 << 2)
        c[1] |= 1 << 2                              # 2 -> 1
        d[2] |= 1 << 1                              # 1 -> 2
        s = bn_scores(BnData.from_samples(X, cards, device=device), np.stack([a, b, c, d]))[0].cpu().numpy()
        assert abs(s[0] - s[1]) <= RTOL * abs(s[0]) and abs(s[2] - s[3]) <= RTOL * abs(s[2])


# ------------------------------------------------------------------------------------------------ dense rows
def _bn_rows(rng, R, n=10, nvt=10):
    """Random valid BN rows: START first, END last, the middle types shuffled (vertex order differs from variable order)."""
    types = np.zeros((R, n), dtype=np.int32)
    preds = np.zeros((R, n), dtype=np.uint32)
    for g in range(R):
        types[g, 1:n - 1] = 2 + rng.permutation(nvt - 2)
        types[g, n - 1] = 1
        loose = set(range(1, n - 1))
        for v in range(1, n - 1):
            m = 0
            for u in range(1, v):
                if rng.random() < 0.35:
                    m |= 1 << u
                    loose.discard(u)
            preds[g, v] = m if m else 1
        preds[g, n - 1] = sum(1 << u for u in loose)
    return types, preds.view(np.int32), np.full(R, n, dtype=np.int32)


def test_dense_rows(device):
    rng = np.random.default_rng(12)
    types, preds, nv = _bn_rows(rng, 40)
    assert all(dvae.row_valid(types[g], preds[g], nv[g], "BN", 10, 0, 1) for g in range(40))
    X = random_samples(rng, 257, MIXED)
    data = BnData.from_samples(X, MIXED, device=device)
    t = lambda a: torch.from_numpy(a).to(device)   # noqa: E731
    scores, n_over = score_dense(data, t(types), t(preds), t(nv), 10)
    strings = [dvae.bn_adj_string(types[g], preds[g], nv[g]) for g in range(40)]
    assert len(set(strings)) > 30
    same_bits(scores.cpu().numpy(), score_strings(data, strings))
    close(scores.cpu().numpy(), [oracle_adj(X, MIXED, np.array(s.split(), dtype=np.int64).reshape(8, 8)) for s in strings])
    assert n_over.tolist() == [0]
    # rows made invalid: a duplicated type, a short row
    types2, nv2 = types.copy(), nv.copy()
    types2[3, 4] = types2[3, 5]
    nv2[7] = 9
    types2[7, 9] = -1
    bad, n_over = score_dense(data, t(types2), t(preds), t(nv2), 10)
    bad = bad.cpu().numpy()
    assert np.isnan(bad[3]) and np.isnan(bad[7]) and n_over.tolist() == [0]
    keep = np.array([g for g in range(40) if g not in (3, 7)])
    np.testing.assert_array_equal(bad[keep].view(np.int64), scores.cpu().numpy()[keep].view(np.int64))


def test_store_scores(device):
    rows = synth.bn_rows(3, 50)
    store = DagStore.from_rows(rows, "BN", nvt=10, device=device)
    X = synth.asia_samples(1, 500)
    data = BnData.from_samples(X, [2] * 8, device=device)
    a = store.arrays
    nv = torch.full((50,), 10, dtype=torch.int32, device=device)
    every, _ = score_dense(data, a["types"], a["preds"], nv, 10)
    assert np.isfinite(every.cpu().numpy()).all()
    got, n_over = store_scores(data, store)
    np.testing.assert_array_equal(_bits(got), _bits(every))
    assert n_over.tolist() == [0]
    idx = [4, 4, 49, 0, 17, 4]
    np.testing.assert_array_equal(_bits(store_scores(data, store, idx)[0]), _bits(every)[idx])
    host_types, host_preds = a["types"].cpu().numpy(), a["preds"].cpu().numpy()
    strings = [dvae.bn_adj_string(host_types[g], host_preds[g], 10) for g in range(50)]
    close(every.cpu().numpy(), [oracle_adj(X, [2] * 8, np.array(s.split(), dtype=np.int64).reshape(8, 8)) for s in strings])


# ------------------------------------------------------------------------------------------------ decode_and_score
def _count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, sum("synchroniz" in str(w.message).lower() for w in seen)


def test_decode_and_score_on_a_seeded_model(device):
    model = Hh.dvae_decoder_model("bn", max_n=10, nvt=10, hs=32, L=2, seed=3).to(device)
    B, A = 6, 12
    g = torch.Generator(device=device).manual_seed(21)
    z = torch.randn(B, model.nz, device=device, generator=g)
    st, se = dvae.draw_shapes(model.max_n, B, A)
    draws = (torch.rand(st, device=device, generator=g), torch.rand(se, device=device, generator=g))
    data = BnData.from_samples(synth.asia_samples(2, 300), [2] * 8, device=device)
    want = dvae.decode_from_latent_space(z, model, A, "variable", False, "BN", draws=draws)
    decode_and_score(z, model, data, A, draws=draws)   # (warm-up)
    (strings, scores), n_sync = _count_syncs(lambda: decode_and_score(z, model, data, A, draws=draws))
    _, n_plain = _count_syncs(lambda: dvae.decode_from_latent_space(z, model, A, "variable", False, "BN", draws=draws))
    assert strings == want
    assert n_sync == n_plain and n_plain >= 1
    assert scores.dtype == np.float64 and scores.shape == (B,)
    assert [math.isnan(v) for v in scores] == [s is None for s in strings]
    same_bits(scores, score_strings(data, strings))


def test_decode_and_score_on_the_reference_rows(device):
    """The same on rows with valid and invalid attempts for certain: a stand-in model serves the `dvae_select_bn_a12`
    fixture's rows (the reference's own) from the device; the strings must be the fixture's."""
    meta, arr = Hh.load("dvae_select_bn_a12")
    A, B, n = meta["A"], meta["B"], meta["n"]
    rows = {k: torch.from_numpy(np.ascontiguousarray(arr[k])).to(device) for k in ("types", "preds", "nv")}

    class Rows(object):
        max_n, nvt, START_TYPE, END_TYPE = n, meta["nvt"], 0, 1

        def __init__(self):
            self.at = 0

        def decode_dense(self, z, stochastic, attempts, draws):
            sl = slice(self.at, self.at + attempts)
            self.at += attempts
            return dvae.DecodedDense(rows["types"][sl], rows["preds"][sl], rows["nv"][sl], None)

        def select_dense(self, d, data_type, n_nodes, select):
            return dvae.select_decoded(d, data_type, self.nvt, 0, 1, n_nodes, select)

    X = random_samples(np.random.default_rng(9), 200, MIXED)
    data = BnData.from_samples(X, MIXED, device=device)
    run = [r for r in meta["runs"] if r["n_nodes"] == "variable"][0]
    strings, scores = decode_and_score(torch.zeros(B, 4, device=device), Rows(), data, A, chunk=5)
    assert strings == run["strings"]
    assert any(s is None for s in strings) and any(s is not None for s in strings)
    assert [math.isnan(v) for v in scores] == [s is None for s in strings]
    same_bits(scores, score_strings(data, strings))
    keep = [b for b, s in enumerate(strings) if s is not None]
    close(scores[keep], [oracle_adj(X, MIXED, np.array(strings[b].split(), dtype=np.int64).reshape(8, 8)) for b in keep])
