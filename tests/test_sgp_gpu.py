"""The sparse GP's HIP path (csrc/sgp.hip: dagnn_sgp_project, dagnn_sgp_ei_step) on the GPU against float64.

No fixture can come from the reference (its sparse GP is Theano code, which does not run here); the yardstick is the float64
restatement of tests/test_sgp_cpu.py (explicit inverses, re-inverted Kzz_expanded).

Tolerance of everything that goes through fp32 (DESIGN.md 4i's convention): the error of torch's own fp32 evaluation of the
same whitened formula, on the same device and the same fp32 operands, against float64 - times 4, floored at 4 ulp of the
result's scale (sf for a variance, the largest |mean| for a mean).  Both errors are measured and printed by every test.
Shapes are those at which a code path begins: N around the 32-row tile and the 64-row argmin block, M around the 32-column
MFMA tile and the 256-thread kernel builder, d around the 64 lanes of the greedy step, a row pitch above d."""
import math

import numpy as np
import pytest
import torch

from dagnn_amd import _lib, engine, sgp, synth
from dagnn_amd.bn_score import BnData, score_strings

from . import helpers as Hh
from .test_sgp_cpu import make, ref_greedy_var, ref_kernel, ref_log_ei, ref_predict

pytestmark = pytest.mark.gpu

ULP32 = float(np.finfo(np.float32).eps)
_MODELS = {}


def model(d, M, device):
    """One model per shape for the whole module (derived once; nothing below changes its parameters)."""
    key = (d, M)
    if key not in _MODELS:
        g, P, rng = make(d, M, n=max(40, M + 20), device=device)
        _MODELS[key] = (g, P)
    return _MODELS[key]


def pitched(X: np.ndarray, device) -> torch.Tensor:
    """The rows as an fp32 view with a row pitch above d (a multiple of 4 floats: read in place)."""
    N, d = X.shape
    buf = torch.full((N, (d + 3) // 4 * 4 + 4), float("nan"), dtype=torch.float32, device=device)
    buf[:, :d] = torch.from_numpy(X).to(device, torch.float32)
    return buf[:, :d]


def torch_fp32(D, X32):
    """The whitened formula on torch ops in fp32: (mean, var0 = sf - |G k|^2, var1 = sf - |W k|^2, U = k W^T)."""
    M = D.M
    z = D.zt.T
    df = X32[:, None, :] - z[None, :, :]
    K = D.sf * torch.exp(-0.5 * (df * df * D.inv_ls32).sum(-1))
    T = K @ D.Tt
    return K @ D.a32, D.sf - (T[:, :M] ** 2).sum(1), D.sf - (T[:, M:] ** 2).sum(1), T[:, M:]


def tol4(name, got, want, base, scale):
    """4x the error of `base` (torch fp32) against `want` (float64), floored at 4 ulp of `scale`."""
    e_got, e_base = float(np.abs(got - want).max()), float(np.abs(base - want).max())
    tol = max(4.0 * e_base, 4.0 * ULP32 * scale)
    print("%s: kernel err %.3g, torch fp32 err %.3g (ratio %.2f), tol %.3g" % (name, e_got, e_base, e_got / max(e_base, 1e-300), tol))
    return e_got, tol


CASES = sorted(set([(N, 33, 3) for N in (1, 63, 64, 65, 257)] + [(65, M, 3) for M in (1, 7, 32, 33)] +
                   [(65, 33, d) for d in (1, 3, 56, 57)] + [(257, 500, 56), (65, 500, 57)]))


@pytest.mark.parametrize("N,M,d", CASES)
def test_project_and_predict_against_float64(device, N, M, d):
    g, P = model(d, M, device)
    D = g.derived()
    rng = np.random.RandomState(N + M + d)
    X = (0.7 * rng.randn(N, d)).astype(np.float32).astype(np.float64)
    Xv = pitched(X, device)
    assert Xv.stride(0) > d
    m64, v64 = ref_predict(P, X)
    assert v64.min() > 0
    r64 = ref_greedy_var(P, X, X[:0])
    tm, tv0, tv1, tU = (t.double().cpu().numpy() for t in torch_fp32(D, Xv.contiguous()))
    mscale = max(float(np.abs(m64).max()), 1e-30)
    # T stacked: G and W in one launch, the W half stored with a pitch
    U = torch.full((N, M + 5), float("nan"), dtype=torch.float32, device=device)
    mean, var0, var1 = engine.sgp_project(Xv, D.zt, D.inv_ls32, D.sf, D.Tt, 2 * M, M, D.a32, U=U, u_col0=M, want_var0=True,
                                          want_var1=True)
    for name, got, want, base, scale in (("mean", mean, m64, tm, mscale), ("var0", var0, v64, tv0, D.sf), ("var1", var1, r64, tv1, D.sf)):
        e, tol = tol4("stacked %s" % name, got.double().cpu().numpy(), want, base, scale)
        assert e <= tol
    assert torch.isnan(U[:, M:]).all()
    U64 = ref_kernel(P[0], P[1], X, P[2]) @ D.W.T
    e, tol = tol4("stacked U", U[:, :M].double().cpu().numpy(), U64, tU, float(np.abs(U64).max()))
    assert e <= tol
    # T single (the G half alone): the same bits for the mean and var0
    mean1, var01, none = engine.sgp_project(Xv, D.zt, D.inv_ls32, D.sf, D.Tt, M, M, D.a32, want_var0=True)
    assert none is None and torch.equal(mean1, mean) and torch.equal(var01, var0)
    # a row does not depend on its neighbours: the contiguous copy, one row at a time for the first and last
    for i in sorted({0, N - 1}):
        mi, vi, _ = engine.sgp_project(Xv[i:i + 1].contiguous(), D.zt, D.inv_ls32, D.sf, D.Tt, M, M, D.a32, want_var0=True)
        assert torch.equal(mi, mean[i:i + 1]) and torch.equal(vi, var0[i:i + 1])
    # the public call
    pm, pv = g.predict(Xv)
    assert pm.shape == (N, 1) and pv.dtype == torch.float64
    assert torch.equal(pm[:, 0], mean.double())
    np.testing.assert_allclose(pv[:, 0].cpu().numpy(), np.abs(var0.double().cpu().numpy()) + math.exp(float(P[5])), rtol=1e-15)


def test_report_matches_float64(device):
    g, P = model(3, 33, device)
    rng = np.random.RandomState(2)
    X = rng.randn(200, 3).astype(np.float32).astype(np.float64)
    y = np.sin(X.sum(1))
    rep = g.report(X, y)
    m64, v64 = ref_predict(P, X)
    v64 = np.abs(v64) + math.exp(float(P[5]))
    assert rep["n"] == 200
    # (fp32 predictions of size ~1: each differs from float64 by ~1e-6 at most, and so does every average below)
    assert abs(rep["rmse"] - math.sqrt(np.mean((m64 - y) ** 2))) <= 1e-5
    assert abs(rep["pearson"] - np.corrcoef(m64, y)[0, 1]) <= 1e-5
    assert abs(rep["ll"] - np.mean(-0.5 * np.log(2 * np.pi * v64) - 0.5 * (m64 - y) ** 2 / v64)) <= 1e-5


# ------------------------------------------------------------------------------------------------ the epilogue and the argmin
def ei_keys(mean, var, inc, device, mode=_lib.SGP_ARGMIN_EI):
    m = torch.from_numpy(np.asarray(mean, dtype=np.float32)).to(device)
    v = torch.from_numpy(np.asarray(var, dtype=np.float32)).to(device)
    res, keys = engine.sgp_ei_step(mode, m, v, inc, want_keys=True)
    res = res.cpu().numpy()
    return int(res[0]), int(res[1]), float(res[2:3].view(np.float64)[0]), keys.cpu().numpy()


def test_epilogue_alone(device):
    """-log EI of the device against the float64 formula on the device's own fp32 (mean, var), 1e-12 relative - with rows on the
    series branch (s < -10) and in (-10, -5), where 1/2 (1 + erf) would be noise."""
    rng = np.random.RandomState(0)
    mean = rng.randn(300).astype(np.float32)
    var = (0.05 + rng.rand(300)).astype(np.float32)
    m64, v64 = mean.astype(np.float64), var.astype(np.float64)
    seen_far = seen_mid = False
    for k in (0.0, 3.0, 7.0, 9.5, 12.0):
        inc = float(m64.min() - k * math.sqrt(v64.max()))   # (k = 12 forces s < -10 on every row)
        i, bad, key, keys = ei_keys(mean, var, inc, device)
        want = -ref_log_ei(m64, v64, inc)
        s = (inc - m64) / np.sqrt(v64)
        seen_far |= bool((s < -10).any())
        seen_mid |= bool(((s > -10) & (s < -5)).any())
        err = np.abs(keys - want) / np.abs(want)
        print("k = %4.1f: s in [%.2f, %.2f], max relative error %.3g" % (k, s.min(), s.max(), err.max()))
        np.testing.assert_allclose(keys, want, rtol=1e-12, atol=0)
        assert bad == 0 and i == int(np.argmin(keys)) and key == keys[i]
        if k == 12.0:
            assert (s < -10).all()
    assert seen_far and seen_mid


def test_argmin_is_numpy_argmin(device):
    rng = np.random.RandomState(1)
    mean = rng.randn(193).astype(np.float32)
    var = (0.05 + rng.rand(193)).astype(np.float32)
    inc = float(mean.min())
    i, bad, key, keys = ei_keys(mean, var, inc, device)
    assert i == int(np.argmin(keys)) and bad == 0
    # a NaN row: the first NaN wins, every row without a positive variance is counted
    v2 = var.copy()
    v2[[150, 70, 191]] = [-1.0, 0.0, float("nan")]
    i, bad, key, keys = ei_keys(mean, v2, inc, device)
    assert np.isnan(keys[[70, 150, 191]]).all() and np.isfinite(np.delete(keys, [70, 150, 191])).all()
    assert i == int(np.argmin(keys)) == 70 and bad == 3 and math.isnan(key)
    # a tie: the lowest index wins, in both modes and across workgroups
    best = int(np.argmin(ei_keys(mean, var, inc, device)[3]))
    for other in (best + 70) % 193, (best + 1) % 193:
        m3, v3 = mean.copy(), var.copy()
        m3[other], v3[other] = mean[best], var[best]
        i, _, _, keys = ei_keys(m3, v3, inc, device)
        assert keys[other] == keys[best] and i == int(np.argmin(keys)) == min(best, other)
        m4 = mean.copy()
        m4[[best, other]] = mean.min() - 1.0
        i, bad, key, keys = ei_keys(m4, var, 0.0, device, _lib.SGP_ARGMIN_MEAN)
        assert np.array_equal(keys, m4.astype(np.float64)) and i == int(np.argmin(keys)) == min(best, other) and bad == 0
        assert key == float(m4.min())
    # N = 1
    i, bad, key, keys = ei_keys(mean[:1], var[:1], inc, device)
    assert i == 0 and key == keys[0] and keys.shape == (1,)


def test_a_duplicated_grid_row_ties(device):
    """Through the grid: the best row, planted again in front of the grid, gives the same bits and wins as index 0."""
    g, P = model(3, 33, device)
    rng = np.random.RandomState(5)
    grid = torch.from_numpy(rng.randn(130, 3)).to(device, torch.float32)
    inc = g.get_incumbent(grid, refine=None)
    keys = -g.log_ei(grid, inc)
    a = int(np.argmin(keys.cpu().numpy()))
    grid2 = torch.cat([grid[a:a + 1], grid], 0)
    keys2 = -g.log_ei(grid2, inc)
    assert torch.equal(keys2[1:], keys) and keys2[0] == keys2[a + 1]
    D = g.derived()
    m, v, _ = engine.sgp_project(grid2, D.zt, D.inv_ls32, D.sf, D.Tt, D.M, D.M, D.a32, want_var0=True)
    res = engine.sgp_ei_step(_lib.SGP_ARGMIN_EI, m, v, inc)[0].cpu().numpy()
    assert int(res[0]) == 0 == int(np.argmin(keys2.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ the greedy step
def run_steps(g, D, grid32, pts, device):
    """q update steps with the given points; returns the residual variance after every step, U and the results."""
    M, q, N = D.M, len(pts), grid32.shape[0]
    U = torch.zeros(N, M + q, dtype=torch.float32, device=device)
    mean, _, r = engine.sgp_project(grid32, D.zt, D.inv_ls32, D.sf, D.Tt, 2 * M, M, D.a32, U=U, u_col0=M, want_var1=True)
    fac = sgp._Factor(D, q)
    rs, results = [r.clone()], []
    for p in pts:
        Me = fac.Me
        c, delta = fac.extend(p)
        pc = torch.from_numpy(np.concatenate([p, c]).astype(np.float32)).to(device)
        res, keys = engine.sgp_ei_step(_lib.SGP_ARGMIN_EI, mean, r, float(mean.min()),
                                       update=(grid32, D.inv_ls32, D.sf, pc[:D.d], U, Me, pc[D.d:], 1.0 / delta), want_keys=True)
        rs.append(r.clone())
        results.append((res.clone(), keys))
    return mean, rs, U, results, fac


@pytest.mark.parametrize("d,M,N", [(3, 7, 65), (56, 500, 257)])
def test_ei_step_against_the_reinverted_matrix(device, d, M, N):
    g, P = model(d, M, device)
    D = g.derived()
    rng = np.random.RandomState(d + M)
    grid = (0.7 * rng.randn(N, d)).astype(np.float32).astype(np.float64)
    pts = (0.7 * rng.randn(5, d)).astype(np.float32).astype(np.float64)   # off the grid
    grid32 = torch.from_numpy(grid).to(device, torch.float32)
    mean, rs, U, results, fac = run_steps(g, D, grid32, pts, device)
    # torch's fp32 evaluation of the same incremental formula, from the same start
    _, _, r_t, U_t = torch_fp32(D, grid32)
    U_t = torch.cat([U_t, torch.zeros(N, 5, device=device)], 1)
    fac_t = sgp._Factor(D, 5)
    for j in range(5):
        Me = fac_t.Me
        c, delta = fac_t.extend(pts[j])
        p32, c32 = (torch.from_numpy(a.astype(np.float32)).to(device) for a in (pts[j], c))
        df = grid32 - p32
        w = (D.sf * torch.exp(-0.5 * (df * df * D.inv_ls32).sum(1)) - U_t[:, :Me] @ c32) * np.float32(1.0 / delta)
        U_t[:, Me] = w
        r_t = r_t - w * w
        want = ref_greedy_var(P, grid, pts[:j + 1])
        assert want.min() > 0
        e, tol = tol4("step %d r" % j, rs[j + 1].double().cpu().numpy(), want, r_t.double().cpu().numpy(), D.sf)
        assert e <= tol
        # the step's argmin is numpy's on the device's own keys, and the keys are the epilogue of the device's own (mean, r)
        res, keys = results[j][0].cpu().numpy(), results[j][1].cpu().numpy()
        assert int(res[0]) == int(np.argmin(keys)) and int(res[1]) == 0
        np.testing.assert_allclose(keys, -sgp.log_ei_host(mean.double().cpu().numpy(), rs[j + 1].double().cpu().numpy(),
                                                          float(mean.min())), rtol=1e-12, atol=0)
    mean2, rs2, U2, results2, _ = run_steps(g, D, grid32, pts, device)
    assert torch.equal(mean, mean2) and torch.equal(U, U2)
    assert all(torch.equal(a, b) for a, b in zip(rs, rs2))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(results, results2))


def test_batched_greedy_ei_end_to_end(device):
    """refine=None on a 1 000-row grid: in float64, the row chosen at every step may lie below the step's float64 optimum by no
    more than the fp32 errors of (mean, variance) allow.  With s = (inc - mean) / sqrt(v) and d log EI / ds ~ |s| (+ 1 near 0),
    d s = |s| / (2 v) d v + d mean / sqrt(v): bound(row) = (|s| + 1) (|s| / (2 v) tol_v + tol_m / sqrt(v)), for the chosen row
    and the optimum both; tol_v and tol_m are 4x torch's fp32 errors on this grid (floored as everywhere)."""
    d, M, q, N = 8, 33, 4, 1000
    g, P = model(d, M, device)
    D = g.derived()
    rng = np.random.RandomState(9)
    grid = (0.8 * rng.randn(N, d)).astype(np.float32).astype(np.float64)
    pts, info = g.batched_greedy_ei(q, -5.0, 5.0, grid=grid, refine=None, return_info=True)
    idx = info["index"]
    assert pts.shape == (q, d) and np.array_equal(pts, grid[idx]) and info["bad"] == [0] * q
    m64, v64 = ref_predict(P, grid)
    tm, tv0, tv1, _ = (t.double().cpu().numpy() for t in torch_fp32(D, torch.from_numpy(grid).to(device, torch.float32)))
    tol_m = max(4 * np.abs(tm - m64).max(), 4 * ULP32 * np.abs(m64).max())
    tol_v = max(4 * np.abs(tv0 - v64).max(), 4 * np.abs(tv1 - ref_greedy_var(P, grid, grid[:0])).max(), 4 * ULP32 * D.sf)
    inc = info["incumbent"]
    assert abs(inc - m64.min()) <= tol_m
    for j in range(q):
        v = v64 if j == 0 else ref_greedy_var(P, grid, grid[idx[:j]])
        lei = ref_log_ei(m64, v, inc)
        s = (inc - m64) / np.sqrt(v)
        bound = (np.abs(s) + 1) * (np.abs(s) / (2 * v) * tol_v + tol_m / np.sqrt(v))
        best = int(np.nanargmax(lei))
        print("step %d: chose %d (log EI %.6f), optimum %d (%.6f), allowed gap %.3g" % (j, idx[j], lei[idx[j]], best, lei[best],
                                                                                    bound[idx[j]] + bound[best]))
        assert lei[idx[j]] >= lei[best] - (bound[idx[j]] + bound[best])


def test_lbfgs_refinement_on_the_device_grid(device):
    """refine='lbfgs', the default, on a GPU model - the device twin of test_sgp_cpu's
    test_refinement_stays_inside_the_bounds_and_never_loses: in float64, every point is at least as good as the grid row it
    started from (`_refine` never returns worse than its start, and both are judged by the same restatement, so the fp32 grid
    does not enter); only the choice of the incumbent's start row is fp32, hence tol_m of the test above."""
    pytest.importorskip("scipy.optimize")
    d, M, N, q = 3, 7, 60, 4
    g, P = model(d, M, device)
    D = g.derived()
    rng = np.random.RandomState(d + M)
    lo, up = -1.5 * np.ones(d), 1.5 * np.ones(d)
    grid = (lo + rng.rand(N, d) * (up - lo)).astype(np.float32).astype(np.float64)
    pts, info = g.batched_greedy_ei(q, lo, up, grid=grid, refine="lbfgs", return_info=True)
    assert pts.shape == (q, d) and (pts >= lo).all() and (pts <= up).all()
    inc = info["incumbent"]
    for j in range(q):
        both = np.stack([pts[j], grid[info["index"][j]]])
        mean, v0 = ref_predict(P, both)
        v = v0 if j == 0 else ref_greedy_var(P, both, pts[:j])
        lei = ref_log_ei(mean, v, inc)
        print("step %d: log EI %.12g from row %d at %.12g" % (j, lei[0], info["index"][j], lei[1]))
        assert lei[0] >= lei[1] - 1e-9 * max(1.0, abs(lei[1])), (j, lei)
    m64 = ref_predict(P, grid)[0]
    tm = torch_fp32(D, torch.from_numpy(grid).to(device, torch.float32))[0].double().cpu().numpy()
    tol_m = max(4 * np.abs(tm - m64).max(), 4 * ULP32 * np.abs(m64).max())
    print("incumbent %.12g, the grid's smallest float64 mean %.12g, tol_m %.3g" % (inc, m64.min(), tol_m))
    assert inc <= m64.min() + tol_m
    assert g.get_incumbent(grid, lo, up) == inc
    np.testing.assert_array_equal(g.batched_greedy_ei(q, lo, up, grid=grid, refine="lbfgs"), pts)   # bitwise repeatable


def test_bo_round_decodes_and_scores(device):
    model_bn = Hh.dvae_decoder_model("bn", max_n=10, nvt=10, hs=32, L=2, seed=3).to(device)
    nz = model_bn.nz
    rng = np.random.RandomState(4)
    X = rng.randn(60, nz)
    y = np.sin(X.sum(1))
    g = sgp.SparseGP(X, y, 9, device=device)
    g.initialize(rng, 60)
    data = BnData.from_samples(synth.asia_samples(2, 300), [2] * 8, device=device)
    q = 5
    points, strings, scores = sgp.bo_round(g, model_bn, q, -3.0 * np.ones(nz), 3.0 * np.ones(nz), X.mean(0), X.std(0), data=data,
                                           decode_attempts=12, grid_size=200, rng=rng, refine=None)
    assert points.shape == (q, nz) and len(strings) == q and scores.shape == (q,) and scores.dtype == np.float64
    want = np.asarray(score_strings(data, strings))
    assert np.array_equal(np.isnan(scores), np.isnan(want)) and np.array_equal(scores[~np.isnan(want)], want[~np.isnan(want)])
    points2, strings2, none = sgp.bo_round(g, model_bn, 2, -3.0, 3.0, X.mean(0), X.std(0), decode_attempts=4, grid_size=100,
                                           rng=rng, refine=None, data_type="BN")
    assert points2.shape == (2, nz) and len(strings2) == 2 and none is None
