"""refine="multistart" of the sparse GP (dagnn_amd/sgp.py: `refine_host`, `greedy_host`, `batched_greedy_ei`) on the CPU.

The yardstick is an independent float64 restatement of posterior, greedy variance and log EI with explicit inverses, as
tests/test_sgp_cpu.py has one (restated here, not imported), and scipy's L-BFGS-B on the module's own objective from start 0.

The margin against scipy, 1e-7 max(1, |f|), is 45 times the stopping rule's 2.2e-9 (both optimisers stop on a relative
decrease of that size, so either may stop that far above the optimum they share); a CPU prototype of the state machine
measured at most 6.1e-10 on these shapes with seeds 0 and 1.  The seeds below are 0 and 1 and none had to be replaced."""
import math

import numpy as np
import pytest

from dagnn_amd import sgp
from dagnn_amd.sgp import SparseGP

EPS = np.finfo(np.float64).eps
SHAPES = [(3, 7, 60), (8, 32, 400), (20, 48, 300)]


# ------------------------------------------------------------------------------------------------ the restatement
def ref_kernel(lls, lsf, x, z):
    ls, sf = np.exp(lls), np.exp(lsf)
    r2 = np.sum(x * x / ls, 1)[:, None] - 2.0 * (x / ls) @ z.T + (np.ones_like(x) / ls) @ (z.T ** 2)
    return sf * np.exp(-0.5 * r2)


def ref_predict(P, X):
    lls, lsf, z, m, L, _ = P
    M = z.shape[0]
    KzzInv = np.linalg.inv(ref_kernel(lls, lsf, z, z) + np.eye(M) * sgp.JITTER * np.exp(lsf))
    cov = np.linalg.inv(KzzInv + L @ L.T)
    K = ref_kernel(lls, lsf, X, z)
    B = KzzInv @ cov @ KzzInv - KzzInv
    return (K @ (KzzInv @ (cov @ m)))[:, 0], np.exp(lsf) + np.sum(K * (K @ B), 1)


def ref_greedy_var(P, x, chosen):
    lls, lsf, z = P[0], P[1], P[2]
    ze = np.concatenate([z, chosen], 0)
    Ke = ref_kernel(lls, lsf, ze, ze) + np.eye(ze.shape[0]) * sgp.JITTER * np.exp(lsf)
    k = ref_kernel(lls, lsf, x, ze)
    return np.exp(lsf) - np.sum(k * (k @ np.linalg.inv(Ke)), 1)


def ref_neg_log_ei(m, v, inc):
    out = np.empty(len(m))
    for i, (mi, vi) in enumerate(zip(m, v)):
        if not vi > 0:
            out[i] = np.nan
            continue
        s = (inc - mi) / math.sqrt(vi)
        if s < -10:
            ratio = -(1.0 / s - 1.0 / s ** 3 + 3.0 / s ** 5 - 15.0 / s ** 7)
        else:
            ratio = 0.5 * math.erfc(-s / math.sqrt(2.0)) / (math.exp(-0.5 * s * s) / math.sqrt(2.0 * math.pi))
        out[i] = -(math.log((inc - mi) * ratio + math.sqrt(vi)) - 0.5 * math.log(2.0 * math.pi) - 0.5 * s * s)
    return out


def ref_objective(P, x, chosen, inc, j):
    """-log EI of the rows of x at greedy step j (0: the posterior; j >= 1: the averaged EI given chosen[:j])."""
    mean, v0 = ref_predict(P, x)
    return ref_neg_log_ei(mean, v0 if j == 0 else ref_greedy_var(P, x, chosen[:j]), inc)


def make(d, M, n=40, seed=0, device="cpu"):
    rng = np.random.RandomState(100 * d + M + seed)
    X = rng.randn(n, d)
    y = np.sin(X.sum(1)) + 0.1 * rng.randn(n)
    g = SparseGP(X, y, M, device=device)
    g.initialize(rng, n)
    P = [p.cpu().numpy().copy() for p in g.get_params()]
    P[0] = P[0] + 0.2 * rng.randn(d)
    P[1] = np.float64(0.3)
    P[4] = 0.3 * P[4]
    P[5] = np.float64(-1.0)
    g.set_params(P)
    return g, [np.asarray(p, dtype=np.float64) for p in P], rng


def step_objectives(D, pts, inc):
    """The module's objective of every greedy step, given the points chosen before it."""
    fac = sgp._Factor(D, len(pts))
    funs = [sgp._ei_objective(lambda x: sgp._posterior_point(D, x), inc)]
    for j in range(1, len(pts)):
        fac.extend(pts[j - 1])
        snap = sgp._Factor(D, len(pts))
        snap.ze[:], snap.W[:], snap.Me = fac.ze, fac.W, fac.Me
        funs.append(sgp._ei_objective(snap.point, inc))
    return funs


# ------------------------------------------------------------------------------------------------ against scipy
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("d,M,N", SHAPES)
def test_multistart_against_scipy_from_start_0(d, M, N, seed):
    spo = pytest.importorskip("scipy.optimize")
    q = 4 if seed == 0 else 5
    g, P, rng = make(d, M, n=N, seed=seed)   # (N training rows - the inducing rows are drawn from them - and N grid rows)
    lo, up = -1.5 * np.ones(d), 1.5 * np.ones(d)
    grid = lo + rng.rand(N, d) * (up - lo)
    pts, info = g.batched_greedy_ei(q, lo, up, grid=grid, refine="multistart", return_info=True)
    assert pts.shape == (q, d) and pts.dtype == np.float64
    assert (pts >= lo).all() and (pts <= up).all()
    assert len(info["starts"]) == q + 1 and all(len(r["status"]) == 16 for r in info["starts"])
    inc = info["incumbent"]
    assert inc <= ref_predict(P, grid)[0].min() + 1e-12
    funs = step_objectives(g.derived(), pts, inc)
    for j in range(q):
        x0 = np.clip(grid[info["index"][j]], lo, up)
        f_ref = ref_objective(P, np.stack([pts[j], x0]), pts, inc, j)
        assert f_ref[0] <= f_ref[1] + 1e-9 * max(1.0, abs(f_ref[1])), (j, f_ref)
        xs, fs, _ = spo.fmin_l_bfgs_b(funs[j], x0, bounds=list(zip(lo.tolist(), up.tolist())), maxiter=150)
        f_mine = funs[j](pts[j])[0]
        print("d %d M %d seed %d step %d: multistart %.12g scipy %.12g (above by %.3g)" % (d, M, seed, j, f_mine, fs, f_mine - fs))
        assert f_mine <= fs + 1e-7 * max(1.0, abs(fs)), (j, f_mine, fs)


def test_one_start_from_the_same_row_reaches_scipys_optimum():
    spo = pytest.importorskip("scipy.optimize")
    g, P, rng = make(8, 32)
    D = g.derived()
    lo, up = -1.5 * np.ones(8), 1.5 * np.ones(8)
    grid = lo + rng.rand(50, 8) * (up - lo)
    mean = sgp.predict_host(D, grid)[0]
    fun = sgp._ei_objective(lambda x: sgp._posterior_point(D, x), float(mean.min()))
    for row in grid[:6]:
        x, f, info = sgp.refine_host(fun, row[None, :], lo, up, 64)
        xs, fs, _ = spo.fmin_l_bfgs_b(fun, row, bounds=list(zip(lo.tolist(), up.tolist())), maxiter=150)
        assert info["status"][0] in (1, 2, 3) and info["evals"][0] <= 64
        assert f <= fun(row)[0]
        # (two local optimisers from one row may still part ways; where they end in one basin they agree to the stopping rule)
        if np.abs(x - xs).max() < 1e-2:
            assert abs(f - fs) <= 1e-7 * max(1.0, abs(fs)), (f, fs)


# ------------------------------------------------------------------------------------------------ edge cases
def quad(center, scale=1.0):
    center = np.asarray(center, dtype=np.float64)
    return lambda x: (0.5 * scale * float((x - center) @ (x - center)), scale * (x - center))


def test_a_start_on_a_bound_with_the_gradient_pointing_outward_stays_there():
    lo, up = np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0])
    trace = []

    def fun(x):
        trace.append(np.array(x))
        return quad([3.0, 0.25, -2.0])(x)

    x, f, info = sgp.refine_host(fun, np.array([[1.0, -0.5, -1.0]]), lo, up, 64)
    assert all(t[0] == 1.0 and t[2] == -1.0 for t in trace)          # never leaves the two active bounds, in any trial
    np.testing.assert_allclose(x, [1.0, 0.25, -1.0], atol=1e-5)
    assert info["status"] == [1] and info["best"] == 0
    # a start outside the bounds is clipped before its first evaluation
    trace.clear()
    sgp.refine_host(fun, np.array([[5.0, 0.0, 0.0]]), lo, up, 8)
    assert trace[0][0] == 1.0


def test_dead_starts_are_never_chosen_and_all_dead_falls_back_to_the_grid_row():
    g, P, rng = make(3, 7)
    D = g.derived()
    inc = float(sgp.predict_host(D, g.X.numpy())[0].min())

    def fun(x):   # the variance is not positive left of x_0 = 0: NaN, as `_neg_log_ei_point` answers there
        if x[0] < 0:
            return float("nan"), np.zeros(3)
        return sgp._ei_objective(lambda t: sgp._posterior_point(D, t), inc)(x)

    lo, up = -2.0 * np.ones(3), 2.0 * np.ones(3)
    X0 = np.array([[-0.5, 0.1, 0.2], [0.5, 0.1, 0.2], [-1.0, 0.0, 0.0]])
    x, f, info = sgp.refine_host(fun, X0, lo, up, 32)
    assert info["status"][0] == 4 and info["status"][2] == 4 and info["evals"][0] == 1 and info["best"] == 1
    assert np.isnan(info["f"][0]) and np.isnan(info["x"][0]).all()
    assert x[0] >= 0 and f <= fun(X0[1])[0]
    x, f, info = sgp.refine_host(fun, X0[[0, 2]], lo, up, 32)
    assert x is None and info["best"] == -1 and info["status"] == [4, 4]
    # the greedy flow then takes the clipped grid row
    grid = np.array([[-3.0, 0.1, 0.2], [-1.0, 0.0, 0.0]])
    x, f, _ = sgp._multistart(fun, grid, np.array([0.5, 1.0]), 0, lo, up, 16, 32)
    np.testing.assert_array_equal(x, [-2.0, 0.1, 0.2])
    # rows without a finite key are no starts at all: fewer starts
    assert sgp._pick_starts(np.array([np.nan, 2.0, -np.inf, 1.0, 1.0, np.inf]), 16).tolist() == [3, 4, 1]
    assert sgp._pick_starts(np.array([3.0, 2.0, 1.0, 1.0]), 2).tolist() == [2, 3]


def test_one_start_and_a_grid_smaller_than_starts():
    g, P, rng = make(3, 7)
    lo, up = -1.5 * np.ones(3), 1.5 * np.ones(3)
    grid = lo + rng.rand(60, 3) * (up - lo)
    one, info = g.batched_greedy_ei(3, lo, up, grid=grid, refine="multistart", starts=1, return_info=True)
    assert one.shape == (3, 3) and all(len(r["status"]) == 1 for r in info["starts"])
    inc = info["incumbent"]
    for j in range(3):
        f = ref_objective(P, np.stack([one[j], np.clip(grid[info["index"][j]], lo, up)]), one, inc, j)
        assert f[0] <= f[1] + 1e-9 * max(1.0, abs(f[1]))
    few, info = g.batched_greedy_ei(3, lo, up, grid=grid[:5], refine="multistart", starts=16, return_info=True)
    assert few.shape == (3, 3) and all(len(r["status"]) == 5 for r in info["starts"])
    assert (few >= lo).all() and (few <= up).all()
    # more starts never lose against one: start 0 is the same row
    many, minfo = g.batched_greedy_ei(1, lo, up, grid=grid, refine="multistart", starts=16, return_info=True)
    solo, sinfo = g.batched_greedy_ei(1, lo, up, grid=grid, refine="multistart", starts=1, return_info=True)
    assert minfo["incumbent"] <= sinfo["incumbent"]
    assert isinstance(g.get_incumbent(grid, lo, up, refine="multistart"), float)
    assert g.get_incumbent(grid, lo, up, refine="multistart") <= g.get_incumbent(grid, refine=None) + 1e-12
    assert g.get_incumbent(grid, lo, up, refine="multistart", starts=4) == sgp.greedy_host(
        g.derived(), grid, 1, "multistart", lo, up, starts=4)[1]["incumbent"]


def test_budget_and_monotone_descent():
    fun = quad([0.3, -0.2, 0.1, 0.7], 50.0)
    lo, up = -np.ones(4), np.ones(4)
    X0 = np.array([[0.9, 0.9, -0.9, -0.9], [0.0, 0.0, 0.0, 0.0]])
    x4, f4, i4 = sgp.refine_host(fun, X0, lo, up, 4)
    x64, f64, i64 = sgp.refine_host(fun, X0, lo, up, 64)
    assert all(e <= 4 for e in i4["evals"]) and all(s in (1, 2, 3) for s in i4["status"])
    assert f64 <= f4 <= min(fun(X0[0])[0], fun(X0[1])[0])
    assert all(i64["f"][k] <= fun(X0[k])[0] for k in range(2))
    np.testing.assert_allclose(x64, [0.3, -0.2, 0.1, 0.7], atol=1e-5)


# ------------------------------------------------------------------------------------------------ arguments, defaults
def test_argument_checks():
    g, _, rng = make(3, 7)
    grid = rng.randn(20, 3)
    for kw in (dict(starts=0), dict(starts=33), dict(max_evals=3), dict(max_evals=1025)):
        with pytest.raises(ValueError):
            g.batched_greedy_ei(2, -1.0, 1.0, grid=grid, refine="multistart", **kw)
        with pytest.raises(ValueError):
            g.get_incumbent(grid, -1.0, 1.0, refine="multistart", **kw)
    with pytest.raises(ValueError):
        g.get_incumbent(grid, refine="multistart")                       # the bounds are needed
    with pytest.raises(ValueError):
        g.batched_greedy_ei(2, None, 1.0, grid=grid, refine="multistart")
    with pytest.raises(ValueError):
        g.batched_greedy_ei(2, -1.0, 1.0, grid=grid, refine="newton")
    with pytest.raises(ValueError):
        sgp.refine_host(quad([0.0]), np.zeros((1, 1)), -1.0, 1.0, 2)
    with pytest.raises(ValueError):
        sgp.greedy_host(g.derived(), grid, 2, "multistart", -1.0, 1.0, starts=40)
    assert sgp.MAX_STARTS == 32 and sgp.REFINE_STATUS == ("running", "converged", "stalled", "budget", "dead")
    assert g.batched_greedy_ei(2, -1.0, 1.0, grid=grid, refine="multistart", starts=32, max_evals=4).shape == (2, 3)


def test_the_other_modes_give_the_points_they_gave():
    g, P, rng = make(3, 7)
    lo, up = -1.5 * np.ones(3), 1.5 * np.ones(3)
    grid = lo + rng.rand(60, 3) * (up - lo)
    D = g.derived()
    a, ia = g.batched_greedy_ei(4, lo, up, grid=grid, refine=None, return_info=True)
    b, ib = sgp.greedy_host(D, grid, 4)
    np.testing.assert_array_equal(a, b)
    assert ia["index"] == ib["index"] and ia["incumbent"] == ib["incumbent"] and "starts" not in ia
    pytest.importorskip("scipy.optimize")
    a, ia = g.batched_greedy_ei(4, lo, up, grid=grid, return_info=True)          # the default is still 'lbfgs'
    b, ib = sgp.greedy_host(D, grid, 4, "lbfgs", lo, up)
    np.testing.assert_array_equal(a, b)
    assert ia["index"] == ib["index"] and ia["incumbent"] == ib["incumbent"] and "starts" not in ia
    assert g.get_incumbent(grid, lo, up) == ib["incumbent"]
