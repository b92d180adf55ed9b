"""The sparse GP of the BO loop (dagnn_amd/sgp.py) on the CPU: the module's float64 mirrors, the training energy, the start
and the acquisition flow.

No fixture can come from the reference: its sparse GP is Theano code and Theano does not run here.  The yardstick is an
independent float64 restatement of the written formulas (sparse_gp_theano_internal.py: compute_output, compute_log_ei,
compute_log_averaged_ei, getContributionToEnergy; gauss.py: compute_kernel), written below with explicit inverses as the
reference has them - not the whitened form and not the incremental factor the module uses.

Tolerances.  The restatement inverts Kzz (condition number up to (M + jitter) / jitter ~ 1e3 M) and Kzz^-1 + P; both sides
carry a relative error of about eps cond.  `cond_tol` measures the two condition numbers of the case and allows
64 eps cond(Kzz) cond(Kzz^-1 + P)^(1/2) relative to sf - the product bounds the error of B = Kzz^-1 covPost Kzz^-1 - Kzz^-1;
`greedy_tol` is 64 eps cond(Kzz_expanded) sf for the variance of the averaged EI, which inverts that matrix."""
import math

import numpy as np
import pytest
import torch

from dagnn_amd import sgp
from dagnn_amd.sgp import SparseGP

EPS = np.finfo(np.float64).eps
SHAPES = [(1, 1), (3, 7), (8, 16)]


# ------------------------------------------------------------------------------------------------ the restatement
def ref_kernel(lls, lsf, x, z):
    ls, sf = np.exp(lls), np.exp(lsf)
    r2 = np.sum(x * x / ls, 1)[:, None] - 2.0 * (x / ls) @ z.T + (np.ones_like(x) / ls) @ (z.T ** 2)
    return sf * np.exp(-0.5 * r2)


def ref_posterior(P, cav=1.0):
    lls, lsf, z, m, L, _ = P
    M = z.shape[0]
    Kzz = ref_kernel(lls, lsf, z, z) + np.eye(M) * sgp.JITTER * np.exp(lsf)
    KzzInv = np.linalg.inv(Kzz)
    LLt = L @ L.T
    covInv = KzzInv + LLt * cav
    cov = np.linalg.inv(covInv)
    mean = cov @ (cav * m)
    return Kzz, KzzInv, covInv, cov, mean


def ref_predict(P, X):
    """(mean, v_out) - v_out without |.| and without the noise."""
    lls, lsf, z = P[0], P[1], P[2]
    _, KzzInv, _, cov, mean = ref_posterior(P)
    K = ref_kernel(lls, lsf, X, z)
    B = KzzInv @ cov @ KzzInv - KzzInv
    return (K @ (KzzInv @ mean))[:, 0], np.exp(lsf) + np.sum(K * (K @ B), 1)


def ref_log_ei(m, v, inc):
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
        out[i] = math.log((inc - mi) * ratio + math.sqrt(vi)) - 0.5 * math.log(2.0 * math.pi) - 0.5 * s * s
    return out


def ref_greedy_var(P, x, chosen):
    """v_out of compute_log_averaged_ei: sf - k_e Kzz_expanded^-1 k_e^T with z_e = [z; chosen], re-inverted."""
    lls, lsf, z = P[0], P[1], P[2]
    ze = np.concatenate([z, chosen], 0)
    Ke = ref_kernel(lls, lsf, ze, ze) + np.eye(ze.shape[0]) * sgp.JITTER * np.exp(lsf)
    k = ref_kernel(lls, lsf, x, ze)
    return np.exp(lsf) - np.sum(k * (k @ np.linalg.inv(Ke)), 1)


def ref_energy(P, X, y, n):
    lls, lsf, z, m, L, lvn = P
    M = z.shape[0]
    cav = (n - 1.0) / n
    _, KzzInv, covCavInv, covCav, meanCav = ref_posterior(P, cav)
    _, _, covPostInv, covPost, meanPost = ref_posterior(P, 1.0)
    K = ref_kernel(lls, lsf, X, z)
    B = KzzInv @ covCav @ KzzInv - KzzInv
    mean = K @ (KzzInv @ meanCav)
    var = np.abs(np.exp(lsf) + np.sum(K * (K @ B), 1))[:, None] + np.exp(lvn)
    half = 0.5 * M * np.log(2 * np.pi)
    ld = lambda S: np.linalg.slogdet(S)[1]   # noqa: E731
    logZcav = half + 0.5 * ld(covCav) + 0.5 * (meanCav.T @ covCavInv @ meanCav)[0, 0]
    logZprior = half - 0.5 * ld(KzzInv)
    logZpost = half + 0.5 * ld(covPost) + 0.5 * (meanPost.T @ covPostInv @ meanPost)[0, 0]
    logZ = -0.5 * np.log(2 * np.pi * var) - 0.5 * (y - mean) ** 2 / var
    return ((logZcav - logZpost) + logZpost / n - logZprior / n) * X.shape[0] + logZ.sum()


def cond_tol(P):
    Kzz, KzzInv, covInv, _, _ = ref_posterior(P)
    return 64.0 * EPS * np.linalg.cond(Kzz) * math.sqrt(np.linalg.cond(covInv)) * float(np.exp(P[1]))


def greedy_tol(P, chosen):
    """The same rule for the averaged EI's variance: the matrix inverted there is Kzz_expanded."""
    ze = np.concatenate([P[2], chosen], 0)
    Ke = ref_kernel(P[0], P[1], ze, ze) + np.eye(ze.shape[0]) * sgp.JITTER * np.exp(P[1])
    return 64.0 * EPS * np.linalg.cond(Ke) * float(np.exp(P[1]))


# ------------------------------------------------------------------------------------------------ models
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


# ------------------------------------------------------------------------------------------------ mirrors
@pytest.mark.parametrize("d,M", SHAPES)
def test_predict_and_log_ei_mirrors(d, M):
    g, P, rng = make(d, M)
    X = rng.randn(23, d)
    tol = cond_tol(P)
    m_ref, v_ref = ref_predict(P, X)
    m, v = sgp.predict_host(g.derived(), X)
    print("mean err %.3g var err %.3g tol %.3g" % (np.abs(m - m_ref).max(), np.abs(v - v_ref).max(), tol))
    scale = max(1.0, np.abs(P[3]).max())
    assert np.abs(m - m_ref).max() <= tol * scale
    assert np.abs(v - v_ref).max() <= tol
    pm, pv = g.predict(X)
    assert pm.shape == (23, 1) and pv.shape == (23, 1) and pm.dtype == torch.float64
    np.testing.assert_allclose(pm.numpy()[:, 0], m_ref, atol=tol * scale, rtol=0)
    np.testing.assert_allclose(pv.numpy()[:, 0], np.abs(v_ref) + np.exp(P[5]), atol=tol, rtol=0)
    # the epilogue on the same (mean, var): three incumbents - ordinary, s in (-10, -5), s < -10
    for k in (0.0, 7.0, 12.0):
        inc = m_ref.min() - k * math.sqrt(v.max())
        want = ref_log_ei(m_ref, v, inc)
        got = sgp.log_ei_host(m_ref, v, inc)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    s = (m_ref.min() - 7.0 * math.sqrt(v.max()) - m_ref) / np.sqrt(v)
    assert (s < -5).all()
    got = g.log_ei(X, m_ref.min()).numpy()
    assert np.isfinite(got).all()
    assert np.isnan(sgp.log_ei_host([0.0, 0.0], [0.0, -1.0], 0.0)).all()


@pytest.mark.parametrize("d,M", SHAPES)
def test_greedy_variance_against_the_reinverted_matrix(d, M):
    g, P, rng = make(d, M)
    D = g.derived()
    grid = rng.randn(31, d)
    pts = rng.randn(4, d)
    fac = sgp._Factor(D, 4)
    K = sgp.kernel_host(D.lls, D.lsf, grid, D.z)
    U = np.zeros((31, M + 4))
    U[:, :M] = K @ D.W.T
    r = D.sf - np.sum(U[:, :M] ** 2, 1)
    np.testing.assert_allclose(r, ref_greedy_var(P, grid, pts[:0]), atol=greedy_tol(P, pts[:0]), rtol=0)
    for j in range(4):
        Me = fac.Me
        c, delta = fac.extend(pts[j])
        w = (sgp.kernel_host(D.lls, D.lsf, grid, pts[j:j + 1])[:, 0] - U[:, :Me] @ c) / delta
        U[:, Me] = w
        r = r - w * w
        tol = greedy_tol(P, pts[:j + 1])
        print("step %d: err %.3g tol %.3g" % (j, np.abs(r - ref_greedy_var(P, grid, pts[:j + 1])).max(), tol))
        np.testing.assert_allclose(r, ref_greedy_var(P, grid, pts[:j + 1]), atol=tol, rtol=0)
        x = rng.randn(d)
        assert abs(fac.point(x)[1] - ref_greedy_var(P, x[None, :], pts[:j + 1])[0]) <= tol


# ------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("d,M", [(3, 7)])
def test_energy_and_its_gradient(d, M):
    g, P, rng = make(d, M)
    X, y = g.X[:17], g.y[:17]
    params = g.get_params()
    for p in params:
        p.requires_grad_(True)
    E = g.energy(X, y)
    want = ref_energy(P, X.numpy(), y.numpy(), g.n_points)
    assert abs(float(E.detach()) - want) <= 1e-9 * max(1.0, abs(want)), (float(E.detach()), want)
    grads = torch.autograd.grad(E, params)
    for p in params:
        p.requires_grad_(False)
    h = 1e-6
    for k, (p, gr) in enumerate(zip(params, grads)):
        flat, gf = p.detach().reshape(-1), gr.reshape(-1)
        for i in rng.choice(flat.numel(), min(flat.numel(), 6), replace=False):
            old = float(flat[i])
            with torch.no_grad():
                flat[i] = old + h
                up = float(g.energy(X, y))
                flat[i] = old - h
                dn = float(g.energy(X, y))
                flat[i] = old
            fd = (up - dn) / (2 * h)
            # central differences: truncation ~ h^2 f''' and round-off ~ eps |E| / h
            tol = 1e-6 * max(1.0, abs(fd)) + 8 * EPS * abs(want) / h
            assert abs(fd - float(gf[i])) <= tol, (k, int(i), fd, float(gf[i]))


def test_one_adam_step_is_adam_theano():
    g, P, rng = make(3, 7)
    params = g.get_params()
    for p in params:
        p.requires_grad_(True)
    grads = [t.numpy().copy() for t in torch.autograd.grad(g.energy(g.X, g.y), params)]
    for p in params:
        p.requires_grad_(False)
    lr = 1e-2
    g.train_via_adam(max_iterations=1, minibatch_size=g.n_points, learning_rate=lr, rng=np.random.RandomState(5), verbose=False,
                     initialize=False)
    for p0, gE, p in zip(P, grads, g.get_params()):
        gl = -gE                                   # adam_theano minimises -e
        m, v = 0.1 * gl, 0.001 * gl ** 2
        want = p0 - lr * (m / (1 - 0.9)) / (np.sqrt(v / (1 - 0.999)) + 1e-8)
        # (the shuffled batch adds the rows in another order: the gradient moves by a few ulp, the step by far less than 1e-9 lr)
        np.testing.assert_allclose(p.numpy(), want, rtol=0, atol=1e-6 * lr)


def test_initialize_draws_in_the_reference_order():
    rng = np.random.RandomState(3)
    X = rng.randn(30, 4)
    y = rng.randn(30)
    g = SparseGP(X, y, 5, device="cpu")
    g.initialize(np.random.RandomState(11), minibatch_size=20)
    r = np.random.RandomState(11)
    sub = r.choice(30, 30, replace=False)[0:20]
    Xs = X[sub]
    sel = r.choice(20, 5, replace=False)
    L = r.normal(size=(5, 5))
    sq = np.outer(np.sum(Xs ** 2, 1), np.ones(20))
    dist = sq - 2 * Xs @ Xs.T + sq.T
    lls = np.log(0.5 * (np.median(dist[np.triu_indices(20, 1)]) + 1e-3)) * np.ones(4)
    got = [p.numpy() for p in g.get_params()]
    assert [tuple(p.shape) for p in got] == [(4,), (), (5, 4), (5, 1), (5, 5), ()]
    np.testing.assert_array_equal(got[0], lls)
    assert got[1] == 0.0 and got[5] == 0.0
    np.testing.assert_array_equal(got[2], Xs[sel])
    np.testing.assert_array_equal(got[3][:, 0], y[sub][sel])
    np.testing.assert_array_equal(got[4], L)
    with pytest.raises(ValueError):
        g.initialize(np.random.RandomState(0), minibatch_size=3)


# ------------------------------------------------------------------------------------------------ the acquisition
def test_single_point_objective_gradient():
    g, P, rng = make(3, 7)
    D = g.derived()
    fac = sgp._Factor(D, 3)
    for j in range(3):
        fac.extend(rng.randn(3))
    inc = float(sgp.predict_host(D, g.X.numpy())[0].min())
    for fn in (sgp._ei_objective(fac.point, inc), sgp._ei_objective(lambda x: sgp._posterior_point(D, x), inc),
               sgp._ei_objective(fac.point, inc - 40.0)):   # (the last one sits on the series branch)
        for _ in range(3):
            x = rng.randn(3)
            f, gr = fn(x)
            for c in range(3):
                e = np.zeros(3)
                e[c] = 1e-6
                fd = (fn(x + e)[0] - fn(x - e)[0]) / 2e-6
                assert abs(fd - gr[c]) <= 1e-6 * max(1.0, abs(fd)) + 8 * EPS * abs(f) / 1e-6, (c, fd, gr[c])


def brute_force(P, grid, q):
    mean, v0 = ref_predict(P, grid)
    inc = mean.min()
    idx = [int(np.argmin(-ref_log_ei(mean, v0, inc)))]
    for j in range(1, q):
        v = ref_greedy_var(P, grid, grid[idx])
        idx.append(int(np.argmin(-ref_log_ei(mean, v, inc))))
    return inc, idx


@pytest.mark.parametrize("d,M", SHAPES)
def test_greedy_without_refinement_is_the_brute_force_loop(d, M):
    g, P, rng = make(d, M)
    grid = 2.0 * rng.randn(50, d)
    pts, info = g.batched_greedy_ei(4, -5.0, 5.0, grid=grid, refine=None, return_info=True)
    inc, idx = brute_force(P, grid, 4)
    assert info["index"] == idx
    assert abs(info["incumbent"] - inc) <= cond_tol(P) * max(1.0, np.abs(P[3]).max())
    np.testing.assert_array_equal(pts, grid[idx])
    assert pts.shape == (4, d) and pts.dtype == np.float64


def test_greedy_draws_the_reference_grid():
    g, P, _ = make(3, 7)
    lo, up = -2.0 * np.ones(3), 2.0 * np.ones(3)
    mean, std = 0.1 * np.ones(3), 1.5 * np.ones(3)
    r = np.random.RandomState(4)
    a = g.batched_greedy_ei(2, lo, up, mean, std, sample="normal", grid_size=40, rng=np.random.RandomState(4), refine=None)
    np.testing.assert_array_equal(a, g.batched_greedy_ei(2, lo, up, grid=mean + r.randn(40, 3) * std, refine=None))
    r = np.random.RandomState(4)
    a = g.batched_greedy_ei(2, lo, up, sample="uniform", grid_size=40, rng=np.random.RandomState(4), refine=None)
    np.testing.assert_array_equal(a, g.batched_greedy_ei(2, lo, up, grid=lo + r.rand(40, 3) * (up - lo), refine=None))


def test_refinement_stays_inside_the_bounds_and_never_loses():
    pytest.importorskip("scipy.optimize")
    g, P, rng = make(3, 7)
    lo, up = -1.5 * np.ones(3), 1.5 * np.ones(3)
    grid = lo + rng.rand(60, 3) * (up - lo)
    pts, info = g.batched_greedy_ei(4, lo, up, grid=grid, refine="lbfgs", return_info=True)
    assert pts.shape == (4, 3)
    assert (pts >= lo).all() and (pts <= up).all()
    inc = info["incumbent"]
    assert inc <= ref_predict(P, grid)[0].min() + 1e-12
    for j in range(4):
        both = np.stack([pts[j], grid[info["index"][j]]])
        mean, v0 = ref_predict(P, both)
        v = v0 if j == 0 else ref_greedy_var(P, both, pts[:j])
        lei = ref_log_ei(mean, v, inc)
        assert lei[0] >= lei[1] - 1e-9 * max(1.0, abs(lei[1])), (j, lei)
    assert isinstance(g.get_incumbent(grid, lo, up), float)
    assert g.get_incumbent(grid, lo, up) <= g.get_incumbent(grid, refine=None) + 1e-12


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_checks():
    X = np.random.RandomState(0).randn(20, 3)
    y = X.sum(1)
    with pytest.raises(ValueError):
        SparseGP(X, y, sgp.MAX_M + 1, device="cpu")
    with pytest.raises(ValueError):
        SparseGP(np.zeros((4, sgp.MAX_D + 1)), np.zeros(4), 2, device="cpu")
    with pytest.raises(ValueError):
        SparseGP(X, y[:5], 2, device="cpu")
    with pytest.raises(ValueError):
        SparseGP(X[0], y, 2, device="cpu")
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        SparseGP(bad, y, 2, device="cpu")
    assert (sgp.MAX_M, sgp.MAX_D, sgp.MAX_Q) == (512, 128, 128)
    g, _, _ = make(3, 7)
    with pytest.raises(ValueError):
        g.predict(np.zeros((4, 2)))
    with pytest.raises(ValueError):
        g.predict(bad)
    with pytest.raises(ValueError):
        g.batched_greedy_ei(sgp.MAX_Q + 1, -1.0, 1.0, grid=X, refine=None)
    with pytest.raises(ValueError):
        g.batched_greedy_ei(2, -1.0, 1.0, grid=bad, refine=None)
    with pytest.raises(ValueError):
        g.batched_greedy_ei(2, np.zeros(2), 1.0, grid=X, refine=None)
    with pytest.raises(ValueError):
        g.batched_greedy_ei(2, -1.0, 1.0, grid=X, refine="newton")
    with pytest.raises(ValueError):
        g.batched_greedy_ei(2, -1.0, 1.0, sample="sobol", refine=None)
    with pytest.raises(ValueError):
        g.set_params(g.get_params()[:5])
    params = [p.numpy().copy() for p in g.get_params()]
    g.set_params(params)
    assert all(np.array_equal(a, b.numpy()) for a, b in zip(params, g.get_params()))
