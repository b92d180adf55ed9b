"""The sparse GP of the D-VAE BO loop (bayesian_optimization/sparse_gp.py, sparse_gp_theano_internal.py, gauss.py; used by
bo.py:256-261, 289): the model that proposes the points of a round.

    sgp = SparseGP(X_train, y_train, 500, device="cuda")
    sgp.train_via_adam(X_test, y_test, max_iterations=100, minibatch_size=1000, learning_rate=5e-4, rng=rng)    # bo.py:257
    mean, var = sgp.predict(X_test)                                                                             # bo.py:261
    fit = sgp.report(X_test, y_test)                     # {'rmse', 'll', 'pearson', 'n'} of bo.py:265-270
    points = sgp.batched_greedy_ei(50, lower, upper, mean, std, sample="normal", rng=rng)                       # bo.py:289
    points = sgp.batched_greedy_ei(50, lower, upper, mean, std, refine="multistart", starts=16, max_evals=64)   # on the device
    points, strings, scores = bo_round(sgp, model, 50, lower, upper, mean, std, data=bn_data)                   # bo.py:289-306

The model (ignore_variances = True, the only path of the reference that bo.py runs): sf = exp(lsf), ls = exp(lls),
    k(x, z) = sf exp(-1/2 sum_c (x_c - z_c)^2 / ls_c),      Kzz = k(z, z) + 1e-3 sf I,      P = LParamPost LParamPost^T,
    covPost = (Kzz^-1 + P)^-1,      a = Kzz^-1 covPost mParamPost,      B = Kzz^-1 covPost Kzz^-1 - Kzz^-1,
    mean(x) = k(x, z) a,      var(x) = |sf + k B k^T| + exp(lvar_noise).
Training (`energy`, `train_via_adam`) runs by default on torch ops in float64 with autograd; `train_via_adam(grad="hip")` and
`energy_and_grad` take the fused step of csrc/sgp_train.hip instead: energy and the six gradients by analytic adjoints in one
library call.  Every `predict` and every grid of `batched_greedy_ei` runs in csrc/sgp.hip on matrices derived
once per parameter version in float64 and handed over rounded to fp32, in the whitened form:
    Kzz = L L^T,   A = L^T P L,   I - (I + A)^-1 = R^T R,   G = R L^-1,   var = sf - |G k|^2,   a = L^-T (I + A)^-1 L^T mParamPost
and for the averaged EI, W = L^-1 extended by one row per chosen point.  refine="multistart" replaces the reference's one
L-BFGS-B run per step by `starts` projected L-BFGS runs in lock-step (`refine_host` is the definition; on the GPU
csrc/sgp_refine.hip, float64, no scipy).  A model on the CPU goes through the float64 numpy
mirrors of this module (`*_host`); a model on the GPU never does.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import _lib, core, engine

__all__ = ["SparseGP", "bo_round", "MAX_M", "MAX_D", "MAX_Q", "JITTER", "kernel_host", "predict_host", "log_ei_host",
           "greedy_host", "energy_grad_host", "refine_host", "REFINE_STATUS", "MAX_STARTS"]

MAX_M = _lib.SGP_MAX_M   # DAGNN_SGP_MAX_M: inducing points
MAX_D = _lib.SGP_MAX_D   # DAGNN_SGP_MAX_D: input columns
MAX_Q = _lib.SGP_MAX_Q   # DAGNN_SGP_MAX_Q: points of one greedy batch
MAX_STARTS = _lib.SGP_REFINE_MAX_STARTS   # DAGNN_SGP_REFINE_MAX_STARTS: starts of refine="multistart"
REFINE_STATUS = _lib.SGP_REFINE_STATUS    # the names of a start's status, by its number
JITTER = 1e-3
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
_SQRT_2PI = math.sqrt(2.0 * math.pi)


# --------------------------------------------------------------------------------- the host mirrors (float64 numpy)
def kernel_host(lls, lsf, x, z) -> np.ndarray:
    """k(x, z) [Nx, Nz] in float64, from the differences (the reference expands the square: gauss.py:11-29)."""
    x, z = np.atleast_2d(np.asarray(x, dtype=np.float64)), np.atleast_2d(np.asarray(z, dtype=np.float64))
    il = np.exp(-np.asarray(lls, dtype=np.float64)).reshape(-1)
    out = np.empty((x.shape[0], z.shape[0]), dtype=np.float64)
    for i in range(0, x.shape[0], 256):   # (bounded scratch: [256, Nz, d])
        df = x[i:i + 256, None, :] - z[None, :, :]
        out[i:i + 256] = np.einsum("nmc,c,nmc->nm", df, il, df)
    return math.exp(float(lsf)) * np.exp(-0.5 * out)


def _erfc(x: np.ndarray) -> np.ndarray:
    return torch.special.erfc(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def log_ei_host(mean, var, incumbent: float) -> np.ndarray:
    """The row epilogue of `dagnn_sgp_ei_step` in float64 numpy: with s = (incumbent - mean) / sqrt(var),
        log EI = log((incumbent - mean) ratio(s) + sqrt(var)) - 1/2 log(2 pi) - 1/2 s^2,
    ratio(s) the reference's series below s = -10 and Phi(s) / phi(s) with Phi(s) = 1/2 erfc(-s / sqrt 2) otherwise; NaN where
    var is not positive."""
    m, v = np.asarray(mean, dtype=np.float64).reshape(-1), np.asarray(var, dtype=np.float64).reshape(-1)
    out = np.full(m.shape, np.nan)
    ok = v > 0
    sd = np.sqrt(v[ok])
    u = float(incumbent) - m[ok]
    s = u / sd
    with np.errstate(all="ignore"):
        far = s < -10.0
        x = np.where(far, s, -11.0)
        x2 = x * x
        x3 = x2 * x
        x5 = x3 * x2
        x7 = x5 * x2
        series = -(1.0 / x - 1.0 / x3 + 3.0 / x5 - 15.0 / x7)
        near = (0.5 * _erfc(-s * math.sqrt(0.5))) / (np.exp(-0.5 * s * s) / _SQRT_2PI)
        out[ok] = np.log(u * np.where(far, series, near) + sd) - _HALF_LOG_2PI - 0.5 * s * s
    return out


def _neg_log_ei_point(m: float, v: float, inc: float):
    """(-log EI, d / d mean, d / d var) at one point, of the expression `log_ei_host` evaluates (the series branch is
    differentiated as the series it is)."""
    if not v > 0:
        return float("nan"), 0.0, 0.0
    sd = math.sqrt(v)
    s = (inc - m) / sd
    if s < -10.0:
        rho = -(1.0 / s - 1.0 / s ** 3 + 3.0 / s ** 5 - 15.0 / s ** 7)
        drho = 1.0 / s ** 2 - 3.0 / s ** 4 + 15.0 / s ** 6 - 105.0 / s ** 8
    else:
        phi = math.exp(-0.5 * s * s) / _SQRT_2PI
        if phi == 0.0:
            return float("-inf"), 0.0, 0.0   # (s beyond 38: the formula's own overflow)
        rho = 0.5 * math.erfc(-s * math.sqrt(0.5)) / phi
        drho = 1.0 + s * rho
    h = (inc - m) * rho + sd
    if not h > 0:
        return float("nan"), 0.0, 0.0
    lei = math.log(h) - _HALF_LOG_2PI - 0.5 * s * s
    gs = (rho + s * drho) / (s * rho + 1.0) - s
    return -lei, gs / sd, -(1.0 - gs * s) / (2.0 * v)


def predict_host(D, X):
    """(mean [N], var0 [N]) of the rows of X from the derived matrices `D` (`SparseGP.derived()`), float64:
    mean = k a and var0 = sf - |G k|^2, the posterior variance without |.| and without the noise."""
    K = kernel_host(D.lls, D.lsf, X, D.z)
    GK = K @ D.G.T
    return K @ D.a, D.sf - np.einsum("nm,nm->n", GK, GK)


class _Factor(object):
    """The inverse Cholesky factor of Kzz_expanded = k(z_e, z_e) + jitter sf I, z_e = [z; chosen points], in float64 on the
    host: W_e = L_e^-1, extended by one row per point (never re-inverted)."""

    def __init__(self, D, q: int):
        M = D.z.shape[0]
        self.D, self.M, self.Me = D, M, M
        self.ze = np.zeros((M + q, D.z.shape[1]))
        self.ze[:M] = D.z
        self.W = np.zeros((M + q, M + q))
        self.W[:M, :M] = D.W

    def extend(self, p: np.ndarray):
        """Append the point p: returns (c [Me], delta) with c = L_e^-1 k(p, z_e), delta = sqrt(sf + jitter sf - c^T c)."""
        D, Me = self.D, self.Me
        kv = kernel_host(D.lls, D.lsf, p[None, :], self.ze[:Me])[0]
        c = self.W[:Me, :Me] @ kv
        d2 = D.sf * (1.0 + JITTER) - float(c @ c)
        if not d2 > 0:
            raise FloatingPointError("batched_greedy_ei: Kzz_expanded is not positive definite at point %d" % (Me - self.M))
        delta = math.sqrt(d2)
        self.W[Me, :Me] = -(c @ self.W[:Me, :Me]) / delta
        self.W[Me, Me] = 1.0 / delta
        self.ze[Me] = p
        self.Me = Me + 1
        return c, delta

    def point(self, x: np.ndarray):
        """(mean, r, d mean / dx, d r / dx) at one point: r = sf - |W_e k(x, z_e)|^2 - O(Me^2)."""
        D, Me, M = self.D, self.Me, self.M
        ke = kernel_host(D.lls, D.lsf, x[None, :], self.ze[:Me])[0]
        dk = -ke[:, None] * (x[None, :] - self.ze[:Me]) * D.inv_ls[None, :]
        u = self.W[:Me, :Me] @ ke
        return float(ke[:M] @ D.a), D.sf - float(u @ u), D.a @ dk[:M], -2.0 * ((u @ self.W[:Me, :Me]) @ dk)


def _posterior_point(D, x: np.ndarray):
    """(mean, var0, d mean / dx, d var0 / dx) at one point under the posterior (compute_log_ei)."""
    k = kernel_host(D.lls, D.lsf, x[None, :], D.z)[0]
    dk = -k[:, None] * (x[None, :] - D.z) * D.inv_ls[None, :]
    u = D.G @ k
    return float(k @ D.a), D.sf - float(u @ u), D.a @ dk, -2.0 * ((u @ D.G) @ dk)


def _ei_objective(point_fn, inc: float):
    def fun(x):
        m, v, dm, dv = point_fn(np.asarray(x, dtype=np.float64).reshape(-1))
        f, fm, fv = _neg_log_ei_point(m, v, inc)
        return f, fm * dm + fv * dv
    return fun


def _scipy_optimize():
    try:
        import scipy.optimize as spo
    except ImportError as e:   # pragma: no cover - scipy is an optional dependency
        raise ImportError("refine='lbfgs' runs the reference's scipy.optimize.fmin_l_bfgs_b and scipy is not installed: "
                          "install scipy, or pass refine=None to take the best grid rows") from e
    return spo


def _refine(fun, x0: np.ndarray, lower: np.ndarray, upper: np.ndarray):
    """global_optimization's second half (sparse_gp.py:31-43): L-BFGS-B from the best grid row inside the bounds, maxiter 150.
    Returns (x, f); never worse than the (clipped) start."""
    spo = _scipy_optimize()
    x0 = np.clip(x0, lower, upper)
    f0 = fun(x0)[0]
    x, f, _ = spo.fmin_l_bfgs_b(fun, x0, bounds=list(zip(lower.tolist(), upper.tolist())), maxiter=150)
    x = np.clip(np.asarray(x, dtype=np.float64).reshape(-1), lower, upper)
    if not f <= f0:
        return x0, f0
    return x, float(f)


_RUNNING, _CONVERGED, _STALLED, _BUDGET, _DEAD = range(5)   # DAGNN_SGP_REFINE_RUNNING .. _DEAD
_HISTORY, _MAX_HALVINGS = _lib.SGP_REFINE_HISTORY, 20


def _refine_start(objective, x0: np.ndarray, lo: np.ndarray, up: np.ndarray, max_evals: int):
    """One start of `refine_host`: (x, f, status, evals), x = None for a dead start."""
    clip = lambda v: np.minimum(np.maximum(v, lo), up)   # noqa: E731
    xt = clip(x0)
    x = g = p = None
    f, t, halv, evals, status = float("nan"), 0.0, 0, 0, _RUNNING
    S, Y, SY = [], [], []
    while evals < max_evals and status == _RUNNING:
        ft, gt = objective(xt)
        ft, gt = float(ft), np.asarray(gt, dtype=np.float64).reshape(-1)
        evals += 1
        took = False
        if evals == 1:
            if not math.isfinite(ft):
                status = _DEAD
                break
            x, f, g, took = xt, ft, gt, True
        else:
            s = xt - x
            if math.isfinite(ft) and ft <= f + 1e-4 * float(g @ s):
                y = gt - g
                sy = float(s @ y)
                if sy > 1e-10 * math.sqrt(float(s @ s)) * math.sqrt(float(y @ y)):
                    S, Y, SY = (S + [s])[-_HISTORY:], (Y + [y])[-_HISTORY:], (SY + [sy])[-_HISTORY:]
                if f - ft <= 2.2e-9 * max(abs(f), abs(ft), 1.0):   # scipy's default factr
                    status = _CONVERGED
                x, f, g, took = xt, ft, gt, True
            elif halv >= _MAX_HALVINGS:
                status = _STALLED
            else:
                halv, t = halv + 1, 0.5 * t
                xt = clip(x + t * p)
        if took and status == _RUNNING:
            if float(np.max(np.abs(x - clip(x - g)))) <= 1e-5:       # scipy's pgtol
                status = _CONVERGED
                continue
            free = ~(((x <= lo) & (g > 0)) | ((x >= up) & (g < 0)))
            qv = np.where(free, g, 0.0)
            alpha = [0.0] * len(S)
            for i in range(len(S) - 1, -1, -1):
                alpha[i] = float(S[i] @ qv) / SY[i]
                qv = qv - alpha[i] * Y[i]
            r = qv * (SY[-1] / float(Y[-1] @ Y[-1])) if S else qv
            for i in range(len(S)):
                beta = float(Y[i] @ r) / SY[i]
                r = r + S[i] * (alpha[i] - beta)
            p = np.where(free, -r, 0.0)
            if not float(g @ p) < 0:
                S, Y, SY = [], [], []
                p = np.where(free, -g, 0.0)
            if S:
                t = 1.0
            else:
                pn = math.sqrt(float(p @ p))
                t = min(1.0, 1.0 / pn) if pn > 0 else 1.0
            halv = 0
            xt = clip(x + t * p)
    if status == _RUNNING:
        status = _BUDGET
    return x, f, status, evals


def refine_host(objective, X0, lower, upper, max_evals: int = 64):
    """The definition of refine="multistart" (csrc/sgp_refine.hip implements the same state machine): every row of X0 [S, d],
    clipped into [lower, upper], is one start of a projected L-BFGS with 8 curvature pairs on `objective` (x -> (f, grad)),
    one evaluation per tick for at most `max_evals` ticks.  Per start: the first tick evaluates clip(x0) - not finite: the start
    is dead.  After an accepted point x: stop `converged` if max |x - clip(x - g)| <= 1e-5; coordinate i is fixed if it sits on
    a bound with the gradient pointing outward; p = -H g by the two-loop recursion on g with the fixed coordinates zeroed
    (scaling s.y / y.y of the newest pair), fixed coordinates of p zeroed; if g.p is not below 0 the pairs are dropped and
    p = -g on the free set; t = 1 with pairs, else min(1, 1 / |p|).  A trial xt = clip(x + t p) is accepted if f(xt) is finite
    and f(xt) <= f + 1e-4 g.(xt - x), else t halves (`stalled` after 20 halvings).  On acceptance the pair (xt - x, gt - g) is
    kept if s.y > 1e-10 |s| |y|, and the start stops `converged` if f - f(xt) <= 2.2e-9 max(|f|, |f(xt)|, 1); the point is taken
    either way.  A start out of ticks stops with `budget`.  The result is the accepted point with the smallest f (ties: the
    lower start).  Returns (x [d] or None, f, info): info['best'] (-1: no start has a finite objective), info['status'] and
    info['evals'] per start, info['x'] [S, d] and info['f'] [S] (NaN for a dead start)."""
    X0 = np.atleast_2d(np.asarray(X0, dtype=np.float64))
    d = X0.shape[1]
    lo, up = _bounds(lower, d, "lower"), _bounds(upper, d, "upper")
    max_evals = int(max_evals)
    if not 4 <= max_evals <= 1024:
        raise ValueError("refine_host: 4 <= max_evals <= 1024 needed (got %d)" % max_evals)
    xs, fs, status, evals = np.full(X0.shape, np.nan), np.full(X0.shape[0], np.nan), [], []
    best = -1
    for k in range(X0.shape[0]):
        x, f, st, ne = _refine_start(objective, X0[k], lo, up, max_evals)
        status.append(st)
        evals.append(ne)
        if x is not None:
            xs[k], fs[k] = x, f
            if math.isfinite(f) and (best < 0 or f < fs[best]):
                best = k
    info = {"best": best, "status": status, "evals": evals, "x": xs, "f": fs}
    if best < 0:
        return None, float("nan"), info
    return xs[best].copy(), float(fs[best]), info


def _pick_starts(keys: np.ndarray, starts: int) -> np.ndarray:
    """The rows of the `starts` smallest finite keys, ties to the lower row."""
    keys = np.asarray(keys, dtype=np.float64)
    fin = np.isfinite(keys)
    return np.argsort(np.where(fin, keys, np.inf), kind="stable")[:min(int(starts), int(fin.sum()))]


def _multistart(objective, grid: np.ndarray, keys: np.ndarray, i0: int, lo, up, starts: int, max_evals: int):
    """(x, f, info) of one greedy step under refine="multistart": `refine_host` from the best rows of the grid; without a start
    of finite objective the clipped grid row i0, as `_refine` falls back to."""
    rows = _pick_starts(keys, starts)
    x, f, info = None, float("nan"), {"best": -1, "status": [], "evals": []}
    if rows.size:
        x, f, info = refine_host(objective, grid[rows], lo, up, max_evals)
    if x is None:
        x = np.clip(grid[i0], lo, up)
        f = float(objective(x)[0])
    return x, f, info


def _check_refine(refine, lower=None, upper=None, starts: int = 16, max_evals: int = 64):
    if refine not in (None, "lbfgs", "multistart"):
        raise ValueError("refine must be None, 'lbfgs' or 'multistart' (got %r)" % (refine,))
    if refine == "lbfgs":
        _scipy_optimize()
    if refine == "multistart":
        if not 1 <= int(starts) <= MAX_STARTS:
            raise ValueError("refine='multistart': 1 <= starts <= %d needed (got %r)" % (MAX_STARTS, starts))
        if not 4 <= int(max_evals) <= 1024:
            raise ValueError("refine='multistart': 4 <= max_evals <= 1024 needed (got %r)" % (max_evals,))
        if lower is None or upper is None:
            raise ValueError("refine='multistart' needs the bounds lower and upper")


# --------------------------------------------------------------------------------- the greedy flow and its step providers
def _posterior_mean(D):
    """x -> (mean, d mean / dx) under the posterior: the objective of the incumbent's refinement."""
    return lambda x: _posterior_point(D, np.asarray(x, dtype=np.float64).reshape(-1))[0::2]


def _incumbent(prov, D):
    """Stage 0 of a greedy batch, and all of `get_incumbent`: (the incumbent, the step's run info).  The incumbent is the
    refined objective, and the best row's mean where no refinement has one (none asked for, or no live start)."""
    _, _, key, _, f, run = prov.incumbent(_posterior_mean(D))
    return (f if math.isfinite(f) else key), run


def _greedy_flow(prov, D, q: int):
    """The order of a greedy batch, written once for the host mirror and the device: the incumbent, the first point by the
    posterior EI under G, then per further point the factor extended by the previous point and the averaged EI under it.
    `prov` evaluates the grid and picks the points - `incumbent(fun)`, `posterior(inc, fun)`, `averaged(inc, fun, fac, c, delta)`,
    each returning (grid row, rows without a positive variance, the row's key, x, f, run info or None); `fun` is the step's
    float64 objective on the host, for a provider that refines there.  Returns (points [q, d], info) as `greedy_host` has them."""
    inc, run = _incumbent(prov, D)
    steps = [prov.posterior(inc, _ei_objective(lambda x: _posterior_point(D, x), inc))]
    fac = _Factor(D, q)
    for _ in range(1, q):
        c, delta = fac.extend(steps[-1][3])
        steps.append(prov.averaged(inc, _ei_objective(fac.point, inc), fac, c, delta))
    info = {"incumbent": inc, "index": [s[0] for s in steps], "r": prov.r, "bad": [s[1] for s in steps]}
    if run is not None:
        info["starts"] = [run] + [s[5] for s in steps]
    return np.stack([s[3] for s in steps]), info


def _from_row(refine, fun, x: np.ndarray, key: float, lower, upper):
    """(x, f, None) of a step that starts from its best grid row x alone: the row with its key, or `_refine` from it."""
    return _refine(fun, x, lower, upper) + (None,) if refine else (x, key, None)


def _decode(res: np.ndarray):
    """(grid row, rows without a positive variance, the row's key) of the result words of `dagnn_sgp_ei_step`."""
    return int(res[0]), int(res[1]), float(res[2:3].view(np.float64)[0])


def _stage(row: torch.Tensor, dev, *parts):
    """Fills the front of one pinned staging row with `parts`, back to back, and sends it: the row on the device."""
    v = np.concatenate(parts)
    row[:v.size] = torch.from_numpy(v)
    return row.to(dev, non_blocking=True)


class _HostGrid(object):
    """The steps of a CPU model and of `greedy_host`: the grid in float64 numpy, the point by `_refine` (refine='lbfgs') or
    `_multistart` from the rows as given."""

    def __init__(self, D, grid, q: int, refine, lower, upper, starts: int, max_evals: int):
        grid = np.asarray(grid, dtype=np.float64)
        if refine == "multistart":
            _check_refine(refine, lower, upper, starts, max_evals)
        if refine:
            lower, upper = _bounds(lower, grid.shape[1], "lower"), _bounds(upper, grid.shape[1], "upper")
        self.D, self.grid, self.q, self.refine, self.point_args = D, grid, q, refine, (lower, upper, starts, max_evals)
        self.K = kernel_host(D.lls, D.lsf, grid, D.z)
        self.mean = self.K @ D.a

    def _step(self, keys, fun, var=None):
        i = int(np.argmin(keys))
        key = float(keys[i])
        if self.refine == "multistart":
            point = _multistart(fun, self.grid, keys, i, *self.point_args)
        else:
            point = _from_row(self.refine, fun, self.grid[i], key, *self.point_args[:2])
        return (i, 0 if var is None else int((~(var > 0)).sum()), key) + point

    def incumbent(self, fun):
        return self._step(self.mean, fun)

    def posterior(self, inc, fun):
        D, K, M = self.D, self.K, self.D.z.shape[0]
        GK, U0 = K @ D.G.T, K @ D.W.T
        var0 = D.sf - np.einsum("nm,nm->n", GK, GK)
        self.r = D.sf - np.einsum("nm,nm->n", U0, U0)
        self.U = np.zeros((K.shape[0], M + self.q))
        self.U[:, :M] = U0
        return self._step(-log_ei_host(self.mean, var0, inc), fun, var0)

    def averaged(self, inc, fun, fac, c, delta):
        D, Me = self.D, fac.Me - 1   # (fac holds the previous point as row Me of z_e)
        w = (kernel_host(D.lls, D.lsf, self.grid, fac.ze[Me:Me + 1])[:, 0] - self.U[:, :Me] @ c) / delta
        self.U[:, Me] = w
        self.r = self.r - w * w
        return self._step(-log_ei_host(self.mean, self.r, inc), fun, self.r)


_INCUMBENT, _POSTERIOR, _AVERAGED = range(3)


class _DeviceGrid(object):
    """The steps of a GPU model with refine None or 'lbfgs': `dagnn_sgp_project` over the grid once, then per step one launch
    of `dagnn_sgp_ei_step` and one 32-byte read; `_refine` runs on the host from the row as the kernels see it.  q = 0 (the
    incumbent alone) projects the mean only."""

    def __init__(self, model, D, grid, q: int, refine, lo, up):
        M, d, dev = D.M, D.d, model.device
        self.D, self.dev, self.refine, self.lo, self.up = D, dev, refine, lo, up
        self.g32 = g32 = grid.to(dev, torch.float32).contiguous()
        self.host = g32.double().cpu().numpy() if q > 0 and refine != "multistart" else None   # (else `_row` reads the one row)
        if q < 1:   # (the argmin of the mean never looks at the variance)
            self.mean = self.var0 = engine.sgp_project(g32, D.zt, D.inv_ls32, D.sf, None, 0, 0, D.a32)[0]
            return
        self.U = torch.empty(grid.shape[0], M + q, dtype=torch.float32, device=dev)
        self.mean, self.var0, self.r = engine.sgp_project(g32, D.zt, D.inv_ls32, D.sf, D.Tt, 2 * M, M, D.a32, U=self.U, u_col0=M,
                                                          want_var0=True, want_var1=True)
        self.stage = torch.empty(q, d + M + q, dtype=torch.float32).pin_memory()   # (a row per step: p, then c)

    def _row(self, i: int) -> np.ndarray:   # row i of the grid as the kernels see it, float64 on the host
        return self.g32[i].double().cpu().numpy() if self.host is None else self.host[i]

    def _send(self, fac, c):
        """Stages what the step's kernels need of `fac`'s extension by its last point p: the fp32 row [p, c] on the device."""
        Me = fac.Me - 1
        return _stage(self.stage[Me + 1 - self.D.M], self.dev, fac.ze[Me], c)

    def _step(self, kind, var, inc, update, fun, Me):
        res, keys = engine.sgp_ei_step(_lib.SGP_ARGMIN_MEAN if kind == _INCUMBENT else _lib.SGP_ARGMIN_EI, self.mean, var, inc,
                                       update=update, want_keys=self.refine == "multistart")
        return self._point(res, keys, kind, inc, fun, Me)

    def _point(self, res, keys, kind, inc, fun, Me):
        i, nb, key = _decode(res.cpu().numpy())   # the step's one read
        if kind == _INCUMBENT and not self.refine:
            return i, nb, key, None, key, None    # (the row's mean is all that is asked for: the row stays where it is)
        return (i, nb, key) + _from_row(self.refine, fun, self._row(i), key, self.lo, self.up)

    def incumbent(self, fun):
        return self._step(_INCUMBENT, self.var0, 0.0, None, fun, self.D.M)

    def posterior(self, inc, fun):
        return self._step(_POSTERIOR, self.var0, inc, None, fun, self.D.M)

    def averaged(self, inc, fun, fac, c, delta):
        D, d, Me = self.D, self.D.d, fac.Me - 1
        pc = self._send(fac, c)
        return self._step(_AVERAGED, self.r, inc, (self.g32, D.inv_ls32, D.sf, pc[:d], self.U, Me, pc[d:], 1.0 / delta), fun, fac.Me)


class _DeviceMultistart(_DeviceGrid):
    """The steps of a GPU model with refine='multistart': the grid step hands its keys on, csrc/sgp_refine.hip refines the `starts`
    best rows in float64, and the step still reads the device once.  Kept in float64 on the device: ze [M + q, d] and its transpose
    (the kernel columns read that one), W_e [M + q, M + q] (none for q = 0), the bounds and the workspace."""

    def __init__(self, model, D, grid, q: int, lo, up, starts: int, max_evals: int):
        super().__init__(model, D, grid, q, "multistart", lo, up)
        model._derived64(D)
        M, d, dev = D.M, D.d, self.dev
        self.S, self.max_evals = starts, max_evals
        self.lo_t, self.up_t = torch.from_numpy(lo.copy()).to(dev), torch.from_numpy(up.copy()).to(dev)
        self.ze = torch.zeros(M + q, d, dtype=torch.float64, device=dev)
        self.ze[:M] = D.z64
        self.zet = torch.zeros(d, M + q, dtype=torch.float64, device=dev)
        self.zet[:, :M] = D.z64.t()
        self.We = None
        if q > 0:
            self.We = torch.zeros(M + q, M + q, dtype=torch.float64, device=dev)
            self.We[:M, :M] = D.W64
            self.stage64 = torch.empty(q, d + M + q, dtype=torch.float64).pin_memory()   # (p, then the new row of W_e)
        self.inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
        self.work = torch.empty(engine.sgp_refine_words(M, q, d, starts), dtype=torch.float64, device=dev)

    def _send(self, fac, c):
        pc = super()._send(fac, c)
        Me, d = fac.Me - 1, self.D.d
        pw = _stage(self.stage64[Me + 1 - self.D.M], self.dev, fac.ze[Me], fac.W[Me, :Me + 1])
        self.ze[Me].copy_(pw[:d])
        self.zet[:, Me].copy_(pw[:d])
        self.We[Me, :Me + 1].copy_(pw[d:d + Me + 1])
        return pc

    def _point(self, res, keys, kind, inc, fun, Me):
        """The starts (a stable sort), the refinement and the step's one read; without a live start the clipped grid row, f = NaN."""
        D, S, d = self.D, self.S, self.D.d
        mode, T = ((_lib.SGP_REFINE_MEAN, None), (_lib.SGP_REFINE_EI, D.G64), (_lib.SGP_REFINE_EI, self.We))[kind]
        fin = torch.isfinite(keys)
        rows = torch.sort(torch.where(fin, keys, self.inf), stable=True)[1][:S]
        nstart = fin.sum().clamp(max=S).to(torch.int32).reshape(1)
        X0 = torch.zeros(S, d, dtype=torch.float64, device=keys.device)
        X0[:rows.numel()] = self.g32[rows].double()   # the rows as the kernels see them; the run clips them
        out = engine.sgp_refine_run(mode, X0, self.lo_t, self.up_t, self.ze, D.inv_ls64, D.sf, D.a64, T, Me, kind == _AVERAGED, inc,
                                    self.max_evals, nstart, self.work, zet=self.zet)
        both = torch.cat([res, out.view(torch.int64)]).cpu().numpy()   # the step's one read
        i, nb, key = _decode(both)
        o = both[4:].view(np.float64)
        best = int(o[0])
        info = {"best": best, "status": [int(v) for v in o[2 + d:2 + d + S]], "evals": [int(v) for v in o[2 + d + S:2 + d + 2 * S]],
                "f": o[2 + d + 2 * S:2 + d + 3 * S].copy()}
        if best >= 0:
            return i, nb, key, o[2:2 + d].copy(), float(o[1]), info
        return i, nb, key, np.clip(self._row(i), self.lo, self.up), float("nan"), info


def greedy_host(D, grid: np.ndarray, q: int, refine=None, lower=None, upper=None, starts: int = 16, max_evals: int = 64):
    """The numpy mirror of the device flow of `batched_greedy_ei` over `grid` [N, d], in float64: incumbent (argmin of the
    mean), first point (posterior log EI), q - 1 points by the averaged EI with the incrementally extended factor.  Returns
    (points [q, d], info): info['incumbent'], info['index'] (the grid row of every step), info['r'] (the residual variance
    [N] after the last step), info['bad'] (rows without a positive variance, per step).  refine='multistart' runs
    `refine_host` from the `starts` best rows of every step (the rows as given: float64) and adds info['starts'], the info of
    `refine_host` per step, the incumbent's first."""
    return _greedy_flow(_HostGrid(D, grid, q, refine, lower, upper, starts, max_evals), D, q)


# --------------------------------------------------------------------------------- the training step's host mirror (float64 torch)
def _kernel_diff(il: torch.Tensor, sf: torch.Tensor, x: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """k(x, z) [Nx, Nz] from the differences, in chunks of 128 rows (bounded scratch)."""
    out = torch.empty(x.shape[0], z.shape[0], dtype=torch.float64)
    for i in range(0, x.shape[0], 128):
        df = x[i:i + 128, None, :] - z[None, :, :]
        out[i:i + 128] = torch.einsum("nmc,c,nmc->nm", df, il, df)
    return sf * torch.exp(-0.5 * out)


def _kernel_adjoint(il: torch.Tensor, g: torch.Tensor, x: torch.Tensor, z: torch.Tensor):
    """With g = Kbar o K [Nx, Nz]: (sum_r g_rm (x_rc - z_mc) [Nz, d], sum_rm g_rm (x_rc - z_mc)^2 [d]), from the differences."""
    dz, dl = torch.zeros_like(z), torch.zeros_like(il)
    for i in range(0, x.shape[0], 128):
        df = x[i:i + 128, None, :] - z[None, :, :]
        dz += torch.einsum("nm,nmc->mc", g[i:i + 128], df)
        dl += torch.einsum("nm,nmc,nmc->c", g[i:i + 128], df, df)
    return dz, dl


def energy_grad_host(params, X, y, n_points: int):
    """The energy of one minibatch and its six gradients (in `get_params()` order) in float64 torch on the CPU, by the analytic
    adjoints of the whitened form - the mirror of `dagnn_sgp_energy_grad`, product by product; no autograd.
    Returns (E [], [g_lls, g_lsf, g_z, g_mParamPost, g_LParamPost, g_lvar_noise])."""
    lls, lsf, z, mP, Lp, lvn = [torch.as_tensor(p).detach().to("cpu", torch.float64) for p in params]
    X = torch.as_tensor(X).detach().to("cpu", torch.float64)
    y = torch.as_tensor(y).detach().to("cpu", torch.float64).reshape(-1)
    M, b, n = z.shape[0], X.shape[0], float(n_points)
    mP = mP.reshape(M, 1)
    c = (n - 1.0) / n
    sf, il, noise = torch.exp(lsf), torch.exp(-lls), torch.exp(lvn)
    eye = torch.eye(M, dtype=torch.float64)
    inv = lambda T: torch.linalg.solve_triangular(T, eye, upper=False)   # noqa: E731
    # forward
    Kzz = _kernel_diff(il, sf, z, z) + eye * (JITTER * sf)
    L = torch.linalg.cholesky(Kzz)
    W = inv(L)
    C = Lp.T @ L
    A = C.T @ C
    Lc, L1 = torch.linalg.cholesky(eye + c * A), torch.linalg.cholesky(eye + A)
    Wc, W1 = inv(Lc), inv(L1)
    Sci, S1i = Wc.T @ Wc, W1.T @ W1
    t = L.T @ mP
    al, be = Sci @ t, S1i @ t
    G = -torch.log(torch.diagonal(Lc)).sum() + 0.5 * c * c * (t * al).sum() \
        - c * (-torch.log(torch.diagonal(L1)).sum() + 0.5 * (t * be).sum())
    Kx = _kernel_diff(il, sf, X, z)
    U = W @ Kx.T
    R = Sci @ U
    v = sf - (U * U).sum(0) + (U * R).sum(0)
    mean = c * (al * U).sum(0)
    out = v.abs() + noise
    r = y - mean
    E = b * G + (-0.5 * torch.log(2.0 * math.pi * out) - 0.5 * r * r / out).sum()
    # adjoints of the rows
    d_out = -0.5 / out + 0.5 * r * r / (out * out)
    d_v, d_mean = d_out * torch.sign(v), r / out
    Ub = (2.0 * (R - U)) * d_v + (c * al) * d_mean
    rho = R @ d_mean.reshape(b, 1)
    T3 = (R * d_v) @ R.T
    # adjoints of S_c, S_1 -> A, t
    Ab = c * (-0.5 * b * Sci - 0.5 * b * c * c * (al @ al.T) - T3 - 0.5 * c * (rho @ al.T + al @ rho.T)) \
        + 0.5 * c * b * (S1i + be @ be.T)
    tb = b * c * c * al + c * rho - c * b * be
    X1 = C @ Ab
    g_Lp = 2.0 * (L @ X1.T)
    g_m = L @ tb
    KxbT = W.T @ Ub
    Lb = torch.tril(2.0 * (Lp @ X1) - KxbT @ U.T + mP @ tb.T)
    # the Cholesky adjoint: Kzz_bar = L^-T Phi(L^T L_bar) L^-1, Phi = the lower triangle with half the diagonal
    Phi = torch.tril(L.T @ Lb)
    Phi.diagonal().mul_(0.5)
    Kb = W.T @ (Phi @ W)
    # the kernel's own derivative
    gz, gx = (Kb + Kb.T) * Kzz, KxbT.T * Kx
    dz1, dl1 = _kernel_adjoint(il, gz, z, z)
    dz2, dl2 = _kernel_adjoint(il, gx, X, z)
    g_z = (dz1 + dz2) * il
    g_lls = 0.5 * il * (0.5 * dl1 + dl2)
    g_lsf = 0.5 * gz.sum() + gx.sum() + sf * d_v.sum()
    g_noise = noise * d_out.sum()
    return E, [g_lls, g_lsf.reshape(()), g_z, g_m.reshape(M, 1), g_Lp, g_noise.reshape(())]


# --------------------------------------------------------------------------------- the model
def _as_rows(X, d: int, what: str) -> torch.Tensor:
    if not isinstance(X, torch.Tensor):
        X = torch.from_numpy(np.ascontiguousarray(np.asarray(X, dtype=np.float64)))
    if X.dim() != 2 or X.shape[1] != d or not X.is_floating_point():
        raise ValueError("%s: a floating-point [N, d=%d] matrix needed (got %s %s)" % (what, d, tuple(X.shape), X.dtype))
    if not X.is_cuda and bool(torch.isnan(X).any()):
        raise ValueError("%s: X holds NaN" % what)
    return X


def _bounds(v, d: int, what: str) -> np.ndarray:
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.full(d, float(a[0]))
    if a.size != d:
        raise ValueError("batched_greedy_ei: %s must hold one value per column (d=%d, got %d)" % (what, d, a.size))
    return a


class SparseGP(object):
    """The reference's `SparseGP(input_means, input_vars, training_targets, n_inducing_points)` without the input variances
    (bo.py passes zeros; ignore_variances is true).  The six parameters are float64 tensors on `device` under the reference's
    names: lls [d], lsf [], z [M, d], mParamPost [M, 1], LParamPost [M, M], lvar_noise []."""

    def __init__(self, X, y, n_inducing: int, device=None):
        X = np.asarray(X.detach().cpu() if isinstance(X, torch.Tensor) else X, dtype=np.float64)
        y = np.asarray(y.detach().cpu() if isinstance(y, torch.Tensor) else y, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("SparseGP: X must be [n >= 1, d >= 1] (got %s)" % (X.shape,))
        if y.size != X.shape[0] or y.ndim > 2 or (y.ndim == 2 and y.shape[1] != 1):
            raise ValueError("SparseGP: y must be [n] or [n, 1] for n = %d rows (got %s)" % (X.shape[0], y.shape))
        if np.isnan(X).any() or np.isnan(y).any():
            raise ValueError("SparseGP: X or y holds NaN")
        M = int(n_inducing)
        if not 1 <= M <= MAX_M:
            raise ValueError("SparseGP: 1 <= n_inducing <= %d needed (got %d)" % (MAX_M, M))
        if X.shape[1] > MAX_D:
            raise ValueError("SparseGP: at most %d input columns (got %d)" % (MAX_D, X.shape[1]))
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.n_points, self.d_input, self.n_inducing = int(X.shape[0]), int(X.shape[1]), M
        self.X = torch.from_numpy(np.ascontiguousarray(X)).to(self.device)
        self.y = torch.from_numpy(np.ascontiguousarray(y.reshape(-1, 1))).to(self.device)
        kw = dict(dtype=torch.float64, device=self.device)
        self.lls, self.lsf = torch.zeros(self.d_input, **kw), torch.zeros((), **kw)
        self.z, self.mParamPost = torch.zeros(M, self.d_input, **kw), torch.zeros(M, 1, **kw)
        self.LParamPost, self.lvar_noise = torch.zeros(M, M, **kw), torch.zeros((), **kw)
        self._cache = core.DerivedCache()

    @property
    def on_gpu(self) -> bool:
        return self.device.type == "cuda"

    def get_params(self):
        return [self.lls, self.lsf, self.z, self.mParamPost, self.LParamPost, self.lvar_noise]

    def set_params(self, params) -> None:
        params = list(params)
        if len(params) != 6:
            raise ValueError("set_params: six arrays in the order of get_params() needed (got %d)" % len(params))
        with torch.no_grad():
            for p, v in zip(self.get_params(), params):
                v = torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64))
                if v.numel() != p.numel():
                    raise ValueError("set_params: %d values for a parameter of shape %s" % (v.numel(), tuple(p.shape)))
                p.copy_(v.reshape(p.shape))
        self._cache.invalidate()

    def initialize(self, rng=None, minibatch_size: int = 4000) -> None:
        """The start of `train_via_ADAM` (sparse_gp.py:202-210, sparse_gp_theano_internal.py:203-234), drawing from `rng` (a
        numpy RandomState; default: numpy's global one, as the reference) in the reference's order: the minibatch subset, the
        inducing rows out of it, then L ~ N(0, 1)."""
        rng = np.random if rng is None else rng
        n, M = self.n_points, self.n_inducing
        sub = rng.choice(n, n, replace=False)[0:min(n, int(minibatch_size))]
        if sub.shape[0] < M:
            raise ValueError("initialize: %d inducing points need at least as many rows (the subset has %d)" % (M, sub.shape[0]))
        Xs, ys = self.X.cpu().numpy()[sub, :], self.y.cpu().numpy()[sub, :]
        sel = rng.choice(Xs.shape[0], M, replace=False)
        sq = np.outer(np.sum(Xs ** 2, 1), np.ones(Xs.shape[0]))
        dist = sq - 2 * np.dot(Xs, Xs.T) + sq.T
        tri = dist[np.triu_indices(Xs.shape[0], 1)]
        med = float(np.median(tri)) if tri.size else 0.0
        L = rng.normal(size=(M, M)) * 1.0
        self.set_params([np.log(0.5 * (med + 1e-3)) * np.ones(self.d_input), 0.0, Xs[sel, :], ys[sel, :], L, 0.0])

    # ----------------------------------------------------------------------------- training: torch ops, float64
    def energy(self, X: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """The energy of one minibatch (getContributionToEnergy, sparse_gp_theano_internal.py:163-198, 255-257) with the
        training graph's cavity factor (n - 1) / n, as a float64 scalar that autograd differentiates."""
        n, M = float(self.n_points), self.n_inducing
        cav = (n - 1.0) / n
        sf, il = torch.exp(self.lsf), torch.exp(-self.lls)

        def kern(a, b):   # (the reference's expansion, gauss.py:22-27: smooth where a row of a equals a row of b)
            r2 = (a * a * il).sum(1, keepdim=True) - 2.0 * (a * il) @ b.T + ((b * b) @ il)[None, :]
            return sf * torch.exp(-0.5 * r2)

        def inv_psd(S):
            return torch.cholesky_inverse(torch.linalg.cholesky(0.5 * (S + S.T)))

        def logdet_psd(S):
            return 2.0 * torch.log(torch.diagonal(torch.linalg.cholesky(0.5 * (S + S.T)))).sum()

        eye = torch.eye(M, dtype=torch.float64, device=self.z.device)
        Kzz = kern(self.z, self.z) + eye * (JITTER * sf)
        KzzInv = inv_psd(Kzz)
        LLt = self.LParamPost @ self.LParamPost.T
        covCavInv = KzzInv + LLt * cav
        covCav = inv_psd(covCavInv)
        meanCav = covCav @ (cav * self.mParamPost)
        covPostInv = KzzInv + LLt
        covPost = inv_psd(covPostInv)
        meanPost = covPost @ self.mParamPost
        Kxz = kern(X, self.z)
        B = KzzInv @ covCav @ KzzInv - KzzInv
        v_out = sf + ((Kxz @ B) * Kxz).sum(1, keepdim=True)
        out_mean = Kxz @ (KzzInv @ meanCav)
        out_var = v_out.abs() + torch.exp(self.lvar_noise)
        half = 0.5 * M * math.log(2.0 * math.pi)
        logZcav = half + 0.5 * logdet_psd(covCav) + 0.5 * (meanCav.T @ covCavInv @ meanCav)[0, 0]
        logZprior = half - 0.5 * logdet_psd(KzzInv)
        logZpost = half + 0.5 * logdet_psd(covPost) + 0.5 * (meanPost.T @ covPostInv @ meanPost)[0, 0]
        logZ = -0.5 * torch.log(2.0 * math.pi * out_var) - 0.5 * (y.reshape(-1, 1) - out_mean) ** 2 / out_var
        return ((logZcav - logZpost) + logZpost / n - logZprior / n) * float(X.shape[0]) + logZ.sum()

    def energy_and_grad(self, X, y, fail: Optional[torch.Tensor] = None, work: Optional[torch.Tensor] = None):
        """(E, [six gradients in `get_params()` order]) of one minibatch, float64 on the model's device, by the analytic
        adjoints of the whitened form; no autograd graph.  On a GPU model one call of `dagnn_sgp_energy_grad`
        (csrc/sgp_train.hip), nothing synchronises: a pivot that is not positive gives NaN outputs and counts on `fail` (an int32
        device word; default: the model's own, `train_failures()` reads it).  On a CPU model `energy_grad_host`."""
        X = _as_rows(X, self.d_input, "energy_and_grad")
        y = y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y, dtype=np.float64))
        if y.numel() != X.shape[0] or X.shape[0] < 1:
            raise ValueError("energy_and_grad: y must hold one value per row of X, at least one (got %d for %d rows)"
                             % (y.numel(), X.shape[0]))
        params = [p.detach() for p in self.get_params()]
        if not self.on_gpu:
            return energy_grad_host(params, X, y, self.n_points)
        X, y = X.detach().to(self.device, torch.float64), y.detach().to(self.device, torch.float64)
        E, grads = engine.sgp_energy_grad(X, y, params, self.n_points, self._fail_word() if fail is None else fail, work)
        return E.reshape(()), grads

    def _fail_word(self) -> torch.Tensor:
        if getattr(self, "_fail", None) is None:
            self._fail = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._fail

    def train_failures(self) -> int:
        """The failed pivots counted by `energy_and_grad` on the GPU since the last call of this method (one device read)."""
        if not self.on_gpu or getattr(self, "_fail", None) is None:
            return 0
        n = int(self._fail.item())
        self._fail.zero_()
        return n

    def train_via_adam(self, X_test=None, y_test=None, max_iterations: int = 500, minibatch_size: int = 4000,
                       learning_rate: float = 1e-3, rng=None, verbose: bool = True, initialize: bool = True,
                       grad: str = "autograd"):
        """`train_via_ADAM` (sparse_gp.py:195-270): `initialize`, then per epoch the reference's shuffle and minibatches, every
        minibatch one step of `torch.optim.Adam` (default betas, eps = 1e-8: the rule of `adam_theano`) on minus the energy.
        With `verbose` (and a test set) the epoch's train / test RMSE and test log-likelihood are printed, through `predict`.
        grad='autograd' differentiates `energy`; grad='hip' writes the gradients of `energy_and_grad` (one library call per
        minibatch on a GPU model; the same draws, minibatches and optimiser) - the failure counter is read once, at the end,
        and a non-zero count raises DagnnHipError.  Returns the last minibatch's energy."""
        rng = np.random if rng is None else rng
        mb = int(minibatch_size)
        if mb < 1 or int(max_iterations) < 0:
            raise ValueError("train_via_adam: minibatch_size >= 1 and max_iterations >= 0 needed")
        if grad not in ("autograd", "hip"):
            raise ValueError("train_via_adam: grad must be 'autograd' or 'hip' (got %r)" % (grad,))
        if grad == "hip":
            return self._train_analytic(X_test, y_test, int(max_iterations), mb, float(learning_rate), rng, verbose, initialize)
        if initialize:
            self.initialize(rng, mb)
        Xt = yt = None
        if X_test is not None:
            Xt = _as_rows(X_test, self.d_input, "train_via_adam").to(self.device, torch.float64)
            yt = torch.as_tensor(np.asarray(y_test.cpu() if isinstance(y_test, torch.Tensor) else y_test, dtype=np.float64)).reshape(-1, 1).to(self.device)
        params = self.get_params()
        for p in params:
            p.requires_grad_(True)
        opt = torch.optim.Adam(params, lr=float(learning_rate), betas=(0.9, 0.999), eps=1e-8)
        X, y, n = self.X, self.y, self.n_points
        n_batches = int(np.ceil(1.0 * n / mb))
        last = None
        try:
            for j in range(int(max_iterations)):
                perm = torch.from_numpy(np.asarray(rng.choice(n, n, replace=False), dtype=np.int64)).to(self.device)
                X, y = X[perm], y[perm]
                for i in range(n_batches):
                    opt.zero_grad(set_to_none=True)
                    loss = -self.energy(X[i * mb:min((i + 1) * mb, n)], y[i * mb:min((i + 1) * mb, n)])
                    loss.backward()
                    opt.step()
                    last = loss.detach()
                self._cache.invalidate()
                if verbose:
                    tr = self.report(X, y)
                    msg = "Epoch %d, Train error: %.4f" % (j, tr["rmse"])
                    if Xt is not None:
                        te = self.report(Xt, yt)
                        msg += " Test error: %.4f Test ll: %.4f" % (te["rmse"], te["ll"])
                    print(msg, flush=True)
        finally:
            for p in params:
                p.requires_grad_(False)
            self._cache.invalidate()
        return None if last is None else -float(last)

    def _train_analytic(self, X_test, y_test, max_iterations, mb, learning_rate, rng, verbose, initialize):
        """`train_via_adam(grad='hip')`: the same loop with `p.grad` written from `energy_and_grad`."""
        if initialize:
            self.initialize(rng, mb)
        Xt = yt = None
        if X_test is not None:
            Xt = _as_rows(X_test, self.d_input, "train_via_adam").to(self.device, torch.float64)
            yt = torch.as_tensor(np.asarray(y_test.cpu() if isinstance(y_test, torch.Tensor) else y_test, dtype=np.float64)).reshape(-1, 1).to(self.device)
        params = self.get_params()
        opt = torch.optim.Adam(params, lr=learning_rate, betas=(0.9, 0.999), eps=1e-8)
        X, y, n = self.X, self.y, self.n_points
        n_batches = int(np.ceil(1.0 * n / mb))
        fail = work = None
        if self.on_gpu:
            fail = torch.zeros(1, dtype=torch.int32, device=self.device)
            work = torch.empty(engine.sgp_energy_grad_words(self.n_inducing, self.d_input, min(mb, n)), dtype=torch.float64,
                               device=self.device)
        last = None
        try:
            for j in range(max_iterations):
                perm = torch.from_numpy(np.asarray(rng.choice(n, n, replace=False), dtype=np.int64)).to(self.device)
                X, y = X[perm], y[perm]
                for i in range(n_batches):
                    E, grads = self.energy_and_grad(X[i * mb:min((i + 1) * mb, n)], y[i * mb:min((i + 1) * mb, n)], fail, work)
                    for p, g in zip(params, grads):
                        p.grad = g.neg_()   # (the optimiser minimises minus the energy)
                    opt.step()
                    last = E
                self._cache.invalidate()
                if verbose:
                    tr = self.report(X, y)
                    msg = "Epoch %d, Train error: %.4f" % (j, tr["rmse"])
                    if Xt is not None:
                        te = self.report(Xt, yt)
                        msg += " Test error: %.4f Test ll: %.4f" % (te["rmse"], te["ll"])
                    print(msg, flush=True)
        finally:
            for p in params:
                p.grad = None
            self._cache.invalidate()
        if fail is not None:
            bad = int(fail.item())   # the call's one read of the counter
            if bad:
                raise _lib.DagnnHipError("train_via_adam(grad='hip'): %d Cholesky pivots were not positive: the parameters "
                                         "hold NaN from the first of them on" % bad)
        return None if last is None else float(last)

    # ----------------------------------------------------------------------------- derived matrices
    def derived(self):
        """The matrices the prediction side runs on, derived in float64 (torch.linalg on the model's device) once per
        parameter version (`core.DerivedCache`): host copies (z, ls, a, G, W = L^-1: numpy float64) and, on the GPU, the
        kernels' operands rounded to fp32 (zt, inv_ls, Tt = [G; W]^T, a)."""
        return self._cache.get(self.get_params(), self._derive)

    def _derive(self):
        M = self.n_inducing
        z, il, sf = self.z.detach(), torch.exp(-self.lls.detach()), torch.exp(self.lsf.detach())
        eye = torch.eye(M, dtype=torch.float64, device=z.device)
        df = z[:, None, :] - z[None, :, :]
        Kzz = sf * torch.exp(-0.5 * (df * df * il).sum(-1)) + eye * (JITTER * sf)
        L = torch.linalg.cholesky(Kzz)
        W = torch.linalg.solve_triangular(L, eye, upper=False)
        Lp = self.LParamPost.detach()
        A = L.T @ (Lp @ Lp.T) @ L
        lam, V = torch.linalg.eigh(0.5 * (A + A.T))
        lam = lam.clamp_min(0.0)
        G = (torch.sqrt(lam / (1.0 + lam))[:, None] * V.T) @ W              # R L^-1, R^T R = I - (I + A)^-1
        S = (V / (1.0 + lam)[None, :]) @ V.T                                  # (I + A)^-1
        a = torch.linalg.solve_triangular(L.T, S @ (L.T @ self.mParamPost.detach()), upper=True).reshape(-1)
        h = lambda t: t.cpu().numpy()   # noqa: E731
        D = SimpleNamespace(lls=h(self.lls.detach()), lsf=float(self.lsf), sf=float(sf), inv_ls=h(il), z=h(z), a=h(a), G=h(G), W=h(W),
                            noise=math.exp(float(self.lvar_noise)), M=M, d=self.d_input)
        if self.on_gpu:
            f = lambda t: t.to(torch.float32).contiguous()   # noqa: E731
            D.zt, D.inv_ls32, D.a32, D.Tt = f(z.T), f(il), f(a), f(torch.cat([G, W], 0).T)
        return D

    # ----------------------------------------------------------------------------- prediction
    def _rows32(self, X, what: str) -> torch.Tensor:
        X = _as_rows(X, self.d_input, what)
        return X.to(self.device, torch.float32, non_blocking=True)

    def predict(self, X):
        """(mean, var) of the rows of X, float64 [N, 1] on the model's device: var = |sf - |G k|^2| + exp(lvar_noise).  On the GPU
        one launch of `dagnn_sgp_project` (fp32), nothing synchronises."""
        D = self.derived()
        if not self.on_gpu:
            X = _as_rows(X, self.d_input, "predict")
            m, v = predict_host(D, X.detach().numpy())
            return torch.from_numpy(m).reshape(-1, 1), torch.from_numpy(np.abs(v) + D.noise).reshape(-1, 1)
        X = self._rows32(X, "predict")
        m, v, _ = engine.sgp_project(X, D.zt, D.inv_ls32, D.sf, D.Tt, D.M, D.M, D.a32, want_var0=True)
        return m.double().reshape(-1, 1), (v.double().abs() + D.noise).reshape(-1, 1)

    def report(self, X, y) -> dict:
        """What the reference prints of a fit (sparse_gp.py:250-252, bo.py:265-270): rmse = sqrt(mean (pred - y)^2), ll = mean
        log N(pred - y; 0, var), pearson = pearsonr(pred, y)[0], n.  On the GPU the sums are `dagnn_fit_sums` and the call
        synchronises once."""
        m, v = self.predict(X)
        y = torch.as_tensor(np.asarray(y, dtype=np.float64)) if not isinstance(y, torch.Tensor) else y
        y = y.reshape(-1, 1).to(m.device, torch.float64)
        n = m.shape[0]
        if y.shape[0] != n or n < 1:
            raise ValueError("report: y must hold one value per row of X (got %d for %d rows)" % (y.shape[0], n))
        ll = (-0.5 * torch.log(2.0 * math.pi * v) - 0.5 * (m - y) ** 2 / v).sum().reshape(1)
        if self.on_gpu:   # p = (-pred - 0) / 1 of dagnn_fit_sums: hand it minus the mean
            s = torch.cat([engine.fit_sums((-m).reshape(-1).float(), y.reshape(-1), 0.0, 1.0), ll]).tolist()
        else:
            p, t = m.reshape(-1).numpy(), y.reshape(-1).numpy()
            s = [p.sum(), t.sum(), (p * p).sum(), (t * t).sum(), (p * t).sum(), ((p - t) ** 2).sum(), float(ll)]
        sp, sy, spp, syy, spy, sd, sll = (float(x) for x in s)
        cov, vp, vy = spy - sp * sy / n, spp - sp * sp / n, syy - sy * sy / n
        return {"rmse": math.sqrt(sd / n), "ll": sll / n, "pearson": cov / math.sqrt(vp * vy) if vp > 0 and vy > 0 else float("nan"),
                "n": n}

    # ----------------------------------------------------------------------------- the acquisition
    def log_ei(self, X, incumbent: float) -> torch.Tensor:
        """`compute_log_ei(x, incumbent)` per row of X, float64 [N] on the model's device: the posterior mean and variance
        (no |.|, no noise), NaN where the variance is not positive."""
        D = self.derived()
        if not self.on_gpu:
            X = _as_rows(X, self.d_input, "log_ei")
            m, v = predict_host(D, X.detach().numpy())
            return torch.from_numpy(log_ei_host(m, v, incumbent))
        X = self._rows32(X, "log_ei")
        m, v, _ = engine.sgp_project(X, D.zt, D.inv_ls32, D.sf, D.Tt, D.M, D.M, D.a32, want_var0=True)
        return -engine.sgp_ei_step(_lib.SGP_ARGMIN_EI, m, v, float(incumbent), want_keys=True)[1]

    def get_incumbent(self, grid, lower=None, upper=None, refine="lbfgs", starts: int = 16, max_evals: int = 64) -> float:
        """`get_incumbent` (sparse_gp.py:272-283): the smallest predictive mean - over the grid, then refined from the best row
        by L-BFGS-B inside the bounds (refine=None: the best grid row's mean; refine='multistart': `refine_host`'s flow from the
        `starts` best rows, on the device for a GPU model): stage 0 of the flow of `batched_greedy_ei`."""
        _check_refine(refine, lower, upper, starts, max_evals)
        D = self.derived()
        grid = _as_rows(grid, self.d_input, "get_incumbent")
        if refine:
            lower, upper = _bounds(lower, self.d_input, "lower"), _bounds(upper, self.d_input, "upper")
        return _incumbent(self._steps(D, grid, 0, refine, lower, upper, starts, max_evals), D)[0]

    def _steps(self, D, grid: torch.Tensor, q: int, refine, lo, up, starts, max_evals):
        """The step provider of `_greedy_flow`: a CPU model's never touches `engine`, a GPU model's never the `*_host` grid."""
        if not self.on_gpu:
            return _HostGrid(D, grid.detach().numpy(), q, refine, lo, up, starts, max_evals)
        if refine == "multistart":
            return _DeviceMultistart(self, D, grid, q, lo, up, int(starts), int(max_evals))
        return _DeviceGrid(self, D, grid, q, refine, lo, up)

    def batched_greedy_ei(self, q: int, lower, upper, mean=None, std=None, sample: str = "normal", grid=None,
                          grid_size: int = 10000, rng=None, refine="lbfgs", return_info: bool = False, starts: int = 16,
                          max_evals: int = 64):
        """`batched_greedy_ei` (sparse_gp.py:296-335): q points [q, d] (float64 numpy) - the incumbent, the first point by
        `compute_log_ei`, q - 1 points by `compute_log_averaged_ei` (n_samples = 1, zero randomness: the posterior mean and the
        prior variance given z and the points chosen so far).  grid=None draws the reference's grid from `rng`
        (sample='normal': mean + randn std; 'uniform': lower + rand (upper - lower)).  Every step is one grid evaluation
        (`dagnn_sgp_ei_step` on the GPU: one launch and one 32-byte read) and, with refine='lbfgs', the reference's L-BFGS-B from
        the best grid row (float64 on the host, scipy); refine=None returns the best grid rows.  refine='multistart' refines
        on the device instead (csrc/sgp_refine.hip; no scipy): the `starts` <= 32 rows with the smallest finite key of the
        step, each a projected L-BFGS run of at most `max_evals` evaluations (`refine_host` is the definition), advanced in
        lock-step in float64; the step's point is the best of them, and the step still reads the device once.  Both defaults
        come from a CPU prototype on synthetic models, not from a BO run on the real latent spaces."""
        _check_refine(refine, lower, upper, starts, max_evals)
        q, d = int(q), self.d_input
        if not 1 <= q <= MAX_Q:
            raise ValueError("batched_greedy_ei: 1 <= q <= %d needed (got %d)" % (MAX_Q, q))
        lo, up = _bounds(lower, d, "lower"), _bounds(upper, d, "upper")
        if grid is None:
            rng = np.random if rng is None else rng
            if sample == "normal":
                if mean is None or std is None:
                    raise ValueError("batched_greedy_ei: sample='normal' needs mean and std")
                grid = np.asarray(mean, dtype=np.float64) + rng.randn(int(grid_size), d) * np.asarray(std, dtype=np.float64)
            elif sample == "uniform":
                grid = lo + rng.rand(int(grid_size), d) * (up - lo)
            else:
                raise ValueError("batched_greedy_ei: sample must be 'normal' or 'uniform' (got %r)" % (sample,))
        grid = _as_rows(grid, d, "batched_greedy_ei")
        if grid.shape[0] < 1:
            raise ValueError("batched_greedy_ei: the grid has no row")
        D = self.derived()
        points, info = _greedy_flow(self._steps(D, grid, q, refine, lo, up, starts, max_evals), D, q)
        return (points, info) if return_info else points

    # ----------------------------------------------------------------------------- refine="multistart" on the device
    def _derived64(self, D):
        """The float64 device operands of csrc/sgp_refine.hip, built when refine='multistart' first asks for them and kept
        with `D` for the parameter version (the other paths never pay for them)."""
        if getattr(D, "z64", None) is None:
            t = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(self.device)   # noqa: E731
            D.z64, D.inv_ls64, D.a64, D.G64, D.W64 = t(D.z), t(D.inv_ls), t(D.a), t(D.G), t(D.W)
        return D


# --------------------------------------------------------------------------------- a BO round
def bo_round(sgp: SparseGP, model, q: int, lower, upper, mean=None, std=None, data=None, decode_attempts: int = 500,
             data_type: Optional[str] = None, **greedy):
    """bo.py:289-306 as two calls: `batched_greedy_ei` proposes q latent points, then `decode_and_score` (with a `BnData`: the
    BN objective) or `decode_from_latent_space` decodes them on `model`.  Returns (points [q, nz] float64 numpy, strings,
    scores float64 numpy [q] or None).  `greedy`: further arguments of `batched_greedy_ei` (sample, grid, grid_size, rng,
    refine, starts, max_evals)."""
    from . import bn_score, dvae
    points = sgp.batched_greedy_ei(q, lower, upper, mean, std, **greedy)
    dev = next(model.parameters()).device
    zq = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev)
    if data is not None:
        strings, scores = bn_score.decode_and_score(zq, model, data, decode_attempts=decode_attempts)
        return points, strings, scores
    strings = dvae.decode_from_latent_space(zq, model, decode_attempts=decode_attempts, data_type=data_type or "ENAS")
    return points, strings, None
