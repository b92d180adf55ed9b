"""refine="multistart" on the GPU (csrc/sgp_refine.hip: dagnn_sgp_refine_eval, dagnn_sgp_refine_run) against float64 on the CPU.

The evaluation alone is held against the module's own float64 numpy evaluation (`_posterior_point`, `_Factor.point`); the bound
is 4x the error that an independent float64 evaluation - the re-inverted-matrix form of tests/test_sgp_refine_cpu.py, explicit
inverses and the expanded square - shows against the same values, floored at the summation bound terms * eps * sum|terms| of the sum behind the value (the
convention of tests/test_sgp_train_gpu.py: with one start and a small model the independent evaluation can hit a value
exactly).  terms = Me; sum|terms| is |a|_1 sf for the mean, 2 sf for v = sf - |T k|^2 (positive, so |T k|^2 < sf), the
gradient's own scale max|.| for the two gradient vectors (no cancellation assumed: the stricter reading), and for f the two
floors of mean and v carried through |df / d mean| and |df / d v| plus 8 eps max(1, |f|) for sqrt, erfc, exp and log.  Both
errors and the floor are printed.  The whole refinement is held against the mirror `refine_host` on the same starts: status and evaluation count
per start equal, points within 1e-9 (1 + |x|).  The kernels are bitwise repeatable, so a seed either always passes or never;
the seeds below are the first ones tried unless a comment says otherwise."""
import math

import numpy as np
import pytest
import torch

from dagnn_amd import _lib, engine, sgp, synth
from dagnn_amd.bn_score import BnData

from . import helpers as Hh
from .test_sgp_refine_cpu import make, ref_kernel, ref_objective, step_objectives

pytestmark = pytest.mark.gpu

_MODELS = {}


def model(d, M, device):
    """One model per shape for the whole module (nothing below changes its parameters)."""
    if (d, M) not in _MODELS:
        g, P, rng = make(d, M, n=max(40, M + 20), device=device)
        _MODELS[(d, M)] = (g, P)
    return _MODELS[(d, M)]


def operands(g, P, q, rng, device):
    """The float64 device operands after j = 0 .. q chosen points, and the host factor of each j."""
    D = g._derived64(g.derived())
    M, d = D.M, D.d
    pts = 0.8 * rng.randn(q, d)
    fac, facs = sgp._Factor(D, q), []
    for j in range(q):
        fac.extend(pts[j])
        snap = sgp._Factor(D, q)
        snap.ze[:], snap.W[:], snap.Me = fac.ze, fac.W, fac.Me
        facs.append(snap)
    ze, We = torch.from_numpy(fac.ze).to(device), torch.from_numpy(fac.W).to(device)
    return D, pts, facs, ze, We


def independent(P, X, chosen):
    """(mean, v, d mean / dx, d v / dx) per row of X from explicit inverses: the posterior (chosen = None) or the averaged EI."""
    lls, lsf, z, m, L, _ = P
    ls, sf, M = np.exp(lls), np.exp(lsf), z.shape[0]
    KzzInv = np.linalg.inv(ref_kernel(lls, lsf, z, z) + np.eye(M) * sgp.JITTER * sf)
    cov = np.linalg.inv(KzzInv + L @ L.T)
    beta = (KzzInv @ (cov @ m))[:, 0]
    if chosen is None:
        ze, B = z, KzzInv @ cov @ KzzInv - KzzInv
    else:
        ze = np.concatenate([z, chosen], 0)
        B = -np.linalg.inv(ref_kernel(lls, lsf, ze, ze) + np.eye(ze.shape[0]) * sgp.JITTER * sf)
    K = ref_kernel(lls, lsf, X, ze)
    dK = -K[:, :, None] * (X[:, None, :] - ze[None, :, :]) / ls[None, None, :]
    return K[:, :M] @ beta, sf + np.sum(K * (K @ B), 1), np.einsum("m,smc->sc", beta, dK[:, :M]), \
        2.0 * np.einsum("sm,smc->sc", K @ B, dK)


EPS = float(np.finfo(np.float64).eps)


def held(name, got, want, indep, floor):
    e_got, e_ind = float(np.abs(got - want).max()), float(np.abs(indep - want).max())
    print("%s: kernel err %.3g, independent float64 err %.3g (ratio %.3g), floor %.3g" % (name, e_got, e_ind, e_got / max(e_ind, 1e-300), floor))
    assert e_got <= max(4.0 * e_ind, floor), (name, e_got, e_ind, floor)


# Me crosses a multiple of 4 and of 16 (15, 16, 17, 18; 30 .. 34), d = 3 and 5, S = 1, 5, 17, and one case with more than
# one row of tiles, more than one workgroup per product and both lane halves of the coordinates in use
EVAL_CASES = [(15, 3, 1, 3), (15, 5, 17, 3), (30, 5, 5, 4), (30, 3, 17, 4), (130, 56, 17, 3), (70, 70, 5, 2)]


@pytest.mark.parametrize("M,d,S,q", EVAL_CASES)
def test_the_evaluation_alone(device, M, d, S, q):
    g, P = model(d, M, device)
    rng = np.random.RandomState(M + d + S)
    D, pts, facs, ze, We = operands(g, P, q, rng, device)
    X = 0.8 * rng.randn(S, d)
    Xd = torch.from_numpy(X).to(device)
    inc = float(sgp.predict_host(D, g.X.cpu().numpy())[0].min())
    # the incumbent's objective: the mean alone
    f, mean, v, dm, dv = [t.cpu().numpy() for t in engine.sgp_refine_eval(_lib.SGP_REFINE_MEAN, Xd, ze, D.inv_ls64, D.sf, D.a64)]
    want = [sgp._posterior_point(D, x) for x in X]
    ind = independent(P, X, None)
    a1 = float(np.abs(D.a).sum())
    held("mean (M %d d %d S %d)" % (M, d, S), mean, np.array([w[0] for w in want]), ind[0], M * EPS * a1 * D.sf)
    held("d mean / dx", dm, np.stack([w[2] for w in want]), ind[2], M * EPS * np.abs(np.stack([w[2] for w in want])).max())
    np.testing.assert_array_equal(f, mean)
    for j in range(q + 1):
        if j == 0:
            out = engine.sgp_refine_eval(_lib.SGP_REFINE_EI, Xd, ze, D.inv_ls64, D.sf, D.a64, D.G64, M, False, inc)
            want, ind = [sgp._posterior_point(D, x) for x in X], independent(P, X, None)
        else:
            out = engine.sgp_refine_eval(_lib.SGP_REFINE_EI, Xd, ze, D.inv_ls64, D.sf, D.a64, We, M + j, True, inc)
            want, ind = [facs[j - 1].point(x) for x in X], independent(P, X, pts[:j])
            full = engine.sgp_refine_eval(_lib.SGP_REFINE_EI, Xd, ze, D.inv_ls64, D.sf, D.a64, We, M + j, False, inc)
        f, mean, v, dm, dv = [t.cpu().numpy() for t in out]
        tag, Me = "Me %d" % (M + j), M + j
        dm_w, dv_w = np.stack([w[2] for w in want]), np.stack([w[3] for w in want])
        fl_m, fl_v = M * EPS * a1 * D.sf, Me * EPS * 2.0 * D.sf
        held(tag + " mean", mean, np.array([w[0] for w in want]), ind[0], fl_m)
        held(tag + " v", v, np.array([w[1] for w in want]), ind[1], fl_v)
        held(tag + " d mean / dx", dm, dm_w, ind[2], M * EPS * np.abs(dm_w).max())
        held(tag + " d v / dx", dv, dv_w, ind[3], Me * EPS * np.abs(dv_w).max())
        pt = [sgp._neg_log_ei_point(w[0], w[1], inc) for w in want]
        f_want = np.array([t[0] for t in pt])
        f_ind = np.array([sgp._neg_log_ei_point(a, b, inc)[0] for a, b in zip(ind[0], ind[1])])
        assert np.isfinite(f_want).all()
        held(tag + " f", f, f_want, f_ind, max(abs(t[1]) * fl_m + abs(t[2]) * fl_v + 8.0 * EPS * max(1.0, abs(t[0])) for t in pt))
        if j > 0:   # the skipped tiles hold zeros: the full product gives the same sums but for the split of k among the waves
            held(tag + " d v / dx, all tiles", full[4].cpu().numpy(), dv_w, ind[3], Me * EPS * np.abs(dv_w).max())


def test_the_objective_on_its_branches(device):
    """-log EI and its gradient on the series branch (s < -10) and where the variance is not positive."""
    g, P = model(3, 15, device)
    D = g._derived64(g.derived())
    rng = np.random.RandomState(5)
    X = 0.8 * rng.randn(5, 3)
    Xd = torch.from_numpy(X).to(device)
    want = [sgp._posterior_point(D, x) for x in X]
    inc = min(w[0] for w in want) - 12.0 * math.sqrt(max(w[1] for w in want))
    f = engine.sgp_refine_eval(_lib.SGP_REFINE_EI, Xd, D.z64, D.inv_ls64, D.sf, D.a64, D.G64, 15, False, inc)[0].cpu().numpy()
    f_want = np.array([sgp._neg_log_ei_point(w[0], w[1], inc)[0] for w in want])
    assert all((inc - w[0]) / math.sqrt(w[1]) < -10 for w in want)
    np.testing.assert_allclose(f, f_want, rtol=1e-12, atol=0)
    f = engine.sgp_refine_eval(_lib.SGP_REFINE_EI, Xd, D.z64, D.inv_ls64, D.sf, D.a64, 1e3 * D.G64, 15, False, inc)[0].cpu().numpy()
    assert np.isnan(f).all()   # |T k|^2 above sf: no positive variance


def starts_and_objective(g, P, device, d, M, S, q, seed):
    rng = np.random.RandomState(seed)
    D, pts, facs, ze, We = operands(g, P, q, rng, device)
    lo, up = -1.5 * np.ones(d), 1.5 * np.ones(d)
    X0 = (lo + rng.rand(S, d) * (up - lo)).astype(np.float32).astype(np.float64)
    X0[0] = 2.0                                          # a start outside the bounds: clipped onto a corner
    inc = float(sgp.predict_host(D, g.X.cpu().numpy())[0].min())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    return D, facs, ze, We, lo, up, X0, inc, t


@pytest.mark.parametrize("d,M,S,q,seed", [(3, 15, 5, 3, 0), (5, 30, 17, 4, 0), (56, 130, 8, 2, 0)])
def test_the_whole_refinement_against_the_mirror(device, d, M, S, q, seed):
    g, P = model(d, M, device)
    D, facs, ze, We, lo, up, X0, inc, t = starts_and_objective(g, P, device, d, M, S, q, seed)
    stages = [("mean", _lib.SGP_REFINE_MEAN, None, M, False, lambda x: sgp._posterior_point(D, np.asarray(x).reshape(-1))[0::2]),
              ("posterior", _lib.SGP_REFINE_EI, D.G64, M, False, sgp._ei_objective(lambda x: sgp._posterior_point(D, x), inc)),
              ("averaged", _lib.SGP_REFINE_EI, We, M + q, True, sgp._ei_objective(facs[-1].point, inc))]
    for name, mode, T, Me, tri, fun in stages:
        out, xs = engine.sgp_refine_run(mode, t(X0), t(lo), t(up), ze, D.inv_ls64, D.sf, D.a64, T, Me, tri, inc, 64, want_points=True)
        again = engine.sgp_refine_run(mode, t(X0), t(lo), t(up), ze, D.inv_ls64, D.sf, D.a64, T, Me, tri, inc, 64, want_points=True)
        assert torch.equal(out.view(torch.int64), again[0].view(torch.int64)) and torch.equal(xs.view(torch.int64), again[1].view(torch.int64))
        out, xs = out.cpu().numpy(), xs.cpu().numpy()
        x, f, info = sgp.refine_host(fun, X0, lo, up, 64)
        status, evals = out[2 + d:2 + d + S].astype(int).tolist(), out[2 + d + S:2 + d + 2 * S].astype(int).tolist()
        print(name, "status", status, "evals", evals, "mirror", info["status"], info["evals"])
        assert status == info["status"] and evals == info["evals"]
        assert int(out[0]) == info["best"]
        err = np.abs(xs - info["x"]) / (1.0 + np.abs(info["x"]))
        print(name, "largest point difference %.3g, f difference %.3g" % (err.max(), np.abs(out[2 + d + 2 * S:] - info["f"]).max()))
        assert err.max() <= 1e-9
        np.testing.assert_allclose(out[2:2 + d], x, rtol=0, atol=1e-9 * (1.0 + np.abs(x).max()))
        assert (xs >= lo).all() and (xs <= up).all()
        assert xs[0, 0] <= 1.5 and all(fun(xs[k])[0] <= fun(np.clip(X0[k], lo, up))[0] for k in range(S))


def test_dead_starts_and_the_start_count(device):
    g, P = model(3, 15, device)
    D, facs, ze, We, lo, up, X0, inc, t = starts_and_objective(g, P, device, 3, 15, 5, 3, 1)
    # a factor 1000 G drives the variance below zero everywhere: every start is dead, there is no best start
    out = engine.sgp_refine_run(_lib.SGP_REFINE_EI, t(X0), t(lo), t(up), ze, D.inv_ls64, D.sf, D.a64, 1e3 * D.G64, 15, False, inc, 8)
    out = out.cpu().numpy()
    assert out[0] == -1 and np.isnan(out[1]) and out[5:10].tolist() == [4.0] * 5 and out[10:15].tolist() == [1.0] * 5
    # nstart = 2: the rows from 2 on are never evaluated
    n2 = torch.tensor([2], dtype=torch.int32, device=device)
    out = engine.sgp_refine_run(_lib.SGP_REFINE_MEAN, t(X0), t(lo), t(up), ze, D.inv_ls64, D.sf, D.a64, max_evals=16, nstart=n2).cpu().numpy()
    assert out[0] in (0, 1) and out[7:10].tolist() == [4.0] * 3 and out[12:15].tolist() == [0.0] * 3 and (out[10:12] >= 1).all()
    two = engine.sgp_refine_run(_lib.SGP_REFINE_MEAN, t(X0[:2]), t(lo), t(up), ze, D.inv_ls64, D.sf, D.a64, max_evals=16).cpu().numpy()
    np.testing.assert_array_equal(out[1:5], two[1:5])
    with pytest.raises(ValueError):
        engine.sgp_refine_run(_lib.SGP_REFINE_MEAN, t(X0), t(lo), t(up), ze, D.inv_ls64, D.sf, D.a64, max_evals=3)
    with pytest.raises(ValueError):
        engine.sgp_refine_run(_lib.SGP_REFINE_MEAN, t(np.zeros((33, 3))), t(lo), t(up), ze, D.inv_ls64, D.sf, D.a64)
    with pytest.raises(ValueError):
        engine.sgp_refine_eval(_lib.SGP_REFINE_EI, t(X0), ze, D.inv_ls64, D.sf, D.a64, D.G64, 19, False, inc)   # Me above ze's rows


@pytest.mark.parametrize("d,M,N", [(3, 7, 60), (8, 32, 400)])
def test_batched_greedy_ei_end_to_end(device, d, M, N):
    g, P = model(d, M, device)
    rng = np.random.RandomState(d + M)
    lo, up = -1.5 * np.ones(d), 1.5 * np.ones(d)
    grid = (lo + rng.rand(N, d) * (up - lo)).astype(np.float32).astype(np.float64)
    q = 4
    pts, info = g.batched_greedy_ei(q, lo, up, grid=grid, refine="multistart", return_info=True)
    again = g.batched_greedy_ei(q, lo, up, grid=grid, refine="multistart")
    np.testing.assert_array_equal(pts, again)                     # bitwise repeatable
    assert pts.shape == (q, d) and pts.dtype == np.float64 and (pts >= lo).all() and (pts <= up).all()
    assert len(info["starts"]) == q + 1 and all(r["best"] >= 0 for r in info["starts"])
    inc = info["incumbent"]
    assert inc <= g.get_incumbent(grid, refine=None) + 1e-6       # (the grid's mean is fp32)
    assert g.get_incumbent(grid, lo, up, refine="multistart") == inc
    funs = step_objectives(g.derived(), pts, inc)
    for j in range(q):
        x0 = np.clip(grid[info["index"][j]], lo, up)
        f_ref = ref_objective(P, np.stack([pts[j], x0]), pts, inc, j)
        assert f_ref[0] <= f_ref[1] + 1e-9 * max(1.0, abs(f_ref[1])), (j, f_ref)
    spo = pytest.importorskip("scipy.optimize")
    for j in range(q):
        x0 = np.clip(grid[info["index"][j]], lo, up)
        xs, fs = sgp._refine(funs[j], x0, lo, up)                 # the host 'lbfgs' result on the same objective
        f_mine = funs[j](pts[j])[0]
        print("step %d: multistart %.12g lbfgs %.12g (above by %.3g)" % (j, f_mine, fs, f_mine - fs))
        assert f_mine <= fs + 1e-7 * max(1.0, abs(fs)), (j, f_mine, fs)
    few = g.batched_greedy_ei(2, lo, up, grid=grid[:5], refine="multistart", starts=16)     # a grid smaller than `starts`
    assert few.shape == (2, d) and (few >= lo).all() and (few <= up).all()
    one = g.batched_greedy_ei(2, lo, up, grid=grid, refine="multistart", starts=1, max_evals=4)
    assert one.shape == (2, d)


def test_the_other_modes_never_build_the_float64_operands(device):
    g, P, rng = make(3, 7, device=device)
    grid = rng.randn(40, 3)
    g.batched_greedy_ei(2, -1.5, 1.5, grid=grid, refine=None)
    assert not hasattr(g.derived(), "z64")
    g.batched_greedy_ei(2, -1.5, 1.5, grid=grid, refine="multistart")
    assert g.derived().z64.dtype == torch.float64 and g.derived().W64.is_cuda


@pytest.mark.parametrize("refine", [None, "lbfgs", "multistart"])
def test_reads_per_greedy_batch(device, monkeypatch, refine):
    """How often a greedy batch waits for the device, counted as `Tensor.cpu` on device tensors: the grid's copy to the host,
    the incumbent and q steps without refinement on the device; with it the incumbent and q steps alone, as long as every
    step has a live start (no step then reads its grid row back)."""
    if refine == "lbfgs":
        pytest.importorskip("scipy.optimize")
    d, M, N, q = 3, 7, 60, 3
    g, P = model(d, M, device)
    g._derived64(g.derived())            # (deriving the operands reads the device too: once per parameter version, not per batch)
    rng = np.random.RandomState(d + M)
    lo, up = -1.5 * np.ones(d), 1.5 * np.ones(d)
    grid = (lo + rng.rand(N, d) * (up - lo)).astype(np.float32).astype(np.float64)
    reads, to_host = [], torch.Tensor.cpu

    def counting(t, *args, **kwargs):
        if t.is_cuda:
            reads.append(tuple(t.shape))
        return to_host(t, *args, **kwargs)

    monkeypatch.setattr(torch.Tensor, "cpu", counting)
    pts, info = g.batched_greedy_ei(q, lo, up, grid=grid, refine=refine, return_info=True)
    monkeypatch.undo()
    print("refine=%r: %d reads, of shapes %s" % (refine, len(reads), reads))
    assert pts.shape == (q, d)
    if refine == "multistart":
        assert all(r["best"] >= 0 for r in info["starts"])
        assert len(reads) == q + 1
    else:
        assert len(reads) == q + 2


def test_bo_round_with_multistart(device):
    model_bn = Hh.dvae_decoder_model("bn", max_n=10, nvt=10, hs=32, L=2, seed=3).to(device)
    nz = model_bn.nz
    rng = np.random.RandomState(4)
    X = rng.randn(60, nz)
    y = np.sin(X.sum(1))
    g = sgp.SparseGP(X, y, 9, device=device)
    g.initialize(rng, 60)
    data = BnData.from_samples(synth.asia_samples(2, 300), [2] * 8, device=device)
    q = 3
    points, strings, scores = sgp.bo_round(g, model_bn, q, -3.0 * np.ones(nz), 3.0 * np.ones(nz), X.mean(0), X.std(0), data=data,
                                           decode_attempts=12, grid_size=200, rng=rng, refine="multistart", starts=8, max_evals=32)
    assert points.shape == (q, nz) and len(strings) == q and scores.shape == (q,) and scores.dtype == np.float64
    assert (points >= -3.0).all() and (points <= 3.0).all()
