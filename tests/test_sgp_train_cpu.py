"""The sparse GP's fused training step on the CPU: `energy_grad_host` (the float64 mirror of csrc/sgp_train.hip's analytic
adjoints) and `train_via_adam(grad="hip")` on a CPU model.

Yardstick (DESIGN.md 4i's convention, measured per case, never fixed):
  g_ref    `SparseGP.energy` differentiated by torch autograd in float64 on the CPU - the code as it stood before the step.
  g_white  a second, independent float64 evaluation: `white_energy` below restates the whitened formulas of DESIGN.md 17 on
           torch.linalg.cholesky / solve_triangular and lets autograd differentiate them.
  bound    per parameter p, on max|g_new - g_ref| / max|g_ref|: 4 delta_p with delta_p = max|g_white - g_ref| / max|g_ref|,
           floored at the summation bound terms_p * eps * sum|terms| of csrc/sgp_train.hip (`terms`: the additions behind one
           value).  For a gradient sum|terms| is taken at the gradient's own scale max|g_ref| (no cancellation assumed: the
           stricter reading).  The energy likewise with |E_white - E_ref| / |E_ref|; its terms do cancel - b G is a difference
           of log-determinants and quadratic forms that grow with LParamPost while E does not - so its sum|terms| is formed
           term by term from the whitened restatement (`white_energy`'s third result), never from the code under test.
A case whose own delta_p exceeds 1e-6 is badly conditioned: `reference` refuses it instead of tolerating it.
The references of a shape are computed once per process and shared with tests/test_sgp_train_gpu.py."""
import math

import numpy as np
import pytest
import torch

from dagnn_amd import sgp

EPS = float(np.finfo(np.float64).eps)
NAMES = ["lls", "lsf", "z", "mParamPost", "LParamPost", "lvar_noise"]
# (n, d, M, b, trained)
SMALL = [(2, 1, 1, 1, False), (40, 3, 7, 9, False), (200, 5, 33, 65, False), (300, 3, 65, 64, True)]
LARGE = (3000, 56, 500, 1000, False)
_REF = {}


def terms(d, M, b):
    """Additions behind one value, from csrc/sgp_train.hip: the final contraction plus the products that feed its terms."""
    return {"E": b + 4 * M, "lls": M * (b + M) + 3 * M, "lsf": M * (b + M) + b + 3 * M, "z": (b + M) + 3 * M,
            "mParamPost": 2 * M + b, "LParamPost": 2 * M + b, "lvar_noise": b + 2 * M}


def white_energy(params, X, y, n_points):
    """The whitened form of the energy on torch ops, for autograd; independent of dagnn_amd.sgp.  Returns (E,
    v [b], sum|terms| of E)."""
    lls, lsf, z, mP, Lp, lvn = params
    M, b, n = z.shape[0], X.shape[0], float(n_points)
    c = (n - 1.0) / n
    sf, il = torch.exp(lsf), torch.exp(-lls)
    eye = torch.eye(M, dtype=torch.float64)

    def kern(a, q):
        df = a[:, None, :] - q[None, :, :]
        return sf * torch.exp(-0.5 * (df * df * il).sum(-1))

    L = torch.linalg.cholesky(kern(z, z) + 1e-3 * sf * eye)
    C = Lp.T @ L
    A = C.T @ C
    Lc, L1 = torch.linalg.cholesky(eye + c * A), torch.linalg.cholesky(eye + A)
    t = L.T @ mP.reshape(M, 1)
    wc = torch.linalg.solve_triangular(Lc, t, upper=False)
    w1 = torch.linalg.solve_triangular(L1, t, upper=False)
    G = -torch.log(torch.diagonal(Lc)).sum() + 0.5 * c * c * (wc * wc).sum() \
        - (1.0 - 1.0 / n) * (-torch.log(torch.diagonal(L1)).sum() + 0.5 * (w1 * w1).sum())
    U = torch.linalg.solve_triangular(L, kern(X, z).T, upper=False)
    Q = torch.linalg.solve_triangular(Lc, U, upper=False)
    v = sf - (U * U).sum(0) + (Q * Q).sum(0)
    mean = c * (Q * wc).sum(0)
    out = v.abs() + torch.exp(lvn)
    ll = -0.5 * torch.log(2.0 * math.pi * out) - 0.5 * (y.reshape(-1) - mean) ** 2 / out
    mass = b * (torch.log(torch.diagonal(Lc)).abs().sum() + 0.5 * c * c * (wc * wc).sum()
                + c * (torch.log(torch.diagonal(L1)).abs().sum() + 0.5 * (w1 * w1).sum())) + ll.abs().sum()
    return b * G + ll.sum(), v, mass.detach()


def autograd_of(fn, params):
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    E = fn(ps)
    return E.detach(), [g.detach() for g in torch.autograd.grad(E, ps)]


def problem(n, d, M, b, trained=False):
    """A CPU model at the start of `train_via_adam` (or 30 Adam steps past it) and its minibatch: (model, X [b, d], y [b, 1])."""
    rng = np.random.RandomState(0)
    X = rng.randn(n, d)
    y = np.sin(X.sum(1)) + 0.1 * rng.randn(n)
    g = sgp.SparseGP(X, y, M, device="cpu")
    g.initialize(np.random.RandomState(1))
    if trained:
        g.train_via_adam(max_iterations=15, minibatch_size=(n + 1) // 2, learning_rate=1e-2, rng=np.random.RandomState(2),
                         verbose=False, initialize=False)
    rows = torch.arange(b)
    if n == 2:   # (the one row must not be the inducing row itself: every kernel derivative would be exactly zero)
        rows = torch.tensor([int((g.X[:, 0] != g.z[0, 0]).nonzero()[0])])
    return g, g.X[rows].clone(), g.y[rows].clone()


def energy_ref(g, params, X, y):
    """The parent's energy at `params` (a list in get_params() order) - `SparseGP.energy` on a shallow copy of the model."""
    import copy
    h = copy.copy(g)
    h.lls, h.lsf, h.z, h.mParamPost, h.LParamPost, h.lvar_noise = params
    return h.energy(X, y)


def reference(case):
    """{'g': model, 'X', 'y', 'E_ref', 'g_ref', 'E_white', 'g_white', 'bound_E', 'bounds': [6]} of a case, computed once."""
    if case in _REF:
        return _REF[case]
    n, d, M, b, trained = case
    g, X, y = problem(n, d, M, b, trained)
    tm = terms(d, M, b)
    _REF[case] = yardstick(g, X, y, tm)
    return _REF[case]


def yardstick(g, X, y, tm):
    """g_ref, g_white and the bounds at the model's present parameters."""
    n = g.n_points
    params = [p.detach().clone() for p in g.get_params()]
    E_ref, g_ref = autograd_of(lambda ps: energy_ref(g, ps, X, y), params)
    E_white, g_white = autograd_of(lambda ps: white_energy(ps, X, y, n)[0], params)
    mass = float(white_energy(params, X, y, n)[2])
    delta_E = abs(float(E_white - E_ref)) / abs(float(E_ref))
    deltas = [float((a - r).abs().max() / r.abs().max()) for a, r in zip(g_white, g_ref)]
    assert delta_E <= 1e-6 and max(deltas) <= 1e-6, "badly conditioned case: delta_E %.3g, delta_p %r" % (delta_E, deltas)
    return {"g": g, "X": X, "y": y, "E_ref": E_ref, "g_ref": g_ref, "E_white": E_white, "g_white": g_white,
            "delta_E": delta_E, "deltas": deltas, "bound_E": max(4.0 * delta_E, tm["E"] * EPS * mass / abs(float(E_ref))),
            "bounds": [max(4.0 * dl, tm[nm] * EPS) for dl, nm in zip(deltas, NAMES)]}


def check_against_ref(what, case, E, grads):
    """Print every figure, then assert the yardstick."""
    R = reference(case)
    E = E.detach().cpu().double().reshape(())
    err_E = abs(float(E - R["E_ref"])) / abs(float(R["E_ref"]))
    print("%s %r: E err %.3g (delta %.3g, bound %.3g)" % (what, case, err_E, R["delta_E"], R["bound_E"]))
    bad = [] if err_E <= R["bound_E"] else ["E"]
    for nm, gn, gr, dl, bd in zip(NAMES, grads, R["g_ref"], R["deltas"], R["bounds"]):
        gn = gn.detach().cpu().double()
        assert gn.shape == gr.shape, (nm, gn.shape, gr.shape)
        err = float((gn - gr).abs().max() / gr.abs().max())
        print("    %-11s err %.3g  delta_p %.3g  ratio %.2f  bound %.3g" % (nm, err, dl, err / max(dl, 1e-300), bd))
        if not err <= bd:
            bad.append(nm)
    assert not bad, "%s %r: beyond the bound: %s" % (what, case, bad)


@pytest.mark.parametrize("case", SMALL + [LARGE], ids=lambda c: "n%d-d%d-M%d-b%d%s" % (c[:4] + ("-trained" if c[4] else "",)))
def test_energy_grad_host_against_autograd(case):
    R = reference(case)
    E, grads = sgp.energy_grad_host(R["g"].get_params(), R["X"], R["y"], R["g"].n_points)
    check_against_ref("energy_grad_host", case, E, grads)


def test_energy_and_grad_on_a_cpu_model_is_the_host_mirror():
    R = reference(SMALL[1])
    g = R["g"]
    E, grads = g.energy_and_grad(R["X"], R["y"])
    E2, grads2 = sgp.energy_grad_host(g.get_params(), R["X"], R["y"], g.n_points)
    assert torch.equal(E, E2) and all(torch.equal(a, q) for a, q in zip(grads, grads2))
    assert [tuple(a.shape) for a in grads] == [tuple(p.shape) for p in g.get_params()]
    assert g.train_failures() == 0


def hand_loop(g, epochs, mb, lr, rng, step):
    """The reference's shuffle and minibatches with `step(X, y) -> (E, grads)` and torch's Adam on minus the energy."""
    params = g.get_params()
    opt = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    X, y, n = g.X, g.y, g.n_points
    last = None
    for _ in range(epochs):
        perm = torch.from_numpy(np.asarray(rng.choice(n, n, replace=False), dtype=np.int64)).to(X.device)
        X, y = X[perm], y[perm]
        for i in range(int(np.ceil(n / mb))):
            E, grads = step(X[i * mb:min((i + 1) * mb, n)], y[i * mb:min((i + 1) * mb, n)])
            for p, q in zip(params, grads):
                p.grad = -q
            opt.step()
            last = E
    for p in params:
        p.grad = None
    return float(last)


def fresh(n, d, M, device="cpu"):
    rng = np.random.RandomState(3)
    X = rng.randn(n, d)
    y = np.sin(X.sum(1)) + 0.1 * rng.randn(n)
    return sgp.SparseGP(X, y, M, device=device)


def test_train_via_adam_hip_equals_the_hand_written_loop_bitwise():
    # 3 epochs of 2 minibatches, the last one short (25 rows + 16)
    a, h = fresh(41, 3, 7), fresh(41, 3, 7)
    e1 = a.train_via_adam(max_iterations=3, minibatch_size=25, learning_rate=1e-2, rng=np.random.RandomState(5), verbose=False,
                          grad="hip")
    rng = np.random.RandomState(5)
    h.initialize(rng, 25)
    e2 = hand_loop(h, 3, 25, 1e-2, rng, lambda X, y: sgp.energy_grad_host(h.get_params(), X, y, h.n_points))
    assert e1 == e2
    for p, q in zip(a.get_params(), h.get_params()):
        assert torch.equal(p, q) and not p.requires_grad and p.grad is None
    start = fresh(41, 3, 7)
    start.initialize(np.random.RandomState(5), 25)
    assert not torch.equal(a.z, start.z)   # the loop moved the parameters


def test_grad_autograd_is_the_default_bitwise():
    a, h = fresh(41, 3, 7), fresh(41, 3, 7)
    kw = dict(max_iterations=2, minibatch_size=25, learning_rate=1e-2, verbose=False)
    e1 = a.train_via_adam(rng=np.random.RandomState(5), **kw)
    e2 = h.train_via_adam(rng=np.random.RandomState(5), grad="autograd", **kw)
    assert e1 == e2 and all(torch.equal(p, q) for p, q in zip(a.get_params(), h.get_params()))


def test_argument_checks():
    g = fresh(41, 3, 7)
    g.initialize(np.random.RandomState(1))
    with pytest.raises(ValueError):
        g.train_via_adam(max_iterations=1, verbose=False, grad="triton")
    with pytest.raises(ValueError):
        g.train_via_adam(max_iterations=1, minibatch_size=0, verbose=False, grad="hip")
    with pytest.raises(ValueError):
        g.energy_and_grad(g.X[:4, :2], g.y[:4])          # a column short
    with pytest.raises(ValueError):
        g.energy_and_grad(g.X[:4], g.y[:3])              # a target short
    with pytest.raises(ValueError):
        g.energy_and_grad(g.X[:0], g.y[:0])              # no row
    with pytest.raises(ValueError):
        g.energy_and_grad(torch.full((2, 3), float("nan"), dtype=torch.float64), g.y[:2])
