"""The sparse GP's fused training step on the GPU (csrc/sgp_train.hip: dagnn_sgp_energy_grad) against float64 on the CPU.

The yardstick is that of tests/test_sgp_train_cpu.py (g_ref = the parent's `energy` under float64 autograd; bound = 4x the error
of an independent whitened evaluation, floored at the summation bound), and its references are shared.  Shapes: one tile
(M = 1, 7), the 16-wide MFMA tile and the 64-wide product tile +- 1 (M = 33, 64, 65; b = 63, 64, 65), a second factorisation
panel (M = 65), d below and above 56, a single row, and the workload's own M = 500, b = 1000 once."""
import numpy as np
import pytest
import torch

from dagnn_amd import _lib, engine, sgp

from .test_sgp_train_cpu import (LARGE, SMALL, check_against_ref, fresh, hand_loop, problem, reference, white_energy)

pytestmark = pytest.mark.gpu

CASES = SMALL + [(200, 57, 64, 63, False), (200, 3, 33, 1, False), LARGE]
IDS = ["n%d-d%d-M%d-b%d%s" % (c[:4] + ("-trained" if c[4] else "",)) for c in CASES]


def on_gpu(g, device):
    """A GPU model with the CPU model's data and parameters."""
    h = sgp.SparseGP(g.X.numpy(), g.y.numpy(), g.n_inducing, device=device)
    h.set_params(g.get_params())
    return h


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_energy_and_grad_against_autograd_and_host(device, case):
    R = reference(case)
    h = on_gpu(R["g"], device)
    E, grads = h.energy_and_grad(R["X"].to(device), R["y"].to(device))
    assert E.is_cuda and E.dtype == torch.float64 and all(a.is_cuda and a.dtype == torch.float64 for a in grads)
    assert h.train_failures() == 0
    check_against_ref("dagnn_sgp_energy_grad", case, E, grads)
    # against the host mirror of the same adjoints: both sit inside the bound around g_ref, so within twice the bound of each other
    Eh, gh = sgp.energy_grad_host(R["g"].get_params(), R["X"], R["y"], R["g"].n_points)
    assert abs(float(E.cpu() - Eh)) <= 2.0 * R["bound_E"] * abs(float(R["E_ref"]))
    for a, q, r, bd in zip(grads, gh, R["g_ref"], R["bounds"]):
        assert float((a.cpu() - q).abs().max()) <= 2.0 * bd * float(r.abs().max())


def test_v_cannot_turn_negative_and_large_LParamPost_stays_inside_the_bound(device):
    """The sign(v) branch: v = (sf - k Kzz^-1 k^T) + |Q|^2, and the bracket is the Schur complement of the positive definite
    [[Kzz, k^T], [k, sf (1 + 1e-3)]] less the jitter - positive for every finite parameter set.  Scaling LParamPost up only
    drives |Q| to 0 and v down to that bracket, never below it, so no input reaches v < 0 and the branch cannot be exercised
    from outside; in the kernel it is the expression d_v = sign(v) d_out of the host mirror.  What can be checked: v_white stays
    positive over 100 decades of the scale, and at a scale where the case is still well conditioned the GPU's gradients hold
    the yardstick."""
    n, d, M, b = 200, 5, 33, 65
    g, X, y = problem(n, d, M, b)
    L0 = g.LParamPost.clone()
    for scale in (1.0, 1e2, 1e4, 1e8, 1e50, 1e100):
        g.LParamPost.copy_(L0 * scale)
        v = white_energy(g.get_params(), X, y, n)[1]
        print("scale %g: min v_white %.6g" % (scale, float(v.min())))
        assert float(v.min()) > 0.0
    g.LParamPost.copy_(L0 * 1e2)
    case = ("scaled", n, d, M, b)
    from . import test_sgp_train_cpu as T
    T._REF[case] = T.yardstick(g, X, y, T.terms(d, M, b))
    E, grads = on_gpu(g, device).energy_and_grad(X.to(device), y.to(device))
    check_against_ref("dagnn_sgp_energy_grad, LParamPost x 100", case, E, grads)


def test_two_calls_are_bitwise_equal_and_a_row_does_not_depend_on_b(device):
    case = (200, 5, 33, 128, False)
    g, X, y = problem(*case)
    h = on_gpu(g, device)
    Xd, yd = X.to(device), y.to(device)
    E1, g1 = h.energy_and_grad(Xd, yd)
    E2, g2 = h.energy_and_grad(Xd, yd)
    assert torch.equal(E1, E2) and all(torch.equal(a, q) for a, q in zip(g1, g2))
    # E = b G + sum of the rows' terms, G independent of the rows: E[0:64) + E[64:128) = E[0:128) exactly in b G, and the
    # rows' terms must agree within the energy's bound (the scale: the largest of the three energies)
    Ea, _ = h.energy_and_grad(Xd[:64], yd[:64])
    Eb, _ = h.energy_and_grad(Xd[64:], yd[64:])
    R = reference(case)
    scale = max(abs(float(E1)), abs(float(Ea)), abs(float(Eb)))
    print("E %.17g, halves %.17g + %.17g, difference %.3g, bound %.3g" % (float(E1), float(Ea), float(Eb),
                                                                           abs(float(Ea) + float(Eb) - float(E1)), R["bound_E"] * scale))
    assert abs(float(Ea) + float(Eb) - float(E1)) <= R["bound_E"] * scale
    assert h.train_failures() == 0


def test_train_via_adam_hip_equals_the_hand_written_loop_bitwise(device):
    # (200, 5, 33): 2 epochs of 2 minibatches, the last one short (128 rows + 72)
    a, h = fresh(200, 5, 33, device), fresh(200, 5, 33, device)
    e1 = a.train_via_adam(max_iterations=2, minibatch_size=128, learning_rate=1e-2, rng=np.random.RandomState(5), verbose=False,
                          grad="hip")
    rng = np.random.RandomState(5)
    h.initialize(rng, 128)
    z0 = h.z.clone()
    e2 = hand_loop(h, 2, 128, 1e-2, rng, lambda X, y: h.energy_and_grad(X, y))
    assert e1 == e2 and np.isfinite(e1)
    for p, q in zip(a.get_params(), h.get_params()):
        assert torch.equal(p, q) and not p.requires_grad and p.grad is None
    assert not torch.equal(a.z, z0) and h.train_failures() == 0


def test_nan_parameters_give_nan_and_count_and_training_raises(device):
    g, X, y = problem(200, 5, 33, 65)
    h = on_gpu(g, device)
    with torch.no_grad():
        h.lls[2] = float("nan")
    E, grads = h.energy_and_grad(X.to(device), y.to(device))
    assert bool(torch.isnan(E)) and all(bool(torch.isnan(a).any()) for a in grads)
    assert h.train_failures() > 0 and h.train_failures() == 0   # (read and reset)
    with pytest.raises(_lib.DagnnHipError):
        h.train_via_adam(max_iterations=1, minibatch_size=128, verbose=False, initialize=False, grad="hip")


def test_limits_raise_value_error(device):
    with pytest.raises(ValueError):
        engine.sgp_energy_grad_words(513, 3, 10)
    with pytest.raises(ValueError):
        engine.sgp_energy_grad_words(7, 129, 10)
    with pytest.raises(ValueError):
        engine.sgp_energy_grad_words(7, 3, 0)
    assert engine.sgp_energy_grad_words(512, 128, 1000) > 0
