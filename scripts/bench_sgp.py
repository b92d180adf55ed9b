#!/usr/bin/env python
"""Times the sparse GP of the BO loop (dagnn_amd/sgp.py, csrc/sgp.hip) at bo.py's shape: d = 56, M = 500.

  predict            --rows rows (default 5 000, 10 000, 19 020) through `dagnn_sgp_project`, by HIP events around the call,
                     beside the torch-ops form of the same whitened formula (pairwise distances, exp, two matmuls, fp32) on the
                     same GPU and the same fp32 operands - distances from the differences as the kernel has them, and
                     (`torch_mm`) from the expanded square on a matmul as the reference has them
  batched_greedy_ei  q = --q points on a --grid-row grid: the HIP flow without refinement, the same loop on torch ops (one
                     grid evaluation, the argmin and one read per step), the HIP flow with the L-BFGS-B refinement (scipy, on
                     the host) and with refine="multistart" (--starts starts, --max-evals ticks, on the device); wall clock
                     including every synchronisation
  train_via_adam     wall time per Adam step at minibatch --minibatch: the default path (float64 torch ops under autograd) and
                     grad="hip" (csrc/sgp_train.hip) in the same run; one energy + gradient evaluation of each path alone
                     (`energy_grad_*_ms`, their largest relative difference per parameter before anything is timed); and one
                     bo.py-sized fit, --fit-rows rows for --fit-epochs epochs, on each path (--fit-epochs 0 skips it)

Median (and 90th percentile) over --steps windows after --warmup (a `predict` window is 20 calls); the results are checked against each other before anything is
timed.  One JSON line at the end.

    python scripts/bench_sgp.py [--steps 10] [--warmup 3] [--q 50] [--grid 10000] [--train-only]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagnn_amd import sgp  # noqa: E402


def event_ms(fn, steps, warmup, reps=20):
    """Per call, from HIP events around `reps` calls in a row (a window of one 0.2 ms call would measure the clock)."""
    ts = []
    for k in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append(a.elapsed_time(b) / reps)
    return round(float(np.median(ts)), 4), round(float(np.percentile(ts, 90)), 4)


def wall_ms(fn, steps, warmup):
    ts = []
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3), round(float(np.percentile(ts, 90)), 3)


def torch_kernel(D, X32, mm=False):
    """k(X, z) on torch ops: distances from the differences (the kernels' form), or - mm - from the expanded square on a
    matmul (the reference's form, gauss.py:24; it loses digits to cancellation in fp32)."""
    z = D.zt.T
    s = torch.sqrt(D.inv_ls32)
    mode = "use_mm_for_euclid_dist" if mm else "donot_use_mm_for_euclid_dist"
    return D.sf * torch.exp(-0.5 * torch.cdist(X32 * s, z * s, compute_mode=mode) ** 2)


def torch_predict(D, X32, mm=False):
    K = torch_kernel(D, X32, mm)
    GK = K @ D.Tt[:, :D.M]
    return K @ D.a32, (D.sf - (GK * GK).sum(1)).abs() + D.noise


def torch_neg_log_ei(mean, var, inc):
    m, v = mean.double(), var.double()
    sd = torch.sqrt(v)
    u = inc - m
    s = u / sd
    far = s < -10.0
    x = torch.where(far, s, torch.full_like(s, -11.0))
    series = -(1.0 / x - 1.0 / x ** 3 + 3.0 / x ** 5 - 15.0 / x ** 7)
    near = (0.5 * torch.special.erfc(-s * 0.5 ** 0.5)) / (torch.exp(-0.5 * s * s) / (2.0 * np.pi) ** 0.5)
    lei = torch.log(u * torch.where(far, series, near) + sd) - 0.5 * np.log(2.0 * np.pi) - 0.5 * s * s
    return torch.where(v > 0, -lei, torch.full_like(lei, float("nan")))


def torch_greedy(D, grid32, q):
    """The flow of `batched_greedy_ei(refine=None)` on torch ops: the same incremental factor, one read per step."""
    M = D.M
    K = torch_kernel(D, grid32)
    T = K @ D.Tt
    mean = K @ D.a32
    var0 = D.sf - (T[:, :M] ** 2).sum(1)
    r = D.sf - (T[:, M:] ** 2).sum(1)
    U = torch.zeros(grid32.shape[0], M + q, dtype=torch.float32, device=grid32.device)
    U[:, :M] = T[:, M:]
    host = grid32.double().cpu().numpy()
    inc = float(mean.min())
    idx = [int(torch.argmin(torch_neg_log_ei(mean, var0, inc)))]
    fac = sgp._Factor(D, q)
    for _ in range(1, q):
        Me = fac.Me
        p = host[idx[-1]]
        c, delta = fac.extend(p)
        pc = torch.from_numpy(np.concatenate([p, c]).astype(np.float32)).to(grid32.device)
        df = grid32 - pc[:D.d]
        w = (D.sf * torch.exp(-0.5 * (df * df * D.inv_ls32).sum(1)) - U[:, :Me] @ pc[D.d:]) * (1.0 / delta)
        U[:, Me] = w
        r = r - w * w
        idx.append(int(torch.argmin(torch_neg_log_ei(mean, r, inc))))
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[5000, 10000, 19020])
    ap.add_argument("--grid", type=int, default=10000)
    ap.add_argument("--q", type=int, default=50)
    ap.add_argument("--d", type=int, default=56)
    ap.add_argument("--inducing", type=int, default=500)
    ap.add_argument("--minibatch", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-refine", action="store_true")
    ap.add_argument("--starts", type=int, default=16)
    ap.add_argument("--max-evals", type=int, default=64)
    ap.add_argument("--train-only", action="store_true")
    ap.add_argument("--fit-rows", type=int, default=5000)
    ap.add_argument("--fit-epochs", type=int, default=100)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    n, d, M = 4000, a.d, a.inducing
    X = rng.randn(n, d)
    y = np.sin(X[:, :4].sum(1)) + 0.1 * rng.randn(n)
    g = sgp.SparseGP(X, y, M, device=dev)
    out = {"d": d, "M": M, "device": torch.cuda.get_device_name(0)}

    # training first: the timed steps also leave a posterior that is not the start
    g.initialize(rng, a.minibatch)
    t = []
    for k in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.train_via_adam(max_iterations=1, minibatch_size=a.minibatch, learning_rate=5e-4, rng=rng, verbose=False, initialize=False)
        torch.cuda.synchronize()
        if k >= a.warmup:
            t.append((time.perf_counter() - t0) * 1e3 / int(np.ceil(n / a.minibatch)))
    out["adam_step_ms"] = [round(float(np.median(t)), 3), round(float(np.percentile(t, 90)), 3)]
    t = []
    for k in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.train_via_adam(max_iterations=1, minibatch_size=a.minibatch, learning_rate=5e-4, rng=rng, verbose=False, initialize=False,
                         grad="hip")   # (reads the failure counter once per call: every synchronisation is inside the window)
        torch.cuda.synchronize()
        if k >= a.warmup:
            t.append((time.perf_counter() - t0) * 1e3 / int(np.ceil(n / a.minibatch)))
    out["adam_step_hip_ms"] = [round(float(np.median(t)), 3), round(float(np.percentile(t, 90)), 3)]

    # one energy + gradient evaluation of each path, no optimiser
    Xb, yb = g.X[:a.minibatch], g.y[:a.minibatch]

    def autograd_step():
        ps = g.get_params()
        for p in ps:
            p.requires_grad_(True)
        try:
            return torch.autograd.grad(g.energy(Xb, yb), ps)
        finally:
            for p in ps:
                p.requires_grad_(False)

    ga, (_, gh) = autograd_step(), g.energy_and_grad(Xb, yb)
    out["energy_grad_maxreldiff"] = [float((u - v).abs().max() / u.abs().max()) for u, v in zip(ga, gh)]
    out["energy_grad_autograd_ms"] = wall_ms(autograd_step, a.steps, a.warmup)
    out["energy_grad_hip_ms"] = wall_ms(lambda: g.energy_and_grad(Xb, yb), a.steps, a.warmup)
    out["train_failures"] = g.train_failures()

    if a.fit_epochs > 0:   # bo.py:256-260 at the BN loop's size
        Xf = rng.randn(a.fit_rows, d)
        yf = np.sin(Xf[:, :4].sum(1)) + 0.1 * rng.randn(a.fit_rows)
        for path in ("hip", "autograd"):
            f = sgp.SparseGP(Xf, yf, M, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f.train_via_adam(max_iterations=a.fit_epochs, minibatch_size=a.minibatch, learning_rate=5e-4, rng=np.random.RandomState(1),
                             verbose=False, grad=path)
            torch.cuda.synchronize()
            out["fit_%dx%d_%s_s" % (a.fit_rows, a.fit_epochs, path)] = round(time.perf_counter() - t0, 3)
            out["fit_%s_rmse" % path] = round(f.report(f.X, f.y)["rmse"], 6)
    if a.train_only:
        print(json.dumps(out))
        return
    D = g.derived()

    for N in a.rows:
        Z = torch.from_numpy(rng.randn(N, d)).to(dev, torch.float32)
        m, v = g.predict(Z)
        tm, tv = torch_predict(D, Z)
        out["predict_%d_maxdiff" % N] = [float((m[:, 0] - tm.double()).abs().max()), float((v[:, 0] - tv.double()).abs().max())]
        out["predict_%d_hip_ms" % N] = event_ms(lambda: g.predict(Z), a.steps, a.warmup)
        # the call's rate: the products k T^T and k a plus three operations per (row, inducing row, column) of the kernel tile
        out["predict_%d_hip_tflops" % N] = round(N * M * (2.0 * M + 2.0 + 3.0 * d) / (out["predict_%d_hip_ms" % N][0] * 1e-3) / 1e12, 2)
        out["predict_%d_torch_ms" % N] = event_ms(lambda: torch_predict(D, Z), a.steps, a.warmup)
        out["predict_%d_torch_mm_ms" % N] = event_ms(lambda: torch_predict(D, Z, True), a.steps, a.warmup)
        tm2, tv2 = torch_predict(D, Z, True)
        out["predict_%d_torch_mm_maxdiff" % N] = [float((m[:, 0] - tm2.double()).abs().max()), float((v[:, 0] - tv2.double()).abs().max())]

    grid = (X.mean(0) + rng.randn(a.grid, d) * X.std(0)).astype(np.float32)
    g32 = torch.from_numpy(grid).to(dev)
    lo, up = X.min(0), X.max(0)
    _, info = g.batched_greedy_ei(a.q, lo, up, grid=g32, refine=None, return_info=True)
    idx_t = torch_greedy(D, g32, a.q)
    out["greedy_same_rows"] = sum(int(i == j) for i, j in zip(info["index"], idx_t))
    out["greedy_q"], out["greedy_grid"] = a.q, a.grid
    steps, warm = max(a.steps // 2, 3), 1
    out["greedy_hip_ms"] = wall_ms(lambda: g.batched_greedy_ei(a.q, lo, up, grid=g32, refine=None), steps, warm)
    out["greedy_torch_ms"] = wall_ms(lambda: torch_greedy(D, g32, a.q), steps, warm)
    if not a.no_refine:
        out["greedy_hip_lbfgs_ms"] = wall_ms(lambda: g.batched_greedy_ei(a.q, lo, up, grid=g32, refine="lbfgs"), 3, 1)
        # the same call refined on the device: `--starts` starts in lock-step, `--max-evals` ticks of three launches each
        # (two for the products, one that reduces, advances and builds the next kernel columns; one for the incumbent's mean)
        ms = dict(refine="multistart", starts=a.starts, max_evals=a.max_evals)
        _, minfo = g.batched_greedy_ei(a.q, lo, up, grid=g32, return_info=True, **ms)
        runs = minfo["starts"]
        out["greedy_multistart"] = {"starts": a.starts, "max_evals": a.max_evals, "launches_per_tick": 3,
                                    "status": {name: sum(r["status"].count(k) for r in runs) for k, name in enumerate(sgp.REFINE_STATUS)},
                                    "evals_of_the_best_median": float(np.median([r["evals"][r["best"]] for r in runs if r["best"] >= 0])),
                                    "best_is_start_0": sum(int(r["best"] == 0) for r in runs), "steps": len(runs)}
        out["greedy_hip_multistart_ms"] = wall_ms(lambda: g.batched_greedy_ei(a.q, lo, up, grid=g32, **ms), 3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
