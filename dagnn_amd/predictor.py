"""The performance predictor of the D-VAE loop (`--predictor` of dvae/train.py:184-191, 243-250, 262-263, 305-308 and of
bayesian_optimization/bo.py:250-286), on the device.

The reference hangs `Linear(nz, hs) -> Tanh -> Linear(hs, 1)` on mu, adds `MSELoss(reduction='sum')` against every graph's
score to the loss and trains the predictor with the encoder; `bo.py --predictor` then scores latent points with it in place
of the sparse GP.  Here: `attach_predictor` (the reference's modules under the reference's names, so checkpoints load both
ways), `predictor_mse` (values and every gradient in one HIP launch), `predict_latent` (a latent matrix in one launch per
chunk), `predictor_report` (the RMSE and Pearson r that bo.py prints, from six float64 sums made on the device).  Kernels:
csrc/predictor.hip; layout and limits: DESIGN.md 15.

    attach_predictor(model)                                     # before the optimizer is built
    loss, recon, kld, pred = train_epoch(model, optimizer, store, train_ids, 32, seed=epoch, predictor=True)
    rmse = test_predictor(model, store, test_ids, 64)
    scores = predict_latent(model, Z_test)
    fit = predictor_report(model, Z_test, Y_test, mean_y_train, std_y_train)     # {'rmse', 'pearson', 'n'}
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import engine
from ._lib import PREDICTOR_MAX_HS as MAX_HS
from ._lib import PREDICTOR_MAX_NZ as MAX_NZ

__all__ = ["attach_predictor", "predictor_mse", "predict_latent", "fit_sums_host", "predictor_report", "MAX_NZ", "MAX_HS"]

_LIMITS = "the predictor kernels serve 1 <= nz <= %d and 1 <= hs <= %d" % (MAX_NZ, MAX_HS)


def _check_widths(nz: int, hs: int, who: str) -> None:
    if not (1 <= int(nz) <= MAX_NZ and 1 <= int(hs) <= MAX_HS):
        raise ValueError("%s: %s (got nz=%d, hs=%d)" % (who, _LIMITS, nz, hs))


def attach_predictor(model, hs: Optional[int] = None):
    """`model.predictor = Sequential(Linear(nz, hs), Tanh(), Linear(hs, 1))` and `model.mseloss = MSELoss(reduction='sum')`,
    exactly as dvae/train.py:185-191 (there hs is the model's own `--hs`: the default here).  The state_dict gains
    `predictor.0.weight`, `predictor.0.bias`, `predictor.2.weight`, `predictor.2.bias`: a reference `--predictor` checkpoint
    loads with strict=True and ours loads in the reference.  Attach before the optimizer is built (and before `.to(device)`,
    or move the model again): the four tensors are then ordinary parameters of the model.  Returns the model."""
    nz = int(model.nz)
    hs = int(model.hs if hs is None else hs)
    _check_widths(nz, hs, "attach_predictor")
    model.predictor = nn.Sequential(nn.Linear(nz, hs), nn.Tanh(), nn.Linear(hs, 1))
    model.mseloss = nn.MSELoss(reduction="sum")
    ref = next((p for p in model.parameters() if p.is_cuda), None)
    if ref is not None:
        model.predictor.to(ref.device)
    return model


def _predictor_of(model, who: str):
    pred = getattr(model, "predictor", None)
    if not isinstance(pred, nn.Sequential) or len(pred) != 3 or not isinstance(pred[0], nn.Linear) or \
            not isinstance(pred[1], nn.Tanh) or not isinstance(pred[2], nn.Linear) or pred[2].out_features != 1 or \
            pred[2].in_features != pred[0].out_features or pred[0].bias is None or pred[2].bias is None:
        raise ValueError("%s: the model has no predictor Linear(nz, hs) -> Tanh -> Linear(hs, 1) (call attach_predictor first)"
                         % who)
    _check_widths(pred[0].in_features, pred[0].out_features, who)
    return pred[0], pred[2]


class _PredictorMSE(torch.autograd.Function):
    """sum (predictor(mu) - y)^2 and y_pred, values and gradients in one HIP launch (`dagnn_predictor_mse`); the backward scales
    the kept gradients by the incoming scalar.  The gradient that arrives for y_pred (nothing in the D-VAE loop sends one)
    is not propagated: y_pred is marked non-differentiable."""

    @staticmethod
    def forward(ctx, mu, y, W1, b1, W2, b2):
        need = [mu.requires_grad, W1.requires_grad, b1.requires_grad, W2.requires_grad, b2.requires_grad]
        y_pred, loss, ctx.grads, ctx.dmu = engine.predictor_mse(mu, y, W1, b1, W2, b2, any(need), need[0])
        ctx.need = need
        y_pred = y_pred.view(-1, 1)
        ctx.mark_non_differentiable(y_pred)
        return loss[0], y_pred

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_pred):
        # out of place: `backward(retain_graph=True)` may run this again on the same kept gradients
        need = ctx.need
        out = [ctx.dmu * g if need[0] else None, None]
        for want, t in zip(need[1:], ctx.grads):
            out.append(t * g if want else None)
        return tuple(out)


def _targets(y, B: int, device) -> torch.Tensor:
    """`torch.FloatTensor(y_batch).unsqueeze(1).to(device)` of train.py:244 as a flat fp32 [B] tensor: `y` [B] or [B, 1], a
    tensor on any device or a host list / array."""
    if not isinstance(y, torch.Tensor):
        y = torch.as_tensor(np.asarray(y, dtype=np.float32))
    if y.numel() != B:
        raise ValueError("predictor_mse: y must hold one score per row of mu (got %s for %d rows)" % (tuple(y.shape), B))
    if y.dim() > 2 or (y.dim() == 2 and y.shape[1] != 1):
        raise ValueError("predictor_mse: y must be [B] or [B, 1] (got %s)" % (tuple(y.shape),))
    y = y.reshape(B)
    if y.dtype != torch.float32:
        y = y.to(torch.float32)
    if y.device != device:
        y = y.pin_memory().to(device, non_blocking=True) if (device.type == "cuda" and not y.is_cuda) else y.to(device)
    return y


def predictor_mse(model, mu: torch.Tensor, y):
    """`(pred_loss, y_pred)` of dvae/train.py:244-246: y_pred = model.predictor(mu) [B, 1] and pred_loss =
    model.mseloss(y_pred, y) = sum (y_pred - y)^2.  `mu` [B, nz] fp32 (a view with a row pitch is read in place); `y` [B] or
    [B, 1] - fp32 on the device (`b.y` of a DagStore batch), or a host list as the reference passes it.

    On the GPU everything is ONE launch (`dagnn_predictor_mse`): with gradients enabled it also leaves d mu and the four
    parameter gradients for an upstream gradient of 1, and the backward only multiplies them by the gradient that arrives
    (d mu is skipped when mu needs none).  Under `no_grad` the forward-only form runs; its values are the same bits.  The
    parameters are read in place on every call.  Gradients flow through pred_loss only; y_pred is returned detached.
    On CPU tensors it is the reference's own two lines on torch ops.  nz > 128 or hs > 1024: ValueError."""
    l1, l2 = _predictor_of(model, "predictor_mse")
    if not isinstance(mu, torch.Tensor) or mu.dim() != 2 or mu.shape[0] < 1 or mu.shape[1] != l1.in_features:
        raise ValueError("predictor_mse: mu must be [B >= 1, nz=%d] (got %s)"
                         % (l1.in_features, tuple(mu.shape) if isinstance(mu, torch.Tensor) else type(mu)))
    y = _targets(y, mu.shape[0], mu.device)
    if not mu.is_cuda:
        y_pred = model.predictor(mu)
        return model.mseloss(y_pred, y.unsqueeze(1)), y_pred.detach()
    if torch.is_grad_enabled():
        return _PredictorMSE.apply(mu, y, l1.weight, l1.bias, l2.weight, l2.bias)
    y_pred, loss, _, _ = engine.predictor_mse(mu, y, l1.weight, l1.bias, l2.weight, l2.bias, False, False)
    return loss[0], y_pred.view(-1, 1)


def predict_latent(model, Z, batch_rows: Optional[int] = None) -> torch.Tensor:
    """`model.predictor(torch.FloatTensor(Z).to(device))` of bo.py:251, 277 as pred [M] fp32 on the model's device, without
    gradients: `dagnn_predictor_forward`, one launch (or one per `batch_rows` rows - the result is the same bits, a row's
    arithmetic does not depend on its neighbours).  `Z` [M, nz]: a tensor or a numpy array.  A row gives the bits
    `predictor_mse` gives for it.  A predictor on the CPU runs the torch modules."""
    l1, l2 = _predictor_of(model, "predict_latent")
    dev = l1.weight.device
    if not isinstance(Z, torch.Tensor):
        Z = torch.as_tensor(np.ascontiguousarray(Z, dtype=np.float32))
    if Z.dim() != 2 or Z.shape[1] != l1.in_features:
        raise ValueError("predict_latent: Z must be [M, nz=%d] (got %s)" % (l1.in_features, tuple(Z.shape)))
    if batch_rows is not None and int(batch_rows) < 1:
        raise ValueError("predict_latent: batch_rows must be positive")
    if Z.dtype != torch.float32:
        Z = Z.to(torch.float32)
    if Z.device != dev:
        Z = Z.to(dev, non_blocking=True)
    M = Z.shape[0]
    step = M if batch_rows is None else int(batch_rows)
    with torch.no_grad():
        if dev.type != "cuda":
            return model.predictor(Z).reshape(M)
        out = torch.empty(M, dtype=torch.float32, device=dev)
        for i in range(0, M, max(step, 1)):
            engine.predictor_forward(Z[i:i + step], l1.weight, l1.bias, l2.weight, l2.bias, out=out[i:i + step])
    return out


def fit_sums_host(pred, y, mean: float, std: float) -> np.ndarray:
    """The definition `dagnn_fit_sums` implements, in numpy float64: with p = (-pred - mean) / std (bo.py:253),
    [sum p, sum y, sum p^2, sum y^2, sum p y, sum (p - y)^2]."""
    h = lambda a: (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64).reshape(-1)   # noqa: E731
    p = (-h(pred) - float(mean)) / float(std)
    t = h(y)
    return np.array([p.sum(), t.sum(), (p * p).sum(), (t * t).sum(), (p * t).sum(), ((p - t) ** 2).sum()], dtype=np.float64)


def _report(s, n: int) -> dict:
    sp, sy, spp, syy, spy, sd = (float(v) for v in s)
    cov, vp, vy = spy - sp * sy / n, spp - sp * sp / n, syy - sy * sy / n
    pearson = cov / math.sqrt(vp * vy) if vp > 0 and vy > 0 else float("nan")
    return {"rmse": math.sqrt(sd / n), "pearson": pearson, "n": n}


def predictor_report(model, Z, Y, mean: float, std: float) -> dict:
    """What bo.py:263-286 prints of the predictor on (Z, Y), Y in the units bo.py compares in (its y_test / y_train: negated,
    standardised scores): with p = (-predictor(Z) - mean) / std (bo.py:253),
        rmse = sqrt(mean (p - Y)^2)   (bo.py:265),    pearson = pearsonr(p, Y)[0]   (bo.py:269),    n = len(Y).
    `predict_latent`, then six float64 sums in one launch (`dagnn_fit_sums`) and ONE read of 48 bytes - the only
    synchronisation of the call; a predictor on the CPU takes `fit_sums_host`.  The reference's `testll` is left out: with
    uncert = 0 it is a log-density at scale 0 (bo.py:254, 266) and carries no information."""
    pred = predict_latent(model, Z)
    if not isinstance(Y, torch.Tensor):
        Y = torch.as_tensor(np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1)))
    n = pred.numel()
    if Y.numel() != n or n < 1:
        raise ValueError("predictor_report: Y must hold one value per row of Z (got %d for %d rows)" % (Y.numel(), n))
    if not float(std) > 0:
        raise ValueError("predictor_report: std must be positive (got %r)" % (std,))
    if not pred.is_cuda:
        return _report(fit_sums_host(pred, Y, mean, std), n)
    return _report(engine.fit_sums(pred, Y.to(pred.device, non_blocking=True), mean, std).tolist(), n)
