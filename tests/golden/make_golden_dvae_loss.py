#!/usr/bin/env python
"""Generate the `dvae_loss_*` fixtures from the REAL reference's `DVAE_PYG.loss()` (dvae/models_pyg.py:398-456).

Runs only in the build container (needs the reference and the igraph stand-in under oracle/pyg_standin).  The
reference's `DAGNN` / `DAGNN_BN` (dvae/dagnn.py, dvae/dagnn_bn.py) run unmodified in eval() mode (z = mu), on graphs
decoded by the reference's own `decode_ENAS_to_pygraph` / `decode_BN_to_pygraph`.  Each fixture stores loss, res, kld
and the gradients of mu, logvar and every parameter, plus the padding width P of every `_ipropagate_to` call, recorded
by wrapping the reference's method at run time.

    python tests/golden/make_golden_dvae_loss.py
"""
from __future__ import annotations

import copy
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _save, _setup_paths, sample_grad  # noqa: E402
from oracle.seeding import seeded_fill  # noqa: E402
from dagnn_amd import synth  # noqa: E402


def _record_widths(model):
    """Wrap (not copy) the reference's `_ipropagate_to`: append the padding width P of every call (0 with H given)."""
    widths = []
    inner = model._ipropagate_to

    def wrapped(G, v, propagator, H=None, reverse=False):
        alive = [g for g in G if g.vcount() > v]
        widths.append(0 if H is not None or not alive else max(len(g.predecessors(v)) for g in alive))
        return inner(G, v, propagator, H, reverse)

    model._ipropagate_to = wrapped
    return widths


def make_loss(ref_mod, ref_util, cls_name, name, *, kind, hs, L, B, w_seed, data_seed, with_encode=False):
    if kind == "na":
        nvt, rows = 8, synth.enas_rows(data_seed, B)
        graphs = [ref_util.decode_ENAS_to_pygraph(r)[0] for r in rows]
    else:
        nvt, rows = 10, synth.bn_rows(data_seed, B)
        graphs = [ref_util.decode_BN_to_pygraph(r)[0] for r in rows]
    model = getattr(ref_mod, cls_name)(nvt, hs, hs, nvt, nvt, 0, 1, hs=hs, nz=56, num_nodes=nvt, agg="attn_h",
                                       num_layers=L, bidirectional=kind == "bn", out_wx=False, out_pool_all=False,
                                       out_pool="max", dropout=0.0).eval()
    seeded_fill(model, w_seed)
    rng = np.random.default_rng(data_seed + 1000)
    if with_encode:
        mu, logvar = model.encode([copy.deepcopy(g) for g in graphs])
    else:
        mu = torch.from_numpy(rng.standard_normal((B, 56)).astype(np.float32)).requires_grad_(True)
        logvar = torch.from_numpy((rng.standard_normal((B, 56)) * 0.3).astype(np.float32)).requires_grad_(True)
    if with_encode:
        mu.retain_grad()
        logvar.retain_grad()
    widths = _record_widths(model)
    loss, res, kld = model.loss(mu, logvar, graphs)
    loss.backward()
    arrays = dict(loss=np.array(float(loss.detach())), res=np.array(float(res.detach())), kld=np.array(float(kld.detach())),
                  mu=mu.detach().numpy(), logvar=logvar.detach().numpy(), widths=np.array(widths, dtype=np.int64),
                  rows=np.array([json.dumps(r) for r in rows]))
    strides = {}
    for k, g in (("mu", mu.grad), ("logvar", logvar.grad)):
        arrays["g::" + k], strides[k], arrays["gsum::" + k] = sample_grad(k, g.numpy())
    for k, p in model.named_parameters():
        g = np.zeros(tuple(p.shape), np.float32) if p.grad is None else p.grad.numpy()
        arrays["g::" + k], strides[k], arrays["gsum::" + k] = sample_grad(k, g)
    meta = dict(kind=kind, hs=hs, L=L, B=B, w_seed=w_seed, data_seed=data_seed, bidir=kind == "bn", encode=with_encode,
                grad_stride=strides, state_dict={k: list(v.shape) for k, v in model.state_dict().items()})
    _save(name, meta, **arrays)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not found at %s - fixtures can only be regenerated in the build container" % REF)
    _setup_paths()
    torch.manual_seed(0)
    ref_util = importlib.import_module("util")
    ref_na = importlib.import_module("dagnn")
    ref_bn = importlib.import_module("dagnn_bn")
    make_loss(ref_na, ref_util, "DAGNN", "dvae_loss_na_h64_L2", kind="na", hs=64, L=2, B=16, w_seed=231, data_seed=41)
    make_loss(ref_bn, ref_util, "DAGNN_BN", "dvae_loss_bn_h32_L3", kind="bn", hs=32, L=3, B=12, w_seed=232, data_seed=42)
    make_loss(ref_na, ref_util, "DAGNN", "dvae_loss_na_h501_L2", kind="na", hs=501, L=2, B=32, w_seed=233, data_seed=43)
    make_loss(ref_bn, ref_util, "DAGNN_BN", "dvae_loss_bn_h501_L2", kind="bn", hs=501, L=2, B=32, w_seed=234, data_seed=44)
    make_loss(ref_na, ref_util, "DAGNN", "dvae_loss_na_h64_encode", kind="na", hs=64, L=2, B=16, w_seed=235, data_seed=45,
              with_encode=True)


if __name__ == "__main__":
    main()
