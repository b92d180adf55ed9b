#!/usr/bin/env python
"""Generate the `dvae_gated_*` fixtures: the REAL reference's `DVAE_PYG.loss()` / `.backward()` and `decode()`
(dvae/models_pyg.py:338-456) for `DAGNN(agg='gated_sum')` (dvae/dagnn.py), the original D-VAE's aggregator.

Runs only in the build container (needs the reference).  Same recipe as make_golden_dvae_loss.py and
make_golden_dvae_decode.py, whose helpers it uses: the reference runs unmodified in eval() mode, `_ipropagate_to`,
`np.random.choice` and `torch.rand_like` are wrapped at run time to record padding widths and draws, and decode seeds
whose smallest decision margin is below 1e-4 are rejected.  `meta["agg"]` makes tests/helpers.dvae_model build the
matching model.

    python tests/golden/make_golden_dvae_gated.py
"""
from __future__ import annotations

import copy
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _save, _setup_paths, sample_grad  # noqa: E402
from make_golden_dvae_decode import MIN_MARGIN, _decode  # noqa: E402
from make_golden_dvae_loss import _record_widths  # noqa: E402
from oracle.seeding import seeded_fill  # noqa: E402
from dagnn_amd import synth  # noqa: E402

AGG = "gated_sum"
NZ = 56


def _model(ref_mod, hs, L):
    n = nvt = 8   # ENAS: num_nodes == max_n, which the gated decoder's one-hot vertex ids need
    return ref_mod.DAGNN(nvt, hs, hs, n, nvt, 0, 1, hs=hs, nz=NZ, num_nodes=n, agg=AGG, num_layers=L, bidirectional=False,
                         out_wx=False, out_pool_all=False, out_pool="max", dropout=0.0).eval()


def make_loss(ref_mod, ref_util, name, *, hs, L, B, w_seed, data_seed, with_encode=False):
    rows = synth.enas_rows(data_seed, B)
    graphs = [ref_util.decode_ENAS_to_pygraph(r)[0] for r in rows]
    model = _model(ref_mod, hs, L)
    seeded_fill(model, w_seed)
    rng = np.random.default_rng(data_seed + 1000)
    if with_encode:
        mu, logvar = model.encode([copy.deepcopy(g) for g in graphs])
        mu.retain_grad()
        logvar.retain_grad()
    else:
        mu = torch.from_numpy(rng.standard_normal((B, NZ)).astype(np.float32)).requires_grad_(True)
        logvar = torch.from_numpy((rng.standard_normal((B, NZ)) * 0.3).astype(np.float32)).requires_grad_(True)
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
    meta = dict(kind="na", agg=AGG, hs=hs, L=L, B=B, w_seed=w_seed, data_seed=data_seed, bidir=False, encode=with_encode,
                grad_stride=strides, state_dict={k: list(v.shape) for k, v in model.state_dict().items()})
    _save(name, meta, **arrays)


def make_decode(ref_mod, name, *, hs, L, B, w_seed, z_seed, stochastic):
    n = 8
    model = _model(ref_mod, hs, L)
    for attempt in range(50):
        ws, seed = w_seed + 100 * attempt, z_seed + 1000 * attempt
        seeded_fill(model, ws)
        rng = np.random.default_rng(seed)
        z = torch.from_numpy(rng.standard_normal((B, NZ)).astype(np.float32))
        G, u_type, u_edge, widths, coupled, margin = _decode(model, z, n, B, stochastic, seed + 1)
        if margin >= MIN_MARGIN:
            break
        print("%s: seeds %d / %d rejected (margin %.2e)" % (name, ws, seed, margin))
    else:
        raise SystemExit("%s: no seed with a decision margin >= %g" % (name, MIN_MARGIN))
    types = np.full((B, n), -1, dtype=np.int32)
    preds = np.zeros((B, n), dtype=np.int64)
    nv = np.zeros(B, dtype=np.int32)
    states = np.zeros((B, n, hs), dtype=np.float32)
    edges = []
    for b, g in enumerate(G):
        nv[b] = g.vcount()
        types[b, :nv[b]] = g.vs["type"]
        for u, v in g.get_edgelist():
            preds[b, v] |= 1 << u
        edges.append(g.get_edgelist())
        top = g.vs.deleted["H_forward%d" % (L - 1)]
        for v in range(nv[b]):
            states[b, v] = top[v].numpy()[0]
    loose = [bin(int(preds[b, nv[b] - 1])).count("1") for b in range(B)]
    meta = dict(kind="na", agg=AGG, hs=hs, L=L, B=B, n=n, w_seed=ws, z_seed=seed, stochastic=stochastic, bidir=False,
                margin=margin, edge_order=[[list(e) for e in es] for es in edges],
                coverage=dict(early_end=int((nv < n).sum()), forced_end=int((nv == n).sum()),
                              end_joins_two=int(sum(x >= 2 for x in loose)), coupled_updates=int(sum(coupled))))
    print(name, meta["coverage"], "margin %.2e" % margin)
    _save(name, meta, z=z.numpy(), u_type=u_type[None], u_edge=u_edge[None], types=types, preds=preds, nv=nv,
          states=states, widths=np.array(widths, dtype=np.int64))


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not found at %s - fixtures can only be regenerated in the build container" % REF)
    decode = "--decode" in sys.argv
    if not decode:   # (the decode fixtures need another igraph stand-in: they run in a process of their own)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--decode"], check=True)
    _setup_paths()
    if decode:
        sys.path.insert(0, os.path.join(HERE, "decode_standin"))   # ahead of oracle/pyg_standin's igraph
    torch.manual_seed(0)
    ref_util = importlib.import_module("util")
    ref_na = importlib.import_module("dagnn")
    if not decode:
        make_loss(ref_na, ref_util, "dvae_gated_loss_na_h64_L2", hs=64, L=2, B=16, w_seed=251, data_seed=61)
        make_loss(ref_na, ref_util, "dvae_gated_loss_na_h501_L2", hs=501, L=2, B=32, w_seed=252, data_seed=62)
        make_loss(ref_na, ref_util, "dvae_gated_loss_na_h64_encode", hs=64, L=2, B=16, w_seed=253, data_seed=63,
                  with_encode=True)
        return
    for st in (False, True):
        make_decode(ref_na, "dvae_gated_decode_na_h64_L2_" + ("sample" if st else "argmax"), hs=64, L=2, B=16, w_seed=261,
                    z_seed=71, stochastic=st)
    make_decode(ref_na, "dvae_gated_decode_na_h501_L2_sample", hs=501, L=2, B=32, w_seed=263, z_seed=73, stochastic=True)


if __name__ == "__main__":
    main()
