#!/usr/bin/env python
"""Generate the `*_attn_x` fixtures of the BN D-VAE: the REAL reference's `DAGNN_BN` (dvae/dagnn_bn.py) with the
input-keyed aggregators `agg='attn_x'` (encoder, `loss()` / `.backward()`, `decode()`) and `agg='self_attn_x'` (encoder
only: its decoder path calls an undefined `attn_linear`, dvae/dagnn_bn.py:311-315).

Runs only in the build container (needs the reference).  Same recipe as make_golden_dvae_gated.py: the encoder fixtures
come from make_golden.py's `make_bn` / `make_bn_grad`, the loss and decode cases use the helpers of
make_golden_dvae_loss.py and make_golden_dvae_decode.py.  The reference runs unmodified in eval() mode, `_ipropagate_to`,
`np.random.choice` and `torch.rand_like` are wrapped at run time to record padding widths and draws, and decode seeds
whose smallest decision margin is below 1e-4 are rejected.  `meta["agg"]` makes tests/helpers.dvae_model build the
matching model.  (`make_golden.make_ipropagate` builds its model with agg='attn_h' itself: there is no single-vertex
step fixture, tests check that step against the float64 restatement.)

    python tests/golden/make_golden_dvae_bn_attn_x.py
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
from make_golden import REF, _save, _setup_paths, make_bn, make_bn_grad, sample_grad  # noqa: E402
from make_golden_dvae_decode import MIN_MARGIN, _decode  # noqa: E402
from make_golden_dvae_loss import _record_widths  # noqa: E402
from oracle.seeding import seeded_fill  # noqa: E402
from dagnn_amd import synth  # noqa: E402

AGG = "attn_x"
NZ = 56
N = NVT = 10   # BN: ten variables, the type of a vertex is its variable (emb_dim == nvt, which the type keys need)


def _model(ref_mod, hs, L):
    return ref_mod.DAGNN_BN(NVT, hs, hs, N, NVT, 0, 1, hs=hs, nz=NZ, num_nodes=N, agg=AGG, num_layers=L, bidirectional=True,
                            out_wx=False, out_pool_all=False, out_pool="max", dropout=0.0).eval()


def make_loss(ref_mod, ref_util, name, *, hs, L, B, w_seed, data_seed, with_encode=False):
    rows = synth.bn_rows(data_seed, B)
    graphs = [ref_util.decode_BN_to_pygraph(r)[0] for r in rows]
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
    meta = dict(kind="bn", agg=AGG, hs=hs, L=L, B=B, w_seed=w_seed, data_seed=data_seed, bidir=True, encode=with_encode,
                grad_stride=strides, state_dict={k: list(v.shape) for k, v in model.state_dict().items()})
    _save(name, meta, **arrays)


def make_decode(ref_mod, name, *, hs, L, B, w_seed, z_seed, stochastic):
    n = N
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
    meta = dict(kind="bn", agg=AGG, hs=hs, L=L, B=B, n=n, w_seed=ws, z_seed=seed, stochastic=stochastic, bidir=True,
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
    ref_bn = importlib.import_module("dagnn_bn")
    if decode:
        for st in (False, True):
            make_decode(ref_bn, "dvae_decode_bn_attn_x_h32_L3_" + ("sample" if st else "argmax"), hs=32, L=3, B=16, w_seed=281,
                        z_seed=91, stochastic=st)
        make_decode(ref_bn, "dvae_decode_bn_attn_x_h501_L2_sample", hs=501, L=2, B=8, w_seed=283, z_seed=93, stochastic=True)
        return
    ref_batch_mod = importlib.import_module("batch")
    make_bn(ref_bn, ref_util, ref_batch_mod, "bn_h64_attn_x", hs=64, L=2, bidir=True, w_seed=271, data_seed=21, nrows=12, agg=AGG)
    make_bn(ref_bn, ref_util, ref_batch_mod, "bn_h64_self_attn_x", hs=64, L=2, bidir=False, w_seed=272, data_seed=22, nrows=12,
            out_pool_all=True, out_pool="mean", agg="self_attn_x")
    make_bn_grad(ref_bn, ref_util, "grad_bn_h64_attn_x", hs=64, L=2, bidir=True, w_seed=273, data_seed=23, nrows=10, agg=AGG)
    make_bn_grad(ref_bn, ref_util, "grad_bn_h64_self_attn_x", hs=64, L=2, bidir=True, w_seed=274, data_seed=24, nrows=10,
                 agg="self_attn_x")
    make_loss(ref_bn, ref_util, "dvae_loss_bn_attn_x_h32_L3", hs=32, L=3, B=16, w_seed=275, data_seed=81)
    make_loss(ref_bn, ref_util, "dvae_loss_bn_attn_x_h501_L2", hs=501, L=2, B=8, w_seed=276, data_seed=82)
    make_loss(ref_bn, ref_util, "dvae_loss_bn_attn_x_h32_encode", hs=32, L=2, B=16, w_seed=277, data_seed=83, with_encode=True)


if __name__ == "__main__":
    main()
