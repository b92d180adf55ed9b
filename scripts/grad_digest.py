"""The bits of a training step, recorded from the outside: small models (seeded weights, 3-graph code2 batches of at most 40
nodes, D-VAE batches of 8-node graphs) run two training steps each, and the sha256 of the loss and of every parameter gradient
of both steps is written as JSON with sorted keys.  Run it on two commits: equal files mean that no bit of a gradient moved.

    python scripts/grad_digest.py OUT.json

The cases are those of `route_cases.py` that train, plus what it takes to cover every reverse path once: hidden sizes 64 and
72 (gate blocks at a pitch), one and two stacked layers and directions, with and without the edge encoder; the reverse
dataflow sweep with and without static rows from the forward launch, the reverse lock-step launches, the 320-wide and the 512-wide
paths; an `attn_x` model; the D-VAE encoders (fused read-out, all-node read-out, BN, `gated_sum`); the constructor-string
variants on the per-layer sweep and `add` / `max` on the persistent kernels; an empty batch.  `engine.TABLE_GRADS = 1`: the
embedding-table gradients in their one fixed order (torch's atomic `index_add_` is not repeatable).  Only names both commits
have are used."""
import hashlib
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dagnn_amd import DAGNN, DAGNN_BN, DAGNN_NA, ASTNodeEncoder, engine, synth  # noqa: E402
from oracle.seeding import seeded_fill  # noqa: E402


def code2(name, H=64, L=2, bidir=True, wea=True, agg="attn_h", flags=None, backend=None, empty=False, **kw):
    return dict(name=name, kind="code2", H=H, L=L, bidir=bidir, wea=wea, agg=agg, flags=flags or {}, backend=backend, empty=empty, kw=kw)


def dvae_case(name, kind, hs=64, **kw):
    return dict(name=name, kind=kind, H=hs, L=2, flags={}, kw=kw)


def all_cases():
    out = []
    for H in (64, 72):
        for L in (1, 2):
            for bidir in (True, False):
                for wea in (True, False):
                    out.append(code2("main_h%d_L%d_%ddir%s" % (H, L, 1 + bidir, "" if wea else "_no_edge_attr"), H, L, bidir, wea))
    out += [code2("stat_fwd0", flags={"STAT_FWD": 0}), code2("bwd_df_max_bytes0", flags={"BWD_DF_MAX_BYTES": 0}),
            code2("bwd_dataflow0", flags={"BWD_DATAFLOW": 0}), code2("dataflow0", flags={"DATAFLOW": 0}),
            code2("h256_L1", 256, 1), code2("h300_L2", 300), code2("h300_L2_stat_fwd0", 300, flags={"STAT_FWD": 0}),
            code2("h320_L1", 320, 1), code2("h384_L2", 384), code2("h512_L2", 512), code2("h512_L1", 512, 1),
            code2("attn_x_h64", agg="attn_x"), code2("self_attn_h_h64", agg="self_attn_h"),
            dvae_case("na_fused", "na"), dvae_case("na_output_all", "na", out_pool_all=True), dvae_case("na_hs501", "na", 501),
            dvae_case("bn", "bn"), dvae_case("bn_hs501", "bn", 501), dvae_case("na_gated_sum", "na", agg="gated_sum")]
    for agg in ("gated_sum", "mattn_h", "add", "max"):
        out.append(code2("variant_%s" % agg, agg=agg))
    out += [code2("variant_add_h72_no_edge_attr", 72, wea=False, agg="add"), code2("variant_recurr0", recurr=0),
            code2("variant_agg_x", agg="gated_sum", agg_x=True),
            code2("plain_add_dataflow", agg="add", backend="dataflow"), code2("plain_max_dataflow", agg="max", backend="dataflow"),
            code2("plain_max_dataflow_h72_L1_1dir", 72, 1, False, agg="max", backend="dataflow"),
            code2("empty_batch", empty=True), code2("empty_batch_add", agg="add", empty=True)]
    assert len({c["name"] for c in out}) == len(out)
    return out


def build(case, seed):
    H, L = case["H"], case["L"]
    if case["kind"] == "code2":
        m = DAGNN(num_vocab=8, max_seq_len=2, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(H, 98, 10030, 20),
                  w_edge_attr=case["wea"], num_layers=L, bidirectional=case["bidir"], agg=case["agg"], out_wx=False,
                  out_pool_all=False, out_pool="max", dropout=0.0, **case["kw"])
        if case["backend"]:
            m.variant_backend = case["backend"]
        G = synth.code2_batch(seed, 3, 20, 40)
        if case["empty"]:   # the same fields, no node, no edge, no graph
            for k, v in list(vars(G).items()):
                setattr(G, k, 0 if k == "num_graphs" else v[:1] if k == "ptr" else v[:, :0] if k == "edge_index" else v[:0])
    else:
        cls, nn_, rows, dec = (DAGNN_NA, 8, synth.enas_rows, synth.decode_enas_row) if case["kind"] == "na" else \
            (DAGNN_BN, 10, synth.bn_rows, synth.decode_bn_row)
        m = cls(nn_, H, H, nn_, nn_, 0, 1, hs=H, nz=56, num_nodes=nn_, num_layers=L, bidirectional=case["kind"] == "bn", **case["kw"])
        G = synth.dvae_batch([dec(r) for r in rows(seed, 5)])
    seeded_fill(m, 100 + seed)
    return m, G


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def train_steps(m, G, dev, steps=2):
    """`steps` times: zero the gradients, forward, a loss every output reaches, backward, one plain SGD update."""
    out = {}
    m.train()
    for s in range(steps):
        m.zero_grad(set_to_none=True)
        y = m(G.clone().to(dev))
        loss = y.square().mean() if torch.is_tensor(y) else sum(p.square().mean() for p in y)
        loss.backward()
        torch.cuda.synchronize()
        m.check()
        out["step%d/loss" % s] = sha(loss)
        for k, p in sorted(m.named_parameters()):
            out["step%d/grad/%s" % (s, k)] = None if p.grad is None else sha(p.grad)
        with torch.no_grad():
            for p in m.parameters():
                if p.grad is not None:
                    p.sub_(0.05 * p.grad)
    out["path"] = str(getattr(m, "last_variant_path", None))
    return out


def main():
    dev = torch.device("cuda:0")
    engine.TABLE_GRADS = 1
    cases = {}
    for seed, case in enumerate(all_cases()):
        saved = {k: getattr(engine, k) for k in case["flags"]}
        try:
            for k, v in case["flags"].items():
                setattr(engine, k, v)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                m, G = build(case, seed)
                cases[case["name"]] = train_steps(m.to(dev), G, dev)
        except (ValueError, IndexError, AttributeError, RuntimeError, engine.DagnnHipError) as e:
            # an empty batch a model class does not accept says so, on both commits alike; anything else ends the run
            if not case.get("empty") or "illegal memory access" in str(e):
                raise
            cases[case["name"]] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
        finally:
            for k, v in saved.items():
                setattr(engine, k, v)
        print(case["name"], len(cases[case["name"]]), cases[case["name"]].get("error", ""), flush=True)
    text = json.dumps({"cases": cases}, sort_keys=True, indent=0) + "\n"
    with open(sys.argv[1], "w") as f:
        f.write(text)
    print("%d cases, %d digests, sha256 %s" % (len(cases), sum(len(c) for c in cases.values()), hashlib.sha256(text.encode()).hexdigest()))


if __name__ == "__main__":
    main()
