"""The ogbg-code2 LP task, CPU tier (-m "not gpu"): `ASTNodeEncoder2`, the numpy mirrors of the csrc/lp.hip kernels and the
host side of `dagnn_amd.lp` against fixtures generated from the reference (tests/golden/make_golden_code2_lp.py)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dagnn_amd
from dagnn_amd import ASTNodeEncoder2, ClassAccuracy, lp
from oracle.seeding import seeded_fill
from tests import helpers as Hh

MODELS = ["code2_lp_gated_h64", "code2_lp_attn_h32_bidir"]


def lp_model(meta):
    """The fixture's model: the LP script's constructor arguments, `ASTNodeEncoder2`, seeded weights."""
    H = meta["H"]
    enc = ASTNodeEncoder2(H, 98, meta["n_attr"], 20)
    model = dagnn_amd.DAGNN(num_vocab=None, max_seq_len=None, emb_dim=H, hidden_dim=H, out_dim=None, encoder=enc, **meta["ctor"]).eval()
    seeded_fill(model, meta["w_seed"])
    return model


def row_lse_loss64(logits, targ):
    """The float64 oracle of the class loss: per row log-sum-exp minus the target's logit, mean over the rows."""
    x = np.asarray(logits, dtype=np.float64)
    t = np.asarray(targ).astype(np.int64)
    m = x.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(x - m).sum(axis=1))
    return float(np.mean(lse - x[np.arange(x.shape[0]), t]))


def test_public_names():
    for name in ("ASTNodeEncoder2", "lp", "lp_targets", "class_cross_entropy", "ClassAccuracy", "lp_batches", "evaluate_lp"):
        assert hasattr(dagnn_amd, name), name
    assert set(lp.__all__) >= {"graph_depth_host", "class_hits_host"}


@pytest.mark.parametrize("name", MODELS)
def test_encoder2_loads_reference_names_and_matches_the_fixture(name):
    meta, arr = Hh.load(name)
    model = lp_model(meta)
    enc = model.encoder
    assert sorted(enc.state_dict()) == ["attribute_encoder.weight", "type_encoder.weight"]
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == meta["state_dict"]
    fresh = ASTNodeEncoder2(meta["H"], 98, meta["n_attr"], 20)
    fresh.load_state_dict({k: v.clone() for k, v in enc.state_dict().items()}, strict=True)
    depth = torch.from_numpy(arr["node_depth"].copy())
    with torch.no_grad():
        out = fresh(torch.from_numpy(arr["x"]), depth)
    assert np.array_equal(depth.numpy(), arr["node_depth_after"])       # clamped in place (utils2.py:27)
    assert np.array_equal(out.numpy()[arr["rows"]], arr["x_emb"])       # one fp32 add: bit for bit


def test_encoder2_clamps_depth_in_place():
    enc = ASTNodeEncoder2(8, 5, 7, 3)
    depth = torch.tensor([0, 3, 4, 99])
    out = enc(torch.tensor([[0, 1], [4, 6], [2, 2], [1, 0]]), depth)
    assert depth.tolist() == [0, 3, 3, 3] and tuple(out.shape) == (4, 8)


@pytest.mark.parametrize("name", MODELS)
def test_graph_depth_host_is_len_longest_path(name):
    meta, arr = Hh.load(name)
    got = lp.graph_depth_host(arr["layer0"], arr["batch"], meta["B"])
    assert got.dtype == np.int64 and np.array_equal(got, arr["len_longest_path"].astype(np.int64))
    assert np.array_equal(lp.graph_depth_host(arr["layer0"], arr["batch"]), got)
    assert lp.graph_depth_host(arr["layer0"], arr["batch"], meta["B"] + 2).tolist() == got.tolist() + [0, 0]
    G = Hh.code2_batch(arr)
    t = lp.lp_targets(G)
    assert t.dtype == torch.int64 and np.array_equal(t.numpy(), got)


def test_lp_targets_prefers_the_attribute():
    meta, arr = Hh.load(MODELS[0])
    G = Hh.code2_batch(arr)
    G.len_longest_path = torch.arange(meta["B"], dtype=torch.float32) + 0.75   # (cast as the reference casts: toward zero)
    t = lp.lp_targets(G)
    assert t.dtype == torch.int64 and t.tolist() == list(range(meta["B"]))


def test_accuracy_is_the_evaluators_number_exactly():
    meta, arr = Hh.load("code2_lp_acc")
    tok, targ = torch.from_numpy(arr["tok"]), torch.from_numpy(arr["targ"])
    metric, o = ClassAccuracy(), 0
    for i, n in enumerate(meta["splits"]):
        t = tok[o:o + n].view(-1, 1) if i % 2 else tok[o:o + n]
        metric.update(t, targ[o:o + n])
        o += n
    counts = metric.counts()
    assert counts.shape == (len(meta["splits"]), 2) and counts[3, 0] == 0 and counts[3, 1] > 0   # the batch without a hit
    res = metric.compute()
    assert res["n"] == meta["labelled"] and int(counts[:, 0].sum()) == meta["hits"]
    assert res["acc"] == float(arr["acc"])
    metric.reset()
    with pytest.raises(ValueError):
        metric.compute()
    metric.update(torch.tensor([1, 2]), torch.tensor([float("nan"), float("nan")]))
    with pytest.raises(ValueError):
        metric.compute()


def test_class_hits_host_rules():
    nan = float("nan")
    logits = np.array([[1.0, 3.0, 3.0, 0.0],     # a tie: the lowest column
                       [0.0, nan, 9.0, nan],     # a NaN beats every number, the first one wins
                       [-0.0, 0.0, -1.0, -2.0],  # -0 == +0: column 0
                       [5.0, 1.0, 1.0, 1.0],
                       [0.0, 0.0, 0.0, 7.0]], dtype=np.float32)
    assert lp.class_hits_host(logits, np.array([1.0, 1.0, 0.0, nan, 3.5])).tolist() == [3, 4]
    assert lp.class_hits_host(logits, np.array([2, 3, 1, 0, 3])).tolist() == [2, 5]
    assert lp.class_hits_host(np.array([[1], [3]]), np.array([1.0, 3.5], dtype=np.float32)).tolist() == [1, 2]
    assert lp.class_hits_host(torch.from_numpy(logits), torch.tensor([1, 1, 0, 0, 3])).tolist() == [5, 5]


def test_lp_batches_drops_what_the_reference_drops():
    def mk(n, graphs):
        return SimpleNamespace(x=torch.zeros(n, 2, dtype=torch.int64), num_graphs=graphs,
                               batch=torch.arange(graphs).repeat_interleave(max(n // graphs, 1))[:n])
    batches = [mk(1, 1), mk(7, 1), mk(9, 3), mk(2, 2), mk(1, 1), mk(30, 1)]
    # main_pyg_lp.py:51 and :84, verbatim in effect
    ref_train = [b for b in batches if not b.x.shape[0] == 1 and not b.batch[-1] == 0]
    ref_eval = [b for b in batches if not b.x.shape[0] == 1]
    assert [id(b) for b in lp.lp_batches(batches, training=True)] == [id(b) for b in ref_train]
    assert [id(b) for b in lp.lp_batches(batches, training=False)] == [id(b) for b in ref_eval]
    assert len(ref_train) == 2 and len(ref_eval) == 4


@pytest.mark.parametrize("name", MODELS)
def test_float64_loss_oracle_matches_the_reference_loss(name):
    meta, arr = Hh.load(name)
    assert abs(row_lse_loss64(arr["pred"], arr["len_longest_path"]) - float(arr["loss"])) < 1e-6
    # ... and the CPU route of `class_cross_entropy` is the reference's expression
    loss = lp.class_cross_entropy(torch.from_numpy(arr["pred"]), torch.from_numpy(arr["len_longest_path"]))
    assert abs(float(loss) - float(arr["loss"])) < 1e-6
    assert lp.class_hits_host(arr["pred"], arr["len_longest_path"]).tolist() == [round(float(arr["acc"]) * meta["B"]), meta["B"]]
