"""The ogbg-code2 evaluation path on the GPU (-m gpu): `DAGNN.predict` against token matrices made by the reference's own
`argmax` + `cat`, the tie / NaN rules of the two argmax kernels exactly, `dagnn_heads_argmax` against float64 at free shapes,
the F1 counts and the accumulator against the reference evaluator's numbers, and the contract of `predict` / `evaluate`.

The margin rule: the project's parity bound on logits is 1e-4, so two logits that each move by it can swap if they are within
TAU = 2e-4.  Where the reference's (or float64's) best two logits are further apart the token must be equal; elsewhere it must
be one of those two columns."""
import copy
import json
import warnings

import numpy as np
import pytest
import torch

from dagnn_amd import SeqF1, engine, evaluate, synth
from tests import helpers as Hh

pytestmark = pytest.mark.gpu
TAU = 2e-4
TOL = 1e-4


@pytest.fixture(params=["dataflow", "lockstep", "pergraph"])
def schedule(request, monkeypatch):
    """The three HIP schedules of the recurrence, as the golden parity tests parametrise them."""
    monkeypatch.setenv("DAGNN_AMD_SCHEDULE", "pergraph" if request.param == "pergraph" else "lockstep")
    monkeypatch.setattr(engine, "DATAFLOW", 1 if request.param == "dataflow" else 0)
    return request.param


def _sync_count(fn):
    """Synchronisations torch reports while fn runs (blocking copies and reads of device values)."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, sum("synchroniz" in str(x.message) for x in w)


def eval_model(name, device):
    """The fixture's model: seeded weights, then the stored bias boosts (EOS column of every head, `__UNK__` column of head 0)."""
    meta, arr = Hh.load(name)
    model = Hh.code2_model(meta)
    if meta["heads"] > 1:
        V = meta["V"]
        with torch.no_grad():
            for s, hd in enumerate(model.graph_pred_linear_list):
                hd.bias[V - 1] += torch.tensor(arr["boost_eos"][s])
            model.graph_pred_linear_list[0].bias[V - 2] += torch.tensor(arr["boost_unk"][0])
    return meta, arr, model.to(device)


def check_against_reference(arr, tok, top):
    tok, top = tok.cpu().numpy(), top.cpu().numpy()
    top_val, top_col = arr["top_val"], arr["top_col"]
    assert tok.shape == arr["tok"].shape and tok.dtype == np.int64
    clear = top_val[:, :, 0] - top_val[:, :, 1] > TAU
    wrong = int((tok[clear] != arr["tok"][clear]).sum())
    stray = int(((tok != top_col[:, :, 0]) & (tok != top_col[:, :, 1]))[~clear].sum())
    err = float(np.abs(top - top_val[:, :, :2]).max())
    print("entries %d, ambiguous %d, wrong %d, stray %d, max |top - reference| %.3e" % (tok.size, int((~clear).sum()), wrong, stray, err))
    assert wrong == 0 and stray == 0
    assert err < TOL


# ----------------------------------------------------------------------------- predict against the reference's tokens
@pytest.mark.parametrize("name", ["code2_eval_b64_h64", "code2_eval_b128_h128", "code2_eval_unidir_wx", "code2_eval_numclass"])
def test_predict_matches_the_reference_tokens(device, name, schedule):
    meta, arr, model = eval_model(name, device)
    tok, top = model.predict(Hh.code2_batch(arr, device), return_top=True)
    assert tuple(tok.shape) == (meta["B"], meta["heads"]) and tuple(top.shape) == (meta["B"], meta["heads"], 2)
    check_against_reference(arr, tok, top)


def test_predict_matches_the_reference_tokens_on_a_variant_model(device):
    meta, arr, model = eval_model("code2_eval_gated_sum", device)
    assert not model._hip_supported()   # the constructor-string variants' path (variants.run_hip)
    tok, top = model.predict(Hh.code2_batch(arr, device), return_top=True)
    check_against_reference(arr, tok, top)


# ----------------------------------------------------------------------------- tie and NaN rules, exactly
def _exact_case(D, seed):
    """Small-integer operands (every product and partial sum exact in fp32 in any order) with planted equal maxima: inside one
    tile (head 0), across two tiles of which one is the partial last one (head 1), in column 0 and column V - 1 (head 2), both
    inside the partial last tile (head 3)."""
    S, V, B = 4, 300, 5
    g = torch.Generator().manual_seed(seed)
    out = torch.randint(-2, 3, (B, D), generator=g).float()
    w = torch.randint(-2, 3, (S * V, D), generator=g).float()
    b = torch.randint(-3, 4, (S * V,), generator=g).float()
    pairs = [(5, 9), (130, 270), (0, V - 1), (290, 295)]
    for s, (c0, c1) in enumerate(pairs):
        w[s * V + c1] = w[s * V + c0]
        b[s * V + c0] = b[s * V + c1] = 1000.0
    return S, V, out, w, b, pairs


@pytest.mark.parametrize("D", [8, 32, 6])   # float4 tiles / the 32-wide stage / scalar loads
def test_heads_argmax_ties_go_to_the_lowest_column(device, D):
    S, V, out, w, b, pairs = _exact_case(D, 11 + D)
    tok, top = engine.heads_argmax(out.to(device), w.to(device), b.to(device), S, V)
    logits = (out.double() @ w.double().t() + b.double()).view(-1, S, V)
    srt = logits.sort(dim=2, descending=True).values
    assert tok.cpu().tolist() == [[c0 for c0, _ in pairs]] * out.shape[0]
    assert torch.equal(tok.cpu(), logits.argmax(dim=2))
    assert torch.equal(top.cpu().double(), srt[:, :, :2])               # bit-equal: the values are exact in fp32
    assert torch.equal(top[:, :, 0], top[:, :, 1])                       # a tie's runner-up is the winner's value


def test_heads_argmax_nan_beats_everything_and_the_first_nan_wins(device):
    S, V, out, w, b, pairs = _exact_case(8, 5)
    b[0 * V + 200] = float("nan")                                        # one NaN
    b[1 * V + 100] = b[1 * V + 50] = float("nan")                        # two: the first wins
    b[3 * V + V - 1] = float("nan")                                      # the last live column of the partial tile
    tok, top = engine.heads_argmax(out.to(device), w.to(device), b.to(device), S, V)
    tok, top = tok.cpu(), top.cpu()
    assert tok[:, 0].tolist() == [200] * 5 and tok[:, 1].tolist() == [50] * 5 and tok[:, 3].tolist() == [V - 1] * 5
    assert tok[:, 2].tolist() == [0] * 5
    assert torch.isnan(top[:, [0, 1, 3], 0]).all() and torch.isnan(top[:, 1, 1]).all()
    assert top[:, 0, 1].tolist() == [1000.0 + float(out[i] @ w[5]) for i in range(5)]
    lg = torch.addmm(b, out, w.t())                                      # what torch.argmax decides on the CPU
    assert torch.equal(tok, torch.stack([lg[:, s * V:(s + 1) * V].argmax(dim=1) for s in range(S)], dim=1))


@pytest.mark.parametrize("B,S,V,pad", [(7, 5, 5002, 0), (9, 3, 17, 5), (4, 1, 50, 2), (130, 2, 301, 3), (1, 5, 48, 0)])
def test_rows_argmax_equals_torch_argmax_on_the_cpu(device, B, S, V, pad):
    g = torch.Generator().manual_seed(B * 1000 + V)
    wide = torch.randn(B, S * V + pad, generator=g)
    for k in range(3 * B * S):    # planted ties, NaNs and infinities
        r, s = int(torch.randint(0, B, (1,), generator=g)), int(torch.randint(0, S, (1,), generator=g))
        c = torch.randint(0, V, (3,), generator=g)
        val = [9.0, float("nan"), float("inf"), -0.0][k % 4]
        wide[r, s * V + c[:2 if k % 4 != 1 else 3]] = val
    wide[0, :V] = 0.0
    wide[0, 3] = -0.0                                                     # -0 == +0: column 0
    logits = wide.to(device)[:, :S * V]                                   # strided rows when pad > 0
    want = torch.stack([wide[:, s * V:(s + 1) * V].argmax(dim=1) for s in range(S)], dim=1)
    assert torch.equal(engine.rows_argmax(logits, S, V).cpu(), want)
    if pad == 0:   # S views of one [B, S V] tensor, as `forward` returns them: the one-launch path
        assert torch.equal(evaluate.rows_argmax(list(logits.split(V, dim=1))).cpu(), want)


# ----------------------------------------------------------------------------- shapes, against float64
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("V", [17, 48, 5002])
@pytest.mark.parametrize("D", [64, 300, 1024])
def test_heads_argmax_shapes_against_float64(device, D, V, S):
    g = torch.Generator(device=device).manual_seed(D * 7 + V + S)
    a = 1.0 / D ** 0.5   # nn.Linear's own initial range; pooled GRU states lie in (-1, 1)
    w = (torch.rand(S * V, D, generator=g, device=device) * 2 - 1) * a
    b = (torch.rand(S * V, generator=g, device=device) * 2 - 1) * a
    for B in (0, 1, 3, 128, 257):
        out = torch.rand(B, D, generator=g, device=device) * 2 - 1
        tok, top = engine.heads_argmax(out, w, b, S, V)
        assert tuple(tok.shape) == (B, S) and tuple(top.shape) == (B, S, 2) and tok.dtype == torch.int64
        if B == 0:
            continue
        ref = (out.double() @ w.double().t() + b.double()).view(B, S, V)
        val, col = ref.topk(2, dim=2)
        clear = val[:, :, 0] - val[:, :, 1] > TAU
        assert torch.equal(tok[clear], col[:, :, 0][clear])
        assert bool(((tok == col[:, :, 0]) | (tok == col[:, :, 1])).all())
        assert float((top.double() - val).abs().max()) < TOL
        assert bool((ref.gather(2, tok.unsqueeze(2)).squeeze(2) >= val[:, :, 0] - TAU).all())


def test_heads_argmax_reads_strided_rows_and_odd_widths(device):
    """`out` and the heads as views with a row pitch (16-byte aligned and not), D % 4 != 0 (`out_wx` read-outs)."""
    g = torch.Generator(device=device).manual_seed(9)
    for D, pitch in ((70, 72), (70, 71), (96, 100), (37, 37)):
        S, V, B = 2, 150, 33
        out = (torch.rand(B, pitch, generator=g, device=device) * 2 - 1)[:, :D]
        w = ((torch.rand(S * V, pitch, generator=g, device=device) * 2 - 1) / D ** 0.5)[:, :D]
        b = torch.rand(S * V, generator=g, device=device)
        lib = engine._lib.load()
        tok = torch.empty(B, S, dtype=torch.int64, device=device)
        top = torch.empty(B, S, 2, dtype=torch.float32, device=device)
        work = torch.empty(lib.dagnn_heads_argmax_bytes(B, S, V) // 8, dtype=torch.int64, device=device)
        engine.check(lib.dagnn_heads_argmax(out.data_ptr(), pitch, w.data_ptr(), pitch, b.data_ptr(), B, D, S, V, tok.data_ptr(),
                                            top.data_ptr(), work.data_ptr(), work.numel() * 8, engine._stream(out)), "heads_argmax")
        ref = (out.double() @ w.double().t() + b.double()).view(B, S, V)
        val, col = ref.topk(2, dim=2)
        clear = val[:, :, 0] - val[:, :, 1] > TAU
        assert torch.equal(tok[clear], col[:, :, 0][clear]) and float((top.double() - val).abs().max()) < TOL


# ----------------------------------------------------------------------------- counts and F1
def _f1_fixture(name):
    meta, arr = Hh.load(name)
    words = {k: json.loads(bytes(arr[k]).decode()) for k in ("idx2vocab", "seq_ref", "seq_pred")}
    return meta, arr, words, {w: i for i, w in enumerate(words["idx2vocab"])}


@pytest.mark.parametrize("name", ["code2_f1_b1", "code2_f1_b3000"])
def test_counts_kernel_and_accumulator_match_the_reference_evaluator(device, name):
    meta, arr, words, vocab2idx = _f1_fixture(name)
    tok = torch.from_numpy(arr["tok"]).to(device)
    ref_ids, ref_extra = evaluate.encode_ref_sets(words["seq_ref"], vocab2idx)
    counts = engine.seq_f1_counts(tok, meta["eos"], ref_ids.to(device), ref_extra.to(device))
    np.testing.assert_array_equal(counts.cpu().numpy(), evaluate.f1_counts_host(arr["tok"], meta["eos"], ref_ids, ref_extra))
    assert evaluate.tokens_to_seqs(tok, words["idx2vocab"]) == words["seq_pred"]
    for splits in ([meta["B"]], meta["splits"]):
        metric, o = SeqF1(meta["eos"]), 0
        for n in splits:
            ids, extra = evaluate.encode_ref_sets(words["seq_ref"][o:o + n], vocab2idx)
            metric.update(tok[o:o + n], ids, extra)
            o += n
        res, syncs = _sync_count(metric.compute)
        assert syncs == 1 and res["n"] == meta["B"]
        assert [res["precision"], res["recall"], res["F1"]] == arr["f1"].tolist()   # exactly: integers in, the evaluator's float64 steps


def test_counts_kernel_on_predicted_tokens(device):
    meta, arr, model = eval_model("code2_eval_b64_h64", device)
    tok = model.predict(Hh.code2_batch(arr, device))
    V, B = meta["V"], meta["B"]
    rng = np.random.default_rng(4)
    host = tok.cpu().numpy()
    ref_ids = rng.integers(-1, V, size=(B, 7)).astype(np.int32)
    ref_ids[:, 0] = host[:, 0]                       # some true positives
    ref_ids[::3, 1] = host[::3, 2]
    ref_ids[::5, 3] = ref_ids[::5, 0]                # repeated label ids count once
    ref_extra = rng.integers(0, 3, size=B).astype(np.int32)
    counts = engine.seq_f1_counts(tok, V - 1, torch.from_numpy(ref_ids).to(device), torch.from_numpy(ref_extra).to(device))
    want = evaluate.f1_counts_host(host, V - 1, ref_ids, ref_extra)
    np.testing.assert_array_equal(counts.cpu().numpy(), want)
    assert want[:, 0].sum() > 0 and (want[:, 3] < meta["S"]).any() and (want[:, 3] == meta["S"]).any()


# ----------------------------------------------------------------------------- contract
def _labelled_batches(device, V, sizes=(12, 5, 20)):
    vocab2idx = {"w%d" % i: i for i in range(V - 2)}
    vocab2idx["__UNK__"], vocab2idx["__EOS__"] = V - 2, V - 1
    rng = np.random.default_rng(2)
    batches = []
    for k, B in enumerate(sizes):
        b = synth.code2_batch(seed=40 + k, num_graphs=B, mean_n=30)
        b.x[:, 1] %= 300
        b = b.to(device)
        b.y = [["w%d" % int(i) for i in rng.integers(0, V + 50, size=int(rng.integers(0, 7)))] for _ in range(B)]
        batches.append(b)
    return vocab2idx, batches


def test_predict_leaves_forwards_side_effects_and_is_repeatable(device):
    meta, arr, model = eval_model("code2_eval_b64_h64", device)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    G0, G1, G2 = (Hh.code2_batch(arr, device) for _ in range(3))
    with torch.no_grad():
        pred = model(G0)
    tok, top = model.predict(G1, return_top=True)
    tok2, top2 = model.predict(G2, return_top=True)
    assert torch.equal(tok, tok2) and torch.equal(top, top2)             # bitwise repeatable
    for G in (G1, G2):
        assert torch.equal(G.x, G0.x) and torch.equal(G.node_depth, G0.node_depth) and torch.equal(G.batch, G0.batch)
        assert torch.equal(G.bi_layer_index, G0.bi_layer_index)
        assert len(G.h) == len(G0.h) and all(torch.equal(a, b) for ha, hb in zip(G.h, G0.h) for a, b in zip(ha, hb))
    # against the module's own logits: equal wherever they are not within TAU of each other
    val, col = torch.stack(pred, dim=1).topk(2, dim=2)
    clear = val[:, :, 0] - val[:, :, 1] > TAU
    assert torch.equal(tok[clear], col[:, :, 0][clear]) and float((top - val).abs().max()) < TOL
    assert torch.equal(evaluate.rows_argmax(pred), torch.cat([torch.argmax(p, dim=1).view(-1, 1) for p in pred], dim=1))
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    model.check()
    model.train()
    with pytest.raises(RuntimeError, match="evaluation pass"):
        model.predict(Hh.code2_batch(arr, device))


def test_evaluate_adds_one_synchronisation_to_its_passes(device):
    meta, arr, model = eval_model("code2_eval_b64_h64", device)
    vocab2idx, batches = _labelled_batches(device, meta["V"])
    fresh = lambda: [copy.deepcopy(b) for b in batches]   # noqa: E731  (a pass replaces G.x: every run gets its own copies)
    evaluate.evaluate(model, fresh(), vocab2idx)          # warm-up: caches, arenas, pinned pools
    bs = fresh()
    toks, base = _sync_count(lambda: [model.predict(b) for b in bs])
    bs = fresh()
    res, syncs = _sync_count(lambda: evaluate.evaluate(model, bs, vocab2idx))
    assert syncs == base + 1, (syncs, base)
    assert res["n"] == sum(b.num_graphs for b in batches) and not model.training
    # the same numbers from the words: the evaluator's definition on the decoded predictions
    idx2vocab = sorted(vocab2idx, key=vocab2idx.get)
    seq_pred = [s for t in toks for s in evaluate.tokens_to_seqs(t, idx2vocab)]
    seq_ref = [y for b in batches for y in b.y]
    p, r, f = [], [], []
    for l, q in zip(seq_ref, seq_pred):
        label, prediction = set(l), set(q)
        tp, fp, fn = len(label & prediction), len(prediction - label), len(label - prediction)
        p.append(tp / (tp + fp) if tp + fp > 0 else 0)
        r.append(tp / (tp + fn) if tp + fn > 0 else 0)
        f.append(2 * p[-1] * r[-1] / (p[-1] + r[-1]) if p[-1] + r[-1] > 0 else 0)
    assert [res["precision"], res["recall"], res["F1"]] == [np.average(p), np.average(r), np.average(f)]
