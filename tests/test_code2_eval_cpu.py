"""The ogbg-code2 evaluation path, host tier: the metric's host functions against fixtures made by the reference's own
`get_vocab_mapping`, `decode_arr_to_seq` and `Evaluator._eval_F1` (tests/golden/make_golden_code2_eval.py), the ambiguity cap of
the model fixtures, and the argument checks of the three C entry points that need no device."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from dagnn_amd import SeqF1, _lib, evaluate
from tests import helpers as Hh

F1_FIXTURES = ["code2_f1_b1", "code2_f1_b3000"]
EVAL_FIXTURES = ["code2_eval_b64_h64", "code2_eval_b128_h128", "code2_eval_unidir_wx", "code2_eval_numclass",
                 "code2_eval_gated_sum"]
TAU = 2e-4   # two logits that each move by the project's parity bound (1e-4) can swap if they are within 2e-4


def f1_fixture(name):
    meta, arr = Hh.load(name)
    words = {k: json.loads(bytes(arr[k]).decode()) for k in ("idx2vocab", "seq_ref", "seq_pred")}
    vocab2idx = {w: i for i, w in enumerate(words["idx2vocab"])}
    return meta, arr, words, vocab2idx


def test_encode_ref_sets_by_hand():
    vocab2idx = {"a": 0, "b": 1, "c": 2, "__UNK__": 3, "__EOS__": 4}
    ref_ids, ref_extra = evaluate.encode_ref_sets([["b", "a", "b", "zz"], [], ["zz", "yy", "zz"], ["__UNK__", "c", "__EOS__"]],
                                                  vocab2idx)
    assert ref_ids.dtype == torch.int32 and ref_extra.dtype == torch.int32
    assert ref_ids.tolist() == [[1, 0, -1], [-1, -1, -1], [-1, -1, -1], [3, 2, 4]]
    assert ref_extra.tolist() == [1, 0, 2, 0]
    ref_ids, ref_extra = evaluate.encode_ref_sets([[], []], vocab2idx)   # R is at least 1
    assert tuple(ref_ids.shape) == (2, 1) and ref_ids.tolist() == [[-1], [-1]] and ref_extra.tolist() == [0, 0]


@pytest.mark.parametrize("name", F1_FIXTURES)
def test_host_metric_matches_the_reference_evaluator(name):
    meta, arr, words, vocab2idx = f1_fixture(name)
    tok = torch.from_numpy(arr["tok"])
    assert evaluate.tokens_to_seqs(tok, words["idx2vocab"]) == words["seq_pred"]
    ref_ids, ref_extra = evaluate.encode_ref_sets(words["seq_ref"], vocab2idx)
    counts = evaluate.f1_counts_host(tok, meta["eos"], ref_ids, ref_extra)
    assert counts.dtype == np.int32 and counts.shape == (meta["B"], 4)
    tp, fp, fn = arr["tpfpfn"].T
    np.testing.assert_array_equal(counts[:, 0], tp)
    np.testing.assert_array_equal(counts[:, 1] - counts[:, 0], fp)
    np.testing.assert_array_equal(counts[:, 2] - counts[:, 0], fn)
    np.testing.assert_array_equal(counts[:, 3], [len(p) for p in words["seq_pred"]])
    # the accumulator, fed in one piece and in the fixture's uneven pieces: the evaluator's three numbers, exactly
    for splits in ([meta["B"]], meta["splits"]):
        metric, o = SeqF1(meta["eos"]), 0
        for n in splits:
            ids, extra = evaluate.encode_ref_sets(words["seq_ref"][o:o + n], vocab2idx)
            metric.update(tok[o:o + n], ids, extra)
            o += n
        res = metric.compute()
        assert res["n"] == meta["B"]
        assert [res["precision"], res["recall"], res["F1"]] == arr["f1"].tolist()
        metric.reset()
        assert metric.counts().shape == (0, 4)


def test_f1_fixture_covers_the_branches():
    meta, arr, words, vocab2idx = f1_fixture("code2_f1_b3000")
    tok, eos, S = arr["tok"], meta["eos"], meta["S"]
    first = np.where((tok == eos).any(1), (tok == eos).argmax(1), S)
    assert set(first.tolist()) == set(range(S + 1))                        # EOS at every position, and absent
    assert (tok == meta["unk"]).any() and any(len(set(r)) < len(r) for r in tok.tolist())
    refs = words["seq_ref"]
    assert any(len(r) == 0 for r in refs) and any(len(r) > S for r in refs) and any(len(set(r)) < len(r) for r in refs)
    assert any(w not in vocab2idx for r in refs for w in r)
    assert any("__UNK__" in r for r in refs) and any("__EOS__" in r for r in refs)
    assert len(set(meta["splits"])) > 3 and sum(meta["splits"]) == meta["B"]


@pytest.mark.parametrize("name", EVAL_FIXTURES)
def test_model_fixture_ambiguity_cap(name):
    """An entry (graph, head) is ambiguous when the reference's two best logits are within TAU.  At most 2 % of a fixture may
    be, and the third logit lies more than TAU below the first everywhere: then a result within the parity bound of the
    reference's logits can only ever pick the reference's first or second column."""
    meta, arr = Hh.load(name)
    top_val, top_col, tok = arr["top_val"], arr["top_col"], arr["tok"]
    assert top_val.shape == (meta["B"], meta["heads"], 3) and tok.shape == (meta["B"], meta["heads"])
    assert meta["tau"] == TAU
    margin = top_val[:, :, 0] - top_val[:, :, 1]
    assert (margin >= 0).all() and (top_val[:, :, 1] >= top_val[:, :, 2]).all()
    assert float((margin <= TAU).mean()) <= 0.02
    assert float((top_val[:, :, 0] - top_val[:, :, 2]).min()) > TAU
    clear = margin > 0
    np.testing.assert_array_equal(tok[clear], top_col[:, :, 0][clear])
    if meta["heads"] > 1:
        share = float((tok == meta["V"] - 1).mean())
        assert 0.10 <= share <= 0.60 and (tok[:, 0] == meta["V"] - 2).any()


# ----------------------------------------------------------------------------- the C entry points' argument checks
def test_entry_points_refuse_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    EINVAL, ENOSPC = -22, -28
    nbytes = lib.dagnn_heads_argmax_bytes
    assert nbytes(128, 5, 5002) == 128 * 5 * 40 * 16 and nbytes(1, 1, 1) == 16 and nbytes(0, 5, 48) > 0
    assert nbytes(-1, 5, 48) == 0 and nbytes(4, 0, 48) == 0 and nbytes(4, 5, 0) == 0 and nbytes(4, 1 << 16, 1 << 16) == 0
    p = C.c_void_p(4096)   # a non-null, 16-byte aligned address nothing dereferences: every call below returns before a launch
    h = lib.dagnn_heads_argmax
    assert h(p, 64, p, 64, p, 0, 64, 5, 48, p, p, p, 1 << 20, None) == 0                  # B = 0 returns at once
    assert h(None, 64, None, 64, None, 0, 64, 5, 48, None, None, None, 0, None) == 0
    assert h(None, 64, p, 64, p, 4, 64, 5, 48, p, p, p, 1 << 20, None) == EINVAL          # null pointers
    assert h(p, 64, None, 64, p, 4, 64, 5, 48, p, p, p, 1 << 20, None) == EINVAL
    assert h(p, 64, p, 64, None, 4, 64, 5, 48, p, p, p, 1 << 20, None) == EINVAL
    assert h(p, 64, p, 64, p, 4, 64, 5, 48, None, p, p, 1 << 20, None) == EINVAL
    assert h(p, 64, p, 64, p, 4, 64, 5, 48, p, p, None, 1 << 20, None) == EINVAL
    assert h(p, 64, p, 64, p, 4, 64, 5, 48, p, p, C.c_void_p(4100), 1 << 20, None) == EINVAL   # misaligned scratch
    assert h(p, 63, p, 64, p, 4, 64, 5, 48, p, p, p, 1 << 20, None) == EINVAL             # row pitch below D
    assert h(p, 64, p, 60, p, 4, 64, 5, 48, p, p, p, 1 << 20, None) == EINVAL
    assert h(p, 64, p, 64, p, 4, 0, 5, 48, p, p, p, 1 << 20, None) == EINVAL
    assert h(p, 64, p, 64, p, -1, 64, 5, 48, p, p, p, 1 << 20, None) == EINVAL
    assert h(p, 64, p, 64, p, 4, 64, 0, 48, p, p, p, 1 << 20, None) == EINVAL
    assert h(p, 64, p, 64, p, 4, 64, 5, 0, p, p, p, 1 << 20, None) == EINVAL
    assert h(p, 64, p, 64, p, 4, 64, 5, 48, p, p, p, nbytes(4, 5, 48) - 1, None) == ENOSPC
    r = lib.dagnn_rows_argmax
    assert r(p, 240, 0, 5, 48, p, None) == 0
    assert r(None, 240, 4, 5, 48, p, None) == EINVAL and r(p, 240, 4, 5, 48, None, None) == EINVAL
    assert r(p, 239, 4, 5, 48, p, None) == EINVAL and r(p, 240, -1, 5, 48, p, None) == EINVAL
    assert r(p, 240, 4, 0, 48, p, None) == EINVAL and r(p, 240, 4, 5, 0, p, None) == EINVAL
    assert r(C.c_void_p(4098), 240, 4, 5, 48, p, None) == EINVAL
    f = lib.dagnn_seq_f1_counts
    assert f(p, 0, 5, 51, p, 3, p, p, None) == 0
    assert f(None, 4, 5, 51, p, 3, p, p, None) == EINVAL and f(p, 4, 5, 51, None, 3, p, p, None) == EINVAL
    assert f(p, 4, 5, 51, p, 3, p, None, None) == EINVAL and f(p, 4, 5, 51, p, 3, p, C.c_void_p(4100), None) == EINVAL
    assert f(p, 4, 0, 51, p, 3, p, p, None) == EINVAL and f(p, 4, 5, 51, p, 0, p, p, None) == EINVAL
    assert f(p, -1, 5, 51, p, 3, p, p, None) == EINVAL


def test_predict_raises_in_training_mode_and_rows_argmax_loops_on_the_host():
    meta, _ = Hh.load("code2_eval_numclass")
    model = Hh.code2_model(meta).train()
    with pytest.raises(RuntimeError, match="evaluation pass"):
        model.predict(object())
    g = torch.Generator().manual_seed(3)
    pred = [torch.randn(6, 11, generator=g) for _ in range(3)]
    pred[1][2, 4] = pred[1][2, 7] = 9.0   # a tie: the lowest column
    want = torch.cat([torch.argmax(p, dim=1).view(-1, 1) for p in pred], dim=1)
    assert torch.equal(evaluate.rows_argmax(pred), want) and int(want[2, 1]) == 4
    assert torch.equal(evaluate.rows_argmax(pred[0]), want[:, :1])
