"""The ogbg-code2 training epoch on the GPU (-m gpu): the two STEP instances of csrc/loss.hip's kernel against the entry points they
fuse - bit for bit, no tolerance -, the epoch accumulators, `GraphStore.train_tok` / `train_lp` against the loop written out on
the pieces, against the fixtures of the reference's own `train()` loop bodies (tests/golden/make_golden_code2_train.py),
and that nothing synchronises inside the loop.

Bounds.  Everything the kernels add is integer work or a float64 sum of float32 values in stream order: exact.  The loss
against the fixture: max(2e-4, 4 x loss_err_ref) around `loss64` - 2e-4 is twice the project's 1e-4 logit parity bound (a
cross-entropy moves by at most twice the largest logit error), 4 x the reference's own fp32 error is the convention of
DESIGN.md 4i.  Measured on an MI355X: |loss - loss64| <= 1.7e-7 (TOK) and 1.4e-7 (LP) over the three steps - 0.00085 and
0.00068 of the bound, which the 2e-4 term sets (4 x loss_err_ref is at most 1.5e-6) -, the mean loss 1.4e-7 / 2.7e-8."""

import numpy as np
import pytest
import torch

import dagnn_amd
from dagnn_amd import ASTNodeEncoder, ASTNodeEncoder2, EpochMeter, engine, lp, train
from dagnn_amd import _lib as L
from dagnn_amd.evaluate import SeqF1, f1_counts_host, rows_argmax
from dagnn_amd.train import ClipAdam, seq_ce_step, seq_cross_entropy
from oracle.seeding import seeded_fill
from tests.test_code2_train_cpu import LP, TOK, assert_fixture_batches, fixture_raw, special_rows

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENT = -7777777


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    """Bit for bit where the values are numbers (so -0 and +0 differ), NaN where NaN: a NaN's sign and payload are not part
    of any value (the two kernels' subtractions hand on different ones of a NaN logit)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(bits(a)[~na], bits(b)[~nb])


def _words(device):
    """A fresh zeroed (ticket, epoch_sum, epoch_steps, epoch_hits[2]) set."""
    return (torch.zeros(1, dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.float64, device=device),
            torch.zeros(1, dtype=torch.int64, device=device), torch.zeros(2, dtype=torch.int64, device=device))


# ============================================================================= 1. the TOK kernel against the entry points it fuses
def _seq_case(B, S, V, R, seed, finite=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * S, V, generator=g)
    cases = special_rows(x, V, finite)
    eos = V - 1
    x[0, eos] = 60.0                                   # EOS at position 0 of graph 0: an empty prediction
    if B > 1:
        x[S:2 * S, eos] = -60.0                        # ... and nowhere in graph 1
    y = torch.randint(0, V, (B, S), generator=g)
    ref_ids = torch.randint(-1, V, (B, R), generator=g).to(torch.int32)
    ref_extra = torch.randint(0, 3, (B,), generator=g).to(torch.int32)
    ref_ids[B - 1] = -1                                # a graph whose label words are all outside the vocabulary
    ref_extra[B - 1] = 2
    return x.view(B, S * V), y, eos, ref_ids, ref_extra, cases


@pytest.mark.parametrize("rows", ["special", "finite"])   # with the NaN / -inf rows (whose losses make the sum NaN), and without
@pytest.mark.parametrize("R", [1, 9])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B,S,V", [(1, 1, 1), (1, 5, 7), (3, 5, 255), (3, 5, 257), (5, 2, 5002), (65, 5, 300)])
def test_seq_step_kernel_is_bitwise_the_pieces(device, B, S, V, pad, R, rows):
    lib, st = L.load(), None
    x, y, eos, ref_ids, ref_extra, cases = _seq_case(B, S, V, R, 100 * B + V + R, finite=rows == "finite")
    ld = S * V + pad
    logits = torch.full((B, ld), NAN, device=device)
    logits[:, :S * V] = x.to(device)
    y, ref_ids, ref_extra = y.to(device), ref_ids.to(device), ref_extra.to(device)
    st = engine._stream(logits)
    ld_d = (S * V + 3) // 4 * 4
    off, cap = 3, B + 5
    # the fused launch
    dl = torch.full((B, ld_d), NAN, device=device)
    row, loss, tok = torch.empty(B * S, device=device), torch.empty(1, device=device), torch.full((B, S), SENT, dtype=torch.int64, device=device)
    counts = torch.full((cap, 4), SENT, dtype=torch.int32, device=device)
    ticket, esum, esteps, _ = _words(device)
    assert lib.dagnn_seq_ce_step(logits.data_ptr(), ld, y.data_ptr(), B, S, V, dl.data_ptr(), ld_d, row.data_ptr(), loss.data_ptr(),
                                 tok.data_ptr(), eos, ref_ids.data_ptr(), R, ref_extra.data_ptr(), counts.data_ptr(), cap, off,
                                 esum.data_ptr(), esteps.data_ptr(), ticket.data_ptr(), st) == 0
    # the pieces
    dl0 = torch.full((B, ld_d), NAN, device=device)
    row0, loss0, tok0 = torch.empty(B * S, device=device), torch.empty(1, device=device), torch.empty(B, S, dtype=torch.int64, device=device)
    counts0 = torch.empty(B, 4, dtype=torch.int32, device=device)
    t0 = torch.zeros(1, dtype=torch.int32, device=device)
    assert lib.dagnn_seq_ce(logits.data_ptr(), ld, y.data_ptr(), B, S, V, dl0.data_ptr(), ld_d, row0.data_ptr(), loss0.data_ptr(),
                            t0.data_ptr(), st) == 0
    assert lib.dagnn_rows_argmax(logits.data_ptr(), ld, B, S, V, tok0.data_ptr(), st) == 0
    assert lib.dagnn_seq_f1_counts(tok0.data_ptr(), B, S, eos, ref_ids.data_ptr(), R, ref_extra.data_ptr(), counts0.data_ptr(), st) == 0
    assert same(loss, loss0) and same(row, row0)
    assert same(dl, dl0)                                  # (the pitch's padding columns: both left NaN)
    assert torch.equal(tok, tok0)
    assert torch.equal(counts[off:off + B], counts0)
    assert bool((counts[:off] == SENT).all()) and bool((counts[off + B:] == SENT).all())
    assert int(ticket) == 0 and int(esteps) == 1
    if rows == "finite":
        assert np.isfinite(float(loss)) and float(esum) == float(loss)
    else:
        assert np.isnan(float(esum)) == np.isnan(float(loss))
    # ... and the definition
    host = train.seq_ce_step_host(x, y.cpu(), eos, ref_ids.cpu(), ref_extra.cpu())
    assert np.array_equal(tok.cpu().numpy(), host["tok"]) and np.array_equal(counts0.cpu().numpy(), host["counts"])
    flat = tok.view(-1).cpu()
    if "tie" in cases:
        assert int(flat[cases["tie"]]) == cases["tie_cols"][0]
    if "nan" in cases:
        assert int(flat[cases["nan"]]) == V // 2
    if "zeros" in cases:
        assert int(flat[cases["zeros"]]) == 1
    if V > 1:
        assert int(counts0[0, 3]) == 0 and (B == 1 or int(counts0[1, 3]) == S)   # EOS at position 0 / nowhere
    # without dlogits and without label sets: the same loss and tokens, the counts untouched
    tok2 = torch.empty_like(tok)
    counts.fill_(SENT)
    assert lib.dagnn_seq_ce_step(logits.data_ptr(), ld, y.data_ptr(), B, S, V, None, 0, row.data_ptr(), loss.data_ptr(),
                                 tok2.data_ptr(), eos, None, 1, None, None, 0, 0, esum.data_ptr(), esteps.data_ptr(),
                                 ticket.data_ptr(), st) == 0
    assert same(loss, loss0) and torch.equal(tok2, tok0) and bool((counts == SENT).all()) and int(esteps) == 2


def test_seq_step_tie_columns_sit_in_different_waves():
    x = torch.zeros(1, 300)
    cases = special_rows(x, 300)
    lo, hi = cases["tie_cols"]
    assert (lo % 256) // 64 != (hi % 256) // 64 and lo < hi


# ============================================================================= 2. the LP kernel
def _lp_targets(B, C, kind, g, finite):
    t = torch.randint(0, C, (B,), generator=g)
    if kind == "int64":
        return t
    t = t.to(torch.float32 if kind == "float32" else torch.float64)
    if B > 2:
        if not finite:
            t[1] = NAN                                 # unlabelled; its row loss, and the loss, NaN
        t[2] = t[2] + 0.5                              # truncated for the loss, matches no class
    if B > 4 and C > 1:
        t[4] = 3.5 if C > 3 else 0.5
    return t


@pytest.mark.parametrize("kind", ["float32", "int64", "float64"])
@pytest.mark.parametrize("B", [1, 65, 257])
@pytest.mark.parametrize("C", [1, 24, 275, 1030])
def test_class_step_kernel_is_bitwise_the_pieces(device, C, B, kind):
    lib = L.load()
    for pad, finite in ((3, True), (0, False)):        # without and with the rows / targets that make the loss NaN
        g = torch.Generator().manual_seed(C * 1000 + B)
        x = torch.randn(B, C, generator=g)
        special_rows(x, C, finite)
        targ = _lp_targets(B, C, kind, g, finite)
        hit = torch.nonzero(targ == targ).view(-1)[::2]    # every second labelled row: a sure hit
        for r in hit.tolist():
            if float(targ[r]) == int(targ[r]) and not torch.isnan(x[r]).any():
                x[r, int(targ[r])] = 70.0
        ld = C + pad
        logits = torch.full((B, ld), NAN, device=device)
        logits[:, :C] = x.to(device)
        t_dev = targ.to(device)
        k = engine._LP_KINDS[targ.dtype]
        st = engine._stream(logits)
        ld_d = (C + 3) // 4 * 4
        dl, dl0 = torch.full((B, ld_d), NAN, device=device), torch.full((B, ld_d), NAN, device=device)
        row, loss, tok = torch.empty(B, device=device), torch.empty(1, device=device), torch.full((B,), SENT, dtype=torch.int64, device=device)
        ticket, esum, esteps, ehits = _words(device)
        ehits += torch.tensor([5, 9], device=device)
        assert lib.dagnn_class_ce_step(logits.data_ptr(), ld, t_dev.data_ptr(), k, B, C, dl.data_ptr(), ld_d, row.data_ptr(),
                                       loss.data_ptr(), tok.data_ptr(), ehits.data_ptr(), esum.data_ptr(), esteps.data_ptr(),
                                       ticket.data_ptr(), st) == 0
        row0, loss0, tok0 = torch.empty(B, device=device), torch.empty(1, device=device), torch.empty(B, dtype=torch.int64, device=device)
        t0 = torch.zeros(1, dtype=torch.int32, device=device)
        assert lib.dagnn_class_ce(logits.data_ptr(), ld, t_dev.data_ptr(), k, B, C, dl0.data_ptr(), ld_d, row0.data_ptr(),
                                  loss0.data_ptr(), t0.data_ptr(), st) == 0
        assert lib.dagnn_rows_argmax(logits.data_ptr(), ld, B, 1, C, tok0.data_ptr(), st) == 0
        pair = engine.class_hits(logits[:, :C], t_dev)
        assert same(loss, loss0) and same(row, row0) and same(dl, dl0)
        assert torch.equal(tok, tok0)
        assert (ehits - torch.tensor([5, 9], device=device)).tolist() == pair.tolist() == lp.class_hits_host(x, targ).tolist()
        assert int(ticket) == 0 and int(esteps) == 1
        if finite:
            assert np.isfinite(float(loss)) and float(esum) == float(loss)
        else:
            assert np.isnan(float(esum)) == np.isnan(float(loss))
    if B > 2 and C > 1:                                # (the last variant: one NaN target among the float kinds)
        assert int(pair[0]) > 0 and int(pair[1]) == (B if kind == "int64" else B - 1)


@pytest.mark.parametrize("B,C", [(1, 1), (3, 255), (3, 257), (65, 300), (5, 5002)])
def test_class_ce_is_bitwise_seq_ce_with_one_head(device, B, C):
    """`dagnn_class_ce` with int64 targets and `dagnn_seq_ce` with S = 1 are two instances of one kernel around one row stage
    (csrc/loss.hip, csrc/rows_dev.h): on the same logits `loss`, `row_loss` and `dlogits` are the same bits, NaN where NaN.
    Rows from the back (`special_rows`): a two-way tie, a NaN, one finite value among -inf; with every target in range, then
    with the target of row 0 out of range."""
    lib = L.load()
    g = torch.Generator().manual_seed(7000 * B + C)
    x = torch.randn(B, C, generator=g)
    cases = special_rows(x, C)
    assert C < 2 or "tie" in cases and (B < 2 or "nan" in cases)
    ld, ld_d = C + 3, (C + 3) // 4 * 4
    logits = torch.full((B, ld), NAN, device=device)
    logits[:, :C] = x.to(device)
    st = engine._stream(logits)
    targ = torch.randint(0, C, (B,), generator=g)
    for out_of_range in (False, True):
        if out_of_range:
            targ[0] = C
        t_dev = targ.to(device)
        got = []
        for entry in ("class", "seq"):
            dl = torch.full((B, ld_d), NAN, device=device)
            row, loss = torch.full((B,), SENT, dtype=torch.float32, device=device), torch.full((1,), SENT, dtype=torch.float32, device=device)
            ticket = torch.zeros(1, dtype=torch.int32, device=device)
            if entry == "class":
                rc = lib.dagnn_class_ce(logits.data_ptr(), ld, t_dev.data_ptr(), L.LP_INT64, B, C, dl.data_ptr(), ld_d,
                                        row.data_ptr(), loss.data_ptr(), ticket.data_ptr(), st)
            else:
                rc = lib.dagnn_seq_ce(logits.data_ptr(), ld, t_dev.data_ptr(), B, 1, C, dl.data_ptr(), ld_d, row.data_ptr(),
                                      loss.data_ptr(), ticket.data_ptr(), st)
            assert rc == 0 and int(ticket) == 0
            got.append((loss, row, dl))
        (loss_c, row_c, dl_c), (loss_s, row_s, dl_s) = got
        assert same(loss_c, loss_s) and same(row_c, row_s) and same(dl_c, dl_s)   # (the pitch's padding columns: both left NaN)
        nan_rows = torch.isnan(row_c).nonzero().view(-1).tolist()
        want = sorted(({0} if out_of_range else set()) | ({cases["nan"]} if "nan" in cases else set()))
        assert nan_rows == want and bool(torch.isnan(loss_c)) == bool(want)
        assert torch.isnan(dl_c[:, :C]).any(dim=1).nonzero().view(-1).tolist() == ([cases["nan"]] if "nan" in cases else [])


# ============================================================================= 3. the accumulators
def test_epoch_accumulators_over_four_calls(device):
    B, S, V, R = 7, 3, 41, 4
    cap = 4 * B + 3

    def run():
        ticket, esum, esteps, _ = _words(device)
        counts = torch.full((cap, 4), SENT, dtype=torch.int32, device=device)
        keep = []
        for k in range(4):
            x, y, eos, ref_ids, ref_extra, _ = _seq_case(B, S, V, R, 50 + k, finite=True)
            x, y, ref_ids, ref_extra = x.to(device), y.to(device), ref_ids.to(device), ref_extra.to(device)
            row, loss, tok = torch.empty(B * S, device=device), torch.empty(1, device=device), torch.empty(B, S, dtype=torch.int64, device=device)
            assert L.load().dagnn_seq_ce_step(x.data_ptr(), S * V, y.data_ptr(), B, S, V, None, 0, row.data_ptr(), loss.data_ptr(),
                                              tok.data_ptr(), eos, ref_ids.data_ptr(), R, ref_extra.data_ptr(), counts.data_ptr(), cap,
                                              k * B, esum.data_ptr(), esteps.data_ptr(), ticket.data_ptr(), engine._stream(x)) == 0
            keep.append((loss, tok, ref_ids, ref_extra, x, y, row))
        # one read, after the four launches
        host = torch.cat([bits(esum).to(torch.int64), esteps, ticket.to(torch.int64), counts.view(-1).to(torch.int64)]).cpu()
        return host, keep

    host, keep = run()
    total = 0.0
    for loss, *_ in keep:
        total += float(loss)                                                      # `loss_accum += loss.item()`
    got_sum = host[:2].to(torch.int32).view(torch.float64)
    assert float(got_sum) == total and total > 0
    assert int(host[2]) == 4 and int(host[3]) == 0
    counts = host[4:].view(cap, 4)
    for k, (loss, tok, ref_ids, ref_extra, *_) in enumerate(keep):
        want = f1_counts_host(tok, V - 1, ref_ids, ref_extra)
        assert np.array_equal(counts[k * B:(k + 1) * B].numpy(), want), k
    assert bool((counts[4 * B:] == SENT).all())
    again, _ = run()
    assert torch.equal(host, again)


# ============================================================================= 4. the epoch against the loop written out
def _tok_model(meta, arr, device, training=True):
    H = meta["H"]
    model = dagnn_amd.DAGNN(num_vocab=meta["V"], max_seq_len=meta["S"], emb_dim=H, hidden_dim=H, out_dim=None,
                            encoder=ASTNodeEncoder(H, 98, meta["n_attr"], 20), **meta["ctor"])
    seeded_fill(model, meta["w_seed"])
    with torch.no_grad():
        for s, hd in enumerate(model.graph_pred_linear_list):
            hd.bias[meta["V"] - 1] += torch.tensor(arr["boost_eos"][s])
    return model.to(device)


def _lp_model(meta, device):
    H = meta["H"]
    model = dagnn_amd.DAGNN(num_vocab=None, max_seq_len=None, emb_dim=H, hidden_dim=H, out_dim=None,
                            encoder=ASTNodeEncoder2(H, 98, meta["n_attr"], 20), **meta["ctor"])
    seeded_fill(model, meta["w_seed"])
    return model.to(device)


_STORES = {}


def _store(name, device):
    if name not in _STORES:
        meta, arr, raw, vocab = fixture_raw(name)
        _STORES[name] = (meta, arr, dagnn_amd.GraphStore.from_graphs(raw, device, vocab))
    return _STORES[name]


def _hand_loop(task, store, model, opt, ids, bs, clip):
    """The reference's `train()` on the parent's public pieces, one host read per step."""
    model.train()
    metric = SeqF1(store.eos_id) if task == "tok" else lp.ClassAccuracy()
    accum, chunks = 0, 0
    for i in range(0, len(ids), bs):
        chunks += 1
        chunk = ids[i:i + bs]
        if len(chunk) == 1:
            continue
        batch = store.batch(chunk)
        if task == "tok":
            y_arr, ref_ids, ref_extra = batch.y_arr, batch.ref_ids, batch.ref_extra
            pred = model(batch)
            opt.zero_grad()
            loss = seq_cross_entropy(pred, y_arr)
        else:
            targ = batch.len_longest_path
            pred = model(batch)
            opt.zero_grad()
            loss = lp.class_cross_entropy(pred, targ)
        loss.backward()
        if clip > 0:
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
        opt.step()
        accum += float(loss.detach())
        if task == "tok":
            metric.update(rows_argmax(pred), ref_ids, ref_extra)
        else:
            metric.update(pred.detach(), targ)
    return accum / chunks, metric.compute()


def _assert_same_state(a, b, oa, ob):
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), k
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    assert sorted(sa) == sorted(sb) and len(sa) > 4
    for k in sa:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(torch.as_tensor(sa[k][name]).cpu(), torch.as_tensor(sb[k][name]).cpu()), (k, name)


@pytest.mark.parametrize("optim", ["clip_adam", "adam_clip"])
@pytest.mark.parametrize("task", ["tok", "lp"])
def test_epoch_equals_the_hand_written_loop_bitwise(device, monkeypatch, task, optim):
    monkeypatch.setattr(engine, "TABLE_GRADS", 1)
    meta, arr, store = _store(TOK if task == "tok" else LP, device)
    ids = list(range(36)) + [5]                        # 4 chunks of 12, 12, 12 and ONE graph: skipped, and counted
    make = (lambda: _tok_model(meta, arr, device)) if task == "tok" else (lambda: _lp_model(meta, device))
    a, b = make(), make()
    if optim == "clip_adam":
        oa, ob, clip = ClipAdam(a.parameters(), lr=1e-3, max_norm=0.25), ClipAdam(b.parameters(), lr=1e-3, max_norm=0.25), 0.0
    else:
        oa, ob, clip = torch.optim.Adam(a.parameters(), lr=1e-3), torch.optim.Adam(b.parameters(), lr=1e-3), 0.25
    got = (store.train_tok if task == "tok" else store.train_lp)(a, oa, ids, 12, clip=clip)
    want = _hand_loop(task, store, b, ob, ids, 12, clip)
    assert isinstance(got[0], float) and got[0] == want[0]
    assert got[1] == want[1] and got[1]["n"] == 36
    _assert_same_state(a, b, oa, ob)
    assert a.training


# ============================================================================= 5. the reference's own loop
def _fixture_epoch(name, device):
    """Three steps through the public step functions on the fixture's batches: per-step losses (one read each - this is a
    test), the tokens, and the epoch's result."""
    meta, arr, store = _store(name, device)
    tok_task = meta["kind"] == "code2_train_tok"
    model = _tok_model(meta, arr, device) if tok_task else _lp_model(meta, device)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=meta["lr"])
    meter = EpochMeter(device, 36, store.eos_id if tok_task else None)
    losses, toks = [], []
    for batch in store.loader(np.arange(36), 12, training=True):
        if tok_task:
            y_arr, ref_ids, ref_extra = batch.y_arr, batch.ref_ids, batch.ref_extra
            pred = model(batch)
            opt.zero_grad()
            loss = seq_ce_step(pred, y_arr, meter, ref_ids, ref_extra)
        else:
            targ = batch.len_longest_path
            pred = model(batch)
            opt.zero_grad()
            loss = lp.class_ce_step(pred, targ, meter)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        toks.append(meter.tok.cpu().numpy().reshape(12, -1))
    return meta, arr, losses, toks, meter.result(3)


@pytest.mark.parametrize("name", [TOK, LP])
def test_three_steps_against_the_reference_fixture(device, name):
    meta, arr, store = _store(name, device)
    assert_fixture_batches(meta, arr, store)
    meta, arr, losses, toks, (mean, metric) = _fixture_epoch(name, device)
    for s in range(3):
        assert np.array_equal(toks[s], arr["s%d::tok" % s]), s                  # (no token of the fixture is ambiguous)
    if meta["kind"] == "code2_train_tok":
        assert [metric["precision"], metric["recall"], metric["F1"]] == arr["f1"].tolist() and metric["n"] == 36
    else:
        assert metric == {"acc": float(arr["acc"]), "n": 36}
    ratios = []
    for s in range(3):
        bound = max(2e-4, 4 * float(arr["loss_err_ref"][s]))
        err = abs(losses[s] - float(arr["loss64"][s]))
        ratios.append(err / bound)
        print("%s step %d  loss %.9f  loss64 %.9f  err %.3e  bound %.3e" % (name, s, losses[s], float(arr["loss64"][s]), err, bound))
        assert err <= bound, (s, err, bound)
    bound = max(2e-4, 4 * abs(meta["mean_loss"] - meta["mean_loss64"]))
    err = abs(mean - meta["mean_loss64"])
    print("%s mean loss %.9f  mean_loss64 %.9f  err %.3e  bound %.3e  step ratios %s" % (name, mean, meta["mean_loss64"], err, bound, ratios))
    assert err <= bound, (err, bound)
    assert mean == sum(losses) / 3                                             # the device's float64 sum IS the host's


def test_train_tok_on_the_fixture_gives_the_fixture_metric(device):
    meta, arr, store = _store(TOK, device)
    model = _tok_model(meta, arr, device)
    mean, metric = store.train_tok(model, torch.optim.Adam(model.parameters(), lr=meta["lr"]), np.arange(36), 12)
    assert [metric["precision"], metric["recall"], metric["F1"]] == arr["f1"].tolist()
    assert abs(mean - meta["mean_loss64"]) <= max(2e-4, 4 * abs(meta["mean_loss"] - meta["mean_loss64"]))


# ============================================================================= 6. nothing synchronises inside the loop
@pytest.mark.parametrize("where", ["cuda:0", "cuda"])
@pytest.mark.parametrize("task", ["tok", "lp"])
def test_no_synchronisation_inside_the_loop(device, monkeypatch, task, where):
    """`train_tok` / `train_lp` over three chunks with torch's synchronisation check on "error" around the whole loop body -
    loader, forward, loss, backward, clip, step; only `EpochMeter.result`, the epoch's one read, runs outside it.  A first
    epoch outside the guard warms the caches.  Every step must take the fused launch: the pieces only the composed route
    calls raise, and the fused wrapper is counted.  `where`: the store made on `torch.device("cuda:0")` and on the string
    "cuda" (the module docstring's own spelling; `torch.device("cuda") != torch.device("cuda:0")`, so a route chosen by
    comparing the caller's spelling with a tensor's device would miss).

    LP: the fixture's model (`gated_sum`) runs on the per-layer variant launches, whose training forward reads the batch's
    layer schedule on the host (`PlanHandle.read_schedule`: the counterpart of the reference's `.item()` at dagnn.py:137) - a
    legitimate synchronisation of the forward, not of this feature.  There the guard is lifted for the forward alone and
    covers the loader, the loss with its metric and bookkeeping, backward and the optimizer."""
    meta, arr, store = _store(TOK if task == "tok" else LP, device)
    if where == "cuda":
        _, _, raw, vocab = fixture_raw(TOK if task == "tok" else LP)
        store = dagnn_amd.GraphStore.from_graphs(raw, "cuda", vocab)
        assert store.device != device and EpochMeter("cuda", 2, 1).device == device == EpochMeter("cuda", 0).hits.device
    model = _tok_model(meta, arr, device) if task == "tok" else _lp_model(meta, device)
    if task == "lp":
        forward = model.forward

        def unguarded(batch):
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("default")
            try:
                return forward(batch)
            finally:
                torch.cuda.set_sync_debug_mode(mode)

        monkeypatch.setattr(model, "forward", unguarded)
    opt = ClipAdam(model.parameters(), lr=1e-3, max_norm=0.25)
    run = store.train_tok if task == "tok" else store.train_lp
    run(model, opt, np.arange(36), 12)
    reads = []
    orig = EpochMeter.result

    def result(self, n):
        torch.cuda.set_sync_debug_mode("default")
        reads.append(1)
        return orig(self, n)

    monkeypatch.setattr(EpochMeter, "result", result)

    def composed(*a, **k):
        raise AssertionError("the composed route ran")

    monkeypatch.setattr(train, "seq_cross_entropy", composed)
    monkeypatch.setattr(lp, "class_cross_entropy", composed)
    for piece in ("rows_argmax", "seq_f1_counts", "class_hits", "class_ce"):
        monkeypatch.setattr(engine, piece, composed)
    fused = []
    for piece in ("seq_ce_step", "class_ce_step"):
        monkeypatch.setattr(engine, piece, lambda *a, _f=getattr(engine, piece), **k: (fused.append(1), _f(*a, **k))[1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        mean, metric = run(model, opt, np.arange(36), 12)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert reads == [1] and fused == [1, 1, 1] and np.isfinite(mean) and metric["n"] == 36


def test_a_step_without_label_sets_needs_no_room(device):
    """The fused route, like the composed one and the C entry point, asks for rows of the counts table only when the step
    counts graphs: a full table, or one smaller than the batch, still takes loss and tokens."""
    B, S, V, R = 3, 5, 7, 2
    x, y, eos, ref_ids, ref_extra, _ = _seq_case(B, S, V, R, 3, finite=True)
    base = x.to(device).requires_grad_()
    views = [base[:, i * V:(i + 1) * V] for i in range(S)]
    m = EpochMeter(device, 5, eos)
    l0 = seq_ce_step(views, y.to(device), m, ref_ids, ref_extra)
    with pytest.raises(ValueError, match="do not fit"):
        seq_ce_step(views, y.to(device), m, ref_ids, ref_extra)                 # 3 + 3 > 5
    assert m.graphs == 3 and int(m.steps) == 1
    l1 = seq_ce_step(views, y.to(device), m)
    assert m.graphs == 3 and int(m.steps) == 2 and torch.equal(l0.detach(), l1.detach())
    assert bool((m.counts[3:] == 0).all()) and float(m.loss_sum) == float(l0.detach()) + float(l1.detach())
    tiny = EpochMeter(device, 1, eos)                                           # capacity below B
    seq_ce_step(views, y.to(device), tiny)
    assert tiny.graphs == 0 and int(tiny.steps) == 1 and torch.equal(tiny.tok, m.tok)


def test_engine_class_ce_step_checks_its_logits(device):
    """Called directly, the wrapper refuses what the kernel cannot read and copies what it can only read contiguous."""
    B, C = 9, 24
    p = torch.randn(B, C, generator=torch.Generator().manual_seed(4)).to(device)
    targ = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(5)).to(device)
    qa, qb = EpochMeter(device, 0), EpochMeter(device, 0)
    la, da, ta = engine.class_ce_step(p, targ, True, qa.hits, qa.loss_sum, qa.steps)
    strided = p.t().contiguous().t()
    assert strided.stride(1) != 1
    lb, db, tb = engine.class_ce_step(strided, targ, True, qb.hits, qb.loss_sum, qb.steps)
    assert torch.equal(la, lb) and torch.equal(da, db) and torch.equal(ta, tb) and torch.equal(qa.hits, qb.hits)
    for bad in (p.double(), p.view(-1), p[:, :0], p.cpu()):
        with pytest.raises(engine.DagnnHipError):
            engine.class_ce_step(bad, targ, False, qa.hits, qa.loss_sum, qa.steps)
    assert int(qa.steps) == 1


# ============================================================================= 7. the fallback route
def test_fallback_route_gives_the_fused_route_s_numbers(device):
    B, S, V, R = 13, 5, 257, 3
    x, y, eos, ref_ids, ref_extra, _ = _seq_case(B, S, V, R, 7)
    x = torch.nan_to_num(x, nan=0.25, neginf=-30.0)                             # (finite: the losses are compared)
    base = x.to(device).requires_grad_()
    views = [base[:, i * V:(i + 1) * V] for i in range(S)]
    assert train.heads_base(views) is not None
    loose = [v.detach().clone().requires_grad_() for v in views]                # S tensors of their own
    assert train.heads_base(loose) is None
    ma, mb = EpochMeter(device, B, eos), EpochMeter(device, B, eos)
    la = seq_ce_step(views, y.to(device), ma, ref_ids, ref_extra)               # (host label sets: copied through pinned memory)
    lb = seq_ce_step(loose, y.to(device), mb, ref_ids.to(device), ref_extra.to(device))
    assert torch.equal(ma.tok, mb.tok) and torch.equal(ma.counts, mb.counts) and ma.graphs == mb.graphs == B
    assert int(ma.steps) == int(mb.steps) == 1
    want = sum(torch.nn.functional.cross_entropy(x.double()[:, i * V:(i + 1) * V], y[:, i]) for i in range(S)) / S
    tol = 4 * (2.0 ** -24) * (abs(float(want)) + float(np.log(V)) + float(x.abs().max()))   # a few roundings of the row's terms
    assert abs(float(la.detach()) - float(want)) <= tol and abs(float(lb.detach()) - float(want)) <= tol
    la.backward()
    lb.backward()
    gb = torch.cat([t.grad for t in loose], dim=1)
    assert float((base.grad - gb).abs().max()) <= 1e-6
    assert ma.result(1)[1] == mb.result(1)[1]
    # LP: a pred with strided columns takes the composed route
    C = 24
    p = torch.randn(B, C, generator=torch.Generator().manual_seed(1))
    targ = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(2)).float()
    qa, qb = EpochMeter(device, 0), EpochMeter(device, 0)
    fa = lp.class_ce_step(p.to(device).requires_grad_(), targ.to(device), qa)
    strided = p.to(device).t().contiguous().t().requires_grad_()
    assert strided.stride(1) != 1
    fb = lp.class_ce_step(strided, targ.to(device), qb)
    assert torch.equal(qa.tok, qb.tok) and torch.equal(qa.hits, qb.hits) and abs(float(fa) - float(fb)) <= 1e-6 * float(fa)
    assert qa.result(1)[1] == qb.result(1)[1]
