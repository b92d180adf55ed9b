"""The host-side pieces the three differentiable recurrences share (`autograd.wgrad_jobs`, `autograd.unflatten_params`,
`engine.PassRecord`): what they hand on, checked without a GPU."""
import pytest
import torch

from dagnn_amd import DAGNN, ASTNodeEncoder, autograd, engine, variants
from dagnn_amd.route import Route


@pytest.mark.parametrize("dirs,L", [((0, 1), 2), ((1,), 1)])
def test_wgrad_jobs_come_in_cell_order_input_side_first(dirs, L):
    N, H, Hp = 5, 6, 8
    res = {(d, i): {"dgi": torch.full((N, 3 * Hp), 10.0 * d + i), "dgh": torch.full((N, 3 * Hp), 10.0 * d + i + 0.5),
                    "a": torch.full((N, Hp), 100.0 + 10 * d + i)} for d in dirs for i in range(L)}
    inputs = {k: torch.full((N, 3), 200.0 + 10 * k[0] + k[1]) for k in res}
    jobs = autograd.wgrad_jobs(res, lambda d, i: inputs[(d, i)], dirs, L, H)
    cells = [(d, i) for d in dirs for i in range(L)]
    assert len(jobs) == 2 * len(cells)
    for q, k in enumerate(cells):
        (dgi, inp, bias_i), (dgh, agg, bias_h) = jobs[2 * q], jobs[2 * q + 1]
        assert dgi is res[k]["dgi"] and inp is inputs[k] and bias_i is True
        assert dgh is res[k]["dgh"] and bias_h is True
        assert tuple(agg.shape) == (N, H) and agg.data_ptr() == res[k]["a"].data_ptr() and agg.stride(0) == Hp   # the first H columns, pitch kept


@pytest.mark.parametrize("kw", [dict(agg="add", w_edge_attr=True), dict(agg="gated_sum", w_edge_attr=False),
                                dict(agg="attn_h", w_edge_attr=True, recurr=0)], ids=["add_edge_encoder", "gated_sum", "recurr0"])
def test_unflatten_params_round_trips_cell_params(kw):
    H, L = 8, 2
    m = DAGNN(num_vocab=8, max_seq_len=2, emb_dim=H, hidden_dim=H, out_dim=None, encoder=ASTNodeEncoder(H, 98, 10030, 20),
              num_layers=L, bidirectional=True, out_wx=False, out_pool_all=False, out_pool="max", dropout=0.0, **kw)
    spec = {(d, i): variants._cell_params(m, d, i) for d in m.dirs for i in range(L)}
    flat = [p for d in m.dirs for i in range(L) for _, p in spec[(d, i)]]
    names, cellp = autograd.unflatten_params(m, flat)
    assert names == [(d, i, n) for d in m.dirs for i in range(L) for n, _ in spec[(d, i)]]
    assert len(names) == len(flat) and list(cellp) == list(spec)
    for k, cell in spec.items():
        assert list(cellp[k]) == [n for n, _ in cell]
        assert all(cellp[k][n] is p for n, p in cell)
    assert [cellp[(d, i)][n] is p for (d, i, n), p in zip(names, flat)] == [True] * len(flat)   # and back: flat order again


def test_pass_record_reports_its_handover():
    stat = Route(64, 5, "dataflow", 0, None, True, "dataflow", None)
    rec = engine.PassRecord(stat)
    assert rec.route is stat and rec.handover() is None   # nothing handed over before the forward launch ran
    rec.stat[(0, 0)] = torch.zeros(4)
    assert rec.handover() == "stat"
    rec = engine.PassRecord()
    rec.gh[(0, 0)] = torch.zeros(4)
    assert rec.handover() == "preact" and not rec.gi   # (a single layer keeps no gi)
    assert engine.PassRecord().handover() is None
    with pytest.raises(AttributeError):
        rec.preact = {}   # (typed: no keys beyond the slots)
