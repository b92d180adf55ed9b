"""The per-row comparison of `tests/forward_states_f64.py` can fail, and points at the right rows: here the fp32 oracle plays
the kernel (no GPU), and faults are put into its INPUT - an in-edge dropped, two edge-feature pairs swapped - or into one row
of its output.  `check` must pass the unmodified oracle and must name the mutated node's own class first."""
import functools

import numpy as np
import pytest
import torch

from dagnn_amd import DAGNN, ASTNodeEncoder
from oracle.seeding import seeded_fill
from tests import forward_states_f64 as FS

WIDTHS = [64, 256]


@functools.lru_cache(maxsize=None)
def _model(H):
    enc = ASTNodeEncoder(H, 98, 300, 20)
    model = DAGNN(num_vocab=7, max_seq_len=2, emb_dim=H, hidden_dim=H, out_dim=None, encoder=enc, w_edge_attr=True, num_layers=2,
                  bidirectional=True, agg="attn_h", out_wx=False, out_pool_all=True, out_pool="max", dropout=0.0).eval()
    seeded_fill(model, 1000 + H)
    return model


def _small():
    return FS.graphs_of("SMALL"), FS.build_batch("SMALL")


@functools.lru_cache(maxsize=None)
def _ref(H):
    return FS.reference(_model(H), _small()[1])


def _classes(batch):
    return {d: FS.classes(batch, d) for d in (0, 1)}


def _fp32(H, batch):
    model = _model(H)
    return FS.blocks_of(FS.oracle_rows(FS._cpu_state(model), batch, FS.oracle_kw(model), torch.float32), model)


def _node_of_class(batch, k):
    """The first target of the first ladder whose forward in-degree is exactly k."""
    deg = np.bincount(batch.edge_index[1].numpy(), minlength=batch.x.shape[0])
    first = FS.N_SRC + FS.N_MID
    return first + int(np.flatnonzero(deg[first:] == k)[0])


def test_batches_meet_the_class_condition_and_the_size_limits():
    small, general = _small()[1], FS.build_batch("GENERAL")
    for b in (small, general, FS.build_batch("SMALL", twin=True), FS.build_batch("GENERAL", twin=True)):
        FS.assert_classes(b, want=FS.DEGS)
        for d in (0, 1):
            cls, lay = FS.classes(b, d)
            assert set(cls.tolist()) == set(FS.DEGS)
    assert FS.within_small_limits(small)
    assert general.x.shape[0] > FS.SMALL_LIMITS[0] and general.edge_index.shape[1] > FS.SMALL_LIMITS[1]
    # a target's predecessors span two layers; the in-edges of one node do not all carry the same pair
    cls, lay = FS.classes(small, 0)
    ei, ea = small.edge_index.numpy(), small.edge_attr.numpy()
    for k in FS.DEGS[2:]:
        v = _node_of_class(small, k)
        e = np.flatnonzero(ei[1] == v)
        assert len(set(ei[0][e].tolist())) == k and len(set(lay[ei[0][e]].tolist())) >= 2 and lay[v] >= 2
        assert len({tuple(p) for p in ea[e].tolist()}) > 1
    for b in (FS.build_batch("DVAE"), FS.build_batch("DVAE", twin=True)):
        assert FS.within_small_limits(b)
        for d in (0, 1):
            assert set(FS.classes(b, d)[0].tolist()) == {k for k in FS.DEGS if k <= 13}
    with pytest.raises(AssertionError, match="layer >= 2"):   # the degenerate graphs alone: their fan-in of 200 sits at layer 1
        FS.assert_classes(FS.collate(FS._degenerate_graphs()))


@pytest.mark.parametrize("H", WIDTHS)
def test_the_fp32_oracle_passes_on_the_batch_and_on_its_twin(H):
    graphs, batch = _small()
    twin = FS.build_batch("SMALL", twin=True)
    ref_t = FS.reference(_model(H), twin)
    for b, ref in ((batch, _ref(H)), (twin, ref_t)):
        report = FS.check(_fp32(H, b), ref, _classes(b))
        assert max(r[-1] for r in report) <= 1.0   # (it IS one of the baselines)
        assert sum(r[3] for r in report if r[0] == (0, 0)) == b.x.shape[0]   # every row of the block, once
    # the twin is the same mathematics: same classes, same float64 rows
    for d in (0, 1):
        assert np.array_equal(FS.classes(batch, d)[0], FS.classes(twin, d)[0])
    for blk, r in _ref(H)["rows"].items():
        assert float((r - ref_t["rows"][blk]).abs().max()) <= 1e-12


@pytest.mark.parametrize("k", [5, 9, 65, 129])
@pytest.mark.parametrize("H", WIDTHS)
def test_a_dropped_in_edge_fails_at_the_class_of_its_node(H, k):
    graphs, batch = _small()
    v = _node_of_class(batch, k)   # (a node of the first graph: batch ids are graph ids)
    g = graphs[0]
    last = int(np.flatnonzero(g.edge_index[1].numpy() == v)[-1])
    keep = torch.arange(g.edge_index.shape[1]) != last
    mutated = FS.collate([FS._rebuilt(g, g.edge_index[:, keep], g.edge_attr[keep])] + list(graphs[1:]))
    with pytest.raises(FS.StateMismatch) as exc:
        FS.check(_fp32(H, mutated), _ref(H), _classes(batch))
    assert (exc.value.block, exc.value.cls, exc.value.node) == ((0, 0), k, v), str(exc.value)


@pytest.mark.parametrize("H", WIDTHS)
def test_swapped_edge_features_fail_at_the_class_of_their_node(H):
    graphs, batch = _small()
    g = graphs[0]
    deg = np.bincount(g.edge_index[1].numpy(), minlength=g.x.shape[0])
    for v in np.flatnonzero(deg == 8):
        e = np.flatnonzero(g.edge_index[1].numpy() == v)
        if not torch.equal(g.edge_attr[e[4]], g.edge_attr[e[5]]):
            break
    else:
        raise AssertionError("no class-8 node whose 5th and 6th in-edge differ")
    attr = g.edge_attr.clone()
    attr[[e[4], e[5]]] = attr[[e[5], e[4]]]
    mutated = FS.collate([FS._rebuilt(g, g.edge_index, attr)] + list(graphs[1:]))
    with pytest.raises(FS.StateMismatch) as exc:
        FS.check(_fp32(H, mutated), _ref(H), _classes(batch))
    assert (exc.value.block, exc.value.cls, exc.value.node) == ((0, 0), 8, int(v)), str(exc.value)


@pytest.mark.parametrize("H", WIDTHS)
def test_one_row_off_by_1e_5_fails_at_its_class(H):
    batch = _small()[1]
    cls_by_dir = _classes(batch)
    for block, d, k in (((0, 1), 0, 13), ((1, 0), 1, 64), ((1, 1), 1, 1)):
        got = {b: t.clone() for b, t in _fp32(H, batch).items()}
        cls, lay = cls_by_dir[d]
        v = int(np.flatnonzero((cls == k) & (lay >= 2))[-1])
        got[block][v] += 1e-5
        with pytest.raises(FS.StateMismatch) as exc:
            FS.check(got, _ref(H), cls_by_dir)
        assert (exc.value.block, exc.value.cls, exc.value.node) == (block, k, v), str(exc.value)
        assert "class %d" % k in str(exc.value) and "node %d" % v in str(exc.value)
