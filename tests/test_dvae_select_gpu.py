"""`decode_from_latent_space` on the GPU (csrc/dvae_select.hip): the kernel against the `dvae_select_*` fixtures of the
reference's own dvae/util.py, and the whole function against the host mirror applied to `decode_dense`."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from dagnn_amd import _lib, dvae, engine, synth
from tests import helpers as Hh
from tests.test_dvae_select_cpu import FIXTURES, fixture_rows

pytestmark = pytest.mark.gpu

E2E = [("dvae_decode_na_h501_L2_sample", "ENAS"), ("dvae_gated_decode_na_h501_L2_sample", "ENAS"),
       ("dvae_decode_bn_h501_L2_sample", "BN")]


def _model(name, device):
    meta, _ = Hh.load(name)
    model, _ = Hh.dvae_model(meta)
    return model.to(device).eval()


def _host_keys(types, preds, nv, valid, kind, n, nvt):
    A, B = nv.shape
    keys = np.zeros((B, A, dvae.select_key_words(kind, n, nvt)), dtype=np.int64)
    for a, b in zip(*np.nonzero(valid)):
        keys[b, a] = dvae.select_key(types[a, b], preds[a, b], nv[a, b], kind, n, nvt)
    return keys


@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_matches_the_reference_fixtures(device, name):
    meta, types, preds, nv, valid = fixture_rows(name)
    kind, n, nvt = meta["kind"], meta["n"], meta["nvt"]
    form = dvae.enas_string if kind == "ENAS" else dvae.bn_adj_string
    d = dvae.DecodedDense(*(torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in (types, preds, nv)), None)
    for run, want_valid in zip(meta["runs"], valid):
        nn_ = None if run["n_nodes"] == "variable" else run["n_nodes"]
        for select, pick, same in (("first", "pick", "n_same"), ("most_common", "mode_pick", "mode_same")):
            sel = dvae.select_decoded(d, kind, nvt, 0, 1, nn_, select)
            np.testing.assert_array_equal(sel.valid.cpu().numpy().astype(bool), want_valid)
            assert sel.pick.tolist() == run[pick] and sel.n_same.tolist() == run[same], (name, select)
            assert sel.n_valid.tolist() == run["n_valid"]
            np.testing.assert_array_equal(sel.keys.cpu().numpy(), _host_keys(types, preds, nv, want_valid, kind, n, nvt))
        got = [None if p < 0 else form(types[p, b], preds[p, b], nv[p, b])
               for b, p in enumerate(dvae.select_decoded(d, kind, nvt, 0, 1, nn_).pick.tolist())]
        assert got == run["strings"]


def _mirror(model, z, A, kind, n_nodes, select="first"):
    torch.manual_seed(1234)
    d = model.decode_dense(z, True, attempts=A)
    types, preds, nv = (t.cpu().numpy() for t in (d.types, d.preds, d.nv))
    valid, pick, n_valid, n_same, _ = dvae.select_host(types, preds, nv, kind, model.nvt, model.START_TYPE, model.END_TYPE,
                                                       n_nodes, select)
    form = dvae.enas_string if kind == "ENAS" else dvae.bn_adj_string
    strings = [None if p < 0 else form(types[p, b], preds[p, b], nv[p, b]) for b, p in enumerate(pick)]
    return d, (types, preds, nv), valid, pick, n_valid, n_same, strings


@pytest.mark.parametrize("name,kind", E2E)
def test_decode_from_latent_space_matches_the_host_mirror(device, name, kind):
    """bo.py's call - decode_from_latent_space(z, model, 500, max_n, False, data_type) at B = 50 - against the host mirror
    on decode_dense under the same seed; return_igraph's graphs are the last equal-string rows of the call."""
    model = _model(name, device)
    z = torch.from_numpy(np.random.default_rng(5).standard_normal((50, 56)).astype(np.float32)).to(device)
    n = model.max_n
    for n_nodes in (n, "variable"):
        nn_ = None if n_nodes == "variable" else n_nodes
        d, (types, preds, nv), valid, pick, n_valid, n_same, strings = _mirror(model, z, 500, kind, nn_)
        sel = model.select_dense(d, kind, nn_)
        np.testing.assert_array_equal(sel.valid.cpu().numpy().astype(bool), valid)
        assert sel.pick.tolist() == pick.tolist() and sel.n_valid.tolist() == n_valid.tolist()
        assert sel.n_same.tolist() == n_same.tolist()
        torch.manual_seed(1234)
        assert dvae.decode_from_latent_space(z, model, 500, n_nodes, False, kind) == strings
        torch.manual_seed(1234)
        graphs, strings2 = dvae.decode_from_latent_space(z, model, 500, n_nodes, True, kind)
        assert strings2 == strings
        form = dvae.enas_string if kind == "ENAS" else dvae.bn_adj_string
        last = {}
        for bb in range(50):
            for a in np.nonzero(valid[:, bb])[0]:
                last[form(types[a, bb], preds[a, bb], nv[a, bb])] = (bb, a)
        for b, g in enumerate(graphs):
            if strings[b] is None:
                assert g is None
                continue
            sb, sa = last[strings[b]]
            want = dvae.graphs_from_dense(types[sa, sb][None], preds[sa, sb][None], nv[sa, sb][None], model.END_TYPE)[0]
            assert g.vs["type"] == want.vs["type"] and sorted(g.get_edgelist()) == sorted(want.get_edgelist())
        torch.manual_seed(1234)
        assert dvae.decode_from_latent_space(z, model, 500, n_nodes, False, kind, select="most_common") == \
            _mirror(model, z, 500, kind, nn_, "most_common")[-1]


def test_result_does_not_depend_on_the_chunk(device):
    model = _model("dvae_decode_na_h64_L2_sample", device)
    z = torch.from_numpy(np.random.default_rng(6).standard_normal((50, 56)).astype(np.float32)).to(device)
    out = []
    for chunk in (1, 64, 500, None):
        torch.manual_seed(99)
        out.append(dvae.decode_from_latent_space(z, model, 500, "variable", True, "ENAS", chunk=chunk))
    for graphs, strings in out[1:]:
        assert strings == out[0][1]
        assert [None if g is None else (g.vs["type"], g.get_edgelist()) for g in graphs] == \
            [None if g is None else (g.vs["type"], g.get_edgelist()) for g in out[0][0]]
    st, se = dvae.draw_shapes(model.max_n, 50, 500)
    torch.manual_seed(99)
    u = torch.rand(int(np.prod(st)) + int(np.prod(se)), device=device)
    draws = (u[:int(np.prod(st))].view(st), u[int(np.prod(st)):].view(se))
    assert dvae.decode_from_latent_space(z, model, 500, "variable", False, "ENAS", draws=draws, chunk=37) == out[0][1]


@pytest.mark.parametrize("kind,n,nvt", [("ENAS", 8, 8), ("BN", 10, 10), ("ENAS", 32, 64), ("BN", 32, 30)])
def test_large_attempt_counts_match_the_host_mirror(device, kind, n, nvt):
    """A = 5000 attempts: more keys than one LDS tile holds; and the widest keys (n = 32)."""
    A, B = (5000, 4) if n < 32 else (700, 3)
    types, preds, nv = synth.decoded_rows(17 + n, kind, A, B, n, nvt)
    d = dvae.DecodedDense(*(torch.from_numpy(x).to(device) for x in (types, preds, nv)), None)
    for select in ("first", "most_common"):
        valid, pick, n_valid, n_same, _ = dvae.select_host(types, preds, nv, kind, nvt, 0, 1, None, select)
        sel = dvae.select_decoded(d, kind, nvt, 0, 1, None, select)
        np.testing.assert_array_equal(sel.valid.cpu().numpy().astype(bool), valid)
        assert sel.pick.tolist() == pick.tolist() and sel.n_same.tolist() == n_same.tolist()
        assert sel.n_valid.tolist() == n_valid.tolist()
    np.testing.assert_array_equal(sel.keys.cpu().numpy(), _host_keys(types, preds, nv, valid, kind, n, nvt))


def test_select_dense_does_not_synchronise_and_repeats_bitwise(device):
    model = _model("dvae_decode_bn_h32_L3_sample", device)
    z = torch.from_numpy(np.random.default_rng(8).standard_normal((50, 56)).astype(np.float32)).to(device)
    d = model.decode_dense(z, True, attempts=500)
    first = model.select_dense(d, "BN")   # (warm-up: library load, allocator)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        runs = [model.select_dense(d, "BN", select=s) for s in ("first", "most_common", "first")]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(first, runs[2]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0].valid, runs[1].valid) and torch.equal(runs[0].n_valid, runs[1].n_valid)
    out = engine.dvae_select(d.types, d.preds, d.nv, model.nvt, 0, 1, _lib.DVAE_BN, 0, _lib.DVAE_FIRST_VALID)
    for a, b in zip(out, first):
        assert torch.equal(a, b)
