"""The D-VAE decoder's description is checked once for both entry points (csrc/dvae_common.h behind
dagnn_dvae_decode_* and dagnn_dvae_sample; `engine._marshal_decoder` in front of them): one table of bad arguments, run
over both entry points and both struct generations; every weight pointer missing in turn; the same table from C with the
earlier struct in front of an inaccessible page (tests/native/dvae_decoder_args.cpp); and the binding's shape table with
one wrong shape per tensor.  Nothing here launches: workspace sizes are 0, so arguments that pass every check stop at
DAGNN_ENOSPC."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import pytest
import torch

from dagnn_amd import _lib, build, engine
from tests import helpers as Hh

EINVAL, ENOSPC = -22, -28
_BUF = (C.c_float * 64)()
PTR = C.addressof(_BUF)   # what every pointer of a baseline holds; never dereferenced
L = 2
WEIGHTS = ["h0", "w_key", "av_w1", "av_b1", "av_w2", "av_b2", "ae_w1", "ae_b1", "ae_w2", "ae_b2"] + \
          [(name, l) for name in ("w_ih", "w_hh", "b_ih", "b_hh") for l in range(L)]

# (id, fields to set, needs the current struct: the row sets key_type or has it looked at).  The baseline is NA attn_h
# with n 8, hs 6, L 2, nvt 5, start_type 0; ranges as dagnn_hip.h states them (MAX_N 32, MAX_STACKED 8, MAX_TYPES 64).
BAD = [
    ("n_below", dict(n=1), False), ("n_above", dict(n=_lib.DVAE_MAX_N + 1), False), ("hs_below", dict(hs=0), False),
    ("L_below", dict(L=0), False), ("L_above", dict(L=_lib.MAX_STACKED + 1), False), ("nvt_below", dict(nvt=0), False),
    ("nvt_above", dict(nvt=65), False), ("start_type_below", dict(start_type=-1), False),
    ("start_type_above", dict(start_type=5), False), ("bn_below", dict(bn=-1), False), ("bn_above", dict(bn=2), False),
    ("edge_hidden_below", dict(edge_hidden=0), False), ("vertex_hidden_below", dict(vertex_hidden=0), False),
    ("agg_below", dict(agg=-1), False), ("agg_above", dict(agg=_lib.DVAE_AGG_ATTN_X + 1), False),
    ("gated_sum_bn", dict(agg=_lib.DVAE_AGG_GATED_SUM, bn=1), False),
    ("gated_sum_no_gate_w", dict(agg=_lib.DVAE_AGG_GATED_SUM, gate_w=None), False),
    ("gated_sum_no_gate_b", dict(agg=_lib.DVAE_AGG_GATED_SUM, gate_b=None), False),
    ("gated_sum_no_mapper_w", dict(agg=_lib.DVAE_AGG_GATED_SUM, mapper_w=None), False),
    ("attn_x_na", dict(agg=_lib.DVAE_AGG_ATTN_X, bn=0), False),
    ("attn_x_no_key_type", dict(agg=_lib.DVAE_AGG_ATTN_X, bn=1, key_type=None), True),
]


STRUCTS = [_lib.DvaeDecodeArgs, _lib.DvaeDecodeArgsTyped, _lib.DvaeSampleArgs, _lib.DvaeSampleArgsTyped]


def _baseline(cls):
    a = cls()
    a.B, a.n, a.hs, a.L, a.nvt, a.start_type, a.bn, a.edge_hidden, a.vertex_hidden = 4, 8, 6, L, 5, 0, 0, 16, 32
    a.agg = _lib.DVAE_AGG_ATTN_H
    for name in WEIGHTS + ["vid_bias", "gate_w", "gate_b", "mapper_w", "types", "preds"]:
        _set(a, name, PTR)
    if hasattr(cls, "key_type"):
        a.key_type = PTR
    if issubclass(cls, _lib.DvaeSampleArgs):
        a.G, a.end_type, a.stochastic = 2, 1, 1
        a.u_type = a.u_edge = a.nv = a.work = PTR
    else:
        a.ll = a.saved = PTR
    return a   # (saved_bytes / work_bytes stay 0)


def _set(a, name, value):
    if isinstance(name, tuple):
        getattr(a, name[0])[name[1]] = value
    else:
        setattr(a, name, value)


def _grads():
    g = _lib.DvaeDecodeGradsTyped()
    for name, kind in g._fields_ + _lib.DvaeDecodeGrads._fields_:
        if name == "work_bytes":
            continue
        for l in range(L) if kind is not C.c_void_p else [None]:
            _set(g, name if l is None else (name, l), PTR)
    return g


def _queries(lib, a):
    if isinstance(a, _lib.DvaeSampleArgs):
        return [lib.dagnn_dvae_sample_work_bytes(C.byref(a))]
    return [lib.dagnn_dvae_decode_saved_bytes(C.byref(a)), lib.dagnn_dvae_decode_work_bytes(C.byref(a))]


def _entries(lib, a):
    if isinstance(a, _lib.DvaeSampleArgs):
        return [lib.dagnn_dvae_sample(C.byref(a), None)]
    return [lib.dagnn_dvae_decode_forward(C.byref(a), None), lib.dagnn_dvae_decode_backward(C.byref(a), C.byref(_grads()), None)]


@pytest.mark.parametrize("cls", STRUCTS, ids=lambda c: c.__name__)
def test_baseline_passes_every_check_and_stops_for_want_of_workspace(cls):
    lib = _lib.load()
    a = _baseline(cls)
    assert all(q > 0 for q in _queries(lib, a))
    assert _entries(lib, a) == [ENOSPC] * len(_entries(lib, a))


# (the earlier struct has no key_type for the library to miss: that it does not look is the C program's part)
BAD_CASES = [(cls, row) for cls in STRUCTS for row in BAD if not row[2] or hasattr(cls, "key_type")]


@pytest.mark.parametrize("cls,row", BAD_CASES, ids=["%s-%s" % (c.__name__, r[0]) for c, r in BAD_CASES])
def test_bad_decoder_arguments_are_refused_alike(cls, row):
    fields = row[1]
    lib = _lib.load()
    a = _baseline(cls)
    for k, v in fields.items():
        setattr(a, k, v)
    assert _queries(lib, a) == [0] * len(_queries(lib, a))
    assert _entries(lib, a) == [EINVAL] * len(_entries(lib, a))


@pytest.mark.parametrize("cls", STRUCTS, ids=lambda c: c.__name__)
def test_every_missing_weight_pointer_is_refused(cls):
    lib = _lib.load()
    for name in WEIGHTS:
        a = _baseline(cls)
        _set(a, name, None)
        assert all(q > 0 for q in _queries(lib, a)), name   # (the size queries do not look at pointers of attn_h)
        assert _entries(lib, a) == [EINVAL] * len(_entries(lib, a)), name


def test_the_same_table_from_c_with_the_earlier_struct_before_an_inaccessible_page(tmp_path):
    lib_path = _lib.load()._name
    exe = str(tmp_path / "dvae_decoder_args")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "dvae_decoder_args.cpp")
    lib_dir, lib_name = os.path.split(lib_path)
    cmd = [build.hipcc_path(), "--offload-arch=" + build.ARCH, "-std=c++17", "-O1", src, "-L" + lib_dir, "-l:" + lib_name,
           "-Wl,-rpath," + lib_dir, "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), (res.returncode, res.stdout, res.stderr)


# ------------------------------------------------------------------ the binding's shape table
MODELS = [("na", "attn_h"), ("na", "gated_sum"), ("bn", "attn_h"), ("bn", "attn_x")]


def _description(kind, agg):
    model = Hh.dvae_decoder_model(kind, max_n=6, nvt=5, hs=6, L=L, agg=agg, seed=3)
    d = model._decoder()
    assert d.agg == {"attn_h": _lib.DVAE_AGG_ATTN_H, "gated_sum": _lib.DVAE_AGG_GATED_SUM, "attn_x": _lib.DVAE_AGG_ATTN_X}[agg]
    return d


def _wrong(t):
    return t.new_zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 1,))


def _one_wrong_shape_each(d):
    """(what, description with that one tensor a column too wide) for every tensor of the description."""
    for field in ("av", "ae"):
        for i in range(4):
            ts = list(getattr(d, field))
            ts[i] = _wrong(ts[i])
            yield "%s[%d]" % (field, i), d._replace(**{field: ts})
    for l in range(d.L):
        for i in range(4):
            cells = [list(c) for c in d.cells]
            cells[l][i] = _wrong(cells[l][i])
            yield "cells[%d][%d]" % (l, i), d._replace(cells=cells)
    for field in ("w_key", "vid_bias", "key_type"):
        if getattr(d, field) is not None:
            yield field, d._replace(**{field: _wrong(getattr(d, field))})
    if d.gate is not None:
        for i in range(3):
            gate = list(d.gate)
            gate[i] = _wrong(gate[i])
            yield "gate[%d]" % i, d._replace(gate=gate)


@pytest.mark.parametrize("kind,agg", MODELS, ids=["%s_%s" % m for m in MODELS])
def test_shape_table_names_every_tensor_once_and_refuses_one_wrong_shape_each(kind, agg):
    d = _description(kind, agg)
    want = engine.decoder_shapes(d)
    views = {"attn_h": 1 + (kind == "na"), "gated_sum": 3, "attn_x": 1}[agg]
    assert len(want) == 8 + 4 * L + views and all(tuple(t.shape) == shape for t, shape in want)
    assert (d.w_key is None, d.vid_bias is None, d.key_type is None, d.gate is None) == \
        (agg != "attn_h", not (agg == "attn_h" and kind == "na"), agg != "attn_x", agg != "gated_sum")
    rows = list(_one_wrong_shape_each(d))
    assert len(rows) == len(want)
    for entry in ("dagnn_dvae_decode", "dagnn_dvae_sample"):
        engine.check_shapes(entry, want)
        for what, bad in rows:
            with pytest.raises(ValueError, match="^%s: a tensor of shape" % entry):
                engine.check_shapes(entry, engine.decoder_shapes(bad))


@pytest.mark.parametrize("kind,agg", MODELS, ids=["%s_%s" % m for m in MODELS])
def test_both_entry_points_are_marshalled_by_the_same_function(kind, agg, monkeypatch):
    """`_marshal_decoder` with the device check taken out (the tensors stay on the CPU, nothing is launched): both
    structs get the same dimensions, aggregator code and pointers, the library's own checks accept them, and a wrong
    shape is refused under the entry point's name before any field is set."""
    monkeypatch.setattr(engine, "_dev", lambda t, what, dtype=None: t.to(dtype).contiguous())
    d = _description(kind, agg)
    lib = _lib.load()
    filled = []
    for cls, entry in ((_lib.DvaeDecodeArgsTyped, "dagnn_dvae_decode"), (_lib.DvaeSampleArgsTyped, "dagnn_dvae_sample")):
        a = cls()
        kept = engine._marshal_decoder(a, d, entry)
        assert (a.n, a.hs, a.L, a.nvt, a.start_type, a.bn, a.agg) == (6, 6, L, 5, 0, int(kind == "bn"), d.agg)
        assert (a.vertex_hidden, a.edge_hidden) == (d.av[0].shape[0], d.ae[0].shape[0])
        for name, t in (("w_key", d.w_key), ("vid_bias", d.vid_bias), ("key_type", d.key_type)):
            assert getattr(a, name) == (None if t is None else t.data_ptr()), name
        if d.gate is not None:
            assert [a.gate_w, a.gate_b, a.mapper_w] == [t.data_ptr() for t in d.gate]
        assert [a.av_w1, a.av_b1, a.av_w2, a.av_b2, a.ae_w1, a.ae_b1, a.ae_w2, a.ae_b2] == [t.data_ptr() for t in d.av + d.ae]
        for l, c in enumerate(d.cells):
            assert [a.w_ih[l], a.w_hh[l], a.b_ih[l], a.b_hh[l]] == [t.data_ptr() for t in c]
        assert kept.cells[0][0].data_ptr() == d.cells[0][0].data_ptr()   # (float32 and contiguous already: borrowed, not copied)
        a.B, a.h0 = 3, PTR
        if cls is _lib.DvaeSampleArgsTyped:
            a.G, a.end_type = 2, d.end_type
        assert all(q > 0 for q in _queries(lib, a))
        filled.append(bytes(a)[cls.n.offset:cls.n.offset + 16] + bytes(a)[cls.w_ih.offset:cls.u_type.offset if hasattr(cls, "u_type") else cls.ll.offset])
        what, bad = next(_one_wrong_shape_each(d))
        with pytest.raises(ValueError, match="^%s: a tensor of shape" % entry):
            engine._marshal_decoder(cls(), bad, entry)
        with pytest.raises(_lib.DagnnHipError, match="^%s: 1 to 8 stacked cells" % entry):
            engine._marshal_decoder(cls(), d._replace(L=0, cells=[]), entry)
    assert filled[0] == filled[1]   # n, hs, L, nvt and the shared weight block w_ih .. ae_b2, byte for byte
    assert torch.is_tensor(d.params[0]) and len(d.params) == (3 if agg == "gated_sum" else 1) + 4 * L + 8
