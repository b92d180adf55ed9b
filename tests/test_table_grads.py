"""The summation order of the embedding-table gradients (`dagnn_table_grads`) as its host mirror states it
(`autograd.table_grads_host`), on the CPU: against float64 within the bound the order implies, and on hand-computed cases
that tell the order from a strict left-to-right sum.

Bound.  A row of n members in m = ceil(n / 32) chunks: a term passes at most k = min(n, 32) - 1 + max(m - 1, 0) rounding
adds (the adds inside its chunk, then the adds of the later partials; +0.0 + p0 is exact), so
|out - exact| <= k u / (1 - k u) sum |g| with u = 2^-24."""
import ctypes as C

import numpy as np
import torch

from dagnn_amd import _lib
from dagnn_amd.autograd import TABLE_GRADS_CHUNK, table_grads_host

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126


def order_bound(g, key, R):
    """(exact float64 sums, the bound above) of one table."""
    g64 = torch.from_numpy(np.asarray(g, dtype=np.float64))
    key = np.asarray(key).reshape(-1)
    ok = (key >= 0) & (key < R)
    idx = torch.from_numpy(key[ok].astype(np.int64))
    want = torch.zeros(R, g64.shape[1], dtype=torch.float64).index_add_(0, idx, g64[torch.from_numpy(ok)]).numpy()
    sumabs = torch.zeros(R, g64.shape[1], dtype=torch.float64).index_add_(0, idx, g64[torch.from_numpy(ok)].abs()).numpy()
    n = np.bincount(key[ok], minlength=R).astype(np.float64)
    m = np.ceil(n / TABLE_GRADS_CHUNK)
    k = (np.minimum(n, TABLE_GRADS_CHUNK) - 1).clip(min=0) + (m - 1).clip(min=0)
    return want, (k * U / (1 - k * U))[:, None] * sumabs


def spread_gradients(N, H, seed):
    """Normal values times 10^(-3 .. 3): a sum in another order differs in its last bits."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, H)) * 10.0 ** rng.uniform(-3, 3, (N, H))).astype(np.float32)


def skewed_keys(N, R, seed, share=0.6):
    """`share` of the nodes on one key, the rest uniform over the table."""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, R, N)
    key[rng.random(N) < share] = min(7, R - 1)
    return key


def test_chunk_is_one_constant_in_header_binding_and_mirror():
    assert _lib.TABLE_GRADS_CHUNK == TABLE_GRADS_CHUNK == 32   # (binding against header: tests/test_abi_cpu.py)


def raw_call(g, ld_g, N, H, tables, ws, ws_bytes, stages=0, stream=None):
    """`dagnn_table_grads` on raw addresses; tables: (keys, key_stride, R, out, ld_out) each."""
    a = _lib.TableGradsArgs()
    a.g, a.ld_g, a.N, a.H, a.num_tables = g, ld_g, N, H, len(tables)
    for t, tab in enumerate(tables[:_lib.TABLE_GRADS_MAX_TABLES]):
        a.table[t] = _lib.TableGradsTable(*tab)
    a.workspace, a.workspace_bytes, a.stages = ws, ws_bytes, stages
    return _lib.load().dagnn_table_grads(C.byref(a), stream)


def refused_calls(g, keys, out, ws, ws_bytes, N=100, H=8, R=9):
    """Every argument error of the header, each on otherwise valid arguments; the checks come before any HIP call."""
    tab = lambda keys=keys, stride=1, R=R, out=out, ld=H: (keys, stride, R, out, ld)   # noqa: E731
    call = lambda g=g, ld_g=H, N=N, H=H, tables=None, ws=ws, nb=ws_bytes, stages=0: raw_call(   # noqa: E731
        g, ld_g, N, H, [tab()] if tables is None else tables, ws, nb, stages)
    einval = {
        "g NULL": call(g=None), "keys NULL": call(tables=[tab(keys=None)]), "out NULL": call(tables=[tab(out=None)]),
        "workspace NULL": call(ws=None), "H % 4": call(H=6, ld_g=8), "H 0": call(H=0), "ld_g < H": call(ld_g=4),
        "ld_g % 4": call(ld_g=9), "ld_out < H": call(tables=[tab(ld=4)]), "ld_out % 4": call(tables=[tab(ld=10)]),
        "N 2^24": call(N=1 << 24), "N < 0": call(N=-1), "R 0": call(tables=[tab(R=0)]), "R 2^24": call(tables=[tab(R=1 << 24)]),
        "no table": call(tables=[]), "four tables": call(tables=[tab()] * 4), "g misaligned": call(g=g + 4),
        "out misaligned": call(tables=[tab(out=out + 8)]), "stages": call(stages=3), "out NULL, N 0": call(N=0, tables=[tab(out=None)]),
    }
    assert all(rc == -22 for rc in einval.values()), einval
    assert call(nb=64) == -28


def test_argument_errors_are_refused_on_the_host():
    lib = _lib.load()
    a = 4096   # (never dereferenced: every call is refused before a launch)
    refused_calls(a, a, a, a, 1 << 30)
    rows = (C.c_int64 * 3)(98, 10030, 21)
    size = lib.dagnn_table_grads_workspace_bytes
    assert size(16561, 256, rows, 3) > 0 and size(16561, 256, rows, 3) % 16 == 0 and size(0, 256, rows, 3) > 0
    assert size(1 << 24, 256, rows, 3) == 0 and size(100, 6, rows, 3) == 0 and size(100, 8, rows, 4) == 0 and size(100, 8, rows, 0) == 0
    assert size(100, 8, (C.c_int64 * 1)(0), 1) == 0 and size(100, 8, (C.c_int64 * 1)(1 << 24), 1) == 0
    assert size(16561, 256, rows, 3) < 16 << 20     # the headline call: the key counts dominate (64 node ranges x 10 149 rows)


def test_mirror_within_the_bound_of_its_order():
    for N, R, seed in ((1, 5, 0), (33, 1, 1), (700, 21, 2), (5000, 98, 3), (16000, 10030, 4)):
        g = spread_gradients(N, 8, seed)
        for key in (skewed_keys(N, R, seed), np.random.default_rng(seed).integers(0, R, N), np.zeros(N, dtype=np.int64)):
            out, = table_grads_host(g, [key], [R])
            assert out.dtype == np.float32 and out.shape == (R, 8)
            want, bound = order_bound(g, key, R)
            err = np.abs(out.astype(np.float64) - want)
            assert (err <= bound + FLT_MIN).all(), (N, R, float((err - bound).max()))


def test_the_order_is_not_a_strict_sequential_sum():
    """34 members: 2^24, 31 zeros, 1, 1.  Chunk 0 sums to 2^24, chunk 1 to 2, (0 + 2^24) + 2 = 2^24 + 2; one after the other
    in fp32 both ones are lost to rounding (2^24 + 1 ties to even, 2^24)."""
    col = np.array([2.0 ** 24] + [0.0] * 31 + [1.0, 1.0], dtype=np.float32)
    seq = np.float32(0)
    for x in col:
        seq = np.float32(seq + x)
    assert float(seq) == 2.0 ** 24
    out, = table_grads_host(col[:, None].repeat(4, 1), [np.zeros(34, dtype=np.int64)], [1])
    assert out.shape == (1, 4) and (out == np.float32(2.0 ** 24 + 2)).all()
    # the same values in 32 members are one chunk: both orders lose the ones
    col32 = np.array([2.0 ** 24] + [0.0] * 29 + [1.0, 1.0], dtype=np.float32)
    out32, = table_grads_host(col32[:, None].repeat(4, 1), [np.zeros(32, dtype=np.int64)], [1])
    assert (out32 == np.float32(2.0 ** 24)).all()
    # chunks are cut by position in the row's list, not by node index: other rows' nodes in between change nothing
    key = np.full(68, 1, dtype=np.int64)
    key[0::2] = 0
    g = np.zeros((68, 4), dtype=np.float32)
    g[0::2] = col[:, None]
    out2, = table_grads_host(g, [key], [2])
    assert (out2[0] == np.float32(2.0 ** 24 + 2)).all() and (out2[1] == 0).all()


def test_empty_rows_are_positive_zero_and_foreign_keys_are_ignored():
    g = np.full((6, 4), -0.0, dtype=np.float32)
    g[3] = 5.0
    out, = table_grads_host(g, [np.array([0, 0, -1, 2, 4, 9])], [4])     # -1, R and beyond: ignored
    assert not np.signbit(out).any()                                     # +0.0 + (-0.0 + -0.0) = +0.0; rows 1 and 3 are empty
    assert (out[2] == 5.0).all() and (out[[0, 1, 3]] == 0).all()
    out_r, = table_grads_host(g, [np.array([0, 0, 4, 2, 4, 9])], [5])
    assert (out_r[:4] == out).all() and (out_r[4] == 0).all()


def test_strided_key_views_and_tensors():
    N = 300
    gen = torch.Generator().manual_seed(5)
    x = torch.stack([torch.randint(0, 9, (N,), generator=gen), torch.randint(0, 31, (N,), generator=gen)], 1)
    depth = torch.randint(0, 6, (N,), generator=gen)
    g = torch.from_numpy(spread_gradients(N, 12, 6))
    outs = table_grads_host(g, [x[:, 0], x[:, 1], depth], [9, 31, 6])
    assert not x[:, 1].is_contiguous() and [o.shape for o in outs] == [(9, 12), (31, 12), (6, 12)]
    for o, key, R in zip(outs, (x[:, 0], x[:, 1], depth), (9, 31, 6)):
        again, = table_grads_host(g.numpy(), [key.contiguous().numpy()], [R])
        assert np.array_equal(o, again)
        want, bound = order_bound(g.numpy(), key.numpy(), R)
        assert (np.abs(o.astype(np.float64) - want) <= bound + FLT_MIN).all()
