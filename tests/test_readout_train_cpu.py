"""CPU tier (-m "not gpu") of the training read-out (csrc/readout.hip): the two batch entry points exist and their
argument validation runs before any HIP call (their mirrors against the C structs: tests/test_abi_cpu.py)."""
import ctypes as C

from dagnn_amd import _lib

EINVAL = -22
FWD, BWD = "dagnn_readout_pool_batch", "dagnn_readout_pool_backward_batch"


def _plan():
    return _lib.Plan(64, 0, 4, 3, 1, 0)   # (a non-NULL address nobody reads: every case returns before a launch)


def _fwd_job(**kw):
    j = dict(h=64, ld_h=8, width=8, scope=0, mode=_lib.POOL_ADD, col_off=0)
    j.update(kw)
    return _lib.PoolJob(j["h"], j["ld_h"], j["width"], j["scope"], j["mode"], j["col_off"])


def _bwd_job(**kw):
    j = dict(h=64, grad_h=128, ld_h=8, ld_g=8, width=8, scope=0, mode=_lib.POOL_ADD, col_off=0)
    j.update(kw)
    return _lib.PoolBwdJob(j["h"], j["grad_h"], j["ld_h"], j["ld_g"], j["width"], j["scope"], j["mode"], j["col_off"])


def test_both_symbols_exist():
    lib = _lib.load()
    for name in (FWD, BWD):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name


def test_error_returns_follow_the_other_readout_entry_points():
    lib = _lib.load()
    plan = _plan()
    for name, arr in ((FWD, (_lib.PoolJob * 1)(_fwd_job())), (BWD, (_lib.PoolBwdJob * 1)(_bwd_job()))):
        fn = getattr(lib, name)
        assert fn(None, arr, 1, 64, 8, None) == EINVAL, name                                     # NULL plan
        assert fn(C.byref(plan), None, 1, 64, 8, None) == EINVAL, name                           # NULL jobs with n > 0
        assert fn(C.byref(plan), arr, 0, 64, 8, None) == 0 and fn(C.byref(plan), None, 0, None, 8, None) == 0, name   # n == 0
        assert fn(C.byref(plan), arr, _lib.MAX_READOUT_JOBS + 1, 64, 8, None) == EINVAL, name    # more jobs than a launch takes
        assert fn(C.byref(plan), arr, -1, 64, 8, None) == EINVAL, name
        assert fn(C.byref(plan), arr, 1, None, 8, None) == EINVAL, name                          # NULL out / grad_out


def test_a_bad_job_is_refused_before_any_launch():
    """One planted bad value per case: a misplaced field in the ctypes mirror would move it."""
    lib = _lib.load()
    plan = _plan()
    bad = [dict(width=0), dict(scope=3), dict(scope=-1), dict(mode=3), dict(mode=-1), dict(col_off=-1), dict(col_off=1)]
    for kw in bad + [dict(h=None), dict(ld_h=7)]:
        arr = (_lib.PoolJob * 1)(_fwd_job(**kw))
        assert lib.dagnn_readout_pool_batch(C.byref(plan), arr, 1, 64, 8, None) == EINVAL, kw
    for kw in bad + [dict(grad_h=None), dict(ld_g=7), dict(h=None, mode=_lib.POOL_MAX), dict(ld_h=7, mode=_lib.POOL_MAX)]:
        arr = (_lib.PoolBwdJob * 1)(_bwd_job(**kw))
        assert lib.dagnn_readout_pool_backward_batch(C.byref(plan), arr, 1, 64, 8, None) == EINVAL, kw


def test_equal_grad_h_in_two_jobs_is_refused():
    lib = _lib.load()
    plan = _plan()
    arr = (_lib.PoolBwdJob * 2)(_bwd_job(col_off=0), _bwd_job(col_off=8))
    assert lib.dagnn_readout_pool_backward_batch(C.byref(plan), arr, 2, 64, 16, None) == EINVAL
    # h is read for the max only: NULL is fine otherwise (an empty plan: validated, nothing launched)
    empty = _lib.Plan(64, 0, 0, 0, 0, 0)
    arr = (_lib.PoolBwdJob * 2)(_bwd_job(h=None, ld_h=0, mode=_lib.POOL_MEAN), _bwd_job(grad_h=256, col_off=8))
    assert lib.dagnn_readout_pool_backward_batch(C.byref(empty), arr, 2, 64, 16, None) == 0
