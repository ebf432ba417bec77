"""CPU checks of the value refresh (no GPU needed): the host twin of the pipe engine's scatter kernel on every case of
tests/pipe_cases.py, the argument check of TwoLevelSchwarz.update_values, and the prototypes of the new exports.

The twin (pipe::refresh_values, csrc/trsv_pipe_host.hpp) writes a row's factor values where pipe::build put them, found from the
row's slot word alone -- what k_pipe_scatter does on the device with the same words.  A stream built from the factor of M and
refreshed with the factor of new_values(M) must be, byte for byte, the stream built from the second factor, and the emulated kernel
must solve with it what the oracle solves."""
import ctypes
import functools
import os
import subprocess
import types

import numpy as np
import pytest

from tests import pipe_cases as pc
from tests import refresh_cases as rc

CPP = pc.CPP


@functools.lru_cache(maxsize=None)
def harness():
    """tests/cpp/refresh_host_test.cpp with the flags of the libpipe_host_test.so line of tests/cpp/Makefile"""
    out = os.path.join(CPP, "build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "librefresh_host_test.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O2", "-Wall", "-fPIC", "-ffp-contract=off", "-shared",
                           "-I" + os.path.join(pc.ROOT, "dune-ddm_amd", "csrc"), "-o", so, os.path.join(CPP, "refresh_host_test.cpp"), "-lpthread"])
    lib = ctypes.CDLL(so)
    lib.refresh_test_case.restype = ctypes.c_int
    return lib


@pytest.mark.parametrize("name", pc.NAMES)
def test_refreshed_stream_is_the_stream_built_from_the_new_factor(ddm, name):
    c = pc.case(name)                                            # (ddm: some generators import the package's synthesis)
    M2 = rc.new_values(c.M, 7)
    rc.assert_dominant(M2)
    assert rc.same_pattern(c.M, M2) and not np.array_equal(M2.data, c.M.data)
    _, lu1, diag = pc.oracle_factor(c.M)
    f2, lu2, diag2 = pc.oracle_factor(M2)
    assert np.array_equal(diag, diag2)
    d = pc.ref(name).d[0]
    x_ref = pc.oracle_solve(f2, d)
    n = c.n
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rp, ci = np.asarray(c.M.indptr, dtype=np.int64), np.asarray(c.M.indices, dtype=np.int32)
    bp = np.asarray(c.block_ptr, dtype=np.int64)
    lu1, lu2 = np.ascontiguousarray(lu1, dtype=np.float64), np.ascontiguousarray(lu2, dtype=np.float64)
    diag = np.ascontiguousarray(diag, dtype=np.int64)
    dd = np.ascontiguousarray(d, dtype=np.float64)
    x = np.full(n, np.nan)
    out = np.zeros(4, dtype=np.int64)
    err = ctypes.create_string_buffer(256)
    got = harness().refresh_test_case(ctypes.c_int64(n), p(rp), p(ci), p(lu1), p(lu2), p(diag), ctypes.c_int(len(bp) - 1), p(bp), ctypes.c_int(pc.DELTA),
                                      ctypes.c_int(pc.MAX_SPAN), ctypes.c_int(pc.VOTE), ctypes.c_int(pc.PACK_STEPS), p(dd), p(x), p(out), err, 256)
    if name in pc.DECLINES:                                      # nothing to refresh: the factor ends on xcd2, whatever its values
        assert got == 1 and err.value.decode() == pc.DECLINES[name], (got, err.value)
        return
    assert got == 0, (got, err.value)
    nbytes, before, after, same_layout = out.tolist()
    print(f"\n{name}: stream {nbytes} bytes, {before} differ before the refresh, {after} after it")
    assert same_layout == 1, "the schedule depends on the values"
    assert before > 0                                            # (the two factors do differ; `packed` has inverse pivots only)
    assert after == 0
    assert np.array_equal(x, x_ref), int(np.sum(x != x_ref))


def test_update_values_checks_the_lengths_first(ddm):
    """update_values compares both lengths with the stored patterns before it touches anything else: on an object that only has the
    two matrices' entry counts, wrong lengths raise ValueError, right ones get past the check and fail on the first attribute the
    refresh itself needs (AttributeError)."""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    tl = object.__new__(TwoLevelSchwarz)                        # no __init__: no device, no context
    tl.A, tl.A_dir = types.SimpleNamespace(nnz=10), types.SimpleNamespace(nnz=12)
    for na, nd in ((9, 12), (10, 11), (12, 10), (0, 0), (11, 13)):
        with pytest.raises(ValueError, match="update_values"):
            tl.update_values(np.zeros(na), np.zeros(nd))
    with pytest.raises(ValueError, match="update_values"):
        tl.update_values(np.zeros((10, 1)), np.zeros(12))
    with pytest.raises(AttributeError):
        tl.update_values(np.zeros(10), np.zeros(12))


def test_wrappers_check_shapes_before_the_library(ddm):
    A = object.__new__(ddm.CsrMatrix)
    A.nnz = 5
    with pytest.raises(ValueError, match="set_values"):
        A.set_values(np.zeros(4))
    G = object.__new__(ddm.GalerkinPreconditioner)
    G.K = 3
    with pytest.raises(ValueError, match="set_inverse"):
        G.set_inverse(np.zeros((3, 2)))


def test_new_exports_are_declared(ddm):
    names = ("ddm_csr_set_values", "ddm_ilu0_refresh", "ddm_schwarz_refresh", "ddm_op_refresh", "ddm_galerkin_set_inverse")
    header = open(os.path.join(pc.ROOT, "include", "ddm_hip.h")).read()
    for name in names:
        assert name in ddm.SYMBOLS and ("int " + name + "(") in header, name
    if os.path.exists(ddm.LIB_PATH):
        lib = ctypes.CDLL(ddm.LIB_PATH)
        for name in names:
            assert hasattr(lib, name), name


def test_new_values_rule():
    """the rule itself: same pattern, factors in [0.7, 1.3] off the diagonal, not symmetric, strictly dominant rows"""
    M = pc.case("w13").M
    M2 = rc.new_values(M, 3)
    rc.assert_dominant(M2)
    assert rc.same_pattern(M, M2)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    off = M.indices != rows
    q = M2.data[off] / M.data[off]
    assert q.min() >= 0.7 and q.max() <= 1.3 and q.std() > 0.1
    assert abs(M2 - M2.T).max() > 1e-3
    with pytest.raises(AssertionError):
        rc.assert_dominant(rc.with_data(M, np.where(off, M.data, 0.5 * M.data)))
