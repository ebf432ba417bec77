"""The x windows of the diagonal-row-block layout (dia_build in dune-ddm_amd/csrc/csr.hpp) through the two host entries: the
layout is built and applied on the CPU, x indexed through the window positions exactly as k_spmv_dia reads its LDS array.  Same
products in the same order as the CSR row sum => bit-exact, staged or not; the runs, window sizes and staged flags are the ones
the merge rule (an offset joins the run before it when at most WG apart) and the capacity give.  No GPU needed."""
import numpy as np
import pytest

from tests.dia_cases import cases, reference_mv, vector
from tests.dia_window_cases import window_cases

WG = 256
OLD = {name: (M, None, None) for name, (M, _) in cases().items()}
_REF = {}


def _all_cases(ddm):
    _, capacity = ddm.dia_windows_host(OLD["one_by_one"][0])
    return {**OLD, **window_cases(capacity, WG)}, capacity


NAMES = sorted(OLD) + sorted(window_cases())


def _reference(name, M, x):
    if name not in _REF:
        with np.errstate(invalid="ignore"):
            _REF[name] = reference_mv(M, x)
    return _REF[name]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.parametrize("stage", ["default", "0"])
@pytest.mark.parametrize("name", NAMES)
def test_windows_and_host_apply(ddm, monkeypatch, name, stage):
    if stage == "0":
        monkeypatch.setenv("DDM_SPMV_STAGE_X", "0")
    else:
        monkeypatch.delenv("DDM_SPMV_STAGE_X", raising=False)
    all_cases, capacity = _all_cases(ddm)
    M, x, expected = all_cases[name]
    n = M.shape[0]
    x = vector(n, 11) if x is None else x
    y, kinds, counts = ddm.dia_build_and_apply_host(M, x)
    ref = _reference(name, M, x)
    assert np.array_equal(y, ref, equal_nan=True)
    finite = np.isfinite(ref)
    assert _same_bits(y[finite], ref[finite])                                   # the sign of a zero counts
    assert np.array_equal(np.isnan(y), np.isnan(ref))
    segs, cap = ddm.dia_windows_host(M)
    assert cap == capacity >= 2048 and len(segs) == counts["segments"]
    for s in segs:                                                              # the invariants of every table
        runs = s["runs"]
        assert 1 <= len(runs) <= 32
        at = 0
        for j, (first, length, start) in enumerate(runs):
            assert start == at and length >= WG
            if j:
                assert first - (runs[j - 1][0] + runs[j - 1][1] - WG) > WG          # more than WG behind the last offset of the run before
            at += length
        assert s["window"] == at
        assert s["staged"] == (stage == "default" and at <= capacity)
    if expected is not None:
        assert [(s["staged"], len(s["runs"]), s["window"]) for s in segs] == [(st and stage == "default", r, w) for st, r, w in expected]


def test_staged_segments_of_the_earlier_cases(ddm, monkeypatch):
    monkeypatch.delenv("DDM_SPMV_STAGE_X", raising=False)
    segs, _ = ddm.dia_windows_host(OLD["csr_in_the_middle"][0])                 # CSR-stream and staged blocks in one launch
    assert [(s["staged"], s["runs"]) for s in segs] == [(True, [(-2, WG + 4, 0)])] * 2
    segs, _ = ddm.dia_windows_host(OLD["two_boxes"][0])
    assert [(s["staged"], len(s["runs"]), s["window"]) for s in segs] == [(True, 1, WG + 2 * 26), (True, 1, WG + 2 * 50)]
    segs, _ = ddm.dia_windows_host(OLD["45_per_row"][0])                        # all CSR: no segment
    assert segs == []


def test_absent_entries_are_skipped_not_added_as_zero(ddm, monkeypatch):
    monkeypatch.delenv("DDM_SPMV_STAGE_X", raising=False)
    all_cases, _ = _all_cases(ddm)
    M, x, _ = all_cases["empty_column"]
    y, _, _ = ddm.dia_build_and_apply_host(M, x)
    c = int(np.flatnonzero(np.isnan(x))[0])
    assert M[:, c].nnz == 0
    assert np.isinf(y[[c - 4, c - 3, c + 3, c + 4]]).all()                      # rows that read one of the two infinite entries, and not x[c]
    assert np.isfinite(np.delete(y, np.arange(c - 4, c + 5))).all()
