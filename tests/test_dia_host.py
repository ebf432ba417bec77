"""The diagonal-row-block layout of the operator product (dia_build in dune-ddm_amd/csrc/csr.hpp) through its host entry: the
layout is built and applied on the CPU with the indexing of k_spmv_dia.  Same products in the same order as the CSR row sum =>
bit-exact; the reported blocks are the ones the greedy split has to find.  No GPU needed."""
import numpy as np
import pytest

from tests.dia_cases import cases, reference_mv, vector

CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_apply_is_the_csr_row_sum(ddm, name):
    M, blocks = CASES[name]
    n = M.shape[0]
    x = vector(n, 11)
    y, kinds, counts = ddm.dia_build_and_apply_host(M, x)
    ref = reference_mv(M, x)
    assert np.array_equal(y, ref)
    assert np.array_equal(np.signbit(y), np.signbit(ref))                      # (-0.0 == 0.0 for array_equal)
    assert kinds[0, 0] == 0 and kinds[-1, 1] == n and np.array_equal(kinds[1:, 0], kinds[:-1, 1])   # the blocks tile the rows
    assert counts["blocks"] == len(kinds) == counts["dia"] + counts["csr"]
    assert counts["dia"] == int((kinds[:, 2] > 0).sum())
    assert counts["rows_dia"] == int((kinds[:, 1] - kinds[:, 0])[kinds[:, 2] > 0].sum())
    assert counts["slots"] == int(((kinds[:, 1] - kinds[:, 0]) * kinds[:, 3]).sum())
    assert ((kinds[:, 3] == kinds[:, 2]) | (kinds[:, 3] == (kinds[:, 2] + 1) // 2)).all()        # all slabs, or the offsets >= 0
    if blocks is not None:
        assert [tuple(k) for k in kinds.tolist()] == blocks


def test_block_kinds_of_the_remaining_cases(ddm):
    _, kinds, counts = ddm.dia_build_and_apply_host(CASES["45_per_row"][0], np.ones(200))
    assert counts["dia"] == 0 and counts["slots"] == 0                          # all CSR: the operator keeps the CSR product
    _, kinds, counts = ddm.dia_build_and_apply_host(CASES["irregular"][0], np.ones(200))
    assert counts["rows_dia"] <= 20                                             # (a short tail may fill its few diagonals)
    _, kinds, counts = ddm.dia_build_and_apply_host(CASES["table_changes_midway"][0], np.ones(512))
    assert counts["segments"] == 2 and counts["symmetric_segments"] == 1
    _, kinds, counts = ddm.dia_build_and_apply_host(CASES["two_boxes"][0], np.ones(270))
    assert counts["segments"] == 2 and counts["symmetric_segments"] == 2
    _, kinds, counts = ddm.dia_build_and_apply_host(CASES["one_ulp_off_symmetry"][0], np.ones(120))
    assert counts["segments"] == 1 and counts["symmetric_segments"] == 0


def test_non_finite_x_reaches_only_the_rows_that_read_it(ddm):
    M, _ = CASES["two_boxes"]
    x = vector(270, 12)
    x[100] = np.inf
    x[200] = np.nan
    y, _, _ = ddm.dia_build_and_apply_host(M, x)
    with np.errstate(invalid="ignore"):
        ref = reference_mv(M, x)
    assert np.array_equal(y, ref, equal_nan=True)
    assert np.isfinite(y[:60]).all()                                            # absent entries are skipped, not multiplied by zero
