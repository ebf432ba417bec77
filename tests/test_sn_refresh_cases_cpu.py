"""CPU proof of what tests/sn_refresh_cases.py promises (no GPU needed): the new values of every case of tests/sn_cases.py keep the
pattern (explicit zeros included) and satisfy the precondition of the factorisation they are handed to -- exactly symmetric and
strictly dominant with a positive diagonal for Cholesky (hence positive definite), strictly column dominant for L U (hence no row
exchange) -- and the partners of the refinement, failure and hand-over tests are what they are said to be."""
import numpy as np
import pytest

from tests import refresh_cases as rc
from tests import sn_cases as sc
from tests import sn_refresh_cases as src


def test_every_case_has_new_values():
    assert set(src.CHOLESKY) | set(src.LU) == set(sc.NAMES) and set(src.LU_SEED) == set(src.LU)


@pytest.mark.parametrize("name", src.CHOLESKY)
def test_cholesky_values(ddm, name):
    c = sc.case(name)
    M = src._sorted(c.M)
    assert src.symmetric_pattern(M) and src.is_symmetric(M)
    M2 = src.new_matrix(name)
    assert rc.same_pattern(M, M2) and M2.nnz == M.nnz, "explicit zeros are kept"
    assert src.is_symmetric(M2)
    rc.assert_dominant(M2)
    assert M2.diagonal().min() > 0
    rows = src._rows(M)
    off = (M.indices != rows) & (M.data != 0)
    q = M2.data[off] / M.data[off]
    assert q.min() >= 0.7 and q.max() <= 1.3 and q.std() > 0.1
    assert not np.array_equal(M2.data, M.data)
    # dominance with a positive diagonal => positive definite: the smallest Gershgorin bound is positive
    radius = np.asarray(abs(M2).sum(axis=1)).ravel() - np.abs(M2.diagonal())
    assert (M2.diagonal() - radius).min() > 0
    if c.n <= 400:                                               # (and directly, where a dense factorisation is cheap)
        np.linalg.cholesky(M2.toarray())


def test_new_values_of_the_ilu_tests_are_not_symmetric(ddm):
    """why the Cholesky cases have a rule of their own"""
    M = src._sorted(sc.case("chain1d").M)
    assert not src.is_symmetric(rc.new_values(M, 11))


@pytest.mark.parametrize("name", src.LU)
def test_lu_values(ddm, name):
    c = sc.case(name)
    M, M2 = src._sorted(c.M), src.new_matrix(name)
    assert rc.same_pattern(M, M2)
    if name in sc.EXCHANGING:                                    # (dominant once its rows are exchanged: tests/test_sn_cases_reference.py)
        assert sc.column_dominance(M) < 0 and sc.column_dominance(M2) > 0
    else:
        assert sc.column_dominance(M) > 0 and sc.column_dominance(M2) > 0
    assert not np.array_equal(M.data, M2.data)
    assert abs(M2 - M2.T).max() > 1e-3 * abs(M2).max()


def test_pivoting_partners(ddm):
    M, bp = src.pivoting()
    B = src.pivoting_benign()
    assert rc.same_pattern(M, B) and sc.column_dominance(B) > 0
    assert sc.column_dominance(M) < 0                           # (the pivoting matrix itself is far from it)
    assert np.array_equal(src.pivoting_like(1e-6).data, M.data)
    H = src.pivoting_like(src.HANDOVER_SCALE)
    assert rc.same_pattern(M, H)
    rows = src._rows(M)
    third = (M.indices == rows) & (rows % 3 == 0)                # the entries that differ: every third diagonal entry
    assert np.array_equal(H.data[~third], M.data[~third])
    assert np.allclose(H.data[third], M.data[third] * (src.HANDOVER_SCALE / 1e-6), rtol=1e-12, atol=0) and np.all(H.data[third] != 0)


@pytest.mark.parametrize("name", ("one21", "chain1d"))
def test_not_positive_definite_partner(ddm, name):
    M2 = src.new_matrix(name)
    N, i = src.not_positive_definite(M2)
    assert rc.same_pattern(M2, N) and src.is_symmetric(N)
    assert N[i, i] == -M2[i, i] and N[i, i] < 0                  # e_i^T N e_i < 0: not positive definite
    assert int(np.sum(N.data != M2.data)) == 1
    if N.shape[0] <= 400:                                        # (and directly, where dense eigenvalues are cheap)
        assert np.linalg.eigvalsh(N.toarray())[0] < 0
