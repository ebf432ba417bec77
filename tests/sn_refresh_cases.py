"""New values for the matrices of tests/sn_cases.py in their unchanged patterns, shared by tests/test_sn_refresh_cases_cpu.py (which
proves the preconditions stated here) and tests/test_gpu_sn_refresh.py: the value refresh of the DEVICE supernodal factor
(csrc/sn_refresh.hpp).  Nothing here needs a GPU, and nothing of tests/sn_cases.py is modified.

Cholesky cases (`cholesky_values`): every stored entry (i, j) times ONE factor f(i, j) = f(j, i) in [0.7, 1.3] per unordered index
pair, so the values stay exactly symmetric; then the diagonal raised to 1.05 sum_j |a_ij| + 1e-3 a_ii wherever it is not above
1.05 sum_j |a_ij|.  The diagonal is positive and every row strictly dominant, so the matrix is symmetric positive definite
(Gershgorin).  tests/refresh_cases.new_values draws an independent factor per ENTRY: its values are not symmetric and must not be
handed to a Cholesky factor.

L U cases (`lu_values`): sn_cases._column_dominant with another seed on the case's own matrix -- its pattern is already the
symmetrised one, so the pattern stays; strictly column dominant, hence no row exchange (sn_cases' module docstring).  The
row-exchanging cases (sn_cases.EXCHANGING) get such values too: their refresh goes from a pivot order that exchanges rows to the
identity and back.

`pivoting_benign`: standard-normal values off the diagonal of the pattern of sn_cases.pivoting_matrix(), the diagonal 1 + the
column's sum of moduli: the benign partner of the matrix that needs refinement by design.  `pivoting_like(scale)`: that matrix's
construction with another scale of every third diagonal entry (scale = 1e-6 is pivoting_matrix() itself).

`not_positive_definite`: cholesky_values with ONE diagonal entry negated: symmetric, and e_i^T A e_i < 0."""
import functools

import numpy as np
import scipy.sparse as sp

from tests import refresh_cases as rc
from tests import sn_cases as sc

CHOLESKY = tuple(n for n in sc.NAMES if not sc._CASES[n][1])
LU = tuple(n for n in sc.NAMES if sc._CASES[n][1])
LU_SEED = {"lu13": 129, "lu17": 131, "lx13": 137, "lx17": 141, "lx21": 143}   # (sn_cases: 29, 31; 37, 41, 43)
HANDOVER_SCALE = 1e-11                                                  # pivoting_like(HANDOVER_SCALE): see test_gpu_sn_refresh.py, test 5


def _sorted(M):
    M = sp.csr_matrix(M)
    if not M.has_sorted_indices:
        M = M.sorted_indices()
    return M


def _rows(M):
    return np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))


def pair_factors(M, seed):
    """one factor in [0.7, 1.3] per unordered index pair of the stored entries of M (symmetric pattern), in M's entry order"""
    M = _sorted(M)
    rows, cols = _rows(M), M.indices.astype(np.int64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    key = lo * M.shape[0] + hi
    pairs, inverse = np.unique(key, return_inverse=True)
    return np.random.default_rng(seed).uniform(0.7, 1.3, len(pairs))[inverse]


def cholesky_values(M, seed):
    M = _sorted(M)
    N = rc.with_data(M, M.data * pair_factors(M, seed))
    rows = _rows(N)
    dg = N.indices == rows
    assert int(dg.sum()) == N.shape[0], "every row stores its diagonal"
    off = np.bincount(rows[~dg], weights=np.abs(N.data[~dg]), minlength=N.shape[0])
    d = N.data[dg]
    assert np.all(d > 0)
    data = N.data.copy()
    data[dg] = np.where(d <= 1.05 * off, 1.05 * off + 1e-3 * d, d)
    return rc.with_data(M, data)


def is_symmetric(M):
    """exactly, value by value (stored zeros included)"""
    M = _sorted(M)
    T = _sorted(sp.csr_matrix(M.T))
    return rc.same_pattern(M, T) and np.array_equal(M.data, T.data)


def symmetric_pattern(M):
    M = _sorted(M)
    P = sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
    return rc.same_pattern(P, _sorted(sp.csr_matrix(P.T)))


def lu_values(name):
    c = sc.case(name)
    assert c.general
    A, _ = sc._column_dominant((c.M, c.block_ptr), LU_SEED[name])
    return _sorted(A)


def _column_dominant_on(M, seed):
    """standard-normal values at the stored off-diagonal entries of M, the diagonal 1 + the column's sum of moduli: M's own pattern"""
    M = _sorted(M)
    rows = _rows(M)
    dg = M.indices == rows
    assert int(dg.sum()) == M.shape[0]
    data = np.random.default_rng(seed).standard_normal(M.nnz)
    data[dg] = 0.0
    col = np.bincount(M.indices, weights=np.abs(data), minlength=M.shape[0])
    data[dg] = 1.0 + col[M.indices[dg]]
    return rc.with_data(M, data)


@functools.lru_cache(maxsize=None)
def pivoting():
    M, bp = sc.pivoting_matrix()
    return _sorted(M), bp


@functools.lru_cache(maxsize=None)
def pivoting_benign(seed=41):
    return _column_dominant_on(pivoting()[0], seed)


def pivoting_like(scale):
    """sn_cases.pivoting_matrix() with every third diagonal entry times `scale` instead of 1e-6 (the same random factors)"""
    M = pivoting()[0]
    d = M.diagonal()
    d[::3] *= scale / 1e-6
    N = M.copy()                                                         # (sp.csr_matrix(M) would share the cached matrix's data)
    N.setdiag(d)
    N = _sorted(N)
    assert rc.same_pattern(M, N)
    return N


def not_positive_definite(M2, row=None):
    """M2 with the diagonal entry of `row` (default: the middle row) negated"""
    M2 = _sorted(M2)
    i = M2.shape[0] // 2 if row is None else row
    k = M2.indptr[i] + int(np.searchsorted(M2.indices[M2.indptr[i]:M2.indptr[i + 1]], i))
    assert M2.indices[k] == i and M2.data[k] > 0
    data = M2.data.copy()
    data[k] = -data[k]
    return rc.with_data(M2, data), i


@functools.lru_cache(maxsize=None)
def new_matrix(name, seed=7):
    """the second matrix of a case of sn_cases: Cholesky or L U values by the case's kind"""
    c = sc.case(name)
    return lu_values(name) if c.general else cholesky_values(c.M, seed + sc.NAMES.index(name))
