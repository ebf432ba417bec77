"""New matrix values in an unchanged pattern, shared by tests/test_refresh_cpu.py and tests/test_gpu_refresh.py.

`new_values(M, seed)`: every stored entry of M times an independent factor in [0.7, 1.3] (so the values are not symmetric), then the
diagonal raised where needed so that every row is strictly diagonally dominant: |a_ii| >= 1.05 sum_j |a_ij| + 1e-3 |a_ii| wherever
the perturbed row missed that.  A strictly row-dominant matrix has an ILU(0) without a vanishing pivot (Gaussian elimination keeps
row dominance, and dropping fill only removes off-diagonal mass).  `assert_dominant` is the check every test makes on the CPU.
Nothing here needs a GPU."""
import dataclasses

import numpy as np
import scipy.sparse as sp


def _rows(M):
    return np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))


def _raise_diagonal(M):
    """M (CSR, sorted indices, a stored diagonal in every row) with |a_ii| raised to 1.05 sum_j |a_ij| where it is not above that"""
    rows = _rows(M)
    dg = M.indices == rows
    assert int(dg.sum()) == M.shape[0], "every row stores its diagonal"
    off = np.bincount(rows[~dg], weights=np.abs(M.data[~dg]), minlength=M.shape[0])
    d = M.data[dg]
    need = np.abs(d) <= 1.05 * off
    sign = np.where(d < 0, -1.0, 1.0)
    d = np.where(need, sign * (1.05 * off + 1e-3 * np.abs(d)), d)
    data = M.data.copy()
    data[dg] = d
    return data


def with_data(M, data):
    """M's pattern (explicit zeros kept) with other values"""
    N = sp.csr_matrix((np.asarray(data, dtype=np.float64), M.indices.copy(), M.indptr.copy()), shape=M.shape)
    N.has_sorted_indices = True
    return N


def new_values(M, seed):
    M = sp.csr_matrix(M)
    assert M.has_sorted_indices
    f = np.random.default_rng(seed).uniform(0.7, 1.3, M.nnz)
    return with_data(M, _raise_diagonal(with_data(M, M.data * f)))


def assert_dominant(M):
    M = sp.csr_matrix(M)
    rows = _rows(M)
    dg = M.indices == rows
    off = np.bincount(rows[~dg], weights=np.abs(M.data[~dg]), minlength=M.shape[0])
    d = np.abs(M.data[dg])
    assert d.shape == off.shape and bool(np.all(d > off)), "a row is not strictly diagonally dominant"


def same_pattern(M, N):
    return M.shape == N.shape and np.array_equal(M.indptr, N.indptr) and np.array_equal(M.indices, N.indices)


def perturbed_decomposition(dec, seed):
    """`dec` with a changed coefficient: the entry (i, j) of every subdomain's A and A_dir times the factor f(global i, global j) in
    [0.7, 1.3] (one factor per pair of global unknowns, so the additive matrices, the overlapping matrices and their overlaps stay
    consistent with each other), then the diagonal rule of new_values on every matrix.  Everything else of `dec` is kept."""
    F = np.random.default_rng(seed).uniform(0.7, 1.3, (dec.nglobal, dec.nglobal))
    subs = []
    for sd in dec.subs:
        g = np.asarray(sd.glob, dtype=np.int64)
        out = {}
        for key in ("A", "A_dir"):
            M = sp.csr_matrix(getattr(sd, key))
            M.sort_indices()
            gi = g[:M.shape[0]]
            out[key] = with_data(M, _raise_diagonal(with_data(M, M.data * F[gi[_rows(M)], gi[M.indices]])))
        subs.append(dataclasses.replace(sd, **out))
    return dataclasses.replace(dec, subs=subs, meta=dict(dec.meta))
