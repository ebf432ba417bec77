"""Inputs of the kept GenEO eigensolver's tests (tests/test_geneo_refresh_cases_cpu.py, tests/test_gpu_geneo_refresh.py).

The base problem is the islands problem of tests/test_gpu_geneo.py: StructuredPoisson 25^3 split 2 x 2 x 2, islands_kappa(contrast 1e4,
period 6, width 2), overlap 2, distance POU, Neumann matrices, nev = 4, tolerance 1e-5.  The new values: the same grid with
kappa * default_rng(7).uniform(0.7, 1.3, kappa.shape) -- every cell's coefficient changed by up to 30 %, the patterns untouched.

Beside it three built pencil inputs for the pencil assembly and its value refresh (pencil_cases): patterns that are strict subsets of
one another either way, a Dirichlet mask on rows that only B has entries in, and a row of more than 64 pencil entries beside rows of 1.

Everything is computed once per process and handed out as is: callers must not write into what they get."""
import functools

import numpy as np
import scipy.sparse as sp

N = (25, 25, 25)
SPLIT = (2, 2, 2)
NEV = 4
TOL = 1e-5
SHIFT = 1e-3
THRESHOLD = {"nev": 4, "threshold": 0.5}          # the parameters of test_geneo_threshold_mode_matches_oracle: one doubling, nev_max = 8


def _sorted_csr(M):
    M = sp.csr_matrix(M)
    return M if M.has_sorted_indices else M.sorted_indices()


@functools.lru_cache(maxsize=None)
def kappa(which):
    from dune_ddm_amd import synth
    k = synth.islands_kappa(tuple(n - 1 for n in N), contrast=1e4, period=6, width=2)
    if which == "new":
        k = k * np.random.default_rng(7).uniform(0.7, 1.3, k.shape)
    return k


@functools.lru_cache(maxsize=None)
def decomposition(which):
    """which: "old" or "new" """
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    return build_structured(synth.StructuredPoisson(N, SPLIT, kappa(which)), overlap=2, pou_type="distance", neumann=True)


def neumann_values(which):
    """({sub id: data of A_neu}, {sub id: data of B_neu}) in CSR order with sorted column indices"""
    dec = decomposition(which)
    return ({sd.id: _sorted_csr(sd.A_neu).data for sd in dec.subs}, {sd.id: _sorted_csr(sd.B_neu).data for sd in dec.subs})


def rank_values(which):
    """(data of the rank-local A, of A_dir) of a one-rank run, in CSR order with sorted column indices"""
    from dune_ddm_amd.problem import RankLocal
    rl = RankLocal(decomposition(which), 0, 1)
    return _sorted_csr(rl.A).data, _sorted_csr(rl.A_dir).data


@functools.lru_cache(maxsize=None)
def oracle(which, threshold=False):
    """{sub id: (vectors with the Dirichlet entries zeroed, eigenvalues)} from the oracle's Spectra restatement"""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import geneo_oracle as go
    dec = decomposition(which)
    par = dict(THRESHOLD) if threshold else {"nev": NEV}
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(lambda sd: go.geneo_basis(sd.A_neu, sd.B_neu, sd.pou, dict(par)), dec.subs))
    out = {}
    for sd, (vecs, lam) in zip(dec.subs, res):
        ov = np.array(vecs)
        ov[:, sd.dirichlet_ovlp > 0] = 0.0
        out[sd.id] = (ov, np.asarray(lam))
    return out


def block_pencil_input(which):
    """(A, B, pou, dirichlet) of the whole rank: block-diagonal Neumann matrices as the eigensolver gets them"""
    from dune_ddm_amd.problem import RankLocal, _block_diag
    dec = decomposition(which)
    rl = RankLocal(dec, 0, 1)
    A = sp.csr_matrix(_block_diag([sd.A_neu for sd in rl.subs]))
    B = sp.csr_matrix(_block_diag([sd.B_neu for sd in rl.subs]))
    return A, B, np.asarray(rl.pou, dtype=np.float64), np.asarray(rl.dirichlet_ovlp, dtype=np.uint8)


def _random_values(M, rng):
    M = _sorted_csr(M).copy()
    M.data = rng.uniform(-2.0, 2.0, M.nnz)
    return M


def _pattern(n, rows_cols):
    r, c = zip(*rows_cols)
    M = sp.csr_matrix((np.ones(len(r)), (np.array(r), np.array(c))), shape=(n, n))
    M.sum_duplicates()
    return _sorted_csr(M)


@functools.lru_cache(maxsize=None)
def pencil_cases():
    """name -> (A_old, B_old, A_new, B_new, pou, dirichlet or None): square scipy CSR matrices with sorted indices, new = same pattern,
    other values.  Neither matrix needs the diagonal; the pencil entry absent in one of them takes 0 from it."""
    rng = np.random.default_rng(11)
    cases = {}
    n = 40
    tri = [(i, j) for i in range(n) for j in (i - 1, i, i + 1) if 0 <= j < n]
    wide = tri + [(i, j) for i in range(n) for j in (i - 7, i + 5) if 0 <= j < n]
    no_diag = [(i, j) for (i, j) in tri if i != j]
    pou = rng.uniform(0.0, 1.0, n)
    pou[::9] = 0.0
    for name, pa, pb in (("B_inside_A", wide, no_diag), ("A_inside_B", no_diag, wide)):
        Pa, Pb = _pattern(n, pa), _pattern(n, pb)
        cases[name] = (_random_values(Pa, rng), _random_values(Pb, rng), _random_values(Pa, rng), _random_values(Pb, rng), pou, None)
    # Dirichlet rows whose entries exist only in B: rows 3, 17 and 30 are empty in A
    dirrows = (3, 17, 30)
    pa = [(i, j) for (i, j) in tri if i not in dirrows]
    Pa, Pb = _pattern(n, pa), _pattern(n, wide)
    dm = np.zeros(n, dtype=np.uint8)
    dm[list(dirrows)] = 1
    dm[8] = 1                                            # and one that both have
    cases["dirichlet_rows_only_in_B"] = (_random_values(Pa, rng), _random_values(Pb, rng), _random_values(Pa, rng), _random_values(Pb, rng), pou, dm)
    # a row of 150 pencil entries (A has the even columns and B every third: 100 + 67 - 17 shared), rows of one entry beside it
    n2 = 200
    pa = [(i, i) for i in range(n2) if i % 2] + [(100, j) for j in range(0, n2, 2)]
    pb = [(i, i) for i in range(n2) if not i % 2 and i != 100] + [(100, j) for j in range(0, n2, 3)]
    Pa, Pb = _pattern(n2, pa), _pattern(n2, pb)
    pou2 = rng.uniform(0.1, 1.0, n2)
    dm2 = np.zeros(n2, dtype=np.uint8)
    dm2[[6, 51]] = 1
    cases["long_row"] = (_random_values(Pa, rng), _random_values(Pb, rng), _random_values(Pa, rng), _random_values(Pb, rng), pou2, dm2)
    return cases


def pencil_numpy(A, B, pou, dirichlet, sigma):
    """The pencil in numpy, entry by entry in the operation order of the library: vc = 0 if row or column is Dirichlet, else
    (b * pou_i) * pou_c; A~ = a + sigma * vc; an entry absent in A or B contributes 0.  Returns (rowptr, col, val_At, val_C)."""
    A, B = _sorted_csr(A), _sorted_csr(B)
    n = A.shape[0]
    rp, ci, vt, vc_ = [0], [], [], []
    for i in range(n):
        ra = dict(zip(A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]))
        rb = dict(zip(B.indices[B.indptr[i]:B.indptr[i + 1]], B.data[B.indptr[i]:B.indptr[i + 1]]))
        for c in sorted(set(ra) | set(rb)):
            a = np.float64(ra.get(c, 0.0))
            vc = np.float64(0.0)
            if c in rb:
                masked = dirichlet is not None and (dirichlet[i] or dirichlet[c])
                vc = np.float64(0.0) if masked else (np.float64(rb[c]) * np.float64(pou[i])) * np.float64(pou[c])
            ci.append(c)
            vc_.append(vc)
            vt.append(a + np.float64(sigma) * vc)
        rp.append(len(ci))
    return np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(vt, dtype=np.float64), np.array(vc_, dtype=np.float64)
