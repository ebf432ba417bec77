"""CPU checks of block GMRES (ddm_bgmres_solve_multi and its test exports; no GPU needed): the ctypes prototypes and header text, the
argument checks that fail before any device work, TwoLevelSchwarz.solve_block_gmres, the host factor of a block's Gram matrix
(ddm_dense_bgmres_factor_host) against an extended-precision eigen-solve, and the numpy restatement of the algorithm
(tests/bgmres_reference.py) that the GPU tests compare the device driver with: at m = 1 it takes the iterations of flexible GMRES, at
m = 8 with a long cycle every column needs fewer block iterations than its independent run, degenerate and exhausting blocks are safe,
and its history moves far less than the GPU tests' rule allows when only the order of the additions in the scalar products changes."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from tests.test_bcg_cpu import random_columns
from tests.test_fgmres_cpu import CONFIGS, problem

REDUCTION, MAXIT = 1e-10, 200
RANK_TOL = 1e-12
KEYS = ("poisson_rm", "dg_umfpack")
# errors of the numpy factor (tests/bgmres_reference.py::factor) against the extended-precision eigen-solve on the seven matrices of
# test_factor, in the scaled metric of that test: S^T S 2.2e-15 at most, C C^T 2.5e-15 at most, C^T G C - I 2.6e-15 at most (all three
# on the duplicated column).  4 x the largest, rounded up.  (The library: 1.9e-15, 2.8e-15 and 4.4e-15 at most, at p = 32.)
FACTOR_TOL = 1.2e-14
# max_k |h_k - h_k^FGMRES| / h_k^FGMRES of the restatement at m = 1 against tests/fgmres_reference.py, (problem, restart) -> measured:
# the two differ in the orthogonalisation (block classical Gram-Schmidt twice against modified Gram-Schmidt) and in the last row of
# every cycle, which block GMRES recomputes; a long cycle lets modified Gram-Schmidt drift further.  4 x, rounded up.
FGMRES_HISTORY_MEASURED = {("poisson_rm", 6): 9.7e-11, ("poisson_rm", 50): 2.1e-6, ("dg_umfpack", 6): 8.6e-12, ("dg_umfpack", 50): 3.4e-8}
FGMRES_HISTORY_TOL = {("poisson_rm", 6): 4e-10, ("poisson_rm", 50): 9e-6, ("dg_umfpack", 6): 4e-11, ("dg_umfpack", 50): 1.4e-7}
# max over the cycles and running columns of |monitored - recomputed| / def0 on the restatement: 5.6e-17 (poisson_rm) and 7.1e-16
# (dg_umfpack) at m = 8, 5.8e-17 and 4.9e-16 on the degenerate block (restart 6 and 50).  4 x the largest, rounded up.
TRUE_GAP_TOL = 3e-15
SIX = ("cgsolver", "restartedgmressolver", "restartedflexiblegmressolver", "restartedfcgsolver", "completefcgsolver", "bicgstabsolver")
NAMES = ("ddm_bgmres_solve_multi", "ddm_bgmres_project_multi", "ddm_bgmres_combine_multi", "ddm_bgmres_combine_gram_multi", "ddm_dense_bgmres_factor_host")


def test_bgmres_prototypes(ddm):
    """the five new symbols are exported with the documented signatures, declared in the header and wrapped; the header states the
    algorithm; the default rank_tol of the wrapper is the header's"""
    lib = ddm.load_library()
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    R = ctypes.POINTER(ddm.SolveResult)
    assert ddm.SYMBOLS["ddm_bgmres_solve_multi"] == (I, [P, P, P, I, P, P, D, I, I, D, P, P, R])
    assert ddm.SYMBOLS["ddm_bgmres_project_multi"] == (I, [P, P, I, I, P, P, P])
    assert ddm.SYMBOLS["ddm_bgmres_combine_multi"] == (I, [P, P, I, I, I, I, P, P, P])
    assert ddm.SYMBOLS["ddm_bgmres_combine_gram_multi"] == (I, [P, P, I, I, P, P, P, P])
    assert ddm.SYMBOLS["ddm_dense_bgmres_factor_host"] == (I, [I, P, P, D, P, P, P])
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ddm_hip.h")).read()
    for name in NAMES:
        assert getattr(lib, name) is not None
        assert "int " + name + "(" in header, name
    for name in ("bgmres_solve_multi", "bgmres_project_multi", "bgmres_combine_multi", "bgmres_combine_gram_multi", "dense_bgmres_factor_host"):
        assert callable(getattr(ddm, name)), name
    assert "#define DDM_BGMRES_RANK_TOL_DEFAULT 1e-12" in header and ddm.BGMRES_RANK_TOL == RANK_TOL
    for phrase in ("block GMRES", "Cycle start (deflation)", "BEFORE the orthogonalisation", "width_hist_host", "stayed passed", "the space is exhausted"):
        assert phrase in header, phrase


@pytest.mark.parametrize("nrhs, maxit, restart, rank_tol", [(4, 10, 5, 1e-12), (0, 10, 5, 1e-12), (33, 10, 5, 1e-12), (4, -1, 5, 1e-12), (4, 10, 0, 1e-12),
                                                            (4, 10, 5, 0.0), (4, 10, 5, 1.0)])
def test_bgmres_rejects_bad_arguments_without_a_device(ddm, nrhs, maxit, restart, rank_tol):
    """null handles and a null X with otherwise valid numbers, nrhs 0 and 33, maxit -1, restart 0, rank_tol 0 and 1: DDM_EINVAL naming
    the function, from the driver and from the three kernel exports"""
    lib = ddm.load_library()
    res = (ddm.SolveResult * 33)()
    lib.ddm_cg_solve_multi(None, None, None, 4, None, None, 1e-10, 10, None, res)   # (leaves another function's name in the error text)
    assert lib.ddm_bgmres_solve_multi(None, None, None, nrhs, None, None, 1e-10, maxit, restart, rank_tol, None, None, res) == ddm.DDM_EINVAL
    assert "ddm_bgmres_solve_multi" in lib.ddm_last_error(None).decode()
    assert lib.ddm_bgmres_project_multi(None, None, nrhs, 1, None, None, None) == ddm.DDM_EINVAL
    assert "ddm_bgmres_project_multi" in lib.ddm_last_error(None).decode()
    assert lib.ddm_bgmres_combine_multi(None, None, 0, nrhs, nrhs, 1, None, None, None) == ddm.DDM_EINVAL
    assert "ddm_bgmres_combine_multi" in lib.ddm_last_error(None).decode()
    assert lib.ddm_bgmres_combine_gram_multi(None, None, nrhs, 1, None, None, None, None) == ddm.DDM_EINVAL
    assert "ddm_bgmres_combine_gram_multi" in lib.ddm_last_error(None).decode()


def test_factor_rejects_bad_arguments(ddm):
    lib = ddm.load_library()
    G, S, C = np.eye(2), np.zeros((2, 2)), np.zeros((2, 2))
    rank = ctypes.c_int(0)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    rk = ctypes.byref(rank)
    for args in [(0, hp(G), None, 1e-12, hp(S), hp(C), rk), (2, None, None, 1e-12, hp(S), hp(C), rk), (2, hp(G), None, 0.0, hp(S), hp(C), rk),
                 (2, hp(G), None, 1.0, hp(S), hp(C), rk), (2, hp(G), None, 1e-12, hp(S), hp(S), rk), (2, hp(G), None, 1e-12, hp(G), hp(C), rk),
                 (2, hp(G), None, 1e-12, hp(S), hp(C), None)]:
        assert lib.ddm_dense_bgmres_factor_host(*args) == ddm.DDM_EINVAL
        assert "ddm_dense_bgmres_factor_host" in lib.ddm_last_error(None).decode()
    G[0, 1] = np.nan
    assert lib.ddm_dense_bgmres_factor_host(2, hp(G), None, 1e-12, hp(S), hp(C), rk) == ddm.DDM_ENUMERIC


def test_solve_block_gmres_exists_and_solver_tuples_are_unchanged(ddm):
    """solve_block_gmres is a method of its own: no name was added to SOLVERS / SOLVERS_MULTI and solve_block keeps its signature; on an
    object without a device it fails on the first attribute it needs"""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    assert TwoLevelSchwarz.SOLVERS == SIX and TwoLevelSchwarz.SOLVERS_MULTI == SIX[:5]
    tl = object.__new__(TwoLevelSchwarz)
    with pytest.raises(AttributeError):
        tl.solve_block_gmres(np.zeros((4, 2)))
    sig = inspect.signature(TwoLevelSchwarz.solve_block_gmres)
    assert list(sig.parameters)[1:] == ["B", "reduction", "maxit", "restart", "history", "X0", "rank_tol"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["reduction"], d["maxit"], d["restart"], d["history"], d["X0"], d["rank_tol"]) == (1e-10, 1000, 100, True, None, RANK_TOL)
    assert list(inspect.signature(TwoLevelSchwarz.solve_block).parameters)[1:] == ["B", "reduction", "maxit", "history", "X0", "rank_tol"]


# ---- the host factor ---------------------------------------------------------------------------------------------------------------------
def _eig_longdouble(A):
    """cyclic Jacobi eigen-solver in numpy.longdouble (the one of tests/test_bcg_cpu.py): eigenvalues, eigenvectors as columns"""
    L = np.longdouble
    A = np.array(A, dtype=L)
    m = A.shape[0]
    V = np.eye(m, dtype=L)
    for _ in range(60):
        if np.sqrt(np.sum(np.tril(A, -1) ** 2)) <= np.finfo(L).eps * 1e-2 * np.sqrt(np.sum(A * A)):
            break
        for p in range(m - 1):
            for q in range(p + 1, m):
                if A[p, q] == 0:
                    continue
                theta = (A[q, q] - A[p, p]) / (2 * A[p, q])
                t = L(1) if theta == 0 else np.sign(theta) / (abs(theta) + np.hypot(theta, L(1)))
                c = 1 / np.hypot(t, L(1))
                s = t * c
                rp, rq = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * rp - s * rq, s * rp + c * rq
                cp, cq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * cp - s * cq, s * cp + c * cq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
    return np.diag(A).copy(), V


def _factor_cases():
    rng = np.random.default_rng(11)
    W8 = rng.standard_normal((40, 8))
    dup = W8.copy()
    dup[:, 5] = dup[:, 2]
    zero = W8.copy()
    zero[:, 3] = 0.0
    spread = W8 * 10.0 ** np.linspace(-10.0, 0.0, 8)[None, :]        # diagonal entries of the Gram matrix spread over 1e-20 .. 1
    noise = W8.copy()
    noise[:, 6] *= 1e-15                                             # what the orthogonalisation leaves of a column of size one
    Gn = noise.T @ noise
    scale2 = np.diag(Gn).copy()
    scale2[6] = float(W8[:, 6] @ W8[:, 6])
    W32 = rng.standard_normal((100, 32))
    return [("full", W8.T @ W8, None, 8), ("duplicate", dup.T @ dup, None, 7), ("zero", zero.T @ zero, None, 7), ("spread", spread.T @ spread, None, 8),
            ("p1", np.array([[3.5]]), None, 1), ("p32", W32.T @ W32, None, 32), ("noise", Gn, scale2, 7)]


@pytest.mark.parametrize("case", range(7))
def test_factor(ddm, case):
    """ddm_dense_bgmres_factor_host on a full-rank 8 x 8 Gram matrix (rank 8), the same with a duplicated column (7), with a zero column
    (7), with diagonal entries spread over 1e-20 .. 1 (8: the scaling must keep every direction), p = 1, p = 32, and a column of
    rounding noise judged against its norm BEFORE the orthogonalisation (7: the rank must drop; scaled by its own diagonal the same
    matrix has rank 8, which is asserted too).  Against an extended-precision eigen-solve of the scaled matrix: S^T S against the kept
    part of G and C C^T against its pseudo-inverse, in the scaled metric max |E_ij| / (d_i d_j) resp. max |E_ij| d_i d_j relative to
    the largest entry, and (W C)^T (W C) = C^T G C = I evaluated in extended precision.  The bound is the error of numpy's factor
    (tests/bgmres_reference.py::factor) against the same reference (printed), x 4, rounded up: FACTOR_TOL."""
    from tests.bgmres_reference import factor
    name, G, scale2, want_rank = _factor_cases()[case]
    L = np.longdouble
    d = np.sqrt(np.abs(np.diag(G) if scale2 is None else scale2))
    d[d == 0.0] = 1.0
    dd = d[:, None] * d[None, :]
    lam, U = _eig_longdouble(np.asarray(G, dtype=L) / dd)
    keep = lam > RANK_TOL * lam.max()
    kept = (U[:, keep] * lam[keep]) @ U[:, keep].T        # scaled metric
    pinv = (U[:, keep] / lam[keep]) @ U[:, keep].T
    assert int(keep.sum()) == want_rank

    def errors(S, C):
        S, C = S.astype(L), C.astype(L)
        e_s = float(np.max(np.abs((S.T @ S) / dd - kept)) / np.max(np.abs(kept)))
        e_c = float(np.max(np.abs((C @ C.T) * dd - pinv)) / np.max(np.abs(pinv)))
        e_i = float(np.max(np.abs(C.T @ np.asarray(G, dtype=L) @ C - np.eye(C.shape[1]))))
        return e_s, e_c, e_i
    S_np, C_np, rank_np = factor(G, scale2, RANK_TOL)
    S, C, rank = ddm.dense_bgmres_factor_host(G, scale2, RANK_TOL)
    err_np, err = errors(S_np, C_np), errors(S, C)
    print(name, "rank", rank, "numpy vs extended", err_np, "library vs extended", err)
    assert rank == rank_np == want_rank and S.shape == (rank, G.shape[0]) and C.shape == (G.shape[0], rank)
    assert max(err_np) <= FACTOR_TOL / 4
    assert max(err) <= FACTOR_TOL
    if name == "noise":
        assert ddm.dense_bgmres_factor_host(G, None, RANK_TOL)[2] == 8      # what the earlier scale is for
    if name == "spread":
        assert np.linalg.matrix_rank(G, hermitian=True) < 8                 # what the scaling is for


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
_DECS = {}


def dec_of(ddm, key):
    if key not in _DECS:
        _DECS[key] = problem(ddm, CONFIGS[key][0])
    return _DECS[key]


def rhs(dec):
    return [sd.b.copy() for sd in dec.subs]


def block_m8(dec):
    """column 0 is the problem's b, seven consistent random columns from default_rng(5)"""
    return [rhs(dec)] + random_columns(dec, 7, 5)


def block_degenerate(dec):
    """b; a random column; 2 b; zero; another random column (default_rng(6))"""
    r1, r2 = random_columns(dec, 2, 6)
    b = rhs(dec)
    return [b, r1, [2.0 * v for v in b], [np.zeros(sd.n_o) for sd in dec.subs], r2]


def block_exhausting(dec, okw):
    """b and A M^-1 b: the second column lies in the image of the first cycle's first block"""
    from tests.oracle_bridge import oracle_objects
    op, sp_, prec, sch, gal = oracle_objects(dec, **okw)
    b = rhs(dec)
    z, w = [np.zeros_like(v) for v in b], [np.zeros_like(v) for v in b]
    prec.apply(z, b)
    op.apply(z, w)
    return [b, w]


def true_reductions(dec, okw, Bcols, X):
    from tests.oracle_bridge import oracle_objects
    op, sp_, prec, sch, gal = oracle_objects(dec, **okw)
    out = []
    for col, x in zip(Bcols, X):
        bb = [np.array(v, dtype=float) for v in col]
        n0 = sp_.norm(bb)
        op.applyscaleadd(-1.0, x, bb)
        out.append(sp_.norm(bb) / n0 if n0 > 0.0 else 0.0)
    return np.array(out)


def _independent(dec, okw, col, restart):
    from tests import fgmres_reference as fr
    it, conv, hist, red, x = fr.reference_solve(dec, reduction=REDUCTION, maxit=MAXIT, restart=restart, b=col, **okw)
    assert conv
    return it, hist


@pytest.mark.parametrize("key, restart, want", [("poisson_rm", 6, 13), ("poisson_rm", 50, 12), ("dg_umfpack", 6, 22), ("dg_umfpack", 50, 19)])
def test_one_column_is_flexible_gmres(ddm, key, restart, want):
    """m = 1: the block of width 1 is right-preconditioned restarted GMRES; with a fixed preconditioner that is what
    tests/fgmres_reference.py computes.  Equal iteration counts (13 / 12 and 22 / 19), width 1 throughout, and the history deviation
    under FGMRES_HISTORY_TOL (4 x the measured FGMRES_HISTORY_MEASURED)."""
    from tests.bgmres_reference import reference_solve
    dec, okw = dec_of(ddm, key), CONFIGS[key][1]
    its, conv, hist, widths, X = reference_solve(dec, [rhs(dec)], REDUCTION, MAXIT, restart, RANK_TOL, **okw)
    it_f, h_f = _independent(dec, okw, rhs(dec), restart)
    k = min(len(hist), len(h_f))
    dev = float(np.max(np.abs(hist[:k, 0] - h_f[:k]) / h_f[:k]))
    print(key, "restart", restart, "iterations", its, it_f, "max |h - h_FGMRES| / h_FGMRES", dev)
    assert conv == [True] and its == [it_f] == [want] and widths == [1] * want and len(hist) == len(h_f)
    assert dev <= FGMRES_HISTORY_TOL[key, restart]


@pytest.mark.parametrize("key", KEYS)
def test_eight_columns_need_fewer_iterations(ddm, key):
    """m = 8, restart 50: every column passes no later than its independent flexible GMRES run, the slowest block column strictly
    earlier than the fastest independent one (measured 10 against 11-12 on poisson_rm, 13 against 19-20 on dg_umfpack), the width is 8
    throughout; the recomputed true reduction is below 1e-10 and the monitored defect agrees with the recomputed one at every cycle end
    within TRUE_GAP_TOL."""
    from tests.bgmres_reference import reference_solve
    dec, okw = dec_of(ddm, key), CONFIGS[key][1]
    B = block_m8(dec)
    gaps = []
    its, conv, hist, widths, X = reference_solve(dec, B, REDUCTION, MAXIT, 50, RANK_TOL, gaps=gaps, **okw)
    ind = [_independent(dec, okw, col, 50)[0] for col in B]
    true = true_reductions(dec, okw, B, X)
    print(key, "block", its, "independent", ind, "gap", max(gaps), "true", float(true.max()))
    assert all(conv) and all(i <= j for i, j in zip(its, ind)) and max(its) < min(ind)
    assert widths == [8] * max(its) and hist.shape == (max(its) + 1, 8)
    assert np.all(true < REDUCTION) and max(gaps) <= TRUE_GAP_TOL
    assert float(np.max(np.abs(hist[-1] / hist[0] - true))) <= TRUE_GAP_TOL


@pytest.mark.parametrize("key", KEYS)
def test_degenerate_block(ddm, key):
    """b, random, 2 b, zero, random at restart 6: every cycle has width <= 3; the zero column has 0 iterations, its x stays zero and its
    history is zero; every non-zero column converges to a true reduction < 1e-10; x_2 = 2 x_0 within 1e-8 of the largest entry; the
    monitored and the recomputed defect agree within TRUE_GAP_TOL."""
    from tests.bgmres_reference import reference_solve
    dec, okw = dec_of(ddm, key), CONFIGS[key][1]
    B = block_degenerate(dec)
    gaps = []
    its, conv, hist, widths, X = reference_solve(dec, B, REDUCTION, MAXIT, 6, RANK_TOL, gaps=gaps, **okw)
    true = true_reductions(dec, okw, B, X)
    nz = [0, 1, 2, 4]
    x0, x2 = np.concatenate(X[0]), np.concatenate(X[2])
    print(key, "iterations", its, "widths", widths, "gap", max(gaps), "max |x2 - 2 x0| / max |x0|", float(np.max(np.abs(x2 - 2.0 * x0)) / np.max(np.abs(x0))))
    assert max(widths) <= 3 and len(widths) == len(hist) - 1
    assert its[3] == 0 and conv[3] and not np.any(np.concatenate(X[3])) and not np.any(hist[:, 3])
    assert all(conv) and np.all(true[nz] < REDUCTION) and max(gaps) <= TRUE_GAP_TOL
    assert float(np.max(np.abs(x2 - 2.0 * x0))) <= 1e-8 * float(np.max(np.abs(x0)))


@pytest.mark.parametrize("key", KEYS)
def test_exhausting_block(ddm, key):
    """[b, A M^-1 b] at restart 6: the first cycle is ONE step of width 2 (the image of its first block holds the second column, so the
    new block has rank 1 and the space is exhausted); column 1 passes at iteration 1 and stays passed; every later cycle has width 1;
    both columns converge."""
    from tests.bgmres_reference import reference_solve
    dec, okw = dec_of(ddm, key), CONFIGS[key][1]
    B = block_exhausting(dec, okw)
    its, conv, hist, widths, X = reference_solve(dec, B, REDUCTION, MAXIT, 6, RANK_TOL, **okw)
    true = true_reductions(dec, okw, B, X)
    print(key, "iterations", its, "widths", widths)
    assert widths[0] == 2 and widths[1:] == [1] * (len(widths) - 1) and len(widths) > 1
    assert its[1] == 1 and all(conv) and its[0] == len(widths) and np.all(true < REDUCTION)
    assert np.all(hist[1:, 1] == hist[1, 1]) and hist[1, 1] < REDUCTION * hist[0, 1]      # a column that does not run repeats its value


def test_rank_tol_default(ddm):
    """The default rank_tol on the degenerate block of poisson_rm at restart 6, by the criterion 'recomputed against monitored
    reduction'.  Every value from 1e-16 to 1e-6 gives the same iteration counts (13, 11, 13, 0, 11) and the same gap (5.8e-17, under
    TRUE_GAP_TOL): the exact duplicate 2 b has a relative eigenvalue of rounding size and is dropped by all of them, so the first two
    cycles have width 3 throughout.  The values differ only in the last cycle, where b and 2 b alone still run and their defects, 1e-9
    of def0 by then, have drifted apart by rounding relative to def0: up to 1e-12 the drift counts as a second direction (width 2),
    from 1e-10 on it does not (width 1); neither costs an iteration.  1e-12 sits four decades above the smallest value tried and at
    m = 8 with independent columns it drops nothing (test_eight_columns_need_fewer_iterations)."""
    from tests.bgmres_reference import reference_solve
    dec, okw = dec_of(ddm, "poisson_rm"), CONFIGS["poisson_rm"][1]
    B = block_degenerate(dec)
    runs = {}
    for tol in (1e-16, 1e-14, RANK_TOL, 1e-10, 1e-8, 1e-6):
        gaps = []
        its, conv, hist, widths, X = reference_solve(dec, B, REDUCTION, MAXIT, 6, tol, gaps=gaps, **okw)
        print("rank_tol", tol, "iterations", its, "widths", widths, "gap", max(gaps))
        runs[tol] = (its, widths, max(gaps))
        assert all(conv)
    for tol, (its, widths, gap) in runs.items():
        assert its == runs[RANK_TOL][0] == [13, 11, 13, 0, 11] and gap <= TRUE_GAP_TOL
        assert widths[:12] == [3] * 12 and len(widths) == 13
    assert [runs[t][1][12] for t in (1e-16, 1e-14, RANK_TOL)] == [2, 2, 2]
    assert [runs[t][1][12] for t in (1e-10, 1e-8, 1e-6)] == [1, 1, 1]


@pytest.mark.parametrize("key, name, restart", [(k, n, r) for k in KEYS for n, r in (("m1", 6), ("degenerate", 6), ("m8", 6), ("m8", 50))])
def test_summation_order_sensitivity(ddm, key, name, restart):
    """How far the restatement itself moves when nothing but the order of the additions in its scalar products changes (ascending,
    descending, pairwise: oracle/kernels.c orc_masked_dot_order), on the blocks of the GPU test.  The device sums in yet another order,
    so this is the envelope its deviation from the restatement is judged by: iteration counts and widths must not move, and the GPU
    test's history rule 1e-7 |r_k| + 1e-11 |r_0| (RTOL_HIST, ATOL_HIST of tests/test_gpu_multi_gmres.py) must be at least 4 x the largest
    deviation at EVERY iteration and column.  Measured smallest rule / deviation: 4.6e3 (poisson_rm, degenerate block) to 3.9e5
    (poisson_rm, m = 1); the largest relative deviation, 4.9e-4, is at a defect of 1e-11 def0 (poisson_rm, m = 8, restart 50)."""
    from oracle import apply_oracle as ao
    from tests.bgmres_reference import reference_solve
    from tests.test_gpu_multi_gmres import ATOL_HIST, RTOL_HIST
    dec, okw = dec_of(ddm, key), CONFIGS[key][1]
    B = {"m1": lambda: [rhs(dec)], "degenerate": lambda: block_degenerate(dec), "m8": lambda: block_m8(dec)}[name]()
    runs = {}
    try:
        for order in (0, 1, 2):
            ao.set_dot_order(order)
            runs[order] = reference_solve(dec, B, REDUCTION, MAXIT, restart, RANK_TOL, **okw)
    finally:
        ao.set_dot_order(0)
    its0, conv0, h0, widths0, X0 = runs[0]
    rule = RTOL_HIST * h0 + ATOL_HIST * h0[0]
    margin, worst = np.inf, 0.0
    for order in (1, 2):
        its, conv, h, widths, X = runs[order]
        assert its == its0 and widths == widths0 and all(conv)
        dev = np.abs(h - h0)
        live = h0[0] > 0.0                                              # (the zero column's history is all zero in every order)
        assert not np.any(dev[:, ~live])
        margin = min(margin, float(np.min(rule[:, live] / np.maximum(dev[:, live], 1e-300))))
        worst = max(worst, float(np.max(dev[:, live] / h0[:, live])))
    print(key, name, "restart", restart, "iterations", its0, "min rule / deviation", margin, "max relative deviation", worst)
    assert margin >= 4.0
