"""CPU checks of block CG (ddm_bcg_solve_multi and its test exports; no GPU needed): the ctypes prototypes and header declarations, the
argument checks that fail before any device work, TwoLevelSchwarz.solve_block, the host pseudo-inverse of the coupling matrix
(ddm_dense_sym_pinv_host) against numpy and an extended-precision reference, and the numpy restatement of the algorithm
(tests/bcg_reference.py) that the GPU tests compare the device driver with: at m = 1 it is CG, at m = 8 every column needs fewer
iterations than CG on it, a degenerate block (duplicate and zero columns) is safe, and its history moves far less than the GPU tests'
rule allows when only the order of the additions in the scalar products changes."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_fcg_cpu import CONFIGS
from tests.test_fgmres_cpu import golden_poisson

OKW, TKW = CONFIGS["poisson_sa"]     # standard Schwarz, additive, POU coarse space: a symmetric positive definite preconditioner
REDUCTION, MAXIT = 1e-10, 200
RANK_TOL = 1e-12
# error of numpy.linalg.pinv against the extended-precision pseudo-inverse on the six matrices of test_pinv, in the Jacobi-scaled
# metric of that test: 8.1e-16, 8.9e-16, 9.6e-16, 8.9e-16, 0, 1.17e-15 (m = 32).  4 x the largest, rounded up.  (The library against
# numpy: 2.1e-15 at most; against the extended-precision reference: 1.5e-15 at most.)
PINV_TOL = 5e-15
# max_k |h_k - h_k^CG| / h_k^CG of the restatement at m = 1 against ao.cg_solve on the golden problem: 3.25e-12.  4 x, rounded up.
CG_HISTORY_TOL = 1.5e-11
# |reported reduction - recomputed ||b - A x|| / def0|: 4.7e-17 at m = 8, 4.5e-18 on the degenerate block.  4 x, rounded up.
TRUE_GAP_M8, TRUE_GAP_DEGENERATE = 2e-16, 2e-17
SIX = ("cgsolver", "restartedgmressolver", "restartedflexiblegmressolver", "restartedfcgsolver", "completefcgsolver", "bicgstabsolver")


def test_bcg_prototypes(ddm):
    """the five new symbols are exported (load_library resolves every entry of SYMBOLS) with the documented signatures, declared in the
    header and wrapped; the default rank_tol of the wrapper is the header's"""
    lib = ddm.load_library()
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    R = ctypes.POINTER(ddm.SolveResult)
    assert ddm.SYMBOLS["ddm_bcg_solve_multi"] == (I, [P, P, P, I, P, P, D, I, D, P, P, R])
    assert ddm.SYMBOLS["ddm_bcg_gram_multi"] == (I, [P, P, I, P, P, P, P])
    assert ddm.SYMBOLS["ddm_bcg_update_multi"] == (I, [P, P, I, P, P, P, P, P, P])
    assert ddm.SYMBOLS["ddm_bcg_direction_multi"] == (I, [P, P, I, P, P, P])
    assert ddm.SYMBOLS["ddm_dense_sym_pinv_host"] == (I, [I, P, D, P, P])
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ddm_hip.h")).read()
    for name in ("ddm_bcg_solve_multi", "ddm_bcg_gram_multi", "ddm_bcg_update_multi", "ddm_bcg_direction_multi", "ddm_dense_sym_pinv_host"):
        assert getattr(lib, name) is not None
        assert "int " + name + "(" in header, name
    for name in ("bcg_solve_multi", "bcg_gram_multi", "bcg_update_multi", "bcg_direction_multi", "dense_sym_pinv_host"):
        assert callable(getattr(ddm, name)), name
    assert "#define DDM_BCG_RANK_TOL_DEFAULT 1e-12" in header and ddm.BCG_RANK_TOL == RANK_TOL


@pytest.mark.parametrize("nrhs, maxit, rank_tol", [(4, 10, 1e-12), (0, 10, 1e-12), (33, 10, 1e-12), (4, -1, 1e-12), (4, 10, 0.0), (4, 10, 1.0)])
def test_bcg_rejects_bad_arguments_without_a_device(ddm, nrhs, maxit, rank_tol):
    """null handles with otherwise valid numbers, nrhs 0 and 33, maxit -1, rank_tol 0 and 1: DDM_EINVAL naming the function, from the
    driver and from the three kernel exports"""
    lib = ddm.load_library()
    res = (ddm.SolveResult * 33)()
    lib.ddm_cg_solve_multi(None, None, None, 4, None, None, 1e-10, 10, None, res)   # (leaves another function's name in the error text)
    assert lib.ddm_bcg_solve_multi(None, None, None, nrhs, None, None, 1e-10, maxit, rank_tol, None, None, res) == ddm.DDM_EINVAL
    assert "ddm_bcg_solve_multi" in lib.ddm_last_error(None).decode()
    assert lib.ddm_bcg_gram_multi(None, None, nrhs, None, None, None, None) == ddm.DDM_EINVAL
    assert "ddm_bcg_gram_multi" in lib.ddm_last_error(None).decode()
    assert lib.ddm_bcg_update_multi(None, None, nrhs, None, None, None, None, None, None) == ddm.DDM_EINVAL
    assert "ddm_bcg_update_multi" in lib.ddm_last_error(None).decode()
    assert lib.ddm_bcg_direction_multi(None, None, nrhs, None, None, None) == ddm.DDM_EINVAL
    assert "ddm_bcg_direction_multi" in lib.ddm_last_error(None).decode()


def test_pinv_rejects_bad_arguments(ddm):
    lib = ddm.load_library()
    W = np.eye(2)
    out = np.zeros((2, 2))
    rank = ctypes.c_int(0)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    for args in [(0, hp(W), 1e-12, hp(out), ctypes.byref(rank)), (2, None, 1e-12, hp(out), ctypes.byref(rank)), (2, hp(W), 0.0, hp(out), ctypes.byref(rank)),
                 (2, hp(W), 1.0, hp(out), ctypes.byref(rank)), (2, hp(W), 1e-12, hp(W), ctypes.byref(rank)), (2, hp(W), 1e-12, hp(out), None)]:
        assert lib.ddm_dense_sym_pinv_host(*args) == ddm.DDM_EINVAL
        assert "ddm_dense_sym_pinv_host" in lib.ddm_last_error(None).decode()
    W[0, 1] = np.nan
    assert lib.ddm_dense_sym_pinv_host(2, hp(W), 1e-12, hp(out), ctypes.byref(rank)) == ddm.DDM_ENUMERIC


def test_solve_block_exists_and_solver_tuples_are_unchanged(ddm):
    """solve_block is a method of its own: no name was added to SOLVERS / SOLVERS_MULTI; on an object without a device it fails on the
    first attribute it needs"""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    assert TwoLevelSchwarz.SOLVERS == SIX and TwoLevelSchwarz.SOLVERS_MULTI == SIX[:5]
    tl = object.__new__(TwoLevelSchwarz)
    with pytest.raises(AttributeError):
        tl.solve_block(np.zeros((4, 2)))
    import inspect
    sig = inspect.signature(TwoLevelSchwarz.solve_block)
    assert list(sig.parameters)[1:] == ["B", "reduction", "maxit", "history", "X0", "rank_tol"]
    assert sig.parameters["rank_tol"].default == RANK_TOL and sig.parameters["reduction"].default == 1e-10 and sig.parameters["maxit"].default == 1000


# ---- the host pseudo-inverse ---------------------------------------------------------------------------------------------------------
def _jacobi_scale(W):
    d = np.sqrt(np.abs(np.diag(W)))
    d[d == 0.0] = 1.0
    return d


def _pinv_longdouble(W, tol):
    """extended-precision reference: cyclic Jacobi eigen-solver in numpy.longdouble on the Jacobi-scaled symmetrised matrix"""
    L = np.longdouble
    W = np.asarray(W, dtype=L)
    m = W.shape[0]
    d = _jacobi_scale(W)
    A = (W + W.T) / 2 / d[:, None] / d[None, :]
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
    lam = np.diag(A).copy()
    keep = lam > tol * lam.max()
    return (V[:, keep] / lam[keep]) @ V[:, keep].T / d[:, None] / d[None, :], int(keep.sum())


def _pinv_cases():
    rng = np.random.default_rng(11)

    def spd(m):
        A = rng.standard_normal((m, m))
        return A @ A.T + m * np.eye(m)
    S8 = spd(8)
    dup = S8.copy()
    dup[5, :] = dup[2, :]
    dup[:, 5] = dup[:, 2]
    dup[5, 5] = dup[2, 2]
    zero = S8.copy()
    zero[3, :] = 0.0
    zero[:, 3] = 0.0
    sc = 10.0 ** np.linspace(-10.0, 0.0, 8)                 # diagonal entries spread over 1e-20 .. 1
    return [("spd8", S8, 8), ("duplicate", dup, 7), ("zero", zero, 7), ("spread", S8 * sc[:, None] * sc[None, :], 8), ("m1", np.array([[3.5]]), 1),
            ("m32", spd(32), 32)]


@pytest.mark.parametrize("case", range(6))
def test_pinv(ddm, case):
    """ddm_dense_sym_pinv_host against numpy.linalg.pinv, with the returned rank: an SPD 8 x 8 matrix (rank 8), the same with a
    duplicated row and column (7), with a zero row and column (7), with diagonal entries spread over 1e-20 .. 1 (8: the Jacobi scaling
    must keep every direction; numpy.linalg.pinv on the UNSCALED matrix keeps 6 of them, so numpy runs on the scaled matrix here, as the
    contract says), m = 1 and m = 32.  Errors are measured in the Jacobi-scaled metric, max_ij |E_ij| d_i d_j / max_ij |P_ij| d_i d_j.
    The bound is numpy's own error against an extended-precision pseudo-inverse (printed), x 4, rounded up: PINV_TOL."""
    name, W, want_rank = _pinv_cases()[case]
    d = _jacobi_scale(W)
    dd = d[:, None] * d[None, :]
    ref, rank_ref = _pinv_longdouble(W, RANK_TOL)
    ref = np.asarray(ref, dtype=float)
    npv = np.linalg.pinv(0.5 * (W + W.T) / dd, rcond=RANK_TOL, hermitian=True) / dd
    mine, rank = ddm.dense_sym_pinv_host(W, RANK_TOL)
    top = np.max(np.abs(ref * dd))
    err_numpy = float(np.max(np.abs(npv - ref) * dd) / top)
    err_mine = float(np.max(np.abs(mine - ref) * dd) / top)
    dev = float(np.max(np.abs(mine - npv) * dd) / top)
    print(name, "rank", rank, "reference", rank_ref, "numpy vs extended", err_numpy, "library vs extended", err_mine, "library vs numpy", dev)
    assert rank == want_rank == rank_ref
    assert err_numpy <= PINV_TOL / 4
    assert dev <= PINV_TOL and err_mine <= PINV_TOL
    assert np.max(np.abs(mine - mine.T) * dd) / top <= PINV_TOL
    if name == "spread":
        assert np.linalg.matrix_rank(W, hermitian=True) < 8       # what the scaling is for


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dec(ddm):
    return golden_poisson(ddm)


def random_columns(dec, k, seed):
    """k consistent random columns (the same value on every holder of a DoF), per-rank lists"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        xg = rng.standard_normal(dec.nglobal)
        out.append([xg[sd.glob[:sd.n_o]].copy() for sd in dec.subs])
    return out


def block_m8(dec):
    """column 0 is the problem's b, seven consistent random columns from default_rng(5)"""
    return [[sd.b.copy() for sd in dec.subs]] + random_columns(dec, 7, 5)


def block_degenerate(dec):
    """b; a random column; 2 b; zero; another random column (default_rng(6))"""
    r1, r2 = random_columns(dec, 2, 6)
    b = [sd.b.copy() for sd in dec.subs]
    return [b, r1, [2.0 * v for v in b], [np.zeros(sd.n_o) for sd in dec.subs], r2]


def _oracle(dec):
    from tests.oracle_bridge import oracle_objects
    return oracle_objects(dec, **OKW)


def _cg(dec, col):
    from oracle import apply_oracle as ao
    op, sp_, prec, sch, gal = _oracle(dec)
    x = [np.zeros(sd.n_o) for sd in dec.subs]
    b = [np.array(v, dtype=float) for v in col]
    it, conv, hist = ao.cg_solve(op, sp_, prec, x, b, REDUCTION, MAXIT)
    return it, conv, np.asarray(hist, dtype=float)


def _true_reductions(dec, Bcols, X):
    op, sp_, prec, sch, gal = _oracle(dec)
    out = []
    for col, x in zip(Bcols, X):
        bb = [np.array(v, dtype=float) for v in col]
        n0 = sp_.norm(bb)
        op.applyscaleadd(-1.0, x, bb)
        out.append(sp_.norm(bb) / n0 if n0 > 0.0 else 0.0)
    return np.array(out)


def test_one_column_is_cg(dec):
    """m = 1: the coupling is the scalar <p, A p>; the restatement takes CG's 30 iterations on the golden problem and its history
    differs from ao.cg_solve's by 3.25e-12 relative at most (other groupings of the same products); asserted under CG_HISTORY_TOL."""
    from tests.bcg_reference import reference_solve
    b = [sd.b.copy() for sd in dec.subs]
    its, conv, hist, ranks, X = reference_solve(dec, [b], REDUCTION, MAXIT, RANK_TOL, **OKW)
    it_cg, conv_cg, h_cg = _cg(dec, b)
    dev = float(np.max(np.abs(hist[:, 0] - h_cg) / h_cg))
    print("iterations", its, it_cg, "max |h - h_CG| / h_CG", dev)
    assert conv == [True] and conv_cg and its == [it_cg] == [30] and ranks == [1] * 30
    assert dev <= CG_HISTORY_TOL


def test_eight_columns_need_fewer_iterations_than_cg(dec):
    """m = 8: every column passes its test no later than independent CG does on it (measured 26-27 against 30); the coupling matrix has
    full rank throughout; the recomputed true reduction agrees with the reported one (gap 4.7e-17, asserted under TRUE_GAP_M8) and
    max |W - W^T| / max |W| over the iterations is rounding (2.3e-17; asserted under 4 eps)."""
    from tests.bcg_reference import reference_solve
    B = block_m8(dec)
    trace = []
    its, conv, hist, ranks, X = reference_solve(dec, B, REDUCTION, MAXIT, RANK_TOL, trace=trace, **OKW)
    cg_its = [_cg(dec, col)[0] for col in B]
    true = _true_reductions(dec, B, X)
    gap = float(np.max(np.abs(hist[-1] / hist[0] - true)))
    asym = max(float(np.max(np.abs(W - W.T)) / np.max(np.abs(W))) for W in trace)
    print("block", its, "CG", cg_its, "gap", gap, "asymmetry", asym)
    assert all(conv) and all(i <= j for i, j in zip(its, cg_its)) and max(its) < min(cg_its)
    assert ranks == [8] * max(its) and hist.shape == (max(its) + 1, 8)
    assert np.all(true < REDUCTION) and gap <= TRUE_GAP_M8
    assert asym <= 4 * np.finfo(float).eps


def test_degenerate_block(dec):
    """b, random, 2 b, zero, random: the rank is 3 in every iteration; the zero column has 0 iterations and its x stays all zero;
    column 2's x is 2 x column 0's (measured: exactly -- the doubling is exact in binary arithmetic and the Jacobi scaling makes the two
    rows of the coupling matrix identical --, so equality is asserted); every non-zero column converges in <= 30 iterations (30, 28, 30,
    28) to a true reduction < 1e-10 that agrees with the reported one (gap 4.5e-18, asserted under TRUE_GAP_DEGENERATE)."""
    from tests.bcg_reference import reference_solve
    B = block_degenerate(dec)
    its, conv, hist, ranks, X = reference_solve(dec, B, REDUCTION, MAXIT, RANK_TOL, **OKW)
    true = _true_reductions(dec, B, X)
    nz = [0, 1, 2, 4]
    gap = float(np.max(np.abs(hist[-1, nz] / hist[0, nz] - true[nz])))
    x0, x2 = np.concatenate(X[0]), np.concatenate(X[2])
    print("iterations", its, "ranks", sorted(set(ranks)), "gap", gap, "max |x2 - 2 x0|", float(np.max(np.abs(x2 - 2.0 * x0))))
    assert set(ranks) == {3} and len(ranks) == max(its)
    assert its[3] == 0 and conv[3] and not np.any(np.concatenate(X[3])) and not np.any(hist[:, 3])
    assert np.array_equal(x2, 2.0 * x0)
    assert all(conv) and all(its[c] <= 30 for c in nz)
    assert np.all(true[nz] < REDUCTION) and gap <= TRUE_GAP_DEGENERATE


def test_rank_tol_default(dec):
    """The default rank_tol on the degenerate block, by the criterion 'recomputed true reduction against reported reduction': every
    value from 1e-15 to 1e-6 gives the same run (rank 3 throughout, iterations 30, 28, 30, 0, 28, gap 4.5e-18); 1e-16 lets rounding
    noise through as a fourth direction in some iterations (ranks 3 and 4), which costs iterations (35, 30, 35, 0, 30) though the
    solve still converges (gap 7.7e-17).  1e-12 sits three decades above the lower edge of that plateau and six below its upper
    end, and at m = 8 with independent columns it drops nothing (rank 8 throughout, test_eight_columns_need_fewer_iterations_than_cg)."""
    from tests.bcg_reference import reference_solve
    B = block_degenerate(dec)
    runs = {}
    for tol in (1e-16, 1e-14, RANK_TOL, 1e-8, 1e-6):
        its, conv, hist, ranks, X = reference_solve(dec, B, REDUCTION, MAXIT, tol, **OKW)
        true = _true_reductions(dec, B, X)
        nz = [0, 1, 2, 4]
        gap = float(np.max(np.abs(hist[-1, nz] / hist[0, nz] - true[nz])))
        print("rank_tol", tol, "iterations", its, "ranks", sorted(set(ranks)), "gap", gap)
        runs[tol] = (its, ranks, gap)
        assert all(conv)
    for tol in (1e-14, 1e-8, 1e-6):
        assert runs[tol][:2] == runs[RANK_TOL][:2]
    assert runs[RANK_TOL][2] <= TRUE_GAP_DEGENERATE
    assert max(runs[1e-16][0]) > max(runs[RANK_TOL][0]) and 4 in runs[1e-16][1]


@pytest.mark.parametrize("name", ["m1", "degenerate", "m8"])
def test_summation_order_sensitivity(dec, name):
    """How far the restatement itself moves when nothing but the order of the additions in its scalar products changes (ascending,
    descending, pairwise: oracle/kernels.c orc_masked_dot_order), on the three blocks of the GPU test.  The device sums in yet another
    order, so this is the envelope its deviation from the restatement is judged by: iteration counts and ranks must not move, and the GPU
    test's history rule 1e-7 |r_k| + 1e-11 |r_0| (RTOL_HIST, ATOL_HIST of tests/test_gpu_multi_gmres.py) must be at least 4 x the largest
    deviation at EVERY iteration and column.  Measured (smallest rule / deviation; largest relative deviation): m = 1 1.7e7 (8.4e-12),
    degenerate 9.2e6 (4.3e-10), m = 8 4.0e6 (1.2e-9)."""
    from oracle import apply_oracle as ao
    from tests.bcg_reference import reference_solve
    from tests.test_gpu_multi_gmres import ATOL_HIST, RTOL_HIST
    B = {"m1": lambda: [[sd.b.copy() for sd in dec.subs]], "degenerate": lambda: block_degenerate(dec), "m8": lambda: block_m8(dec)}[name]()
    runs = {}
    try:
        for order in (0, 1, 2):
            ao.set_dot_order(order)
            runs[order] = reference_solve(dec, B, REDUCTION, MAXIT, RANK_TOL, **OKW)
    finally:
        ao.set_dot_order(0)
    its0, conv0, h0, ranks0, X0 = runs[0]
    rule = RTOL_HIST * h0 + ATOL_HIST * h0[0]
    margin, worst = np.inf, 0.0
    for order in (1, 2):
        its, conv, h, ranks, X = runs[order]
        assert its == its0 and ranks == ranks0 and all(conv)
        dev = np.abs(h - h0)
        live = h0[0] > 0.0                                              # (the zero column's history is all zero in every order)
        assert not np.any(dev[:, ~live])
        margin = min(margin, float(np.min(rule[:, live] / np.maximum(dev[:, live], 1e-300))))
        worst = max(worst, float(np.max(dev[:, live] / h0[:, live])))
    print(name, "iterations", its0, "min rule / deviation", margin, "max relative deviation", worst)
    assert margin >= 4.0
