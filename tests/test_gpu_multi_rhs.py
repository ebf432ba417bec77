"""-m gpu: several right-hand sides at once (the ddm_*_multi entry points and ddm_cg_solve_multi) against the single-vector entry
points column by column, and column 0 of a block CG solve against the CPU oracle.

Which comparisons are exact: the halo exchanges, the owner-masked dots (same grid, rows per thread and block_sum as the single-vector
kernels) and the coarse prolongation keep the single-vector summation order, so ``dot_multi`` is compared with ``==``.  The products
(CSR block SpMV), the local solve (the level engine for all columns instead of the single-launch engine) and the coarse restriction
(one pass over the basis for all columns) sum in another order: those results are compared within 1e-13 of the column's largest entry."""
import numpy as np
import pytest

from tests.test_gpu_parity import ATOL_HIST, RTOL_HIST, _build

pytestmark = pytest.mark.gpu

RTOL_APPLY = 1e-13


def _consistent_block(tl, dec, m, seed):
    """(n_o, m) block of consistent vectors (the same value on every holder of a DoF), as a host array"""
    rng = np.random.default_rng(seed)
    cols = []
    for _ in range(m):
        xg = rng.standard_normal(dec.nglobal)
        cols.append(tl.rl.cat_novlp([xg[sd.glob[:sd.n_o]] for sd in dec.subs]))
    return np.stack(cols, axis=1)


def _close(a, b, rtol=RTOL_APPLY):
    return float(np.max(np.abs(a - b))) <= rtol * max(float(np.max(np.abs(b))), 1e-300)


def _geneo_tl(dec, stype, mode):
    from dune_ddm_amd.geneo import geneo_basis
    from dune_ddm_amd.solver import TwoLevelSchwarz
    tl = TwoLevelSchwarz(dec, coarse="none", schwarz_type=stype)
    basis = geneo_basis(tl, nev=4, tol=1e-5)
    tl.set_coarse_basis(basis)
    tl.rebuild_combined(mode)
    return tl


@pytest.fixture(scope="module")
def problems(ddm):
    return {"pou": _build(ddm, (13, 12, 11), (2, 2, 2)), "geneo": _build(ddm, (13, 12, 11), (2, 2, 2), neumann=True)}


@pytest.mark.parametrize("coarse", ["pou", "geneo"])
@pytest.mark.parametrize("m", [1, 3, 8])
def test_multi_applies_match_single_applies(ddm, problems, coarse, m):
    """op_apply_multi, applyscaleadd_multi, dot_multi, schwarz_apply_multi (standard, restricted), galerkin_apply_multi and
    combined_apply_multi (additive, multiplicative): column j against the single-vector entry point on column j."""
    import torch
    from dune_ddm_amd.solver import TwoLevelSchwarz
    dec = problems[coarse]
    for stype, mode in (("standard", "additive"), ("restricted", "additive"), ("standard", "multiplicative"), ("restricted", "multiplicative")):
        tl = _geneo_tl(dec, stype, mode) if coarse == "geneo" else TwoLevelSchwarz(dec, coarse="pou", schwarz_type=stype, mode=mode)
        n_o = tl.rl.n_o
        X = tl.to_device(_consistent_block(tl, dec, m, seed=11 + m))
        Y0 = tl.to_device(_consistent_block(tl, dec, m, seed=97 + m))
        col = lambda B, j: B[:, j].contiguous()   # noqa: E731

        # operator: Y = A X, Y += alpha A X
        Y = torch.empty_like(X)
        tl.op.apply_multi(X, Y)
        Ys = torch.stack([tl.zeros(n_o) for _ in range(m)], dim=1)
        for j in range(m):
            y = tl.zeros(n_o)
            tl.op.apply(col(X, j), y)
            Ys[:, j] = y
        tl.ctx.sync()
        assert _close(Y.cpu().numpy(), Ys.cpu().numpy())
        Y = Y0.clone()
        tl.op.applyscaleadd_multi(-0.5, X, Y)
        for j in range(m):
            y = col(Y0, j).clone()
            tl.op.applyscaleadd(-0.5, col(X, j), y)
            Ys[:, j] = y
        tl.ctx.sync()
        assert _close(Y.cpu().numpy(), Ys.cpu().numpy())

        # dots: bit-identical (same reduction tree per column)
        d = tl.op.dot_multi(X, Y0)
        assert all(d[j] == tl.op.dot(col(X, j), col(Y0, j)) for j in range(m)), d

        # preconditioners, each column against the single-vector apply
        for dev in (tl.schwarz, tl.galerkin, tl.prec):
            Z = torch.full_like(X, float("nan"))          # every entry must be written
            dev.apply_multi(Z, Y0)
            Zs = torch.empty_like(X)
            for j in range(m):
                z = tl.zeros(n_o)
                dev.apply(z, col(Y0, j))
                Zs[:, j] = z
            tl.ctx.sync()
            assert _close(Z.cpu().numpy(), Zs.cpu().numpy()), (type(dev).__name__, stype, mode)
        tl.prec.check_status()
        tl.ctx.close()


def _rhs_block(tl, dec):
    """m = 5: the problem's right-hand side, a random consistent one, twice the first (exact scaling), zero, another random one"""
    b0 = np.asarray(tl.rl.b, dtype=np.float64)
    R = _consistent_block(tl, dec, 2, seed=5)
    return np.stack([b0, R[:, 0], 2.0 * b0, np.zeros_like(b0), R[:, 1]], axis=1)


def test_cg_multi_columns_match_single_solves(ddm):
    """Every column of ddm_cg_solve_multi behaves like ddm_cg_solve on it: same iteration count and convergence flag, history within
    the RTOL_HIST / ATOL_HIST rule of test_gpu_parity.py, x within 1e-8.  A column that is twice another one runs the same recurrences
    exactly scaled (bit for bit); the zero column is converged at once; converged columns stay frozen (bit-unchanged x)."""
    import torch
    from dune_ddm_amd.solver import TwoLevelSchwarz
    dec = _build(ddm, (17, 17, 17), (2, 2, 2))
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="standard", mode="additive")
    Bh = _rhs_block(tl, dec)
    m = Bh.shape[1]
    res, hist, X = tl.solve_multi(Bh, reduction=1e-10, maxit=300)
    Xh = X.cpu().numpy()
    assert len(res) == m and hist.shape == (max(r.iterations for r in res) + 1, m)
    for j in range(m):
        if j == 3:
            continue
        r1, h1, x1 = tl.solve(reduction=1e-10, maxit=300, b=Bh[:, j])
        assert res[j].iterations == r1.iterations and res[j].converged == r1.converged == 1, (j, res[j].iterations, r1.iterations)
        hj = hist[:res[j].iterations + 1, j]
        assert (np.abs(hj - h1) <= RTOL_HIST * h1 + ATOL_HIST * h1[0]).all(), j
        assert np.isnan(hist[res[j].iterations + 1:, j]).all()          # the history stops where the column converged
        x1 = x1.cpu().numpy()
        assert np.max(np.abs(Xh[:, j] - x1)) <= 1e-8 * np.max(np.abs(x1)), j
        assert res[j].reduction <= 1e-10
    # exact scaling: column 2 = 2 x column 0 in every iterate
    assert res[2].iterations == res[0].iterations
    assert np.array_equal(Xh[:, 2], 2.0 * Xh[:, 0]) and np.array_equal(hist[:, 2], 2.0 * hist[:, 0])
    # zero right-hand side: converged at once, x untouched
    assert res[3].iterations == 0 and res[3].converged == 1 and res[3].def0 == 0.0
    assert not np.any(Xh[:, 3]) and hist[0, 3] == 0.0 and np.isnan(hist[1:, 3]).all()
    # frozen columns: rerun up to the iteration where the earliest (non-zero) column converged; its x then is the final one bit for bit
    its = [r.iterations for r in res]
    early = min((j for j in range(m) if j != 3), key=lambda j: its[j])
    res2, _, X2 = tl.solve_multi(Bh, reduction=1e-10, maxit=its[early])
    assert res2[early].converged == 1 and res2[early].iterations == its[early]
    assert torch.equal(X2[:, early], X[:, early])
    if its[early] < max(its):
        assert not all(r.converged for r in res2)                        # the others were still running
    tl.prec.check_status()
    tl.ctx.close()


def test_cg_multi_column0_matches_oracle(ddm):
    """Column 0 (the problem's right-hand side) of the same block solve against the CPU oracle's CG."""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    from tests.oracle_bridge import oracle_solve
    dec = _build(ddm, (17, 17, 17), (2, 2, 2))
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="standard", mode="additive")
    res, hist, X = tl.solve_multi(_rhs_block(tl, dec), reduction=1e-10, maxit=300)
    it, conv, hist_o, xo = oracle_solve(dec, reduction=1e-10, maxit=300, coarse="pou", schwarz_type="standard", mode="additive")
    ho = np.array(hist_o)
    assert res[0].iterations == it and res[0].converged and conv
    h0 = hist[:it + 1, 0]
    assert (np.abs(h0 - ho) <= RTOL_HIST * ho + ATOL_HIST * ho[0]).all()
    want = np.concatenate(xo)
    assert np.max(np.abs(X[:, 0].cpu().numpy() - want)) <= 1e-8 * np.max(np.abs(want))
    tl.ctx.close()


def test_cg_multi_with_direct_local_solver(ddm):
    """The sparse direct local solver (`direct`, standard, additive, cgsolver) through cg_solve_multi: the multi-RHS solve of a direct
    factor.  Columns against single solves, column 0 against the oracle with the exact local solve."""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    from tests.oracle_bridge import oracle_solve
    dec = _build(ddm, (17, 16, 15), (2, 2, 2))
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="standard", mode="additive", subdomain_solver="direct")
    b0 = np.asarray(tl.rl.b, dtype=np.float64)
    Bh = np.concatenate([b0[:, None], _consistent_block(tl, dec, 2, seed=23)], axis=1)
    res, hist, X = tl.solve_multi(Bh, reduction=1e-10, maxit=200)
    for j in range(Bh.shape[1]):
        r1, h1, x1 = tl.solve(reduction=1e-10, maxit=200, b=Bh[:, j])
        assert res[j].converged and res[j].iterations == r1.iterations, (j, res[j].iterations, r1.iterations)
        assert (np.abs(hist[:r1.iterations + 1, j] - h1) <= 1e-7 * h1 + 1e-11 * h1[0]).all()
        x1 = x1.cpu().numpy()
        assert np.max(np.abs(X[:, j].cpu().numpy() - x1)) <= 1e-8 * np.max(np.abs(x1))
    it, conv, hist_o, xo = oracle_solve(dec, reduction=1e-10, maxit=200, coarse="pou", schwarz_type="standard", mode="additive", local_solver="direct")
    ho = np.array(hist_o)
    assert res[0].iterations == it and conv
    assert (np.abs(hist[:it + 1, 0] - ho) <= 1e-7 * ho + 1e-11 * ho[0]).all()
    tl.prec.check_status()
    tl.ctx.close()


def test_multi_argument_checks_and_local_status(ddm):
    """nrhs = 0 and nrhs = 33 are DDM_EINVAL; a local-solve status word that is already set makes the block applies and the block CG
    return DDM_ENUMERIC (fail fast, as the single-vector applies)."""
    import ctypes
    import torch
    from dune_ddm_amd.solver import TwoLevelSchwarz
    dec = _build(ddm, (11, 10, 9), (2, 2, 2))
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="standard", mode="additive")
    lib, h = tl.ctx.lib, tl.ctx.h
    n_o = tl.rl.n_o
    X = torch.zeros((n_o, 33), dtype=torch.float64, device=tl.dev)
    B = torch.ones((n_o, 33), dtype=torch.float64, device=tl.dev)
    res = (ddm.SolveResult * 33)()
    dots = np.zeros(33)
    for m in (0, 33):
        assert lib.ddm_cg_solve_multi(h, tl.op.h, tl.prec.h, m, X.data_ptr(), B.data_ptr(), 1e-10, 10, None, res) == ddm.DDM_EINVAL
        assert "nrhs" in lib.ddm_last_error(h).decode()
        assert lib.ddm_op_apply_multi(h, tl.op.h, m, X.data_ptr(), B.data_ptr()) == ddm.DDM_EINVAL
        assert lib.ddm_dot_multi(h, tl.op.h, m, X.data_ptr(), B.data_ptr(), dots.ctypes.data) == ddm.DDM_EINVAL
        for fn, obj in ((lib.ddm_schwarz_apply_multi, tl.schwarz), (lib.ddm_galerkin_apply_multi, tl.galerkin), (lib.ddm_combined_apply_multi, tl.prec)):
            assert fn(h, obj.h, m, X.data_ptr(), B.data_ptr()) == ddm.DDM_EINVAL
    F = ctypes.c_void_p(tl.schwarz.local_solver())
    assert lib.ddm_ilu0_set_status(F, 1) == ddm.DDM_OK
    try:
        Xs, Bs = X[:, :4].contiguous(), B[:, :4].contiguous()
        assert lib.ddm_cg_solve_multi(h, tl.op.h, tl.prec.h, 4, Xs.data_ptr(), Bs.data_ptr(), 1e-10, 10, None, res) == ddm.DDM_ENUMERIC
        assert lib.ddm_schwarz_apply_multi(h, tl.schwarz.h, 4, Xs.data_ptr(), Bs.data_ptr()) == ddm.DDM_ENUMERIC
        assert lib.ddm_combined_apply_multi(h, tl.prec.h, 4, Xs.data_ptr(), Bs.data_ptr()) == ddm.DDM_ENUMERIC
    finally:
        assert lib.ddm_ilu0_set_status(F, 0) == ddm.DDM_OK
    r, hist, Xr = tl.solve_multi(np.asarray(tl.rl.b)[:, None], maxit=200)   # m = 1 works once the word is clear
    r1, h1, _ = tl.solve(maxit=200)
    assert r[0].converged and r[0].iterations == r1.iterations
    tl.ctx.close()


def test_block_drivers_share_one_work_pool(ddm):
    """All block drivers take their n x width work blocks from one grow-only pool of the preconditioner object (KrylovWork).  Run back
    to back on ONE preconditioner -- the pool grown (3 -> 5 columns: dropped and allocated afresh), kept (5 -> 2, 4, 2, 3) and reused
    with whatever another driver left in it -- every call returns bit for bit what the same call returns on a preconditioner made
    fresh for it: x, histories, ranks / widths and results.  The first and the last call are the same call and agree as well.  No
    tolerance: that each driver's numbers are right is what its own tests assert."""
    import torch
    from dune_ddm_amd.solver import TwoLevelSchwarz
    from tests.test_apply_shapes_reference import consistent_columns
    from tests.test_fgmres_cpu import golden_poisson
    dec = golden_poisson(ddm)
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="standard", mode="additive")
    B5 = consistent_columns(dec, 5, seed=23)
    kw = dict(reduction=1e-8, maxit=200)
    calls = [                                            # (driver, its width argument or None, columns)
        (ddm.bicgstab_solve_queue, 3, 5),
        (ddm.bcg_solve_multi, None, 5),
        (ddm.cg_solve_queue, 2, 5),
        (ddm.cg_solve_multi, None, 4),
        (lambda *a, **k: ddm.bgmres_solve_multi(*a, restart=5, **k), None, 2),
        (ddm.bicgstab_solve_queue, 3, 5),
    ]

    def run(fn, width, m):
        X, B = torch.zeros((tl.rl.n_o, m), dtype=torch.float64, device=tl.dev), tl.to_device(B5[:, :m])
        out = fn(tl.ctx, tl.op, tl.prec, X, B, *(() if width is None else (width,)), **kw)
        tl.prec.check_status()
        res = [(r.iterations, r.converged, r.def0, r.reduction) for r in out[0]]
        return X.cpu().numpy(), res, [np.asarray(a).copy() for a in out[1:]]

    def same(a, b):
        return np.array_equal(a[0], b[0]) and a[1] == b[1] and len(a[2]) == len(b[2]) and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a[2], b[2]))

    shared = [run(*c) for c in calls]                    # one preconditioner, one pool
    for k, c in enumerate(calls):
        tl.rebuild_combined("additive")                  # a fresh preconditioner: an empty pool
        assert same(shared[k], run(*c)), k
    assert same(shared[0], shared[-1])
    assert all(all(r[1] == 1 for r in s[1]) for s in shared)   # (every column converged: the runs are whole solves)
    tl.ctx.close()
