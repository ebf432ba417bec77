"""CPU checks of flexible restarted GMRES (ddm_fgmres_solve, ddm_fgmres_solve_multi; no GPU needed): the ctypes prototypes of the new
entry points, the argument checks that fail before any device work, the solver dispatch of TwoLevelSchwarz.solve / solve_multi, and
the numpy restatement of the algorithm (tests/fgmres_reference.py) that the GPU tests compare the device drivers with."""
import ctypes
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# |monitored norm - recomputed ||b - A x_j||| <= TRUE_DEFECT_TOL * def0 (test_monitored_norm_is_the_true_defect_norm measures it)
TRUE_DEFECT_TOL = 1e-14


def test_fgmres_prototypes(ddm):
    """the four new symbols are exported by the library (load_library resolves every entry of SYMBOLS) with the documented signatures"""
    lib = ddm.load_library()
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    R = ctypes.POINTER(ddm.SolveResult)
    assert ddm.SYMBOLS["ddm_fgmres_solve"] == (I, [P, P, P, P, P, D, I, I, P, R])
    assert ddm.SYMBOLS["ddm_fgmres_solve"] == ddm.SYMBOLS["ddm_gmres_solve"]
    assert ddm.SYMBOLS["ddm_fgmres_solve_multi"] == (I, [P, P, P, I, P, P, D, I, I, P, R])
    assert ddm.SYMBOLS["ddm_fgmres_solve_multi"] == ddm.SYMBOLS["ddm_gmres_solve_multi"]
    assert ddm.SYMBOLS["ddm_schwarz_set_multi_precision"] == (I, [P, I])
    assert ddm.SYMBOLS["ddm_fgmres_defect_multi"] == (I, [P, P, I, P, P, P, I, P])
    for name in ("ddm_fgmres_solve", "ddm_fgmres_solve_multi", "ddm_schwarz_set_multi_precision", "ddm_fgmres_defect_multi"):
        assert getattr(lib, name) is not None
    assert callable(ddm.fgmres_solve) and callable(ddm.fgmres_solve_multi) and callable(ddm.SchwarzPreconditioner.set_multi_precision)
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "ddm_hip.h")).read()
    for name in ("ddm_fgmres_solve(", "ddm_fgmres_solve_multi(", "ddm_schwarz_set_multi_precision(", "ddm_fgmres_defect_multi("):
        assert "int " + name in header, name


@pytest.mark.parametrize("nrhs, maxit, restart", [(4, 10, 5), (0, 10, 5), (33, 10, 5), (4, 10, 0), (4, -1, 5)])
def test_fgmres_rejects_bad_arguments_without_a_device(ddm, nrhs, maxit, restart):
    """null handles with otherwise valid numbers, nrhs 0 and 33, restart 0, maxit -1: DDM_EINVAL naming the function"""
    lib = ddm.load_library()
    res = (ddm.SolveResult * 33)()
    lib.ddm_cg_solve_multi(None, None, None, 4, None, None, 1e-10, 10, None, res)   # (leaves another function's name in the error text)
    assert lib.ddm_fgmres_solve_multi(None, None, None, nrhs, None, None, 1e-10, maxit, restart, None, res) == ddm.DDM_EINVAL
    assert "ddm_fgmres_solve_multi" in lib.ddm_last_error(None).decode()
    assert lib.ddm_fgmres_solve(None, None, None, None, None, 1e-10, maxit, restart, None, res) == ddm.DDM_EINVAL
    assert "ddm_fgmres_solve:" in lib.ddm_last_error(None).decode()
    assert lib.ddm_gmres_solve(None, None, None, None, None, 1e-10, maxit, restart, None, res) == ddm.DDM_EINVAL   # the same checks as its siblings
    assert "ddm_gmres_solve:" in lib.ddm_last_error(None).decode()
    assert lib.ddm_schwarz_set_multi_precision(None, 1) == ddm.DDM_EINVAL
    assert lib.ddm_fgmres_defect_multi(None, None, nrhs, None, None, None, 1, None) == ddm.DDM_EINVAL


def test_solver_dispatch_knows_the_flexible_solver(ddm):
    """The dispatch happens first and reads no attribute of the object for a solver type it rejects.  The flexible solver is accepted:
    on an object without a device the call gets past the dispatch and fails on the first attribute it needs (AttributeError), while
    minressolver (both methods) and bicgstabsolver (solve_multi) are still refused by name, the message naming the four device solvers."""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    tl = object.__new__(TwoLevelSchwarz)                 # no __init__: no device, no context
    for call in (tl.solve, tl.solve_multi):
        with pytest.raises(AttributeError):
            call(solver="restartedflexiblegmressolver")
        with pytest.raises(NotImplementedError, match="minressolver") as e:
            call(solver="minressolver")
        for name in ("cgsolver", "restartedgmressolver", "restartedflexiblegmressolver", "bicgstabsolver"):
            assert name in str(e.value)
    with pytest.raises(NotImplementedError, match="bicgstabsolver"):
        tl.solve_multi(solver="bicgstabsolver")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def golden_poisson(ddm):
    """the 12^3 problem of tests/golden/poisson12_2x2x2.npz (its index maps are pinned by tests/test_golden.py)"""
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    dec = build_structured(synth.StructuredPoisson((12, 12, 12), (2, 2, 2)), overlap=2, pou_type="distance", shrink=0, neumann=True)
    gold = np.load(os.path.join(GOLD, "poisson12_2x2x2.npz"), allow_pickle=False)
    assert dec.nglobal == int(gold["nglobal"]) and all(np.array_equal(np.asarray(sd.glob, dtype=np.int64), gold[f"sub{s}_glob"]) for s, sd in enumerate(dec.subs))
    return dec


def golden_dg(ddm):
    """the Q1-DG problem of tests/golden/dg32_2x2.npz"""
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    dec = build_structured(synth.StructuredDG2D((32, 32), (2, 2)), overlap=2, pou_type="distance", shrink=0, neumann=True)
    gold = np.load(os.path.join(GOLD, "dg32_2x2.npz"), allow_pickle=False)
    assert dec.nglobal == int(gold["nglobal"]) and all(np.array_equal(np.asarray(sd.glob, dtype=np.int64), gold[f"sub{s}_glob"]) for s, sd in enumerate(dec.subs))
    return dec


# the configurations of the GPU tests (tests/test_gpu_fgmres.py): name -> (problem, oracle_objects' keywords, TwoLevelSchwarz' keywords)
CONFIGS = {
    "poisson_rm": ("poisson", dict(coarse="pou", schwarz_type="restricted", mode="multiplicative"), dict(coarse="pou", schwarz_type="restricted", mode="multiplicative")),
    "poisson_sa": ("poisson", dict(coarse="pou", schwarz_type="standard", mode="additive"), dict(coarse="pou", schwarz_type="standard", mode="additive")),
    "dg_umfpack": ("dg", dict(coarse="pou", schwarz_type="standard", mode="additive", local_solver="direct"),
                   dict(coarse="pou", schwarz_type="standard", mode="additive", subdomain_solver="umfpack")),
}
REDUCTION, MAXIT, RESTART = 1e-10, 200, 6


def problem(ddm, kind):
    return golden_poisson(ddm) if kind == "poisson" else golden_dg(ddm)


def _to_global(dec, xs):
    g = np.zeros(dec.nglobal)
    for sd, v in zip(dec.subs, xs):
        own = np.asarray(sd.owner_novlp) > 0
        g[np.asarray(sd.glob[:sd.n_o])[own]] = v[own]
    return g


def _from_global(dec, g):
    return [g[np.asarray(sd.glob[:sd.n_o])].copy() for sd in dec.subs]


def test_restatement_is_right_preconditioned_gmres(ddm):
    """Fixed preconditioner, restart >= maxit (one cycle) on the 12^3 golden problem, restricted Schwarz + multiplicative coarse level:
    the iterate x_j of the restatement against x_j = M^-1 Q c with c = argmin ||r_0 - (A M^-1 Q) c||_2 by a dense least-squares solve
    (numpy lstsq: SVD), Q an orthonormal basis (classical Gram-Schmidt applied twice, with numpy's dot) of the Krylov space
    span{r_0, (A M^-1) r_0, ..., (A M^-1)^{j-1} r_0}, in global vectors (one entry per degree of freedom, Euclidean norm = the
    owner-masked norm of the solver).

    Tolerance: both sides solve the same least-squares problem with the matrix C = A M^-1 Q, once through Givens rotations of the
    Hessenberg matrix of a modified Gram-Schmidt Arnoldi process (backward stable; its loss of orthogonality is O(eps kappa(C))), once
    through an SVD.  The minimiser is perturbed by at most O(kappa(C) eps) relative, so the test allows 1000 kappa(C) eps ||x|| with
    kappa(C) taken from the singular values of C: 1000 covers the 12 steps, the constants of the two backward error bounds
    and the 12 preconditioner applies in the basis.  kappa(C) is 3.4 here, the bound 7.5e-13; measured: 1.2e-15."""
    from tests.fgmres_reference import fgmres_solve
    from tests.oracle_bridge import oracle_objects
    dec = golden_poisson(ddm)
    kw = CONFIGS["poisson_rm"][1]
    op, sp_, prec, sch, gal = oracle_objects(dec, **kw)
    J = 12
    x = [np.zeros(sd.n_o) for sd in dec.subs]
    b = [sd.b.copy() for sd in dec.subs]
    its = []
    it, conv, hist, red = fgmres_solve(op, sp_, prec, x, b, 1e-30, J, 50, iterates=its)
    assert it == J and len(its) == J and not conv

    def A_Minv(g):
        z = [np.zeros(sd.n_o) for sd in dec.subs]
        prec.apply(z, _from_global(dec, g))
        y = [np.zeros(sd.n_o) for sd in dec.subs]
        op.apply(z, y)
        return _to_global(dec, z), _to_global(dec, y)

    r0 = _to_global(dec, [sd.b for sd in dec.subs])
    assert abs(np.linalg.norm(r0) - hist[0]) <= 1e-14 * hist[0]
    Q = np.zeros((dec.nglobal, J))
    MQ = np.zeros((dec.nglobal, J))
    C = np.zeros((dec.nglobal, J))
    worst = 0.0
    nxt = r0
    for j in range(J):
        q = nxt.copy()
        for _ in range(2):                                   # orthonormal basis of the Krylov space, independent of the solver's
            q -= Q[:, :j] @ (Q[:, :j].T @ q)
        Q[:, j] = q / np.linalg.norm(q)
        MQ[:, j], C[:, j] = A_Minv(Q[:, j])
        nxt = C[:, j]
        c = np.linalg.lstsq(C[:, :j + 1], r0, rcond=None)[0]
        xj = MQ[:, :j + 1] @ c
        sv = np.linalg.svd(C[:, :j + 1], compute_uv=False)
        tol = 1000.0 * (sv[0] / sv[-1]) * np.finfo(float).eps
        dev = np.max(np.abs(_to_global(dec, its[j]) - xj)) / np.max(np.abs(xj))
        worst = max(worst, dev / tol)
        assert dev <= tol, (j, dev, tol)
        # and the monitored norm is the minimum of the least-squares problem
        assert abs(np.linalg.norm(r0 - C[:, :j + 1] @ c) - hist[j + 1]) <= TRUE_DEFECT_TOL * hist[0], j
    print("kappa(C)", sv[0] / sv[-1], "tolerance", tol, "worst deviation / tolerance", worst)


@pytest.mark.parametrize("key, restart", [(k, RESTART) for k in sorted(CONFIGS)] + [("poisson_rm", 200), ("dg_umfpack", 200)])
def test_monitored_norm_is_the_true_defect_norm(ddm, key, restart):
    """|s_{j+1}| against the recomputed ||b - A x_j|| at EVERY iteration j, on the three configurations of the GPU tests with
    restart = 6 (the true defect is recomputed at each restart) and on two of them without a restart.

    Measured max_j | |s_{j+1}| - ||b - A x_j|| | / def0: 1.1e-16 (Poisson, both configurations), 2.9e-16 (DG) with restart 6;
    1.5e-16 and 2.9e-16 in one cycle.  That is the rounding of the recomputation itself (b - A x is formed from vectors of size
    def0) and does not grow while the defect falls by ten orders of magnitude.  TRUE_DEFECT_TOL = 1e-14 (45 eps, relative to def0)
    leaves a factor 20 for another summation order in the operator and in the norm (the device's); the final defects of these runs
    are 4e-11 def0 to 8e-11 def0, so the bound is 2.5e-4 of the smallest quantity it is applied to."""
    from tests.fgmres_reference import reference_solve
    from tests.oracle_bridge import oracle_objects
    kind, okw, _ = CONFIGS[key]
    dec = problem(ddm, kind)
    its = []
    it, conv, hist, red, x = reference_solve(dec, reduction=REDUCTION, maxit=MAXIT, restart=restart, iterates=its, **okw)
    assert conv and it == len(its) and it > (2 * RESTART if restart == RESTART else 8), it
    assert red < REDUCTION and red == hist[-1] / hist[0]
    op, sp_, prec, sch, gal = oracle_objects(dec, **okw)
    worst = 0.0
    for j, xj in enumerate(its, start=1):
        bb = [sd.b.copy() for sd in dec.subs]
        op.applyscaleadd(-1.0, xj, bb)
        worst = max(worst, abs(sp_.norm(bb) - hist[j]) / hist[0])
    print(key, "restart", restart, "iterations", it, "max |monitored - true| / def0", worst)
    assert worst <= TRUE_DEFECT_TOL
    assert all(np.array_equal(a, c) for a, c in zip(its[-1], x))     # the last iterate is the solution that is returned


def test_restatement_tolerates_a_changing_preconditioner(ddm):
    """M^-1 alternates between the two-level preconditioner and the Schwarz level alone: the monitored norm is still the true defect
    norm, and the solve converges (what a left-preconditioned GMRES cannot offer)."""
    from tests.fgmres_reference import fgmres_solve
    from tests.oracle_bridge import oracle_objects
    dec = golden_poisson(ddm)
    op, sp_, prec, sch, gal = oracle_objects(dec, **CONFIGS["poisson_sa"][1])
    x = [np.zeros(sd.n_o) for sd in dec.subs]
    b = [sd.b.copy() for sd in dec.subs]
    it, conv, hist, red = fgmres_solve(op, sp_, prec, x, b, 1e-8, 200, 10, prec_apply=lambda j, z, v: (prec if j % 2 == 0 else sch).apply(z, v))
    assert conv and red < 1e-8
    bb = [sd.b.copy() for sd in dec.subs]
    op.applyscaleadd(-1.0, x, bb)
    assert abs(sp_.norm(bb) - hist[-1]) <= TRUE_DEFECT_TOL * hist[0] and sp_.norm(bb) < 1e-8 * hist[0]
