"""CPU checks of flexible CG (ddm_fcg_solve, ddm_fcg_solve_multi, ddm_fcg_orth_multi; no GPU needed): the ctypes prototypes and header
declarations of the new entry points, the argument checks that fail before any device work, the solver dispatch of
TwoLevelSchwarz.solve / solve_multi, and the numpy restatement of the algorithm (tests/fcg_reference.py) that the GPU tests compare the
device drivers with: on a symmetric preconditioner it is CG, on the non-symmetric ones it converges where CG is slower or fails, the
norm it tests is the true defect norm, the window it orthogonalises against is A-orthogonal to the fresh direction, and its history
moves far less than the GPU tests' rule allows when only the order of the additions in the dots changes."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_fgmres_cpu import CONFIGS as GMRES_CONFIGS
from tests.test_fgmres_cpu import TRUE_DEFECT_TOL, golden_poisson

# the configurations of the GPU tests (tests/test_gpu_fcg.py) on tests/golden/poisson12_2x2x2.npz with the POU coarse space:
# name -> (oracle_objects' keywords, TwoLevelSchwarz' keywords)
_RA = dict(coarse="pou", schwarz_type="restricted", mode="additive")
CONFIGS = {
    "poisson_sa": GMRES_CONFIGS["poisson_sa"][1:],       # standard Schwarz, additive: a symmetric positive definite preconditioner
    "poisson_ra": (_RA, _RA),                            # restricted Schwarz, additive: the reference's default Schwarz type
    "poisson_rm": GMRES_CONFIGS["poisson_rm"][1:],       # restricted Schwarz, multiplicative
}
REDUCTION, MAXIT = 1e-10, 200
# (mmax, complete) of the GPU tests: mmax = 3 restarted swaps slot 0 and slot 3 several times, mmax = 3 complete wraps with stale higher
# slots in the window, mmax = 1 restarted swaps slots 0 and 1
SETTINGS = ((3, False), (3, True), (1, False))
# iterations of the restatement, mmax = 3: (restarted, complete)
ITERATIONS_MMAX3 = {"poisson_sa": (30, 30), "poisson_ra": (19, 17), "poisson_rm": (13, 13)}
# |reported reduction - recomputed ||b - A x|| / def0|: 1.1e-16 at most on the two non-symmetric configurations (1.9e-16 on poisson_sa),
# the rounding of the recomputation; TRUE_DEFECT_TOL = 1e-14 of tests/test_fgmres_cpu.py is the larger of the two and is what is asserted
FCG_TRUE_DEFECT_TOL = max(TRUE_DEFECT_TOL, 1.1e-16)
CG_HISTORY_TOL = 2e-9       # 4 x 4.03e-10 (test_spd_preconditioner_fcg_is_cg), rounded up
ORTHOGONALITY_TOL = 1.5e-15  # 4 x 3.6e-16 (test_window_is_a_orthogonal), rounded up


def test_fcg_prototypes(ddm):
    """the three new symbols are exported by the library (load_library resolves every entry of SYMBOLS) with the documented signatures,
    declared in the header and wrapped"""
    lib = ddm.load_library()
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    R = ctypes.POINTER(ddm.SolveResult)
    assert ddm.SYMBOLS["ddm_fcg_solve"] == (I, [P, P, P, P, P, D, I, I, I, P, R])
    assert ddm.SYMBOLS["ddm_fcg_solve_multi"] == (I, [P, P, P, I, P, P, D, I, I, I, P, R])
    assert ddm.SYMBOLS["ddm_fcg_orth_multi"] == (I, [P, P, I, I, P, P, P, P, P, I, P])
    for name in ("ddm_fcg_solve", "ddm_fcg_solve_multi", "ddm_fcg_orth_multi"):
        assert getattr(lib, name) is not None
    assert callable(ddm.fcg_solve) and callable(ddm.fcg_solve_multi) and callable(ddm.fcg_orth_multi)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ddm_hip.h")).read()
    for name in ("ddm_fcg_solve(", "ddm_fcg_solve_multi(", "ddm_fcg_orth_multi("):
        assert "int " + name in header, name


@pytest.mark.parametrize("nrhs, maxit, mmax", [(4, 10, 3), (4, 10, 0), (4, -1, 3), (0, 10, 3), (33, 10, 3)])
def test_fcg_rejects_bad_arguments_without_a_device(ddm, nrhs, maxit, mmax):
    """null handles with otherwise valid numbers, mmax 0, maxit -1, nrhs 0 and 33, both variants: DDM_EINVAL naming the function"""
    lib = ddm.load_library()
    res = (ddm.SolveResult * 33)()
    for complete in (0, 1):
        lib.ddm_cg_solve_multi(None, None, None, 4, None, None, 1e-10, 10, None, res)   # (leaves another function's name in the error text)
        assert lib.ddm_fcg_solve_multi(None, None, None, nrhs, None, None, 1e-10, maxit, mmax, complete, None, res) == ddm.DDM_EINVAL
        assert "ddm_fcg_solve_multi" in lib.ddm_last_error(None).decode()
        assert lib.ddm_fcg_solve(None, None, None, None, None, 1e-10, maxit, mmax, complete, None, res) == ddm.DDM_EINVAL
        assert "ddm_fcg_solve:" in lib.ddm_last_error(None).decode()
    assert lib.ddm_fcg_orth_multi(None, None, nrhs, 2, None, None, None, None, None, 1, None) == ddm.DDM_EINVAL
    assert "ddm_fcg_orth_multi" in lib.ddm_last_error(None).decode()


def test_solver_dispatch_knows_the_fcg_solvers(ddm):
    """The two new solver types get past the dispatch of solve and solve_multi: on an object without a device the call fails on the
    first attribute it needs (AttributeError).  minressolver is still refused by name, the message naming all six device solvers;
    solve_many refuses the new types (there is no queued flexible CG loop)."""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    tl = object.__new__(TwoLevelSchwarz)                 # no __init__: no device, no context
    six = ("cgsolver", "restartedgmressolver", "restartedflexiblegmressolver", "restartedfcgsolver", "completefcgsolver", "bicgstabsolver")
    assert TwoLevelSchwarz.SOLVERS == six
    for call in (tl.solve, tl.solve_multi):
        for name in ("restartedfcgsolver", "completefcgsolver"):
            with pytest.raises(AttributeError):
                call(solver=name, mmax=3)
        with pytest.raises(NotImplementedError, match="minressolver") as e:
            call(solver="minressolver")
        for name in six:
            assert name in str(e.value)
    for name in ("restartedfcgsolver", "completefcgsolver"):
        with pytest.raises(NotImplementedError, match=name):
            tl.solve_many(None, solver=name)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dec(ddm):
    return golden_poisson(ddm)


def _cg(dec, okw, maxit=MAXIT):
    from oracle import apply_oracle as ao
    from tests.oracle_bridge import oracle_objects
    op, sp_, prec, sch, gal = oracle_objects(dec, **okw)
    x = [np.zeros(sd.n_o) for sd in dec.subs]
    b = [sd.b.copy() for sd in dec.subs]
    it, conv, hist = ao.cg_solve(op, sp_, prec, x, b, REDUCTION, maxit)
    bb = [sd.b.copy() for sd in dec.subs]
    op.applyscaleadd(-1.0, x, bb)
    return it, conv, np.asarray(hist, dtype=float), sp_.norm(bb) / hist[0]


def _true_reduction(dec, okw, x):
    from tests.oracle_bridge import oracle_objects
    op, sp_, prec, sch, gal = oracle_objects(dec, **okw)
    b0 = [sd.b.copy() for sd in dec.subs]
    bb = [sd.b.copy() for sd in dec.subs]
    op.applyscaleadd(-1.0, x, bb)
    return sp_.norm(bb) / sp_.norm(b0)


def test_spd_preconditioner_fcg_is_cg(dec):
    """Standard Schwarz + additive coarse level is a symmetric positive definite preconditioner; there flexible CG is CG in exact
    arithmetic, whatever mmax and the variant: the directions CG drops are A-orthogonal to the new one already.  All six of
    mmax = 1, 3, 10 x restarted, complete take ao.cg_solve's 30 iterations, and max_k |h_k - h_k^CG| / h_k^CG, measured on the oracle,
    is 8.8e-12, 8.8e-12 (mmax 1), 8.3e-12, 4.7e-11 (mmax 3), 7.2e-11, 4.03e-10 (mmax 10; restarted, complete).  Asserted under
    4 x the largest, rounded up: 2e-9 (the factor 4 is the project's margin for another summation order)."""
    from tests.fcg_reference import reference_solve
    okw = CONFIGS["poisson_sa"][0]
    it_cg, conv_cg, h_cg, true_cg = _cg(dec, okw)
    assert conv_cg and it_cg == 30
    for mmax in (1, 3, 10):
        for complete in (False, True):
            it, conv, hist, red, x = reference_solve(dec, REDUCTION, MAXIT, mmax, complete, **okw)
            assert conv and it == it_cg, (mmax, complete, it)
            dev = float(np.max(np.abs(hist - h_cg) / h_cg))
            print("mmax", mmax, "complete", complete, "iterations", it, "max |h - h_CG| / h_CG", dev)
            assert dev <= CG_HISTORY_TOL, (mmax, complete, dev)


@pytest.mark.parametrize("key", ["poisson_ra", "poisson_rm"])
def test_nonsymmetric_preconditioner(dec, key):
    """Restricted Schwarz, additive and multiplicative, mmax = 3, both variants: all four runs converge, in 19 / 17 and 13 / 13
    iterations (restarted / complete); the recomputed true reduction ||b - A x|| / def0 is below 1e-10 and agrees with the reported one
    within TRUE_DEFECT_TOL = 1e-14 (relative to def0) -- measured here: 1.0e-16, 4.4e-17 (additive), 5.8e-17, 7.2e-17 (multiplicative),
    bound 1.1e-16, which is smaller than TRUE_DEFECT_TOL, so the latter is asserted.  CG on the same preconditioner: 24 iterations
    (additive; slower) and no convergence in 200 iterations (multiplicative; true reduction 4.7e-5)."""
    from tests.fcg_reference import reference_solve
    okw = CONFIGS[key][0]
    for complete, want in zip((False, True), ITERATIONS_MMAX3[key]):
        it, conv, hist, red, x = reference_solve(dec, REDUCTION, MAXIT, 3, complete, **okw)
        true = _true_reduction(dec, okw, x)
        print(key, "complete", complete, "iterations", it, "reported", red, "true", true, "|reported - true|", abs(red - true))
        assert conv and it == want, (it, want)
        assert red == hist[-1] / hist[0] and len(hist) == it + 1
        assert true < REDUCTION
        assert abs(red - true) <= FCG_TRUE_DEFECT_TOL
    it_cg, conv_cg, h_cg, true_cg = _cg(dec, okw)
    print(key, "CG: iterations", it_cg, "converged", conv_cg, "true reduction", true_cg)
    if key == "poisson_rm":
        assert not conv_cg and it_cg == MAXIT and true_cg > 1e-6
    else:
        assert conv_cg and it_cg > max(ITERATIONS_MMAX3[key])


def test_window_is_a_orthogonal(dec):
    """|<d_s, A d_k>| / sqrt(g_s g_k) for the fresh direction after its orthogonalisation against every slot k of its window, over all
    iterations, on the symmetric configuration: measured 2.9e-16 (mmax 1), 3.6e-16 (mmax 3 and 10, both variants) -- classical
    Gram-Schmidt against a window that is itself A-orthogonal to rounding.  Asserted under 4 x the largest, rounded up: 1.5e-15.
    Every window has the size the variant prescribes: restarted s slots, complete klimit slots without s."""
    from tests.fcg_reference import reference_solve
    from tests.oracle_bridge import oracle_objects
    okw = CONFIGS["poisson_sa"][0]
    op, sp_, prec, sch, gal = oracle_objects(dec, **okw)
    for mmax in (1, 3, 10):
        for complete in (False, True):
            W = []
            it, conv, hist, red, x = reference_solve(dec, REDUCTION, MAXIT, mmax, complete, windows=W, **okw)
            assert len(W) == it
            sizes = [len(win) for (d, Ad, g, win) in W]
            if complete:
                assert sizes == [min(j, mmax) for j in range(it)], sizes                    # after the first pass: all slots but s
            else:
                assert sizes == [j if j <= mmax else (j - mmax - 1) % mmax + 1 for j in range(it)], sizes
            worst = 0.0
            for (d, Ad, g, win) in W:
                for (dk, Adk, gk) in win:
                    worst = max(worst, abs(sp_.dot(d, Adk)) / np.sqrt(g * gk))
            print("mmax", mmax, "complete", complete, "max |<d_s, A d_k>| / sqrt(g_s g_k)", worst)
            assert worst <= ORTHOGONALITY_TOL, (mmax, complete, worst)


@pytest.mark.parametrize("key", sorted(CONFIGS))
def test_summation_order_sensitivity(dec, key):
    """How far the restatement itself moves when nothing but the order of the additions in its dots changes (ascending, descending,
    pairwise: oracle/kernels.c orc_masked_dot_order, as tests/test_oracle_order_sensitivity.py does for CG), on the nine runs of the
    GPU test (three configurations x SETTINGS).  The device sums in yet another order, so this is the envelope its deviation from the
    restatement is judged by: the iteration counts must not move, and the GPU test's history rule 1e-7 |r_k| + 1e-11 |r_0| (RTOL_HIST,
    ATOL_HIST of tests/test_gpu_multi_gmres.py) must be at least 4 x the largest deviation at EVERY iteration.
    Measured (smallest rule / deviation over the iterations and the two other orders; largest relative deviation):
      poisson_sa  mmax 3 restarted 1.5e7 (1.3e-11), mmax 3 complete 4.9e6 (5.5e-11), mmax 1 restarted 2.0e7 (1.5e-11)
      poisson_ra  mmax 3 restarted 2.2e5 (3.5e-12), mmax 3 complete 2.3e5 (4.3e-12), mmax 1 restarted 1.7e6 (5.1e-13)
      poisson_rm  mmax 3 restarted 6.1e5 (3.3e-12), mmax 3 complete 1.5e6 (3.0e-10), mmax 1 restarted 1.1e6 (5.6e-13)
    so no configuration had to be replaced.  Reported reductions (against 1e-10): 9.06e-11 (poisson_sa, every setting), 1.67e-11 /
    6.05e-11 / 8.21e-11 (poisson_ra), 8.84e-11 / 2.04e-11 / 8.80e-11 (poisson_rm): none sits at the threshold."""
    from oracle import apply_oracle as ao
    from tests.fcg_reference import reference_solve
    from tests.test_gpu_multi_gmres import ATOL_HIST, RTOL_HIST
    okw = CONFIGS[key][0]
    for mmax, complete in SETTINGS:
        runs = {}
        try:
            for order in (0, 1, 2):
                ao.set_dot_order(order)
                runs[order] = reference_solve(dec, REDUCTION, MAXIT, mmax, complete, **okw)
        finally:
            ao.set_dot_order(0)
        it0, conv0, h0, red0, x0 = runs[0]
        rule = RTOL_HIST * h0 + ATOL_HIST * h0[0]
        margin, worst = np.inf, 0.0
        for order in (1, 2):
            it, conv, h, red, x = runs[order]
            assert conv and conv0 and it == it0, (mmax, complete, order, it, it0)
            dev = np.abs(h - h0)
            margin = min(margin, float(np.min(rule / np.maximum(dev, 1e-300))))
            worst = max(worst, float(np.max(dev / h0)))
        print(key, "mmax", mmax, "complete", complete, "iterations", it0, "reduction", red0, "min rule / deviation", margin, "max relative deviation", worst)
        assert margin >= 4.0, (mmax, complete, margin)
