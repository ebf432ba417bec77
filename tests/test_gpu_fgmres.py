"""-m gpu: flexible restarted GMRES on the device (ddm_fgmres_solve, ddm_fgmres_solve_multi) against the numpy restatement of the algorithm
(tests/fgmres_reference.py, checked on the CPU by tests/test_fgmres_cpu.py), against the recomputed true defect, the block driver
against the single-vector one, the fused restart kernel against the kernels it replaces, the single-precision local solve as a
preconditioner that differs from the one the reference uses, and the host-side refusals.

Tolerances: histories under the project's GMRES rule (1e-7 |r_k| + 1e-11 |r_0|); monitored against recomputed
defect norm TRUE_DEFECT_TOL = 1e-14 def0, measured in tests/test_fgmres_cpu.py; block against single x 2e-14 relative (the
block-GMRES figure).  Everything that compares the block driver with itself is bitwise."""
import ctypes

import numpy as np
import pytest

from tests.test_fgmres_cpu import CONFIGS, MAXIT, REDUCTION, RESTART, TRUE_DEFECT_TOL, problem
from tests.test_gpu_multi_gmres import ATOL_HIST, RTOL_HIST
from tests.test_gpu_multi_rhs import _consistent_block
from tests.test_gpu_parity import _build

pytestmark = pytest.mark.gpu

SOLVER = "restartedflexiblegmressolver"
XTOL_BLOCK = 2e-14
WIDTHS = (1, 3, 8, 13, 32)


# ---- 1, 2: one right-hand side ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def references(ddm):
    """the restatement's runs, computed once per configuration"""
    from tests.fgmres_reference import reference_solve
    made = {}

    def get(key):
        if key not in made:
            kind, okw, _ = CONFIGS[key]
            made[key] = reference_solve(problem(ddm, kind), reduction=REDUCTION, maxit=MAXIT, restart=RESTART, **okw)
        return made[key]
    return get


def _true_defect_norm(tl, x, b_host):
    """||b - A x|| with ddm_op_apply and ddm_norm"""
    y = tl.zeros(tl.rl.n_o)
    tl.op.apply(x, y)
    r = tl.to_device(np.asarray(b_host, dtype=np.float64)) - y
    return tl.op.norm(r)


@pytest.mark.parametrize("key", sorted(CONFIGS))
def test_single_vector_matches_restatement_and_true_defect(ddm, references, key):
    """restart = 6, maxit = 200, reduction 1e-10 on poisson12_2x2x2 (POU coarse space; restricted + multiplicative, standard + additive)
    and dg32_2x2 (umfpack local solves): iteration count and converged flag equal to the restatement's, history within
    1e-7 |r_k| + 1e-11 |r_0|.

    How far the restatement itself moves when nothing but the order of the additions in its dots changes (ascending / descending /
    pairwise, as tests/test_oracle_order_sensitivity.py does for CG), measured on these three inputs: the same iteration counts
    (13, 36, 22) and max_k |r_k' - r_k| / |r_k| = 6.0e-10, 3.4e-13, 3.2e-11, all in the last iterations, where the rule is dominated by
    1e-11 |r_0|: the rule is 2.4e5, 3.7e6 and 9.1e4 times the deviation at the iteration where that ratio is smallest (>= 4 required).

    Then the true defect: ||b - A x|| recomputed with ddm_op_apply and ddm_norm agrees with res.reduction def0 within
    TRUE_DEFECT_TOL def0 and is below reduction def0, while ddm_gmres_solve on the same problem reports a reduction (of the
    preconditioned defect) that its own recomputed true reduction does not agree with."""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    kind, okw, tkw = CONFIGS[key]
    dec = problem(ddm, kind)
    it, conv, hist_ref, red_ref, x_ref = references(key)
    tl = TwoLevelSchwarz(dec, **tkw)
    res, hist, x = tl.solve(reduction=REDUCTION, maxit=MAXIT, solver=SOLVER, restart=RESTART)
    tl.prec.check_status()
    print(key, "iterations", res.iterations, it, "reduction", res.reduction, red_ref,
          "history deviation / rule", float(np.max(np.abs(hist[:it + 1] - hist_ref) / (RTOL_HIST * hist_ref + ATOL_HIST * hist_ref[0]))) if res.iterations == it else None)
    assert conv and it > 2 * RESTART                                                       # several cycles
    assert res.iterations == it and res.converged == 1
    assert len(hist) == it + 1 and bool((np.abs(hist - hist_ref) <= RTOL_HIST * hist_ref + ATOL_HIST * hist_ref[0]).all())
    want = np.concatenate(x_ref)
    assert np.max(np.abs(x.cpu().numpy() - want)) <= 1e-7 * np.max(np.abs(want))
    # the true defect
    true = _true_defect_norm(tl, x, tl.rl.b)
    print(key, "true defect / def0", true / res.def0, "reported", res.reduction, "difference", abs(true / res.def0 - res.reduction))
    assert res.reduction == hist[-1] / hist[0] and res.def0 == hist[0]
    assert abs(true - res.reduction * res.def0) <= TRUE_DEFECT_TOL * res.def0
    assert true < REDUCTION * res.def0
    # left-preconditioned GMRES tests another quantity
    res_g, hist_g, x_g = tl.solve(reduction=REDUCTION, maxit=MAXIT, solver="restartedgmressolver", restart=RESTART)
    b_norm = tl.op.norm(tl.to_device(np.asarray(tl.rl.b, dtype=np.float64)))
    true_g = _true_defect_norm(tl, x_g, tl.rl.b) / b_norm
    print(key, "GMRES: reported reduction", res_g.reduction, "true reduction", true_g)
    assert res_g.converged and b_norm == res.def0
    assert abs(true_g - res_g.reduction) > TRUE_DEFECT_TOL
    tl.ctx.close()


# ---- 3: block against single -------------------------------------------------------------------------------------------------------------
TINY = 2.0 ** -83     # about 1e-25: a column scaled by it is stopped by the absolute test norm < 1e-30 after about half the iterations


class Shapes:
    """the (13, 12, 11) grid of tests/test_gpu_apply_shapes.py, restricted Schwarz (ILU(0)) + POU coarse level, additive; 32 fixed
    columns: the problem's right-hand side, a zero column, seeded random consistent vectors of which every third is scaled by 2^-83.
    A block of width m is made of the first m columns; single-vector solves are computed once per column."""

    def __init__(self, ddm):
        from dune_ddm_amd.solver import TwoLevelSchwarz
        self.ddm = ddm
        self.dec = _build(ddm, (13, 12, 11), (2, 2, 2))
        self.tl = TwoLevelSchwarz(self.dec, coarse="pou", schwarz_type="restricted", mode="additive")
        B = _consistent_block(self.tl, self.dec, 32, seed=23)
        B[:, 0] = np.asarray(self.tl.rl.b, dtype=np.float64)
        B[:, 1] = 0.0
        B[:, 2::3] *= TINY
        self.B = B
        self._single = {}

    def single(self, c):
        if c not in self._single:
            tl = self.tl
            bd = tl.to_device(self.B[:, c].copy())
            x = tl.zeros(tl.rl.n_o)
            res, hist = self.ddm.fgmres_solve(tl.ctx, tl.op, tl.prec, x, bd, REDUCTION, MAXIT, RESTART, True)
            self._single[c] = (res.iterations, res.converged, res.reduction, hist.copy(), x.cpu().numpy())
        return self._single[c]

    def block(self, cols, maxit=MAXIT):
        import torch
        tl = self.tl
        Bd = tl.to_device(np.ascontiguousarray(self.B[:, cols])).contiguous().clone()
        X = torch.zeros_like(Bd)
        res, hist = self.ddm.fgmres_solve_multi(tl.ctx, tl.op, tl.prec, X, Bd, REDUCTION, maxit, RESTART, True)
        return res, hist, X, Bd


@pytest.fixture(scope="module")
def shapes(ddm):
    s = Shapes(ddm)
    yield s
    s.tl.prec.check_status()
    s.tl.ctx.close()


@pytest.mark.parametrize("m", WIDTHS)
def test_block_matches_single(ddm, shapes, m):
    """m = 1, 3, 8, 13, 32 (the widths at which the 8 / 4 / 2 / 1 column groups of the block kernels change), restart = 6, columns that
    stop in different restart cycles.  Per column: iteration count and flag equal to ddm_fgmres_solve's, x within 2e-14 of its largest
    entry, the history under the GMRES rule.  A frozen column's x, history tail and column of B are those of a run that ends where it
    stopped, bit for bit; a permutation of the columns and a second solve are bitwise identical; the zero column reports converged with
    0 iterations and is never touched."""
    import torch
    cols = list(range(m))
    res, hist, X, Bd = shapes.block(cols)
    Xh = X.cpu().numpy()
    its = [r.iterations for r in res]
    print("m", m, "iterations", its)
    assert hist.shape == (max(its) + 1, m)
    for c in cols:
        if c == 1:
            continue
        it1, conv1, red1, h1, x1 = shapes.single(c)
        dev = float(np.max(np.abs(Xh[:, c] - x1)) / np.max(np.abs(x1)))
        print("  column", c, "iterations", its[c], it1, "x deviation", dev)
        assert its[c] == it1 and res[c].converged == conv1 == 1, (c, its[c], it1)
        assert dev <= XTOL_BLOCK, (c, dev)
        hc = hist[:its[c] + 1, c]
        assert bool((np.abs(hc - h1) <= RTOL_HIST * h1 + ATOL_HIST * h1[0]).all()), c
        assert np.isnan(hist[its[c] + 1:, c]).all()                                      # the history tail is never written
    if m >= 3:
        assert its[1] == 0 and res[1].converged == 1 and res[1].def0 == 0.0
        assert not np.any(Xh[:, 1]) and not torch.any(Bd[:, 1]) and hist[0, 1] == 0.0 and np.isnan(hist[1:, 1]).all()
        cycles = {(i - 1) // RESTART for c, i in enumerate(its) if c != 1}
        assert len(cycles) >= 2, its                                                    # columns stop in different restart cycles
        # frozen: the earliest column, in a run that ends at its last iteration, against the full run (where it sat frozen through
        # the later iterations and restarts)
        early = min((c for c in cols if c != 1), key=lambda c: its[c])
        assert (its[early] - 1) // RESTART < (max(its) - 1) // RESTART
        res2, hist2, X2, Bd2 = shapes.block(cols, maxit=its[early])
        assert res2[early].converged == 1 and res2[early].iterations == its[early]
        assert torch.equal(X2[:, early], X[:, early]) and torch.equal(Bd2[:, early], Bd[:, early])
        assert np.array_equal(hist2[:, early], hist[:its[early] + 1, early])
        for c in cols:
            if its[c] > its[early]:
                assert res2[c].converged == 0 and res2[c].iterations == its[early], c
                assert np.array_equal(hist2[:, c], hist[:its[early] + 1, c])
    perm = list(np.random.default_rng(m).permutation(m))
    resp, histp, Xp, Bp = shapes.block(perm)
    assert [r.iterations for r in resp] == [its[p] for p in perm]
    assert np.array_equal(Xp.cpu().numpy(), Xh[:, perm]) and np.array_equal(histp, hist[:, perm], equal_nan=True) and torch.equal(Bp, Bd[:, perm])
    res3, hist3, X3, Bd3 = shapes.block(cols)
    assert torch.equal(X3, X) and torch.equal(Bd3, Bd) and np.array_equal(hist3, hist, equal_nan=True)


# ---- 4: the fused restart kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3, 8, 13])
def test_fused_restart_kernel_matches_its_composition(ddm, shapes, m):
    """k_defect_norm_multi (B -= T in the active columns, partial sums of <B_c, B_c> in the same pass) against the kernels it replaces
    (AXPY with unit coefficients, ddm_dot_multi) on the same inputs, one column masked (for m = 1: once active, once masked): B and
    the squared norms are bitwise equal, the masked column of B is untouched, and B is what the element-wise subtraction gives."""
    import torch
    tl = shapes.tl
    T0 = tl.to_device(_consistent_block(tl, shapes.dec, m, seed=31)).contiguous()
    B0 = tl.to_device(_consistent_block(tl, shapes.dec, m, seed=37)).contiguous()
    masks = [[1], [0]] if m == 1 else [[0 if c == m // 2 else 1 for c in range(m)]]
    for active in masks:
        Bf, Bu = B0.clone(), B0.clone()
        nf = ddm.fgmres_defect_multi(tl.ctx, tl.op, active, T0, Bf, fused=True)
        nu = ddm.fgmres_defect_multi(tl.ctx, tl.op, active, T0, Bu, fused=False)
        on = torch.tensor(active, device=B0.device, dtype=torch.bool)
        want = torch.where(on[None, :], B0 - T0, B0)
        assert torch.equal(Bf, Bu) and torch.equal(Bf, want)
        assert np.array_equal(nf, nu) and np.array_equal(nf, tl.op.dot_multi(want, want))
        assert np.all(nf > 0)


# ---- 5: a preconditioner that changes ------------------------------------------------------------------------------------------------------
def test_single_precision_local_solves_as_preconditioner(ddm, shapes):
    """ddm_schwarz_set_multi_precision(S, 1) on the ILU(0) Poisson problem at m = 8 (random consistent right-hand sides): the local
    solves run in single precision, the flexible driver still converges to a RECOMPUTED true reduction below 1e-10 in every column.
    Switching back to 0 reproduces the double run bit for bit.
    Iterations per column, recorded on an MI355X: double 17, 18, 18, 18, 18, 18, 18, 18; single precision the same eight counts (the
    single-precision sweeps perturb the preconditioner by ~1e-6, far below what changes an iteration count here); recomputed true
    reductions 1.8e-11 to 9.9e-11.  No ratio is asserted."""
    import torch
    tl = shapes.tl
    Bh = _consistent_block(tl, shapes.dec, 8, seed=41)

    def run():
        Bd = tl.to_device(Bh.copy()).contiguous().clone()
        X = torch.zeros_like(Bd)
        res, hist = ddm.fgmres_solve_multi(tl.ctx, tl.op, tl.prec, X, Bd, REDUCTION, MAXIT, RESTART, True)
        return res, hist, X

    def true_reductions(X):
        Y = torch.zeros_like(X)
        tl.op.apply_multi(X, Y)
        B0 = tl.to_device(Bh.copy()).contiguous()
        R = B0 - Y
        return np.sqrt(tl.op.dot_multi(R, R) / tl.op.dot_multi(B0, B0))

    res_d, hist_d, X_d = run()
    tl.schwarz.set_multi_precision(True)
    try:
        res_s, hist_s, X_s = run()
    finally:
        tl.schwarz.set_multi_precision(False)
    res_d2, hist_d2, X_d2 = run()
    red_s = true_reductions(X_s)
    print("iterations double", [r.iterations for r in res_d], "single precision", [r.iterations for r in res_s], "true reductions", red_s)
    assert all(r.converged for r in res_d) and all(r.converged for r in res_s)
    assert not torch.equal(X_s, X_d)                                                    # the switch reached the local solve
    assert np.all(red_s < REDUCTION)
    assert np.all(np.abs(red_s - np.array([r.reduction for r in res_s])) <= TRUE_DEFECT_TOL)
    assert torch.equal(X_d2, X_d) and np.array_equal(hist_d2, hist_d, equal_nan=True)
    assert [r.iterations for r in res_d2] == [r.iterations for r in res_d]


# ---- 6: errors --------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_host_side_refusals(ddm, shapes):
    """DDM_EINVAL before any device work (a poisoned X stays poisoned, B stays the right-hand side), DDM_ENOTIMPL with the byte count for
    two bases larger than the free device memory (a restart computed from hipMemGetInfo, nothing of that size is allocated), and a set
    local-solve status word; the context works afterwards."""
    import torch
    tl = shapes.tl
    lib, h = tl.ctx.lib, tl.ctx.h
    m = 4
    Bh = np.ascontiguousarray(shapes.B[:, [0, 3, 4, 6]])
    n_o = Bh.shape[0]
    res = (ddm.SolveResult * 33)()
    B0 = tl.to_device(Bh.copy()).contiguous()
    Bd = B0.clone()
    X = torch.full_like(Bd, 123.456)
    poison = X.clone()

    def multi(nrhs, Xp, Bp, maxit, restart, resp=res):
        rc = lib.ddm_fgmres_solve_multi(h, tl.op.h, tl.prec.h, nrhs, Xp, Bp, 1e-10, maxit, restart, None, resp)
        tl.ctx.sync()
        return rc, lib.ddm_last_error(h).decode()

    for args in [(0, X.data_ptr(), Bd.data_ptr(), 50, 6), (33, X.data_ptr(), Bd.data_ptr(), 50, 6), (m, X.data_ptr(), Bd.data_ptr(), 50, 0),
                 (m, X.data_ptr(), Bd.data_ptr(), -1, 6), (m, X.data_ptr(), X.data_ptr(), 50, 6), (m, None, Bd.data_ptr(), 50, 6),
                 (m, X.data_ptr(), None, 50, 6)]:
        rc, msg = multi(*args)
        assert rc == ddm.DDM_EINVAL and "ddm_fgmres_solve_multi" in msg, (args, rc, msg)
    assert multi(m, X.data_ptr(), Bd.data_ptr(), 50, 6, None)[0] == ddm.DDM_EINVAL
    x1, b1 = X[:, 0].contiguous(), Bd[:, 0].contiguous()
    for args in [(x1.data_ptr(), b1.data_ptr(), 50, 0), (x1.data_ptr(), b1.data_ptr(), -1, 6), (x1.data_ptr(), x1.data_ptr(), 50, 6), (None, b1.data_ptr(), 50, 6)]:
        assert lib.ddm_fgmres_solve(h, tl.op.h, tl.prec.h, args[0], args[1], 1e-10, args[2], args[3], None, res) == ddm.DDM_EINVAL
        assert "ddm_fgmres_solve:" in lib.ddm_last_error(h).decode()
    tl.ctx.sync()
    assert torch.equal(X, poison) and torch.equal(Bd, B0) and torch.equal(x1, poison[:, 0]) and torch.equal(b1, B0[:, 0])

    free, total = torch.cuda.mem_get_info()
    big = int(free // (2 * n_o * m * 8)) + 1                                   # 2 big + 2 blocks of n_o x m doubles exceed the free memory
    need = (2 * big + 2) * n_o * m * 8
    assert need > free and big < 2**31 - 8
    rc, msg = multi(m, X.data_ptr(), Bd.data_ptr(), big, big)
    assert rc == ddm.DDM_ENOTIMPL and "bytes" in msg and "ddm_fgmres_solve_multi" in msg and str(need) in msg, msg
    big1 = int(free // (2 * n_o * 8)) + 1
    if big1 < 2**31 - 8:
        rc = lib.ddm_fgmres_solve(h, tl.op.h, tl.prec.h, x1.data_ptr(), b1.data_ptr(), 1e-10, big1, big1, None, res)
        msg = lib.ddm_last_error(h).decode()
        assert rc == ddm.DDM_ENOTIMPL and str((2 * big1 + 2) * n_o * 8) in msg and "ddm_fgmres_solve:" in msg, msg
    tl.ctx.sync()
    assert torch.cuda.mem_get_info()[0] >= free - (64 << 20)                   # nothing of that size was allocated
    assert torch.equal(X, poison) and torch.equal(Bd, B0)

    F = ctypes.c_void_p(tl.schwarz.local_solver())
    assert lib.ddm_ilu0_set_status(F, 1) == ddm.DDM_OK
    try:
        rc, msg = multi(m, X.data_ptr(), Bd.data_ptr(), 50, 6)
        assert rc == ddm.DDM_ENUMERIC
        assert lib.ddm_fgmres_solve(h, tl.op.h, tl.prec.h, x1.data_ptr(), b1.data_ptr(), 1e-10, 50, 6, None, res) == ddm.DDM_ENUMERIC
        tl.ctx.sync()
        assert torch.equal(X, poison) and torch.equal(Bd, B0)                  # refused on entry: nothing was launched
    finally:
        assert lib.ddm_ilu0_set_status(F, 0) == ddm.DDM_OK
    Bnan = Bh.copy()
    Bnan[7, 1] = np.nan
    Bn = tl.to_device(Bnan).contiguous()
    Xn = torch.zeros_like(Bn)
    rc, msg = multi(m, Xn.data_ptr(), Bn.data_ptr(), 50, 6)
    assert rc == ddm.DDM_ENUMERIC and "column 1" in msg and "ddm_fgmres_solve_multi" in msg, msg
    X.zero_()                                                                   # the context is still usable
    rc, msg = multi(m, X.data_ptr(), Bd.data_ptr(), MAXIT, RESTART)
    assert rc == ddm.DDM_OK and all(res[c].converged for c in range(m)), msg
