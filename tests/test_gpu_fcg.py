"""-m gpu: flexible CG on the device (ddm_fcg_solve, ddm_fcg_solve_multi; restarted and complete) against the numpy restatement of the
algorithm (tests/fcg_reference.py, checked on the CPU by tests/test_fcg_cpu.py) and against the recomputed true defect, the fused
orthogonalisation kernels against the composition they replace, the block driver against the single-vector one, the single-precision
local solve as a preconditioner that changes, and maxit shorter than one pass over the slots.

Tolerances: histories under the project's GMRES rule (1e-7 |r_k| + 1e-11 |r_0|; tests/test_fcg_cpu.py::test_summation_order_sensitivity
shows it is >= 2e5 times what another summation order moves these runs); reported against recomputed defect norm 1e-14 def0
(FCG_TRUE_DEFECT_TOL, measured there: 1.9e-16 at most); block against single x 2e-14 relative (the block-GMRES figure).  Everything that
compares a kernel with its composition, or the block driver with itself, is bitwise."""
import numpy as np
import pytest

from tests.test_fcg_cpu import CONFIGS, FCG_TRUE_DEFECT_TOL, MAXIT, REDUCTION, SETTINGS
from tests.test_fgmres_cpu import golden_poisson
from tests.test_gpu_fgmres import WIDTHS, XTOL_BLOCK, Shapes, _true_defect_norm
from tests.test_gpu_multi_gmres import ATOL_HIST, RTOL_HIST
from tests.test_gpu_multi_rhs import _consistent_block

pytestmark = pytest.mark.gpu

NAMES = {False: "restartedfcgsolver", True: "completefcgsolver"}
MMAX = 3


# ---- 1: one right-hand side against the restatement ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(ddm):
    """the 12^3 golden problem, one device object per configuration (built on first use), the restatement's runs computed once"""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    from tests.fcg_reference import reference_solve
    dec = golden_poisson(ddm)
    tls, refs = {}, {}

    def tl(key):
        if key not in tls:
            tls[key] = TwoLevelSchwarz(dec, **CONFIGS[key][1])
        return tls[key]

    def ref(key, mmax, complete):
        if (key, mmax, complete) not in refs:
            refs[key, mmax, complete] = reference_solve(dec, REDUCTION, MAXIT, mmax, complete, **CONFIGS[key][0])
        return refs[key, mmax, complete]
    yield tl, ref
    for t in tls.values():
        t.prec.check_status()
        t.ctx.close()


@pytest.mark.parametrize("mmax, complete", SETTINGS)
@pytest.mark.parametrize("key", sorted(CONFIGS))
def test_single_vector_matches_restatement_and_true_defect(ddm, golden, key, mmax, complete):
    """reduction 1e-10, maxit 200 on poisson12_2x2x2 with the POU coarse space: standard + additive (a symmetric preconditioner),
    restricted + additive and restricted + multiplicative; mmax = 3 restarted (slot 0 <-> slot 3 swapped several times), mmax = 3
    complete (wraps with stale higher slots in the window) and mmax = 1 restarted (slots 0 and 1 swapped).  Iteration count and
    converged flag equal to the restatement's, the history within 1e-7 |r_k| + 1e-11 |r_0|, x within 1e-7 of its largest entry; the
    true defect ||b - A x||, recomputed with ddm_op_apply and ddm_norm, agrees with res.reduction def0 within 1e-14 def0 (the bound
    measured on the CPU) and is below reduction def0."""
    tl_of, ref_of = golden
    tl = tl_of(key)
    it, conv, hist_ref, red_ref, x_ref = ref_of(key, mmax, complete)
    res, hist, x = tl.solve(reduction=REDUCTION, maxit=MAXIT, solver=NAMES[complete], mmax=mmax)
    tl.prec.check_status()
    print(key, "mmax", mmax, "complete", complete, "iterations", res.iterations, it, "reduction", res.reduction, red_ref,
          "history deviation / rule", float(np.max(np.abs(hist[:it + 1] - hist_ref) / (RTOL_HIST * hist_ref + ATOL_HIST * hist_ref[0]))) if res.iterations == it else None)
    assert conv and it > 2 * (mmax + 1)                                                    # several passes over the slots
    assert res.iterations == it and res.converged == 1
    assert len(hist) == it + 1 and bool((np.abs(hist - hist_ref) <= RTOL_HIST * hist_ref + ATOL_HIST * hist_ref[0]).all())
    want = np.concatenate(x_ref)
    assert np.max(np.abs(x.cpu().numpy() - want)) <= 1e-7 * np.max(np.abs(want))
    true = _true_defect_norm(tl, x, tl.rl.b)
    print(key, "true defect / def0", true / res.def0, "reported", res.reduction, "difference", abs(true / res.def0 - res.reduction))
    assert res.reduction == hist[-1] / hist[0] and res.def0 == hist[0]
    assert abs(true - res.reduction * res.def0) <= FCG_TRUE_DEFECT_TOL * res.def0
    assert true < REDUCTION * res.def0


# ---- 2, 3, 4, 5: the (13, 12, 11) grid -----------------------------------------------------------------------------------------------------
class FcgShapes(Shapes):
    """Shapes of tests/test_gpu_fgmres.py -- the (13, 12, 11) grid of tests/test_gpu_apply_shapes.py (n_o is no multiple of the 1024
    rows a workgroup of the reductions takes), restricted Schwarz (ILU(0)) + POU coarse level, additive; 32 fixed columns: the
    problem's right-hand side, a zero column, seeded random consistent vectors of which every third is scaled by 2^-83 -- solved by
    flexible CG with mmax = 3.  Single-vector solves are computed once per (column, variant)."""

    def single(self, c, complete):
        if (c, complete) not in self._single:
            tl = self.tl
            bd = tl.to_device(self.B[:, c].copy())
            x = tl.zeros(tl.rl.n_o)
            res, hist = self.ddm.fcg_solve(tl.ctx, tl.op, tl.prec, x, bd, REDUCTION, MAXIT, MMAX, complete, True)
            self._single[c, complete] = (res.iterations, res.converged, res.reduction, hist.copy(), x.cpu().numpy())
        return self._single[c, complete]

    def block(self, cols, complete, maxit=MAXIT, B=None, X0=None):
        import torch
        tl = self.tl
        Bd = tl.to_device(np.ascontiguousarray((self.B if B is None else B)[:, cols])).contiguous().clone()
        X = torch.zeros_like(Bd) if X0 is None else X0.clone()
        res, hist = self.ddm.fcg_solve_multi(tl.ctx, tl.op, tl.prec, X, Bd, REDUCTION, maxit, MMAX, complete, True)
        return res, hist, X, Bd


@pytest.fixture(scope="module")
def shapes(ddm):
    s = FcgShapes(ddm)
    yield s
    s.tl.prec.check_status()
    s.tl.ctx.close()


@pytest.mark.parametrize("m", WIDTHS)
@pytest.mark.parametrize("nslots", [0, 1, 2, 5, 11])
def test_fused_orthogonalisation_matches_its_composition(ddm, shapes, nslots, m):
    """ddm_fcg_orth_multi: k_fcg_project_multi (one pass over W for 4 slots x the columns of a group), one all-reduce, k_fcg_coef_multi
    and k_fcg_orth_multi (one read-modify-write of W) against the composition (ddm_dot_multi's kernel per slot on the unmodified W,
    the same coefficient kernel, k_axpy_negdev_multi per slot).  nslots = 0, 1, 2, 5, 11: below the slot group of 4, across it, and
    two full groups with a remainder; m = 1, 3, 8, 13, 32: every column group 8 / 4 / 2 / 1; all columns active, then with frozen
    columns (every third, from the first; for m = 1 the one column).  W and the coefficients are bitwise equal, frozen columns of W
    bitwise untouched and their coefficients 0.  Against the formula: each coefficient is <Ad_k, W> (ddm_dot_multi on the W passed in,
    bitwise the numerator) / g_k within 2 eps relative, and W is W0 - sum_k coef_k d_k in ascending k within 8 eps (nslots + 1) (max|W0| + sum_k max|coef_k| max|d_k|)."""
    import torch
    tl = shapes.tl
    n = tl.rl.n_o
    rng = np.random.default_rng(1000 * nslots + m)
    W0 = tl.to_device(_consistent_block(tl, shapes.dec, m, seed=51 + m)).contiguous()
    AD = tl.to_device(rng.standard_normal((max(nslots, 1), n, m))).contiguous()[:nslots]
    DS = tl.to_device(rng.standard_normal((max(nslots, 1), n, m))).contiguous()[:nslots]
    g = rng.uniform(0.5, 2.0, (nslots, m)) * np.where(rng.random((nslots, m)) < 0.3, -1.0, 1.0)
    eps = np.finfo(float).eps
    for active in ([1] * m, [0 if c % 3 == 0 else 1 for c in range(m)]):
        Wf, Wu = W0.clone(), W0.clone()
        cf = ddm.fcg_orth_multi(tl.ctx, tl.op, active, AD if nslots else None, DS if nslots else None, g, Wf, fused=True)
        cu = ddm.fcg_orth_multi(tl.ctx, tl.op, active, AD if nslots else None, DS if nslots else None, g, Wu, fused=False)
        on = np.array(active, dtype=bool)
        assert cf.shape == (nslots, m) and np.array_equal(cf, cu) and torch.equal(Wf, Wu)
        assert torch.equal(Wf[:, ~torch.tensor(on)], W0[:, ~torch.tensor(on)])               # frozen columns: bitwise untouched
        assert not np.any(cf[:, ~on])
        want = W0.clone()
        for k in range(nslots):
            num = tl.op.dot_multi(AD[k].contiguous(), W0)
            ck = num / g[k]
            assert np.all(np.abs(cf[k, on] - ck[on]) <= 2 * eps * np.abs(ck[on])), k
            term = DS[k] * torch.as_tensor(np.where(on, cf[k], 0.0), device=W0.device)[None, :]
            want = want - term
        scale = float(W0.abs().max()) + sum(float(np.abs(cf[k]).max()) * float(DS[k].abs().max()) for k in range(nslots))
        assert float((Wf - want).abs().max()) <= 8 * eps * (nslots + 1) * scale
        if nslots and on.any():
            assert not torch.equal(Wf[:, torch.tensor(on)], W0[:, torch.tensor(on)])


@pytest.mark.parametrize("complete", [False, True])
@pytest.mark.parametrize("m", WIDTHS)
def test_block_matches_single(ddm, shapes, m, complete):
    """m = 1, 3, 8, 13, 32 (the widths at which the 8 / 4 / 2 / 1 column groups of the block kernels change), mmax = 3, both variants,
    columns that stop in different iterations.  Per column: iteration count and flag equal to ddm_fcg_solve's, x within 2e-14 of its
    largest entry, the history under the rule.  The zero column reports converged with 0 iterations and is never touched; a column
    that stopped early is, in a run that ends at its last iteration, bit for bit what it is in the full run (nothing writes it while
    it sits frozen); a permutation of the columns and a second solve are bitwise identical."""
    import torch
    cols = list(range(m))
    res, hist, X, Bd = shapes.block(cols, complete)
    Xh = X.cpu().numpy()
    its = [r.iterations for r in res]
    print("m", m, "complete", complete, "iterations", its)
    assert hist.shape == (max(its) + 1, m)
    for c in cols:
        if c == 1:
            continue
        it1, conv1, red1, h1, x1 = shapes.single(c, complete)
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
        early = min((c for c in cols if c != 1), key=lambda c: its[c])
        assert its[early] < max(its), its                                                # columns stop in different iterations
        res2, hist2, X2, Bd2 = shapes.block(cols, complete, maxit=its[early])
        assert res2[early].converged == 1 and res2[early].iterations == its[early]
        assert torch.equal(X2[:, early], X[:, early]) and torch.equal(Bd2[:, early], Bd[:, early])
        assert np.array_equal(hist2[:, early], hist[:its[early] + 1, early])
        for c in cols:
            if its[c] > its[early]:
                assert res2[c].converged == 0 and res2[c].iterations == its[early], c
                assert np.array_equal(hist2[:, c], hist[:its[early] + 1, c])
    perm = list(np.random.default_rng(m).permutation(m))
    resp, histp, Xp, Bp = shapes.block(perm, complete)
    assert [r.iterations for r in resp] == [its[p] for p in perm]
    assert np.array_equal(Xp.cpu().numpy(), Xh[:, perm]) and np.array_equal(histp, hist[:, perm], equal_nan=True) and torch.equal(Bp, Bd[:, perm])
    res3, hist3, X3, Bd3 = shapes.block(cols, complete)
    assert torch.equal(X3, X) and torch.equal(Bd3, Bd) and np.array_equal(hist3, hist, equal_nan=True)


@pytest.mark.parametrize("complete", [False, True])
def test_single_precision_local_solves_as_preconditioner(ddm, shapes, complete):
    """ddm_schwarz_set_multi_precision(S, 1) on the ILU(0) Poisson problem at m = 8, mmax = 3 (random consistent right-hand sides): the
    local solves run in single precision -- a preconditioner that is not the one of the double run --, every column still converges to
    a RECOMPUTED true reduction below 1e-10 that agrees with the reported one within 1e-14.  Switching back reproduces the double run
    bit for bit.  No iteration count or ratio is asserted."""
    import torch
    tl = shapes.tl
    Bh = _consistent_block(tl, shapes.dec, 8, seed=41)
    cols = list(range(8))

    def true_reductions(X):
        Y = torch.zeros_like(X)
        tl.op.apply_multi(X, Y)
        B0 = tl.to_device(Bh.copy()).contiguous()
        R = B0 - Y
        return np.sqrt(tl.op.dot_multi(R, R) / tl.op.dot_multi(B0, B0))

    res_d, hist_d, X_d, _ = shapes.block(cols, complete, B=Bh)
    tl.schwarz.set_multi_precision(True)
    try:
        res_s, hist_s, X_s, _ = shapes.block(cols, complete, B=Bh)
    finally:
        tl.schwarz.set_multi_precision(False)
    res_d2, hist_d2, X_d2, _ = shapes.block(cols, complete, B=Bh)
    red_s = true_reductions(X_s)
    print("complete", complete, "iterations double", [r.iterations for r in res_d], "single precision", [r.iterations for r in res_s], "true reductions", red_s)
    assert all(r.converged for r in res_d) and all(r.converged for r in res_s)
    assert not torch.equal(X_s, X_d)                                                    # the switch reached the local solve
    assert np.all(red_s < REDUCTION)
    assert np.all(np.abs(red_s - np.array([r.reduction for r in res_s])) <= FCG_TRUE_DEFECT_TOL)
    assert torch.equal(X_d2, X_d) and np.array_equal(hist_d2, hist_d, equal_nan=True)
    assert [r.iterations for r in res_d2] == [r.iterations for r in res_d]


@pytest.mark.parametrize("complete", [False, True])
def test_maxit_shorter_than_a_pass_and_zero(ddm, shapes, complete):
    """maxit = 2 < mmax + 1 = 4 (the loop ends inside the first pass; only min(mmax, maxit) + 1 slots exist) and maxit = 0, single
    vector and block (m = 3: a running column, the zero column, a scaled column): iterations = maxit, converged = 0, maxit + 1 history
    entries that are bitwise the first of the full run; with maxit = 0 x stays what it was and b becomes the defect b - A x."""
    import torch
    tl = shapes.tl
    cols = [0, 1, 2]
    full_res, full_hist, full_X, _ = shapes.block(cols, complete)
    for maxit in (2, 0):
        res, hist, X, Bd = shapes.block(cols, complete, maxit=maxit)
        assert hist.shape == (maxit + 1, 3)
        for c in (0, 2):
            assert res[c].iterations == maxit and res[c].converged == 0
            assert np.array_equal(hist[:, c], full_hist[:maxit + 1, c])
            assert res[c].reduction == hist[maxit, c] / hist[0, c]
        assert res[1].iterations == 0 and res[1].converged == 1
        if maxit == 0:
            assert not torch.any(X)
        else:
            assert torch.any(X[:, 0]) and not torch.any(X[:, 1])
        bd = tl.to_device(shapes.B[:, 0].copy())
        x = tl.zeros(tl.rl.n_o)
        r1, h1 = ddm.fcg_solve(tl.ctx, tl.op, tl.prec, x, bd, REDUCTION, maxit, MMAX, complete, True)
        it_full, conv_full, red_full, h_full, x_full = shapes.single(0, complete)
        assert r1.iterations == maxit and r1.converged == 0 and len(h1) == maxit + 1 and np.array_equal(h1, h_full[:maxit + 1])
        if maxit == 0:
            assert not torch.any(x) and torch.equal(bd, tl.to_device(shapes.B[:, 0].copy()))
    # x untouched means untouched: a start vector survives maxit = 0, and b is then b - A x
    X0 = tl.to_device(_consistent_block(tl, shapes.dec, 3, seed=61)).contiguous()
    res, hist, X, Bd = shapes.block(cols, complete, maxit=0, X0=X0)
    Y = torch.zeros_like(X0)
    tl.op.apply_multi(X0, Y)
    assert torch.equal(X, X0) and all(r.iterations == 0 and r.converged == 0 for r in res)
    want = tl.to_device(np.ascontiguousarray(shapes.B[:, cols])) - Y
    assert float((Bd - want).abs().max()) <= 1e-13 * float(want.abs().max())


def test_refusals(ddm, shapes):
    """DDM_EINVAL before any device work with live handles (x == b, mmax = 0, maxit = -1, nrhs = 33: a poisoned X stays poisoned), and
    DDM_ENOTIMPL with the byte count for 2 (mmax + 1) blocks larger than the free device memory (nothing of that size is allocated)."""
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

    def multi(nrhs, Xp, Bp, maxit, mmax):
        rc = lib.ddm_fcg_solve_multi(h, tl.op.h, tl.prec.h, nrhs, Xp, Bp, 1e-10, maxit, mmax, 0, None, res)
        tl.ctx.sync()
        return rc, lib.ddm_last_error(h).decode()

    for args in [(0, X.data_ptr(), Bd.data_ptr(), 50, 3), (33, X.data_ptr(), Bd.data_ptr(), 50, 3), (m, X.data_ptr(), Bd.data_ptr(), 50, 0),
                 (m, X.data_ptr(), Bd.data_ptr(), -1, 3), (m, X.data_ptr(), X.data_ptr(), 50, 3), (m, None, Bd.data_ptr(), 50, 3)]:
        rc, msg = multi(*args)
        assert rc == ddm.DDM_EINVAL and "ddm_fcg_solve_multi" in msg, (args, rc, msg)
    x1, b1 = X[:, 0].contiguous(), Bd[:, 0].contiguous()
    for args in [(x1.data_ptr(), b1.data_ptr(), 50, 0), (x1.data_ptr(), b1.data_ptr(), -1, 3), (x1.data_ptr(), x1.data_ptr(), 50, 3)]:
        assert lib.ddm_fcg_solve(h, tl.op.h, tl.prec.h, args[0], args[1], 1e-10, args[2], args[3], 1, None, res) == ddm.DDM_EINVAL
        assert "ddm_fcg_solve:" in lib.ddm_last_error(h).decode()
    tl.ctx.sync()
    assert torch.equal(X, poison) and torch.equal(Bd, B0)
    free, total = torch.cuda.mem_get_info()
    big = int(free // (2 * n_o * m * 8)) + 1                                   # 2 (big + 1) blocks of n_o x m doubles exceed the free memory
    need = 2 * (big + 1) * n_o * m * 8
    assert need > free and big < 2**31 - 8
    rc, msg = multi(m, X.data_ptr(), Bd.data_ptr(), big, big)
    assert rc == ddm.DDM_ENOTIMPL and "bytes" in msg and "ddm_fcg_solve_multi" in msg and str(need) in msg, msg
    tl.ctx.sync()
    assert torch.cuda.mem_get_info()[0] >= free - (64 << 20)                   # nothing of that size was allocated
    assert torch.equal(X, poison) and torch.equal(Bd, B0)
