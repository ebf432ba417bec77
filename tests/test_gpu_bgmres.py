"""-m gpu: block GMRES on the device (ddm_bgmres_solve_multi, TwoLevelSchwarz.solve_block_gmres).  Its three kernels against numpy at the
widths and stored-block counts their layouts branch on, the driver against the numpy restatement (tests/bgmres_reference.py, checked on
the CPU by tests/test_bgmres_cpu.py) and against the recomputed true defect, and what it leaves behind for the other block drivers.

Tolerances.  Projection and Gram entries: 1e-13 sum |u||v| (the project's rule for Gram products).  Combination, per
entry: 2 (K p + 2) u (|out| + sum |V||C|), u = 2^-53 (K p products, K p - 1 additions, one more addition).  Histories: 1e-7 |r_k| +
1e-11 |r_0| (tests/test_bgmres_cpu.py::test_summation_order_sensitivity shows the rule is at least 4.6e3 times what another summation
order moves these runs).  x: 1e-8 of the restatement's largest entry.  Reported against recomputed reduction: TRUE_GAP_TOL of
tests/test_bgmres_cpu.py.  Repeated calls are bitwise equal."""
import numpy as np
import pytest

from tests.test_bgmres_cpu import MAXIT, RANK_TOL, REDUCTION, TRUE_GAP_TOL, block_degenerate, block_m8, rhs
from tests.test_fgmres_cpu import CONFIGS, problem
from tests.test_gpu_bcg import Raw, _dev, raw, small  # noqa: F401  (raw, small: fixtures)
from tests.test_gpu_multi_gmres import ATOL_HIST, RTOL_HIST

pytestmark = pytest.mark.gpu

# the thread layouts branch on odd p (the zero pad column of the staged tiles), on the row slices 256 / ceil(p / 2)^2 and on the rows per
# quarter tile 256 / p; the projection takes the stored blocks in groups of GROUP
WIDTHS = (1, 2, 3, 7, 8, 9, 16, 17, 31, 32)
GROUP = 4                                            # BGM_SG of csrc/multi_kernels.hpp
COUNTS = (1, 2, GROUP, GROUP + 1, 2 * GROUP + 1)
U_ROUND = 2.0 ** -53
L = np.longdouble


def _check_project(ddm, ctx, op, mask, n, p, K, seed):
    rng = np.random.default_rng(seed)
    V, W = rng.standard_normal((K, n, p)), rng.standard_normal((n, p))
    V[:, ~mask] = np.nan                                # rows that are not owned must not be read into the sums
    W[~mask] = np.nan
    Vd, Wd = _dev(V), _dev(W)
    H = ddm.bgmres_project_multi(ctx, op, Vd, Wd)
    H2 = ddm.bgmres_project_multi(ctx, op, Vd, Wd)
    assert H.shape == (K, p, p) and np.isfinite(H).all() and np.array_equal(H, H2)            # no atomics: bit-reproducible
    assert np.array_equal(Vd.cpu().numpy(), V, equal_nan=True) and np.array_equal(Wd.cpu().numpy(), W, equal_nan=True)
    Wo = W[mask].astype(L)
    worst = 0.0
    for k in range(K):
        Vo = V[k][mask].astype(L)
        bound = 1e-13 * np.asarray(np.abs(Vo).T @ np.abs(Wo), dtype=float)
        err = np.abs(H[k] - np.asarray(Vo.T @ Wo, dtype=float))
        worst = max(worst, float(np.max(err / bound)))
        assert (err <= bound).all(), (p, K, k, float(np.max(err / bound)))
    return worst


def _check_combine(ddm, ctx, op, n, pin, q, K, seed):
    import torch
    rng = np.random.default_rng(seed)
    V, C, O = rng.standard_normal((K, n, pin)), rng.standard_normal((K, pin, q)), rng.standard_normal((n, q))
    Vd = _dev(V)
    prod = sum(V[k].astype(L) @ C[k].astype(L) for k in range(K))
    aprod = sum(np.abs(V[k]) @ np.abs(C[k]) for k in range(K))
    worst = 0.0
    for mode, want in ((0, prod), (1, O.astype(L) + prod), (2, O.astype(L) - prod)):
        outs = []
        for _ in range(2):
            Od = _dev(np.full((n, q), np.nan)) if mode == 0 else _dev(O)          # (mode 0 must write every entry)
            ddm.bgmres_combine_multi(ctx, op, mode, Vd, C, Od)
            outs.append(Od)
        assert torch.equal(outs[0], outs[1])
        bound = 2 * (K * pin + 2) * U_ROUND * ((np.abs(O) if mode else 0.0) + aprod)
        err = np.abs(outs[0].cpu().numpy() - np.asarray(want, dtype=float))
        worst = max(worst, float(np.max(err / bound)))
        assert (err <= bound).all(), (pin, q, K, mode, float(np.max(err / bound)))
    assert torch.equal(Vd, _dev(V))
    return worst


def _check_combine_gram(ddm, ctx, op, mask, n, p, K, seed):
    import torch
    rng = np.random.default_rng(seed)
    V, C, W = rng.standard_normal((K, n, p)), rng.standard_normal((K, p, p)), rng.standard_normal((n, p))
    Vd = _dev(V)
    outs = []
    for _ in range(2):
        Wd = _dev(W)
        outs.append((Wd, ddm.bgmres_combine_gram_multi(ctx, op, Vd, C, Wd)))
    (Wd, G), (Wd2, G2) = outs
    assert torch.equal(Wd, Wd2) and np.array_equal(G, G2) and torch.equal(Vd, _dev(V))
    Wo = _dev(W)
    ddm.bgmres_combine_multi(ctx, op, 2, Vd, C, Wo)
    assert torch.equal(Wd, Wo)                                                      # the same subtraction as the kernel without the Gram
    Wn = Wd.cpu().numpy()
    Wm = Wn[mask].astype(L)
    bound = 1e-13 * np.asarray(np.abs(Wm).T @ np.abs(Wm), dtype=float)
    err = np.abs(G - np.asarray(Wm.T @ Wm, dtype=float))
    assert G.shape == (p, p) and np.isfinite(G).all() and (err <= bound).all(), (p, K, float(np.max(err / bound)))
    return float(np.max(err / bound))


@pytest.mark.parametrize("p", WIDTHS)
def test_kernels_against_numpy(ddm, small, p):
    """Projection, combination (=, +=, -=) and combination with Gram on the (13, 12, 11) grid at K = 1, 2, the group size, the group size
    + 1 and twice the group size + 1 stored blocks, against extended-precision numpy under the bounds of the module docstring; rows
    that are not owned hold NaN in the projection inputs; outputs that must be written completely are pre-filled with NaN; two identical
    calls agree bit for bit; inputs are not modified."""
    tl, mask = small
    n = tl.rl.n_o
    for K in COUNTS:
        a = _check_project(ddm, tl.ctx, tl.op, mask, n, p, K, seed=1000 + 10 * p + K)
        b = _check_combine(ddm, tl.ctx, tl.op, n, p, p, K, seed=2000 + 10 * p + K)
        c = _check_combine_gram(ddm, tl.ctx, tl.op, mask, n, p, K, seed=3000 + 10 * p + K)
        print("p", p, "K", K, "worst error / bound: project", a, "combine", b, "combine + Gram", c)


@pytest.mark.parametrize("pin, q, K", [(5, 3, 1), (32, 3, 1), (32, 17, 1), (3, 5, 1), (3, 5, 3), (3, 32, 3), (17, 32, 2)])
def test_combine_non_square(ddm, small, pin, q, K):
    """the non-square uses of the combination: V_0 = R C0 (input width m = 5, 32, output width p = 3, 17) and U = [V_0 ..] Y (input
    width p = 3, 17, output width m = 5, 32 > p)"""
    tl, mask = small
    print("pin", pin, "q", q, "K", K, "worst error / bound", _check_combine(ddm, tl.ctx, tl.op, tl.rl.n_o, pin, q, K, seed=4000 + 100 * pin + q))


def test_kernels_grid_stride(ddm, raw):
    """p = 3, K = 3 with n = 1048876 rows: every kernel's workgroups take several tiles each (grid-stride loop), the last tile partial"""
    a = _check_project(ddm, raw.ctx, raw.op, raw.mask, raw.n, 3, 3, seed=41)
    b = _check_combine(ddm, raw.ctx, raw.op, raw.n, 3, 3, 3, seed=42)
    c = _check_combine_gram(ddm, raw.ctx, raw.op, raw.mask, raw.n, 3, 3, seed=43)
    print("worst error / bound: project", a, "combine", b, "combine + Gram", c)


# ---- the driver against the restatement ------------------------------------------------------------------------------------------------
class Golden:
    """a golden problem with a non-symmetric configuration; the blocks and the restatement's runs on them, computed once"""

    def __init__(self, ddm, key):
        from dune_ddm_amd.solver import TwoLevelSchwarz
        kind, self.okw, tkw = CONFIGS[key]
        self.dec = problem(ddm, kind)
        self.tl = TwoLevelSchwarz(self.dec, **tkw)
        self.blocks = {1: [rhs(self.dec)], 5: block_degenerate(self.dec), 8: block_m8(self.dec)}
        self.refs = {}

    def host(self, cols):
        return np.stack([self.tl.rl.cat_novlp(col) for col in cols], axis=1)

    def get(self, m, restart, maxit=MAXIT):
        from tests.bgmres_reference import reference_solve
        if (m, restart, maxit) not in self.refs:
            self.refs[m, restart, maxit] = reference_solve(self.dec, self.blocks[m], REDUCTION, maxit, restart, RANK_TOL, **self.okw)
        return self.host(self.blocks[m]), self.refs[m, restart, maxit]


@pytest.fixture(scope="module", params=["poisson_rm", "dg_umfpack"])
def golden(ddm, request):
    g = Golden(ddm, request.param)
    yield g
    g.tl.prec.check_status()
    g.tl.ctx.close()


def _true_reductions(tl, Bh, X, def0):
    """||b_c - A x_c|| / def0_c, recomputed with ddm_op_applyscaleadd_multi (0 where def0_c = 0)"""
    R = tl.to_device(Bh.copy()).contiguous()
    tl.op.applyscaleadd_multi(-1.0, X, R)
    d = np.sqrt(tl.op.dot_multi(R, R))
    return np.where(def0 > 0.0, d / np.where(def0 > 0.0, def0, 1.0), 0.0)


def _compare(res, hist, widths, X, ref):
    """iteration counts (one apart only where the two defects straddle the threshold), widths, histories under the rule, x within 1e-8"""
    its, conv, hist_ref, widths_ref, X_ref = ref
    m = hist_ref.shape[1]
    got = [r.iterations for r in res]
    k = min(len(hist), len(hist_ref))
    rule = RTOL_HIST * hist_ref[:k] + ATOL_HIST * hist_ref[0]
    dev = np.abs(hist[:k] - hist_ref[:k])
    print("m", m, "iterations", got, its, "widths", widths.tolist(), "max history deviation / rule", float(np.max(dev / np.maximum(rule, 1e-300))))
    assert abs(len(hist) - len(hist_ref)) <= 1 and np.isfinite(hist).all() and hist.shape[1] == m
    assert bool((dev <= rule).all())
    for c in range(m):
        if got[c] != its[c]:
            kk = min(got[c], its[c])
            thr = REDUCTION * hist_ref[0, c]
            assert abs(got[c] - its[c]) == 1 and (hist[kk, c] < thr) != (hist_ref[kk, c] < thr), (c, got[c], its[c])
    assert len(widths) == len(hist) - 1 and widths[:k - 1].tolist() == list(widths_ref[:k - 1])
    Xh = X.cpu().numpy()
    for c in range(m):
        want = np.concatenate(X_ref[c])
        top = float(np.max(np.abs(want)))
        assert float(np.max(np.abs(Xh[:, c] - want))) <= 1e-8 * top if top > 0.0 else not np.any(Xh[:, c]), c


@pytest.mark.parametrize("m, restart", [(1, 6), (5, 6), (8, 6), (8, 50)])
def test_solve_block_gmres_matches_restatement(ddm, golden, m, restart):
    """reduction 1e-10 on poisson12_2x2x2 (restricted Schwarz, multiplicative POU coarse level) and dg32_2x2 (non-symmetric operator) at
    m = 1 (the problem's b), m = 5 (b, random, 2 b, zero, random: width <= 3) and m = 8 (b and seven random columns) with restart 6,
    and m = 8 with restart 50.  Per column the iteration count equals the restatement's, or differs by one when the defect of the
    earlier of the two iterations lies on either side of the threshold in the two runs; width histories equal; histories within
    1e-7 |r_k| + 1e-11 |r_0|; x within 1e-8; the true reductions, recomputed with ddm_op_applyscaleadd_multi, are below 1e-10 and agree
    with the reported ones within TRUE_GAP_TOL; the zero column is never written.  At m = 8 and restart 50 the block needs fewer block
    iterations than the slowest column of solve_multi with flexible GMRES.  A second call is bitwise the first."""
    import torch
    tl = golden.tl
    Bh, ref = golden.get(m, restart)
    res, hist, X, widths = tl.solve_block_gmres(Bh, reduction=REDUCTION, maxit=MAXIT, restart=restart)
    tl.prec.check_status()
    assert all(r.converged == 1 for r in res) and all(ref[1])
    _compare(res, hist, widths, X, ref)
    got = [r.iterations for r in res]
    Xh = X.cpu().numpy()
    true = _true_reductions(tl, Bh, X, hist[0])
    for c in range(m):
        if res[c].def0 == 0.0:
            assert got[c] == 0 and not np.any(Xh[:, c]) and not np.any(hist[:, c])
            continue
        assert res[c].def0 == hist[0, c] and res[c].reduction == hist[-1, c] / hist[0, c]
        assert true[c] < REDUCTION and abs(true[c] - res[c].reduction) <= TRUE_GAP_TOL, (c, true[c], res[c].reduction)
    if m == 5:
        assert max(widths.tolist()) <= 3 and got[3] == 0
        assert float(torch.max(torch.abs(X[:, 2] - 2.0 * X[:, 0]))) <= 1e-8 * float(torch.max(torch.abs(X[:, 0])))
    if m == 8:
        assert set(widths.tolist()) == {8}
    if m == 8 and restart == 50:
        res_multi, hist_multi, X_multi = tl.solve_multi(Bh, reduction=REDUCTION, maxit=MAXIT, solver="restartedflexiblegmressolver", restart=restart)
        print("   solve_multi iterations", [r.iterations for r in res_multi])
        assert len(hist) - 1 < max(r.iterations for r in res_multi)
    res2, hist2, X2, widths2 = tl.solve_block_gmres(Bh, reduction=REDUCTION, maxit=MAXIT, restart=restart)
    assert torch.equal(X2, X) and np.array_equal(hist2, hist) and np.array_equal(widths2, widths)


def test_exhausting_block(ddm, golden):
    """[b, A M^-1 b] with A M^-1 b formed by the library's own applies, restart 6: width 2 for one iteration, then 1; column 1 reports 1
    iteration; both columns converge to a true reduction below 1e-10"""
    import torch
    tl = golden.tl
    b = tl.to_device(golden.host([rhs(golden.dec)])).contiguous()
    z, w = torch.zeros_like(b), torch.zeros_like(b)
    tl.prec.apply_multi(z, b)
    tl.op.apply_multi(z, w)
    Bh = torch.cat([b, w], dim=1).contiguous().cpu().numpy()
    res, hist, X, widths = tl.solve_block_gmres(Bh, reduction=REDUCTION, maxit=MAXIT, restart=6)
    true = _true_reductions(tl, Bh, X, hist[0])
    print("iterations", [r.iterations for r in res], "widths", widths.tolist(), "true reductions", true)
    assert widths[0] == 2 and len(widths) > 1 and set(widths[1:].tolist()) == {1}
    assert res[1].iterations == 1 and res[0].iterations == len(widths) and all(r.converged == 1 for r in res)
    assert np.all(true < REDUCTION) and np.all(hist[1:, 1] == hist[1, 1])


def test_initial_guess(ddm, golden):
    """a non-zero X0 on the degenerate block at restart 6: the restatement from the same X0 is matched as from zero; the zero column's
    X0 is zero and stays zero"""
    from tests.bgmres_reference import reference_solve
    tl, dec = golden.tl, golden.dec
    rng = np.random.default_rng(77)
    X0 = []
    for c in range(5):
        xg = rng.standard_normal(dec.nglobal) if c != 3 else np.zeros(dec.nglobal)
        X0.append([xg[sd.glob[:sd.n_o]].copy() for sd in dec.subs])
    Bh = golden.host(golden.blocks[5])
    ref = reference_solve(dec, golden.blocks[5], REDUCTION, MAXIT, 6, RANK_TOL, X0=X0, **golden.okw)
    res, hist, X, widths = tl.solve_block_gmres(Bh, reduction=REDUCTION, maxit=MAXIT, restart=6, X0=golden.host(X0))
    assert all(r.converged == 1 for r in res) and all(ref[1]) and hist[0, 3] == 0.0 and not np.any(X[:, 3].cpu().numpy())
    _compare(res, hist, widths, X, ref)
    true = _true_reductions(tl, Bh, X, hist[0])
    assert np.all(true < REDUCTION) and float(np.max(np.abs(true - hist[-1] / np.where(hist[0] > 0.0, hist[0], 1.0)))) <= TRUE_GAP_TOL


def test_state_left_behind_and_maxit(ddm, golden):
    """A solve_multi (GMRES) after a solve_block_gmres on the same object is bit for bit the solve_multi before it (the block driver
    leaves no device-side state); maxit = 2 returns converged = 0 in every non-zero column with rows 0 .. 2 of the history written for
    every column and two widths; maxit = 0 leaves a poisoned x as it was and writes row 0."""
    import torch
    tl = golden.tl
    Bh, _ = golden.get(5, 6)
    res_a, hist_a, X_a = tl.solve_multi(Bh, reduction=REDUCTION, maxit=MAXIT, solver="restartedgmressolver", restart=6)
    res, hist, X, widths = tl.solve_block_gmres(Bh, reduction=REDUCTION, maxit=2, restart=6)
    assert hist.shape == (3, 5) and np.isfinite(hist).all() and widths.tolist() == [3, 3]
    for c in (0, 1, 2, 4):
        assert res[c].converged == 0 and res[c].iterations == 2 and res[c].reduction == hist[2, c] / hist[0, c]
    assert res[3].converged == 1 and res[3].iterations == 0 and not torch.any(X[:, 3])
    Xp = np.full_like(Bh, 0.25)
    Xp[:, 3] = 0.0
    res0, hist0, X0, widths0 = tl.solve_block_gmres(Bh, reduction=REDUCTION, maxit=0, restart=6, X0=Xp)
    assert hist0.shape == (1, 5) and len(widths0) == 0 and np.array_equal(X0.cpu().numpy(), Xp) and np.isfinite(hist0).all()
    assert all(r.iterations == 0 for r in res0) and [r.converged for r in res0] == [0, 0, 0, 1, 0]
    res_b, hist_b, X_b = tl.solve_multi(Bh, reduction=REDUCTION, maxit=MAXIT, solver="restartedgmressolver", restart=6)
    assert torch.equal(X_a, X_b) and np.array_equal(hist_a, hist_b, equal_nan=True)
    assert [r.iterations for r in res_a] == [r.iterations for r in res_b]


def test_refusals_with_live_handles(ddm, golden):
    """DDM_EINVAL before any device work: X == B, a null X, nrhs 0 and 33, maxit -1, restart 0, rank_tol 0 and 1; a poisoned X stays
    poisoned"""
    import torch
    tl = golden.tl
    Bh, _ = golden.get(5, 6)
    lib, h = tl.ctx.lib, tl.ctx.h
    res = (ddm.SolveResult * 33)()
    Bd = tl.to_device(Bh.copy()).contiguous()
    B0 = Bd.clone()
    X = torch.full_like(Bd, 123.456)
    x, b = X.data_ptr(), Bd.data_ptr()
    for nrhs, xp, bp, maxit, restart, tol in [(0, x, b, 10, 6, 1e-12), (33, x, b, 10, 6, 1e-12), (5, x, x, 10, 6, 1e-12), (5, x, b, -1, 6, 1e-12),
                                              (5, x, b, 10, 0, 1e-12), (5, x, b, 10, 6, 0.0), (5, x, b, 10, 6, 1.0), (5, None, b, 10, 6, 1e-12)]:
        rc = lib.ddm_bgmres_solve_multi(h, tl.op.h, tl.prec.h, nrhs, xp, bp, 1e-10, maxit, restart, tol, None, None, res)
        assert rc == ddm.DDM_EINVAL and "ddm_bgmres_solve_multi" in lib.ddm_last_error(h).decode()
    tl.ctx.sync()
    assert torch.equal(X, torch.full_like(Bd, 123.456)) and torch.equal(Bd, B0)
