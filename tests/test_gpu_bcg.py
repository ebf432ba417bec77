"""-m gpu: block CG on the device (ddm_bcg_solve_multi, TwoLevelSchwarz.solve_block).  Its three kernels against numpy at the widths their
thread layouts branch on, the driver against the numpy restatement (tests/bcg_reference.py, checked on the CPU by tests/test_bcg_cpu.py)
and against the recomputed true defect, and what it leaves behind for the other block drivers.

Tolerances.  Gram entries: 1e-13 sum |u||v| (the project's rule for Gram products).  Update and direction, per
entry: 2 (m + 2) u (|x| + sum_j |p_j||alpha_jc|), u = 2^-53 (m products, m - 1 additions, one more addition).  Norms: 1e-12 relative.
Histories: 1e-7 |r_k| + 1e-11 |r_0| (tests/test_bcg_cpu.py::test_summation_order_sensitivity shows the rule is 4.0e6 to 1.7e7 times what another
summation order moves these runs).  x: 1e-8 of the restatement's largest entry.  Reported against recomputed reduction: 1e-14
(FCG_TRUE_DEFECT_TOL, the figure of the other drivers that test the true defect).  Repeated calls are bitwise equal."""
import numpy as np
import pytest

from tests.test_bcg_cpu import MAXIT, OKW, RANK_TOL, REDUCTION, TKW, block_degenerate, block_m8
from tests.test_fcg_cpu import FCG_TRUE_DEFECT_TOL
from tests.test_fgmres_cpu import golden_poisson
from tests.test_gpu_multi_gmres import ATOL_HIST, RTOL_HIST
from tests.test_gpu_parity import _build

pytestmark = pytest.mark.gpu

# 16-wide tiles would branch at 16 / 17 / 32, the column groups of for_column_groups at 1 / 2 / 3 / 7 / 8 / 9; the kernels here branch on
# odd m (the zero pad column of the Gram tiles), on the row slices 256 / (ceil(m / 2))^2 (256, 256, 64, 16, 16, 10, 4, 3, 1, 1) and on
# the rows per quarter tile 256 / m (256 .. 8) with idle threads wherever m does not divide 256
WIDTHS = (1, 2, 3, 7, 8, 9, 16, 17, 31, 32)
U_ROUND = 2.0 ** -53


@pytest.fixture(scope="module")
def small(ddm):
    """the (13, 12, 11) grid: owner masks that are not all ones, n_o no multiple of any tile"""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    dec = _build(ddm, (13, 12, 11), (2, 2, 2))
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="standard", mode="additive")
    mask = np.asarray(tl.rl.owner_novlp, dtype=bool)
    assert 0 < mask.sum() < len(mask) and len(mask) == tl.rl.n_o and tl.rl.n_o % 32 != 0     # (32 rows: the smallest tile, at m = 32)
    yield tl, mask
    tl.prec.check_status()
    tl.ctx.close()


class Raw:
    """an operator that is only its row count and owner mask (identity matrix, no halo): n = 1024 * 1024 + 300 rows, so that at m = 3
    (340 rows per update tile, 512 per Gram tile) the 1024 workgroups of every kernel make several grid-stride trips, the last one
    partial"""

    def __init__(self, ddm):
        import scipy.sparse as sp
        self.n = 1024 * 1024 + 300
        self.ctx = ddm.torch_context()
        self.A = ddm.CsrMatrix(self.ctx, sp.identity(self.n, format="csr", dtype=np.float64))
        self.mask = np.random.default_rng(3).random(self.n) < 0.9
        self.op = ddm.NonOverlappingOperator(self.ctx, self.A, None, self.mask.astype(np.uint8))


@pytest.fixture(scope="module")
def raw(ddm):
    r = Raw(ddm)
    yield r
    r.ctx.close()


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda().contiguous()


def _check_gram(ddm, ctx, op, mask, n, m, seed):
    rng = np.random.default_rng(seed)
    U, V1, V2 = (rng.standard_normal((n, m)) for _ in range(3))
    for a in (U, V1, V2):
        a[~mask] = np.nan                                   # rows that are not owned must not be read into the sums
    Ud, V1d, V2d = _dev(U), _dev(V1), _dev(V2)
    G1, G2 = ddm.bcg_gram_multi(ctx, op, Ud, V1d, V2d)
    H1 = ddm.bcg_gram_multi(ctx, op, Ud, V1d)
    G1b, G2b = ddm.bcg_gram_multi(ctx, op, Ud, V1d, V2d)
    L = np.longdouble
    Uo = U[mask].astype(L)
    worst = 0.0
    for G, V in ((G1, V1), (G2, V2), (H1, V1)):
        Vo = V[mask].astype(L)
        ref = Uo.T @ Vo
        bound = 1e-13 * np.asarray(np.abs(Uo).T @ np.abs(Vo), dtype=float)
        assert G.shape == (m, m) and np.isfinite(G).all()
        err = np.abs(G - np.asarray(ref, dtype=float))
        worst = max(worst, float(np.max(err / bound)))
        assert (err <= bound).all(), (m, float(np.max(err / bound)))
    assert np.array_equal(G1, G1b) and np.array_equal(G2, G2b) and np.array_equal(G1, H1)   # no atomics: bit-reproducible
    return worst


def _check_update_and_direction(ddm, ctx, op, mask, n, m, seed):
    import torch
    rng = np.random.default_rng(seed)
    P, Q, X, R, Z = (rng.standard_normal((n, m)) for _ in range(5))
    alpha = rng.standard_normal((m, m))
    L = np.longdouble
    Pd, Qd = _dev(P), _dev(Q)
    outs = []
    for _ in range(2):
        Xd, Rd = _dev(X), _dev(R)
        nrm = ddm.bcg_update_multi(ctx, op, alpha, Pd, Qd, Xd, Rd)
        outs.append((Xd, Rd, nrm))
    (Xd, Rd, nrm), (Xd2, Rd2, nrm2) = outs
    assert torch.equal(Xd, Xd2) and torch.equal(Rd, Rd2) and np.array_equal(nrm, nrm2)
    assert torch.equal(Pd, _dev(P)) and torch.equal(Qd, _dev(Q))
    bx = 2 * (m + 2) * U_ROUND * (np.abs(X) + np.abs(P) @ np.abs(alpha))
    br = 2 * (m + 2) * U_ROUND * (np.abs(R) + np.abs(Q) @ np.abs(alpha))
    ex = np.abs(Xd.cpu().numpy() - np.asarray(X.astype(L) + P.astype(L) @ alpha.astype(L), dtype=float))
    er = np.abs(Rd.cpu().numpy() - np.asarray(R.astype(L) - Q.astype(L) @ alpha.astype(L), dtype=float))
    assert (ex <= bx).all() and (er <= br).all(), (m, float(np.max(ex / bx)), float(np.max(er / br)))
    Rn = Rd.cpu().numpy()
    want = np.asarray(np.sum(Rn[mask].astype(L) ** 2, axis=0), dtype=float)
    assert nrm.shape == (m,) and np.isfinite(nrm).all() and (np.abs(nrm - want) <= 1e-12 * want).all()
    beta = rng.standard_normal((m, m))
    Zd = _dev(Z)
    outs = []
    for _ in range(2):
        Pw = _dev(P)
        ddm.bcg_direction_multi(ctx, op, beta, Zd, Pw)
        outs.append(Pw)
    assert torch.equal(outs[0], outs[1]) and torch.equal(Zd, _dev(Z))
    bp = 2 * (m + 2) * U_ROUND * (np.abs(Z) + np.abs(P) @ np.abs(beta))
    ep = np.abs(outs[0].cpu().numpy() - np.asarray(Z.astype(L) + P.astype(L) @ beta.astype(L), dtype=float))
    assert (ep <= bp).all(), (m, float(np.max(ep / bp)))
    return float(np.max(ex / bx)), float(np.max(er / br)), float(np.max(ep / bp))


@pytest.mark.parametrize("m", WIDTHS)
def test_kernels_against_numpy(ddm, small, m):
    """Gram (one and two products), update with norms, and direction on the (13, 12, 11) grid, against extended-precision numpy under the
    bounds of the module docstring; rows that are not owned hold NaN in the Gram inputs; outputs that must be written completely are
    pre-filled with NaN by the wrappers; two identical calls agree bit for bit; inputs are not modified."""
    tl, mask = small
    n = tl.rl.n_o
    g = _check_gram(ddm, tl.ctx, tl.op, mask, n, m, seed=100 + m)
    x, r, p = _check_update_and_direction(ddm, tl.ctx, tl.op, mask, n, m, seed=200 + m)
    print("m", m, "worst error / bound: gram", g, "update x", x, "update r", r, "direction", p)


def test_kernels_grid_stride(ddm, raw):
    """m = 3 with n = 1048876 rows: every kernel's 1024 workgroups take several tiles each (grid-stride loop), the last tile partial"""
    g = _check_gram(ddm, raw.ctx, raw.op, raw.mask, raw.n, 3, seed=31)
    x, r, p = _check_update_and_direction(ddm, raw.ctx, raw.op, raw.mask, raw.n, 3, seed=32)
    print("worst error / bound: gram", g, "update x", x, "update r", r, "direction", p)


# ---- the driver against the restatement ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(ddm):
    """the 12^3 golden problem with the symmetric preconditioner; the three blocks and the restatement's runs on them, computed once"""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    from tests.bcg_reference import reference_solve
    dec = golden_poisson(ddm)
    tl = TwoLevelSchwarz(dec, **TKW)
    blocks = {1: [[sd.b.copy() for sd in dec.subs]], 5: block_degenerate(dec), 8: block_m8(dec)}
    refs = {}

    def get(m):
        if m not in refs:
            host = np.stack([tl.rl.cat_novlp(col) for col in blocks[m]], axis=1)
            refs[m] = (host, reference_solve(dec, blocks[m], REDUCTION, MAXIT, RANK_TOL, **OKW))
        return refs[m]
    yield tl, get
    tl.prec.check_status()
    tl.ctx.close()


def _true_reductions(tl, Bh, X):
    R = tl.to_device(Bh.copy()).contiguous()
    B0 = R.clone()
    tl.op.applyscaleadd_multi(-1.0, X, R)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(tl.op.dot_multi(R, R) / tl.op.dot_multi(B0, B0))


@pytest.mark.parametrize("m", [1, 5, 8])
def test_solve_block_matches_restatement(ddm, golden, m):
    """reduction 1e-10 on poisson12_2x2x2 (standard Schwarz + POU coarse level, additive) at m = 1 (the problem's b: block CG is CG),
    m = 5 (b, random, 2 b, zero, random: rank 3) and m = 8 (b and seven random columns).  Per column the iteration count equals the
    restatement's, or differs by one when the defect of the earlier of the two iterations lies on either side of the threshold in
    the two runs; rank histories equal; histories within 1e-7 |r_k| + 1e-11 |r_0|; x within 1e-8; the true reductions, recomputed with
    ddm_op_applyscaleadd_multi, are below 1e-10 and agree with the reported ones within 1e-14; the zero column is never touched.  At
    m = 8 the block needs no more iterations than the slowest column of solve_multi on the same block."""
    import torch
    tl, get = golden
    Bh, (its, conv, hist_ref, ranks_ref, X_ref) = get(m)
    res, hist, X, ranks = tl.solve_block(Bh, reduction=REDUCTION, maxit=MAXIT)
    tl.prec.check_status()
    got = [r.iterations for r in res]
    k = min(len(hist), len(hist_ref))
    rule = RTOL_HIST * hist_ref[:k] + ATOL_HIST * hist_ref[0]
    dev = np.abs(hist[:k] - hist_ref[:k])
    print("m", m, "iterations", got, its, "ranks", sorted(set(ranks.tolist())), "max history deviation / rule",
          float(np.max(dev / np.maximum(rule, 1e-300))))
    assert all(r.converged == 1 for r in res) and all(conv)
    assert abs(len(hist) - len(hist_ref)) <= 1 and np.isfinite(hist).all() and hist.shape[1] == m
    assert bool((dev <= rule).all())
    for c in range(m):
        if got[c] != its[c]:
            kk = min(got[c], its[c])
            thr = REDUCTION * hist_ref[0, c]
            assert abs(got[c] - its[c]) == 1 and (hist[kk, c] < thr) != (hist_ref[kk, c] < thr), (c, got[c], its[c])
    assert len(ranks) == len(hist) - 1 and ranks[:k - 1].tolist() == list(ranks_ref[:k - 1])
    Xh = X.cpu().numpy()
    for c in range(m):
        want = np.concatenate(X_ref[c])
        top = float(np.max(np.abs(want)))
        assert float(np.max(np.abs(Xh[:, c] - want))) <= 1e-8 * top if top > 0.0 else not np.any(Xh[:, c]), c
    true = _true_reductions(tl, Bh, X)
    for c in range(m):
        if res[c].def0 == 0.0:
            assert got[c] == 0 and not np.any(Xh[:, c]) and not np.any(hist[:, c])
            continue
        assert res[c].def0 == hist[0, c] and res[c].reduction == hist[-1, c] / hist[0, c]
        assert true[c] < REDUCTION and abs(true[c] - res[c].reduction) <= FCG_TRUE_DEFECT_TOL, (c, true[c], res[c].reduction)
    if m == 5:
        assert set(ranks.tolist()) == {3} and got[3] == 0
        assert float(torch.max(torch.abs(X[:, 2] - 2.0 * X[:, 0]))) <= 1e-8 * float(torch.max(torch.abs(X[:, 0])))
    if m == 8:
        res_multi, hist_multi, X_multi = tl.solve_multi(Bh, reduction=REDUCTION, maxit=MAXIT)
        print("   solve_multi iterations", [r.iterations for r in res_multi])
        assert len(hist) - 1 <= max(r.iterations for r in res_multi)
        assert max(got) < min(r.iterations for r in res_multi)
    res2, hist2, X2, ranks2 = tl.solve_block(Bh, reduction=REDUCTION, maxit=MAXIT)
    assert torch.equal(X2, X) and np.array_equal(hist2, hist) and np.array_equal(ranks2, ranks)


def test_state_left_behind_and_maxit(ddm, golden):
    """A solve_multi after a solve_block on the same object is bit for bit the solve_multi before it (the block driver shares P and Q
    with it and leaves no device-side state); maxit = 2 returns converged = 0 in every non-zero column with rows 0 .. 2 of the history
    written for every column and two ranks; maxit = 0 leaves x as it was."""
    import torch
    tl, get = golden
    Bh, _ = get(5)
    res_a, hist_a, X_a = tl.solve_multi(Bh, reduction=REDUCTION, maxit=MAXIT)
    res, hist, X, ranks = tl.solve_block(Bh, reduction=REDUCTION, maxit=2)
    assert hist.shape == (3, 5) and np.isfinite(hist).all() and len(ranks) == 2
    for c in (0, 1, 2, 4):
        assert res[c].converged == 0 and res[c].iterations == 2 and res[c].reduction == hist[2, c] / hist[0, c]
    assert res[3].converged == 1 and res[3].iterations == 0 and not torch.any(X[:, 3])
    res0, hist0, X0, ranks0 = tl.solve_block(Bh, reduction=REDUCTION, maxit=0)
    assert hist0.shape == (1, 5) and len(ranks0) == 0 and not torch.any(X0) and np.array_equal(hist0[0], hist[0])
    res_b, hist_b, X_b = tl.solve_multi(Bh, reduction=REDUCTION, maxit=MAXIT)
    assert torch.equal(X_a, X_b) and np.array_equal(hist_a, hist_b, equal_nan=True)
    assert [r.iterations for r in res_a] == [r.iterations for r in res_b]


def test_refusals_with_live_handles(ddm, golden):
    """DDM_EINVAL before any device work: X == B, nrhs 0 and 33, maxit -1, rank_tol 0 and 1; a poisoned X stays poisoned"""
    import torch
    tl, get = golden
    Bh, _ = get(5)
    lib, h = tl.ctx.lib, tl.ctx.h
    res = (ddm.SolveResult * 33)()
    Bd = tl.to_device(Bh.copy()).contiguous()
    B0 = Bd.clone()
    X = torch.full_like(Bd, 123.456)
    for nrhs, xp, bp, maxit, tol in [(0, X.data_ptr(), Bd.data_ptr(), 10, 1e-12), (33, X.data_ptr(), Bd.data_ptr(), 10, 1e-12), (5, X.data_ptr(), X.data_ptr(), 10, 1e-12),
                                     (5, X.data_ptr(), Bd.data_ptr(), -1, 1e-12), (5, X.data_ptr(), Bd.data_ptr(), 10, 0.0), (5, X.data_ptr(), Bd.data_ptr(), 10, 1.0),
                                     (5, None, Bd.data_ptr(), 10, 1e-12)]:
        rc = lib.ddm_bcg_solve_multi(h, tl.op.h, tl.prec.h, nrhs, xp, bp, 1e-10, maxit, tol, None, None, res)
        assert rc == ddm.DDM_EINVAL and "ddm_bcg_solve_multi" in lib.ddm_last_error(h).decode()
    tl.ctx.sync()
    assert torch.equal(X, torch.full_like(Bd, 123.456)) and torch.equal(Bd, B0)
