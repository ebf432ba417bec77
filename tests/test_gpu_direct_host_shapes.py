"""-m gpu: the device solves of the sparse direct factor with the HOST factorisation (DDM_DIRECT_ENGINE=host: direct_create_impl,
csrc/tri_csr.hpp) -- k_trsv_csr_fused, k_trsv_csr_blocks and k_trsv_csr_level for one vector, k_trsv_csr_level_multi for blocks of
columns -- at the shapes those kernels and their launch code branch on.

The cases, what each reaches and the proof that it does are in tests/direct_cases.py and tests/test_direct_cases_reference.py (CPU);
the level counts the library reports are compared with the restated ones, which ties that proof to the schedule actually built.
Checks per result, all against the LIBRARY's factor array (F.factors(), itself compared with ddm.chol_host's):

  (a) Evaluated.ratio <= C = 2 (w_L + w_U + 9): |d - L U x| <= u (C g + 2 h) row by row in the fill-reducing order, g = |L| |U| |x|
      and h the term in |T| |T^-1| |T| of the inverted supernodes (derivation: the module docstring of direct_cases; the float64
      restatement measures 2.7 .. 5.6 against C = 806 .. 3342, a dropped operand, a stale unknown or a skipped dinv 7 10^4 C or more);
  (b) two solutions of one system -- with and without the supernode transformation, a column of a block solve and the
      single-vector solve of it -- differ by no more than their two bounds allow: Evaluated.difference <= 1;
  (c) bit equality of a replay with the first solve, and of a second factor object of the same matrix with the first.

Measured on one MI355X (every case, all three solves / all widths): (a) single vector 1.47 .. 2.82, block sweeps 2.92 .. 12.41,
against C = 806 .. 3342; (b) transformed against untransformed 9.2e-4 and 7.3e-4, block columns against single-vector solves
1.1e-3 .. 3.6e-3 of what the two bounds allow.

No case is skipped or filtered at run time."""
import numpy as np
import pytest

from tests import direct_cases as dc

pytestmark = pytest.mark.gpu

# Sm nrhs = 64, 128, 192, 160, 192, 192, 256, 129, 256 threads per row of a level with S = 64 (rows per workgroup 4, 2, 1, 1, ..: idle
# threads at 192, 160 and 129), then two panels: 256 + 1 and 256 + 4 columns
SWEEP_WIDTHS = (1, 2, 3, 5, 24, 48, 128, 129, 256, 257, 260)
SWEEP_CASES = ("sn8", "rows8", "dg", "uneven5")


class Ref:
    """per case, computed once and never changed: two right-hand sides and a block of columns"""

    def __init__(self, name):
        self.c = c = dc.case(name)
        rng = np.random.default_rng(43)
        self.d = [rng.standard_normal(c.n), rng.standard_normal(c.n)]
        self.D = rng.standard_normal((c.n, max(SWEEP_WIDTHS)))
        for a in (self.d[0], self.d[1], self.D):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def refs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Ref(name)
        return made[name]
    return get


def _factor(ddm, ctx, c, monkeypatch):
    """the factor of case c on the host engine with the case's supernode threshold (both variables are read at every creation)"""
    c.env(monkeypatch)
    F = ddm.Ilu0(ctx, ddm.CsrMatrix(ctx, c.M), c.block_ptr, direct=True, general=c.general)
    assert ctx.lib.ddm_ilu0_is_direct(F.h) == 1 and F.engine() == "levels" and F.refinement()[0] == 0, c.name
    assert (F.num_levels(False), F.num_levels(True)) == c.table.nlev, (c.name, "the library's schedule is not the restated one")
    return F


def _check_factors(F, c):
    lu = F.factors()
    assert lu.shape == c.F.lu.shape == (F.nnz,)
    dev = float(np.max(np.abs(lu - c.F.lu)) / np.max(np.abs(c.F.lu)))
    assert dev < 1e-13, dev                                     # the same host factorisation
    return c.residual(lu)


def _solve(F, ctx, dd, xd):
    xd.fill_(float("nan"))
    F.solve(dd, xd)
    ctx.sync()
    assert F.status() == 0
    return xd.cpu().numpy().copy()


@pytest.mark.parametrize("name", dc.NAMES)
def test_single_vector_solve(ddm, refs, name, monkeypatch):
    """F.solve on every case: engine, level counts and factors as restated; three solves into a NaN-filled x (the capture, its
    replay, another right-hand side) with status 0 after each; (a) for each, (c) for the replay and for a second factor object."""
    import torch
    ref = refs(name)
    c = ref.c
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, c, monkeypatch)
    res = _check_factors(F, c)
    dd = [torch.tensor(d).cuda() for d in ref.d]
    xd = torch.empty(c.n, dtype=torch.float64, device="cuda")
    got = [(k, _solve(F, ctx, dd[k], xd)) for k in (0, 0, 1)]
    for rep, (k, x) in enumerate(got):
        ratio = res.ratio(ref.d[k], x, c.C)
        print(f"\n{name} ({'block path' if c.blocks else 'global levels'}, levels {c.table.nlev}, {len(c.table.runs)} supernodes) solve {rep}: "
              f"residual ratio {ratio:.2f} (C = {c.C})")
        assert ratio <= c.C, (name, rep, ratio, c.C)
    assert np.array_equal(got[0][1], got[1][1]), (name, "replay differs from the first solve")
    F2 = _factor(ddm, ctx, c, monkeypatch)
    x2 = torch.empty_like(xd)
    assert np.array_equal(_solve(F2, ctx, dd[0], x2), got[0][1]), (name, "a second factor of the same matrix gives other bits")
    ctx.close()


@pytest.mark.parametrize("with_sn, without", [("sn8", "rows8"), ("uneven5_sn", "uneven5")])
def test_transformation_does_not_change_the_solution(ddm, refs, with_sn, without, monkeypatch):
    """the same factor solved through inverted supernodes on global levels (k_trsv_csr_fused / _level) and row by row on the block
    path (k_trsv_csr_blocks): (b)"""
    import torch
    a, b = refs(with_sn).c, refs(without).c
    assert a.F is b.F and b.blocks and not a.blocks and a.table.nvirt > 0 and b.table.nvirt == 0
    d = refs(with_sn).d[0]
    ctx = ddm.torch_context(0)
    dd = torch.tensor(d).cuda()
    ev = []
    for c in (a, b):
        F = _factor(ddm, ctx, c, monkeypatch)
        res = _check_factors(F, c)
        xd = torch.empty(c.n, dtype=torch.float64, device="cuda")
        ev.append(res.evaluate(d, _solve(F, ctx, dd, xd)))
        assert ev[-1].ratio(c.C) <= c.C
    q = ev[0].difference(ev[1], a.C, b.C)
    print(f"\n{with_sn} against {without}: |L U (x_a - x_b)| is {q:.2e} of what the two bounds allow; ratios {ev[0].ratio(a.C):.2f}, {ev[1].ratio(b.C):.2f}")
    assert q <= 1.0
    ctx.close()


class _Columns:
    """the evaluated columns of one case: a column with the bits of one seen before is not evaluated again (columns of two widths
    that the kernel sums in the same split are equal bit for bit), every other one is -- no column goes unchecked"""

    def __init__(self, res, D):
        self.res, self.D = res, D
        self.seen = [{} for _ in range(D.shape[1])]              # per column: the bytes of x -> (r, g, h)

    def evaluate(self, X):
        """(Evaluated of the columns of X = solutions of the first columns of D, how many of them had new bits)"""
        m = X.shape[1]
        keys = [np.ascontiguousarray(X[:, j]).tobytes() for j in range(m)]
        new = [j for j in range(m) if keys[j] not in self.seen[j]]
        if new:
            e = self.res.evaluate(self.D[:, new], X[:, new])
            for k, j in enumerate(new):
                self.seen[j][keys[j]] = (e.r[:, k], e.g[:, k], e.h[:, k])
        pick = [self.seen[j][keys[j]] for j in range(m)]
        return dc.Evaluated(*(np.stack([p[i] for p in pick], axis=1) for i in (0, 1, 2))), len(new)


@pytest.mark.parametrize("name", SWEEP_CASES)
def test_block_sweeps(ddm, refs, name, monkeypatch):
    """F.solve_multi at the widths of SWEEP_WIDTHS on the first m columns of one block, X NaN-filled: every column passes (a), and
    (b) against the single-vector F.solve of that column (the summation split differs: `==` is not expected); the replay has the
    bits of the first call.  Widths above 256 run in column panels (direct_cases.panels)."""
    import torch
    ref = refs(name)
    c = ref.c
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, c, monkeypatch)
    cols = _Columns(_check_factors(F, c), ref.D)
    Dd = torch.tensor(ref.D).cuda()
    mmax = Dd.shape[1]
    dj = torch.empty(c.n, dtype=torch.float64, device="cuda")
    xj = torch.empty_like(dj)
    single = np.empty((c.n, mmax))
    for j in range(mmax):                                       # one captured graph, replayed per column
        dj.copy_(Dd[:, j])
        single[:, j] = _solve(F, ctx, dj, xj)
    es, _ = cols.evaluate(single)
    rs = es.ratio(c.C)
    print(f"\n{name}: single-vector solves of {mmax} columns, worst residual ratio {rs.max():.2f} (C = {c.C})")
    assert rs.max() <= c.C
    failures = []
    for m in SWEEP_WIDTHS:
        D = Dd[:, :m].contiguous()
        X = torch.full_like(D, float("nan"))
        F.solve_multi(D, X)
        ctx.sync()
        assert F.status() == 0
        Xh = X.cpu().numpy().copy()
        X.fill_(float("nan"))
        F.solve_multi(D, X)                                     # the replay
        ctx.sync()
        assert F.status() == 0
        e, fresh = cols.evaluate(Xh)
        ratios = e.ratio(c.C)
        diff = e.difference(dc.Evaluated(es.r[:, :m], es.g[:, :m], es.h[:, :m]), c.C, c.C)
        print(f"{name} m = {m} (panels {dc.panels(m)}): worst residual ratio {ratios.max():.2f} (C = {c.C}), against the single-vector solves "
              f"{diff.max():.2e} of the two bounds, {fresh} columns with new bits")
        if not ratios.max() <= c.C:
            failures.append((m, "residual", float(ratios.max()), int(np.argmax(ratios))))
        if not diff.max() <= 1.0:
            failures.append((m, "single-vector", float(diff.max()), int(np.argmax(diff))))
        if not np.array_equal(X.cpu().numpy(), Xh):
            failures.append((m, "replay differs"))
    assert not failures, failures
    ctx.close()


def test_single_solve_survives_wider_block_solves(ddm, refs, monkeypatch):
    """the single-vector graph works on F->pd / F->px, the block solves re-allocate F->pD / F->pX for more columns: the SAME d / x
    tensors before and after block solves of growing width (up to more than one panel) give the same bits"""
    import torch
    ref = refs("uneven5_sn")
    c = ref.c
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, c, monkeypatch)
    res = _check_factors(F, c)
    d = torch.tensor(ref.d[0]).cuda()
    x = torch.empty_like(d)
    x0 = _solve(F, ctx, d, x)
    assert res.ratio(ref.d[0], x0, c.C) <= c.C
    Dd = torch.tensor(ref.D).cuda()
    for m in (24, 48, 260):
        B = Dd[:, :m].contiguous()
        X = torch.full_like(B, float("nan"))
        F.solve_multi(B, X)
        ctx.sync()
        assert F.status() == 0 and bool(torch.isfinite(X).all())
        assert np.array_equal(_solve(F, ctx, d, x), x0), m       # same pointers as the captured graph
    ctx.close()
