"""-m gpu: the solves of the DEVICE supernodal factor (csrc/sn_chol.hpp, sn_solve1.hpp, sn_factor.hpp; DDM_DIRECT_ENGINE=device)
WITHOUT iterative refinement (DDM_DIRECT_REFINE=off), on every route the host driver can take.

The cases, what each reaches and the proof that it does are in tests/sn_cases.py and tests/test_sn_cases_reference.py (CPU).
Single-vector routes (sn_cases.ROUTES, set through the environment before the factor is created): the default (dense chains in
k_sn_top_chain), DDM_SN_CHAINS=0 (k_sn_top1, link by link), DDM_SN_TOP_MAX=0 (level launches only: k_sn_fwd1 / k_sn_bwd1_diag /
k_sn_bwd1_partial at <64> and <128>, the one-wavefront kernels), the same with DDM_SN_SMALL_KERNELS=0, and DDM_SN_TOP_SPREAD = 0 / 1
on the cases with fewer than 8 blocks.  Block solves (k_sn_fwd_diag / k_sn_fwd_update / k_sn_bwd_partial / k_sn_bwd_diag) at the
widths 1, 2, 5, 16, 17, 24, 47, 48, 49, 97: one column through the block kernels, the edges of the 16-column tiles of the matrix
cores (mpad) and of the 48-column panel, two and three panels.  Every factor is asserted to be the device supernodal one with no
refinement step; every output is filled with NaN first; F.status() == 0 after every solve.

  (a) Evaluated.ratio <= 1: |d - A x| <= u (C g + 2 h) row by row, g = |L| |U| |x| from the SciPy / numpy reference factor, C from
      the row widths of the factor, h the term of the explicitly inverted triangles -- supernodes, or whole chains on the routes
      that run them (derivation: the module docstring of sn_cases; the float64 reference solve measures 4.2e-4 .. 1.7e-3, a dropped
      entry of L, a skipped row of an update or a pivot that is not applied 1.7 10^6 or more);
  (b) two routes of one case, and a column of a block solve against the single-vector solve of that column, differ by no more
      than their two bounds allow: Evaluated.difference <= 1;
  (c) a replay gives the bits of the first solve, (d) a second factor of the same matrix gives them too, on every route and width;
  (e) the "pivoting" matrix of tests/test_gpu_sn_chol.py, which needs refinement by design, goes through every route and width
      with refinement on under that test's criterion: probe backward error om[steps] <= 1e-12 and a backward error of the solve
      ||A X - B|| / (||A||_inf ||X|| + ||B||) <= 1e-12.
  (f) L U cases, once per route and factor: F.sn_pivots() -- the order k_sn_lu_diag chose -- equals the reference's replay of the
      threshold rule entry for entry: the identity for lu13 / lu17, the designed exchanges for lx13 / lx17 / lx21 (pairs, 3-cycles,
      several groups per block, in supernodes of every solve class: tests/test_sn_cases_reference.py, (iii) and (iv)).  A wrong
      choice of pivot gives a valid factor of another ordering, which the residual alone need not notice; with the order pinned,
      (a) on these cases -- UNREFINED, no growth -- is the test of every consumer of the order (k_sn_lu_panel, s1_gather behind
      k_sn_fwd1, k_sn_fwd1_small, k_sn_top1, k_chain_scatter, k_sn_fwd_diag): the reference with the exchange of one supernode
      left out, inverted, or not applied to its U panel measures 1.1e11 .. 3.3e12 of the bound.
  (g) test_refresh_between_dominant_and_exchanging_values: a factor refreshed lu13 -> lx13 -> lu13 -> lx13 (lu17 / lx17) on every
      route reports identity -> Q -> identity -> Q and solves with the bits of factors created on those values: a stale d_piv or a
      stale chain inverse (k_chain_scatter folds the order in) shows here.  (tests/test_gpu_sn_refresh.py runs its own pairs on the
      lx cases too.)
  (h) test_vanishing_pivot_column: a pivot column that vanishes inside its diagonal block is replaced by sqrt(eps) max |a_ij|
      and the refinement the library decides repairs it, under criterion (e); the CPU replay predicted 2 steps and the probe
      backward errors 6.28e-09, 1.48e-14, 2.35e-17, one MI355X measured 2 steps and 6.28e-09, 1.48e-14, 2.32e-17 (solves: 4.8e-17,
      17 columns 3.0e-17).  Its ancestors' blocks have real threshold decisions (the closest kept at 0.38 amax), so its order,
      the identity, also pins the threshold itself.

Measured on one MI355X, (a) as a fraction of the bound (1 = the bound):

  case     default  links    levels   levels_nosmall  spread0 / 1  block widths (all columns)  (b) two routes  (b) block column / single
  one21    4.18e-4  5.44e-4  7.55e-4  4.58e-4         4.18e-4      4.2e-4 .. 1.07e-3          3.9e-4          2.2e-4 .. 3.7e-4
  many     3.46e-3  3.46e-3  3.46e-3  1.94e-3         -            2.0e-3 .. 3.84e-3          1.8e-3          1.7e-3 .. 3.2e-3
  eight17  2.10e-3  2.03e-3  2.09e-3  1.07e-3         -            1.2e-3 .. 2.18e-3          1.2e-3          1.1e-3 .. 1.2e-3
  twelve   2.07e-3  2.01e-3  2.03e-3  1.14e-3         -            1.3e-3 .. 2.15e-3          9.9e-4          9.6e-4 .. 1.1e-3
  flat2d   1.83e-3  1.81e-3  2.04e-3  1.51e-3         1.83e-3      1.5e-3 .. 2.55e-3          9.3e-4          6.4e-4 .. 7.2e-4
  chain1d  4.17e-3  4.17e-3  4.17e-3  4.17e-3         4.17e-3      2.2e-3 .. 5.78e-3          8.5e-4          2.2e-4 .. 1.1e-3
  lu13     1.18e-3  1.23e-3  2.05e-3  8.96e-4         1.18e-3      9.7e-4 .. 2.36e-3          1.1e-3          4.4e-4 .. 6.9e-4
  lu17     2.59e-3  2.57e-3  2.58e-3  1.52e-3         -            1.5e-3 .. 2.81e-3          1.3e-3          1.4e-3 .. 1.8e-3
  lx13     1.66e-3  1.69e-3  2.31e-3  1.85e-3         1.66e-3      1.5e-3 .. 2.75e-3          1.2e-3          6.5e-4 .. 9.9e-4
  lx17     3.95e-3  3.96e-3  3.96e-3  1.82e-3         -            1.9e-3 .. 3.26e-3          1.8e-3          1.6e-3 .. 1.8e-3
  lx21     7.54e-4  7.73e-4  1.38e-3  8.18e-4         7.54e-4      9.2e-4 .. 1.42e-3          7.6e-4          3.8e-4 .. 4.2e-4

(many has no top levels: its first three routes are one; the spread switch does not change the arithmetic, only the hand-overs.)
The device stands where the float64 reference stands (4.2e-4 .. 1.7e-3).  (e): probe backward error 3.0e-13 .. 9.4e-13 unrefined,
2.4e-18 .. 3.1e-18 after the one step every route takes; backward error of the solves 3.8e-22 .. 7.3e-22.
What the criterion notices: with the partial products of the big supernodes rounded to SINGLE precision in k_sn_bwd1_diag<128>
alone (an experiment, not committed), one21 / levels measures 1.1e4 and fails, while every test of tests/test_gpu_sn_chol.py passes.
With k_chain_scatter ignoring the pivot order of every link but the first of its chain (an experiment, not committed), the default
route of lx13 / lx17 / lx21 measures 2.6e12 / 2.1e12 / 1.9e12 and fails; the "pivoting" matrix fails too, but at creation, with
an error from the refinement probe that does not tell this from growth.

No case is skipped or filtered at run time."""
import numpy as np
import pytest

from tests import sn_cases as sc

pytestmark = pytest.mark.gpu


def _factor(ddm, ctx, M, block_ptr, general, refined=False):
    F = ddm.Ilu0(ctx, ddm.CsrMatrix(ctx, M), block_ptr, direct=True, general=general)
    assert ctx.lib.ddm_ilu0_is_direct(F.h) == 1 and F.engine() == "supernodal"
    if not refined:
        assert F.refinement()[0] == 0
    return F


def _solve(F, ctx, dd, xd):
    """one vector (F.solve) or a block (F.solve_multi) into the NaN-filled xd"""
    xd.fill_(float("nan"))
    if dd.dim() == 1:
        F.solve(dd, xd)
    else:
        F.solve_multi(dd, xd)
    ctx.sync()
    assert F.status() == 0
    return xd.cpu().numpy().copy()


def _orders(c):
    """the reference's pivot orders as ddm_ilu0_sn_pivots reports them: entry first[s] + k = the block-local row in position k"""
    return (c.ref.src - c.S.first[c.S.sn_of_col]).astype(np.int32)


def _assert_pivots(ddm, F, c, what):
    """(f); the Cholesky factor has no order to report"""
    if not c.general:
        with pytest.raises(ddm.DdmError) as e:
            F.sn_pivots()
        assert e.value.code == ddm.DDM_EINVAL, str(e.value)
        return
    got, want = F.sn_pivots(), _orders(c)
    wrong = np.flatnonzero(got != want)
    assert not len(wrong), (c.name, what, f"{len(wrong)} positions differ from the reference's order, the first in supernode {c.S.sn_of_col[wrong[0]]}: "
                            f"device {got[wrong[:8]]}, reference {want[wrong[:8]]}")


def _route_solution(ddm, ctx, c, route, dd, xd, monkeypatch):
    """(a), (c), (d), (f) of one single-vector route; returns its Evaluated"""
    c.env(monkeypatch, route)
    F = _factor(ddm, ctx, c.M, c.block_ptr, c.general)
    _assert_pivots(ddm, F, c, route)
    x = _solve(F, ctx, dd, xd)
    assert np.array_equal(_solve(F, ctx, dd, xd), x), (c.name, route, "replay differs from the first solve")
    F2 = _factor(ddm, ctx, c.M, c.block_ptr, c.general)
    _assert_pivots(ddm, F2, c, route)
    assert np.array_equal(_solve(F2, ctx, dd, xd), x), (c.name, route, "a second factor of the same matrix gives other bits")
    E = c.evaluate(c.d, x, route)
    sh = c.shapes[route]
    print(f"[sn routes] {c.name} {route} (ntop = {sh.ntop}, bottom {sh.levels()}, {len(sh.chains)} chains, spread {int(sh.spread)}): (a) ratio {E.ratio():.3e}")
    assert E.ratio() <= 1.0, (c.name, route, E.ratio())
    return E


@pytest.mark.parametrize("name", sc.NAMES)
def test_single_vector_routes(ddm, name, monkeypatch):
    """F.solve on every route of the case: (a), (c), (d) per route, (b) for every pair of routes"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device (no CPU fallback exists)"
    c = sc.case(name)
    ctx = ddm.torch_context(0)
    dd = torch.tensor(c.d).cuda()
    xd = torch.empty(c.n, dtype=torch.float64, device="cuda")
    print()
    E = {route: _route_solution(ddm, ctx, c, route, dd, xd, monkeypatch) for route in c.routes}
    worst = 0.0
    for i, ra in enumerate(c.routes):
        for rb in c.routes[i + 1:]:
            diff = E[ra].difference(E[rb])
            worst = max(worst, diff)
            assert diff <= 1.0, (name, ra, rb, diff)
    print(f"[sn routes] {name}: (b) largest difference of two routes {worst:.3e} of what their bounds allow")
    ctx.close()


@pytest.mark.parametrize("name,width", [(n, w) for n in sc.NAMES for w in sc._CASES[n][2]])
def test_block_width(ddm, name, width, monkeypatch):
    """F.solve_multi of `width` columns: (a) per column, (c), (d); (b) for the last column against its single-vector solve on the
    default route (through the same factor, after the block solve)"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device (no CPU fallback exists)"
    c = sc.case(name)
    c.env(monkeypatch, "default")
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, c.M, c.block_ptr, c.general)
    D = np.ascontiguousarray(c.D[:, :width])
    Dd = torch.tensor(D).cuda()
    Xd = torch.empty((c.n, width), dtype=torch.float64, device="cuda")
    X = _solve(F, ctx, Dd, Xd)
    assert np.array_equal(_solve(F, ctx, Dd, Xd), X), (name, width, "replay differs from the first solve")
    F2 = _factor(ddm, ctx, c.M, c.block_ptr, c.general)
    assert np.array_equal(_solve(F2, ctx, Dd, Xd), X), (name, width, "a second factor of the same matrix gives other bits")
    E = c.evaluate(D, X)
    ratio = E.ratio()
    j = width - 1
    dj = np.ascontiguousarray(D[:, j])
    xj = _solve(F, ctx, torch.tensor(dj).cuda(), torch.empty(c.n, dtype=torch.float64, device="cuda"))
    diff = E.column(j).difference(c.evaluate(dj, xj, "default"))
    print(f"\n[sn routes] {name} width {width} ({len(sc.panels(width))} panel(s), mpad {[sc.mpad(w) for _, w in sc.panels(width)]}): (a) ratio {ratio.min():.3e} .. {ratio.max():.3e}; "
          f"(b) column {j} against its single-vector solve {diff:.3e}")
    assert ratio.max() <= 1.0, (name, width, ratio)
    assert diff <= 1.0, (name, width, diff)
    ctx.close()


@pytest.mark.parametrize("name", tuple(sc.SAME_PATTERN))
def test_refresh_between_dominant_and_exchanging_values(ddm, name, monkeypatch):
    """(g) on every route: a factor created on the column dominant values of the same pattern is refreshed to the exchanging ones
    and back and forth again; after every refresh (f) for the values at hand, and the solve (graph captured before the first
    refresh) gives the bits of a factor created on them"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device (no CPU fallback exists)"
    cases = {"exchanging": sc.case(name), "dominant": sc.case(sc.SAME_PATTERN[name])}
    c = cases["exchanging"]
    assert not np.array_equal(_orders(cases["dominant"]), _orders(c)) and not cases["dominant"].ref.exchanging.any()
    ctx = ddm.torch_context(0)
    dd = torch.tensor(c.d).cuda()
    xd = torch.empty(c.n, dtype=torch.float64, device="cuda")
    for route in c.routes:
        c.env(monkeypatch, route)
        fresh = {}
        for key, k in cases.items():
            F = _factor(ddm, ctx, k.M, k.block_ptr, True)
            fresh[key] = _solve(F, ctx, dd, xd)
            del F
        assert not np.array_equal(fresh["dominant"], fresh["exchanging"])
        F = _factor(ddm, ctx, cases["dominant"].M, c.block_ptr, True)
        _assert_pivots(ddm, F, cases["dominant"], route)
        assert np.array_equal(_solve(F, ctx, dd, xd), fresh["dominant"])
        for count, key in enumerate(("exchanging", "dominant", "exchanging"), start=1):
            F.A.set_values(cases[key].M.data)
            F.refresh()
            assert F.engine() == "supernodal" and F.refinement()[0] == 0 and F.refresh_count() == count
            _assert_pivots(ddm, F, cases[key], (route, "refreshed to the", key, "values"))
            x = _solve(F, ctx, dd, xd)
            assert np.array_equal(x, fresh[key]), (name, route, key, f"{int(np.sum(x != fresh[key]))} entries differ from the fresh factor's")
            assert np.array_equal(_solve(F, ctx, dd, xd), x), (name, route, key, "replay after the refresh")
        del F
    ctx.close()


def _backward_error(M, anorm, X, B):
    return float(np.linalg.norm(M @ X - B) / (anorm * np.linalg.norm(X) + np.linalg.norm(B)))


def test_vanishing_pivot_column(ddm, monkeypatch):
    """sn_cases.vanishing_column_matrix(): k_sn_lu_diag replaces the pivot of a column that vanishes inside its diagonal block by
    sqrt(eps) max |a_ij| and the refinement the library decides repairs it (predicted on the CPU by
    tests/test_sn_cases_reference.py: 2 steps, probe backward errors 6.28e-09, 1.48e-14, 2.35e-17, and no row exchanged anywhere).
    Criterion (e), with (c) and (d)."""
    import torch
    M, bp, tiny = sc.vanishing_column_matrix()
    anorm = float(abs(M).sum(axis=1).max())
    B = np.random.default_rng(13).standard_normal((M.shape[0], 17))
    monkeypatch.setenv("DDM_DIRECT_ENGINE", "device")
    monkeypatch.delenv("DDM_DIRECT_REFINE", raising=False)
    sc.set_route(monkeypatch, "default")
    ctx = ddm.torch_context(0)

    def factor():
        F = _factor(ddm, ctx, M, bp, True, refined=True)
        steps, om = F.refinement()
        assert steps >= 1 and om[0] > 1e-13, (steps, om)               # the perturbed pivot needs its refinement
        assert om[steps] <= 1e-12, (steps, om)
        assert np.array_equal(F.sn_pivots(), _orders(sc.case("lu13")))   # (the vanishing column keeps its row; no other is exchanged)
        return F, steps, om
    F, steps, om = factor()
    F2 = factor()[0]
    for Bw in (np.ascontiguousarray(B[:, 0]), B):
        Bd = torch.tensor(Bw).cuda()
        Xd = torch.empty_like(Bd)
        X = _solve(F, ctx, Bd, Xd)
        omega = _backward_error(M, anorm, X, Bw)
        print(f"\n[sn routes] vanishing column, {1 if Bw.ndim == 1 else Bw.shape[1]} column(s): {steps} refinement step(s), probe backward errors {om[:steps + 1]}, "
              f"backward error of the solve {omega:.2e}")
        assert omega <= 1e-12, omega
        assert np.array_equal(_solve(F, ctx, Bd, Xd), X), "replay differs from the first solve"
        assert np.array_equal(_solve(F2, ctx, Bd, Xd), X), "a second factor of the same matrix gives other bits"
    ctx.close()


@pytest.fixture(scope="module")
def pivoting():
    M, bp = sc.pivoting_matrix()
    assert abs(M - M.T).max() > 1e-3 * abs(M).max()
    B = np.random.default_rng(11).standard_normal((M.shape[0], sc.MAX_WIDTH))
    B.setflags(write=False)
    return M, bp, float(abs(M).sum(axis=1).max()), B


def _pivoting_factor(ddm, ctx, M, bp, route, monkeypatch):
    """refinement as the library decides it (DDM_DIRECT_REFINE unset), under the criterion of test_device_lu_matches_superlu"""
    monkeypatch.setenv("DDM_DIRECT_ENGINE", "device")
    monkeypatch.delenv("DDM_DIRECT_REFINE", raising=False)
    sc.set_route(monkeypatch, route)
    F = _factor(ddm, ctx, M, bp, True, refined=True)
    steps, om = F.refinement()
    assert steps >= 1 and om[0] > 1e-13, (route, steps, om)           # the matrix needs its refinement: rows are exchanged, growth ~1e6
    assert om[steps] <= 1e-12, (route, steps, om)
    return F, steps, om


@pytest.mark.parametrize("route", sc.routes_of(1))
def test_pivoting_matrix_single_vector_route(ddm, pivoting, route, monkeypatch):
    """(e) for F.solve, with (c) and (d)"""
    import torch
    M, bp, anorm, B = pivoting
    ctx = ddm.torch_context(0)
    F, steps, om = _pivoting_factor(ddm, ctx, M, bp, route, monkeypatch)
    b = np.ascontiguousarray(B[:, 0])
    bd = torch.tensor(b).cuda()
    xd = torch.empty(len(b), dtype=torch.float64, device="cuda")
    x = _solve(F, ctx, bd, xd)
    omega = _backward_error(M, anorm, x, b)
    print(f"\n[sn routes] pivoting {route}: {steps} refinement step(s), probe backward errors {om[:steps + 1]}, backward error of the solve {omega:.2e}")
    assert omega <= 1e-12, (route, omega)
    assert np.array_equal(_solve(F, ctx, bd, xd), x), (route, "replay differs from the first solve")
    F2, _, _ = _pivoting_factor(ddm, ctx, M, bp, route, monkeypatch)
    assert np.array_equal(_solve(F2, ctx, bd, xd), x), (route, "a second factor of the same matrix gives other bits")
    ctx.close()


@pytest.mark.parametrize("width", sc.WIDTHS_FULL)
def test_pivoting_matrix_block_width(ddm, pivoting, width, monkeypatch):
    """(e) for F.solve_multi, with (c) and (d)"""
    import torch
    M, bp, anorm, B = pivoting
    ctx = ddm.torch_context(0)
    F, steps, om = _pivoting_factor(ddm, ctx, M, bp, "default", monkeypatch)
    Bw = np.ascontiguousarray(B[:, :width])
    Bd = torch.tensor(Bw).cuda()
    Xd = torch.empty(Bw.shape, dtype=torch.float64, device="cuda")
    X = _solve(F, ctx, Bd, Xd)
    omega = _backward_error(M, anorm, X, Bw)
    print(f"\n[sn routes] pivoting width {width}: {steps} refinement step(s), backward error of the block {omega:.2e}")
    assert omega <= 1e-12, (width, omega)
    assert np.array_equal(_solve(F, ctx, Bd, Xd), X), (width, "replay differs from the first solve")
    F2, _, _ = _pivoting_factor(ddm, ctx, M, bp, "default", monkeypatch)
    assert np.array_equal(_solve(F2, ctx, Bd, Xd), X), (width, "a second factor of the same matrix gives other bits")
    ctx.close()
