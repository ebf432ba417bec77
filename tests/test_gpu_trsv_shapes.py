"""-m gpu: the ILU(0) solves of the engines that take every matrix -- xcd2 (k_trsv_xcd2) and levels (k_trsv_small_levels,
k_trsv_lower_level, k_trsv_upper_level) -- and the block sweeps every ILU(0) factor runs its multi-RHS solves on
(k_trsv_level_multi, _multi4, _multi4_f32, _multi_wide), at the shapes those kernels branch on.

The cases, what each reaches and the proof that it does are in tests/trsv_cases.py and tests/test_trsv_cases_reference.py (CPU).
Two checks per result:

  (a) residual_ratio(M, F.factors(), d, x, 2^-53) <= C = 2 (w_L + w_U + 3): L U x = d against the library's own factor array in
      numpy.longdouble, |d - L U x| <= C u |L| |U| |x| row by row (derivation: trsv_cases.bound; the oracle measures 1..7 against
      C = 10..8410, a dropped or stale operand 10^9 or more);
  (b) bit equality with the oracle's sequential solve wherever the kernel sums a row in ascending column order with every product
      rounded before it is subtracted: every xcd2 result (tile entries, then the global tail), every pipe result, and every levels
      result of a case whose merged level schedule has no level in the "few wide rows" branch of k_trsv_small_levels (w >= 32 and
      2 m <= 1024: S lanes per row and a butterfly sum) -- decided from level_table, not by hand.  Where that branch is taken: (a)
      and RTOL_VEC of the largest entry.

The block sweeps are compared column by column with (a) and with the single-vector solve: `==` where every level sums in column
order (no level of w >= 96, or more than 256 columns: the quad / scalar kernels), RTOL_APPLY where k_trsv_level_multi_wide adds
slice sums.  No case is skipped or filtered at run time."""
import numpy as np
import pytest

from tests import trsv_cases as tc
from tests.pipe_cases import TRSV_CASES_ENGINE
from tests.test_gpu_multi_rhs import RTOL_APPLY
from tests.test_gpu_parity import RTOL_VEC

pytestmark = pytest.mark.gpu

U64, U32 = 2.0 ** -53, 2.0 ** -24
MODES = ("xcd2", "levels", "pipe")
SWEEP_WIDTHS = {"band17": (1, 3, 4, 7, 24, 32), "elasticity": (1, 3, 4, 7, 24, 32), "blocks9": (1, 3, 4, 7, 24, 32),
                # 7, 24: 256 / m inexact; 130, 256: one slice; 260 > 256: the quad kernel on the w >= 96 level
                "wide": (1, 7, 24, 130, 256, 260), "layers": (1, 7, 24, 130, 256, 260)}
WG = 256


class Ref:
    """per case, computed once and never changed: the oracle's factor, two right-hand sides and its solves of them, a block of
    columns for the sweeps"""

    def __init__(self, name):
        self.c = c = tc.case(name)
        rng = np.random.default_rng(41)
        self.d = [rng.standard_normal(c.n), rng.standard_normal(c.n)]
        self.lu, x0 = tc.oracle_factor_and_solve(c, self.d[0])
        self.x = [x0, tc.oracle_factor_and_solve(c, self.d[1])[1]]
        self.D = rng.standard_normal((c.n, max(SWEEP_WIDTHS.get(name, (8,)))))
        for a in (self.d[0], self.d[1], self.lu, self.x[0], self.x[1], self.D):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def refs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Ref(name)
        return made[name]
    return get


def _wide_levels(c):
    return any(bool(np.any(t.w >= tc.WIDE_W)) for t in c.whole.triangles)


def _factor(ddm, ctx, c):
    return ddm.Ilu0(ctx, ddm.CsrMatrix(ctx, c.M), c.block_ptr)


def _check_factors(F, ref):
    lu = F.factors()
    dev = float(np.max(np.abs(lu - ref.lu)) / np.max(np.abs(ref.lu)))
    assert dev < 1e-13, dev                                     # same elimination order on the host
    return lu


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", tc.NAMES)
def test_single_vector_solve(ddm, refs, name, mode, monkeypatch):
    """F.solve on every case with DDM_TRSV_MODE = xcd2, levels and pipe (the default path: pipe, or xcd2 where pipe declines the
    matrix): factors against the oracle's, three solves into a NaN-filled x (the capture and two replays with re-used epochs and
    flags; the third with another right-hand side), status 0 after each, checks (a) and (b) of the module docstring."""
    import torch
    monkeypatch.setenv("DDM_TRSV_MODE", mode)
    ref = refs(name)
    c = ref.c
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, c)
    res = tc.Residual(c.M, _check_factors(F, ref))
    dd = [torch.tensor(d).cuda() for d in ref.d]
    xd = torch.empty(c.n, dtype=torch.float64, device="cuda")
    got = []
    for k in (0, 0, 1):
        xd.fill_(float("nan"))
        F.solve(dd[k], xd)
        ctx.sync()
        assert F.status() == 0, (name, mode, F.engine(), len(got))
        got.append((k, xd.cpu().numpy().copy()))
    engine = F.engine()
    # pipe mode: the engine the host builder's verdict on the case implies (recorded by tests/test_pipe_cases_reference.py)
    assert engine == (TRSV_CASES_ENGINE[name] if mode == "pipe" else mode), (mode, engine)
    if len(c.block_ptr) == 2:
        L, U = c.table.blocks[0]
        assert (F.num_levels(False), F.num_levels(True)) == (L.nlev, U.nlev), (name, mode, engine)
    column_order = engine != "levels" or not any(bool(np.any(tc.few_wide(t))) for t in c.whole.triangles)
    for rep, (k, x) in enumerate(got):
        ratio = res.ratio(ref.d[k], x, U64)
        dev = float(np.max(np.abs(x - ref.x[k])) / np.max(np.abs(ref.x[k]))) if np.isfinite(x).all() else float("inf")
        bad = int(np.sum(x != ref.x[k]))
        print(f"\n{name} {mode} (engine {engine}) solve {rep}: residual ratio {ratio:.2f} (C = {c.C}), deviation from the oracle {dev:.2e}, "
              f"{bad} of {c.n} entries differ, column order: {column_order}")
        assert ratio <= c.C, (name, mode, engine, rep, ratio, c.C)
        if column_order:
            assert np.array_equal(x, ref.x[k]), (name, mode, engine, rep, bad, dev)
        else:
            assert dev < RTOL_VEC, (name, mode, engine, rep, dev)
    assert np.array_equal(got[0][1], got[1][1]), (name, mode, engine, "replay differs from the first solve")
    ctx.close()


def _single_columns(F, ctx, D):
    """F.solve on every column of the device block D: (n, m) host array"""
    import torch
    out = []
    for j in range(D.shape[1]):
        dj = D[:, j].contiguous()
        xj = torch.full_like(dj, float("nan"))
        F.solve(dj, xj)
        ctx.sync()
        out.append(xj.cpu().numpy().copy())
    return np.stack(out, axis=1)


@pytest.mark.parametrize("name", sorted(SWEEP_WIDTHS))
def test_block_sweeps(ddm, refs, name, monkeypatch):
    """F.solve_multi (default engine; the sweeps run on the level schedule) for the widths of SWEEP_WIDTHS on the first m columns
    of one block: every column passes (a); every column equals the single-vector F.solve of it bit for bit unless
    k_trsv_level_multi_wide ran (a level of w >= 96 and m <= 256), where RTOL_APPLY of the column's largest entry holds; a
    misaligned (n, 8) block (8 bytes into its allocation, D and X: the scalar kernel) gives the bits of the aligned call (the
    quad kernel)."""
    import torch
    monkeypatch.delenv("DDM_TRSV_MODE", raising=False)
    ref = refs(name)
    c = ref.c
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, c)
    res = tc.Residual(c.M, _check_factors(F, ref))
    Dd = torch.tensor(ref.D).cuda()
    mmax = Dd.shape[1]
    single = _single_columns(F, ctx, Dd)
    assert F.status() == 0
    wide = _wide_levels(c)
    failures = []
    for m in SWEEP_WIDTHS[name]:
        D = Dd[:, :m].contiguous()
        X = torch.full_like(D, float("nan"))
        F.solve_multi(D, X)
        ctx.sync()
        Xh = X.cpu().numpy()
        ratios = [res.ratio(ref.D[:, j], Xh[:, j], U64) for j in range(m)]
        exact = not (wide and m <= WG)
        if np.isfinite(Xh).all():
            dev = float(np.max(np.max(np.abs(Xh - single[:, :m]), axis=0) / np.max(np.abs(single[:, :m]), axis=0)))
        else:
            dev = float("inf")
        print(f"\n{name} m = {m}: worst residual ratio {max(ratios):.2f} (C = {c.C}), deviation from the single-vector solve {dev:.2e} "
              f"({'==' if exact else 'RTOL_APPLY'})")
        if not max(ratios) <= c.C:
            failures.append((m, "residual", max(ratios)))
        if exact and not np.array_equal(Xh, single[:, :m]):
            failures.append((m, "not the single-vector bits", dev))
        if not exact and not dev <= RTOL_APPLY:
            failures.append((m, "single-vector", dev))
    assert not failures, failures
    assert mmax >= 8
    # aligned (quad kernel) against misaligned (scalar kernel) on 8 columns
    D8 = Dd[:, :8].contiguous()
    X8 = torch.full_like(D8, float("nan"))
    assert D8.data_ptr() % 32 == 0 and X8.data_ptr() % 32 == 0
    F.solve_multi(D8, X8)
    bufD = torch.empty(c.n * 8 + 1, dtype=torch.float64, device="cuda")
    bufX = torch.full((c.n * 8 + 1,), float("nan"), dtype=torch.float64, device="cuda")
    Dm, Xm = bufD[1:].view(c.n, 8), bufX[1:].view(c.n, 8)
    Dm.copy_(D8)
    assert Dm.is_contiguous() and Dm.data_ptr() % 32 == 8 and Xm.data_ptr() % 32 == 8
    F.solve_multi(Dm, Xm)
    ctx.sync()
    assert F.status() == 0
    assert np.isfinite(X8.cpu().numpy()).all() and torch.equal(X8, Xm), name
    ctx.close()


@pytest.mark.parametrize("name, m", [("wide", 8), ("band17", 6), ("elasticity", 6)])
def test_single_precision_request_answered_in_double(ddm, refs, name, m, monkeypatch):
    """single_precision=True on a factor with a level of w >= 96 (`wide`) or a width that is no multiple of 4: ilu0_solve_multi_ld
    declines f32 and the double sweeps answer, bit for bit"""
    import torch
    monkeypatch.delenv("DDM_TRSV_MODE", raising=False)
    ref = refs(name)
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, ref.c)
    D = torch.tensor(ref.D[:, :m]).cuda().contiguous()
    X64, X32 = torch.full_like(D, float("nan")), torch.full_like(D, float("nan"))
    F.solve_multi(D, X64)
    F.solve_multi(D, X32, single_precision=True)
    ctx.sync()
    assert F.status() == 0
    assert bool(torch.isfinite(X64).all()) and torch.equal(X64, X32)
    ctx.close()


@pytest.mark.parametrize("m", [4, 24])
@pytest.mark.parametrize("name", ["band17", "elasticity"])
def test_single_precision_sweeps(ddm, refs, name, m, monkeypatch):
    """k_trsv_level_multi4_f32 with w > 16: not the double result; a second call and a call into another output block give the
    same bits; every column satisfies residual_ratio(..., u = 2^-24) <= 2 (w_L + w_U + 5) (the derivation of (a) with one more
    rounding of every factor entry and of d to float)."""
    import torch
    monkeypatch.delenv("DDM_TRSV_MODE", raising=False)
    ref = refs(name)
    c = ref.c
    C32 = tc.bound(c.table, extra=5)
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, c)
    res = tc.Residual(c.M, _check_factors(F, ref))
    D = torch.tensor(ref.D[:, :m]).cuda().contiguous()
    X64, Xa, Xb = (torch.full_like(D, float("nan")) for _ in range(3))
    F.solve_multi(D, X64)
    F.solve_multi(D, Xa, single_precision=True)
    ctx.sync()
    first = Xa.clone()
    Xa.fill_(float("nan"))
    F.solve_multi(D, Xa, single_precision=True)                # replay of the captured graph
    F.solve_multi(D, Xb, single_precision=True)                # another output block: a new capture
    ctx.sync()
    assert F.status() == 0
    Xh = Xa.cpu().numpy()
    ratios = [res.ratio(ref.D[:, j], Xh[:, j], U32) for j in range(m)]
    dev = float(np.max(np.abs(Xh - X64.cpu().numpy())) / np.max(np.abs(X64.cpu().numpy()))) if np.isfinite(Xh).all() else float("inf")
    print(f"\n{name} m = {m} f32: worst residual ratio {max(ratios):.2f} (C = {C32}), deviation from the double sweeps {dev:.2e}")
    assert np.isfinite(Xh).all() and bool(torch.isfinite(X64).all())
    assert not torch.equal(Xa, X64)
    assert torch.equal(Xa, first) and torch.equal(Xa, Xb)
    assert max(ratios) <= C32, (ratios, C32)
    ctx.close()
