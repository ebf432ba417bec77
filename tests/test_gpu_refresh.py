"""-m gpu: the value refresh through every layer -- ddm_csr_set_values + ddm_ilu0_refresh (device ILU(0) factorisation along the
L level schedule, scatter into the level and pipe engines, xcd2 rebuilt), ddm_op_refresh, ddm_galerkin_set_inverse and
TwoLevelSchwarz.update_values -- against objects created on the new values.  One criterion throughout: bit equality (`==`), no
tolerance.  "New values" are tests/refresh_cases.py: every entry times a factor in [0.7, 1.3], rows strictly diagonally dominant
(asserted here on the CPU).  Every test solves at least once BEFORE the refresh with the device buffers it uses afterwards, so a
stale captured graph or a stale buffer shows."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import pipe_cases as pc
from tests import refresh_cases as rc
from tests import trsv_cases as tc
from tests.dia_cases import vector
from tests.dia_code_cases import code_cases
from tests.test_fgmres_cpu import golden_poisson

pytestmark = pytest.mark.gpu

MODES = (None, "levels", "xcd2")                                 # None: DDM_TRSV_MODE unset (pipe, or what it hands the matrix to)
# pipe-engine cases of tests/pipe_cases.py: layered26 -- one block of 5000 rows per level: spread mode, W = 26, remote operands in
# every slot class; mix9 -- 9 uneven blocks, tasks of 1, 2 and 3 steps and longer, a packed task, a one-row block; fanin112 -- tasks
# of 2 and 3 steps with 112 producers
PIPE_NAMES = ("layered26", "mix9", "fanin112")


def _set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("DDM_TRSV_MODE", raising=False)
    else:
        monkeypatch.setenv("DDM_TRSV_MODE", mode)


class Solves:
    """one factor with its device buffers: a single vector, a block of 5 and a block of 8 columns (the latter with float sweeps)"""

    def __init__(self, ddm, ctx, M, block_ptr, seed=17):
        import torch
        self.torch, self.ctx = torch, ctx
        self.A = ddm.CsrMatrix(ctx, M)
        self.F = ddm.Ilu0(ctx, self.A, block_ptr)
        rng = np.random.default_rng(seed)
        n = M.shape[0]
        self.d, self.D5, self.D8 = (torch.as_tensor(rng.standard_normal(s)).cuda().contiguous() for s in ((n,), (n, 5), (n, 8)))
        self.x, self.X5, self.X8 = (torch.empty_like(t) for t in (self.d, self.D5, self.D8))

    def run(self):
        """(x, X5, X8) as host arrays, from NaN-filled outputs"""
        for t in (self.x, self.X5, self.X8):
            t.fill_(float("nan"))
        self.F.solve(self.d, self.x)
        self.F.solve_multi(self.D5, self.X5)
        self.F.solve_multi(self.D8, self.X8, single_precision=True)
        self.ctx.sync()
        assert self.F.status() == 0
        out = tuple(t.cpu().numpy().copy() for t in (self.x, self.X5, self.X8))
        assert all(np.isfinite(a).all() for a in out)
        return out


def _refresh_against_fresh(ddm, M, block_ptr, mode, monkeypatch, tag):
    _set_mode(monkeypatch, mode)
    M2 = rc.new_values(M, 11)
    rc.assert_dominant(M2)
    assert rc.same_pattern(M, M2)
    ctx = ddm.torch_context(0)
    S = Solves(ddm, ctx, M, block_ptr)
    before = S.run()
    S.run()                                                      # (a replay of the captured graphs)
    engine = S.F.engine()
    lu_before = S.F.factors()
    S.A.set_values(M2.data)
    S.F.refresh()
    lu = S.F.factors()
    after = S.run()
    assert S.F.engine() == engine
    fresh = Solves(ddm, ctx, M2, block_ptr)
    want = fresh.run()
    lu_want = fresh.F.factors()
    assert fresh.F.engine() == engine
    bad = int(np.sum(lu != lu_want))
    dev = float(np.max(np.abs(lu - lu_want)) / np.max(np.abs(lu_want)))
    print(f"\n{tag} {mode or 'default'} (engine {engine}): {bad} of {lu.size} factor entries differ from a fresh factor's (relative {dev:.2e}); "
          f"solves differ in {[int(np.sum(a != b)) for a, b in zip(after, want)]} entries")
    assert not np.array_equal(lu, lu_before) and not np.array_equal(after[0], before[0])
    assert np.array_equal(lu, lu_want), (tag, mode, bad, dev)
    for what, a, b in zip(("solve", "solve_multi (5)", "solve_multi_f32 (8)"), after, want):
        assert np.array_equal(a, b), (tag, mode, engine, what, int(np.sum(a != b)))
    second = S.run()                                             # and the refreshed factor replays
    assert all(np.array_equal(a, b) for a, b in zip(second, want))
    del S, fresh
    ctx.close()
    return engine


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", tc.NAMES)
def test_refreshed_factor_equals_a_fresh_one(ddm, name, mode, monkeypatch):
    """every matrix of tests/trsv_cases.py (rows of 17 .. 4200 entries: the LDS and the global path of the factorisation kernel; 600
    one-row levels; a level of 4192 rows; 1 .. 17 uneven blocks; DG and elasticity blocks) on the three engines a refresh serves"""
    c = tc.case(name)
    engine = _refresh_against_fresh(ddm, c.M, c.block_ptr, mode, monkeypatch, name)
    assert engine == (pc.TRSV_CASES_ENGINE[name] if mode is None else mode)


@pytest.mark.parametrize("name", PIPE_NAMES)
def test_refreshed_pipe_factor_equals_a_fresh_one(ddm, name, monkeypatch):
    c = pc.case(name)
    s = pc.schedule(name)
    if name == "layered26":                                      # build_pipe_schedule: nb < 8 and more than 48 * 64 rows per level
        assert c.nblocks < 8 and c.n / 4 > 48 * 64
    else:
        assert s.max_steps > 1 and s.short[2] > 0 and s.short[3] > 0
    assert _refresh_against_fresh(ddm, c.M, c.block_ptr, None, monkeypatch, name) == "pipe"


def _two_blocks():
    """block 0: 4 x 4 dominant; block 1: 3 x 3 whose new values have the singular leading part [[2, 1], [2, 1]]"""
    B0 = np.array([[4.0, 1.0, 0.0, 1.0], [1.0, 5.0, 1.0, 0.0], [0.0, 1.0, 4.0, 1.0], [1.0, 0.0, 1.0, 6.0]])
    B1 = np.array([[4.0, 1.0, 1.0], [2.0, 5.0, 1.0], [1.0, 1.0, 4.0]])
    B1s = np.array([[2.0, 1.0, 1.0], [2.0, 1.0, 1.0], [1.0, 1.0, 4.0]])
    M = sp.csr_matrix(sp.block_diag([B0, B1], format="csr"))
    Ms = sp.csr_matrix(sp.block_diag([1.25 * B0, B1s], format="csr"))
    M.sort_indices(), Ms.sort_indices()
    assert rc.same_pattern(M, Ms)
    return M, Ms, np.array([0, 4, 7], dtype=np.int64)


@pytest.mark.parametrize("mode", MODES)
def test_vanishing_pivot_is_an_error_return_and_keeps_the_factor(ddm, mode, monkeypatch):
    _set_mode(monkeypatch, mode)
    M, Ms, bp = _two_blocks()
    rc.assert_dominant(M)
    ctx = ddm.torch_context(0)
    S = Solves(ddm, ctx, M, bp)
    before = S.run()
    lu_before = S.F.factors()
    S.A.set_values(Ms.data)
    with pytest.raises(ddm.DdmError) as e:
        S.F.refresh()
    assert e.value.code == ddm.DDM_ENUMERIC and "block 1" in str(e.value), str(e.value)
    after = S.run()
    assert all(np.array_equal(a, b) for a, b in zip(after, before))
    assert np.array_equal(S.F.factors(), lu_before)
    # and a refresh after the failed one, on good values, is a fresh factor's again
    M3 = rc.new_values(M, 5)
    rc.assert_dominant(M3)
    S.A.set_values(M3.data)
    S.F.refresh()
    fresh = Solves(ddm, ctx, M3, bp)
    assert np.array_equal(S.F.factors(), fresh.F.factors())
    assert all(np.array_equal(a, b) for a, b in zip(S.run(), fresh.run()))
    del S, fresh
    ctx.close()


def test_direct_and_box_factors_refuse(ddm, monkeypatch):
    import torch
    from tests.test_gpu_pipe import _blocks
    ctx = ddm.torch_context(0)
    made = []
    monkeypatch.delenv("DDM_TRSV_MODE", raising=False)
    c = tc.case("blocks3")
    Ms = sp.csr_matrix(c.M + c.M.T)                              # (symmetric positive definite: dominant, positive diagonal)
    Ms.sort_indices()
    A = ddm.CsrMatrix(ctx, Ms)
    made.append((A, ddm.Ilu0(ctx, A, c.block_ptr, direct=True), Ms, "direct"))
    monkeypatch.setenv("DDM_TRSV_MODE", "box")
    Mb, bpb = _blocks(ddm, (9, 8, 7), (1, 1, 1))
    Mb = sp.csr_matrix(Mb)
    Mb.sort_indices()
    A = ddm.CsrMatrix(ctx, Mb)
    made.append((A, ddm.Ilu0(ctx, A, bpb), Mb, "box"))
    assert made[1][1].engine() == "box"
    for A, F, M, what in made:
        n = M.shape[0]
        d = torch.as_tensor(np.random.default_rng(3).standard_normal(n)).cuda()
        x = torch.full_like(d, float("nan"))
        F.solve(d, x)
        ctx.sync()
        x0 = x.cpu().numpy().copy()
        A.set_values(1.5 * M.data)
        with pytest.raises(ddm.DdmError) as e:
            F.refresh()
        assert e.value.code == ddm.DDM_ENOTIMPL and "create a new factor" in str(e.value), (what, str(e.value))
        x.fill_(float("nan"))
        F.solve(d, x)
        ctx.sync()
        assert np.isfinite(x0).all() and np.array_equal(x.cpu().numpy(), x0), what
    del made, A, F
    ctx.close()


def _bits(t):
    import torch
    return t.view(torch.int64)


def test_operator_refresh_both_directions(ddm, monkeypatch):
    """the matrices of tests/dia_code_cases.py: blocks on at most 16 distinct values (coded) refreshed with values that are all
    different (the factor rule: nothing coded), and the reverse; apply and apply_multi against an operator created on the values"""
    import torch
    for var in ("DDM_SPMV_STAGE_X", "DDM_SPMV_CODE", "DDM_SPMV_FORMAT"):
        monkeypatch.delenv(var, raising=False)
    cases = code_cases()
    ctx = ddm.torch_context(0)
    for name in sorted(cases):
        M, x_host, _ = cases[name]
        M = sp.csr_matrix(M)
        n = M.shape[0]
        R = rc.with_data(M, M.data * np.random.default_rng(9).uniform(0.7, 1.3, M.nnz))
        coded_M, coded_R = (int(ddm.dia_codes_host(Q, arrays=False)["coded"].sum()) for Q in (M, R))
        x = torch.as_tensor(vector(n, 21) if x_host is None else x_host).cuda()
        X = torch.as_tensor(np.random.default_rng(23).standard_normal((n, 4))).cuda().contiguous()
        owner = np.ones(n, dtype=np.uint8)
        for first, second in ((M, R), (R, M)):
            A = ddm.CsrMatrix(ctx, first)
            op = ddm.NonOverlappingOperator(ctx, A, None, owner)
            y, Y = torch.full_like(x, float("nan")), torch.full_like(X, float("nan"))
            op.apply(x, y)
            op.apply_multi(X, Y)
            ctx.sync()
            y_first = y.clone()
            A.set_values(second.data)
            op.refresh()
            y.fill_(float("nan")), Y.fill_(float("nan"))
            op.apply(x, y)
            op.apply_multi(X, Y)
            A2 = ddm.CsrMatrix(ctx, second)
            op2 = ddm.NonOverlappingOperator(ctx, A2, None, owner)
            y2, Y2 = torch.full_like(x, float("nan")), torch.full_like(X, float("nan"))
            op2.apply(x, y2)
            op2.apply_multi(X, Y2)
            ctx.sync()
            assert not torch.equal(_bits(y), _bits(y_first)), name
            assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(Y), _bits(Y2)), (name, first is M)
            del op, op2, A, A2
        print(f"\n{name}: {coded_M} coded blocks with its own values, {coded_R} with the refreshed ones")
        assert coded_R == 0 or name == "random_values" or coded_R < coded_M, name
    ctx.close()


# ---- two levels --------------------------------------------------------------------------------------------------------------------
def _sorted_data(M):
    M = sp.csr_matrix(M)
    if not M.has_sorted_indices:
        M = M.sorted_indices()
    return M


@pytest.fixture(scope="module")
def golden_pair(ddm):
    """the 12^3 golden problem and the same decomposition with a changed coefficient (tests/refresh_cases.py)"""
    from dune_ddm_amd.problem import RankLocal
    dec = golden_poisson(ddm)
    dec2 = rc.perturbed_decomposition(dec, 29)
    rl, rl2 = RankLocal(dec), RankLocal(dec2)
    A2, Ad2 = _sorted_data(rl2.A), _sorted_data(rl2.A_dir)
    assert rc.same_pattern(_sorted_data(rl.A), A2) and rc.same_pattern(_sorted_data(rl.A_dir), Ad2)
    rc.assert_dominant(Ad2)
    for sd in dec2.subs:
        rc.assert_dominant(sd.A_dir)
    assert abs(Ad2 - Ad2.T).max() > 1e-3
    return dec, dec2, A2.data.copy(), Ad2.data.copy()


def _two_level(ddm, golden_pair, mode, solve, subdomain_solver="ilu0", expect_engine=None):
    from dune_ddm_amd.solver import TwoLevelSchwarz
    dec, dec2, va, vd = golden_pair
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="standard" if mode == "additive" else "restricted", mode=mode, subdomain_solver=subdomain_solver)
    first = solve(tl)                                            # (a solve before the refresh, with the objects used afterwards)
    schwarz, galerkin, a0_first = tl.schwarz, tl.galerkin, tl.a0.copy()
    tl.update_values(va, vd)
    assert tl.galerkin is galerkin and (tl.schwarz is schwarz) == (subdomain_solver == "ilu0")
    if expect_engine:
        assert tl.schwarz.engine() == expect_engine
    got = solve(tl)
    fresh = TwoLevelSchwarz(dec2, coarse=tl.host_basis(), schwarz_type="standard" if mode == "additive" else "restricted", mode=mode,
                            subdomain_solver=subdomain_solver)
    want = solve(fresh)
    assert not np.array_equal(tl.a0, a0_first)
    assert np.array_equal(tl.a0, fresh.a0)
    assert any(k.startswith("refresh: ") for k in tl.setup_times)
    return first, got, want


def _single(solver, maxit=200):
    def solve(tl):
        res, hist, x = tl.solve(reduction=1e-8, maxit=maxit, solver=solver, restart=30)
        tl.prec.check_status()
        return [res.iterations], [bool(res.converged)], x.cpu().numpy().copy()
    return solve


def _check(first, got, want, tag):
    it1, _, x1 = first
    it, conv, x = got
    itw, convw, xw = want
    print(f"\n{tag}: {it1} iterations before the refresh, {it} after it, {itw} on fresh objects; x differs in {int(np.sum(x != xw))} of {x.size} entries")
    assert it == itw and conv == convw, tag
    assert np.isfinite(xw).all() and np.array_equal(x, xw), tag
    assert not np.array_equal(x, x1), tag


@pytest.mark.parametrize("mode, solver", [("additive", "cgsolver"), ("multiplicative", "restartedgmressolver")])
def test_update_values_equals_fresh_objects(ddm, golden_pair, mode, solver, monkeypatch):
    monkeypatch.delenv("DDM_TRSV_MODE", raising=False)
    _check(*_two_level(ddm, golden_pair, mode, _single(solver)), f"{mode} / {solver}")


def test_update_values_solve_multi(ddm, golden_pair, monkeypatch):
    monkeypatch.delenv("DDM_TRSV_MODE", raising=False)
    def solve(tl):
        B = np.outer(np.asarray(tl.rl.b, dtype=np.float64), [1.0, -2.0, 0.5, 3.0])   # (consistent right-hand sides, as the problem's own)
        res, hist, X = tl.solve_multi(B, reduction=1e-8, maxit=200)
        tl.prec.check_status()
        return [r.iterations for r in res], [bool(r.converged) for r in res], X.cpu().numpy().copy()
    _check(*_two_level(ddm, golden_pair, "additive", solve), "additive / solve_multi (4 columns)")


def test_update_values_recreates_a_direct_level(ddm, golden_pair, monkeypatch):
    monkeypatch.delenv("DDM_TRSV_MODE", raising=False)
    _check(*_two_level(ddm, golden_pair, "additive", _single("restartedgmressolver"), subdomain_solver="cholmod"), "additive / cholmod (level built anew)")
