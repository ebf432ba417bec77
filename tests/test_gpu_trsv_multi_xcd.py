"""-m gpu: engine `xcd` of the block solve of a plain ILU(0) factor (k_trsv_multi_xcd: both sweeps of all diagonal blocks in one
persistent launch, csrc/engine_multi_xcd.hpp) against engine `levels` (one launch per level, the default) on the SAME factor object
and the same D.  The kernel sums every row over the same entries in the same order as the level kernels, so every comparison is
torch.equal -- no tolerance, no oracle.  The cases, what each reaches and the proof that it does are in tests/trsv_multi_cases.py,
tests/trsv_cases.py and tests/test_trsv_multi_plan.py (CPU).  The time-out paths are not run here (nothing is made non-resident or hung
on purpose); their status plumbing is that of ddm_ilu0_set_status."""
import numpy as np
import pytest

from tests import trsv_cases as tc
from tests import trsv_multi_cases as mc

pytestmark = pytest.mark.gpu

CASES = ("band17", "blocks3", "elasticity", "dg", "blocks9", "blocks17", "chain600", "loop8")
FILL = 7.0


@pytest.fixture(scope="module")
def blocks():
    """per case, computed once and never changed: the case and one (n, 32) block of right-hand sides"""
    made = {}

    def get(name):
        if name not in made:
            c = mc.case(name)
            D = np.random.default_rng(17).standard_normal((c.n, max(mc.WIDTHS)))
            D.setflags(write=False)
            made[name] = (c, D)
        return made[name]
    return get


def _factor(ddm, ctx, c):
    return ddm.Ilu0(ctx, ddm.CsrMatrix(ctx, c.M), c.block_ptr)


def _solve(F, engine, D, X=None, f32=False, ld=False):
    import torch
    F.set_multi_engine(engine)
    if X is None:
        X = torch.full_like(D, float("nan"))
    (F.solve_multi_ld if ld else F.solve_multi)(D, X, single_precision=f32)
    info = F.multi_info()                                        # (synchronises)
    assert F.status() == 0, (engine, info)
    return X, info


def _expect_xcd(ddm, c, info, one_team=False):
    """info of an xcd launch: the engine ran, the grid is the sum of the tickets, the teams are those of the team function"""
    assert info["engine"] == "xcd" and info["declined"] is None, info
    assert info["grid"] == sum(info["tickets"]) and info["grid"] >= 8, info
    want = ddm.trsv_multi_team_host(info["tickets"], len(c.block_ptr) - 1, 0, 0, 0, one_team)
    assert (info["teams"], info["one_team"]) == (want["teams"], want["one_team"]), (info, want)
    if one_team:
        assert info["teams"] == 1 and info["one_team"]
    elif all(t > 0 for t in info["tickets"]):                    # (every XCD hosts workgroups: always so at one workgroup per CU)
        assert info["teams"] == mc.teams(c) and not info["one_team"], info


@pytest.mark.parametrize("name", CASES)
def test_xcd_equals_levels(ddm, blocks, name):
    """widths 1, 3 and 7 (the scalar form), 4, 24 and 32 (the quad form) on the first m columns of one block; band17: one team of 8
    XCDs; blocks3: teams of 3, 3 and 2 XCDs; blocks9 / blocks17: an XCD with two / three blocks of different level counts; chain600:
    600 consecutive one-row levels per sweep; loop8: a second item per thread at m = 32"""
    import torch
    c, Dh = blocks(name)
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, c)
    Dd = torch.tensor(Dh).cuda()
    assert F.multi_info()["engine"] is None and F.multi_info()["requested"] == "levels"
    for m in mc.WIDTHS:
        D = Dd[:, :m].contiguous()
        X0, info0 = _solve(F, "levels", D)
        assert info0["engine"] == "levels" and info0["declined"] == "not requested", info0
        X1, info1 = _solve(F, "xcd", D)
        _expect_xcd(ddm, c, info1)
        assert bool(torch.isfinite(X0).all()) and torch.equal(X0, X1), (name, m, int((X0 != X1).sum()))
    ctx.close()


@pytest.mark.parametrize("name", ["band17", "blocks9"])
def test_column_slices_of_a_wider_block(ddm, blocks, name):
    """solve_multi_ld on m = 8 columns of (n, 24) blocks: the slot at column 8 (aligned: the quad form with ld = 3 m) and the slot at
    column 3 (its offset is no multiple of 4: the scalar form); nothing outside the slot is written"""
    import torch
    c, Dh = blocks(name)
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, c)
    m = 8
    Dw = torch.tensor(Dh[:, :3 * m]).cuda().contiguous()
    for c0 in (8, 3):
        out = []
        for engine in ("levels", "xcd"):
            Xw = torch.full_like(Dw, FILL)
            _, info = _solve(F, engine, Dw[:, c0:c0 + m], Xw[:, c0:c0 + m], ld=True)
            assert info["engine"] == engine
            out.append(Xw)
        assert Dw[:, c0:].data_ptr() % 32 == (0 if c0 == 8 else 24)
        assert torch.equal(out[0], out[1]) and bool(torch.isfinite(out[1]).all()), (name, c0)
        assert bool((out[1][:, :c0] == FILL).all()) and bool((out[1][:, c0 + m:] == FILL).all()) and not bool((out[1][:, c0:c0 + m] == FILL).all())
    ctx.close()


@pytest.mark.parametrize("name", ["band17", "blocks9"])
def test_single_precision_sweeps(ddm, blocks, name):
    """f32 at m = 4 and 24: the bits of the f32 level sweeps (k_trsv_level_multi4_f32), and not the double result; at m = 6 the
    request is answered in double by either engine"""
    import torch
    c, Dh = blocks(name)
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, c)
    for m in (4, 24):
        D = torch.tensor(Dh[:, :m]).cuda().contiguous()
        X0, _ = _solve(F, "levels", D, f32=True)
        X1, info = _solve(F, "xcd", D, f32=True)
        _expect_xcd(ddm, c, info)
        X64, _ = _solve(F, "xcd", D)
        assert bool(torch.isfinite(X0).all()) and torch.equal(X0, X1) and not torch.equal(X1, X64), (name, m)
    D = torch.tensor(Dh[:, :6]).cuda().contiguous()
    X64, _ = _solve(F, "levels", D)
    X1, info = _solve(F, "xcd", D, f32=True)
    _expect_xcd(ddm, c, info)
    assert bool(torch.isfinite(X64).all()) and torch.equal(X64, X1)
    ctx.close()


@pytest.mark.parametrize("name", ["wide", "layers", "direct"])
def test_declined_factors_run_what_they_ran(ddm, name):
    """a level of w >= 96 (k_trsv_level_multi_wide sums in another order) and a direct factor: the request is declined, multi_info
    says why, the results are those of the default"""
    import torch
    from dune_ddm_amd import synth
    ctx = ddm.torch_context(0)
    if name == "direct":
        M = synth.StructuredPoisson((9, 8, 7), (1, 1, 1)).subdomain(0).A.tocsr()
        M.sort_indices()
        F = ddm.Ilu0(ctx, ddm.CsrMatrix(ctx, M), None, direct=True)
        n, why, requested = M.shape[0], "direct factor", "levels"
    else:
        c = mc.case(name)
        F = _factor(ddm, ctx, c)
        n, why, requested = c.n, "wide level", "xcd"
    D = torch.tensor(np.random.default_rng(3).standard_normal((n, 8))).cuda()
    X0, info0 = _solve(F, "levels", D)
    X1, info1 = _solve(F, "xcd", D)
    assert info1["requested"] == requested and info1["engine"] == "levels" and info1["declined"] == why, info1
    assert bool(torch.isfinite(X0).all()) and torch.equal(X0, X1)
    ctx.close()


@pytest.mark.parametrize("name", ["blocks9", "band17"])
def test_one_team_forced(ddm, blocks, name):
    """mode 2: the path taken when a team has no workgroup -- all workgroups in one team that solves every block"""
    import torch
    c, Dh = blocks(name)
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, c)
    for m in (7, 8):
        D = torch.tensor(Dh[:, :m]).cuda().contiguous()
        X0, _ = _solve(F, "levels", D)
        X1, info = _solve(F, "xcd1", D)
        _expect_xcd(ddm, c, info, one_team=True)
        assert bool(torch.isfinite(X0).all()) and torch.equal(X0, X1), (name, m)
    ctx.close()


def test_graph_replay_other_buffers_and_engine_switches(ddm, blocks):
    """the captured launch: a replay into the same buffers, a second output block, a second D into the same X, and the engine switched
    between calls on the same buffers (the graph of the other engine must not answer)"""
    import torch
    c, Dh = blocks("blocks9")
    ctx = ddm.torch_context(0)
    F = _factor(ddm, ctx, c)
    D = torch.tensor(Dh[:, :8]).cuda().contiguous()
    D2 = torch.tensor(Dh[:, 8:16]).cuda().contiguous()
    ref, _ = _solve(F, "levels", D)
    ref2, _ = _solve(F, "levels", D2)
    assert not torch.equal(ref, ref2)
    X, info = _solve(F, "xcd", D)
    _expect_xcd(ddm, c, info)
    assert torch.equal(X, ref)
    X.fill_(float("nan"))
    _solve(F, "xcd", D, X)                                       # replay
    assert torch.equal(X, ref)
    Xb, _ = _solve(F, "xcd", D)                                  # a second output block
    assert torch.equal(Xb, ref)
    _solve(F, "xcd", D2, X)                                      # a second D into the same X
    assert torch.equal(X, ref2)
    for engine in ("levels", "xcd", "xcd1", "levels", "xcd"):
        X.fill_(float("nan"))
        _, info = _solve(F, engine, D, X)
        assert info["engine"] == ("levels" if engine == "levels" else "xcd"), (engine, info)
        assert engine != "xcd1" or info["one_team"], info
        assert torch.equal(X, ref), engine
    ctx.close()


def test_after_a_value_refresh(ddm, blocks):
    """CsrMatrix.set_values + F.refresh(): the plan depends on the pattern only, so the kept plan serves the new values"""
    import torch
    c, Dh = blocks("blocks9")
    ctx = ddm.torch_context(0)
    A = ddm.CsrMatrix(ctx, c.M)
    F = ddm.Ilu0(ctx, A, c.block_ptr)
    D = torch.tensor(Dh[:, :8]).cuda().contiguous()
    old, _ = _solve(F, "xcd", D)
    rows = np.repeat(np.arange(c.n), np.diff(c.M.indptr))
    scale = np.where(c.M.indices == rows, 1.0, np.random.default_rng(99).uniform(0.5, 1.0, c.M.nnz))   # still strictly dominant
    A.set_values(c.M.data * scale)
    F.refresh()
    assert F.refresh_count() == 1
    X1, info = _solve(F, "xcd", D)
    _expect_xcd(ddm, c, info)
    X0, _ = _solve(F, "levels", D)
    assert bool(torch.isfinite(X0).all()) and torch.equal(X0, X1) and not torch.equal(X1, old)
    for m in (4,):                                               # ... and the float copies follow
        Dm = D[:, :m].contiguous()
        Y0, _ = _solve(F, "levels", Dm, f32=True)
        Y1, _ = _solve(F, "xcd", Dm, f32=True)
        assert torch.equal(Y0, Y1)
    ctx.close()


# ---- through the stack, on the 12^3 golden problem ---------------------------------------------------------------------------------
def _golden_tl(ddm, **kw):
    from dune_ddm_amd.solver import TwoLevelSchwarz
    from tests.test_fgmres_cpu import golden_poisson
    dec = golden_poisson(ddm)
    return dec, TwoLevelSchwarz(dec, coarse="pou", schwarz_type="standard", mode="additive", **kw)


def test_schwarz_apply_multi_and_block_solvers(ddm):
    """schwarz.apply_multi, solve_multi (CG, m = 8) and solve_block (block CG) under either engine: equal bits, equal iteration
    counts; TwoLevelSchwarz(multi_engine="xcd") sets the engine"""
    import torch
    from tests.test_gpu_multi_rhs import _consistent_block
    dec, tl = _golden_tl(ddm, multi_engine="xcd")
    B = _consistent_block(tl, dec, 8, seed=23)
    Bd = tl.to_device(B)
    out = {}
    for engine in ("xcd", "levels"):
        tl.schwarz.set_multi_engine(engine)
        X = torch.full_like(Bd, float("nan"))
        tl.schwarz.apply_multi(X, Bd)
        res, hist, Xs = tl.solve_multi(B, reduction=1e-10, maxit=200)
        resb, histb, Xb, ranks = tl.solve_block(B, reduction=1e-10, maxit=200)
        tl.prec.check_status()
        out[engine] = (X, [r.iterations for r in res], Xs, [r.iterations for r in resb], Xb, np.asarray(hist), np.asarray(histb))
    a, b = out["xcd"], out["levels"]
    assert bool(torch.isfinite(a[0]).all()) and torch.equal(a[0], b[0])
    assert a[1] == b[1] and min(a[1]) > 4 and torch.equal(a[2], b[2]) and np.array_equal(a[5], b[5])
    assert a[3] == b[3] and min(a[3]) > 2 and torch.equal(a[4], b[4]) and np.array_equal(a[6], b[6])
    tl.ctx.close()


def test_schwarz_reports_the_engine(ddm):
    """the local solver of a TwoLevelSchwarz(multi_engine="xcd") runs its block applies on xcd (8 subdomains: 8 teams)"""
    import ctypes
    import torch
    from tests.test_gpu_multi_rhs import _consistent_block
    dec, tl = _golden_tl(ddm, multi_engine="xcd")
    Bd = tl.to_device(_consistent_block(tl, dec, 4, seed=1))
    X = torch.full_like(Bd, float("nan"))
    tl.schwarz.apply_multi(X, Bd)
    tl.ctx.sync()
    out = np.zeros(14, dtype=np.int64)
    cnt = ctypes.c_int64()
    assert tl.ctx.lib.ddm_ilu0_multi_info(ctypes.c_void_p(tl.schwarz.local_solver()), out.ctypes.data_as(ctypes.c_void_p), 14, ctypes.byref(cnt)) == ddm.DDM_OK
    assert cnt.value == 14 and out[0] == 1 and out[1] == 1 and out[2] == 0 and out[3] == out[6:14].sum(), out
    assert out[4] == (8 if (out[6:14] > 0).all() else 1), out
    tl.prec.check_status()
    tl.ctx.close()


def test_geneo_basis_with_the_environment_variable(ddm, monkeypatch):
    """DDM_TRSV_MULTI_MODE=xcd when GenEO creates its ILU(0) preconditioner: the basis is bit for bit the default run's"""
    from dune_ddm_amd.geneo import geneo_basis
    from dune_ddm_amd.solver import TwoLevelSchwarz
    from tests.test_fgmres_cpu import golden_poisson
    dec = golden_poisson(ddm)
    out = {}
    for mode in (None, "xcd"):
        if mode is None:
            monkeypatch.delenv("DDM_TRSV_MULTI_MODE", raising=False)
        else:
            monkeypatch.setenv("DDM_TRSV_MULTI_MODE", mode)
        tl = TwoLevelSchwarz(dec, coarse="none")
        basis, info = geneo_basis(tl, nev=4, tol=1e-5, return_info=True, preconditioner="ilu0")
        assert info["converged"]
        out[mode] = (basis, info["iterations"])
        tl.ctx.close()
    monkeypatch.delenv("DDM_TRSV_MULTI_MODE", raising=False)
    assert out[None][1] == out["xcd"][1]
    for s in out[None][0]:
        assert np.array_equal(np.asarray(out[None][0][s]), np.asarray(out["xcd"][0][s])), s


def test_environment_variable_sets_the_initial_mode(ddm, blocks, monkeypatch):
    import torch
    c, Dh = blocks("blocks3")
    ctx = ddm.torch_context(0)
    monkeypatch.setenv("DDM_TRSV_MULTI_MODE", "xcd")
    F = _factor(ddm, ctx, c)
    monkeypatch.setenv("DDM_TRSV_MULTI_MODE", "levels")
    G = _factor(ddm, ctx, c)
    monkeypatch.delenv("DDM_TRSV_MULTI_MODE", raising=False)
    assert F.multi_info()["requested"] == "xcd" and G.multi_info()["requested"] == "levels"
    D = torch.tensor(Dh[:, :4]).cuda().contiguous()
    X1, X0 = torch.full_like(D, float("nan")), torch.full_like(D, float("nan"))
    F.solve_multi(D, X1)
    G.solve_multi(D, X0)
    assert F.multi_info()["engine"] == "xcd" and G.multi_info()["engine"] == "levels"
    assert F.status() == 0 and bool(torch.isfinite(X0).all()) and torch.equal(X0, X1)
    ctx.close()


def test_multi_engine_adaptor(ddm, tmp_path):
    """tests/cpp/multi_engine_adaptor.cc: [schwarz] multi_engine = levels | xcd under Dune::HipCGSolver's block apply, bit for bit; an
    unknown value throws"""
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    from tests.cpp_harness import build, dump_one_rank_problem, run
    exe = build("./build/multi_engine_adaptor")
    dec = build_structured(synth.StructuredPoisson((12, 12, 12), (1, 1, 1)), overlap=1, pou_type="distance")
    dump_one_rank_problem(tmp_path, dec.subs[0])
    p = run(exe, tmp_path, 3)
    out = p.stdout
    assert "engines 0 1 0" in out and "errors_caught 1" in out and "multi_engine_ok" in out, out[-2000:] + p.stderr[-2000:]
    cols = [ln.split() for ln in out.splitlines() if ln.startswith("col ")]
    assert len(cols) == 3 and all(cl[2] == cl[3] and cl[4:] == ["0", "0"] for cl in cols), cols
