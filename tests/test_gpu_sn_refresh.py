"""-m gpu: the value refresh of the DEVICE supernodal direct factor (csrc/sn_refresh.hpp behind ddm_ilu0_refresh;
DDM_DIRECT_ENGINE=device) through every layer, against objects created on the new values.  One criterion throughout, as for the
ILU(0) refresh (tests/test_gpu_refresh.py): bit equality (`==`), no tolerance -- the factorisation is bitwise reproducible
(tests/test_gpu_sn_routes.py, (d)), so a factor refreshed to M2 and a factor created on M2 are the same numbers.

The matrices are those of tests/sn_cases.py, the new values those of tests/sn_refresh_cases.py (preconditions proved on the CPU by
tests/test_sn_refresh_cases_cpu.py).  Every test solves at least once BEFORE the refresh with the device buffers it uses afterwards,
so a stale captured graph, a stale residual matrix or a stale buffer shows; every output is filled with NaN first; F.status() == 0
after every solve; every factor is asserted to be the device supernodal one.

 1  every case x every route of the case, refinement off: solve, replay, set_values(M2), refresh, solve, replay = the fresh factor's
    bits, different from before; refresh_count() == 1; back to M: the bits of the first solve.
 2  block solves at the widths 1, 17, 49, 97 (one column, a 16-column tile edge, two and three 48-column panels) and the single
    vector after them; and the order "block first, then single vector" (sn::reserve's scratch growth resets the single-vector graph).
 3  refinement decided again (DDM_DIRECT_REFINE unset): benign values -> the pivoting matrix -> benign values; steps and probe
    backward errors equal the fresh factor's, the step count changes, the solves are the fresh factor's bits.
 4  a failed refresh (not positive definite): DDM_ENUMERIC, the factor invalid for solve and solve_multi, refresh_count() unchanged,
    then a good refresh gives the fresh bits.  An error return of the numeric check; no device fault is involved.
 5  values an unforced creation hands to the host engine: DDM_ENOTIMPL with "create a new factor".
 6  TwoLevelSchwarz.update_values with a direct local solver keeps the level and takes the in-place path; after a failed refresh
    the Schwarz applies return DDM_ENUMERIC until update_values succeeds.
 7  refresh_count() on an ILU(0) factor and on a refused host-engine direct factor."""
import numpy as np
import pytest

from tests import refresh_cases as rc
from tests import sn_cases as sc
from tests import sn_refresh_cases as src
from tests import trsv_cases as tc
from tests.test_fgmres_cpu import golden_poisson

pytestmark = pytest.mark.gpu

BLOCK_CASES = ("one21", "chain1d", "lu13")
BLOCK_WIDTHS = (1, 17, 49, 97)


class Factor:
    """a matrix on the device and its direct factor, asserted to be the device supernodal one"""

    def __init__(self, ddm, ctx, M, block_ptr, general):
        self.ctx = ctx
        self.A = ddm.CsrMatrix(ctx, M)
        self.F = ddm.Ilu0(ctx, self.A, block_ptr, direct=True, general=general)
        assert ctx.lib.ddm_ilu0_is_direct(self.F.h) == 1 and self.F.engine() == "supernodal"
        assert self.F.refresh_count() == 0

    def solve(self, dd, xd):
        """one vector (F.solve) or a block (F.solve_multi) into the NaN-filled xd"""
        xd.fill_(float("nan"))
        if dd.dim() == 1:
            self.F.solve(dd, xd)
        else:
            self.F.solve_multi(dd, xd)
        self.ctx.sync()
        assert self.F.status() == 0
        x = xd.cpu().numpy().copy()
        assert np.isfinite(x).all()
        return x

    def refresh_to(self, M):
        self.A.set_values(src._sorted(M).data)
        self.F.refresh()
        assert self.F.engine() == "supernodal"


def _device(c):
    import torch
    d = torch.tensor(c.d).cuda()
    return d, torch.empty(c.n, dtype=torch.float64, device="cuda")


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NAMES)
def test_refreshed_factor_equals_a_fresh_one_on_every_route(ddm, name, monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device (no CPU fallback exists)"
    c = sc.case(name)
    M2 = src.new_matrix(name)
    assert rc.same_pattern(src._sorted(c.M), M2)
    ctx = ddm.torch_context(0)
    dd, xd = _device(c)
    xf = torch.empty_like(xd)
    for route in c.routes:
        c.env(monkeypatch, route)                                # (refinement off)
        S = Factor(ddm, ctx, c.M, c.block_ptr, c.general)
        assert S.F.refinement()[0] == 0
        first = S.solve(dd, xd)
        assert np.array_equal(S.solve(dd, xd), first), (name, route, "replay before the refresh")
        S.refresh_to(M2)
        assert S.F.refresh_count() == 1 and S.F.refinement()[0] == 0
        after = S.solve(dd, xd)
        replay = S.solve(dd, xd)
        fresh = Factor(ddm, ctx, M2, c.block_ptr, c.general)
        want = fresh.solve(dd, xf)
        print(f"\n[sn refresh] {name} {route}: the refreshed solve differs from the fresh factor's in {int(np.sum(after != want))} of {c.n} entries, "
              f"from the solve before the refresh in {int(np.sum(after != first))}")
        assert not np.array_equal(want, first), (name, route, "the new values do not change the solution")
        assert np.array_equal(after, want), (name, route, int(np.sum(after != want)))
        assert np.array_equal(replay, want), (name, route, "replay after the refresh")
        S.refresh_to(c.M)                                        # and back
        assert S.F.refresh_count() == 2
        assert np.array_equal(S.solve(dd, xd), first), (name, route, "refreshed back to the first values")
        del S, fresh
    ctx.close()


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,width", [(n, w) for n in BLOCK_CASES for w in BLOCK_WIDTHS])
def test_block_solves_after_a_refresh(ddm, name, width, monkeypatch):
    import torch
    c = sc.case(name)
    c.env(monkeypatch, "default")
    M2 = src.new_matrix(name)
    ctx = ddm.torch_context(0)
    Dd = torch.tensor(np.ascontiguousarray(c.D[:, :width])).cuda()
    Xd, Xf = torch.empty_like(Dd), torch.empty_like(Dd)
    dd, xd = _device(c)
    xf = torch.empty_like(xd)
    S = Factor(ddm, ctx, c.M, c.block_ptr, c.general)
    first = S.solve(Dd, Xd)
    assert np.array_equal(S.solve(Dd, Xd), first)
    S.refresh_to(M2)
    X, x = S.solve(Dd, Xd), S.solve(dd, xd)
    fresh = Factor(ddm, ctx, M2, c.block_ptr, c.general)
    Xw, xw = fresh.solve(Dd, Xf), fresh.solve(dd, xf)
    assert not np.array_equal(Xw, first)
    assert np.array_equal(X, Xw), (name, width, int(np.sum(X != Xw)))
    assert np.array_equal(x, xw), (name, width, "single vector after the block solve")
    assert np.array_equal(S.solve(Dd, Xd), Xw), (name, width, "replay after the refresh")
    assert S.F.refresh_count() == 1
    del S, fresh
    ctx.close()


def test_block_first_then_single_vector(ddm, monkeypatch):
    """single vector (graph captured), then a block of 97 columns (sn::reserve grows the scratch: the single-vector graph is reset),
    refresh, block, single vector -- and the other order on a second factor"""
    import torch
    c = sc.case("one21")
    c.env(monkeypatch, "default")
    M2 = src.new_matrix("one21")
    ctx = ddm.torch_context(0)
    Dd = torch.tensor(np.ascontiguousarray(c.D[:, :97])).cuda()
    Xd, Xf = torch.empty_like(Dd), torch.empty_like(Dd)
    dd, xd = _device(c)
    xf = torch.empty_like(xd)
    fresh = Factor(ddm, ctx, M2, c.block_ptr, c.general)
    xw, Xw = fresh.solve(dd, xf), fresh.solve(Dd, Xf)
    for order in ("single, block", "block, single"):
        S = Factor(ddm, ctx, c.M, c.block_ptr, c.general)
        if order == "single, block":
            S.solve(dd, xd), S.solve(Dd, Xd)
        else:
            S.solve(Dd, Xd), S.solve(dd, xd)
        S.refresh_to(M2)
        X = S.solve(Dd, Xd)
        x = S.solve(dd, xd)
        assert np.array_equal(X, Xw) and np.array_equal(x, xw), order
        assert np.array_equal(S.solve(dd, xd), xw) and np.array_equal(S.solve(Dd, Xd), Xw), order
        del S
    del fresh
    ctx.close()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
def _backward_error(M, X, B):
    return float(np.linalg.norm(M @ X - B) / (float(abs(M).sum(axis=1).max()) * np.linalg.norm(X) + np.linalg.norm(B)))


def test_refinement_is_decided_again(ddm, monkeypatch):
    import torch
    monkeypatch.setenv("DDM_DIRECT_ENGINE", "device")
    monkeypatch.delenv("DDM_DIRECT_REFINE", raising=False)
    sc.set_route(monkeypatch, "default")
    P, bp = src.pivoting()
    B = src.pivoting_benign()
    n = P.shape[0]
    rhs = np.random.default_rng(11).standard_normal((n, 17))
    ctx = ddm.torch_context(0)
    dd, Dd = torch.tensor(np.ascontiguousarray(rhs[:, 0])).cuda(), torch.tensor(rhs).cuda()
    xd, Xd, xf, Xf = torch.empty_like(dd), torch.empty_like(Dd), torch.empty_like(dd), torch.empty_like(Dd)
    fresh = {}
    for key, M in (("benign", B), ("pivoting", P)):
        F = Factor(ddm, ctx, M, bp, True)
        fresh[key] = (F.F.refinement(), F.solve(dd, xf), F.solve(Dd, Xf))
        del F
    (steps_b, om_b), (steps_p, om_p) = fresh["benign"][0], fresh["pivoting"][0]
    print(f"\n[sn refresh] refinement steps: benign {steps_b} (probe {om_b[:steps_b + 1]}), pivoting {steps_p} (probe {om_p[:steps_p + 1]})")
    assert steps_p >= 1 and om_p[steps_p] <= 1e-12                # (the pivoting matrix's own criterion, tests/test_gpu_sn_routes.py (e))
    assert steps_b != steps_p, "the step count has to change across the pair"
    S = Factor(ddm, ctx, B, bp, True)
    assert np.array_equal(S.solve(dd, xd), fresh["benign"][1]) and np.array_equal(S.solve(Dd, Xd), fresh["benign"][2])
    for count, (key, M) in enumerate((("pivoting", P), ("benign", B), ("pivoting", P)), start=1):
        S.refresh_to(M)
        (steps, om), xw, Xw = fresh[key]
        got_steps, got_om = S.F.refinement()
        assert got_steps == steps and np.array_equal(got_om, om), (key, got_steps, got_om, steps, om)
        x, X = S.solve(dd, xd), S.solve(Dd, Xd)
        assert np.array_equal(x, xw), (key, "single vector", int(np.sum(x != xw)))
        assert np.array_equal(X, Xw), (key, "17 columns", int(np.sum(X != Xw)))
        assert np.array_equal(S.solve(dd, xd), xw) and np.array_equal(S.solve(Dd, Xd), Xw), (key, "replay")
        assert S.F.refresh_count() == count
        if key == "pivoting":
            omega = max(_backward_error(P, x, rhs[:, 0]), _backward_error(P, X, rhs))
            print(f"[sn refresh] refreshed to the pivoting matrix: backward error of the solves {omega:.2e}")
            assert omega <= 1e-12
    del S
    ctx.close()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("one21", "chain1d"))
def test_failed_refresh_leaves_an_invalid_factor(ddm, name, monkeypatch):
    import torch
    c = sc.case(name)
    c.env(monkeypatch, "default")
    M2 = src.new_matrix(name)
    N, _ = src.not_positive_definite(M2)
    ctx = ddm.torch_context(0)
    with pytest.raises(ddm.DdmError) as e:                      # what a creation on these values does, with the engine forced
        Factor(ddm, ctx, N, c.block_ptr, False)
    assert e.value.code == ddm.DDM_ENUMERIC and "not positive definite" in str(e.value), str(e.value)
    Dd = torch.tensor(np.ascontiguousarray(c.D[:, :17])).cuda()
    Xd, Xf = torch.empty_like(Dd), torch.empty_like(Dd)
    dd, xd = _device(c)
    xf = torch.empty_like(xd)
    S = Factor(ddm, ctx, c.M, c.block_ptr, False)
    S.solve(dd, xd), S.solve(Dd, Xd)
    S.A.set_values(N.data)
    with pytest.raises(ddm.DdmError) as e:
        S.F.refresh()
    assert e.value.code == ddm.DDM_ENUMERIC and "not positive definite" in str(e.value), str(e.value)
    assert S.F.refresh_count() == 0
    for call in (lambda: S.F.solve(dd, xd), lambda: S.F.solve_multi(Dd, Xd)):
        with pytest.raises(ddm.DdmError) as e:
            call()
        assert e.value.code == ddm.DDM_ENUMERIC and "invalid" in str(e.value), str(e.value)
    S.refresh_to(M2)                                             # a later refresh on good values is a fresh factor's again
    assert S.F.refresh_count() == 1
    fresh = Factor(ddm, ctx, M2, c.block_ptr, False)
    assert np.array_equal(S.solve(dd, xd), fresh.solve(dd, xf))
    assert np.array_equal(S.solve(Dd, Xd), fresh.solve(Dd, Xf))
    del S, fresh
    ctx.close()


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------
def test_values_of_the_host_engine_are_handed_over(ddm, monkeypatch):
    """src.pivoting_like(src.HANDOVER_SCALE): the pivoting construction with every third diagonal entry times HANDOVER_SCALE = 1e-11
    instead of 1e-6, with DDM_DIRECT_REFINE=0 (the probe runs, no refinement step is taken).  Measured on one MI355X, probe backward
    error after 0, 1, .. steps by scale:
        1e-6   9.4e-13, 2.6e-18              1e-13  2.8e-06, 1.4e-09, 1.9e-12, 1.4e-15
        1e-9   6.7e-10, 3.7e-17              1e-15  3.4e-04, .., 2.6e-07 (declined; the host engine refuses it too: pivots below
        1e-11  4.1e-08, 2.8e-12, 1.5e-16            1e-14 max |a_ij|, sparse_chol_host.hpp)
    With the refinement the probe decides, the device engine keeps every scale the host engine accepts (no window), so the case pins
    the step count to 0: at 1e-11 the probe stands at 4.14e-08 > 1e-9 (the engine's bound) and the unforced creation is answered by
    the host engine, whose pivots of 1e-11 are far above its own threshold."""
    import torch
    monkeypatch.delenv("DDM_DIRECT_ENGINE", raising=False)       # not forced
    monkeypatch.setenv("DDM_DIRECT_DEVICE_MIN_FLOPS", "0")
    monkeypatch.setenv("DDM_DIRECT_REFINE", "0")
    sc.set_route(monkeypatch, "default")
    P, bp = src.pivoting()
    B, H = src.pivoting_benign(), src.pivoting_like(src.HANDOVER_SCALE)
    ctx = ddm.torch_context(0)
    A = ddm.CsrMatrix(ctx, H)
    F = ddm.Ilu0(ctx, A, bp, direct=True, general=True)
    assert ctx.lib.ddm_ilu0_is_direct(F.h) == 1 and F.engine() == "levels", F.engine()   # the host engine's factor
    del F, A
    S = Factor(ddm, ctx, B, bp, True)                            # (unforced, and still the device engine: DDM_DIRECT_DEVICE_MIN_FLOPS=0)
    dd = torch.tensor(np.random.default_rng(3).standard_normal(P.shape[0])).cuda()
    xd = torch.empty_like(dd)
    S.solve(dd, xd)
    S.A.set_values(H.data)
    with pytest.raises(ddm.DdmError) as e:
        S.F.refresh()
    print(f"\n[sn refresh] hand-over: {e.value}")
    assert e.value.code == ddm.DDM_ENOTIMPL and "create a new factor" in str(e.value), str(e.value)
    assert S.F.refresh_count() == 0
    with pytest.raises(ddm.DdmError) as e:                      # the panels were overwritten: no factor until a refresh succeeds
        S.F.solve(dd, xd)
    assert e.value.code == ddm.DDM_ENUMERIC and "invalid" in str(e.value), str(e.value)
    S.refresh_to(B)
    fresh = Factor(ddm, ctx, B, bp, True)
    assert np.array_equal(S.solve(dd, xd), fresh.solve(dd, torch.empty_like(dd)))
    del S, fresh
    ctx.close()


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_pair(ddm):
    """the 12^3 golden problem and the same decomposition with a changed coefficient (tests/refresh_cases.py)"""
    from dune_ddm_amd.problem import RankLocal
    dec = golden_poisson(ddm)
    dec2 = rc.perturbed_decomposition(dec, 29)
    rl, rl2 = RankLocal(dec), RankLocal(dec2)
    A2, Ad2 = src._sorted(rl2.A), src._sorted(rl2.A_dir)
    assert rc.same_pattern(src._sorted(rl.A), A2) and rc.same_pattern(src._sorted(rl.A_dir), Ad2)
    return dec, dec2, A2.data.copy(), Ad2.data.copy()


@pytest.mark.parametrize("mode", ("additive", "multiplicative"))
def test_update_values_keeps_a_device_direct_level(ddm, golden_pair, mode, monkeypatch):
    from dune_ddm_amd.solver import TwoLevelSchwarz
    monkeypatch.delenv("DDM_TRSV_MODE", raising=False)
    monkeypatch.setenv("DDM_DIRECT_ENGINE", "device")
    monkeypatch.delenv("DDM_DIRECT_REFINE", raising=False)
    sc.set_route(monkeypatch, "default")
    dec, dec2, va, vd = golden_pair
    kind = "standard" if mode == "additive" else "restricted"

    def solve(tl):
        res, hist, x = tl.solve(reduction=1e-8, maxit=200, solver="restartedgmressolver", restart=30)
        tl.prec.check_status()
        return res.iterations, bool(res.converged), x.cpu().numpy().copy()
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type=kind, mode=mode, subdomain_solver="umfpack")
    assert tl.schwarz.engine() == "supernodal" and tl.schwarz.refresh_count() == 0
    first = solve(tl)                                            # (a solve before the refresh, with the objects used afterwards)
    schwarz, galerkin, prec = tl.schwarz, tl.galerkin, tl.prec
    tl.update_values(va, vd)
    assert tl.schwarz is schwarz and tl.galerkin is galerkin and tl.prec is prec
    assert tl.schwarz.engine() == "supernodal" and tl.schwarz.refresh_count() == 1
    keys = [k for k in tl.setup_times if k.startswith("refresh: local solver")]
    assert keys == ["refresh: local solver (device factorisation, scatter)"], keys
    got = solve(tl)
    fresh = TwoLevelSchwarz(dec2, coarse=tl.host_basis(), schwarz_type=kind, mode=mode, subdomain_solver="umfpack")
    assert fresh.schwarz.engine() == "supernodal"
    want = solve(fresh)
    print(f"\n[sn refresh] two levels, {mode}: {first[0]} iterations before the refresh, {got[0]} after it, {want[0]} on fresh objects; "
          f"x differs in {int(np.sum(got[2] != want[2]))} of {got[2].size} entries")
    assert np.array_equal(tl.a0, fresh.a0)
    assert got[:2] == want[:2] and want[1]
    assert np.isfinite(want[2]).all() and np.array_equal(got[2], want[2])
    assert not np.array_equal(got[2], first[2])


def test_schwarz_applies_refuse_an_invalid_factor(ddm, golden_pair, monkeypatch):
    """the invalid state one layer up: update_values with a not-positive-definite A_dir raises the refresh's DDM_ENUMERIC, the
    Schwarz applies (single vector and block) then return DDM_ENUMERIC "invalid", and update_values with the first values brings
    back the bits of the first solve"""
    import torch
    from dune_ddm_amd.solver import TwoLevelSchwarz
    monkeypatch.delenv("DDM_TRSV_MODE", raising=False)
    monkeypatch.setenv("DDM_DIRECT_ENGINE", "device")
    monkeypatch.delenv("DDM_DIRECT_REFINE", raising=False)
    sc.set_route(monkeypatch, "default")
    dec = golden_pair[0]
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="standard", mode="additive", subdomain_solver="cholmod")
    assert tl.schwarz.engine() == "supernodal"

    def solve():
        res, _, x = tl.solve(reduction=1e-8, maxit=200, solver="cgsolver")
        tl.prec.check_status()
        return res.iterations, x.cpu().numpy().copy()
    first = solve()
    A, Ad = src._sorted(tl.rl.A), src._sorted(tl.rl.A_dir)
    va, vd = A.data.copy(), Ad.data.copy()
    bad, _ = src.not_positive_definite(Ad)
    d = tl.to_device(tl.rl.b)
    x = torch.full_like(d, float("nan"))
    D = d.reshape(-1, 1).repeat(1, 3).contiguous()
    X = torch.full_like(D, float("nan"))
    tl.schwarz.apply(x, d), tl.schwarz.apply_multi(X, D)         # (before the refresh, with the buffers used afterwards)
    tl.ctx.sync()
    with pytest.raises(ddm.DdmError) as e:
        tl.update_values(va, bad.data)
    assert e.value.code == ddm.DDM_ENUMERIC and "not positive definite" in str(e.value), str(e.value)
    assert tl.schwarz.refresh_count() == 0
    for call in (lambda: tl.schwarz.apply(x, d), lambda: tl.schwarz.apply_multi(X, D)):
        with pytest.raises(ddm.DdmError) as e:
            call()
        assert e.value.code == ddm.DDM_ENUMERIC and "invalid" in str(e.value), str(e.value)
    tl.update_values(va, vd)
    assert tl.schwarz.refresh_count() == 1 and tl.schwarz.engine() == "supernodal"
    again = solve()
    assert again[0] == first[0] and np.isfinite(first[1]).all() and np.array_equal(again[1], first[1])


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------
def test_refresh_count_of_other_factor_kinds(ddm, monkeypatch):
    import scipy.sparse as sp
    monkeypatch.delenv("DDM_TRSV_MODE", raising=False)
    monkeypatch.setenv("DDM_DIRECT_ENGINE", "host")
    c = tc.case("blocks3")
    ctx = ddm.torch_context(0)
    M = src._sorted(c.M)
    A = ddm.CsrMatrix(ctx, M)
    F = ddm.Ilu0(ctx, A, c.block_ptr)
    assert F.refresh_count() == 0
    M2 = rc.new_values(M, 11)
    rc.assert_dominant(M2)
    for k in (1, 2):
        A.set_values((M2 if k == 1 else M).data)
        F.refresh()
        assert F.refresh_count() == k
    Ms = src._sorted(sp.csr_matrix(c.M + c.M.T))                 # (symmetric positive definite: dominant, positive diagonal)
    As = ddm.CsrMatrix(ctx, Ms)
    G = ddm.Ilu0(ctx, As, c.block_ptr, direct=True)
    assert ctx.lib.ddm_ilu0_is_direct(G.h) == 1 and G.engine() == "levels"
    As.set_values(1.5 * Ms.data)
    with pytest.raises(ddm.DdmError) as e:
        G.refresh()
    assert e.value.code == ddm.DDM_ENOTIMPL and "create a new factor" in str(e.value)
    assert G.refresh_count() == 0
    assert ctx.lib.ddm_ilu0_refresh_count(None) == 0
    del F, G, A, As
    ctx.close()
