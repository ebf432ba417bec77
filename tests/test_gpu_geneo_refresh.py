"""-m gpu: the GenEO eigensolver kept between calls (GeneoSolver / ddm_geneo): cold identity with geneo_basis, value refresh of pencil
and preconditioner on the device, warm restart from the kept block, the start-block kernel on its own, and
TwoLevelSchwarz.update_values(..., coarse="refresh") end to end.  Inputs and their margins: tests/geneo_refresh_cases.py, proved on the
CPU by tests/test_geneo_refresh_cases_cpu.py.  The criteria against the oracle (eigenvalues rtol 1e-6: eigenvalue error ~ residual^2;
sine of the largest angle < 2e-3: eigenvector error ~ tolerance / gap; CG count +-1) are those of tests/test_gpu_geneo.py."""
import numpy as np
import pytest

from tests import geneo_refresh_cases as gc

pytestmark = pytest.mark.gpu

PRECONDITIONERS = [("ilu0", None), ("cholesky", "device"), ("cholesky", "host")]


def _orth(V):
    q, _ = np.linalg.qr(np.asarray(V).T)
    return q


def _sin_largest_angle(U, V):
    Qu, Qv = _orth(U), _orth(V)
    return float(np.linalg.norm(Qu - Qv @ (Qv.T @ Qu), 2))


def _engine(monkeypatch, engine):
    if engine is None:
        monkeypatch.delenv("DDM_DIRECT_ENGINE", raising=False)
    else:
        monkeypatch.setenv("DDM_DIRECT_ENGINE", engine)


def _tl(which):
    from dune_ddm_amd.solver import TwoLevelSchwarz
    return TwoLevelSchwarz(gc.decomposition(which), coarse="none")


def _assert_same(got, want):
    (b0, i0), (b1, i1) = got, want
    assert i0["iterations"] == i1["iterations"] and i0["converged"] and i1["converged"], (i0["iterations"], i1["iterations"])
    assert i0["nev"] == i1["nev"] and i0["nconv"] == i1["nconv"] and i0["used_direct"] == i1["used_direct"]
    assert sorted(b0) == sorted(b1)
    for s in b0:
        assert np.array_equal(i0["eigenvalues"][s], i1["eigenvalues"][s]), s
        assert np.array_equal(b0[s], b1[s]), s


def _against_oracle(basis, info, which, threshold=False):
    want = gc.oracle(which, threshold)
    for sd in gc.decomposition(which).subs:
        ov, lam = want[sd.id]
        k = len(ov)
        assert info["nconv"][sd.id] == k == basis[sd.id].shape[0], (sd.id, info["nconv"][sd.id], k)
        assert np.allclose(info["eigenvalues"][sd.id][:k], lam[:k], rtol=1e-6), (sd.id, info["eigenvalues"][sd.id], lam)
        assert _sin_largest_angle(basis[sd.id], ov) < 2e-3, sd.id


# ---- 1. cold identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,engine", PRECONDITIONERS)
def test_cold_compute_is_geneo_basis(ddm, monkeypatch, prec, engine):
    from dune_ddm_amd.geneo import GeneoSolver, geneo_basis
    _engine(monkeypatch, engine)
    tl = _tl("old")
    want = geneo_basis(tl, nev=gc.NEV, tol=gc.TOL, preconditioner=prec, return_info=True)
    S = GeneoSolver(tl, nev=gc.NEV, tol=gc.TOL, preconditioner=prec)
    assert S.state() == {"kept_width": 0, "pencil_refreshes": 0, "preconditioner_in_place": 0, "preconditioner_anew": 0}
    got = S.compute("random", return_info=True)
    _assert_same(got, want)
    assert got[1]["used_direct"] == (prec == "cholesky")
    assert S.state()["kept_width"] == gc.NEV + 4
    _assert_same(S.compute("random", return_info=True), want)          # the kept block does not reach a cold compute
    S.close()
    kept = geneo_basis(tl, nev=gc.NEV, tol=gc.TOL, preconditioner=prec, return_info=True, keep=True)
    _assert_same(kept, want)
    assert isinstance(tl.geneo, GeneoSolver) and tl.geneo.state()["kept_width"] == gc.NEV + 4
    tl.geneo.close()
    tl.ctx.close()


def test_cold_compute_is_geneo_basis_in_threshold_mode(ddm):
    """threshold 0.5, one doubling (test_geneo_threshold_mode_matches_oracle): both widths iterate on the one pencil and preconditioner"""
    from dune_ddm_amd.geneo import GeneoSolver, geneo_basis
    tl = _tl("old")
    kw = dict(nev=gc.THRESHOLD["nev"], tol=gc.TOL, threshold=gc.THRESHOLD["threshold"], nev_max=2 * gc.THRESHOLD["nev"])
    want = geneo_basis(tl, return_info=True, **kw)
    assert want[1]["nev"] == 8 and len(set(want[1]["nconv"].values())) > 1
    S = GeneoSolver(tl, **kw)
    _assert_same(S.compute("random", return_info=True), want)
    assert S.state()["kept_width"] == 8 + 4
    S.close()
    tl.ctx.close()


# ---- 2. refresh identity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,engine", PRECONDITIONERS)
def test_refresh_gives_the_bits_of_a_new_eigensolver(ddm, monkeypatch, prec, engine):
    from dune_ddm_amd.geneo import GeneoSolver, geneo_basis
    _engine(monkeypatch, engine)
    tl, tl_new = _tl("old"), _tl("new")
    kw = dict(nev=gc.NEV, tol=gc.TOL, preconditioner=prec)
    want_old = geneo_basis(tl, return_info=True, **kw)
    want_new = geneo_basis(tl_new, return_info=True, **kw)
    assert any(not np.array_equal(want_old[0][s], want_new[0][s]) for s in want_old[0])
    S = GeneoSolver(tl, **kw)
    first = S.compute("random", return_info=True)
    _assert_same(first, want_old)
    in_place = engine != "host"
    for step, which, want in ((1, "new", want_new), (2, "old", want_old)):              # there and back
        a, b = gc.neumann_values(which)
        S.update(a, b)
        A, B, pou, dm = gc.block_pencil_input(which)
        rp, ci, vt, vc, _ = ddm.geneo_pencil_host(A, B, pou, dm, gc.SHIFT)
        drp, dci, dvt, dvc = S.pencil()
        assert np.array_equal(drp, rp) and np.array_equal(dci, ci)
        assert dvt.tobytes() == vt.tobytes() and dvc.tobytes() == vc.tobytes()
        st = S.state()
        assert st["pencil_refreshes"] == step
        assert (st["preconditioner_in_place"], st["preconditioner_anew"]) == ((step, 0) if in_place else (0, step)), st
        _assert_same(S.compute("random", return_info=True), want)
    S.close()
    tl.ctx.close()
    tl_new.ctx.close()


def test_update_checks_the_lengths_first(ddm):
    from dune_ddm_amd.geneo import GeneoSolver
    tl = _tl("old")
    S = GeneoSolver(tl, nev=gc.NEV, tol=gc.TOL, preconditioner="ilu0")
    a, b = gc.neumann_values("new")
    short = dict(a)
    short[3] = short[3][:-1]
    with pytest.raises(ValueError, match="GeneoSolver.update"):
        S.update(short, b)
    with pytest.raises(ValueError, match="GeneoSolver.update"):
        S.update(a, short)
    assert S.state()["pencil_refreshes"] == 0
    S.close()
    tl.ctx.close()


def test_failed_rebuild_is_left_by_the_next_refresh(ddm, monkeypatch):
    """Host-engine Cholesky (built anew by every refresh) and values for which A~ is not positive definite (-A_neu): update raises
    DDM_ENUMERIC and leaves no preconditioner, compute raises the same code, and the next update -- the way out -- builds the factor
    again instead of refreshing the one that is not there; the result is the first one, bit for bit."""
    from dune_ddm_amd.geneo import GeneoSolver
    _engine(monkeypatch, "host")
    tl = _tl("old")
    S = GeneoSolver(tl, nev=gc.NEV, tol=gc.TOL, preconditioner="cholesky")
    first = S.compute("random", return_info=True)
    a, b = gc.neumann_values("old")
    with pytest.raises(ddm.DdmError) as err:
        S.update({s: -v for s, v in a.items()}, b)
    assert err.value.code == ddm.DDM_ENUMERIC
    st = S.state()
    assert st["pencil_refreshes"] == 1 and st["preconditioner_in_place"] == 0 and st["preconditioner_anew"] == 0, st
    for start in ("kept", "random"):
        with pytest.raises(ddm.DdmError) as err:
            S.compute(start)
        assert err.value.code == ddm.DDM_ENUMERIC
    S.update(a, b)
    st = S.state()
    assert st["pencil_refreshes"] == 2 and st["preconditioner_in_place"] == 0 and st["preconditioner_anew"] == 1, st
    _assert_same(S.compute("random", return_info=True), first)
    S.close()
    tl.ctx.close()


def test_setup_seconds_and_changed_parameters_between_computes(ddm):
    """info["setup_s"] is the setup since the last compute (creation, refresh), 0 for a compute that did none; nev lowered and extra
    raised between two computes: the warm run still begins at the kept nev, with the wider block's new columns drawn."""
    from dune_ddm_amd.geneo import GeneoSolver
    tl = _tl("old")
    S = GeneoSolver(tl, nev=gc.NEV, tol=gc.TOL, preconditioner="ilu0")
    _, i0 = S.compute("random", return_info=True)
    _, i1 = S.compute("kept", return_info=True)
    assert i0["setup_s"] > 0.0 and i1["setup_s"] == 0.0
    S.update(*gc.neumann_values("new"))
    S.par.nev, S.par.extra = 2, 6
    basis, i2 = S.compute("kept", return_info=True)
    assert 0.0 < i2["setup_s"] and i2["converged"] and i2["nev"] == gc.NEV and S.state()["kept_width"] == gc.NEV + 6
    _against_oracle(basis, i2, "new")
    S.close()
    tl.ctx.close()


# ---- 3. warm restart ---------------------------------------------------------------------------------------------------------------
def test_warm_restart_after_new_values(ddm):
    from dune_ddm_amd.geneo import GeneoSolver
    tl = _tl("old")
    S = GeneoSolver(tl, nev=gc.NEV, tol=gc.TOL)
    S.compute("random")
    S.update(*gc.neumann_values("new"))
    basis, info = S.compute("kept", return_info=True)
    assert info["converged"]
    _against_oracle(basis, info, "new")
    _, cold = S.compute("random", return_info=True)
    print(f"\n[geneo refresh] 25^3 islands, coefficient x [0.7, 1.3]: {info['iterations']} block iterations from the kept block, {cold['iterations']} from the random one")
    assert info["iterations"] <= cold["iterations"], f"warm {info['iterations']} block iterations, cold {cold['iterations']}"
    # no change of values: the kept block sits at the tolerance (one step of slack for rounding in the recomputed products)
    _, again = S.compute("kept", return_info=True)
    assert again["converged"] and again["iterations"] <= 2, again["iterations"]
    S.close()
    tl.ctx.close()


def test_warm_restart_that_doubles_in_threshold_mode(ddm):
    """The kept block has nev = 4; with the threshold switched on the warm compute on the new values doubles once, the wider block
    starting from the one just converged, and ends with the oracle's number of vectors per subdomain."""
    from dune_ddm_amd.geneo import GeneoSolver
    tl = _tl("old")
    S = GeneoSolver(tl, nev=gc.THRESHOLD["nev"], tol=gc.TOL)
    S.compute("random")
    assert S.state()["kept_width"] == 4 + 4
    S.par.threshold, S.par.nev_max = gc.THRESHOLD["threshold"], 2 * gc.THRESHOLD["nev"]
    S.update(*gc.neumann_values("new"))
    basis, info = S.compute("kept", return_info=True)
    assert info["converged"] and info["nev"] == 8 and S.state()["kept_width"] == 8 + 4
    _against_oracle(basis, info, "new", threshold=True)
    _, again = S.compute("kept", return_info=True)                     # starts at the kept nev = 8: no doubling left
    assert again["converged"] and again["nev"] == 8 and again["iterations"] <= 2
    S.close()
    tl.ctx.close()


# ---- 4. the start-block kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mk,m", [(5, 5), (5, 9), (8, 12), (24, 24)])
def test_start_block_kernel(ddm, mk, m):
    import torch
    ctx = ddm.torch_context(0)
    n, seed = 64 * 37 + 29, 0x5DEECE66D + 3
    rng = np.random.default_rng(100 * mk + m)
    mask = torch.as_tensor((rng.uniform(size=n) > 0.2).astype(np.float64)).cuda()
    assert 0 < int((mask == 0).sum()) < n
    kept = torch.as_tensor(rng.standard_normal((n, mk))).cuda()
    S = torch.full((n, 3 * m), float("nan"), dtype=torch.float64, device="cuda")
    ddm.geneo_start_block(ctx, seed, mask, kept, S)
    cold = torch.full((n, 3 * m), float("nan"), dtype=torch.float64, device="cuda")
    ddm.geneo_random(ctx, [0, n], seed, mask, cold[:, :m])              # the cold generator at the same strides
    ctx.sync()
    free = mask > 0
    assert torch.equal(S[free][:, :mk], kept[free])                     # kept columns bit for bit
    assert bool((S[~free] == 0).all())                                  # masked rows zero
    assert bool((S[:, m:] == 0).all())                                  # W / P slots zero
    assert torch.equal(S[:, mk:m], cold[:, mk:m])                       # new columns: the cold generator's for those column indices
    if m > mk:
        assert float(S[free][:, mk:m].abs().min()) > 0.0
    ctx.close()


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
def _two_level_with_kept_geneo():
    from dune_ddm_amd.geneo import geneo_basis
    from dune_ddm_amd.solver import TwoLevelSchwarz
    tl = TwoLevelSchwarz(gc.decomposition("old"), coarse="none")
    tl.set_coarse_basis(geneo_basis(tl, nev=gc.NEV, tol=gc.TOL, keep=True))
    tl.rebuild_combined("additive")
    return tl


def _new_rhs():
    from dune_ddm_amd.problem import RankLocal
    return np.asarray(RankLocal(gc.decomposition("new"), 0, 1).b, dtype=np.float64)


def test_update_values_with_coarse_refresh(ddm):
    from dune_ddm_amd.geneo import geneo_basis
    from dune_ddm_amd.solver import TwoLevelSchwarz
    b_new = _new_rhs()
    va, vd = gc.rank_values("new")
    a_neu, b_neu = gc.neumann_values("new")
    tl = _two_level_with_kept_geneo()
    with pytest.raises(ValueError, match="GeneoSolver.update"):        # before anything is touched
        tl.update_values(va, vd, A_neu_values={s: v[:-1] for s, v in a_neu.items()}, B_neu_values=b_neu, coarse="refresh")
    with pytest.raises(ValueError, match="A_neu_values"):
        tl.update_values(va, vd, coarse="refresh")
    assert tl.geneo.state()["pencil_refreshes"] == 0 and not any(k.startswith("refresh:") for k in tl.setup_times)
    tl.update_values(va, vd, A_neu_values=a_neu, B_neu_values=b_neu, coarse="refresh")
    assert tl.geneo.state()["pencil_refreshes"] == 1
    assert {"refresh: GenEO pencil and preconditioner", "refresh: GenEO basis from the kept block"} <= set(tl.setup_times)
    res, _, _ = tl.solve(reduction=1e-10, maxit=500, b=b_new)
    fresh = TwoLevelSchwarz(gc.decomposition("new"), coarse="none")
    fresh.set_coarse_basis(geneo_basis(fresh, nev=gc.NEV, tol=gc.TOL))
    fresh.rebuild_combined("additive")
    res_f, _, _ = fresh.solve(reduction=1e-10, maxit=500, b=b_new)
    print(f"\n[geneo refresh] CG iterations on the new values: refreshed basis {res.iterations}, new basis {res_f.iterations}")
    assert res.converged and res_f.converged
    assert abs(res.iterations - res_f.iterations) <= 1, (res.iterations, res_f.iterations)      # same coarse space up to the eigensolver tolerance
    tl.geneo.close()
    tl.ctx.close()
    fresh.ctx.close()


def test_update_values_default_keeps_the_basis(ddm):
    """coarse="keep" (the default) with a kept eigensolver around: the basis stays, the eigensolver is not touched, and the solve is bit
    for bit that of a new object on the new matrices with this basis -- what update_values promised before the keyword existed."""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    b_new = _new_rhs()
    va, vd = gc.rank_values("new")
    keep = _two_level_with_kept_geneo()
    keep.update_values(va, vd)
    assert keep.geneo.state()["pencil_refreshes"] == 0
    res_k, hist_k, x_k = keep.solve(reduction=1e-10, maxit=500, b=b_new)
    same = TwoLevelSchwarz(gc.decomposition("new"), coarse=keep.host_basis())
    res_s, hist_s, x_s = same.solve(reduction=1e-10, maxit=500, b=b_new)
    print(f"\n[geneo refresh] CG iterations on the new values with the stale basis: {res_k.iterations}")
    assert res_k.converged and res_k.iterations == res_s.iterations
    assert np.array_equal(hist_k, hist_s) and np.array_equal(x_k.cpu().numpy(), x_s.cpu().numpy())
    keep.geneo.close()
    keep.ctx.close()
    same.ctx.close()
