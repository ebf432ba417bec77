"""-m gpu: the additive combination with the coarse chain on a side stream beside the local solve (DDM_OVERLAP_COARSE=1) against the
one-stream path (=0).  Both run the same kernels' sums in the same order -- the spread basis passes add what the full-grid ones add, the
pipe engine's output permutation applies the POU scale and the coarse correction either way, the other engines append k_scale / k_axpy --
so every comparison is torch.equal.  The combined preconditioner reads the switches when it is created: each case builds the problem once
and creates the two preconditioners on it, so nothing here depends on the default."""
import ctypes

import numpy as np
import pytest

from tests.coarse_cases import ragged_basis

pytestmark = pytest.mark.gpu

# (grid, coarse space, DDM_TRSV_MODE, DDM_OVERLAP_GRID).  2x2x2 subdomains with overlap 2: 14^3 rows per subdomain at 24^3, 18^3 / 19^3
# at 33^3 -- no multiple of 64, shorter than one 8192-row chunk, the last trip of a wave incomplete.
#   "ragged": restricted Schwarz (the POU scale is folded too), 5 vectors per subdomain (one trip of four and one single vector in the prolongation), subdomain 5 has 3 (zero rows,
#             coarse_index < 0); 8 x 5 work items of the restriction and 8 of the prolongation: most waves of the default grid idle
#   "pou":    one vector, kmax no multiple of 4
CASES = [
    pytest.param(24, "ragged", None, None, id="24-ragged-default-grid"),
    pytest.param(24, "ragged", None, "1", id="24-ragged-one-wave"),
    pytest.param(33, "ragged", None, "7", id="33-ragged-grid7"),
    pytest.param(33, "pou", None, None, id="33-pou"),
    pytest.param(24, "ragged", "levels", None, id="24-ragged-levels-engine"),
]


def build_pair(ddm, monkeypatch, grid, coarse, trsv, side_grid):
    """the problem once, and on it the preconditioner with the coarse chain beside the local solve and the one-stream one"""
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz, pou_basis
    if trsv:
        monkeypatch.setenv("DDM_TRSV_MODE", trsv)
    else:
        monkeypatch.delenv("DDM_TRSV_MODE", raising=False)
    dec = build_structured(synth.StructuredPoisson((grid,) * 3, (2, 2, 2)), overlap=2, pou_type="distance", shrink=0)
    tl = TwoLevelSchwarz(dec, coarse="none", schwarz_type="restricted" if coarse == "ragged" else "standard", mode="additive")
    tl.set_coarse_basis(ragged_basis(tl.rl) if coarse == "ragged" else pou_basis(tl.rl))
    tl.schwarz.wait_setup()
    assert tl.schwarz.engine() == (trsv or "pipe")
    if side_grid:
        monkeypatch.setenv("DDM_OVERLAP_GRID", side_grid)
    else:
        monkeypatch.delenv("DDM_OVERLAP_GRID", raising=False)
    precs = {}
    for on in ("1", "0"):
        monkeypatch.setenv("DDM_OVERLAP_COARSE", on)
        tl.rebuild_combined("additive")
        precs[on] = tl.prec
    return tl, precs["1"], precs["0"]


@pytest.mark.parametrize("grid,coarse,trsv,side_grid", CASES)
def test_overlapped_apply_and_cg_are_bit_identical(ddm, monkeypatch, grid, coarse, trsv, side_grid):
    import torch
    tl, p_on, p_off = build_pair(ddm, monkeypatch, grid, coarse, trsv, side_grid)
    n = tl.rl.n_o
    rng = np.random.default_rng(grid)
    for rep in range(3):
        d = tl.to_device(rng.standard_normal(n))
        out = {}
        for name, p in (("on", p_on), ("off", p_off), ("on again", p_on)):
            x = torch.full((n,), float("nan"), dtype=torch.float64, device=d.device)
            p.apply(x, d)
            tl.ctx.sync()
            p.check_status()
            out[name] = x
        assert torch.isfinite(out["off"]).all()
        assert torch.equal(out["on"], out["off"]) and torch.equal(out["on again"], out["off"])
    runs = {}
    for name, p in (("on", p_on), ("off", p_off)):
        x = tl.zeros(n)
        b = tl.to_device(tl.rl.b)
        cg = ddm.CgIteration(tl.ctx, tl.op, p, x, b)
        cg.steps(4)          # (two calls: the deferred defect norm rides on the coarse all-reduce inside a call and not across calls)
        cg.steps(6)
        deff = cg.defect()
        p.check_status()
        cg.end()
        runs[name] = (x, b, deff)
    assert np.isfinite(runs["off"][2]) and torch.isfinite(runs["off"][0]).all()   # (equal numbers, not equal garbage)
    assert torch.equal(runs["on"][0], runs["off"][0])                           # iterate
    assert torch.equal(runs["on"][1], runs["off"][1])                           # residual
    assert runs["on"][2] == runs["off"][2]                                      # defect norm


def test_failed_cg_call_leaves_no_rider_behind(ddm, monkeypatch):
    """ddm_cg_steps that returns an error (the local solver's status word is set: the first preconditioner apply of the call fails)
    and ddm_cg_end leave no scalar waiting for the next coarse all-reduce: the Galerkin apply that follows reduces exactly K doubles,
    with the chain on the side stream as on one.  (The pending scalar is a local of ddm_cg_steps that reaches the all-reduce as an
    argument of the preconditioner apply, so it cannot outlive the call whichever way the call returns: this test pins that.)"""
    tl, p_on, p_off = build_pair(ddm, monkeypatch, 24, "ragged", None, None)
    lib, n = tl.ctx.lib, tl.rl.n_o
    F = ctypes.c_void_p(tl.schwarz.local_solver())
    for p in (p_on, p_off):
        x, b = tl.zeros(n), tl.to_device(tl.rl.b)
        cg = ddm.CgIteration(tl.ctx, tl.op, p, x, b)
        cg.steps(3)
        assert lib.ddm_ilu0_set_status(F, 1) == ddm.DDM_OK
        try:
            assert lib.ddm_cg_steps(tl.ctx.h, cg.h, 3) == ddm.DDM_ENUMERIC
        finally:
            assert lib.ddm_ilu0_set_status(F, 0) == ddm.DDM_OK
        y = tl.zeros(n)
        before = tl.ctx.comm_counts()
        tl.galerkin.apply(y, b)
        after = tl.ctx.comm_counts()
        assert (after[0] - before[0], after[1] - before[1]) == (1, tl.K)
        cg.steps(2)          # the iteration goes on after the failed call
        cg.end()
        before = tl.ctx.comm_counts()
        tl.galerkin.apply(y, b)
        after = tl.ctx.comm_counts()
        assert (after[0] - before[0], after[1] - before[1]) == (1, tl.K)
        tl.ctx.sync()
        p.check_status()
