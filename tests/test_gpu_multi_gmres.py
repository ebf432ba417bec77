"""-m gpu: restarted GMRES for several right-hand sides at once (ddm_gmres_solve_multi) against ddm_gmres_solve column by column,
against the CPU oracle, and against itself (independence of the columns, frozen columns, the exchange paths).

Tolerances are the project's: GMRES histories within 1e-7 |r_k| + 1e-11 |r_0|, x within 1e-8 (ILU(0)) or 1e-7
(direct local solves) of the largest entry.  Everything that compares the block solver with itself is bitwise: the columns are
independent recurrences."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_multi_rhs import _consistent_block, _rhs_block
from tests.test_gpu_parity import _build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL_HIST, ATOL_HIST = 1e-7, 1e-11
MAXIT = 200

CONFIGS = {
    # the reference's shipped configuration (examples/poisson.ini)
    "a": dict(kind="poisson", stype="restricted", mode="multiplicative", solver="ilu0", restart=100, xtol=1e-8),
    # restart 6: four restart cycles (test_column_frozen_through_restarts adds columns that end in different cycles)
    "b": dict(kind="poisson", stype="restricted", mode="additive", solver="ilu0", restart=6, xtol=1e-8),
    # non-symmetric DG operator, L U local solves (configs[3] in small)
    "c": dict(kind="dg", stype="standard", mode="additive", solver="umfpack", restart=50, xtol=1e-7),
    "d": dict(kind="poisson", stype="restricted", mode="multiplicative", solver="cholmod", restart=100, xtol=1e-7),
}


def _make(ddm, key):
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz
    cfg = CONFIGS[key]
    if cfg["kind"] == "poisson":
        dec = _build(ddm, (17, 16, 15), (2, 2, 2))
    else:
        dec = build_structured(synth.StructuredDG2D((24, 24), (2, 2)), overlap=2)
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type=cfg["stype"], mode=cfg["mode"], subdomain_solver=cfg["solver"])
    return cfg, dec, tl


def _block_solve(ddm, tl, Bh, restart, maxit=MAXIT):
    """the block solve from a zero X on fresh copies: (res, hist, X, B after the solve)"""
    import torch
    Bd = tl.to_device(np.ascontiguousarray(Bh, dtype=np.float64)).contiguous().clone()
    X = torch.zeros_like(Bd)
    res, hist = ddm.gmres_solve_multi(tl.ctx, tl.op, tl.prec, X, Bd, 1e-10, maxit, restart, True)
    return res, hist, X, Bd


def _hist_close(h, ref):
    return bool((np.abs(h - ref) <= RTOL_HIST * ref + ATOL_HIST * ref[0]).all())


@pytest.mark.parametrize("key", sorted(CONFIGS))
def test_columns_match_single_solves(ddm, key):
    """Every column of the m = 5 block (b, random, 2 b, zero, random) against tl.solve(solver="restartedgmressolver") on that column:
    same iteration count and converged flag, history and x within the project's tolerances; the zero column converges at once."""
    cfg, dec, tl = _make(ddm, key)
    Bh = _rhs_block(tl, dec)
    m = Bh.shape[1]
    res, hist, X, _ = _block_solve(ddm, tl, Bh, cfg["restart"])
    Xh = X.cpu().numpy()
    its = [r.iterations for r in res]
    print(key, "block iterations", its)
    assert len(res) == m and hist.shape == (max(its) + 1, m)
    for j in range(m):
        if j == 3:
            continue
        r1, h1, x1 = tl.solve(reduction=1e-10, maxit=MAXIT, b=Bh[:, j], solver="restartedgmressolver", restart=cfg["restart"])
        x1 = x1.cpu().numpy()
        hj = hist[:res[j].iterations + 1, j]
        k = min(len(hj), len(h1))
        print(key, "column", j, "iterations", res[j].iterations, r1.iterations, "history deviation / |r_k|", float(np.max(np.abs(hj[:k] - h1[:k]) / h1[:k])),
              "x deviation", float(np.max(np.abs(Xh[:, j] - x1)) / np.max(np.abs(x1))))
        assert res[j].iterations == r1.iterations and res[j].converged == r1.converged == 1, (j, res[j].iterations, r1.iterations)
        assert _hist_close(hj, h1), j
        assert np.isnan(hist[res[j].iterations + 1:, j]).all()
        assert np.max(np.abs(Xh[:, j] - x1)) <= cfg["xtol"] * np.max(np.abs(x1)), j
        assert res[j].reduction <= 1e-10
    assert res[3].iterations == 0 and res[3].converged == 1 and res[3].def0 == 0.0
    assert not np.any(Xh[:, 3]) and hist[0, 3] == 0.0 and np.isnan(hist[1:, 3]).all()
    tl.prec.check_status()
    tl.ctx.close()


@pytest.mark.parametrize("m", [1, 3, 8, 13])
def test_block_widths_match_single_solves(ddm, m):
    """The widths the column-group dispatch branches on, m = 1, 3 (2 + 1), 8 and 13 (8 + 4 + 1), on configuration a with m seeded
    consistent columns: columns 0 and m - 1 against tl.solve(solver="restartedgmressolver") as in test_columns_match_single_solves."""
    cfg, dec, tl = _make(ddm, "a")
    Bh = _consistent_block(tl, dec, m, seed=40 + m)
    res, hist, X, _ = _block_solve(ddm, tl, Bh, cfg["restart"])
    Xh = X.cpu().numpy()
    its = [r.iterations for r in res]
    print("m", m, "block iterations", its)
    assert len(res) == m and hist.shape == (max(its) + 1, m)
    for j in sorted({0, m - 1}):
        r1, h1, x1 = tl.solve(reduction=1e-10, maxit=MAXIT, b=Bh[:, j], solver="restartedgmressolver", restart=cfg["restart"])
        x1 = x1.cpu().numpy()
        hj = hist[:res[j].iterations + 1, j]
        k = min(len(hj), len(h1))
        print("m", m, "column", j, "iterations", res[j].iterations, r1.iterations, "history deviation / |r_k|", float(np.max(np.abs(hj[:k] - h1[:k]) / h1[:k])),
              "x deviation", float(np.max(np.abs(Xh[:, j] - x1)) / np.max(np.abs(x1))))
        assert res[j].iterations == r1.iterations and res[j].converged == r1.converged == 1, (j, res[j].iterations, r1.iterations)
        assert _hist_close(hj, h1), j
        assert np.isnan(hist[res[j].iterations + 1:, j]).all()
        assert np.max(np.abs(Xh[:, j] - x1)) <= cfg["xtol"] * np.max(np.abs(x1)), j
        assert res[j].reduction <= 1e-10
    tl.prec.check_status()
    tl.ctx.close()


@pytest.mark.parametrize("key", ["a", "b", "c"])
def test_columns_are_independent_bit_for_bit(ddm, key):
    """Exact scaling (column 2 = 2 x column 0), permutation of the columns, and a second solve on the same objects: all bitwise."""
    cfg, dec, tl = _make(ddm, key)
    Bh = _rhs_block(tl, dec)
    res, hist, X, _ = _block_solve(ddm, tl, Bh, cfg["restart"])
    Xh = X.cpu().numpy()
    assert res[2].iterations == res[0].iterations
    assert np.array_equal(Xh[:, 2], 2.0 * Xh[:, 0]) and np.array_equal(hist[:, 2], 2.0 * hist[:, 0], equal_nan=True)
    perm = [4, 2, 0, 3, 1]
    resp, histp, Xp, _ = _block_solve(ddm, tl, Bh[:, perm], cfg["restart"])
    assert [r.iterations for r in resp] == [res[p].iterations for p in perm]
    assert np.array_equal(Xp.cpu().numpy(), Xh[:, perm]) and np.array_equal(histp, hist[:, perm], equal_nan=True)
    res2, hist2, X2, _ = _block_solve(ddm, tl, Bh, cfg["restart"])
    assert np.array_equal(X2.cpu().numpy(), Xh) and np.array_equal(hist2, hist, equal_nan=True)
    tl.prec.check_status()
    tl.ctx.close()


@pytest.mark.parametrize("key", ["a", "b"])
def test_frozen_columns_keep_x_and_b(ddm, key):
    """maxit = the iteration count of the earliest non-zero column: its x and its column of B are those of the full run bit for bit (in
    the full run it sat frozen while the others went on, through restarts in configuration b); the slower columns report
    converged == 0 and iterations == maxit."""
    import torch
    cfg, dec, tl = _make(ddm, key)
    Bh = _rhs_block(tl, dec)
    m = Bh.shape[1]
    res, hist, X, Bd = _block_solve(ddm, tl, Bh, cfg["restart"])
    its = [r.iterations for r in res]
    early = min((j for j in range(m) if j != 3), key=lambda j: its[j])
    if key == "a":
        assert its[early] < max(its), its                                 # the block holds slower columns
    res2, hist2, X2, Bd2 = _block_solve(ddm, tl, Bh, cfg["restart"], maxit=its[early])
    assert res2[early].converged == 1 and res2[early].iterations == its[early]
    assert torch.equal(X2[:, early], X[:, early]) and torch.equal(Bd2[:, early], Bd[:, early])
    assert torch.equal(Bd[:, 3], tl.to_device(Bh[:, 3].copy())) and not torch.any(X[:, 3])   # the zero column was never touched
    for j in range(m):
        if its[j] > its[early]:
            assert res2[j].converged == 0 and res2[j].iterations == its[early], j
            assert np.array_equal(hist2[:, j], hist[:its[early] + 1, j])
    tl.prec.check_status()
    tl.ctx.close()


def test_column_frozen_through_restarts(ddm):
    """Configuration b (restart 6) with columns that end in different restart cycles: b and a random vector, and both scaled by 2^-83
    (about 1e-25), which the absolute test norm < 1e-30 stops after about half the iterations.  Every column against the single-vector
    solve; the early columns sit frozen while the block goes through further restarts (B -= A W, v0 = M^-1 B): their x and their
    columns of B are those of a run that ends where they converged, bit for bit."""
    import torch
    cfg, dec, tl = _make(ddm, "b")
    R = restart = cfg["restart"]
    b0 = np.asarray(tl.rl.b, dtype=np.float64)
    r0 = _consistent_block(tl, dec, 1, seed=5)[:, 0]
    tiny = 2.0 ** -83
    Bh = np.stack([b0, tiny * b0, r0, tiny * r0], axis=1)
    res, hist, X, Bd = _block_solve(ddm, tl, Bh, restart)
    its = [r.iterations for r in res]
    print("iterations", its, "restart", R)
    for j in range(4):
        r1, h1, x1 = tl.solve(reduction=1e-10, maxit=MAXIT, b=Bh[:, j], solver="restartedgmressolver", restart=restart)
        x1 = x1.cpu().numpy()
        assert res[j].iterations == r1.iterations and res[j].converged == r1.converged == 1, (j, its, r1.iterations)
        assert _hist_close(hist[:its[j] + 1, j], h1), j
        assert np.max(np.abs(X[:, j].cpu().numpy() - x1)) <= cfg["xtol"] * np.max(np.abs(x1)), j
    cycle = [(i - 1) // R for i in its]
    assert cycle[1] < cycle[0] and cycle[3] < cycle[2], its               # the scaled columns end in an earlier restart cycle
    for early in (1, 3):
        res2, hist2, X2, Bd2 = _block_solve(ddm, tl, Bh, restart, maxit=its[early])
        assert res2[early].converged == 1 and res2[early].iterations == its[early]
        assert torch.equal(X2[:, early], X[:, early]) and torch.equal(Bd2[:, early], Bd[:, early])
        for j in range(4):
            if its[j] > its[early]:
                assert res2[j].converged == 0 and res2[j].iterations == its[early], j
    tl.prec.check_status()
    tl.ctx.close()


@pytest.mark.parametrize("key", ["a", "c"])
def test_column0_matches_oracle(ddm, key):
    from tests.oracle_bridge import oracle_solve
    cfg, dec, tl = _make(ddm, key)
    res, hist, X, _ = _block_solve(ddm, tl, _rhs_block(tl, dec), cfg["restart"])
    it, conv, hist_o, xo = oracle_solve(dec, reduction=1e-10, maxit=MAXIT, solver="restartedgmressolver", restart=cfg["restart"], coarse="pou",
                                        schwarz_type=cfg["stype"], mode=cfg["mode"], local_solver="ilu0" if cfg["solver"] == "ilu0" else "direct")
    ho = np.array(hist_o)
    assert res[0].iterations == it and res[0].converged and conv, (res[0].iterations, it)
    assert _hist_close(hist[:it + 1, 0], ho)
    want = np.concatenate(xo)
    assert np.max(np.abs(X[:, 0].cpu().numpy() - want)) <= cfg["xtol"] * np.max(np.abs(want))
    tl.ctx.close()


def test_errors_are_host_side_refusals(ddm):
    """A set local-solve status word, a NaN right-hand side and a basis larger than the device's memory: all refused by the host
    before or between launches; the context works afterwards.  Then ddm_gmres_solve on one column: bad arguments (restart 0, maxit -1,
    x == b, a null x), the status word and a basis larger than the free memory are refused in the same way."""
    import torch
    cfg, dec, tl = _make(ddm, "b")
    lib, h = tl.ctx.lib, tl.ctx.h
    Bh = _rhs_block(tl, dec)
    n_o, m = Bh.shape
    res = (ddm.SolveResult * m)()

    def raw(Bhost, maxit, restart):
        Bd = tl.to_device(np.ascontiguousarray(Bhost)).contiguous().clone()
        X = torch.zeros_like(Bd)
        rc = lib.ddm_gmres_solve_multi(h, tl.op.h, tl.prec.h, m, X.data_ptr(), Bd.data_ptr(), 1e-10, maxit, restart, None, res)
        tl.ctx.sync()
        return rc, lib.ddm_last_error(h).decode(), X, Bd

    F = ctypes.c_void_p(tl.schwarz.local_solver())
    assert lib.ddm_ilu0_set_status(F, 1) == ddm.DDM_OK
    try:
        rc, msg, X, Bd = raw(Bh, 50, 6)
        assert rc == ddm.DDM_ENUMERIC
        assert not torch.any(X) and torch.equal(Bd, tl.to_device(Bh.copy()))      # nothing was launched: B is still the right-hand side
    finally:
        assert lib.ddm_ilu0_set_status(F, 0) == ddm.DDM_OK
    rc, msg, X, _ = raw(Bh, MAXIT, 6)
    assert rc == ddm.DDM_OK and all(res[c].converged for c in range(m)), msg

    Bnan = Bh.copy()
    Bnan[7, 1] = np.nan
    rc, msg, _, _ = raw(Bnan, 50, 6)
    assert rc == ddm.DDM_ENUMERIC and "column 1" in msg and "ddm_gmres_solve_multi" in msg, msg

    total = torch.cuda.mem_get_info()[1]
    big = int(total // (n_o * m * 8)) + 1                                       # (big + 2) blocks of n_o x m doubles exceed the device's memory
    assert (big + 2) * n_o * m * 8 > total and big < 2**31 - 8
    free_before = torch.cuda.mem_get_info()[0]
    rc, msg, _, _ = raw(Bh, big, big)
    assert rc == ddm.DDM_ENOTIMPL and "bytes" in msg and "ddm_gmres_solve_multi" in msg, msg
    assert str((big + 2) * n_o * m * 8) in msg, msg
    assert torch.cuda.mem_get_info()[0] >= free_before - (64 << 20)             # nothing of that size was allocated
    rc, msg, X2, _ = raw(Bh, MAXIT, 6)                                          # the context is still usable
    assert rc == ddm.DDM_OK and torch.equal(X2, X), msg

    # ddm_gmres_solve on column 0 refuses the same things: DDM_EINVAL before any device work (a poisoned x stays poisoned, b stays the
    # right-hand side), a set status word on entry, a basis larger than the free device memory
    b0 = tl.to_device(Bh[:, 0].copy())
    b1 = b0.clone()
    x1 = torch.full_like(b1, 123.456)
    poison = x1.clone()

    def single(xp, bp, maxit, restart):
        rc = lib.ddm_gmres_solve(h, tl.op.h, tl.prec.h, xp, bp, 1e-10, maxit, restart, None, res)
        tl.ctx.sync()
        return rc, lib.ddm_last_error(h).decode()

    for args in [(x1.data_ptr(), b1.data_ptr(), 50, 0), (x1.data_ptr(), b1.data_ptr(), -1, 6), (x1.data_ptr(), x1.data_ptr(), 50, 6), (None, b1.data_ptr(), 50, 6)]:
        rc, msg = single(*args)
        assert rc == ddm.DDM_EINVAL and "ddm_gmres_solve:" in msg, (args, rc, msg)
    assert torch.equal(x1, poison) and torch.equal(b1, b0)
    assert lib.ddm_ilu0_set_status(F, 1) == ddm.DDM_OK
    try:
        assert single(x1.data_ptr(), b1.data_ptr(), 50, 6)[0] == ddm.DDM_ENUMERIC
        assert torch.equal(x1, poison) and torch.equal(b1, b0)                  # refused on entry: b is still the right-hand side
    finally:
        assert lib.ddm_ilu0_set_status(F, 0) == ddm.DDM_OK
    free = torch.cuda.mem_get_info()[0]
    big1 = int(free // (n_o * 8)) + 1                                           # (big1 + 2) vectors of n_o doubles exceed the free memory
    if big1 < 2**31 - 8:
        rc, msg = single(x1.data_ptr(), b1.data_ptr(), big1, big1)
        assert rc == ddm.DDM_ENOTIMPL and "bytes" in msg and "ddm_gmres_solve:" in msg and str((big1 + 2) * n_o * 8) in msg, msg
        assert torch.cuda.mem_get_info()[0] >= free - (64 << 20)               # nothing of that size was allocated
        assert torch.equal(x1, poison) and torch.equal(b1, b0)
    x1.zero_()
    rc, msg = single(x1.data_ptr(), b1.data_ptr(), MAXIT, 6)                    # a normal solve afterwards converges
    assert rc == ddm.DDM_OK and res[0].converged == 1 and res[0].reduction <= 1e-10, msg
    tl.prec.check_status()
    tl.ctx.close()


def test_rccl_self_test_is_bit_identical(ddm):
    """The in-library exchange on one GPU (communicator of size 1 in self-test mode: every halo segment and every all-reduce of m
    Gram-Schmidt coefficients goes through RCCL) against the plain single-rank block solve."""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    dec = _build(ddm, (15, 14, 13), (2, 2, 2))
    kw = dict(coarse="pou", schwarz_type="restricted", mode="additive")
    tl0 = TwoLevelSchwarz(dec, **kw)
    Bh = _rhs_block(tl0, dec)
    res0, hist0, X0, _ = _block_solve(ddm, tl0, Bh, 6)
    X0 = X0.cpu().numpy()
    tl0.ctx.close()
    os.environ["DDM_RCCL_SELFTEST"] = "1"
    try:
        tl = TwoLevelSchwarz(dec, **kw)
    finally:
        del os.environ["DDM_RCCL_SELFTEST"]
    assert tl.exchange == "rccl"
    res, hist, X, _ = _block_solve(ddm, tl, Bh, 6)
    tl.prec.check_status()
    assert [r.iterations for r in res] == [r.iterations for r in res0] and all(r.converged for r in res)
    assert np.array_equal(hist, hist0, equal_nan=True) and np.array_equal(X.cpu().numpy(), X0)
    tl.ctx.close()


def test_two_rank_block_gmres_matches_single_rank():
    """two ranks over gloo sharing the GPU (`levels` engine, callback exchange column by column) against the one-rank block solve"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29593", os.path.join(ROOT, "tests", "mp_multi_gmres_worker.py"), "ranks"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "MULTI_GMRES_RANKS_OK 2" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
