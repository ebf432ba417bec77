"""-m gpu: any number of right-hand sides through a CG block of fixed width (ddm_cg_solve_queue, TwoLevelSchwarz.solve_many) against
ddm_cg_solve column by column, against the chunked block call (solve_multi on w columns at a time, what a caller had to do before)
and against itself (refill paths, side effects, status).

Two problems, both 2 x 2 x 2 subdomains with overlap 2, standard Schwarz with ILU(0), additive: "golden", the 12^3 Poisson problem of
tests/golden/poisson12_2x2x2.npz with the POU coarse space, and "shapes", the (13, 12, 11) grid of tests/test_gpu_apply_shapes.py with
its uneven coarse basis.  Column 0 is the problem's right-hand side, the others are seeded consistent random vectors.

Tolerances are those of tests/test_gpu_multi_rhs.py for a block column against the single-vector solve: the same iteration count and
converged flag, the history within RTOL_HIST |r_k| + ATOL_HIST |r_0|, x within 1e-8 of the largest entry (direct local solves: history
1e-7 / 1e-11).  Against the chunked block call and against itself the comparison is bitwise: per column the block kernels' arithmetic
depends on the block width only, not on the slot or on the neighbouring columns, and a refilled slot starts from p = q exactly."""
import ctypes

import numpy as np
import pytest

from tests.test_apply_shapes_reference import SMALL, build_case, consistent_columns
from tests.test_fgmres_cpu import golden_poisson
from tests.test_gpu_parity import ATOL_HIST, RTOL_HIST

pytestmark = pytest.mark.gpu

XTOL = 1e-8          # x of a block column against the single-vector solve (tests/test_gpu_multi_rhs.py)
MAXIT = 300
NCOLS = 70


class Problem:
    """One decomposition with its solver object, NCOLS fixed right-hand sides and, computed once per column, the single-vector solve"""

    def __init__(self, ddm, name, subdomain_solver="ilu0"):
        from dune_ddm_amd.solver import TwoLevelSchwarz
        if name == "golden":
            self.dec, coarse = golden_poisson(ddm), "pou"
        else:
            self.dec, coarse = build_case(ddm, SMALL)
        self.tl = TwoLevelSchwarz(self.dec, coarse=coarse, schwarz_type="standard", mode="additive", subdomain_solver=subdomain_solver)
        R = consistent_columns(self.dec, NCOLS - 1, seed=5)
        self.B = np.concatenate([np.asarray(self.tl.rl.b, dtype=np.float64)[:, None], R], axis=1)
        self.X0 = consistent_columns(self.dec, 4, seed=77)      # non-zero initial guesses for the tests that need some
        self._single = {}

    def single(self, j, maxit=MAXIT, x0=None, key=None, reduction=1e-10):
        """(SolveResult, history, x as a host array) of ddm_cg_solve on column j"""
        k = (j, maxit, key, reduction)
        assert (x0 is None) == (key is None)
        if k not in self._single:
            r, h, x = self.tl.solve(reduction=reduction, maxit=maxit, b=self.B[:, j], x0=x0)
            self._single[k] = (r, np.asarray(h), x.cpu().numpy())
        return self._single[k]


@pytest.fixture(scope="module")
def problems(ddm):
    made = {}

    def get(name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in made:
            made[key] = Problem(ddm, name, **kw)
        return made[key]
    yield get
    for p in made.values():
        p.tl.ctx.close()


def _assert_column_matches_single(res, hist, Xh, j, single, rtol=RTOL_HIST, atol=ATOL_HIST, what=""):
    r1, h1, x1 = single
    assert res[j].iterations == r1.iterations and res[j].converged == r1.converged, (what, j, res[j].iterations, r1.iterations, res[j].converged)
    hj = hist[:res[j].iterations + 1, j]
    assert (np.abs(hj - h1) <= rtol * h1 + atol * h1[0]).all(), (what, j)
    assert np.isnan(hist[res[j].iterations + 1:, j]).all(), (what, j)          # the history is the column's own: it stops where the column stopped
    assert np.max(np.abs(Xh[:, j] - x1)) <= XTOL * np.max(np.abs(x1)), (what, j)
    assert res[j].def0 == hist[0, j] and abs(res[j].def0 - h1[0]) <= rtol * h1[0], (what, j)
    if r1.converged:
        assert res[j].reduction <= 1e-10


# ---- 1. shapes the loop branches on ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["golden", "shapes"])
@pytest.mark.parametrize("M, w", [(1, 1), (5, 8), (9, 4), (32, 32), (70, 32), (13, 7)])
def test_columns_match_single_solves(ddm, problems, name, M, w):
    """M < w, a ragged tail, the full block, more columns than MULTI_MAX, an odd width (scalar SpMM and level kernels): every column
    behaves like ddm_cg_solve on it."""
    p = problems(name)
    res, hist, X = p.tl.solve_many(p.B[:, :M], width=w, reduction=1e-10, maxit=MAXIT)
    Xh = X.cpu().numpy()
    its = [r.iterations for r in res]
    print(f"\n{name} M = {M}, w = {w}: iterations {its}")
    assert len(res) == M and hist.shape == (max(its) + 1, M) and Xh.shape == (p.tl.rl.n_o, M)
    for j in range(M):
        assert res[j].converged == 1
        _assert_column_matches_single(res, hist, Xh, j, p.single(j), what=(name, M, w))
    p.tl.prec.check_status()


# ---- 2. against the chunked block call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["golden", "shapes"])
@pytest.mark.parametrize("M, w", [(16, 4), (64, 32)])
def test_columns_equal_the_chunked_block_solve_bitwise(ddm, problems, name, M, w):
    """x, history and iteration count of every column equal, bit for bit, those of solve_multi on the chunk of w columns that holds it."""
    import torch
    p = problems(name)
    res, hist, X = p.tl.solve_many(p.B[:, :M], width=w, reduction=1e-10, maxit=MAXIT)
    for c0 in range(0, M, w):
        rc, hc, Xc = p.tl.solve_multi(p.B[:, c0:c0 + w], reduction=1e-10, maxit=MAXIT)
        for k in range(w):
            j = c0 + k
            it = rc[k].iterations
            assert res[j].iterations == it and res[j].converged == rc[k].converged == 1, (j, res[j].iterations, it)
            assert res[j].def0 == rc[k].def0 and res[j].reduction == rc[k].reduction, j
            assert np.array_equal(hist[:it + 1, j], hc[:it + 1, k]), (j, float(np.max(np.abs(hist[:it + 1, j] - hc[:it + 1, k]))))
            assert torch.equal(X[:, j], Xc[:, k]), (j, float((X[:, j] - Xc[:, k]).abs().max()))
    p.tl.prec.check_status()


# ---- 3. refill paths --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["golden", "shapes"])
def test_zero_columns_are_finished_at_the_boundary(ddm, problems, name):
    """Zero right-hand sides (def0 < 1e-30: converged with 0 iterations, the slot is refilled again at the same boundary): two of them
    at the head of the queue, two in a row in the middle (a chain of immediate refills) and one as the last column."""
    p = problems(name)
    order = [None, None, 0, 1, None, None, 2, 3, None]           # None: a zero column, j: column j of the problem
    B = np.stack([np.zeros(p.tl.rl.n_o) if j is None else p.B[:, j] for j in order], axis=1)
    res, hist, X = p.tl.solve_many(B, width=3, reduction=1e-10, maxit=MAXIT)
    Xh = X.cpu().numpy()
    for c, j in enumerate(order):
        if j is None:
            assert res[c].iterations == 0 and res[c].converged == 1 and res[c].def0 == 0.0, c
            assert not np.any(Xh[:, c]) and hist[0, c] == 0.0 and np.isnan(hist[1:, c]).all(), c
        else:
            r1, h1, x1 = p.single(j)
            assert res[c].iterations == r1.iterations and res[c].converged == 1, (c, res[c].iterations, r1.iterations)
            assert (np.abs(hist[:r1.iterations + 1, c] - h1) <= RTOL_HIST * h1 + ATOL_HIST * h1[0]).all(), c
            assert np.max(np.abs(Xh[:, c] - x1)) <= XTOL * np.max(np.abs(x1)), c
    # nothing but zero columns: no iteration at all
    res, hist, X = p.tl.solve_many(np.zeros((p.tl.rl.n_o, 5)), width=2, maxit=MAXIT)
    assert all(r.iterations == 0 and r.converged == 1 for r in res) and hist.shape == (1, 5) and not X.any()
    p.tl.prec.check_status()


TINY = 2.0 ** -83     # about 1e-25: a column scaled by it is stopped by the absolute test def < 1e-30 well before it reaches 1e-10 def0


def _assert_equals_chunked(p, B, X0, w, red, res, hist, X):
    """every column of a queued run against solve_multi on the chunk of w columns that holds it, from the same initial guesses: bitwise"""
    import torch
    for c0 in range(0, B.shape[1], w):
        rc, hc, Xc = p.tl.solve_multi(B[:, c0:c0 + w], reduction=red, maxit=MAXIT, X0=None if X0 is None else X0[:, c0:c0 + w])
        for k in range(w):
            j = c0 + k
            it = rc[k].iterations
            assert res[j].iterations == it and res[j].converged == rc[k].converged == 1 and res[j].def0 == rc[k].def0, (j, res[j].iterations, it)
            assert np.array_equal(hist[:it + 1, j], hc[:it + 1, k]) and np.isnan(hist[it + 1:, j]).all(), j
            assert torch.equal(X[:, j], Xc[:, k]), j


def test_warm_started_and_early_columns(ddm, problems):
    """Columns that start from a previously computed solution among columns that start from zero, and columns that leave their slot
    well before the others.

    Warm start: the stop test is relative to the column's own def0, which for a converged X0 is about 1e-10 |b|, so the reduction asked
    for is a mild 1e-3.  Such a def0 is what is left of b - A x after ten digits cancelled, so the single-vector solve (another SpMV
    summation order) is no reference at 1e-8; the reference is the chunked block call from the same initial guesses, bit for bit.
    Measured on the 12^3 problem: the warm columns need 9-10 iterations to 1e-3, exactly as many as the cold ones -- CG converges at
    the same rate from any start, a converged X0 does not make a column finish in 0-1 iterations.

    Early leavers are therefore made with the absolute test: a right-hand side scaled by 2^-83 runs the same recurrence exactly scaled
    and passes def < 1e-30 when its reduction is near 1e-6, iterations before the unscaled column passes 1e-10 def0."""
    p = problems("golden")
    M, w, red = 9, 3, 1e-3
    warm = (0, 1, 4, 8)
    B = p.B[:, :M]
    first, _, Xs = p.tl.solve_many(B, width=w, reduction=1e-10, maxit=MAXIT)
    X0 = np.zeros((p.tl.rl.n_o, M))
    X0[:, warm] = Xs.cpu().numpy()[:, warm]
    res, hist, X = p.tl.solve_many(B, width=w, reduction=red, maxit=MAXIT, X0=X0)
    print(f"\nwarm columns {warm}: iterations {[r.iterations for r in res]}")
    _assert_equals_chunked(p, B, X0, w, red, res, hist, X)
    assert all(res[j].def0 <= 1e-9 * first[j].def0 for j in warm)                  # the warm columns did start from a converged x
    early = (0, 2, 6)
    Bs = B.copy()
    Bs[:, early] *= TINY
    res, hist, X = p.tl.solve_many(Bs, width=w, reduction=1e-10, maxit=MAXIT)
    its = [r.iterations for r in res]
    print(f"columns {early} scaled by 2^-83: iterations {its}, unscaled {[r.iterations for r in first]}")
    _assert_equals_chunked(p, Bs, None, w, 1e-10, res, hist, X)
    for j in range(M):
        if j in early:
            assert 0 < its[j] < first[j].iterations and res[j].reduction > 1e-10 and hist[its[j], j] < 1e-30, (j, its[j], first[j].iterations)
        else:
            assert its[j] == first[j].iterations, j


@pytest.mark.parametrize("name", ["golden", "shapes"])
def test_whole_block_refills_when_every_slot_hits_maxit(ddm, problems, name):
    """maxit = 3: every slot runs out of iterations in the same iteration, the whole block is stored and refilled at once; the columns
    are not converged and their x is written all the same."""
    p = problems(name)
    M, w = 9, 4
    res, hist, X = p.tl.solve_many(p.B[:, :M], width=w, reduction=1e-10, maxit=3)
    Xh = X.cpu().numpy()
    assert hist.shape == (4, M) and not np.isnan(hist).any()
    for j in range(M):
        r1, h1, x1 = p.single(j, maxit=3)
        assert res[j].iterations == r1.iterations == 3 and res[j].converged == r1.converged == 0, j
        assert (np.abs(hist[:, j] - h1) <= RTOL_HIST * h1 + ATOL_HIST * h1[0]).all(), j
        assert np.any(Xh[:, j]) and np.max(np.abs(Xh[:, j] - x1)) <= XTOL * np.max(np.abs(x1)), j
        assert res[j].reduction == hist[3, j] / hist[0, j]
    # maxit = 0: the initial defects and nothing else
    res, hist, X = p.tl.solve_many(p.B[:, :M], width=w, maxit=0)
    assert all(r.iterations == 0 and r.converged == 0 and r.def0 > 0 for r in res) and hist.shape == (1, M) and not X.any()


@pytest.mark.parametrize("name", ["golden", "shapes"])
def test_initial_defect_of_a_refilled_slot_touches_no_running_slot(ddm, problems, name):
    """A non-zero X0 in a column that enters a slot while the other slot is running: the masked B -= A x writes the refilled slot only.
    Every other column's history and x equal, bit for bit, those of the run in which that column starts from zero."""
    import torch
    p = problems(name)
    M, w, special = 6, 2, 3
    res0, hist0, X0run = p.tl.solve_many(p.B[:, :M], width=w, reduction=1e-10, maxit=MAXIT)
    X0 = np.zeros((p.tl.rl.n_o, M))
    X0[:, special] = p.X0[:, 0]
    res1, hist1, X1run = p.tl.solve_many(p.B[:, :M], width=w, reduction=1e-10, maxit=MAXIT, X0=X0)
    for j in range(M):
        if j == special:
            continue
        it = res0[j].iterations
        assert res1[j].iterations == it and res1[j].def0 == res0[j].def0, j
        assert np.array_equal(hist1[:it + 1, j], hist0[:it + 1, j]), j
        assert torch.equal(X1run[:, j], X0run[:, j]), j
    r1, h1, x1 = p.single(special, x0=X0[:, special], key="x0")
    assert res1[special].def0 != res0[special].def0
    _assert_column_matches_single(res1, hist1, X1run.cpu().numpy(), special, (r1, h1, x1), what=name)


# ---- 4. side effects ------------------------------------------------------------------------------------------------------------------
def test_side_effects_and_queue_order(ddm, problems):
    """B is not modified; a repeated call is bitwise identical; a permuted queue gives the permuted results, bitwise when every column
    has a slot of its own from the start (M <= w), within the block-against-single tolerance when the order decides which slot a column
    gets and when (M > w)."""
    import torch
    p = problems("golden")
    tl = p.tl
    for M, w in ((5, 8), (9, 4)):
        Bd = tl.to_device(p.B[:, :M]).contiguous()
        Bkeep = Bd.clone()
        X = torch.zeros_like(Bd)
        res, hist = ddm.cg_solve_queue(tl.ctx, tl.op, tl.prec, X, Bd, w, 1e-10, MAXIT, True)
        tl.ctx.sync()
        assert torch.equal(Bd, Bkeep)                                           # the right-hand sides are only read
        X2 = torch.zeros_like(Bd)
        res2, hist2 = ddm.cg_solve_queue(tl.ctx, tl.op, tl.prec, X2, Bd, w, 1e-10, MAXIT, True)
        assert torch.equal(X2, X) and np.array_equal(hist2, hist, equal_nan=True)
        assert [(r.iterations, r.converged, r.def0, r.reduction) for r in res2] == [(r.iterations, r.converged, r.def0, r.reduction) for r in res]
        perm = np.random.default_rng(3).permutation(M)
        resp, histp, Xp = tl.solve_many(p.B[:, :M][:, perm], width=w, reduction=1e-10, maxit=MAXIT)
        for c, j in enumerate(perm):
            assert resp[c].iterations == res[j].iterations and resp[c].converged == res[j].converged == 1, (M, w, c, j)
            it = res[j].iterations
            if M <= w:
                assert torch.equal(Xp[:, c], X[:, j]) and np.array_equal(histp[:it + 1, c], hist[:it + 1, j]), (M, w, c, j)
            else:
                h = hist[:it + 1, j]
                assert (np.abs(histp[:it + 1, c] - h) <= RTOL_HIST * h + ATOL_HIST * h[0]).all(), (M, w, c, j)
                assert float((Xp[:, c] - X[:, j]).abs().max()) <= XTOL * float(X[:, j].abs().max()), (M, w, c, j)


def _stored_before(its, w, bad):
    """the columns that have left their slot when column `bad` enters one: the refill protocol replayed on the iteration counts (its[j] > 0)"""
    slots, nxt, stored = {}, 0, []
    while True:
        for s in range(w):                       # free slots take the queue head in ascending slot order
            if s not in slots and nxt < len(its):
                if nxt == bad:
                    return sorted(stored)
                slots[s] = [nxt, its[nxt]]
                nxt += 1
        for s in sorted(slots):                  # one block iteration
            slots[s][1] -= 1
            if slots[s][1] == 0:
                stored.append(slots.pop(s)[0])


# ---- 5. status ------------------------------------------------------------------------------------------------------------------------
def test_local_status_word_and_nan_column(ddm, problems):
    """A local-solve status word that is already set makes the call fail like ddm_cg_solve_multi.  A NaN in a column that enters a slot
    late ends the call with DDM_ENUMERIC naming the column: the columns stored before it keep their results, X of every other column is
    as on entry."""
    import torch
    p = problems("golden")
    tl = p.tl
    lib, h = tl.ctx.lib, tl.ctx.h
    M, w = 6, 2
    res = (ddm.SolveResult * M)()
    Bd = tl.to_device(p.B[:, :M]).contiguous()
    X = torch.zeros_like(Bd)
    F = ctypes.c_void_p(tl.schwarz.local_solver())
    assert lib.ddm_ilu0_set_status(F, 1) == ddm.DDM_OK
    try:
        assert lib.ddm_cg_solve_queue(h, tl.op.h, tl.prec.h, M, w, X.data_ptr(), Bd.data_ptr(), 1e-10, MAXIT, None, res) == ddm.DDM_ENUMERIC
        Xs, Bs = X[:, :w].contiguous(), Bd[:, :w].contiguous()
        assert lib.ddm_cg_solve_multi(h, tl.op.h, tl.prec.h, w, Xs.data_ptr(), Bs.data_ptr(), 1e-10, MAXIT, None, res) == ddm.DDM_ENUMERIC
    finally:
        assert lib.ddm_ilu0_set_status(F, 0) == ddm.DDM_OK
    assert not X.any()
    # column 4 enters a slot when both slots have been refilled once and another column stops: which columns are stored by then follows
    # from the columns' iteration counts
    bad = 4
    expect = _stored_before([p.single(j)[0].iterations for j in range(M)], w, bad)
    assert 3 <= len(expect) <= 4 and set(expect) <= {0, 1, 2, 3}, expect
    Bn = Bd.clone()
    Bn[0, bad] = float("nan")
    rc = lib.ddm_cg_solve_queue(h, tl.op.h, tl.prec.h, M, w, X.data_ptr(), Bn.data_ptr(), 1e-10, MAXIT, None, res)
    msg = lib.ddm_last_error(h).decode()
    assert rc == ddm.DDM_ENUMERIC and "ddm_cg_solve_queue" in msg and f"column {bad}" in msg, msg
    Xh = X.cpu().numpy()
    stored = [j for j in range(M) if res[j].iterations > 0]
    assert stored == expect, (stored, expect)
    for j in range(M):
        if j in stored:
            r1, h1, x1 = p.single(j)
            assert res[j].iterations == r1.iterations and res[j].converged == 1, j
            assert np.max(np.abs(Xh[:, j] - x1)) <= XTOL * np.max(np.abs(x1)), j
        else:
            assert res[j].iterations == 0 and res[j].converged == 0 and not np.any(Xh[:, j]), j
    # the object is usable afterwards
    r, _, _ = tl.solve_many(p.B[:, :2], width=2, maxit=MAXIT)
    assert all(q.converged for q in r)
    tl.prec.check_status()


# ---- 6. another local solver ----------------------------------------------------------------------------------------------------------
def test_queue_with_direct_local_solver(ddm, problems):
    """The sparse direct local solver (`cholmod`) on the 12^3 problem: the multi-column direct solves see refilled slots.  Columns
    against single solves under the rule of test_cg_multi_with_direct_local_solver."""
    p = problems("golden", subdomain_solver="cholmod")
    M, w = 9, 4
    res, hist, X = p.tl.solve_many(p.B[:, :M], width=w, reduction=1e-10, maxit=200)
    Xh = X.cpu().numpy()
    print(f"\ncholmod: iterations {[r.iterations for r in res]}")
    for j in range(M):
        assert res[j].converged == 1
        _assert_column_matches_single(res, hist, Xh, j, p.single(j, maxit=200), rtol=1e-7, atol=1e-11, what="cholmod")
    p.tl.prec.check_status()
