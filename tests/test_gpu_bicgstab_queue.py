"""-m gpu: any number of right-hand sides through a BiCGSTAB block of fixed width (ddm_bicgstab_solve_queue,
TwoLevelSchwarz.solve_many(solver="bicgstabsolver")) against ddm_bicgstab_solve column by column, against itself (chunks without
refill, neighbours, scaling, order, repetition), the CPU oracle and the other exchange paths.

The two problems of tests/test_gpu_parity.py::test_bicgstab_history_matches_oracle: "poisson", (17, 16, 15) on 2 x 2 x 2 subdomains,
restricted Schwarz with ILU(0), multiplicative (a non-symmetric preconditioner); "dg", StructuredDG2D((24, 24), (2, 2)) with overlap 2,
standard Schwarz with the direct local solver, additive (a non-symmetric operator).  The right-hand sides are seeded consistent random
vectors, zero on the Dirichlet rows (the problem's own f = 1 vector is a genuine BiCGSTAB breakdown under the multiplicative
combination, see there).  Reduction 1e-9 and maxit 200 unless a test says otherwise.

Against a single solve or the oracle the band is the project's for BiCGSTAB histories, 1e-7 |r_k| + 1e-11 |r_0|,
x within 1e-7 of its largest entry, and equal half-step counts -- one apart only if the shorter run's last defect lies within that band
of def0 * reduction.  Against itself the comparison is bitwise: per column the block kernels' arithmetic depends on the block width
only, not on the slot or on the neighbouring columns, and a slot that is refilled starts from p = r exactly."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.mp_bicgstab_queue_worker import CONFIGS, decomposition
from tests.test_gpu_multi_rhs import _consistent_block
from tests.test_gpu_queue import _stored_before

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL_HIST, ATOL_HIST = 1e-7, 1e-11   # DESIGN.md section 6, the band of test_bicgstab_history_matches_oracle on these problems
XTOL = 1e-7
RED, MAXIT = 1e-9, 200
NCOLS = 40
NAMES = ("poisson", "dg")


class Problem:
    """One decomposition with its solver object, NCOLS fixed right-hand sides and, computed once each, single solves and queued runs"""

    def __init__(self, name):
        from dune_ddm_amd.solver import TwoLevelSchwarz
        self.name = name
        self.kw = dict(coarse="pou", **CONFIGS[name])
        self.dec = decomposition(name)
        self.tl = TwoLevelSchwarz(self.dec, **self.kw)
        self.free = self.tl.rl.cat_novlp([(sd.dirichlet_ovlp[:sd.n_o] == 0).astype(np.float64) for sd in self.dec.subs])
        self.B = _consistent_block(self.tl, self.dec, NCOLS, seed=31) * self.free[:, None]
        self.X0 = _consistent_block(self.tl, self.dec, 2, seed=77) * self.free[:, None]
        self._single, self._runs = {}, {}

    def single(self, j, maxit=MAXIT, x0=None, key=None):
        """(SolveResult, history, x as a host array) of ddm_bicgstab_solve on column j"""
        k = (j, maxit, key)
        assert (x0 is None) == (key is None)
        if k not in self._single:
            r, h, x = self.tl.solve(reduction=RED, maxit=maxit, b=self.B[:, j], x0=x0, solver="bicgstabsolver")
            self._single[k] = (r, np.asarray(h).copy(), x.cpu().numpy())
        return self._single[k]

    def many(self, B, w, maxit=MAXIT, X0=None):
        res, hist, X = self.tl.solve_many(B, width=w, reduction=RED, maxit=maxit, X0=X0, solver="bicgstabsolver")
        return res, hist, X

    def run(self, cols, w):
        """the queued run of the columns `cols` of B through w slots, kept"""
        k = (tuple(cols), w)
        if k not in self._runs:
            self._runs[k] = self.many(self.B[:, list(cols)], w)
        return self._runs[k]


@pytest.fixture(scope="module")
def problems(ddm):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Problem(name)
        return made[name]
    yield get
    for p in made.values():
        p.tl.ctx.close()


def _nh(hist, j):
    """entries of column j's history: its half steps + 1"""
    return int(np.sum(~np.isnan(hist[:, j])))


def _in_band(h, ref):
    k = min(len(h), len(ref))
    return bool((np.abs(h[:k] - ref[:k]) <= RTOL_HIST * ref[:k] + ATOL_HIST * ref[0]).all())


def _assert_matches(h, x, conv, ref_h, ref_x, what):
    """a queued column (history h, solution x) against another solve of it (ref_h, ref_x)"""
    print(f"{what}: half steps {len(h) - 1} against {len(ref_h) - 1}")
    assert conv == 1, what
    assert _in_band(h, ref_h), (what, float(np.max(np.abs(h[:min(len(h), len(ref_h))] - ref_h[:min(len(h), len(ref_h))]) / ref_h[:min(len(h), len(ref_h))])))
    if len(h) != len(ref_h):
        # one half step apart, and the shorter run's last defect within the band of the threshold: the other run saw it just above
        short = h if len(h) < len(ref_h) else ref_h
        assert abs(len(h) - len(ref_h)) == 1 and abs(short[-1] - RED * short[0]) <= RTOL_HIST * short[-1] + ATOL_HIST * short[0], (what, len(h), len(ref_h))
    assert np.max(np.abs(x - ref_x)) <= XTOL * np.max(np.abs(ref_x)), what


def _same(p, resa, hista, Xa, ja, resb, histb, Xb, jb, what):
    """column ja of one run and column jb of another are the same bits"""
    import torch
    n = _nh(hista, ja)
    assert n == _nh(histb, jb) and resa[ja].iterations == resb[jb].iterations == n // 2 and resa[ja].converged == resb[jb].converged, (what, n, _nh(histb, jb))
    assert np.array_equal(hista[:n, ja], histb[:n, jb]), (what, float(np.max(np.abs(hista[:n, ja] - histb[:n, jb]))))
    assert torch.equal(Xa[:, ja], Xb[:, jb]), (what, float((Xa[:, ja] - Xb[:, jb]).abs().max()))
    assert resa[ja].def0 == resb[jb].def0 and resa[ja].reduction == resb[jb].reduction, what


# ---- 3. columns against single solves -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("M, w", [(1, 1), (5, 3), (5, 8), (9, 4), (27, 13)])
def test_columns_match_single_solves(ddm, problems, name, M, w):
    """M < w, a ragged tail, refills, the widths 1, 3, 4, 8 and 13 (column groups 1, 2 + 1, 4, 8 and 8 + 4 + 1): every column behaves
    like ddm_bicgstab_solve on it."""
    p = problems(name)
    res, hist, X = p.run(range(M), w)
    Xh = X.cpu().numpy()
    assert len(res) == M and Xh.shape == (p.tl.rl.n_o, M) and hist.shape == (max(_nh(hist, j) for j in range(M)), M)
    for j in range(M):
        r1, h1, x1 = p.single(j)
        n = _nh(hist, j)
        assert r1.converged == 1 and not np.isnan(hist[:n, j]).any() and res[j].iterations == n // 2, (j, n, res[j].iterations)
        assert res[j].def0 == hist[0, j] and res[j].reduction == hist[n - 1, j] / hist[0, j] <= RED * (1 + 1e-15), j
        _assert_matches(hist[:n, j], Xh[:, j], res[j].converged, h1, x1, (name, M, w, j))
    p.tl.prec.check_status()


# ---- 4. bitwise self-consistency --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("M, w", [(16, 4), (40, 13)])
def test_columns_equal_the_chunks_without_refill_bitwise(ddm, problems, name, M, w):
    """every column equals, bit for bit, the same entry point called on the chunk of w columns that holds it: there no slot is refilled"""
    p = problems(name)
    res, hist, X = p.run(range(M), w)
    for c0 in range(0, M, w):
        cols = range(c0, min(c0 + w, M))
        rc, hc, Xc = p.run(cols, w)
        for k, j in enumerate(cols):
            _same(p, res, hist, X, j, rc, hc, Xc, k, (name, M, w, j))
    p.tl.prec.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_neighbours_scaling_order_and_repetition(ddm, problems, name):
    """A column alone through 4 slots equals itself among eight others; twice a column gives exactly twice x and history; a permuted
    queue gives the permuted results -- bitwise when every column has a slot of its own from the start (M <= w), within the band when
    the order decides which slot a column gets and when (M > w); a repeated call is identical; B is only read."""
    import torch
    p = problems(name)
    tl = p.tl
    res, hist, X = p.run(range(9), 4)
    for j in (0, 4, 8):                                                          # first fill, a refill, the last column
        ra, ha, Xa = p.run([j], 4)
        _same(p, res, hist, X, j, ra, ha, Xa, 0, (name, "alone", j))
    B2 = p.B[:, :6].copy()
    B2[:, 3] = 2.0 * B2[:, 1]
    B2[:, 5] = 0.25 * B2[:, 0]
    r2, h2, X2 = p.many(B2, 4)
    for j, i, f in ((3, 1, 2.0), (5, 0, 0.25)):
        n = _nh(h2, i)
        assert _nh(h2, j) == n and np.array_equal(h2[:n, j], f * h2[:n, i]) and torch.equal(X2[:, j], f * X2[:, i]), (name, j, i)
    for M, w in ((5, 8), (9, 4)):
        Bd = tl.to_device(p.B[:, :M]).contiguous()
        Bkeep = Bd.clone()
        Xa = torch.zeros_like(Bd)
        ra, ha = ddm.bicgstab_solve_queue(tl.ctx, tl.op, tl.prec, Xa, Bd, w, RED, MAXIT, True)
        tl.ctx.sync()
        assert torch.equal(Bd, Bkeep)                                           # the right-hand sides are only read
        Xb = torch.zeros_like(Bd)
        rb, hb = ddm.bicgstab_solve_queue(tl.ctx, tl.op, tl.prec, Xb, Bd, w, RED, MAXIT, True)
        assert torch.equal(Xb, Xa) and np.array_equal(hb, ha, equal_nan=True)
        assert [(r.iterations, r.converged, r.def0, r.reduction) for r in rb] == [(r.iterations, r.converged, r.def0, r.reduction) for r in ra]
        perm = np.random.default_rng(3).permutation(M)
        rp, hp, Xp = p.many(p.B[:, :M][:, perm], w)
        for c, j in enumerate(perm):
            if M <= w:
                _same(p, rp, hp, Xp, c, ra, ha, Xa, j, (name, "perm", M, w, c, j))
            else:
                _assert_matches(hp[:_nh(hp, c), c], Xp[:, c].cpu().numpy(), rp[c].converged, ha[:_nh(ha, j), j], Xa[:, j].cpu().numpy(), (name, "perm", M, w, c, j))


# ---- 5. half-step freezing ------------------------------------------------------------------------------------------------------------
def _residency(nhalf, w):
    """the protocol replayed on the half-step counts: per column (the iteration of the block loop it entered in, the one it left in)"""
    its = [(h + 1) // 2 for h in nhalf]
    slots, nxt, it, span = {}, 0, 0, {}
    while nxt < len(its) or slots:
        for s in range(w):
            if s not in slots and nxt < len(its):
                slots[s] = [nxt, its[nxt], it + 1]
                nxt += 1
        it += 1
        for s in sorted(slots):
            slots[s][1] -= 1
            if slots[s][1] == 0:
                j, _, first = slots.pop(s)
                span[j] = (first, it)
    return span


@pytest.mark.parametrize("name", NAMES)
def test_a_column_that_stops_after_a_first_half_step_sits_out_the_second(ddm, problems, name):
    """Columns that stop after an odd number of half steps while another slot goes through the second half step of the same iteration
    (found by replaying the protocol on the histories): x, history and counts equal, bit for bit, those of the column run alone."""
    p = problems(name)
    M, w = 16, 4
    res, hist, X = p.run(range(M), w)
    nhalf = [_nh(hist, j) - 1 for j in range(M)]
    span = _residency(nhalf, w)
    odd = [j for j in range(M) if nhalf[j] % 2 == 1 and
           any(d != j and span[d][0] <= span[j][1] and (span[d][1] > span[j][1] or (span[d][1] == span[j][1] and nhalf[d] % 2 == 0)) for d in range(M))]
    print(f"\n{name}: half steps {nhalf}, stopped after a first half step beside a running slot: {odd}")
    assert odd, nhalf
    for j in odd[:3]:
        ra, ha, Xa = p.run([j], w)
        _same(p, res, hist, X, j, ra, ha, Xa, 0, (name, "frozen", j))
        assert res[j].iterations == (_nh(hist, j) - 1 + 1) // 2 and res[j].converged == 1


# ---- 6. refill hygiene ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_zero_columns_warm_start_and_maxit(ddm, problems, name):
    """Zero columns (two at the head, two in a row in the middle, one at the end) need no iteration and their slot is refilled again at
    the same boundary; a non-zero X0 in a column that enters while the other slot runs touches nothing but its own slot; maxit = 2 stores
    and refills the whole block at once; maxit = 0 leaves X."""
    import torch
    p = problems(name)
    n_o = p.tl.rl.n_o
    order = [None, None, 0, 1, None, None, 2, 3, None]           # None: a zero column, j: column j of the problem
    B = np.stack([np.zeros(n_o) if j is None else p.B[:, j] for j in order], axis=1)
    res, hist, X = p.many(B, 3)
    rr, hr, Xr = p.run(range(4), 3)
    for c, j in enumerate(order):
        if j is None:
            assert res[c].iterations == 0 and res[c].converged == 1 and res[c].def0 == 0.0 and _nh(hist, c) == 1 and hist[0, c] == 0.0, c
            assert not bool(X[:, c].any()), c
        else:
            # the zero columns take no iteration, so the others meet the same neighbours at the same time as in the run without them
            _same(p, res, hist, X, c, rr, hr, Xr, j, (name, "zeros", c))
    res, hist, X = p.many(np.zeros((n_o, 5)), 2)
    assert all(r.iterations == 0 and r.converged == 1 for r in res) and hist.shape == (1, 5) and not bool(X.any())

    M, w, special = 6, 2, 3
    res0, hist0, Xrun0 = p.run(range(M), w)
    X0 = np.zeros((n_o, M))
    X0[:, special] = p.X0[:, 0]
    res1, hist1, Xrun1 = p.many(p.B[:, :M], w, X0=X0)
    n1 = _nh(hist1, special)
    assert res1[special].def0 != res0[special].def0
    r1, h1, x1 = p.single(special, x0=X0[:, special], key="x0")
    _assert_matches(hist1[:n1, special], Xrun1[:, special].cpu().numpy(), res1[special].converged, h1, x1, (name, "x0"))
    for j in range(M):                                           # every other column: the same bits, whenever it entered and beside whom
        if j != special:
            _same(p, res1, hist1, Xrun1, j, res0, hist0, Xrun0, j, (name, "beside x0", j))

    M, w = 9, 4
    res, hist, X = p.many(p.B[:, :M], w, maxit=2)
    Xh = X.cpu().numpy()
    assert hist.shape == (5, M) and not np.isnan(hist).any()
    for j in range(M):
        r1, h1, x1 = p.single(j, maxit=2)
        assert res[j].iterations == r1.iterations == 2 and res[j].converged == r1.converged == 0 and _nh(hist, j) == len(h1) == 5, j
        assert _in_band(hist[:, j], h1) and np.any(Xh[:, j]) and np.max(np.abs(Xh[:, j] - x1)) <= XTOL * np.max(np.abs(x1)), j
        assert res[j].reduction == hist[4, j] / hist[0, j]
    Xs = p.tl.to_device(np.ascontiguousarray(np.tile(p.X0[:, :1], (1, M))))
    res, hist, X = p.many(p.B[:, :M], w, maxit=0, X0=Xs)
    assert all(r.iterations == 0 and r.converged == 0 and r.def0 > 0 for r in res) and hist.shape == (1, M) and torch.equal(X, Xs)
    p.tl.prec.check_status()


# ---- 7. oracle --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_column0_matches_oracle(ddm, problems, name):
    from tests.oracle_bridge import oracle_solve
    p = problems(name)
    res, hist, X = p.run(range(5), 8)
    off = 0
    for sd in p.dec.subs:                                        # the oracle takes its right-hand side from the decomposition
        sd.b = p.B[off:off + sd.n_o, 0].copy()
        off += sd.n_o
    assert off == p.tl.rl.n_o
    it, conv, hist_o, xo = oracle_solve(p.dec, reduction=RED, maxit=MAXIT, solver="bicgstabsolver", coarse="pou", schwarz_type=p.kw["schwarz_type"],
                                        mode=p.kw["mode"], local_solver="ilu0" if p.kw["subdomain_solver"] == "ilu0" else "direct")
    assert conv
    n = _nh(hist, 0)
    _assert_matches(hist[:n, 0], X[:, 0].cpu().numpy(), res[0].converged, np.array(hist_o), np.concatenate(xo), (name, "oracle"))
    assert abs(res[0].iterations - it) <= abs(n - len(hist_o))


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_status_word_and_nan_column_are_refused(ddm, problems):
    """A local-solve status word that is already set fails the call before any launch.  A NaN in column 5 of 9 ends the call with
    DDM_ENUMERIC naming the column and the function: the columns that left their slots before column 5 entered keep correct results,
    X of the others is as on entry.  The context solves normally afterwards."""
    import torch
    p = problems("poisson")
    tl = p.tl
    lib, h = tl.ctx.lib, tl.ctx.h
    M, w, bad = 9, 4, 5
    res = (ddm.SolveResult * M)()
    nh = (ctypes.c_int32 * M)()
    Bd = tl.to_device(p.B[:, :M]).contiguous()
    X = torch.zeros_like(Bd)
    F = ctypes.c_void_p(tl.schwarz.local_solver())
    assert lib.ddm_ilu0_set_status(F, 1) == ddm.DDM_OK
    try:
        assert lib.ddm_bicgstab_solve_queue(h, tl.op.h, tl.prec.h, M, w, X.data_ptr(), Bd.data_ptr(), RED, MAXIT, None, nh, res) == ddm.DDM_ENUMERIC
    finally:
        assert lib.ddm_ilu0_set_status(F, 0) == ddm.DDM_OK
    tl.ctx.sync()
    assert not bool(X.any())
    r0, h0, X0run = p.run(range(M), w)
    its = [r.iterations for r in r0]
    expect = _stored_before(its, w, bad)
    assert expect and set(expect) <= set(range(bad)), (its, expect)
    Bn = Bd.clone()
    Bn[3, bad] = float("nan")
    rc = lib.ddm_bicgstab_solve_queue(h, tl.op.h, tl.prec.h, M, w, X.data_ptr(), Bn.data_ptr(), RED, MAXIT, None, nh, res)
    msg = lib.ddm_last_error(h).decode()
    tl.ctx.sync()
    assert rc == ddm.DDM_ENUMERIC and "ddm_bicgstab_solve_queue" in msg and f"column {bad}" in msg, msg
    stored = [j for j in range(M) if res[j].iterations > 0]
    assert stored == expect, (stored, expect, its)
    for j in range(M):
        if j in stored:
            assert res[j].iterations == its[j] and res[j].converged == 1 and nh[j] == _nh(h0, j) and torch.equal(X[:, j], X0run[:, j]), j
        else:
            assert res[j].iterations == 0 and res[j].converged == 0 and nh[j] == 0 and not bool(X[:, j].any()), j
    r, _, Xn = p.many(p.B[:, :M], w)
    assert all(q.converged for q in r) and torch.equal(Xn, X0run)
    tl.prec.check_status()


# ---- 9. exchange paths --------------------------------------------------------------------------------------------------------------------
def test_rccl_self_test_is_bit_identical(ddm, problems):
    """The in-library exchange on one GPU (communicator of size 1 in self-test mode: every halo block and every all-reduce of the w or
    2 w sums of a half step goes through RCCL) against the plain single-rank run."""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    p = problems("poisson")
    M, w = 6, 4
    res0, hist0, X0 = p.run(range(M), w)
    os.environ["DDM_RCCL_SELFTEST"] = "1"
    try:
        tl = TwoLevelSchwarz(p.dec, **p.kw)
    finally:
        del os.environ["DDM_RCCL_SELFTEST"]
    assert tl.exchange == "rccl"
    res, hist, X = tl.solve_many(p.B[:, :M], width=w, reduction=RED, maxit=MAXIT, solver="bicgstabsolver")
    tl.prec.check_status()
    assert [r.iterations for r in res] == [r.iterations for r in res0] and all(r.converged for r in res)
    assert np.array_equal(hist, hist0, equal_nan=True) and np.array_equal(X.cpu().numpy(), X0.cpu().numpy())
    tl.ctx.close()


def test_two_rank_queue_matches_single_rank():
    """two ranks over gloo sharing the GPU (callback exchange column by column) against the one-rank run: the same half-step counts,
    x within 1e-7"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29597", os.path.join(ROOT, "tests", "mp_bicgstab_queue_worker.py"), "ranks"]
    q = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert q.returncode == 0 and "BICGSTAB_QUEUE_RANKS_OK 2" in q.stdout, q.stdout[-2000:] + q.stderr[-4000:]
