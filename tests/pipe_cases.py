"""Matrices and host analysis shared by tests/test_pipe_cases_reference.py (CPU) and tests/test_gpu_pipe_shapes.py (GPU): the ILU(0)
solve of the pipe engine (csrc/trsv_pipe.hpp) at the shapes its schedule builder (csrc/trsv_pipe_host.hpp) and its kernel branch on.

`case(name)` builds a matrix on first use; EXPECT[name] is the engine it must end on ("pipe", or "xcd2" with the builder's reason in
DECLINES).  `schedule(name)` runs the HOST BUILDER ITSELF (tests/cpp/pipe_host_test.cpp: pipe_test_case) with the device's default
options -- delta 24, max_span 256, vote 1, pack_steps 64 -- on the oracle's factor and returns what it built: the builder's own
statistics, per-step tile widths, operand words by entry slot and kind, and the CPU emulation of the kernel's data flow.
PRECONDITIONS[name] are the branch conditions a case exists for, as predicates on that; MUTATIONS[name] the (sweep, slot class,
operand kind) whose loss the bit comparison on the device must notice.  Nothing here needs a GPU."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import scipy.sparse as sp

from tests import trsv_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
DELTA, MAX_SPAN, VOTE, PACK_STEPS = 24, 256, 1, 64        # pipe::Options defaults = what build_pipe_schedule (csrc/engine_pipe.hpp) uses
MIN_W, MAX_W, RING, MAXPROD, LANES = 14, 26, 16, 112, 64  # csrc/trsv_pipe_host.hpp
MAX_N, MAX_ENTRIES = 60000, 1500000                       # caps on every case: rows, factor entries
WIDE = "triangular rows wider than the tile format"
PRODUCERS = "a task has too many producer tasks"
STEPS16 = "a task has more steps than the 16-bit progress requirements hold"
L, U = 0, 1
CLASS_NAMES = ("0..13", "14..19", "20..25")
RING_OP, SELF, REMOTE, PAD = 0, 1, 2, 3
KIND_NAMES = ("ring", "self-global", "remote", "padding")


# ---- generators -----------------------------------------------------------------------------------------------------------------
def band(n, offsets, seed):
    return tc.band(n, list(offsets), seed)


def band2(n, lower, upper, seed):
    """lower entries at the offsets `lower`, upper entries at the offsets `upper`: a non-symmetric pattern"""
    P = sp.diags([np.ones(n - k) for k in lower] + [np.ones(n - k) for k in upper], [-k for k in lower] + list(upper), shape=(n, n), format="csr")
    return tc.randomise(P, seed)


def _from_lower(n, ri, cj, seed):
    Lp = sp.csr_matrix((np.ones(len(ri)), (np.asarray(ri), np.asarray(cj))), shape=(n, n))
    return tc.randomise(Lp + Lp.T, seed)


def mixed(n, seed, widths=(3, 3, 18, 18, 26, 26, 3, 26, 18), run=40, first=40):
    """row i has lower entries at the offsets first .. first + w - 1, w = widths[(i // run) % len(widths)]: steps of all three tile
    sizes follow each other inside one task; the upper pattern is the transpose.  (The cycle 3 3 18 18 26 26 3 26 18 holds every
    ordered pair of width classes; with 3 18 26 alone the L sweep only has three of them.)"""
    ri, cj = [], []
    for i in range(n):
        w = widths[(i // run) % len(widths)]
        for k in range(first, first + w):
            if i - k >= 0:
                ri.append(i)
                cj.append(i - k)
    return _from_lower(n, ri, cj, seed)


def snake(nx, ny, seed):
    """nine-point stencil on an nx x ny grid numbered boustrophedon: every row follows its predecessor, operands up to 2 nx - 1 steps back"""
    idx = lambda ix, iy: iy * nx + (ix if iy % 2 == 0 else nx - 1 - ix)
    ri, cj = [], []
    for iy in range(ny):
        for ix in range(nx):
            a = idx(ix, iy)
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    jx, jy = ix + dx, iy + dy
                    if 0 <= jx < nx and 0 <= jy < ny and idx(jx, jy) < a:
                        ri.append(a)
                        cj.append(idx(jx, jy))
    return _from_lower(nx * ny, ri, cj, seed)


def fanin(T, seed, fan=25):
    """Row groups A (64 T rows), B (64 T rows, row i chained to A row i), E (64 free rows), C (64 rows): C row r has `fan` lower entries
    in B at ((fan r + j) 64 + r) mod 64 T and, as its last entry, E row r -- a one-step task whose rows read from every one of the T
    tasks of A-B chains.  The upper pattern is the transpose."""
    m = 64 * T
    ri, cj = list(range(m, 2 * m)), list(range(m))
    for r in range(64):
        for j in range(fan):
            ri.append(2 * m + 64 + r)
            cj.append(m + ((fan * r + j) * 64 + r) % m)
        ri.append(2 * m + 64 + r)
        cj.append(2 * m + r)
    return _from_lower(2 * m + 128, ri, cj, seed)


def stagger(P, base, step, clen, seed):
    """P bidiagonal producer chains of base + step j rows, P free rows, P consumer chains of clen rows: the first row of consumer chain j
    depends on the end of producer j and, as its last entry, on free row j.  The upper pattern is the transpose."""
    lens = [base + step * j for j in range(P)]
    start = np.concatenate([[0], np.cumsum(lens)])
    free0 = int(start[-1])
    cons0 = free0 + P
    ri, cj = [], []
    for j in range(P):
        for i in range(int(start[j]) + 1, int(start[j + 1])):
            ri.append(i)
            cj.append(i - 1)
        c0 = cons0 + j * clen
        ri += [c0, c0]
        cj += [int(start[j + 1]) - 1, free0 + j]
        for i in range(c0 + 1, c0 + clen):
            ri.append(i)
            cj.append(i - 1)
    return _from_lower(cons0 + P * clen, ri, cj, seed)


def diagonal(n, seed):
    return sp.diags(1.0 + np.random.default_rng(seed).random(n), format="csr")


def _one(M):
    return M, np.array([0, M.shape[0]], dtype=np.int64)


def _diag_blocks(mats):
    M = sp.block_diag(mats, format="csr")
    M.sort_indices()
    return M, np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)


# blocks every one of which the pipe builder takes (it sizes W over the whole matrix and declines all of it for one wide block)
_POOL = (lambda s: band(300, range(40, 43), s),
         lambda s: band(300, range(40, 55), s),                 # w = 15
         lambda s: band(300, range(40, 60), s),                 # w = 20
         lambda s: fanin(3, s),                                  # remote wide halves, tasks of 2 and 3 steps
         lambda s: band(300, range(40, 61), s),                 # w = 21
         lambda s: band(300, range(40, 66), s),                 # w = 26
         lambda s: band(300, range(40, 54), s),                 # w = 14
         lambda s: tc.layered([150] * 4, 26, s),                # several tasks, remote operands in every slot class
         lambda s: band(300, range(40, 49), s),                 # w = 9
         lambda s: diagonal(1, s),                               # the one-row block
         lambda s: band(400, (1, 16), s),                       # ring age: self-global operands
         lambda s: band(700, (65, 66), s),                      # a dissolved component: tasks of <= 2 steps, every operand remote
         lambda s: diagonal(100, s))                             # a packed task
MIX_SEEDS = {1: 5, 7: 1, 8: 2, 9: 3, 17: 4}


def _mix(count):
    seed = MIX_SEEDS[count]
    return _diag_blocks([_POOL[(b * 4 + seed) % len(_POOL)](100 * seed + b) for b in range(count)])


WIDTHS = (13, 14, 15, 20, 21, 26)
_BUILDERS = {f"w{w}": (lambda w=w: _one(band(3000, range(40, 40 + w), w))) for w in WIDTHS}
_BUILDERS.update({
    "Lwide": lambda: _one(band2(3000, range(40, 60), (1, 50), 31)),
    "Uwide": lambda: _one(band2(3000, (1, 50), range(40, 66), 32)),
    "mixed": lambda: _one(mixed(3000, 33)),
    "age15": lambda: _one(band(400, (1, 15), 34)),
    "age16": lambda: _one(band(400, (1, 16), 35)),
    "age17": lambda: _one(band(400, (1, 17), 36)),
    "snake": lambda: _one(snake(70, 70, 37)),
    "fanin111": lambda: _one(fanin(111, 38)),
    "fanin112": lambda: _one(fanin(112, 39)),
    "stagger": lambda: _one(stagger(140, 257, 2, 2, 40)),
    "chains64": lambda: _one(band(6000, (64, 65), 41)),
    "chains65": lambda: _one(band(6000, (65, 66), 42)),
    "packed": lambda: (diagonal(4397, 43), np.array([0, 1, 100, 4397], dtype=np.int64)),
    "layered26": lambda: _one(tc.layered([5000] * 4, 26, 44)),
    "mix1": lambda: _mix(1),
    "mix7": lambda: _mix(7),
    "mix8": lambda: _mix(8),
    "mix9": lambda: _mix(9),
    "mix17": lambda: _mix(17),
    # declined: the factor must end on xcd2
    "w27": lambda: _one(band(3000, range(40, 67), 27)),
    "fanin120": lambda: _one(fanin(120, 45)),
    "tc_layers": lambda: (tc.case("layers").M, tc.case("layers").block_ptr),
    "tc_wide": lambda: (tc.case("wide").M, tc.case("wide").block_ptr),
    "tc_elasticity": lambda: (tc.case("elasticity").M, tc.case("elasticity").block_ptr),
})
NAMES = tuple(_BUILDERS)
DECLINES = {"w27": WIDE, "fanin120": PRODUCERS, "tc_layers": WIDE, "tc_wide": WIDE, "tc_elasticity": WIDE}
EXPECT = {name: ("xcd2" if name in DECLINES else "pipe") for name in NAMES}
ACCEPTED = tuple(n for n in NAMES if n not in DECLINES)
CHAINED = ("mix9", "mix17")                                  # the back-to-back runs of the GPU test
# whether the pipe builder takes the cases of tests/trsv_cases.py (default options; asserted by test_pipe_cases_reference.py):
# what test_gpu_trsv_shapes.py expects of F.engine() in pipe mode
TRSV_CASES_ENGINE = {"band17": "pipe", "layers": "xcd2", "wide": "xcd2", "chain600": "pipe", "elasticity": "xcd2", "dg": "pipe",
                     "blocks3": "pipe", "blocks9": "xcd2", "blocks17": "xcd2"}


class Widths:
    """widest lower / upper row: all trsv_cases.bound needs"""

    def __init__(self, M):
        rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
        self.wL = int(np.bincount(rows[M.indices < rows], minlength=M.shape[0]).max())
        self.wU = int(np.bincount(rows[M.indices > rows], minlength=M.shape[0]).max())


class Case:
    def __init__(self, name):
        self.name = name
        self.M, self.block_ptr = _BUILDERS[name]()
        self.M = sp.csr_matrix(self.M)
        self.M.sort_indices()
        self.block_ptr = np.asarray(self.block_ptr, dtype=np.int64)
        self.n = self.M.shape[0]
        self.nblocks = len(self.block_ptr) - 1
        self.widths = Widths(self.M)
        self.C = tc.bound(self.widths)                          # the bound of check (a), as in tests/trsv_cases.py
        self.entries = self.M.nnz - self.n


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def oracle_factor(M):
    """(factor object, lu, diag) of the oracle's sequential ILU(0) of the whole block-diagonal matrix (no entry couples two blocks)"""
    from oracle import apply_oracle as ao
    f = ao.Ilu0(ao.Csr(M))
    return f, f.lu, f.diag


def oracle_solve(f, d):
    x = np.zeros(len(d))
    f.apply(x, np.ascontiguousarray(d, dtype=np.float64))
    return x


# ---- the host builder -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def harness():
    subprocess.check_call(["make", "-C", CPP, "libpipe_host_test.so"], stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(CPP, "libpipe_host_test.so"))
    lib.pipe_test_case.restype = ctypes.c_int
    return lib


_STATS = ("ntasksL", "ntasksU", "nstepsL", "nstepsU", "rows", "entries", "local", "self_global", "remote", "max_prod", "max_steps",
          "regrouped", "nchainsL", "nchainsU", "W", "tile_bytes", "stream_bytes", "nposL", "nposU", "ntasks")


class Built:
    """what pipe::build made of a factor, and the emulated solve"""

    def __init__(self, rc, err, x, stats, widths):
        self.rc, self.err, self.x = rc, err, x
        self.st = dict(zip(_STATS, stats[:20].tolist()))
        self.steps = stats[20:26].reshape(2, 3)                 # [sweep][width class]: steps of W <= 14, 15..20, 21..26
        self.ops = stats[26:50].reshape(2, 3, 4)                # [sweep][slot class][kind]: operand words
        self.min_steps, self.max_steps, self.packed, self.lane_reuse = (int(v) for v in stats[50:54])
        self.short = {k + 1: int(stats[54 + k]) for k in range(3)}  # tasks of 1, 2, 3 steps
        self.mutation = dict(zip(("row", "task", "step", "lane", "slot", "kind"), stats[58:64].tolist()))
        self.tasks = []                                         # (sweep, group, nprod, widths of the steps)
        k = 0
        while rc != 1 and k < len(widths):
            sweep, group, nsteps, nprod = widths[k:k + 4].tolist()
            self.tasks.append((sweep, group, nprod, widths[k + 4:k + 4 + nsteps]))
            k += 4 + nsteps

    def class_pairs(self):
        """ordered pairs (class of step t, class of step t + 1) that occur inside some task"""
        cls = lambda w: np.where(w <= MIN_W, 0, np.where(w <= MIN_W + 6, 1, 2))
        out = set()
        for _, _, _, w in self.tasks:
            c = cls(np.asarray(w))
            out |= set(zip(c[:-1].tolist(), c[1:].tolist()))
        return out

    def figures(self):
        s = self.st
        ops = "; ".join(f"{'LU'[sw]} {CLASS_NAMES[k]}: " + "/".join(str(int(v)) for v in self.ops[sw, k]) for sw in (L, U) for k in range(3) if self.ops[sw, k, :3].any())
        return (f"tasks {s['ntasksL']}+{s['ntasksU']}, chains {s['nchainsL']}+{s['nchainsU']}, steps {s['nstepsL']}+{s['nstepsU']} "
                f"(per task {self.min_steps}..{self.max_steps}; tasks of 1/2/3 steps {self.short[1]}/{self.short[2]}/{self.short[3]}; packed {self.packed}), "
                f"W {s['W']}, steps by width <=14/15-20/21-26: L {'/'.join(map(str, self.steps[L]))} U {'/'.join(map(str, self.steps[U]))}, "
                f"operands ring {s['local']} self-global {s['self_global']} remote {s['remote']}, max producers {s['max_prod']}, "
                f"regrouped {s['regrouped']}, lane re-uses {self.lane_reuse}; words ring/self/remote/pad by slots: {ops}")


def run_builder(M, block_ptr, lu, diag, d, mutate=None):
    """pipe::build with the device's default options and pipe::emulate into a NaN-filled x; mutate = (sweep, slot class, kind or -1)"""
    lib = harness()
    n = M.shape[0]
    rp = np.asarray(M.indptr, dtype=np.int64)
    ci = np.asarray(M.indices, dtype=np.int32)
    bp = np.asarray(block_ptr, dtype=np.int64)
    lu = np.ascontiguousarray(lu, dtype=np.float64)
    diag = np.ascontiguousarray(diag, dtype=np.int64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    x = np.full(n, np.nan)
    stats = np.zeros(64, dtype=np.int64)
    cap = 10 * n + 64                                           # at most 2 n tasks of 4 words and 2 n steps
    widths = np.zeros(cap, dtype=np.int32)
    mut = np.asarray(mutate, dtype=np.int64) if mutate is not None else None
    err = ctypes.create_string_buffer(256)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    rc = lib.pipe_test_case(ctypes.c_int64(n), p(rp), p(ci), p(lu), p(diag), ctypes.c_int(len(bp) - 1), p(bp), ctypes.c_int(DELTA),
                            ctypes.c_int(MAX_SPAN), ctypes.c_int(VOTE), ctypes.c_int(PACK_STEPS), p(d), p(x), p(stats), p(widths),
                            ctypes.c_int64(cap), p(mut), err, 256)
    assert stats[57] <= cap
    return Built(rc, err.value.decode(), x, stats, widths[:int(stats[57])])


class Ref:
    """per case, computed once and never changed: the oracle's factor, two right-hand sides and its solves of them"""

    def __init__(self, name):
        self.c = c = case(name)
        rng = np.random.default_rng(43)
        self.d = [rng.standard_normal(c.n), rng.standard_normal(c.n)]
        self.f, self.lu, self.diag = oracle_factor(c.M)
        self.x = [oracle_solve(self.f, d) for d in self.d]
        for a in (self.d[0], self.d[1], self.lu, self.x[0], self.x[1]):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def ref(name):
    return Ref(name)


@functools.lru_cache(maxsize=None)
def schedule(name):
    r = ref(name)
    return run_builder(r.c.M, r.c.block_ptr, r.lu, r.diag, r.d[0])


def dependants(M, row, sweep):
    """rows whose result of the solve depends on the result of `row` in the sweep (L: forward, then everything the U sweep makes of
    those; U: backward), the row itself included"""
    M = sp.csr_matrix(M)
    n = M.shape[0]
    rp, ci = M.indptr, M.indices
    hit = np.zeros(n, dtype=bool)
    hit[row] = True
    if sweep == L:
        for i in range(row + 1, n):
            c = ci[rp[i]:rp[i + 1]]
            hit[i] = hit[c[c < i]].any()
    for i in range(n - 1 if sweep == L else row - 1, -1, -1):
        if not hit[i]:
            c = ci[rp[i]:rp[i + 1]]
            hit[i] = hit[c[c > i]].any()
    return hit


# ---- the branch conditions --------------------------------------------------------------------------------------------------------
def _st(**want):
    return lambda c, s: all(s.st[k] == v for k, v in want.items())


def _width_edge(w):
    W = max(w, MIN_W)
    kl = 0 if W <= MIN_W else (1 if W <= MIN_W + 6 else 2)
    return [
        (f"accepted, geo.W = {W}, one task per sweep, 40 chains, 75 steps", _st(W=W, ntasksL=1, ntasksU=1, nchainsL=40, nchainsU=40, nstepsL=75, nstepsU=75)),
        ("every operand is a ring operand", lambda c, s: s.st["local"] == s.st["entries"] == c.entries and s.st["remote"] == s.st["self_global"] == 0),
        (f"both sweeps have steps of width class {kl} and none wider", lambda c, s: all(s.steps[sw, kl] > 0 and not s.steps[sw, kl + 1:].any() for sw in (L, U))),
        (f"the widest step of either sweep has exactly {W} entries", lambda c, s: all(max(int(x.max()) for t, _, _, x in s.tasks if t == sw) == W for sw in (L, U))),
    ]


def _mix_pre(count):
    return [
        (f"accepted, {count} blocks", lambda c, s: s.rc == 0 and c.nblocks == count and len({g for _, g, _, _ in s.tasks}) == count),
        ("side of the nb < 8 switch (fewer: write-through hand-overs; 8 or more: XCD-local, XCD 0 owns two or three groups from 9 on)",
         lambda c, s: (c.nblocks < 8) == (count < 8)),
        ("uneven block sizes (one block: nothing to compare)", lambda c, s: count == 1 or len(set(np.diff(c.block_ptr).tolist())) >= 3),
    ] + ([("wide steps of both halves, self-global and remote operands, a one-row block, tasks of 1, 2 and 3 steps, a packed task",
           lambda c, s: s.st["W"] == MAX_W and all(s.steps[sw, 1] and s.steps[sw, 2] for sw in (L, U)) and s.st["self_global"] > 0 and s.st["remote"] > 0 and
           int(np.diff(c.block_ptr).min()) == 1 and all(s.short[k] > 0 for k in (1, 2, 3)) and s.packed > 0)] if count >= 9 else [])


PRECONDITIONS = {f"w{w}": _width_edge(w) for w in WIDTHS}
PRECONDITIONS.update({
    "Lwide": [
        ("L: one task of 40 chains, W = 20", lambda c, s: s.st["ntasksL"] == 1 and s.st["nchainsL"] == 40 and s.st["W"] == 20 and s.steps[L, 1] > 0),
        ("U: a single chain of 3000 steps with 2950 self-global operands", _st(nchainsU=1, nstepsU=3000, self_global=2950)),
        ("the U sweep has no step wider than 14", lambda c, s: not s.steps[U, 1:].any()),
    ],
    "Uwide": [
        ("L: W = 2, 3000 steps", lambda c, s: s.st["nstepsL"] == 3000 and c.widths.wL == 2),
        ("U: W = 26, 74 of its 75 steps wide", lambda c, s: s.st["W"] == 26 and s.st["nstepsU"] == 75 and int(s.steps[U, 1:].sum()) == 74 and s.steps[U, 2] > 0),
        ("the L sweep has no step wider than 14", lambda c, s: not s.steps[L, 1:].any()),
    ],
    "mixed": [
        ("one task per sweep, 75 steps", _st(ntasksL=1, ntasksU=1, nstepsL=75, nstepsU=75)),
        ("49 of the 75 L steps and 66 of the 75 U steps are wide, both halves in both sweeps",
         lambda c, s: s.steps[L].tolist() == [26, 25, 24] and s.steps[U].tolist() == [9, 26, 40]),
        ("all nine ordered pairs of consecutive width classes occur inside a task", lambda c, s: len(s.class_pairs()) == 9),
    ],
    "age15": [("one chain, 400 steps, 1568 ring operands, none self-global", _st(nchainsL=1, nstepsL=400, nchainsU=1, local=1568, self_global=0, remote=0))],
    "age16": [("one chain, 400 steps, 798 ring and 768 self-global operands", _st(nchainsL=1, nstepsL=400, nchainsU=1, local=798, self_global=768, remote=0))],
    "age17": [("one chain, 400 steps, 798 ring and 766 self-global operands", _st(nchainsL=1, nstepsL=400, nchainsU=1, local=798, self_global=766, remote=0))],
    "snake": [("one task of 4900 steps per sweep, 25 668 self-global operands", _st(ntasksL=1, ntasksU=1, nstepsL=4900, nstepsU=4900, self_global=25668, remote=0))],
    "fanin111": [("accepted with max_prod = 111", _st(max_prod=111, W=26))],
    "fanin112": [
        (f"accepted with max_prod = MAXPROD = {MAXPROD}: the last 16-bit half of header word HDR_REQ0 + 55", _st(max_prod=MAXPROD, W=26, regrouped=0)),
        ("3250 remote operands", _st(remote=3250)),
        ("tasks of at most 3 steps, some of 2 and some of 3; a lane re-used", lambda c, s: s.max_steps == 3 and s.short[2] > 0 and s.short[3] > 0 and s.lane_reuse > 0),
        ("L: entry slots 14..19 and 20..25 each hold remote operands, 20..25 ring operands beside them (14..19 hold ring operands in w15 .. w26 and layered26)",
         lambda c, s: s.ops[L, 1, REMOTE] > 0 and s.ops[L, 2, REMOTE] > 0 and s.ops[L, 2, RING_OP] > 0),
    ],
    "stagger": [
        ("n = 55 860, accepted after one halving of max_span", lambda c, s: c.n == 55860 and s.st["regrouped"] == 1),
        ("max_prod = 65, max_steps = 535", _st(max_prod=65, max_steps=535)),
        ("lanes are re-used", lambda c, s: s.lane_reuse > 0),
    ],
    "chains64": [("64 mutually dependent chains (exactly a wave) stay one task per sweep", _st(nchainsL=64, nchainsU=64, ntasksL=1, ntasksU=1, remote=0))],
    "chains65": [
        ("65 mutually dependent chains are dissolved into single rows", lambda c, s: s.st["nchainsL"] == s.st["nchainsU"] == c.n == 6000),
        ("93 + 93 tasks of at most 2 steps, every operand remote", lambda c, s: s.st["ntasksL"] == s.st["ntasksU"] == 93 and s.st["max_steps"] == 2 and
         s.st["remote"] == s.st["entries"] and s.short[2] > 0),
    ],
    "packed": [
        ("blocks of 1, 99 and 4297 rows, packed tasks only", lambda c, s: np.diff(c.block_ptr).tolist() == [1, 99, 4297] and s.packed == s.st["ntasks"] and s.st["entries"] == 0),
        ("a pack of 64 steps, a partial one, a task of one step", lambda c, s: s.max_steps == PACK_STEPS and s.min_steps == 1 and s.short[1] == 2 and
         sorted(len(w) for sw, _, _, w in s.tasks if sw == L) == [1, 2, 4, 64]),
    ],
    "layered26": [
        ("W = 26, 154 122 remote operands", _st(W=26, remote=154122)),
        ("entry slots 14..19 and 20..25 each hold remote and ring operands in some sweep",
         lambda c, s: any(all(s.ops[sw, k, RING_OP] > 0 and s.ops[sw, k, REMOTE] > 0 for k in (1, 2)) for sw in (L, U))),
    ],
    "w27": [("n = 3000, 27 entries per triangular row", lambda c, s: c.widths.wL == c.widths.wU == MAX_W + 1)],
    "fanin120": [("rows of at most 26 entries: declined for its producers, not its width", lambda c, s: max(c.widths.wL, c.widths.wU) == MAX_W)],
    "tc_layers": [("wider than the tile format", lambda c, s: max(c.widths.wL, c.widths.wU) > MAX_W)],
    "tc_wide": [("wider than the tile format", lambda c, s: max(c.widths.wL, c.widths.wU) > MAX_W)],
    "tc_elasticity": [("wider than the tile format, 4 blocks", lambda c, s: max(c.widths.wL, c.widths.wU) > MAX_W and c.nblocks == 4)],
})
PRECONDITIONS.update({f"mix{k}": _mix_pre(k) for k in MIX_SEEDS})
assert set(PRECONDITIONS) == set(NAMES)

# (sweep, slot class, operand kind) whose factor value the sensitivity test zeroes: what the case exists for
MUTATIONS = {f"w{w}": [(sw, 0 if w <= 14 else (1 if w <= 20 else 2), RING_OP) for sw in (L, U)] for w in WIDTHS}
MUTATIONS.update({
    "Lwide": [(L, 1, RING_OP), (U, 0, SELF)],
    "Uwide": [(U, 1, RING_OP), (U, 2, RING_OP), (L, 0, SELF)],
    "mixed": [(L, 1, RING_OP), (L, 2, RING_OP), (U, 1, RING_OP), (U, 2, RING_OP)],
    "age15": [(L, 0, RING_OP), (U, 0, RING_OP)],
    "age16": [(L, 0, SELF), (U, 0, SELF)],
    "age17": [(L, 0, SELF), (U, 0, SELF)],
    "snake": [(L, 0, SELF), (U, 0, SELF), (L, 0, RING_OP)],
    "fanin111": [(L, 2, REMOTE)],
    "fanin112": [(L, 0, REMOTE), (L, 1, REMOTE), (L, 2, REMOTE), (L, 2, RING_OP), (U, 0, REMOTE)],
    "stagger": [(L, 0, REMOTE), (U, 0, REMOTE)],
    "chains64": [(L, 0, RING_OP), (U, 0, RING_OP)],
    "chains65": [(L, 0, REMOTE), (U, 0, REMOTE)],
    "packed": [],
    "layered26": [(L, 0, REMOTE), (L, 1, REMOTE), (L, 2, REMOTE), (L, 1, RING_OP), (L, 2, RING_OP), (U, 0, REMOTE)],
    "mix1": [(L, 0, -1)], "mix7": [(L, 0, -1)], "mix8": [(U, 0, -1)], "mix9": [(L, 2, -1), (U, 0, SELF)], "mix17": [(L, 1, -1), (U, 2, -1)],
})
assert set(MUTATIONS) == set(ACCEPTED)
