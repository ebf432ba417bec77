"""Matrices and host analysis shared by tests/test_box_cases_reference.py (CPU) and tests/test_gpu_box_shapes.py (GPU): the ILU(0)
solve of the box engine (csrc/trsv_box.hpp, csrc/engine_box.hpp) at the shapes its builder (csrc/trsv_box_host.hpp) and its kernel
branch on.

`box(nx, ny, nz, nshell, couple, seed)` is the generator: the full 27-point lexicographic pattern of an nx x ny x nz box with nshell
rows behind it; box row q couples to the shell rows couple(q), shell rows to each other at the offsets `band`; the pattern is
symmetric, the values are trsv_cases.randomise's (independent normals, strictly dominant).  `case(name)` builds a matrix on first use.
EXPECT[name] is the engine the factor must end on: "box", or for what the builder declines (DECLINES[name], the reason word for word)
what the pipe builder then makes of it ("pipe", or "xcd2" where it declines as well).  `built(name)` runs the HOST BUILDER ITSELF
(tests/cpp/box_host_test.cpp: box_test_case) on the oracle's factor and returns what it made: per block the box, the rows behind it,
the histogram of shell entries per box row, the planes detect gave back, lines per lane, and the CPU walks of the kernel's data flow.
PRECONDITIONS[name] are the branch conditions a case exists for, as predicates on that; MUTATIONS[name] the stream values and products
whose loss the checks of the GPU test must notice; NESTED[name] the engine of the factor behind the boxes.  Nothing here needs a GPU."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import scipy.sparse as sp

from tests import pipe_cases as pc
from tests import trsv_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
MAX_NX, MAX_EXT, MAX_STEPS = 120, 20, 1024                        # csrc/trsv_box_host.hpp
MAX_N, MAX_ENTRIES = 60000, 1500000                              # caps on every case: rows, factor entries
L, U = 0, 1
PIVOT, PRODUCT_LOW, PRODUCT_HIGH = 13, -1, -2                    # value slots of a mutation beside the entries e = 0 .. 12
TOO_SMALL = "block too small"
CORNER = f"first row does not have the pattern of a box corner (or nx > {MAX_NX})"
PLANES = "fewer than two conforming planes"
HALF = "the box covers less than half of the block"
STEPS = f"more than {MAX_STEPS} steps per plane"


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def box_pattern(nx, ny, nz, nshell=0, couple=None, band=(1,)):
    """0/1 pattern (without the diagonal) of the box with its rows behind it"""
    nb = nx * ny * nz
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    q = (i + nx * (j + ny * k)).ravel()
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    ri, cj = [], []
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                if (di, dj, dk) == (0, 0, 0):
                    continue
                ok = (i + di >= 0) & (i + di < nx) & (j + dj >= 0) & (j + dj < ny) & (k + dk >= 0) & (k + dk < nz)
                ri.append(q[ok])
                cj.append(q[ok] + di + nx * (dj + ny * dk))
    ri, cj = [np.concatenate(ri)], [np.concatenate(cj)]
    if nshell and couple is not None:
        for row in range(nb):
            cols = sorted(set(int(t) for t in couple(row)))
            assert all(0 <= t < nshell for t in cols)
            ri += [np.full(len(cols), row), nb + np.asarray(cols, dtype=np.int64)]
            cj += [nb + np.asarray(cols, dtype=np.int64), np.full(len(cols), row)]
    for o in band:
        if 0 < o < nshell:
            t = np.arange(nshell - o)
            ri += [nb + t + o, nb + t]
            cj += [nb + t, nb + t + o]
    ri, cj = np.concatenate(ri).astype(np.int64), np.concatenate(cj).astype(np.int64)
    P = sp.csr_matrix((np.ones(len(ri)), (ri, cj)), shape=(nb + nshell, nb + nshell))
    P.sum_duplicates()
    assert abs(P - P.T).nnz == 0
    return P


def box(nx, ny, nz, nshell=0, couple=None, seed=0, band=(1,)):
    return tc.randomise(box_pattern(nx, ny, nz, nshell, couple, band), seed)


def first(count, nshell):
    """box row q couples to the count(q) shell rows q, q + 1, .. (mod nshell)"""
    return lambda q: [(q + t) % nshell for t in range(count(q))]


def permuted(M, a, b):
    p = np.arange(M.shape[0])
    p[[a, b]] = p[[b, a]]
    M = sp.csr_matrix(M[p][:, p])
    M.sort_indices()
    return M


def _one(M):
    return M, np.array([0, M.shape[0]], dtype=np.int64)


def _diag_blocks(mats):
    M = sp.block_diag(mats, format="csr")
    M.sort_indices()
    return M, np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)


def _shrink(seed, shift=0, bad_plane=4):
    """4 x 4 x 5 + 24 rows: one row of plane `bad_plane` has 21 shell entries, the others (q + shift) mod 12"""
    bad = 16 * bad_plane + 6
    return box(4, 4, 5, 24, first(lambda q: 21 if q == bad else (q + shift) % 12, 24), seed)


_BLOCKS = {                                                     # single blocks by name (seed -> matrix)
    "tall70": lambda s: box(2, 2, 70, seed=s),
    "ext20": lambda s: box(4, 4, 4, 24, first(lambda q: q % 21, 24), s),
    "ny65": lambda s: box(5, 65, 3, seed=s),
    "nx120": lambda s: box(120, 2, 2, seed=s),
    "shrink": lambda s: _shrink(s),
    "y66": lambda s: box(7, 66, 2, 10, first(lambda q: q % 3, 10), s),
    "x120y3": lambda s: box(120, 3, 2, seed=s),
}
_HETERO_POOL = ("tall70", "ext20", "ny65", "nx120", "shrink", "y66")
HETERO_SEEDS = {7: 1, 8: 2, 9: 3, 17: 4}


def _hetero(count):
    s = HETERO_SEEDS[count]
    return _diag_blocks([_BLOCKS[_HETERO_POOL[(b + s) % len(_HETERO_POOL)]](100 * s + b) for b in range(count)])


_BUILDERS = {
    "thin1024": lambda: _one(box(2, 512, 2, seed=1)),
    "thin1026": lambda: _one(box(2, 513, 2, seed=2)),
    "thin1023": lambda: _one(box(3, 511, 2, seed=3)),
    "nx120": lambda: _one(_BLOCKS["nx120"](4)),
    "nx121": lambda: _one(box(121, 2, 2, seed=5)),
    "nx3": lambda: _one(box(3, 5, 5, seed=6)),
    "nz2": lambda: _one(box(6, 6, 2, seed=7)),
    "tall70": lambda: _one(_BLOCKS["tall70"](8)),
    "ny64": lambda: _one(box(3, 64, 3, seed=9)),
    "ny65": lambda: _one(_BLOCKS["ny65"](10)),
    "ny128": lambda: _one(box(3, 128, 2, seed=11)),
    "ny129": lambda: _one(box(4, 129, 2, seed=12)),
    "tiny64": lambda: _one(box(4, 4, 4, seed=13)),
    "tiny63": lambda: _one(box(3, 3, 7, seed=14)),
    "ext20": lambda: _one(_BLOCKS["ext20"](15)),
    "ext_odd": lambda: _one(box(4, 4, 4, 24, first(lambda q: 2 * (q % 10) + 1, 24), 16)),
    "shrink": lambda: _one(_BLOCKS["shrink"](17)),
    "shrink20": lambda: _one(_shrink(18, shift=1)),
    "ext21_mid": lambda: _one(_shrink(19, bad_plane=1)),
    "half_ok": lambda: _one(box(4, 4, 4, 64, first(lambda q: q % 12, 64), 20)),
    "half": lambda: _one(box(4, 4, 4, 65, first(lambda q: q % 12, 65), 21)),
    "shell_wide": lambda: _one(box(4, 4, 4, 60, first(lambda q: q % 7, 60), 22, band=range(1, 31))),
    "one_declines": lambda: _diag_blocks([box(4, 4, 4, 12, first(lambda q: q % 5, 12), 23), permuted(box(5, 5, 4, seed=24), 32, 33), box(3, 5, 5, seed=25)]),
    "hetero4": lambda: _diag_blocks([_BLOCKS["tall70"](26), _BLOCKS["y66"](27), _BLOCKS["x120y3"](28), _BLOCKS["ext20"](29)]),
    "hetero7": lambda: _hetero(7),
    "hetero8": lambda: _hetero(8),
    "hetero9": lambda: _hetero(9),
    "hetero17": lambda: _hetero(17),
}
NAMES = tuple(_BUILDERS)
DECLINES = {"thin1026": "block 0: " + STEPS, "nx121": "block 0: " + CORNER, "tiny63": "block 0: " + TOO_SMALL, "ext21_mid": "block 0: " + PLANES,
            "half": "block 0: " + HALF, "one_declines": "block 1: " + PLANES}
# where the box builder declines, the pipe builder gets the matrix (asserted on the CPU with pipe_cases.run_builder): ext21_mid has a
# row of 13 + 21 upper entries, wider than pipe's tile
DECLINED_ENGINE = {"thin1026": "pipe", "nx121": "pipe", "tiny63": "pipe", "ext21_mid": "xcd2", "half": "pipe", "one_declines": "pipe"}
EXPECT = {name: DECLINED_ENGINE.get(name, "box") for name in NAMES}
ACCEPTED = tuple(n for n in NAMES if n not in DECLINES)
# engine of the nested factor (the rows behind the boxes) once settled: pipe, or xcd2 where the pipe builder declines the shell system
# (asserted on the CPU); None: no rows behind the boxes
NESTED = {name: None for name in ACCEPTED}
NESTED.update({name: "pipe" for name in ("ext20", "ext_odd", "shrink", "shrink20", "half_ok", "hetero4", "hetero7", "hetero8", "hetero9", "hetero17")})
NESTED["shell_wide"] = "xcd2"
TAIL = ("ext20", "shrink", "hetero9")
CHAINED = ("hetero9", "hetero17")


class Case:
    def __init__(self, name):
        self.name = name
        self.M, self.block_ptr = _BUILDERS[name]()
        self.M = sp.csr_matrix(self.M)
        self.M.sort_indices()
        self.block_ptr = np.asarray(self.block_ptr, dtype=np.int64)
        self.n = self.M.shape[0]
        self.nblocks = len(self.block_ptr) - 1
        self.widths = pc.Widths(self.M)
        self.C = tc.bound(self.widths)                          # the bound of check (a), as in tests/trsv_cases.py
        self.entries = self.M.nnz - self.n


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---- the host builder -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def harness():
    subprocess.check_call(["make", "-C", CPP, "libbox_host_test.so"], stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(CPP, "libbox_host_test.so"))
    lib.box_test_case.restype = ctypes.c_int
    lib.box_test_shell_system.restype = ctypes.c_int
    return lib


class Block:
    def __init__(self, w):
        self.nx, self.ny, self.nz, self.nsteps, self.shell = (int(v) for v in w[:5])
        self.hist = w[5:26].copy()                              # box rows with 0 .. 20 shell entries
        self.back, self.lines = int(w[26]), int(w[27])          # planes detect gave back; lines a lane serves
        self.figures = (self.nx, self.ny, self.nz, self.nsteps, self.shell)   # what Ilu0.box_info() reports per block


class Built:
    """what box::build made of a factor, and the emulated solve"""

    def __init__(self, rc, err, x, stats, nblocks):
        self.rc, self.err, self.x = rc, err, x
        self.st = dict(zip(("box_rows", "shell_rows", "stream_bytes", "ext_products", "shell_lower_entries", "nested_entries", "nblocks", "nested_widest"),
                           stats[:8].tolist()))
        self.mutation = dict(zip(("row", "block", "plane", "step", "lane", "slot", "product"), stats[8:15].tolist()))
        self.blocks = [Block(stats[16 + 32 * b:48 + 32 * b]) for b in range(nblocks)] if rc != 1 else []

    def figures(self):
        return "; ".join(f"block {b}: {B.nx} x {B.ny} x {B.nz}, {B.nsteps} steps, {B.shell} rows behind, {B.lines} line(s) per lane, {B.back} plane(s) given back, "
                         f"shell entries per row {{{', '.join(f'{k}: {int(v)}' for k, v in enumerate(B.hist) if v)}}}" for b, B in enumerate(self.blocks))


def _args(M, block_ptr, lu, diag):
    rp = np.asarray(M.indptr, dtype=np.int64)
    ci = np.asarray(M.indices, dtype=np.int32)
    bp = np.asarray(block_ptr, dtype=np.int64)
    lu = np.ascontiguousarray(lu, dtype=np.float64)
    diag = np.ascontiguousarray(diag, dtype=np.int64)
    return rp, ci, lu, diag, bp


_p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def run_builder(M, block_ptr, lu, diag, d, mutate=None):
    """box::build and the CPU walks (emulate and emulate_lanes, which must agree bit for bit; with a mutation emulate_lanes alone) into a
    NaN-filled x; mutate = (sweep, e, Jmin, Jmax): box_test_case in tests/cpp/box_host_test.cpp"""
    lib = harness()
    n = M.shape[0]
    rp, ci, lu, diag, bp = _args(M, block_ptr, lu, diag)
    d = np.ascontiguousarray(d, dtype=np.float64)
    x = np.full(n, np.nan)
    nb = len(bp) - 1
    stats = np.zeros(16 + 32 * nb, dtype=np.int64)
    mut = np.asarray(mutate, dtype=np.int64) if mutate is not None else None
    err = ctypes.create_string_buffer(256)
    rc = lib.box_test_case(ctypes.c_int64(n), _p(rp), _p(ci), _p(lu), _p(diag), ctypes.c_int(nb), _p(bp), _p(d), _p(x), _p(stats),
                           ctypes.c_int64(len(stats)), _p(mut), err, 256)
    return Built(rc, err.value.decode(), x, stats, nb)


def shell_system(M, block_ptr, lu, diag):
    """(matrix holding the nested factor's values in its pattern, block_ptr, diag) of the rows behind the boxes; None without such rows"""
    lib = harness()
    n = M.shape[0]
    rp, ci, lu, diag, bp = _args(M, block_ptr, lu, diag)
    sizes = np.zeros(2, dtype=np.int64)
    args = (ctypes.c_int64(n), _p(rp), _p(ci), _p(lu), _p(diag), ctypes.c_int(len(bp) - 1), _p(bp), _p(sizes))
    assert lib.box_test_shell_system(*args, None, None, None, None, None) == 0
    ns, nnz = int(sizes[0]), int(sizes[1])
    if ns == 0:
        return None
    frp, fci, fva = np.zeros(ns + 1, dtype=np.int64), np.zeros(nnz, dtype=np.int32), np.zeros(nnz)
    fdiag, fbp = np.zeros(ns, dtype=np.int64), np.zeros(len(bp), dtype=np.int64)
    assert lib.box_test_shell_system(*args, _p(frp), _p(fci), _p(fva), _p(fdiag), _p(fbp)) == 0
    return sp.csr_matrix((fva, fci, frp), shape=(ns, ns)), fbp, fdiag


class Ref:
    """per case, computed once and never changed: the oracle's factor, two right-hand sides and its solves of them"""

    def __init__(self, name):
        self.c = c = case(name)
        rng = np.random.default_rng(47)
        self.d = [rng.standard_normal(c.n), rng.standard_normal(c.n)]
        self.f, self.lu, self.diag = pc.oracle_factor(c.M)
        self.x = [pc.oracle_solve(self.f, d) for d in self.d]
        for a in (self.d[0], self.d[1], self.lu, self.x[0], self.x[1]):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def ref(name):
    return Ref(name)


@functools.lru_cache(maxsize=None)
def built(name):
    r = ref(name)
    return run_builder(r.c.M, r.c.block_ptr, r.lu, r.diag, r.d[0])


# ---- the branch conditions --------------------------------------------------------------------------------------------------------
def _shape(*figures):
    """one block with exactly these figures (nx, ny, nz, steps per plane, rows behind the box)"""
    return lambda c, s: [B.figures for B in s.blocks] == [figures]


def turns_past(s):
    """turns of the three-turn step loop behind the last step of a plane, per block: the loop runs l = -1, 2, 5, .. in whole trips"""
    return {(-(B.nsteps + 1)) % 3 for B in s.blocks}


def _hetero_pre(count):
    return [
        (f"accepted, {count} blocks", lambda c, s: s.rc == 0 and len(s.blocks) == count),
        ("side of the eight-block switch of local_ok / gcount (fewer than 8: every workgroup serves every block, write-through; 8 or more: an XCD "
         "serves the blocks g = xcc mod 8, two or three of them from 9 / 17 on)", lambda c, s: (len(s.blocks) < 8) == (count < 8)),
        ("blocks of at least five different shapes follow each other: sh_tab is reloaded with another table",
         lambda c, s: len({B.figures for B in s.blocks}) >= 5 and all(a.figures != b.figures for a, b in zip(s.blocks, s.blocks[1:]))),
        ("among them more than 64 planes, two lines per lane, nx = 120, a plane given back, rows of 20 shell entries",
         lambda c, s: any(B.nz > 64 for B in s.blocks) and any(B.lines == 2 for B in s.blocks) and any(B.nx == MAX_NX for B in s.blocks) and
         any(B.back == 1 for B in s.blocks) and any(B.hist[MAX_EXT] > 0 for B in s.blocks)),
    ]


PRECONDITIONS = {
    "thin1024": [("2 x 512 x 2, exactly MAX_STEPS = 1024 steps per plane", _shape(2, 512, 2, MAX_STEPS, 0)),
                 ("a lane serves eight lines", lambda c, s: s.blocks[0].lines == 8)],
    "thin1026": [("2 x 513 x 2 would have 1026 steps", lambda c, s: c.n == 2 * 513 * 2 and 2 + 2 * 512 == 1026)],
    "thin1023": [("3 x 511 x 2, 1023 steps: one below the cap, odd", _shape(3, 511, 2, 1023, 0))],
    "nx120": [("nx = MAX_NX = 120, ny = nz = 2, 122 steps", _shape(MAX_NX, 2, 2, 122, 0))],
    "nx121": [("nx = 121", lambda c, s: c.n == 121 * 4)],
    "nx3": [("nx = 3: a row has both x neighbours only in the middle column", _shape(3, 5, 5, 11, 0))],
    "nz2": [("nz = 2: a first and a last plane only", _shape(6, 6, 2, 16, 0))],
    "tall70": [("2 x 2 x 70: nx = ny = 2, 4 steps per plane, 280 rows", _shape(2, 2, 70, 4, 0)),
               ("more planes than 64, and than the 8 workgroups of DDM_BOX_GRID=8 serve at once", lambda c, s: s.blocks[0].nz > 64)],
    "ny64": [("ny = 64: every lane has exactly one line", lambda c, s: _shape(3, 64, 3, 129, 0)(c, s) and s.blocks[0].lines == 1)],
    "ny65": [("ny = 65: lane 0 serves a second line, whose line J - 1 is lane 63's first", lambda c, s: _shape(5, 65, 3, 133, 0)(c, s) and s.blocks[0].lines == 2)],
    "ny128": [("ny = 128: every lane has exactly two lines", lambda c, s: _shape(3, 128, 2, 257, 0)(c, s) and s.blocks[0].lines == 2)],
    "ny129": [("ny = 129: lane 0 serves a third line", lambda c, s: _shape(4, 129, 2, 260, 0)(c, s) and s.blocks[0].lines == 3)],
    "tiny64": [("a block of exactly 64 rows", lambda c, s: c.n == 64 and _shape(4, 4, 4, 10, 0)(c, s))],
    "tiny63": [("a block of 63 rows", lambda c, s: c.n == 63)],
    "ext20": [("4 x 4 x 4 with 24 rows behind it, 692 product slots", lambda c, s: _shape(4, 4, 4, 10, 24)(c, s) and s.st["ext_products"] == 692),
              ("rows of every count 0 .. MAX_EXT = 20 of shell entries: all ten product slots are filled, the count 20 is reached",
               lambda c, s: (s.blocks[0].hist > 0).all() and s.blocks[0].back == 0)],
    "ext_odd": [("rows of every odd count 1 .. 19 and of no even one: every product slice is padded", lambda c, s: _shape(4, 4, 4, 10, 24)(c, s) and
                 [k for k, v in enumerate(s.blocks[0].hist) if v] == list(range(1, 20, 2)))],
    "shrink": [("4 x 4 x 5 taken as 4 x 4 x 4: detect gave one plane back, its 16 rows are behind the box now", lambda c, s: _shape(4, 4, 4, 10, 40)(c, s) and
                s.blocks[0].back == 1),
               ("the last plane's rows have up to nine shell entries more than the generator gave them", lambda c, s: int(np.flatnonzero(s.blocks[0].hist).max()) > 11)],
    "shrink20": [("as shrink", lambda c, s: _shape(4, 4, 4, 10, 40)(c, s) and s.blocks[0].back == 1),
                 ("a row of the last kept plane has 11 + 9 = 20 shell entries", lambda c, s: s.blocks[0].hist[MAX_EXT] > 0)],
    "ext21_mid": [("a row of plane 1 has 21 shell entries; every triangular row of the matrix shows it to pipe: 13 + 21 upper entries",
                   lambda c, s: c.widths.wU == 13 + MAX_EXT + 1)],
    "half_ok": [("the box is exactly half of the block", _shape(4, 4, 4, 10, 64))],
    "half": [("the box is one row less than half of the block", lambda c, s: c.n == 64 + 65)],
    "shell_wide": [("60 rows behind the box with up to 30 shell-shell entries per triangle row: wider than pipe's tile",
                    lambda c, s: _shape(4, 4, 4, 10, 60)(c, s) and s.st["nested_widest"] > pc.MAX_W)],
    "one_declines": [("three blocks, the one in the middle a permuted box", lambda c, s: c.nblocks == 3 and s.err.startswith("block 1:")),
                     ("no triangular row wider than pipe's tile", lambda c, s: max(c.widths.wL, c.widths.wU) <= pc.MAX_W)],
    "hetero4": [("four blocks of four shapes, 2022 rows", lambda c, s: c.n == 2022 and [B.figures for B in s.blocks] ==
                 [(2, 2, 70, 4, 0), (7, 66, 2, 137, 10), (120, 3, 2, 124, 0), (4, 4, 4, 10, 24)])],
}
PRECONDITIONS.update({f"hetero{k}": _hetero_pre(k) for k in HETERO_SEEDS})
assert set(PRECONDITIONS) == set(NAMES)

# (sweep, value slot, Jmin, Jmax) whose factor value the sensitivity test zeroes; e = 0 .. 12 in ascending column order: L sweep 0 .. 8 the
# previous plane (lines J - 1, J, J + 1), 9 .. 11 line J - 1, 12 the lane's previous result; U sweep (mirrored) 0 the previous result,
# 1 .. 3 line J - 1, 4 .. 12 the previous plane
_ANY = (0, 1 << 30)
_BASE = [(L, 4) + _ANY, (L, 12) + _ANY, (U, 0) + _ANY, (U, 8) + _ANY, (U, PIVOT) + _ANY]
MUTATIONS = {name: list(_BASE) for name in ACCEPTED}
MUTATIONS["tall70"] += [(L, e) + _ANY for e in (0, 8)]                          # previous-plane operands, first and last column of the windows
MUTATIONS["ny65"] += [(L, 10, 64, 64), (L, 0, 64, 64), (U, 2, 64, 64)]          # line J - 1 of lane 0's second line: lane 63's first
MUTATIONS["ny129"] += [(L, 10, 128, 128), (U, 2, 128, 128)]                     # ... of its third line
MUTATIONS["ny128"] += [(L, 11, 64, 127)]
MUTATIONS["thin1024"] += [(L, 10, 448, 511), (U, 5, 448, 511)]                  # a lane's eighth line
for _name in ("ext20", "ext_odd", "shrink", "shrink20", "hetero9", "hetero17"):
    MUTATIONS[_name] += [(U, PRODUCT_LOW) + _ANY, (U, PRODUCT_HIGH) + _ANY]      # a product in slots q < 7, one in slots q >= 7
for _name in ("half_ok", "shell_wide", "hetero4", "hetero7", "hetero8"):
    MUTATIONS[_name] += [(U, PRODUCT_LOW) + _ANY]
