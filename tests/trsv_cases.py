"""Matrices and host analysis shared by tests/test_trsv_cases_reference.py (CPU) and tests/test_gpu_trsv_shapes.py (GPU): the
ILU(0) triangular solves at the shapes the xcd2 and level kernels branch on.

`level_table` restates in numpy what build_schedule (csrc/tri_levels.hpp) and build_xcd_schedule (csrc/engine_xcd2.hpp) compute --
the dependency level of every row per diagonal block and triangle, rows and widest row per level, sliced-ELL entries -- without
calling the library.  `residual_ratio` checks L U x = d against the library's own factor array in numpy.longdouble.  CASES are
built on first use (`case(name)`); PRECONDITIONS[name] are the branch conditions a case exists for, as predicates on its tables.
Nothing here needs a GPU."""
import functools

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
SMALL_LEVEL_ROWS = 2048          # csrc/tri_levels.hpp: a level with more rows gets a launch of its own (k_trsv_lower/upper_level)
SMALL_LEVELS_PER_LAUNCH = 256    # csrc/tri_levels.hpp: consecutive small levels that share one k_trsv_small_levels launch
SMALL_WG = 1024                  # TRSV_SMALL_WG of csrc/kernels.hpp
UNROLL = 16                      # TRSV_UNROLL: entries of a row per trip of the level kernels / per LDS tile of k_trsv_xcd2
WIDE_W = 96                      # enqueue_multi_levels: a level with w >= 96 takes k_trsv_level_multi_wide for nrhs <= 256
XCD_WAVES = 32                   # compute waves of one XCD at the 256-workgroup persistent grid of k_trsv_xcd2
MAX_ELL, MAX_N = 4 * 10 ** 6, 20000   # caps on every case: sliced-ELL entries (sum of m w) and rows


# ---- host analysis --------------------------------------------------------------------------------------------------------------
class Triangle:
    """one triangle of one diagonal block: level[i] of every row of the block, m[l] rows and w[l] widest row of every level"""

    def __init__(self, level, m, w):
        self.level, self.m, self.w = level, m, w
        self.nlev = len(m)
        self.chunks = (m + 63) // 64
        self.entries = int(np.sum(m.astype(np.int64) * w))


class LevelTable:
    def __init__(self, blocks):
        self.blocks = blocks                                   # [(Triangle L, Triangle U)] per diagonal block
        self.entries = sum(t.entries for b in blocks for t in b)
        self.triangles = [t for b in blocks for t in b]
        self.wL = max(int(b[0].w.max()) for b in blocks)
        self.wU = max(int(b[1].w.max()) for b in blocks)

    def summary(self):
        out = []
        for b, (L, U) in enumerate(self.blocks):
            for tag, t in (("L", L), ("U", U)):
                out.append(f"block {b} {tag}: {t.nlev} levels, m {int(t.m.min())}..{int(t.m.max())}, w {int(t.w.min())}..{int(t.w.max())}, "
                           f"chunks up to {int(t.chunks.max())}, sum m w = {t.entries}")
        return out


def _triangle(rp, ci, r0, r1, upper):
    n = r1 - r0
    level = np.zeros(n, dtype=np.int64)
    cnt = np.zeros(n, dtype=np.int64)
    order = range(r1 - 1, r0 - 1, -1) if upper else range(r0, r1)
    for i in order:
        c = ci[rp[i]:rp[i + 1]]
        dep = c[c > i] if upper else c[c < i]
        assert dep.size == 0 or (dep.min() >= r0 and dep.max() < r1), "entry outside the diagonal block"
        cnt[i - r0] = dep.size
        if dep.size:
            level[i - r0] = level[dep - r0].max() + 1
    nlev = int(level.max()) + 1
    m = np.bincount(level, minlength=nlev)
    w = np.zeros(nlev, dtype=np.int64)
    np.maximum.at(w, level, cnt)
    return Triangle(level, m, w)


def level_table(M, block_ptr):
    """Per diagonal block and triangle: level of every row (lower: 1 + the highest level among the columns left of the diagonal,
    rows ascending; upper: the same right of the diagonal, rows descending), rows per level, widest row per level, and the
    sliced-ELL entry count sum of m w over everything."""
    M = sp.csr_matrix(M)
    assert M.has_sorted_indices
    rp, ci = M.indptr.astype(np.int64), M.indices.astype(np.int64)
    bp = np.asarray(block_ptr, dtype=np.int64)
    return LevelTable([(_triangle(rp, ci, int(bp[b]), int(bp[b + 1]), False), _triangle(rp, ci, int(bp[b]), int(bp[b + 1]), True))
                       for b in range(len(bp) - 1)])


class Residual:
    """L U x = d against one factor array, in numpy.longdouble.  lu: the factor in the pattern of M -- multipliers below the
    diagonal (L has a unit diagonal), U above it, the INVERSE pivot on it (so the diagonal term of U x is x_i / lu_ii)."""

    def __init__(self, M, lu):
        M = sp.csr_matrix(M)
        n = M.shape[0]
        rp, self.ci = M.indptr, M.indices
        rows = np.repeat(np.arange(n), np.diff(rp))
        low, up, dg = self.ci < rows, self.ci > rows, self.ci == rows
        assert dg.sum() == n and len(lu) == M.nnz
        lu = np.asarray(lu, dtype=LD)
        zero = LD(0)
        self.low, self.up, self.piv = np.where(low, lu, zero), np.where(up, lu, zero), lu[dg]
        self.start = rp[:-1]                                     # every row holds its diagonal: no empty segment for reduceat

    def ratio(self, d, x, u):
        """max_i |d - L (U x)|_i / (u (|L| (|U| |x|))_i); inf if x has an entry that is not finite"""
        if not np.isfinite(x).all():
            return float("inf")
        d, x = np.asarray(d, dtype=LD), np.asarray(x, dtype=LD)
        ci, start = self.ci, self.start
        xd = x / self.piv
        Ux = np.add.reduceat(self.up * x[ci], start) + xd
        aUx = np.add.reduceat(np.abs(self.up) * np.abs(x)[ci], start) + np.abs(xd)
        LUx = np.add.reduceat(self.low * Ux[ci], start) + Ux
        aLUx = np.add.reduceat(np.abs(self.low) * aUx[ci], start) + aUx
        return float(np.max(np.abs(d - LUx) / (LD(u) * aLUx)))


def residual_ratio(M, lu, d, x, u):
    """max_i |d - L (U x)|_i / (u (|L| (|U| |x|))_i) with the factor array lu of the library's layout (class Residual)"""
    return Residual(M, lu).ratio(d, x, u)


def bound(table, extra=3):
    """C = 2 (w_L + w_U + extra).  Substitution in any summation order gives (T + dT) y = rhs with |dT| <= gamma_(w+1) |T| per
    sweep (w products and the pivot), hence |d - L U x| <= (gamma_L + gamma_U + gamma_L gamma_U) |L| |U| |x|; the factor 2 covers
    the second-order term and the longdouble evaluation.  extra = 5 for the single-precision sweeps: one more rounding of each
    factor entry and of d."""
    return 2 * (table.wL + table.wU + extra)


# ---- generators -----------------------------------------------------------------------------------------------------------------
def randomise(pattern, seed):
    """CSR with the off-diagonal pattern of `pattern` (plus a full diagonal): independent standard-normal values below and above
    the diagonal, diagonal 1 + sum |off-diagonal| of the row (strictly dominant), sorted indices"""
    P = sp.csr_matrix(pattern)
    n = P.shape[0]
    P = sp.csr_matrix((np.ones(P.nnz), P.indices, P.indptr), shape=P.shape)
    P.setdiag(0.0)
    P.eliminate_zeros()
    P.sort_indices()
    rng = np.random.default_rng(seed)
    P.data = rng.standard_normal(P.nnz)
    diag = 1.0 + np.asarray(abs(P).sum(axis=1)).ravel()
    M = sp.csr_matrix(P + sp.diags(diag, format="csr"))
    M.sort_indices()
    assert M.nnz == P.nnz + n
    return M


def layered(sizes, fan, seed):
    """Rows ordered layer by layer; row (l, r), l > 0, has lower entries at (l - 1, (r + j) mod m_(l-1)) for j < min(fan, m_(l-1));
    the upper pattern is the transpose."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    ri, cj = [], []
    for l in range(1, len(sizes)):
        mp, f = sizes[l - 1], min(fan, sizes[l - 1])
        r = np.repeat(np.arange(sizes[l]), f)
        j = np.tile(np.arange(f), sizes[l])
        ri.append(off[l] + r)
        cj.append(off[l - 1] + (r + j) % mp)
    n = int(off[-1])
    if ri:
        ri, cj = np.concatenate(ri), np.concatenate(cj)
        Lp = sp.csr_matrix((np.ones(len(ri)), (ri, cj)), shape=(n, n))
    else:
        Lp = sp.csr_matrix((n, n))
    return randomise(Lp + Lp.T, seed)


def band(n, offsets, seed):
    offs = [k for k in offsets if 0 < k < n]
    Lp = sp.diags([np.ones(n - k) for k in offs], [-k for k in offs], shape=(n, n), format="csr") if offs else sp.csr_matrix((n, n))
    return randomise(Lp + Lp.T, seed)


def poisson_block(N, seed):
    from dune_ddm_amd import synth
    return randomise(synth.StructuredPoisson(N, (1,) * len(N)).subdomain(0).A, seed)


def _structured_blocks(grid, overlap):
    from dune_ddm_amd.problem import build_structured
    dec = build_structured(grid, overlap=overlap)
    return [sp.csr_matrix(sd.A_dir) for sd in dec.subs]


def _diag_blocks(mats):
    M = sp.block_diag(mats, format="csr")
    M.sort_indices()
    return M, np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)


# uneven blocks of at most 1500 rows: small layered, band and Poisson (9, 8, 7) blocks, and a one-row block
_POOL = (lambda s: layered([130, 30, 200, 64, 65], 3, s),
         lambda s: poisson_block((9, 8, 7), s),
         lambda s: band(700, range(140, 160), s),               # 20 entries per row: w > 16
         lambda s: layered([1], 1, s),                          # the one-row block
         lambda s: layered([1] * 40, 1, s),
         lambda s: band(1500, (1, 37, 500), s),
         lambda s: poisson_block((7, 6, 5), s),
         lambda s: layered([80, 2, 80], 40, s),                 # few wide rows: L w = 40, U w = 80 (below the w >= 96 sweep)
         lambda s: band(333, (1, 2, 3), s))


def _blocks(count, seed):
    return _diag_blocks([_POOL[(b * 4 + seed) % len(_POOL)](100 * seed + b) for b in range(count)])


def _one(M):
    return M, np.array([0, M.shape[0]], dtype=np.int64)


def _elasticity():
    from dune_ddm_amd import synth
    return _diag_blocks(_structured_blocks(synth.StructuredElasticity(cells=(20, 4, 6), parts=4), 1))


def _dg():
    from dune_ddm_amd import synth
    return _diag_blocks(_structured_blocks(synth.StructuredDG2D((24, 24), (2, 2)), 2))


_BUILDERS = {
    "band17": lambda: _one(band(12700, range(4192, 4209), 1)),
    "layers": lambda: _one(layered([4200, 1, 4200, 70, 2100, 3, 130], 2, 2)),
    "wide": lambda: _one(layered([300, 2, 300, 40, 40], 40, 3)),
    "chain600": lambda: _one(layered([1] * 600, 1, 4)),
    "elasticity": _elasticity,
    "dg": _dg,
    "blocks3": lambda: _blocks(3, 5),
    "blocks9": lambda: _blocks(9, 6),
    "blocks17": lambda: _blocks(17, 7),
}
NAMES = tuple(_BUILDERS)


class Case:
    """(name, M, block_ptr) with its tables: `table` per diagonal block (what xcd2 schedules), `whole` for the matrix as one block
    (the level engine and the block sweeps: build_schedule merges level l of every block)."""

    def __init__(self, name):
        self.name = name
        self.M, self.block_ptr = _BUILDERS[name]()
        assert self.M.has_sorted_indices
        self.n = self.M.shape[0]
        self.table = level_table(self.M, self.block_ptr)
        self.whole = self.table if len(self.block_ptr) == 2 else level_table(self.M, [0, self.n])
        self.C = bound(self.table)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def cases():
    return [(c.name, c.M, c.block_ptr) for c in map(case, NAMES)]


class _Cases:
    """CASES behaves as the list of (name, M, block_ptr); the matrices are built when it is first iterated"""

    def __iter__(self):
        return iter(cases())

    def __len__(self):
        return len(NAMES)


CASES = _Cases()


# ---- the branch conditions ------------------------------------------------------------------------------------------------------
def few_wide(t):
    """levels of a triangle that take the "few wide rows" branch of k_trsv_small_levels (S lanes per row, butterfly sum)"""
    return (t.w >= 32) & (2 * t.m <= SMALL_WG)


def _any(tris, fn):
    return any(bool(np.any(fn(t))) for t in tris)


def _longest_small_run(t):
    best = run = 0
    for m in t.m:
        run = run + 1 if m <= SMALL_LEVEL_ROWS else 0
        best = max(best, run)
    return best


def _chunk_steps(c):
    """consecutive (previous level, this level) chunk counts of a block: L levels then U levels, as k_trsv_xcd2 walks them"""
    L, U = c.table.blocks[0]
    seq = np.concatenate([L.chunks, U.chunks])
    return list(zip(seq[:-1], seq[1:]))


def _column_order_levels(c):
    """True where the level engine sums every row in column order (no level of the merged schedule in the few-wide-rows branch)"""
    return not _any(c.whole.triangles, few_wide)


PRECONDITIONS = {
    "band17": [
        ("one block, 4 levels per triangle", lambda c: [t.nlev for t in c.table.triangles] == [4, 4]),
        ("a level of m > 2048 rows with a ragged last chunk, in both triangles (k_trsv_lower/upper_level; xcd2: c += W strides)",
         lambda c: all(np.any((t.m > SMALL_LEVEL_ROWS) & (t.m % 64 != 0) & (t.chunks > 2 * XCD_WAVES)) for t in c.table.triangles)),
        ("m = 4192 = 65 full chunks + 32 rows", lambda c: all(int(t.m.max()) == 4192 and int(t.chunks.max()) == 66 for t in c.table.triangles)),
        ("w = 17 > TRSV_UNROLL on three levels per triangle (second trip of the unrolled loop, xcd2 global tail)",
         lambda c: all(int((t.w == 17).sum()) == 3 for t in c.table.triangles)),
        ("the level engine sums in column order everywhere", _column_order_levels),
    ],
    "layers": [
        ("n = 10704, 7 lower levels with chunk counts 66, 1, 66, 2, 33, 1, 3",
         lambda c: c.n == 10704 and list(c.table.blocks[0][0].chunks) == [66, 1, 66, 2, 33, 1, 3]),
        ("nact_prev = min(ncp, W) both ways: a level of > W chunks after a one-chunk level and the reverse",
         lambda c: any(a == 1 and b > XCD_WAVES for a, b in _chunk_steps(c)) and any(a > XCD_WAVES and b == 1 for a, b in _chunk_steps(c))),
        ("waves without a chunk in a level: a level of fewer chunks than W", lambda c: _any(c.table.triangles, lambda t: t.chunks < XCD_WAVES)),
        ("U has a level of more than 10 000 rows with a ragged last chunk", lambda c: _any([c.table.blocks[0][1]], lambda t: (t.m > 10000) & (t.m % 64 != 0))),
        ("U has a one-row level of w = 4200", lambda c: _any([c.table.blocks[0][1]], lambda t: (t.m == 1) & (t.w == 4200))),
        ("a large level between small ones: the launch plan alternates", lambda c: _any(c.table.triangles, lambda t: t.m > SMALL_LEVEL_ROWS) and
         _any(c.table.triangles, lambda t: t.m <= SMALL_LEVEL_ROWS)),
        ("the L sweep of the level engine sums in column order, the U sweep has a few-wide-rows level",
         lambda c: not np.any(few_wide(c.whole.blocks[0][0])) and np.any(few_wide(c.whole.blocks[0][1]))),
    ],
    "wide": [
        ("n = 682, L w = 40, U w = 300", lambda c: c.n == 682 and c.table.wL == 40 and c.table.wU == 300),
        ("exactly one level with w >= 96 (k_trsv_level_multi_wide; f32 declined)", lambda c: sum(int((t.w >= WIDE_W).sum()) for t in c.table.triangles) == 1),
        ("at least three levels per triangle in the few-wide-rows branch", lambda c: all(int(few_wide(t).sum()) >= 3 for t in c.table.triangles)),
        ("S = 64 and S = 16 lanes per row: few-wide levels of m = 2 and of m = 40 rows", lambda c: _any(c.table.triangles, lambda t: few_wide(t) & (t.m == 2)) and
         _any(c.table.triangles, lambda t: few_wide(t) & (t.m == 40))),
    ],
    "chain600": [
        ("600 one-row levels per triangle", lambda c: all(t.nlev == 600 and int(t.m.max()) == 1 for t in c.table.triangles)),
        ("more than 256 consecutive small levels: launch plan 256 + 256 + 88", lambda c: all(_longest_small_run(t) == 600 for t in c.table.triangles) and
         600 > 2 * SMALL_LEVELS_PER_LAUNCH),
    ],
    "elasticity": [
        ("4 blocks of 700..900 rows", lambda c: len(c.table.blocks) == 4 and all(700 <= b[0].level.size <= 900 for b in c.table.blocks)),
        ("w up to 37..41", lambda c: 37 <= max(c.table.wL, c.table.wU) <= 41),
        ("44..57 levels per triangle, at least 32 of them with w > 16", lambda c: all(44 <= t.nlev <= 57 and int((t.w > UNROLL).sum()) >= 32 for t in c.table.triangles)),
        ("at least 10 levels per triangle in the few-wide-rows branch (per block and merged)",
         lambda c: all(int(few_wide(t).sum()) >= 10 for t in c.table.triangles + c.whole.triangles)),
        ("fewer than 8 groups", lambda c: len(c.table.blocks) < 8),
    ],
    "dg": [
        ("4 blocks of 876 rows", lambda c: [b[0].level.size for b in c.table.blocks] == [876] * 4),
        ("96..108 levels per triangle", lambda c: all(96 <= t.nlev <= 108 for t in c.table.triangles)),
        ("non-symmetric values", lambda c: abs(c.M - c.M.T).max() > 1e-3 * abs(c.M).max()),
        ("the level engine sums in column order everywhere", _column_order_levels),
    ],
    "blocks3": [
        ("3 uneven blocks (owners < 8), each <= 1500 rows", lambda c: len(c.table.blocks) == 3 and len({b[0].level.size for b in c.table.blocks}) == 3 and
         max(b[0].level.size for b in c.table.blocks) <= 1500),
    ],
    "blocks9": [
        ("9 blocks: XCD 0 owns two groups, the others one", lambda c: len(c.table.blocks) == 9),
        ("uneven, each <= 1500 rows, one of them a single row", lambda c: max(b[0].level.size for b in c.table.blocks) <= 1500 and
         min(b[0].level.size for b in c.table.blocks) == 1),
        ("w > 16 in some block", lambda c: max(c.table.wL, c.table.wU) > UNROLL),
        ("no level with w >= 96 in the merged schedule (block sweeps == single-vector solve)", lambda c: not _any(c.whole.triangles, lambda t: t.w >= WIDE_W)),
    ],
    "blocks17": [
        ("17 blocks: XCD 0 owns three groups, the others two", lambda c: len(c.table.blocks) == 17),
        ("uneven, each <= 1500 rows, one of them a single row", lambda c: max(b[0].level.size for b in c.table.blocks) <= 1500 and
         min(b[0].level.size for b in c.table.blocks) == 1),
        ("non-symmetric values", lambda c: abs(c.M - c.M.T).max() > 1e-3 * abs(c.M).max()),
    ],
}
assert set(PRECONDITIONS) == set(NAMES)


def oracle_factor_and_solve(c, d):
    """(lu, x): the oracle's sequential ILU(0) of the whole block-diagonal matrix (no entry couples two blocks, so this is the
    factor of every block) and its solve of d"""
    from oracle import apply_oracle as ao
    ref = ao.Ilu0(ao.Csr(c.M))
    x = np.zeros(c.n)
    ref.apply(x, np.ascontiguousarray(d, dtype=np.float64))
    return ref.lu, x
