"""Matrices, host analysis and bounds shared by tests/test_direct_cases_reference.py (CPU) and tests/test_gpu_direct_host_shapes.py
(GPU): the device solves of the sparse direct factor with the HOST factorisation (direct_create_impl with DDM_DIRECT_ENGINE=host,
csrc/tri_csr.hpp, k_trsv_csr_fused / _blocks / _level / _level_multi of csrc/kernels.hpp) at the shapes those kernels branch on.

`schedule_table` restates in numpy, from the arrays ddm.chol_host returns and without calling any schedule code of the library, what
detect_supernodes and build_csr_schedule compute: the supernode runs, the transformed rows (phase-1 rows into virtual unknowns n + q,
phase-2 rows over the inverted diagonal block, plain rows) with their levels, rows / entries / lanes per row S of every level, which
levels are small, the launch plan, the per-block renumbering with blk_lev_ptr, and whether direct_create_impl takes the block path.
`sweeps` is a float64 restatement of the two solves on those rows; `Residual` checks L U x = d against a factor array in
numpy.longdouble.  CASES are built on first use (`case(name)`); PRECONDITIONS[name] are the branch conditions a case exists for, as
predicates on its tables.  Nothing here needs a GPU.

The bounds (u = 2^-53, no constant tuned on device output):

  plain rows.  trsv_cases.bound with extra = 3 + 6: C = 2 (w_L + w_U + 9), w_L / w_U the widest lower / upper row of the factor.
  The kernels give a row to S <= 64 lanes, each sums every S-th product and a butterfly adds the S partial sums: log2 64 = 6
  additions on top of the (at most w) of a lane, so every sweep is a substitution in SOME summation order with at most w + 6 + 1
  operations per row and trsv_cases.bound's derivation holds with extra raised by 6.  Phase-1 rows of a supernode are pieces of
  original rows: the same bound.

  rows of an inverted supernode J (s rows, T the diagonal block of L or U on J; for U with the true pivots on its diagonal).  The
  device holds X = fl(T^-1), computed on the host by substitution, T X = I + R with |R| <= gamma_(s+1) |T| |X|, and forms
  x_J = fl(X t) = (X + dX) t with |dX| <= gamma_(s+6) |X|, t the phase-1 results.  Then T x_J - t = (R + T dX) t and
  |t| <= (1 + O(u)) |T| |x_J|, so the rows of J carry, on top of the plain bound, at most 2 (s + 6) u |T| |X| |T| |x_J|: the plain
  term |T| |x_J| is multiplied through |T| |T^-1|, and no multiple of |L| |U| |x| bounds it row by row.  With
  E = blockdiag over the supernodes of 2 (s + 6) |T| |T^-1| |T| (E_L from L, E_U from U; T^-1 by substitution in longdouble):

      |d - L U x| <= u (C g + 2 h),   g = |L| (|U| |x|),   h = E_L (|U| |x|) + |L| (E_U |x|),

  the factors 2 covering second order and the longdouble evaluation as in trsv_cases.bound.  Evaluated.ratio returns
  max_i |d - L U x|_i / (u (g + 2 h / C)_i), to be compared with C; without supernodes h = 0 and this is trsv_cases.Residual.ratio.

  two solutions of one system (transformed against untransformed, block sweep against single-vector solve).  L U (x_a - x_b) is the
  difference of the two residuals, so |L U (x_a - x_b)| <= u (C g_a + 2 h_a + C g_b + 2 h_b) row by row: Evaluated.difference
  returns the largest quotient, to be compared with 1.

Not covered: the 4096-level cap of one fused run (build_csr_schedule) needs roughly a 40 000-row 3-D block without supernodes, and
the 8192-workgroup cap of k_trsv_csr_level needs more than 32 768 rows in one level; both are beyond the 10 000 rows and the one
second of host factorisation every case here is held to."""
import functools

import numpy as np
import scipy.sparse as sp

from tests import trsv_cases as tc

LD = np.longdouble
U64 = 2.0 ** -53
SMALL_WG = 1024                  # TRSV_SMALL_WG of csrc/kernels.hpp: a level with m S <= 4 SMALL_WG is small
WG = 256
MAX_FUSED = 4096                 # levels of one k_trsv_csr_fused launch
BLOCK_PATH_MIN_BLOCKS, BLOCK_PATH_MIN_LEVELS = 4, 600   # direct_create_impl: nblocks >= 4 and nlev L + U > 600
PANEL = 256                      # CSR_PANEL_COLS of csrc/local_solve.hpp: columns of one panel of a block solve
OFF = 10 ** 6                    # DDM_DIRECT_SUPERNODE_MIN that switches the transformation off
MAX_N = 10000


def panels(nrhs):
    """(first column, width) of the column panels enqueue_csr_direct solves a block of nrhs columns in"""
    return [(c0, min(PANEL, nrhs - c0)) for c0 in range(0, nrhs, PANEL)]


def multi_threads_per_row(S, nrhs):
    """(Sm, rows per workgroup) of k_trsv_csr_level_multi for a level of S lanes per row (enqueue_multi_levels_csr)"""
    smax = 1
    while 2 * smax * nrhs <= WG and smax < 64:
        smax <<= 1
    Sm = min(S, smax)
    return Sm, WG // (Sm * nrhs)


# ---- the factor ------------------------------------------------------------------------------------------------------------------
class Factor:
    """what ddm.chol_host returns: perm[new] = old, the CSR pattern of L + U in the fill-reducing order and lu in the ILU(0)
    storage convention (multipliers below the diagonal, U above it, the inverse pivot on it)"""

    def __init__(self, f, block_ptr):
        self.perm = np.asarray(f["perm"], dtype=np.int64)
        self.rp, self.ci, self.lu = np.asarray(f["rowptr"], dtype=np.int64), np.asarray(f["col"], dtype=np.int64), np.asarray(f["lu"], dtype=np.float64)
        self.n = len(self.perm)
        self.block_ptr = np.asarray(block_ptr, dtype=np.int64)
        rows = np.repeat(np.arange(self.n), np.diff(self.rp))
        self.diag = np.flatnonzero(self.ci == rows)
        assert len(self.diag) == self.n and np.all(np.diff(self.ci)[np.diff(rows) == 0] > 0), "sorted rows, each with its diagonal"
        self.wL, self.wU = int(np.max(self.diag - self.rp[:-1])), int(np.max(self.rp[1:] - self.diag - 1))
        self.pattern = sp.csr_matrix((np.ones(len(self.ci)), self.ci, self.rp), shape=(self.n, self.n))


def supernode_runs(F, min_sn):
    """detect_supernodes: maximal runs [j0, j1) of consecutive rows with a dense diagonal block, of at least min_sn rows"""
    rp, ci, dg, n = F.rp, F.ci, F.diag, F.n
    runs = []
    j0 = 0
    while j0 < n:
        j1 = j0 + 1
        while j1 < n:
            w = j1 - j0
            if dg[j1] - rp[j1] < w or ci[dg[j1] - w] != j0:                       # row j1 holds columns j0 .. j1-1
                break
            if rp[j0 + 1] - dg[j0] - 1 < w or ci[dg[j0] + w] != j1:               # row j0 holds column j1
                break
            j1 += 1
        ok = j1 - j0 >= min_sn
        i = j0
        while ok and i < j1:                                                      # every row holds i+1 .. j1-1 behind its diagonal
            ok = rp[i + 1] - dg[i] - 1 >= j1 - 1 - i and (i == j1 - 1 or ci[dg[i] + (j1 - 1 - i)] == j1 - 1)
            i += 1
        if ok:
            runs.append((j0, j1))
        j0 = j1 if ok else j0 + 1
    return runs


def _dense_blocks(F, j0, j1, dtype):
    """(T_L, T_U) of the run: the unit lower block of L and the upper block of U with the true pivots 1 / lu_ii on its diagonal"""
    s = j1 - j0
    TL, TU = np.eye(s, dtype=dtype), np.zeros((s, s), dtype=dtype)
    for i in range(j0, j1):
        k = i - j0
        TL[k, :k] = F.lu[F.diag[i] - k:F.diag[i]]
        TU[k, k + 1:] = F.lu[F.diag[i] + 1:F.diag[i] + (j1 - i)]
        TU[k, k] = dtype(1) / dtype(F.lu[F.diag[i]])
    return TL, TU


def _inverses(TL, TU, dinv):
    """invert_supernodes, in the dtype of TL: row i of the inverse from the finished rows, Linv[i, :] = e_i - L[i, < i] Linv[< i, :]
    ascending and Uinv[i, :] = dinv_i (e_i - U[i, > i] Uinv[> i, :]) descending, dinv the stored inverse pivots (one product per
    row here, where the library subtracts row after row)"""
    s = TL.shape[0]
    Li, Ui = np.zeros_like(TL), np.zeros_like(TU)
    for i in range(s):
        Li[i, :i] = -(TL[i, :i] @ Li[:i, :i])
        Li[i, i] = 1
    for i in range(s - 1, -1, -1):
        Ui[i, i + 1:] = -(TU[i, i + 1:] @ Ui[i + 1:, i + 1:])
        Ui[i, i] = 1
        Ui[i, i:] *= dinv[i]
    return Li, Ui


# ---- the schedule ----------------------------------------------------------------------------------------------------------------
class Sweep:
    """one triangle's transformed rows in the order build_csr_schedule creates them (a valid order of substitution): row q writes
    unknown dst[q] = (rhs[q] >= 0 ? right-hand side rhs[q] : 0) - sum val x[col], times dinv[q]; and its levels"""

    def __init__(self, n, nvirt, rptr, col, val, dst, rhs, dinv, owner, block_ptr, per_block):
        self.n, self.nvirt = n, nvirt
        self.rptr, self.col, self.val = np.asarray(rptr, dtype=np.int64), col, val
        self.dst, self.rhs, self.dinv, self.owner = (np.asarray(a) for a in (dst, rhs, dinv, owner))
        nr = len(self.dst)
        level = np.zeros(n + nvirt, dtype=np.int64)
        for q in range(nr):
            c = col[self.rptr[q]:self.rptr[q + 1]]
            level[self.dst[q]] = level[c].max() + 1 if c.size else 0
        rlev = level[self.dst]
        self.blk_lev_ptr = None
        if per_block:                                            # levels numbered per block, blocks one after the other
            blk = np.searchsorted(block_ptr, self.owner, side="right") - 1
            nb = len(block_ptr) - 1
            mx = np.full(nb, -1, dtype=np.int64)
            np.maximum.at(mx, blk, rlev)
            self.blk_lev_ptr = np.concatenate([[0], np.cumsum(mx + 1)])
            rlev = rlev + self.blk_lev_ptr[blk]
            self.nlev = int(self.blk_lev_ptr[-1])
        else:
            self.nlev = int(rlev.max()) + 1
        self.rlev = rlev
        self.len = np.diff(self.rptr)
        self.m = np.bincount(rlev, minlength=self.nlev)
        self.entries = np.bincount(rlev, weights=self.len, minlength=self.nlev).astype(np.int64)
        S = np.ones(self.nlev, dtype=np.int64)
        for l in range(self.nlev):
            while S[l] < 64 and 4 * S[l] * self.m[l] < self.entries[l]:
                S[l] <<= 1
        self.S = S
        self.small = self.m * S <= 4 * SMALL_WG
        self.plan = []                                           # (first level, count, fused)
        l = 0
        while l < self.nlev:
            if self.small[l]:
                c = 0
                while l + c < self.nlev and c < MAX_FUSED and self.small[l + c]:
                    c += 1
                self.plan.append((l, c, True))
                l += c
            else:
                self.plan.append((l, 1, False))
                l += 1
        self.widest = int(self.len.max())

    def large(self):
        """levels that get a k_trsv_csr_level launch of their own"""
        return np.flatnonzero(~self.small)


class Table:
    def __init__(self, F, runs, L, U, min_sn, per_block):
        self.F, self.runs, self.L, self.U, self.min_sn, self.per_block = F, runs, L, U, min_sn, per_block
        self.nvirt = L.nvirt
        self.nblocks = len(F.block_ptr) - 1
        self.nlev = (L.nlev, U.nlev)

    def summary(self):
        out = [f"{len(self.runs)} supernodes (>= {self.min_sn} rows) with {self.nvirt} rows, largest {max([b - a for a, b in self.runs], default=0)}"]
        for tag, t in (("L", self.L), ("U", self.U)):
            lg = t.large()
            out.append(f"{tag}: {t.nlev} levels, {len(t.dst)} rows, widest {t.widest}, S {int(t.S.min())}..{int(t.S.max())}, plan of {len(t.plan)} launches, "
                       f"{len(lg)} large levels with S in {sorted(set(int(s) for s in t.S[lg]))}")
        return out


def block_path(table):
    """direct_create_impl's decision, on the table of GLOBAL levels: one workgroup per block (k_trsv_csr_blocks)"""
    assert not table.per_block
    return table.nblocks >= BLOCK_PATH_MIN_BLOCKS and sum(table.nlev) > BLOCK_PATH_MIN_LEVELS


def schedule_table(f, block_ptr, min_sn, per_block=False):
    """f: the dict of ddm.chol_host, or a Factor.  per_block: the schedule of the block path (levels renumbered per block)."""
    F = f if isinstance(f, Factor) else Factor(f, block_ptr)
    rp, ci, lu, dg, n = F.rp, F.ci, F.lu, F.diag, F.n
    runs = supernode_runs(F, max(2, int(min_sn)))
    sn_of = np.full(n, -1, dtype=np.int64)
    virt_of = np.full(n, -1, dtype=np.int64)
    nvirt = 0
    inv = []
    for q, (j0, j1) in enumerate(runs):
        sn_of[j0:j1] = q
        virt_of[j0:j1] = n + nvirt + np.arange(j1 - j0)
        nvirt += j1 - j0
        TL, TU = _dense_blocks(F, j0, j1, np.float64)
        inv.append(_inverses(TL, TU, lu[dg[j0:j1]]))
    sweeps_ = []
    for upper in (False, True):
        rptr, cols, vals, dst, rhs, dinv, owner = [0], [], [], [], [], [], []

        def row(c, v, d_, r_, dv, own):
            cols.append(c)
            vals.append(v)
            rptr.append(rptr[-1] + len(c))
            dst.append(d_)
            rhs.append(r_)
            dinv.append(dv)
            owner.append(own)

        def supernode(q):
            j0, j1 = runs[q]
            Ti = inv[q][1 if upper else 0]
            rng_ = range(j1 - 1, j0 - 1, -1) if upper else range(j0, j1)
            for i in rng_:                                       # phase 1: t_i = rhs_i - F[i, outside J] x
                a, b = (dg[i] + (j1 - i), rp[i + 1]) if upper else (rp[i], dg[i] - (i - j0))
                row(ci[a:b], lu[a:b], virt_of[i], i, 1.0, i)
            for i in rng_:                                       # phase 2: x_i = (T^-1 t)_i
                a, b = (i, j1) if upper else (j0, i + 1)
                row(virt_of[a:b], -Ti[i - j0, a - j0:b - j0], i, -1, 1.0, i)

        for i in (range(n - 1, -1, -1) if upper else range(n)):
            q = sn_of[i]
            if q >= 0:
                if i == (runs[q][1] - 1 if upper else runs[q][0]):
                    supernode(q)
                continue
            if upper:
                row(ci[dg[i] + 1:rp[i + 1]], lu[dg[i] + 1:rp[i + 1]], i, i, lu[dg[i]], i)
            else:
                row(ci[rp[i]:dg[i]], lu[rp[i]:dg[i]], i, i, 1.0, i)
        col = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
        val = np.concatenate(vals) if vals else np.zeros(0)
        sweeps_.append(Sweep(n, nvirt, rptr, col.astype(np.int64), val, dst, rhs, dinv, owner, F.block_ptr, per_block))
    return Table(F, runs, sweeps_[0], sweeps_[1], min_sn, per_block)


# ---- the float64 restatement of the solves ---------------------------------------------------------------------------------------
def sweeps(table, d, drop_last_of=None, stale_unknown=None, skip_dinv_of=None, full=False):
    """x = (L U)^-1 d as the device computes it, in float64 with sequential row sums: gather with perm, the lower and the upper
    sweep over the transformed rows, scatter.  full: (x, work block after the lower sweep, work block after the upper sweep).
    Three switches break it on purpose (`breakages` chooses where): the last operand of row drop_last_of of the lower sweep is
    dropped; the upper sweep's rows read unknown stale_unknown with the value it had before the upper sweep wrote it; the dinv
    factor of row skip_dinv_of of the upper sweep is skipped."""
    F = table.F
    work = np.zeros(F.n + table.nvirt)
    dp = np.asarray(d, dtype=np.float64)[F.perm]
    before = None
    for upper, S in ((False, table.L), (True, table.U)):
        if upper:
            before = work.copy()
        for q in range(len(S.dst)):
            a, b = S.rptr[q], S.rptr[q + 1]
            if not upper and q == drop_last_of:
                b -= 1
            c = S.col[a:b]
            xv = work[c]
            if upper and stale_unknown is not None:
                xv = np.where(c == stale_unknown, before[c], xv)
            s = np.cumsum(S.val[a:b] * xv)[-1] if b > a else 0.0  # cumsum adds in order
            r = S.rhs[q]
            t = ((work[r] if upper else dp[r]) if r >= 0 else 0.0) - s
            work[S.dst[q]] = t * S.dinv[q] if upper and q != skip_dinv_of else t
    x = np.empty(F.n)
    x[F.perm] = work[:F.n]
    return (x, before, work) if full else x


def breakages(table, d):
    """Where the three breakages of `sweeps` are applied, chosen from one intact run so that each changes the arithmetic (the
    Dirichlet rows of the Poisson matrices are identity rows: their factor entries are structural zeros and their unknowns keep the
    value of d through both sweeps): the widest row of the lower sweep whose last operand is a non-zero product; the unknown --
    a virtual one where the table has any -- read by the upper sweep whose value changes most in the upper sweep; the plain row of
    the upper sweep whose result the factor changes most (a Dirichlet row has the pivot 1)."""
    F, L, U = table.F, table.L, table.U
    _, lower, final = sweeps(table, d, full=True)
    last = L.rptr[1:] - 1
    live = np.flatnonzero(L.len > 0)
    live = live[(L.val[last[live]] != 0) & (lower[L.col[last[live]]] != 0)]
    drop = int(live[np.argmax(L.len[live])])
    read = np.unique(U.col)
    if table.nvirt:
        read = read[read >= F.n]
    stale = int(read[np.argmax(np.abs(final[read] - lower[read]))])
    plain = np.flatnonzero((U.rhs >= 0) & (U.dst < F.n))
    skip = int(plain[np.argmax(np.abs(final[U.dst[plain]] * (1.0 / U.dinv[plain] - 1.0)))])
    return {"dropped operand": dict(drop_last_of=drop), "stale unknown": dict(stale_unknown=stale), "skipped dinv": dict(skip_dinv_of=skip)}, \
        {"dropped operand": f"row {drop} of {int(L.len[drop])} entries (widest: {L.widest})", "stale unknown": f"unknown {stale} (n = {F.n})",
         "skipped dinv": f"row {skip}"}


# ---- the residual ----------------------------------------------------------------------------------------------------------------
class Evaluated:
    """d - L U x (formed in long double) and the terms g, h of the module docstring for one vector or the columns of a block, in the
    fill-reducing order"""

    def __init__(self, r, g, h):
        self.r, self.g, self.h = r, g, h

    def ratio(self, C, u=U64):
        """max_i |d - L U x|_i / (u (g + 2 h / C)_i) per column (a float for one vector), to be compared with C; inf where x has
        an entry that is not finite"""
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.abs(self.r) / (u * (self.g + 2 * self.h / C))
        q = np.where(np.isfinite(q), q, np.inf).max(axis=0)
        return float(q) if q.ndim == 0 else q.astype(np.float64)

    def difference(self, other, Ca, Cb, u=U64):
        """max_i |L U (x_a - x_b)|_i / (u (C_a g_a + 2 h_a + C_b g_b + 2 h_b)_i) per column for two solutions of the same system,
        to be compared with 1: L U (x_a - x_b) = r_b - r_a"""
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.abs(self.r - other.r) / (u * (Ca * self.g + 2 * self.h + Cb * other.g + 2 * other.h))
        q = np.where(np.isfinite(q), q, np.inf).max(axis=0)
        return float(q) if q.ndim == 0 else q.astype(np.float64)


class Residual:
    """L U x = d against one factor array lu (trsv_cases.Residual's convention) in the fill-reducing order; d and x are passed
    un-permuted, one vector or (n, m) blocks.  d - L (U x) is formed in long double (orc_lu_residual_ld of oracle/kernels.c, the
    columns in parallel; numpy's longdouble is that type) and kept rounded to double; g and h, sums of non-negative terms that only
    scale the bound, in float64 (relative error below 10^-12); T^-1 of E by substitution in numpy.longdouble."""

    def __init__(self, F, lu, runs):
        self.F, self.perm = F, F.perm
        self.lu = lu = np.ascontiguousarray(lu, dtype=np.float64)
        assert lu.shape == F.lu.shape
        G = F if lu is F.lu else Factor({"perm": F.perm, "rowptr": F.rp, "col": F.ci, "lu": lu}, F.block_ptr)
        rows = np.repeat(np.arange(F.n), np.diff(F.rp))
        piv = np.abs(lu)
        piv[F.diag] = 1.0 / piv[F.diag]                                  # the true pivot: lu holds its inverse
        unit = np.abs(lu)
        unit[F.diag] = 1.0

        def tri(mask, vals):
            rp = np.concatenate([[0], np.cumsum(np.bincount(rows[mask], minlength=F.n))])
            return sp.csr_matrix((vals[mask], F.ci[mask], rp), shape=(F.n, F.n))

        self.aL, self.aU = tri(F.ci <= rows, unit), tri(F.ci >= rows, piv)   # |L| with its unit diagonal, |U|
        EL, EU, at = [], [], []
        for j0, j1 in runs:
            TL, TU = _dense_blocks(G, j0, j1, LD)
            Li, Ui = _inverses(TL, TU, LD(1) / np.diag(TU))
            aTL, aLi, aTU, aUi = (np.abs(a).astype(np.float64) for a in (TL, Li, TU, Ui))
            k = 2.0 * (j1 - j0 + 6)
            EL.append(k * (aTL @ aLi @ aTL))
            EU.append(k * (aTU @ aUi @ aTU))
            at.append(j0)
        self.EL, self.EU = (self._blockdiag(F.n, at, E) for E in (EL, EU))

    @staticmethod
    def _blockdiag(n, at, blocks):
        """the sparse (n, n) matrix with the dense blocks on the diagonal at the rows `at`"""
        if not blocks:
            return sp.csr_matrix((n, n))
        ri = np.concatenate([np.repeat(j0 + np.arange(B.shape[0]), B.shape[0]) for j0, B in zip(at, blocks)])
        cj = np.concatenate([np.tile(j0 + np.arange(B.shape[0]), B.shape[0]) for j0, B in zip(at, blocks)])
        return sp.csr_matrix((np.concatenate([B.ravel() for B in blocks]), (ri, cj)), shape=(n, n))

    def evaluate(self, d, x):
        from oracle import apply_oracle as ao
        F = self.F
        d, x = np.asarray(d, dtype=np.float64)[self.perm], np.asarray(x, dtype=np.float64)[self.perm]
        xt, dt = np.ascontiguousarray(x.T), np.ascontiguousarray(d.T)    # a vector contiguous
        rt = np.empty_like(xt)
        ao.lib().orc_lu_residual_ld(F.n, ao._p(F.rp), ao._p(F.ci), ao._p(self.lu), ao._p(F.diag), xt.size // F.n, ao._p(xt), ao._p(dt), ao._p(rt))
        with np.errstate(invalid="ignore", over="ignore"):
            ax = np.abs(x)
            aUx = self.aU @ ax
            g = self.aL @ aUx
            h = self.EL @ aUx + self.aL @ (self.EU @ ax)
        return Evaluated(rt.T, g, h)

    def ratio(self, d, x, C):
        return self.evaluate(d, x).ratio(C)


# ---- the matrices ----------------------------------------------------------------------------------------------------------------
def _pkg():
    """the product package (directory dune-ddm_amd/, imported as dune_ddm_amd)"""
    import __graft_entry__ as ge
    return ge.import_package()


def _poisson(N, P, overlap):
    _pkg()
    from dune_ddm_amd import synth
    return tc._diag_blocks(tc._structured_blocks(synth.StructuredPoisson(N, P), overlap))


def _dg(k):
    _pkg()
    from dune_ddm_amd import synth
    return tc._diag_blocks(tc._structured_blocks(synth.StructuredDG2D((k, k), (2, 2)), 2))


def _uneven5():
    """an 11 x 10 x 9 block, a one-row block, a 30 x 28 block, a 5-row tridiagonal block, the 11 x 10 x 9 block again"""
    p3 = _poisson((11, 10, 9), (1, 1, 1), 1)[0]
    p2 = _poisson((30, 28), (1, 1), 1)[0]
    one = sp.csr_matrix(np.array([[2.0]]))
    tri = sp.diags([-np.ones(4), 2.0 * np.ones(5), -np.ones(4)], [-1, 0, 1], format="csr")
    return tc._diag_blocks([p3, one, p2, tri, p3])


DG_ROWS_K = 43                   # StructuredDG2D((k, k), (2, 2)): k = 24 has 392 levels, 32: 480, 40: 592, 42: 584, 43: 616 (9508 rows)

_MATRICES = {
    "poisson8": lambda: _poisson((17, 16, 15), (2, 2, 2), 2),
    "uneven5": _uneven5,
    "three": lambda: _poisson((24, 16, 15), (3, 1, 1), 2),
    "one": lambda: _poisson((13, 12, 11), (1, 1, 1), 1),
    "dg24": lambda: _dg(24),
    "dg_rows": lambda: _dg(DG_ROWS_K),
}
# name: (matrix, DDM_DIRECT_SUPERNODE_MIN, general)
_CASES = {
    "sn8": ("poisson8", 8, False),
    "rows8": ("poisson8", OFF, False),
    "uneven5": ("uneven5", OFF, False),
    "uneven5_sn": ("uneven5", 8, False),
    "three": ("three", OFF, False),
    "one": ("one", OFF, False),
    "pairs": ("poisson8", 2, False),
    "dg": ("dg24", 8, True),
    "dg_rows": ("dg_rows", OFF, True),
}
NAMES = tuple(_CASES)


@functools.lru_cache(maxsize=None)
def matrix(key):
    """(M, block_ptr, Factor by general flag) of one matrix; the host factor is computed once per (matrix, general)"""
    M, bp = _MATRICES[key]()
    assert M.has_sorted_indices and M.shape[0] <= MAX_N
    return M, bp


@functools.lru_cache(maxsize=None)
def factor(key, general):
    M, bp = matrix(key)
    return Factor(_pkg().chol_host(M, bp, general=general), bp)


class Case:
    def __init__(self, name):
        self.name = name
        self.key, self.min_sn, self.general = _CASES[name]
        self.M, self.block_ptr = matrix(self.key)
        self.n = self.M.shape[0]
        self.F = factor(self.key, self.general)
        self.table = schedule_table(self.F, self.block_ptr, self.min_sn)
        self.blocks = block_path(self.table)
        self.btable = schedule_table(self.F, self.block_ptr, self.min_sn, per_block=True) if self.blocks else None
        self.C = tc.bound(self.F, extra=9)
        self.res = Residual(self.F, self.F.lu, self.table.runs)

    def env(self, monkeypatch):
        monkeypatch.setenv("DDM_DIRECT_ENGINE", "host")
        monkeypatch.setenv("DDM_DIRECT_SUPERNODE_MIN", str(self.min_sn))

    def residual(self, lu):
        """the Residual of the library's own factor array (this case's, where the arrays are equal)"""
        return self.res if np.array_equal(lu, self.F.lu) else Residual(self.F, lu, self.table.runs)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---- the branch conditions -------------------------------------------------------------------------------------------------------
def _large_S(c):
    return set(int(s) for t in (c.table.L, c.table.U) for s in t.S[t.large()])


def _fused_runs(t):
    return [p for p in t.plan if p[2]]


def _large_between_fused(t):
    return any(t.plan[i - 1][2] and not t.plan[i][2] and t.plan[i + 1][2] for i in range(1, len(t.plan) - 1))


def _block_sizes(c):
    return [int(b) for b in np.diff(c.block_ptr)]


def _one_launch_per_sweep(c):
    return all(len(t.plan) == 1 and t.plan[0][2] for t in (c.table.L, c.table.U))


def _block_levels(c, b):
    """(L, U) levels of block b in the per-block schedule"""
    return tuple(int(t.blk_lev_ptr[b + 1] - t.blk_lev_ptr[b]) for t in (c.btable.L, c.btable.U))


def _run_sizes(c):
    return [b - a for a, b in c.table.runs]


PRECONDITIONS = {
    "sn8": [
        ("8 blocks, 9240 rows, 68 levels: the block path is not taken", lambda c: len(_block_sizes(c)) == 8 and c.n == 9240 and sum(c.table.nlev) == 68 and not c.blocks),
        ("large levels (k_trsv_csr_level) with S = 4 .. 64 in both sweeps", lambda c: {4, 8, 16, 32, 64} <= _large_S(c) and
         all(len(t.large()) >= 5 for t in (c.table.L, c.table.U))),
        ("fused runs between the large levels", lambda c: all(_large_between_fused(t) for t in (c.table.L, c.table.U))),
        ("supernodes found and inverted", lambda c: c.table.nvirt > 0 and min(_run_sizes(c)) >= 8),
    ],
    "rows8": [
        ("8 blocks, 926 levels: the block path", lambda c: len(_block_sizes(c)) == 8 and sum(c.table.nlev) == 926 and c.blocks),
        ("no supernode, rows up to 605 entries", lambda c: c.table.nvirt == 0 and max(c.F.wL, c.F.wU) == 605),
        ("S from 1 to 64 in the per-block schedule", lambda c: {1, 2, 4, 8, 16, 32, 64} <= set(int(s) for t in (c.btable.L, c.btable.U) for s in t.S)),
        ("every block has its own run of levels, together more than the global count", lambda c: all(min(_block_levels(c, b)) > 1 for b in range(8)) and
         c.btable.L.nlev > c.table.L.nlev),
    ],
    "uneven5": [
        ("5 blocks of 990, 1, 840, 5, 990 rows", lambda c: _block_sizes(c) == [990, 1, 840, 5, 990]),
        ("680 levels: the block path", lambda c: sum(c.table.nlev) == 680 and c.blocks and c.table.nvirt == 0),
        ("the one-row block has one level of one empty row", lambda c: _block_levels(c, 1) == (1, 1) and
         all(t.entries[t.blk_lev_ptr[1]] == 0 and t.m[t.blk_lev_ptr[1]] == 1 for t in (c.btable.L, c.btable.U))),
        ("the 5-row block has at most 5 levels", lambda c: all(2 <= l <= 5 for l in _block_levels(c, 3))),
    ],
    "uneven5_sn": [
        ("5 blocks of 990, 1, 840, 5, 990 rows", lambda c: _block_sizes(c) == [990, 1, 840, 5, 990]),
        ("supernodes of different sizes", lambda c: len(set(_run_sizes(c))) >= 3 and min(_run_sizes(c)) >= 8),
        ("the one-row and the 5-row block are too small to hold one", lambda c: all(not (c.block_ptr[1] <= a < c.block_ptr[2] or c.block_ptr[3] <= a < c.block_ptr[4])
                                                                                  for a, _ in c.table.runs)),
        ("every large block holds some", lambda c: all(any(c.block_ptr[b] <= a < c.block_ptr[b + 1] for a, _ in c.table.runs) for b in (0, 2, 4))),
    ],
    "three": [
        ("3 blocks, 1476 levels: not the block path", lambda c: len(_block_sizes(c)) == 3 and sum(c.table.nlev) == 1476 and not c.blocks),
        ("one fused launch per sweep", _one_launch_per_sweep),
    ],
    "one": [
        ("one block, 611 + 611 levels", lambda c: len(_block_sizes(c)) == 1 and c.table.nlev == (611, 611) and not c.blocks),
        ("one fused launch per sweep", _one_launch_per_sweep),
    ],
    "pairs": [
        ("631 supernodes of 2 rows and more", lambda c: len(c.table.runs) == 631 and min(_run_sizes(c)) == 2),
        ("most rows transformed: the largest nvirt of all cases", lambda c: 2 * c.table.nvirt > c.n and
         all(c.table.nvirt >= case(o).table.nvirt for o in NAMES)),
        ("more rows with rhs = -1 than plain rows", lambda c: all(int((t.rhs < 0).sum()) > int(((t.rhs >= 0) & (t.dst < c.n)).sum()) for t in (c.table.L, c.table.U))),
    ],
    "dg": [
        ("4 blocks, general factor with non-symmetric values", lambda c: len(_block_sizes(c)) == 4 and c.general and abs(c.M - c.M.T).max() > 1e-3 * abs(c.M).max()),
        ("44 levels: not the block path", lambda c: sum(c.table.nlev) == 44 and not c.blocks),
        ("plain rows in the upper sweep: dinv is applied", lambda c: int(((c.table.U.rhs >= 0) & (c.table.U.dst < c.n)).sum()) > 0 and c.table.nvirt > 0),
        ("large levels in both sweeps", lambda c: all(len(t.large()) >= 5 for t in (c.table.L, c.table.U))),
    ],
    "dg_rows": [
        ("4 blocks, general factor with non-symmetric values", lambda c: len(_block_sizes(c)) == 4 and c.general and abs(c.M - c.M.T).max() > 1e-3 * abs(c.M).max()),
        ("more than 600 levels: the block path", lambda c: sum(c.table.nlev) > 600 and c.blocks and c.table.nvirt == 0),
        ("k - 1 does not take it (k = 24 .. 42 were searched when the case was fixed: 392 .. 592 levels)", lambda c: not _dg_takes_block_path(DG_ROWS_K - 1)),
    ],
}
assert set(PRECONDITIONS) == set(NAMES)


def _dg_takes_block_path(k):
    M, bp = _dg(k)
    return block_path(schedule_table(_pkg().chol_host(M, bp, general=True), bp, OFF))
