"""Matrices, shape records, a SciPy / numpy reference factor and the residual bound shared by tests/test_sn_cases_reference.py (CPU)
and tests/test_gpu_sn_routes.py (GPU): the solves of the DEVICE supernodal factor (csrc/sn_chol.hpp, sn_solve1.hpp, sn_factor.hpp)
without iterative refinement, on every route the host driver can take.  Nothing here needs a GPU.

`Symbolic` puts what ddm.sn_symbolic_host returns per block into the global numbering sn::build uses.  `Shapes` restates, from
those arrays alone and without calling any plan code of the library, the branch conditions of decide_top_levels, build_chains,
solve_t, factorize and reserve: columns nc and rows nr per supernode, row tiles T = ceil(nr / 64), supernodes per level, ltop / ntop
for a DDM_SN_TOP_MAX, the kernel of every bottom level (small / <64> / <128>), the "big" supernodes (T > BWD_SMALL), the chains of
the top levels and their links.  (decide_top_levels also asks the device for a co-resident grid of 8 .. 1024 workgroups of 512
threads; an MI355X gives 512.  The colours of a level are not restated: the host reports none.)  `single_vector_plan` /
`block_plan` list the kernels a route launches, level by level.

The reference (`Reference`): the factor of P A P^T, P the library's permutation, WITHOUT pivoting (L U: of Q P A P^T, Q the row
exchanges the device's threshold rule makes inside the diagonal blocks -- none for lu13 / lu17) on the library's supernodal pattern, right-looking in float64 with numpy / scipy.linalg only (dense Cholesky or unpivoted L U of a diagonal block, triangular
SUBSTITUTION for the rows below -- no inverse is formed); the two sweeps by substitution; the same solve repeated on residuals formed
in long double (`refined`) until the correction is at rounding level.

L U cases.  The values are non-symmetric on the symmetric pattern and strictly COLUMN diagonally dominant (|a_jj| > sum_i |a_ij|).
One step of Gaussian elimination keeps that property of the trailing matrix: for column j of the Schur complement,
sum_{i != j} |a_ij - a_ik a_kj / a_kk| <= sum_{i != j, k} |a_ij| + |a_kj| / |a_kk| (sum_{i != k} |a_ik| - |a_jk|)
< |a_jj| - |a_kj| + |a_kj| (1 - |a_jk| / |a_kk|) <= |a_jj - a_jk a_kj / a_kk|.  The diagonal entry is then the largest of its
column in every trailing matrix, in particular inside every diagonal block of a supernode, so the device's threshold test
(|a_kk| >= 0.1 max_i |a_ik|, k_sn_lu_diag) never exchanges a row and its factor is the unpivoted L U: the reference's.
`column_dominance` is asserted on the CPU.
Row-exchanging L U cases (lx13, lx17, lx21; `_row_exchanging`).  A is built from a permutation Q of rows INSIDE diagonal blocks
(pairs and 3-cycles) such that Q A is strictly column dominant while the entries Q moves off the diagonal are 100 times smaller
than their column's largest.  The argument above holds for Q A: the largest entry of every column of every trailing matrix of
Q A is the diagonal one, so the threshold test restricted to the block picks exactly Q and the device's factor is the unpivoted
L U of Q A, multipliers below 1, no growth.  `Reference` replays the rule (`threshold_pivots`) and eliminates D[piv] without
pivoting; the rows of the U panel and the gather of the right-hand side follow the order.  The bound below is then that of the
system (Q A) x = Q d, unchanged in form and derived as it stands, Q A being column dominant and eliminated without pivoting: row i
of it is row Q^-1(i) of A x = d, so g and h -- formed from the pivoted Ld, Ud of the units -- are mapped back through the orders
before they are compared with d - A x.  C keeps its value: w_L and w_U are maxima over the rows of the supernodal pattern, and an
exchange stays inside one supernode, whose columns share one row list and one dense U panel.

The bound (u = 2^-53; no number in it comes from the code under test).  Let w_L (w_U) be the largest number of entries of a row of
L (of U) in the supernodal pattern, diagonal included.  Every entry of the factors is a_ij minus at most w_L - 1 products and one
division, in SOME order of summation (matrix-core accumulators, partial sums per tile, colours: all are orders), so
|A - L U| <= gamma_(w_L) |L| |U| (Higham, Accuracy and Stability, 9.3); each sweep is a substitution in some order,
(L + dL) y = d with |dL| <= gamma_(w_L + 1) |L| and (U + dU) x = y with |dU| <= gamma_(w_U + 1) |U|.  Together, with 3 per pass for
the right-hand side, the pivot and the permutation-free copy, C = 2 (2 w_L + w_U + 9): |d - A x| <= u C g, g = |L| (|U| |x|), the
factor 2 covering the second-order terms, the long double evaluation and the difference between the device's and the reference's
rounded factors (g is formed from the reference's).
The device does not substitute inside a diagonal block: it holds explicit inverses X = fl(T^-1) of the diagonal blocks T of L and
of U (W_s = L_ss^-1, sn_chol.hpp) and multiplies -- in the panel of the factor (R_s <- R_s W_s^T; L U: both panels) and in each
sweep.  A product with X in place of a substitution with T of order s adds at most 2 (s + 6) u |T| |X| |T| per use to the plain
term (tests/direct_cases.py derives this for an inverse computed by substitution, T X = I + R with |R| <= gamma_(s+1) |T| |X|; the
device inverts 32 x 32 blocks by substitution and combines them by block products, for which the same form of bound is ASSUMED
here, the constant 6 and the factors 2 being the room left for it).  Each inverse is used twice (factor panel and sweep), so with
E = blockdiag over the units of 4 (s + 6) |T| |T^-1| |T| (E_L from L, E_U from U, T^-1 by substitution in float64: a relative
error of 10^-13 in a term that only scales the bound),

    |d - A x| <= u (C g + 2 h),    h = E_L (|U| |x|) + |L| (E_U |x|),

and Evaluated.ratio = max_i |d - A x|_i / (u (C g + 2 h)_i), to be compared with 1.  The units are the supernodes; where the top
levels run as dense chains (k_sn_top_chain) a chain of links is ONE inverted triangle and is one unit.  The diagonal blocks of a
chain's |T| |T^-1| |T| dominate those of its links entry by entry (the sum holds the links' term and further non-negative ones), so
the chain units also cover the links' inverses used in the factorisation.
Two solutions of one system: A (x_a - x_b) = r_b - r_a, so |A (x_a - x_b)| <= u (C g_a + 2 h_a + C g_b + 2 h_b) row by row;
Evaluated.difference returns the largest quotient, to be compared with 1."""
import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from tests import trsv_cases as tc

U64 = 2.0 ** -53
TILE = 64                        # sn_chol.hpp
SN_MAX_COLS = 128                # sn_chol_host.hpp
BWD_SMALL = 8                    # supernodes with more row tiles take the partial-product kernels of the backward sweep
BWD_ROWS = 256                   # rows of one partial product
UPD_BLOCK = 32                   # k_sn_diag inverts in 32 x 32 blocks
TOP_MAX = 128                    # decide_top_levels: default bound on the supernodes of a top level
TOP_MIN_LEVELS = 4               # fewer top levels are not worth the persistent launch
SMALL_NC, SMALL_NR = 64, 192     # solve_t: a level with lev_maxnc <= 64 and lev_maxnr <= 192 takes the one-wavefront kernels
PANEL = 48                       # columns of one panel of a block solve (ilu0_solve_multi_ld)
SPREAD_BYTES = 256e6             # build_top_plan: panel bytes per block above which fewer than 8 blocks are spread over all XCDs

# single-vector routes: the environment each is selected by (DDM_SN_TOP_MAX, DDM_SN_CHAINS, DDM_SN_TOP_SPREAD at creation,
# DDM_SN_SMALL_KERNELS when the solve is captured)
ROUTES = {
    "default": {},
    "links": {"DDM_SN_CHAINS": "0"},
    "levels": {"DDM_SN_TOP_MAX": "0"},
    "levels_nosmall": {"DDM_SN_TOP_MAX": "0", "DDM_SN_SMALL_KERNELS": "0"},
    "spread0": {"DDM_SN_TOP_SPREAD": "0"},
    "spread1": {"DDM_SN_TOP_SPREAD": "1"},
}
ROUTE_VARS = ("DDM_SN_TOP_MAX", "DDM_SN_CHAINS", "DDM_SN_TOP_SPREAD", "DDM_SN_SMALL_KERNELS")
WIDTHS_FULL = (1, 2, 5, 16, 17, 24, 47, 48, 49, 97)
WIDTHS_SHORT = (1, 17, 49)
MAX_WIDTH = max(WIDTHS_FULL)


def routes_of(nblocks):
    """the single-vector routes of a case: the spread switch only where fewer than 8 blocks leave it a choice"""
    return tuple(r for r in ROUTES if nblocks < 8 or not r.startswith("spread"))


def panels(nrhs):
    """(first column, width) of the column panels of a block solve"""
    return [(c0, min(PANEL, nrhs - c0)) for c0 in range(0, nrhs, PANEL)]


def mpad(w):
    """columns of the zero-padded LDS block of the block kernels: 16-column tiles of the matrix cores, at most SOLVE_MT = 3"""
    return 16 * -(-w // 16)


def _pkg():
    import __graft_entry__ as ge
    return ge.import_package()


# ---- the symbolic structure --------------------------------------------------------------------------------------------------------
class Symbolic:
    """sn::build's global structure: supernode s owns the columns [first[s], first[s + 1]) of the permuted matrix and the rows
    rows[rptr[s] : rptr[s + 1]] below them; perm[new] = old"""

    def __init__(self, M, block_ptr):
        bp = np.asarray(block_ptr, dtype=np.int64)
        per = _pkg().sn_symbolic_host(M, bp)
        self.n, self.nblocks = int(bp[-1]), len(bp) - 1
        first, nrow, rows, level, parent, block, perm = [], [], [], [], [], [], []
        self.entries = base = 0
        for b, d in enumerate(per):
            off = int(bp[b])
            first.append(off + d["first"][:-1].astype(np.int64))
            nrow.append(np.diff(d["rptr"]))
            rows.append(off + d["rows"].astype(np.int64))
            level.append(d["level"].astype(np.int64))
            parent.append(np.where(d["parent"] < 0, -1, base + d["parent"].astype(np.int64)))
            block.append(np.full(len(d["level"]), b, dtype=np.int64))
            perm.append(off + d["perm"].astype(np.int64))
            base += len(d["level"])
            self.entries += d["entries"]
        self.first = np.concatenate(first + [np.array([self.n], dtype=np.int64)])
        self.nr = np.concatenate(nrow).astype(np.int64)
        self.rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        self.level, self.parent, self.block, self.perm = (np.concatenate(a) for a in (level, parent, block, perm))
        self.nc = np.diff(self.first)
        self.nsn = len(self.nc)
        self.rptr = np.concatenate([[0], np.cumsum(self.nr)]).astype(np.int64)
        self.nlev = int(self.level.max()) + 1
        self.sn_of_col = np.repeat(np.arange(self.nsn), self.nc)
        assert sorted(self.perm.tolist()) == list(range(self.n)) and self.nc.min() >= 1 and self.nc.max() <= SN_MAX_COLS
        assert int(np.sum(self.nc * (self.nc + self.nr))) == self.entries
        par = self.parent
        assert np.all((par < 0) | (par > np.arange(self.nsn))), "children are numbered before their parents"

    def rows_of(self, s):
        return self.rows[self.rptr[s]:self.rptr[s + 1]]

    def row_widths(self):
        """(w_L, w_U): the largest number of entries of a row of L and of a row of U (= column of L) in the supernodal pattern"""
        wl = np.zeros(self.n, dtype=np.int64)
        np.add.at(wl, self.rows, np.repeat(self.nc, self.nr))
        wl += np.arange(self.n) - self.first[self.sn_of_col] + 1
        wu = self.first[self.sn_of_col + 1] - np.arange(self.n) + self.nr[self.sn_of_col]
        return int(wl.max()), int(wu.max())


class Shapes:
    """what the host driver decides from the symbolic structure, for one setting of DDM_SN_TOP_MAX / DDM_SN_CHAINS /
    DDM_SN_SMALL_KERNELS"""

    def __init__(self, S, top_max=TOP_MAX, chains=True, small_kernels=True, spread=None):
        self.S = S
        self.nc, self.nr = S.nc, S.nr
        self.T = -(-S.nr // TILE)
        self.nlev = S.nlev
        self.per_level = np.bincount(S.level, minlength=S.nlev)
        self.lev_maxnc = np.array([S.nc[S.level == l].max() for l in range(S.nlev)])
        self.lev_maxnr = np.array([S.nr[S.level == l].max() for l in range(S.nlev)])
        # decide_top_levels
        ltop = S.nlev
        while ltop > 0 and self.per_level[ltop - 1] <= top_max:
            ltop -= 1
        self.ntop = S.nlev - ltop if S.nlev - ltop >= TOP_MIN_LEVELS else 0
        self.ltop = ltop if self.ntop else S.nlev
        self.lbot = self.ltop
        # solve_t, single vector: the kernel of every bottom level
        self.small_kernels = small_kernels
        self.kind = ["small" if small_kernels and self.lev_maxnc[l] <= SMALL_NC and self.lev_maxnr[l] <= SMALL_NR else
                     ("<64>" if self.lev_maxnc[l] <= SMALL_NC else "<128>") for l in range(self.lbot)]
        self.big = self.T > BWD_SMALL
        self.big_per_level = np.bincount(S.level[self.big], minlength=S.nlev)
        self.max_big_tiles = max([int(np.sum(-(-S.nr[(S.level == l) & self.big] // BWD_ROWS))) for l in range(S.nlev)])   # reserve
        # build_top_plan: one group over all XCDs with write-through hand-overs, or block b on XCD b % 8
        self.spread = (S.nblocks < 8 and S.entries * 8.0 / max(1, S.nblocks) > SPREAD_BYTES) if spread is None else bool(spread)
        # build_chains: s -> s + 1 = parent(s) while the parent has no other child and is a top supernode of the same block
        self.chains = []
        if self.ntop and chains:
            nchild = np.bincount(S.parent[S.parent >= 0], minlength=S.nsn)
            done = np.zeros(S.nsn, dtype=bool)
            for s in range(S.nsn):
                if S.level[s] < self.ltop or done[s]:
                    continue
                cur = s
                done[s] = True
                while True:
                    p = S.parent[cur]
                    if p != cur + 1 or nchild[p] != 1 or S.level[p] < self.ltop or S.block[p] != S.block[s]:
                        break
                    done[p] = True
                    cur = p
                self.chains.append((s, cur - s + 1))
        self.max_links = max([k for _, k in self.chains], default=0)

    def levels(self):
        return {"small": self.kind.count("small"), "<64>": self.kind.count("<64>"), "<128>": self.kind.count("<128>")}

    def big_at_bottom(self):
        return int(np.sum(self.big & (self.S.level < self.lbot)))

    def units(self):
        """[first column, end column) of every explicitly inverted triangle of the single-vector solve: chains where there are any"""
        S = self.S
        inside = np.zeros(S.nsn, dtype=bool)
        out = []
        for s, k in self.chains:
            inside[s:s + k] = True
            out.append((int(S.first[s]), int(S.first[s + k])))
        out += [(int(S.first[s]), int(S.first[s + 1])) for s in np.flatnonzero(~inside)]
        return sorted(out)

    # factorisation classes
    def partial_inverse_block(self):
        """supernodes whose last 32-block of k_sn_diag's inverse is partial and not the first"""
        return np.flatnonzero((self.nc > UPD_BLOCK) & (self.nc % UPD_BLOCK != 0))

    def update_tile_rows(self):
        return int(self.T.max())

    def tiles_with_several_targets(self):
        """number of 64-row tiles (= 64-column tiles of k_sn_update) whose rows belong to more than one target supernode"""
        S, cnt = self.S, 0
        for s in np.flatnonzero(S.nr > 0):
            t = S.sn_of_col[S.rows_of(s)]
            for j in range(0, len(t), TILE):
                cnt += int(t[j:j + TILE].min() != t[j:j + TILE].max())
        return cnt


def shapes_for(S, route):
    env = ROUTES[route]
    return Shapes(S, top_max=int(env.get("DDM_SN_TOP_MAX", TOP_MAX)), chains=env.get("DDM_SN_CHAINS", "1") != "0",
                  small_kernels=env.get("DDM_SN_SMALL_KERNELS", "1") != "0", spread=int(env["DDM_SN_TOP_SPREAD"]) if "DDM_SN_TOP_SPREAD" in env else None)


def single_vector_plan(sh, general):
    """[(level or 'top', supernodes, widest, longest, kernels)] of one single-vector solve, plus the kernels of the setup"""
    lu = "<LU>" if general else ""
    out = []
    for l in range(sh.lbot):
        k = sh.kind[l]
        if k == "small":
            ks = ["k_sn_fwd1_small", "k_sn_bwd1_small"]
        else:
            ks = ["k_sn_fwd1" + k, "k_sn_bwd1_diag" + k] + (["k_sn_bwd1_partial" + k] if sh.big_per_level[l] else [])
        out.append((l, int(sh.per_level[l]), int(sh.lev_maxnc[l]), int(sh.lev_maxnr[l]), [q + lu for q in ks]))
    if sh.ntop:
        ks = ["k_sn_top_prologue"] + (["k_sn_top_chain" + lu, "k_chain_scatter" + lu] + (["k_chain_invert"] if sh.max_links > 1 else []) if sh.chains else ["k_sn_top1" + lu])
        out.append(("top", int(sh.per_level[sh.ltop:].sum()), int(sh.lev_maxnc[sh.ltop:].max()), int(sh.lev_maxnr[sh.ltop:].max()), ks))
    return out


def block_plan(sh, general):
    """kernels of a block solve (all levels, any width)"""
    lu = "<LU>" if general else ""
    ks = ["k_sn_fwd_diag" + lu, "k_sn_bwd_diag" + lu] + (["k_sn_fwd_update"] if sh.nr.max() > 0 else []) + (["k_sn_bwd_partial" + lu] if sh.big.any() else [])
    return ks


SOLVE_KERNELS = ("k_sn_fwd1<64>", "k_sn_fwd1<128>", "k_sn_bwd1_diag<64>", "k_sn_bwd1_diag<128>", "k_sn_bwd1_partial<64>", "k_sn_bwd1_partial<128>",
                 "k_sn_fwd1_small", "k_sn_bwd1_small", "k_sn_top_prologue", "k_sn_top1", "k_sn_top_chain", "k_chain_scatter", "k_chain_invert",
                 "k_sn_fwd_diag", "k_sn_fwd_update", "k_sn_bwd_partial", "k_sn_bwd_diag")


# ---- the reference factor ----------------------------------------------------------------------------------------------------------
def _lu_nopivot(D, tiny=0.0):
    """dense L U without pivoting, in place: unit lower L below the diagonal, U on and above it.  tiny > 0: a pivot that is exactly
    0.0 when it is reached is replaced by tiny (k_sn_lu_diag's static perturbation of a pivot column that vanishes)"""
    for k in range(D.shape[0]):
        if tiny > 0.0 and D[k, k] == 0.0:
            D[k, k] = tiny
        if k + 1 < D.shape[0]:
            D[k + 1:, k] /= D[k, k]
            D[k + 1:, k + 1:] -= np.outer(D[k + 1:, k], D[k, k + 1:])
    return D


PIVOT_THRESHOLD = 0.1            # LU_PIVOT_THRESHOLD of sn_chol.hpp (UMFPACK's default)


def threshold_pivots(D, tiny=0.0):
    """k_sn_lu_diag's choice of rows, replayed in float64 on the diagonal block D as it stands when its supernode is reached: the
    diagonal entry is kept when |a_kk| > 0 and |a_kk| >= 0.1 amax, amax the largest modulus in rows k .. nc - 1 of column k;
    otherwise the FIRST largest entry becomes the pivot and its row is exchanged with row k (whole rows: the multipliers already
    computed go with them).  A column that vanishes keeps its row (and gets the pivot tiny).
    Returns (piv, decisions): position k holds the row piv[k] of D; decisions[k] = (|a_kk| / amax, second largest candidate / amax,
    row exchanged?), NaN ratios for a vanishing column."""
    a = np.array(D, dtype=np.float64)
    nc = a.shape[0]
    piv = np.arange(nc)
    decisions = []
    for k in range(nc):
        col = np.abs(a[k:, k])
        imax = int(np.argmax(col))                                       # (the first of equal maxima, as the device's `v > amax`)
        amax, dg = float(col[imax]), float(col[0])
        p = k if dg > 0.0 and dg >= PIVOT_THRESHOLD * amax else k + imax
        if not amax > 0.0:
            a[k, k], p = tiny, k
            decisions.append((np.nan, np.nan, False))
        else:
            second = float(np.partition(col, -2)[-2]) if len(col) > 1 else 0.0
            decisions.append((dg / amax, second / amax, p != k))
        if p != k:
            a[[k, p]] = a[[p, k]]
            piv[[k, p]] = piv[[p, k]]
        if k + 1 < nc:
            a[k + 1:, k] /= a[k, k]
            a[k + 1:, k + 1:] -= np.outer(a[k + 1:, k], a[k, k + 1:])
    return piv, decisions


class Reference:
    """P A P^T = L U (general) or L L^T on the supernodal pattern in float64, right-looking.  Per supernode: Ld (nc x nc lower, unit
    diagonal when general), Ud (nc x nc upper), R = L[rows, s] (nr x nc), V = U[s, rows]^T (nr x nc; R itself for L L^T).
    general: the rows of every diagonal block are first put into the order `threshold_pivots` chooses on the block as it stands when
    its supernode is reached (piv[s]: position k holds the block's row piv[s][k]; the identity for the column dominant cases), then
    the block D[piv] is factorised WITHOUT pivoting, the columns of V_s are taken in that order, and `solve` gathers its right-hand
    side in that order when the forward sweep reaches s -- nothing is applied to the columns on the left, the device's convention
    (sn_chol.hpp, "L U variant").  With Q the product of these exchanges the factors are the unpivoted L U of Q P A P^T; the rows of
    R_s are still named by the rows of P A P^T (`abs_factors` and `unit_blocks` put them where Q sends them).
    pivoting = False leaves the replay out (every piv[s] the identity: the reference as it was before the exchanges were added).
    tiny: the pivot a vanishing column of a diagonal block gets.
    Mutants: skip_update = (s, r) leaves row rows(s)[r] out of the update supernode s sends to its ancestors; unpivoted_panel = s takes
    the columns of V_s in the order of the matrix."""

    def __init__(self, M, S, general, skip_update=None, pivoting=True, unpivoted_panel=None, tiny=0.0):
        self.S, self.general = S, general
        self.piv, self.decisions = [], []
        n, first, nc = S.n, S.first, S.nc
        Ap = sp.csc_matrix(sp.csr_matrix(M)[S.perm][:, S.perm])
        At = sp.csc_matrix(Ap.T) if general else None
        idx = [np.concatenate([np.arange(first[s], first[s + 1]), S.rows_of(s)]) for s in range(S.nsn)]
        P = [Ap[:, first[s]:first[s + 1]][idx[s]].toarray() for s in range(S.nsn)]
        V = [At[:, first[s]:first[s + 1]][S.rows_of(s)].toarray() for s in range(S.nsn)] if general else None
        self.Ld, self.Ud, self.R, self.V = [], [], [], []
        for s in range(S.nsn):
            k, rows = int(nc[s]), S.rows_of(s)
            D, A_rs = P[s][:k], P[s][k:]
            if general:
                piv, dec = threshold_pivots(D, tiny) if pivoting else (np.arange(k), [])
                self.piv.append(piv), self.decisions.append(dec)
                D = _lu_nopivot(D[piv] if pivoting else D.copy(), tiny)
                Ld, Ud = np.tril(D, -1) + np.eye(k), np.triu(D)
                R = sla.solve_triangular(Ud, A_rs.T, trans="T", lower=False).T if len(rows) else A_rs
                Vp = V[s][:, piv] if pivoting and unpivoted_panel != s else V[s]
                Vs = sla.solve_triangular(Ld, Vp.T, lower=True, unit_diagonal=True).T if len(rows) else V[s]
            else:
                self.piv.append(np.arange(k)), self.decisions.append([])
                Ld = np.linalg.cholesky(np.tril(D) + np.tril(D, -1).T)
                Ud = Ld.T
                R = sla.solve_triangular(Ld, A_rs.T, lower=True).T if len(rows) else A_rs
                Vs = R
            self.Ld.append(Ld), self.Ud.append(Ud), self.R.append(R), self.V.append(Vs)
            P[s] = None
            if not len(rows):
                continue
            Rm = R
            if skip_update is not None and skip_update[0] == s:
                Rm = R.copy()
                Rm[skip_update[1]] = 0.0
            W = Rm @ Vs.T                                                # [i, j] is subtracted from entry (rows[i], rows[j])
            t_of = S.sn_of_col[rows]
            cut = np.concatenate([[0], np.flatnonzero(np.diff(t_of)) + 1, [len(rows)]])
            for a, b in zip(cut[:-1], cut[1:]):
                t = int(t_of[a])
                cols = rows[a:b] - first[t]
                below = nc[t] + np.searchsorted(S.rows_of(t), rows[b:])
                assert np.array_equal(S.rows_of(t)[below - nc[t]], rows[b:]), "the rows of a child below a target are rows of the target"
                P[t][np.ix_(np.concatenate([cols, below]), cols)] -= W[a:, a:b]
                if general:
                    V[t][np.ix_(below - nc[t], cols)] -= W[a:b, b:].T
        self._abs = None
        # Q: position i of the eliminated matrix holds the row src[i] of P A P^T, which stands at pos[src[i]] = i
        self.src = np.concatenate([first[s] + self.piv[s] for s in range(S.nsn)]).astype(np.int64)
        self.pos = np.argsort(self.src)
        self.exchanging = np.array([not np.array_equal(p, np.arange(len(p))) for p in self.piv])

    # sparse |L| and |U| of Q P A P^T = L U: rows of L in the order of Q, columns of both in the permuted numbering
    def abs_factors(self):
        if self._abs is None:
            S = self.S
            ri, rl, cj, lv, uv = [], [], [], [], []
            for s in range(S.nsn):
                k = int(S.nc[s])
                col = np.arange(S.first[s], S.first[s + 1])
                idx = np.concatenate([col, S.rows_of(s)])
                ri.append(np.tile(idx, k)), cj.append(np.repeat(col, len(idx)))
                rl.append(np.tile(np.concatenate([col, self.pos[S.rows_of(s)]]), k))
                lv.append(np.abs(np.vstack([self.Ld[s], self.R[s]])).T.ravel())
                uv.append(np.abs(np.vstack([self.Ud[s].T, self.V[s]])).T.ravel())
            ri, rl, cj = np.concatenate(ri), np.concatenate(rl), np.concatenate(cj)
            aL = sp.csr_matrix((np.concatenate(lv), (rl, cj)), shape=(S.n, S.n))
            aU = sp.csr_matrix((np.concatenate(uv), (cj, ri)), shape=(S.n, S.n))
            self._abs = (aL, aU)
        return self._abs

    def solve(self, d, drop=None, no_pivot=None, no_exchange=None, inverse_exchange=None):
        """x = A^-1 d (one vector or the columns of a block) by the two substitutions in float64; the right-hand side of supernode s
        is gathered in the order piv[s] when the forward sweep reaches s.  Mutants: drop = (s, r, k): the entry R_s[r, k] of L is
        left out of the forward sweep; no_pivot = (s, k): the division by the pivot of column k of supernode s is left out of the
        backward sweep; no_exchange = s: the right-hand side of s is not gathered; inverse_exchange = s: it is gathered in the
        inverse of the order."""
        S = self.S
        y = np.array(np.asarray(d, dtype=np.float64)[S.perm])
        for s in range(S.nsn):
            a, b = S.first[s], S.first[s + 1]
            if self.exchanging[s] and no_exchange != s:
                y[a:b] = y[a:b][np.argsort(self.piv[s]) if inverse_exchange == s else self.piv[s]]
            y[a:b] = sla.solve_triangular(self.Ld[s], y[a:b], lower=True, unit_diagonal=self.general)
            if S.nr[s]:
                R = self.R[s]
                if drop is not None and drop[0] == s:
                    R = R.copy()
                    R[drop[1], drop[2]] = 0.0
                y[S.rows_of(s)] -= R @ y[a:b]
        for s in range(S.nsn - 1, -1, -1):
            a, b = S.first[s], S.first[s + 1]
            t = y[a:b] - self.V[s].T @ y[S.rows_of(s)] if S.nr[s] else y[a:b]
            if no_pivot is not None and no_pivot[0] == s:
                Ud, x = self.Ud[s], np.array(t)
                for i in range(b - a - 1, -1, -1):
                    x[i] = t[i] - Ud[i, i + 1:] @ x[i + 1:]
                    if i != no_pivot[1]:
                        x[i] = x[i] / Ud[i, i]
                y[a:b] = x
            else:
                y[a:b] = sla.solve_triangular(self.Ud[s], t, lower=False)
        x = np.empty_like(y)
        x[S.perm] = y
        return x

    def unit_blocks(self, units):
        """(E_L, E_U) of the module docstring for the units [c0, c1): sparse block diagonal matrices"""
        S = self.S
        at, EL, EU = [], [], []
        for c0, c1 in units:
            m = c1 - c0
            TL, TU = np.zeros((m, m)), np.zeros((m, m))
            for s in range(S.sn_of_col[c0], S.sn_of_col[c1 - 1] + 1):
                a, b = S.first[s] - c0, S.first[s + 1] - c0
                TL[a:b, a:b], TU[a:b, a:b] = self.Ld[s], self.Ud[s]
                rows = S.rows_of(s)
                ins = rows < c1                                          # the in-chain part of the rows below
                TL[self.pos[rows[ins]] - c0, a:b] = self.R[s][ins]     # (a row of a later link stands where that link's order puts it)
                TU[a:b, rows[ins] - c0] = self.V[s][ins].T
            eye = np.eye(m)
            Li = sla.solve_triangular(TL, eye, lower=True, unit_diagonal=self.general)
            Ui = sla.solve_triangular(TU, eye, lower=False)
            k = 4.0 * (m + 6)
            EL.append(k * (np.abs(TL) @ np.abs(Li) @ np.abs(TL)))
            EU.append(k * (np.abs(TU) @ np.abs(Ui) @ np.abs(TU)))
            at.append(c0)
        return _blockdiag(S.n, at, EL), _blockdiag(S.n, at, EU)


def _blockdiag(n, at, blocks):
    ri = np.concatenate([np.repeat(j0 + np.arange(B.shape[0]), B.shape[0]) for j0, B in zip(at, blocks)])
    cj = np.concatenate([np.tile(j0 + np.arange(B.shape[0]), B.shape[0]) for j0, B in zip(at, blocks)])
    return sp.csr_matrix((np.concatenate([B.ravel() for B in blocks]), (ri, cj)), shape=(n, n))


# ---- the residual ------------------------------------------------------------------------------------------------------------------
def residual_ld(M, d, x):
    """d - M x formed in long double (orc_csr_residual_ld of oracle/kernels.c), rounded to double; vectors or (n, m) blocks"""
    from oracle import apply_oracle as ao
    M = sp.csr_matrix(M)
    n = M.shape[0]
    rp, ci, va = np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.int32), np.ascontiguousarray(M.data, dtype=np.float64)
    xt, dt = np.ascontiguousarray(np.asarray(x, dtype=np.float64).T), np.ascontiguousarray(np.asarray(d, dtype=np.float64).T)
    rt = np.empty_like(xt)
    ao.lib().orc_csr_residual_ld(n, ao._p(rp), ao._p(ci), ao._p(va), xt.size // n, ao._p(xt), ao._p(dt), ao._p(rt))
    return rt.T


class Evaluated:
    """d - A x (long double, rounded) and the bound u (C g + 2 h) for one vector or the columns of a block"""

    def __init__(self, r, bound):
        self.r, self.bound = r, bound

    @staticmethod
    def _worst(num, den):
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(den > 0, np.abs(num) / den, np.where(num == 0, 0.0, np.inf))
        q = np.where(np.isfinite(q), q, np.inf).max(axis=0)
        return float(q) if q.ndim == 0 else q.astype(np.float64)

    def column(self, j):
        return Evaluated(self.r[:, j], self.bound[:, j])

    def ratio(self):
        """max_i |d - A x|_i / (u (C g + 2 h)_i) per column, to be compared with 1; inf where x is not finite"""
        return self._worst(self.r, self.bound)

    def difference(self, other):
        """max_i |A (x_a - x_b)|_i / (bound_a + bound_b)_i per column for two solutions of one system, to be compared with 1"""
        return self._worst(self.r - other.r, self.bound + other.bound)


# ---- the matrices ------------------------------------------------------------------------------------------------------------------
def _poisson(N, P, overlap=2):
    _pkg()
    from dune_ddm_amd import synth
    return tc._diag_blocks(tc._structured_blocks(synth.StructuredPoisson(N, P), overlap))


def _tridiagonal(m):
    return sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1], format="csr") if m > 1 else sp.csr_matrix(np.array([[2.0]]))


def _chain1d():
    """one block each of 1, 2 and 3 rows and a 300-row tridiagonal block"""
    return tc._diag_blocks([_tridiagonal(m) for m in (1, 2, 3, 300)])


def _column_dominant(MB, seed):
    """non-symmetric standard-normal values on the symmetrised pattern of the STORED entries of M off the diagonal (the Poisson
    matrices store the zeros that couple their Dirichlet rows: the supernodes stay those of M), the diagonal 1 + the column's sum of
    moduli"""
    M, bp = MB
    M = sp.csr_matrix(M)
    P = sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
    P = sp.csr_matrix(P + P.T)
    P.setdiag(0.0)
    P.eliminate_zeros()
    P.sort_indices()
    P.data = np.random.default_rng(seed).standard_normal(P.nnz)
    A = sp.csr_matrix(P + sp.diags(1.0 + np.asarray(abs(P).sum(axis=0)).ravel(), format="csr"))
    A.sort_indices()
    return A, bp


def column_dominance(M):
    """min_j (|a_jj| - sum_{i != j} |a_ij|) / |a_jj|: positive for a strictly column diagonally dominant matrix"""
    M = sp.csc_matrix(M)
    dg = np.abs(M.diagonal())
    return float(np.min((2.0 * dg - np.asarray(abs(M).sum(axis=0)).ravel()) / dg))


class Design:
    """the exchanges a row-exchanging case is built to make: groups = [(supernode, rows of its diagonal block)], a pair (k, p) or a
    3-cycle (k, p, q) in ascending order; src[i] = the row of P A P^T that the elimination puts into position i"""

    def __init__(self, groups, src):
        self.groups, self.src = groups, src

    def of(self, s):
        return [g for t, g in self.groups if t == s]


EXCHANGE_KINDS = ("pair", "several", "cycle", "straddle")


def _row_exchanging(MB, seed):
    """Non-symmetric values on the pattern of _column_dominant(MB), built so that the threshold pivoting of k_sn_lu_diag exchanges
    exactly the rows of `Design` and the factor has no growth.  Two of every three supernodes get groups of rows of their diagonal
    block, drawn (seeded) among the entries the pattern stores: a pair (k, p), k < p, with a_pk and a_kp stored, or a 3-cycle
    (k, p, q), k < p < q, with a_pk, a_qp, a_kq stored; by the kind drawn one pair, several disjoint groups (about one per eight
    columns), a 3-cycle, or a pair on either side of a multiple of 32 (of column 64 in every other supernode of more than 64
    columns); the pair of the first and the last column wherever the pattern stores it (a few supernodes of 8 columns).  Q sends the rows where the elimination will: pair k <-> p; cycle p -> k, q -> p,
    k -> q.  Off the diagonal the values are standard normal; the entries Q moves ONTO the diagonal (a_pk, a_kp; a_pk, a_qp, a_kq)
    are 2 (1 + the sum of the moduli of the other entries of their column), the entries it moves OFF it (a_kk, a_pp; and a_qq) are
    0.01 x standard normal, every other a_jj is 2 (1 + column sum).  A cycle is made in two exchanges, k <-> p and then p <-> q, and
    between them row k stands in position p: the second threshold test has a_kp on the diagonal, so a_kp is 0.01 x standard normal
    too (a standard normal a_kp reaches 0.1 of the 2 (1 + column sum) ~ 44 of a 27-point column, and the diagonal would be kept:
    seen at 0.102 in lx17 before this was added).  Q A is strictly column dominant, so (module docstring) the
    largest entry of every column of every trailing matrix of Q A is the diagonal one: the threshold test picks Q and nothing else,
    and the factor is the unpivoted L U of Q A with multipliers below 1.  Returns (A, block_ptr, Design)."""
    A0, bp = _column_dominant(MB, seed)
    S = Symbolic(A0, bp)
    n = S.n
    iperm = np.empty(n, dtype=np.int64)
    iperm[S.perm] = np.arange(n)
    C = sp.coo_matrix(A0)
    pi, pj = iperm[C.row], iperm[C.col]
    rng = np.random.default_rng(seed + 1000)
    lower = (S.sn_of_col[pi] == S.sn_of_col[pj]) & (pi > pj)
    by_sn = {}
    for i, j in zip(pi[lower], pj[lower]):
        by_sn.setdefault(int(S.sn_of_col[j]), []).append((int(j - S.first[S.sn_of_col[j]]), int(i - S.first[S.sn_of_col[j]])))
    groups = []
    for s in range(S.nsn):
        pairs = sorted(by_sn.get(s, []))
        if s % 3 == 0 or not pairs:
            continue
        nc = int(S.nc[s])
        adj = {}
        for k, p in pairs:
            adj.setdefault(k, set()).add(p), adj.setdefault(p, set()).add(k)
        order = [pairs[i] for i in rng.permutation(len(pairs))]
        kind = EXCHANGE_KINDS[int(rng.integers(len(EXCHANGE_KINDS)))]
        chosen = []
        if (0, nc - 1) in pairs:                                         # (rare -- a few supernodes of 8 columns: taken wherever it is stored)
            chosen = [(0, nc - 1)]
        elif kind == "straddle":
            at64 = [g for g in order if g[0] < 64 <= g[1]]
            at32 = [g for g in order if g[0] // 32 != g[1] // 32 and not g[0] < 64 <= g[1]]
            chosen = (at64 if s % 2 else at32)[:1] or (at32 + at64)[:1]
        elif kind == "cycle":
            for k, p in order:
                q = sorted(t for t in adj[k] & adj[p] if t > p)
                if q:
                    chosen = [(k, p, q[int(rng.integers(len(q)))])]
                    break
        elif kind == "several":
            used = set()
            for g in order:
                if len(chosen) < max(2, nc // 8) and not used & set(g):
                    chosen.append(g)
                    used |= set(g)
        groups += [(s, g) for g in (chosen or order[:1])]
    src = np.arange(n)
    for s, g in groups:
        f = int(S.first[s])
        src[[f + r for r in g]] = [f + r for r in g[1:] + g[:1]]       # pair: src[k] = p, src[p] = k; cycle: src[k] = p, src[p] = q, src[q] = k
    vals = np.array(C.data)
    moved = src != np.arange(n)
    off_diag = (pi == pj) & moved[pj]
    # (a cycle's first exchange puts row k into position p, so the second decision has a_kp on the diagonal: small like a_pp)
    a_kp = [(int(S.first[s]) + g[0]) * n + int(S.first[s]) + g[1] for s, g in groups if len(g) == 3]
    off_diag |= np.isin(pi * n + pj, a_kp)
    vals[off_diag] = 0.01 * rng.standard_normal(int(off_diag.sum()))
    onto = pi == src[pj]                                                 # the diagonal of Q A
    assert int(onto.sum()) == n, "the entries Q moves onto the diagonal are stored"
    vals[onto] = 0.0
    vals[onto] = 2.0 * (1.0 + np.bincount(pj, weights=np.abs(vals), minlength=n)[pj[onto]])
    A = sp.csr_matrix((vals, (C.row, C.col)), shape=A0.shape)
    A.sort_indices()
    assert A.nnz == A0.nnz and np.array_equal(A.indptr, A0.indptr) and np.array_equal(A.indices, A0.indices)
    return A, bp, Design(groups, src)


# No top levels in the DEFAULT configuration (fewer than four levels of at most 128 supernodes) and bottom levels of all three kinds.
# Searched among grids of 13 .. 26 points and 2 .. 6 parts per direction: 26 x 26 x 21 in 5 x 5 x 4 (76 176 rows) and
# 21 x 21 x 13 in 5 x 5 x 3 (38 663) have the property too; 21 x 21 x 9 in 5 x 5 x 2 (23 534) has no top levels but no <64> level either.
MANY_GRID, MANY_PARTS = (21, 17, 13), (5, 4, 3)

# name: (matrix, general, block widths)
_CASES = {
    "one21": (lambda: _poisson((21, 20, 19), (1, 1, 1)), False, WIDTHS_FULL),
    "many": (lambda: _poisson(MANY_GRID, MANY_PARTS), False, WIDTHS_FULL),
    "eight17": (lambda: _poisson((17, 16, 15), (2, 2, 2)), False, WIDTHS_SHORT),
    "twelve": (lambda: _poisson((19, 16, 15), (3, 2, 2)), False, WIDTHS_SHORT),
    "flat2d": (lambda: _poisson((70, 66), (2, 2)), False, WIDTHS_SHORT),
    "chain1d": (_chain1d, False, WIDTHS_FULL),
    "lu13": (lambda: _column_dominant(_poisson((13, 12, 11), (1, 1, 1)), 29), True, WIDTHS_FULL),
    "lu17": (lambda: _column_dominant(_poisson((17, 16, 15), (2, 2, 2)), 31), True, WIDTHS_SHORT),
    # rows ARE exchanged, without growth (_row_exchanging): the grids and blocks of lu13, lu17 and -- for supernodes with more than
    # BWD_SMALL row tiles, which those two do not have -- of one21
    "lx13": (lambda: _row_exchanging(_poisson((13, 12, 11), (1, 1, 1)), 37), True, WIDTHS_FULL),
    "lx17": (lambda: _row_exchanging(_poisson((17, 16, 15), (2, 2, 2)), 41), True, WIDTHS_SHORT),
    "lx21": (lambda: _row_exchanging(_poisson((21, 20, 19), (1, 1, 1)), 43), True, WIDTHS_SHORT),
}
EXCHANGING = ("lx13", "lx17", "lx21")
SAME_PATTERN = {"lx13": "lu13", "lx17": "lu17"}                          # the column dominant case on the same pattern
NAMES = tuple(_CASES)
# the matrices of tests/test_gpu_sn_chol.py: (levels, levels in the persistent top kernel, bottom levels small / <64> / <128>, big at the bottom)
EXISTING = {
    ((13, 12, 11), (1, 1, 1)): (10, 10, (0, 0, 0), 0),
    ((17, 16, 15), (2, 2, 2)): (8, 7, (1, 0, 0), 0),
    ((21, 20, 19), (1, 1, 1)): (19, 19, (0, 0, 0), 0),
    ((33, 31, 29), (2, 2, 2)): (15, 12, (1, 2, 0), 0),
    ((70, 66), (2, 2)): (9, 8, (1, 0, 0), 0),
}


def pivoting_matrix():
    """the "pivoting" matrix of tests/test_gpu_sn_chol.py::test_device_lu_matches_superlu: a 19 x 18 x 17 stencil block with
    non-symmetric values and a tiny diagonal in every third row, so that rows ARE exchanged; it needs refinement by design"""
    M, bp = _poisson((19, 18, 17), (1, 1, 1), overlap=1)
    rng = np.random.default_rng(11)
    M = sp.csr_matrix(sp.csr_matrix(M).tolil())                          # (that test's construction, step by step)
    M.data = M.data * (1.0 + 0.3 * rng.standard_normal(len(M.data)))
    d = M.diagonal()
    d[::3] *= 1e-6
    M.setdiag(d)
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M, bp


# ---- a pivot column that vanishes inside its diagonal block ---------------------------------------------------------------------------
# (supernode of lu13, column of its diagonal block): a leaf of the tree with rows below.  The multipliers of 1e6 under the replaced pivot
# take the column dominance from the ancestors' blocks, and most choices make the threshold test exchange rows there, some at ratios
# near 0.1; with this one the reference keeps every diagonal entry, the closest decision at 0.38 (tests/test_sn_cases_reference.py)
VANISHING = (6, 0)
SQRT_EPS = 2.0 ** -26            # sn_direct_create: tiny = sqrt(eps) max |a_ij|


def vanishing_column_matrix():
    """lu13's values with every entry of ONE column set to an explicit 0.0 inside the diagonal block of one supernode (the entries of
    the column below the block stay, so the matrix stays regular).  The supernode is a leaf, so nothing is added to its block before
    it is eliminated, and inside the block a column of zeros stays one (a_ij -= a_ik a_kj with a_kj = 0): when the elimination
    reaches it, k_sn_lu_diag finds amax = 0, writes tiny onto the diagonal and counts it.  Returns (M, block_ptr, tiny)."""
    c = case("lu13")
    S = c.S
    s, j = VANISHING
    assert S.level[s] == 0 and S.nr[s] > 0 and S.nc[s] >= 2 and j < S.nc[s]
    iperm = np.empty(c.n, dtype=np.int64)
    iperm[S.perm] = np.arange(c.n)
    M = sp.csr_matrix(c.M).copy()
    pi, pj = iperm[np.repeat(np.arange(c.n), np.diff(M.indptr))], iperm[M.indices]
    hit = (pj == S.first[s] + j) & (pi >= S.first[s]) & (pi < S.first[s + 1])
    assert hit.sum() >= 2 and np.all(M.data[hit] != 0.0)
    M.data[hit] = 0.0
    return M, c.block_ptr, SQRT_EPS * float(np.abs(M.data).max())


def probe_rhs(n):
    """the right-hand side of the refinement probe (sn_probe_refinement): a 64-bit linear congruential sequence mapped to [-1, 1)"""
    b, lcg = np.empty(n), 0x9E3779B97F4A7C15
    for i in range(n):
        lcg = (lcg * 6364136223846793005 + 1442695040888963407) % 2 ** 64
        b[i] = float(lcg >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0
    return b


def probe_omega(M, b, x):
    """the probe's backward error as include/ddm_hip.h states it: max(||b - A x|| / (||A||_inf ||x|| + ||b||), 0.01 max_i |b - A x|_i /
    (|A| |x| + |b|)_i)"""
    M = sp.csr_matrix(M)
    r = b - M @ x
    den = abs(M) @ np.abs(x) + np.abs(b)
    comp = float(np.max(np.abs(r)[den > 0] / den[den > 0]))
    return max(float(np.linalg.norm(r) / (abs(M).sum(axis=1).max() * np.linalg.norm(x) + np.linalg.norm(b))), 1e-2 * comp)


def predict_refinement(M, solve, max_steps=3):
    """(steps, [omega after 0, 1, .. steps]) of the rule of include/ddm_hip.h with `solve` in place of the device's sweeps: stop below
    1e-14 or when a step does not halve omega, at most 3 steps"""
    b = probe_rhs(M.shape[0])
    x = solve(b)
    om = [probe_omega(M, b, x)]
    while len(om) - 1 < max_steps:
        if om[-1] < 1e-14 or (len(om) > 1 and om[-1] > om[-2] / 2.0):
            break
        x = x + solve(b - M @ x)
        om.append(probe_omega(M, b, x))
    return len(om) - 1, om


class Case:
    def __init__(self, name):
        self.name = name
        make, self.general, self.widths = _CASES[name]
        self.M, self.block_ptr, self.design = (tuple(make()) + (None,))[:3]
        self.n, self.nblocks = self.M.shape[0], len(self.block_ptr) - 1
        self.S = Symbolic(self.M, self.block_ptr)
        self.routes = routes_of(self.nblocks)
        self.shapes = {r: shapes_for(self.S, r) for r in ROUTES}
        self.wL, self.wU = self.S.row_widths()
        self.C = 2 * (2 * self.wL + self.wU + 9)
        self.D = np.random.default_rng(101 + NAMES.index(name)).standard_normal((self.n, MAX_WIDTH))   # the fixed right-hand sides
        self.d = np.ascontiguousarray(self.D[:, 0])

    @functools.cached_property
    def ref(self):
        return Reference(self.M, self.S, self.general)

    @functools.lru_cache(maxsize=None)
    def _E(self, units):
        return self.ref.unit_blocks(units)

    def units(self, route=None):
        """the inverted triangles of a single-vector route; None: the supernodes (block solves, the reference)"""
        sh = self.shapes["links" if route is None else route]
        return tuple(sh.units())

    def evaluate(self, d, x, route=None):
        S = self.S
        aL, aU = self.ref.abs_factors()
        EL, EU = self._E(self.units(route))
        with np.errstate(invalid="ignore", over="ignore"):
            ax = np.abs(np.asarray(x, dtype=np.float64))[S.perm]
            aUx = aU @ ax
            bound = np.empty_like(ax)                                    # row i of Q P A P^T x = Q P d is row perm[src[i]] of A x = d
            bound[S.perm[self.ref.src]] = U64 * (self.C * (aL @ aUx) + 2.0 * (EL @ aUx + aL @ (EU @ ax)))
        return Evaluated(residual_ld(self.M, d, x), bound)

    def refined(self, d, steps=3):
        """the reference solution made accurate: corrections from residuals in long double until they are at rounding level"""
        x = self.ref.solve(d)
        for _ in range(steps):
            x = x + self.ref.solve(residual_ld(self.M, d, x))
        return x

    def env(self, monkeypatch, route="default", refine="off"):
        monkeypatch.setenv("DDM_DIRECT_ENGINE", "device")
        monkeypatch.setenv("DDM_DIRECT_REFINE", refine) if refine is not None else monkeypatch.delenv("DDM_DIRECT_REFINE", raising=False)
        set_route(monkeypatch, route)


def set_route(monkeypatch, route):
    for v in ROUTE_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def mutants(c, seed=5):
    """One seeded pick per kind among the places where the mutant changes the arithmetic of the intact reference solve of c.d (the
    Dirichlet rows of the Poisson matrices are identity rows: their factor entries are structural zeros):
    (kind, description, solution of the mutant)."""
    S, ref = c.S, c.ref
    rng = np.random.default_rng(seed)
    x = ref.solve(c.d)
    xp = x[S.perm]
    with_rows = np.flatnonzero(S.nr > 0)
    out = []
    while True:                                                          # a non-zero entry of L below a diagonal block, times a non-zero y
        s = int(rng.choice(with_rows))
        r, k = int(rng.integers(S.nr[s])), int(rng.integers(S.nc[s]))
        if abs(ref.R[s][r, k]) * abs(xp[S.first[s] + k]) > 1e-6 * np.abs(xp).max():
            break
    out.append(("dropped entry of L", f"L[{S.rows_of(s)[r]}, {S.first[s] + k}] = {ref.R[s][r, k]:.3g} (supernode {s})", ref.solve(c.d, drop=(s, r, k))))
    while True:                                                          # a row of an update that is not a row of zeros
        s = int(rng.choice(with_rows))
        r = int(rng.integers(S.nr[s]))
        if np.abs(ref.R[s][r]).max() > 1e-3 and np.abs(ref.V[s]).max() > 1e-3:
            break
    out.append(("skipped row of an update", f"row {S.rows_of(s)[r]} of the update of supernode {s} ({S.nc[s]} columns, {S.nr[s]} rows)",
                Reference(c.M, S, c.general, skip_update=(s, r)).solve(c.d)))
    while True:                                                          # a pivot that is not 1, of an unknown that is not 0
        s = int(rng.integers(S.nsn))
        k = int(rng.integers(S.nc[s]))
        if abs(ref.Ud[s][k, k] - 1.0) > 0.1 and abs(xp[S.first[s] + k]) > 1e-3 * np.abs(xp).max():
            break
    out.append(("pivot not applied", f"column {S.first[s] + k} (pivot {ref.Ud[s][k, k]:.3g}, supernode {s})", ref.solve(c.d, no_pivot=(s, k))))
    if c.design is None:
        return out
    # the consumers of the pivot order: one exchanging supernode; then a supernode with a 3-cycle (where the order and its inverse
    # differ) and rows below (a U panel)
    s = int(rng.choice(np.flatnonzero(ref.exchanging)))
    out.append(("exchange not applied", f"supernode {s} ({S.nc[s]} columns, groups {c.design.of(s)})", ref.solve(c.d, no_exchange=s)))
    s = int(rng.choice([t for t, g in c.design.groups if len(g) == 3 and S.nr[t] > 0]))
    out.append(("inverse exchange applied", f"supernode {s} ({S.nc[s]} columns, groups {c.design.of(s)})", ref.solve(c.d, inverse_exchange=s)))
    out.append(("U panel in unpivoted order", f"supernode {s} ({S.nr[s]} rows below)", Reference(c.M, S, c.general, unpivoted_panel=s).solve(c.d)))
    return out


PIVOT_MUTANTS = ("exchange not applied", "inverse exchange applied", "U panel in unpivoted order")
