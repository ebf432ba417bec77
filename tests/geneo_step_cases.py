"""Inputs, restated dispatch conditions and host references shared by tests/test_geneo_step_cases_reference.py (CPU) and
tests/test_gpu_geneo_steps.py (GPU): the device steps of the GenEO block eigensolver (GeneoRun, csrc/geneo.hpp) one by one, on
the eigensolver's own layout.  Nothing here needs a GPU.

Layout.  A block is n x 3m row-major (ld = 3m): the X slot is the columns [0, m), W is [m, 2m), P is [2m, 3m) (`slot`).  The
eigensolver keeps three such arrays, S = [X | W | P], A~ S and C~ S, and one n x m residual block R.

Widths.  `Shapes(m)` restates, from the widths and byte offsets alone and without calling any plan code of the library, the branch
conditions of csr_mm_ld / csr_mm2_ld (csrc/csr.hpp), enqueue_multi_levels and ilu0_solve_multi_ld (csrc/tri_levels.hpp,
local_solve.hpp), GeneoWork::gram and GeneoWork::rotate (csrc/geneo_blocks.hpp).  Every array is taken to start at a 32-byte
boundary (the GPU test asserts that of its tensors), so a slot starts 8 k m bytes into a row.  WIDTHS and what each is there for:

    6   ld = 18 is not a multiple of 4: the scalar product kernel k_spmm_rowmajor and the scalar sweeps k_trsv_level_multi
    7   odd; the W slot starts 56 bytes into a row: the quad kernels are refused on alignment as well
    8   the smallest quad case, nq = 2: k_spmm_rowmajor4_tiled<true> with a row order, k_trsv_level_multi4
    24  the benchmark's width (nev 20 + 4): nq = 6, the rotation in ONE launch (p = 72, q = 48), single-precision sweeps
    28  p = 84 > 80: inner pieces 72 + 12, modes 0 then 3; q = 56: output panels 48 + 8, gap_from = 28 inside the first; nq = 7;
        m x m Gram products still on k_gram_small, with the second 16-column tile
    32  the last width of k_gram_small and of the tiled product (nq = 8)
    36  nq = 9: the untiled k_spmm_rowmajor4<true> although a row order exists; m x m Gram on k_gram_mfma<2, 5> with U == V;
        rotation with q = 72 (48 + 24)
    48  p = 144 as 72 + 72; q = 96 with gap_from = 48 exactly at the panel boundary

Rows of the dense steps (Gram, rotation, helper kernels): subdomains of SIZES rows, as tests/test_gpu_blockvec.py -- no multiples of
the 4-row MFMA step, the 16-row slab or the 2048-row chunk of GeneoWork.  (The eigensolver itself asks for 3m rows per subdomain
because of its Rayleigh-Ritz step; the kernels do not.)

Matrix of the sparse steps (`Sparse`): block diagonal, n = 5324.  Block 0: a 27-point stencil on a 17 x 16 x 17 lexicographic grid,
4624 rows >= the 4096 csr_row_order_tiled asks for.  Block 1: 700 rows whose lengths cycle through LENGTHS = 0, 1, 3, 4, 5, 8, 9, 27
-- empty rows, and lengths on both sides of the unroll depths 4 (k_spmm_rowmajor4) and 8 (k_spmm_rowmajor, ..4_tiled) -- with columns
drawn inside the block; they keep the natural order.  n % 64 = 12 and ceil(n / 64) = 84 = 8 * 10 + 4: a ragged last workgroup of the
tiled kernel and an uneven xcd_remap.  Two value arrays on the one pattern: `va` symmetric and strictly diagonally dominant with a
positive diagonal on the grid block (symmetric positive definite), strictly row diagonally dominant on block 1; `vc` standard-normal
values unrelated to va and asymmetric, so that swapped products or va2 read as va do not pass.
A matrix with an empty row is singular.  The SOLVES therefore factorise `factor_matrix`: va with 1.0 put on the diagonal of the
empty rows of block 1, everything else as it is.

Block entries come from a seeded generator plus COLUMN_STEP times the column index, as in tests/test_gpu_blockvec.py: a transposed
or column-shifted result does not pass.

References (float64 unless said).
  * products: `spmm_restated` adds the rounded products a_k x_k in entry order from 0.0, vectorised over the rows -- with the library
    built -ffp-contract=off that is what all four product kernels do (their padding entries add +0.0 to a sum that is never -0.0
    here), so the GPU test asks for equal bits.  Its own error against the long-double value y_ld (`spmm_longdouble`):
    |y - y_ld| <= (w + 1) u sum |a| |x|, w the entries of the row (w - 1 additions and one rounding per product, first order;
    + 1 for the second-order terms and the rounding of y_ld to double).
  * Gram products U^T V and rotations U Y: the float64 host product, compared on the GPU within 1e-13 sum |a| |b| + 1e-300, the bound
    tests/test_gpu_blockvec.py uses for these kernels (the matrix cores add the same rounded products in another order).  The CPU test
    shows that the float64 host product itself stays within that bound of the long-double value.
  * helper kernels: one rounding per operation, so the numpy expression is exact (`random_block` restates splitmix64 in uint64)."""
import functools

import numpy as np
import scipy.sparse as sp

U64 = 2.0 ** -53
WIDTHS = (6, 7, 8, 24, 28, 32, 36, 48)
SIZES = (4099, 17, 2048, 1, 6150)
SUB_PTR = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
COLUMN_STEP = 0.125

# geneo_blocks.hpp / geneo_kernels.hpp
CHUNK_ROWS = 2048
ROT_TQ = 3                       # 16-column output tiles of one rotation launch
ROT_PANEL = 16 * ROT_TQ
ROT_KMAX, ROT_KPIECE = 80, 72    # inner columns of one launch; the piece size beyond
ROT_PRE = 20                     # registers per lane of a prefetched slab
GRAM_SMALL = 32
# csr.hpp / kernels.hpp
WG = 256
SPMM_TILED_ROWS, SPMM_TILED_NQ = 64, 8
ROW_ORDER_MIN = 4096
UNROLL = {"k_spmm_rowmajor": 8, "k_spmm_rowmajor4": 4, "k_spmm_rowmajor4_tiled": 8}
# local_solve.hpp
SN_PANEL = 48
CSR_PANEL = WG
WIDE_LEVEL = 96                  # rows of so many entries take k_trsv_level_multi_wide and forbid the single-precision sweeps


def slot(m, k):
    """columns of slot k (0 X, 1 W, 2 P) of an n x 3m block"""
    return slice(k * m, (k + 1) * m)


class Shapes:
    """what the host code decides for block width m on arrays with ld = 3m that start at a 32-byte boundary"""

    def __init__(self, m):
        self.m, self.ld, self.p, self.q = m, 3 * m, 3 * m, 2 * m
        self.nq = m // 4 if m % 4 == 0 else None

    def aligned(self, k, ld=None):
        """slot k of a row of ld doubles starts at a 32-byte boundary in every row"""
        ld = self.ld if ld is None else ld
        return (8 * k * self.m) % 32 == 0 and (8 * ld) % 32 == 0

    # csr_mm_ld / csr_mm2_ld: operands in slot k of three different ld = 3m arrays
    def quad_product(self, k):
        return self.m % 4 == 0 and self.ld % 4 == 0 and self.aligned(k)

    def product_kernels(self, k, two, row_order):
        """kernels of Y = A X (two: YA = A X, YC = C X) with X, Y in slot k"""
        if not self.quad_product(k):
            return ["k_spmm_rowmajor"] * (2 if two else 1)
        if not two:
            return ["k_spmm_rowmajor4<false>"]
        return ["k_spmm_rowmajor4_tiled<true>" if row_order and self.nq <= SPMM_TILED_NQ else "k_spmm_rowmajor4<true>"]

    # ilu0_solve_multi_ld(T, m, R, ldd = m, W slot, ldx = 3m, f32)
    def quad_solve(self, ldd=None, ldx=None, kx=1):
        ldd = self.m if ldd is None else ldd
        ldx = self.ld if ldx is None else ldx
        return self.m % 4 == 0 and ldd % 4 == 0 and ldx % 4 == 0 and (8 * kx * self.m) % 32 == 0

    def level_kernel(self, f32, widest_row, contiguous=False):
        quad = self.quad_solve(ldx=self.m, kx=0) if contiguous else self.quad_solve()
        if f32 and quad and widest_row < WIDE_LEVEL:
            return "k_trsv_level_multi4_f32"
        if widest_row >= WIDE_LEVEL and self.m <= WG:
            return "k_trsv_level_multi_wide"
        return "k_trsv_level_multi4" if quad else "k_trsv_level_multi"

    # GeneoWork::gram
    @staticmethod
    def gram_kernel(pu, pv, same):
        if pu <= GRAM_SMALL and pv <= GRAM_SMALL:
            b = lambda v: "true" if v else "false"
            if same:
                return f"k_gram_small<true, {b(pu > 16)}, {b(pu > 16)}>"
            return f"k_gram_small<false, {b(pu > 16)}, {b(pv > 16)}>"
        if pu <= 128 and pv <= 80:
            return "k_gram_mfma<2, 5>"
        if pu <= 144 and pv <= 144:
            return "k_gram_mfma<3, 9>"
        return "k_gram_mfma<2, 5> panels"

    # GeneoWork::rotate
    @staticmethod
    def rotate_launches(pk, q, base):
        """[(first output column, output columns, first inner column, inner columns, mode, 'k_rotate_mfma<PRE, TQ>')]"""
        kp = pk if pk <= ROT_KMAX else ROT_KPIECE
        out = []
        for j0 in range(0, q, ROT_PANEL):
            qq = min(ROT_PANEL, q - j0)
            for k0 in range(0, pk, kp):
                kk = min(kp, pk - k0)
                mode = (1 if base else 0) if k0 == 0 else (2 if base else 3)
                p4 = (kk + 3) & ~3
                pre = ROT_PRE if 16 * p4 <= ROT_PRE * 64 else 0
                out.append((j0, qq, k0, kk, mode, f"k_rotate_mfma<{pre}, {-(-qq // 16)}>"))
        return out

    def rayleigh_ritz_rotation(self):
        return self.rotate_launches(self.p, self.q, False)

    def orthogonalisation(self):
        return self.rotate_launches(self.m, self.m, True)


def chunks(sub_ptr=SUB_PTR):
    """(first row, end row, subdomain) of GeneoWork's chunks"""
    return [(r, min(r + CHUNK_ROWS, int(sub_ptr[s + 1])), s) for s in range(len(sub_ptr) - 1) for r in range(int(sub_ptr[s]), int(sub_ptr[s + 1]), CHUNK_ROWS)]


# ---- dense steps -------------------------------------------------------------------------------------------------------------------
def _block(rng, n, cols):
    return rng.standard_normal((n, cols)) + COLUMN_STEP * np.arange(cols)[None, :]


class Dense:
    """the blocks of the dense steps at width m: S, AS, CS (n x 3m, different), R (n x m), the Ritz coefficients Y (nsub x 3m x 2m),
    the orthogonalisation coefficients G (nsub x m x m), Ritz values mu (nsub x m), row weights w; never changed after creation"""

    def __init__(self, m):
        rng = np.random.default_rng(7000 + m)
        self.m, self.n, self.nsub = m, int(SUB_PTR[-1]), len(SIZES)
        self.S, self.AS, self.CS = (_block(rng, self.n, 3 * m) for _ in range(3))
        self.R = _block(rng, self.n, m)
        self.Y = rng.standard_normal((self.nsub, 3 * m, 2 * m))
        self.G = rng.standard_normal((self.nsub, m, m))
        self.mu = rng.uniform(0.5, 2.0, (self.nsub, m)) * np.where(np.arange(self.nsub)[:, None] % 2, -1.0, 1.0)   # differs per subdomain
        self.w = rng.uniform(0.0, 1.0, self.n)
        self.w[::5] = 0.0                                                # a partition of unity / mask has exact zeros
        self.sub_of_row = np.repeat(np.arange(self.nsub), SIZES)
        for a in (self.S, self.AS, self.CS, self.R, self.Y, self.G, self.mu, self.w):
            a.setflags(write=False)

    def rows(self, s):
        return slice(int(SUB_PTR[s]), int(SUB_PTR[s + 1]))


@functools.lru_cache(maxsize=2)
def dense(m):
    return Dense(m)


def gram_ref(U, V, dtype=np.float64):
    """(G, bound base): per subdomain U^T V and |U|^T |V|"""
    U, V = np.asarray(U, dtype=dtype), np.asarray(V, dtype=dtype)
    G = np.stack([U[SUB_PTR[s]:SUB_PTR[s + 1]].T @ V[SUB_PTR[s]:SUB_PTR[s + 1]] for s in range(len(SIZES))])
    B = np.stack([np.abs(U[SUB_PTR[s]:SUB_PTR[s + 1]]).T @ np.abs(V[SUB_PTR[s]:SUB_PTR[s + 1]]) for s in range(len(SIZES))])
    return G, B


def rotate_ref(U, Y, rows=None, dtype=np.float64):
    """(U Y[sub], |U| |Y[sub]|) row by row; rows: a subset of the rows (the long-double check)"""
    sub = np.repeat(np.arange(len(SIZES)), SIZES)
    idx = np.arange(U.shape[0]) if rows is None else np.asarray(rows)
    out = np.empty((len(idx), Y.shape[2]), dtype=dtype)
    bnd = np.empty_like(out)
    for s in range(len(SIZES)):
        sel = sub[idx] == s
        Us, Ys = np.asarray(U[idx[sel]], dtype=dtype), np.asarray(Y[s], dtype=dtype)
        out[sel] = Us @ Ys
        bnd[sel] = np.abs(Us) @ np.abs(Ys)
    return out, bnd


def sample_rows(per_sub=24):
    """first, last and seeded rows of every subdomain"""
    rng = np.random.default_rng(5)
    out = []
    for s, sz in enumerate(SIZES):
        pick = np.unique(np.concatenate([[0, sz - 1], rng.integers(0, sz, min(per_sub, sz))]))
        out.append(int(SUB_PTR[s]) + pick)
    return np.concatenate(out)


# ---- helper kernels ----------------------------------------------------------------------------------------------------------------
GENEO_SEED_BASE = 0x5DEECE66D    # GeneoRun::start_block adds ddm_geneo_params.seed


def random_block(n, m, seed, mask):
    """k_geneo_random: splitmix64 of the entry index t = i m + j (it does not know the leading dimension), mapped to [-0.5, 0.5),
    times mask[i]"""
    with np.errstate(over="ignore"):
        t = np.arange(n * m, dtype=np.uint64)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (t + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) - 0.5
    return u.reshape(n, m) * np.asarray(mask, dtype=np.float64)[:, None]


def residual_ref(mu, sub_of_row, AX, CX):
    return CX - mu[sub_of_row] * AX


def invsqrt_diag_ref(G):
    g = np.einsum("sjj->sj", G)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(g > 1e-300, 1.0 / np.sqrt(np.where(g > 1e-300, g, 1.0)), 0.0)


def finalize_ref(scale, sub_of_row, V, nev):
    return np.ascontiguousarray((scale[sub_of_row, :nev] * V[:, :nev]).T)


def gram_diagonals(nsub, m):
    """m x m matrices whose diagonals are of mixed size and include 0.0, a negative one and 1e-301 (all three give 0.0)"""
    rng = np.random.default_rng(900 + m)
    G = rng.standard_normal((nsub, m, m))
    d = 10.0 ** rng.uniform(-290.0, 290.0, (nsub, m)) * rng.uniform(1.0, 10.0, (nsub, m))
    d[0, 0], d[1 % nsub, m - 1], d[2 % nsub, m // 2] = 0.0, -3.0, 1e-301
    d[3 % nsub, 1 % m] = 4.0                                             # an exact square
    for s in range(nsub):
        G[s][np.diag_indices(m)] = d[s]
    return G


# ---- sparse steps ------------------------------------------------------------------------------------------------------------------
GRID = (17, 16, 17)              # x fastest
IRREGULAR_ROWS = 700
LENGTHS = (0, 1, 3, 4, 5, 8, 9, 27)


class Sparse:
    def __init__(self):
        rng = np.random.default_rng(20240)
        nx, ny, nz = GRID
        n0 = nx * ny * nz
        x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
        x, y, z = (a.transpose(2, 1, 0).ravel() for a in (x, y, z))      # row = x + nx (y + ny z)
        ri, cj = [], []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if (dz, dy, dx) <= (0, 0, 0):
                        continue                                         # the upper triangle; mirrored below
                    ok = (x + dx >= 0) & (x + dx < nx) & (y + dy >= 0) & (y + dy < ny) & (z + dz >= 0) & (z + dz < nz)
                    r = np.flatnonzero(ok)
                    ri.append(r), cj.append(r + dx + nx * (dy + ny * dz))
        ri, cj = np.concatenate(ri), np.concatenate(cj)
        assert np.all(cj > ri)
        up = sp.csr_matrix((-(0.25 + rng.uniform(0.0, 1.0, len(ri))), (ri, cj)), shape=(n0, n0))
        off = sp.csr_matrix(up + up.T)
        A0 = sp.csr_matrix(off + sp.diags(1.0 + np.asarray(abs(off).sum(axis=1)).ravel()))
        # block 1: row i has LENGTHS[i % 8] entries, the diagonal among them, the others drawn inside the block
        n1 = IRREGULAR_ROWS
        ri, cj, va = [], [], []
        for i in range(n1):
            L = LENGTHS[i % len(LENGTHS)]
            if L == 0:
                continue
            others = rng.choice(n1 - 1, size=L - 1, replace=False)
            others = others + (others >= i)
            v = rng.standard_normal(L - 1)
            ri += [i] * L
            cj += [i] + others.tolist()
            va += [1.0 + np.abs(v).sum()] + v.tolist()
        A1 = sp.csr_matrix((va, (ri, cj)), shape=(n1, n1))
        M = sp.csr_matrix(sp.block_diag([A0, A1], format="csr"))
        M.sort_indices()
        assert M.has_canonical_format
        self.n0, self.n1, self.n = n0, n1, n0 + n1
        self.block_ptr = np.array([0, n0, n0 + n1], dtype=np.int64)
        self.M = M                                                       # the pattern and the first value array
        self.rp, self.ci, self.va = M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.astype(np.float64)
        self.vc = np.random.default_rng(20241).standard_normal(M.nnz) + 0.5
        self.lengths = np.diff(self.rp)
        for a in (self.rp, self.ci, self.va, self.vc):
            a.setflags(write=False)

    @functools.cached_property
    def C(self):
        return sp.csr_matrix((self.vc, self.ci, self.rp), shape=self.M.shape)

    @functools.cached_property
    def factor_matrix(self):
        """va with 1.0 on the diagonal of the empty rows: what the solves factorise"""
        empty = np.flatnonzero(self.lengths == 0)
        F = sp.csr_matrix(self.M + sp.csr_matrix((np.ones(len(empty)), (empty, empty)), shape=self.M.shape))
        F.sort_indices()
        return F

    def blocks(self, m):
        """the X operand array (n x 3m) and the n x m right-hand side of the solves at width m"""
        rng = np.random.default_rng(8000 + m)
        X, D = _block(rng, self.n, 3 * m), _block(rng, self.n, m)
        X.setflags(write=False), D.setflags(write=False)
        return X, D


@functools.lru_cache(maxsize=None)
def sparse():
    return Sparse()


def spmm_restated(rp, ci, va, X):
    """Y = A X: per row the rounded products in entry order, added from 0.0 (a float64 loop over the entry positions, all rows at once)"""
    n = len(rp) - 1
    Y = np.zeros((n, X.shape[1]))
    lengths = np.diff(rp)
    for k in range(int(lengths.max())):
        rows = np.flatnonzero(lengths > k)
        e = rp[rows] + k
        Y[rows] = Y[rows] + va[e][:, None] * X[ci[e]]
    return Y


def spmm_longdouble(rp, ci, va, X):
    """(A X in long double, sum |a| |x| in long double)"""
    n = len(rp) - 1
    Y = np.zeros((n, X.shape[1]), dtype=np.longdouble)
    B = np.zeros_like(Y)
    lengths = np.diff(rp)
    Xl, vl = X.astype(np.longdouble), va.astype(np.longdouble)
    for k in range(int(lengths.max())):
        rows = np.flatnonzero(lengths > k)
        e = rp[rows] + k
        prod = vl[e][:, None] * Xl[ci[e]]
        Y[rows] += prod
        B[rows] += np.abs(prod)
    return Y, B


@functools.lru_cache(maxsize=2)
def products(m):
    """(X, {(slot, 'A' / 'C'): the restated product of the slot's columns}) at width m"""
    sc = sparse()
    X, _ = sc.blocks(m)
    out = {}
    for k in range(3):
        Xk = np.ascontiguousarray(X[:, slot(m, k)])
        out[k, "A"] = spmm_restated(sc.rp, sc.ci, sc.va, Xk)
        out[k, "C"] = spmm_restated(sc.rp, sc.ci, sc.vc, Xk)
    return X, out
