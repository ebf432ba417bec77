"""Cases, shape table and host reference for the harmonic extension ddm_harmonic (csrc/geneo.hpp) and the operators built on it:
the extension u_i = -A_ii^-1 A_ib u_b, the projection P = [0 -A_ii^-1 A_ib; 0 I] of the constrained eigensolver, its transpose and
the T T^T operator of ddm_svd_basis.  No GPU and nothing from the library is used here; tests/test_harmonic_cases_reference.py pins
this file, tests/test_gpu_harmonic_shapes.py runs the device against it.

MATRICES (block diagonal, sorted columns, stored diagonal; the blocks are 7-point boxes, x fastest):
  poisson        the (12, 11, 10) box cut into slabs of 4, 3 and 3 planes (couplings across the cuts left out): diagonal 6, -1 beside it
  dominant_sym   the same pattern, symmetric, independent off-diagonal values in -[0.2, 1], strictly diagonally dominant => SPD
  dominant_gen   non-symmetric values of mixed sign on the same pattern, strictly COLUMN dominant: the argument of tests/sn_cases.py
                 that L U without pivoting exists and does not grow; every principal submatrix (A_ii) inherits it
  nearly_sym_lo  dominant_sym with ONE entry between two interior rows multiplied by 1 + 1e-13: below the 1e-12 of
                 csr_values_symmetric (|a - b| > 1e-12 (|a| + |b|)), so the factor is a Cholesky factor
  nearly_sym_hi  the same entry multiplied by 1 + 1e-9: above it, so the factor is L U
  uneven9        nine boxes of 1584, 1, 60, 1, 36, 18, 120, 63 and 8 rows with dominant_sym values

CLASSIFICATIONS (0 interior, 1 boundary, 2 neither), per block:
  shell          the faces of the box are boundary, the face x = 0 is neither (the MsGFEM layout: Dirichlet rows beside interior rows)
  all            shell with the face x = 0 boundary as well
  random         independent per row, 65 % / 25 % / 10 %; an interior row without a stored diagonal would be made neither (none is)
  dup            shell through ddm_harmonic_create (index lists), every fifth boundary index listed twice
  no_boundary    shell with every boundary row made neither: G_ib has no entry
  blocks         (uneven9) shell, but block 1 is one interior row, block 3 one boundary row, block 4 all interior, block 5 all
                 boundary; block 8 (2 x 2 x 2) has no interior row either
  error          poisson / shell with the diagonal of one interior row not stored and all its neighbours boundary: DDM_ENUMERIC

WIDTHS.  Shapes states from the numbers alone which csr_mm_ld kernel and how many solve panels every call takes:
  extend (public entry point)  nrhs in EXTEND_WIDTHS, ldx in extend_lds(nrhs) = nrhs, nrhs + 3, the next multiple of 4 above nrhs + 4.
                               ddm_harmonic_extend walks chunks of 48 columns at X + c0 (c0 = 0, 48, 96: 32-byte aligned whenever X is);
                               a chunk of w columns takes k_spmm_rowmajor4 iff w % 4 == 0 and ldx % 4 == 0 (its output has ld = w).
  P, P^T, T T^T                m in PROJ_WIDTHS with (ld, slot) in proj_layouts(m): ld = m, or slot 0, 1, 2 of an n x 3m array.  Slot
                               offsets k m keep the 32-byte alignment iff m % 4 == 0, so the quad kernel runs iff m % 4 == 0.
  solve panels                 device supernodal factor: ceil(w / 48); host factor: ceil(w / 256) = 1.  harmonic_apply does not chunk:
                               m = 52 is two panels (48 + 4) on the device engine.

REFERENCE.  splu of A_ii in float64, refined on residuals formed in numpy.longdouble until the correction is at rounding level
(refined_solve); P^T from its definition with A_ii^-T (splu of the transpose), T T^T from a dense T (every boundary column solved and
refined), G_ib / G_bi by slicing A.  Every width reads the leading columns of ONE block per case, so each reference is computed once.

TOLERANCE.  The project's rule for this operation (tests/test_gpu_coarse_spaces.py): 1e-10 of the column's largest reference entry,
per column, over the rows the operation computes."""
import functools
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

TOL = 1e-10
PANEL = 48                                                               # columns of a device panel and of a chunk of ddm_harmonic_extend
HOST_PANEL = 256                                                         # CSR_PANEL_COLS
EXTEND_WIDTHS = (1, 2, 4, 5, 47, 48, 49, 96, 97)
PROJ_WIDTHS = (1, 4, 7, 12, 24, 48, 52)
WMAX = max(EXTEND_WIDTHS)
INTERIOR, BOUNDARY, NEITHER = 0, 1, 2
LD = np.longdouble

SLABS = [(12, 11, 4), (12, 11, 3), (12, 11, 3)]
NINE = [(12, 11, 12), (1, 1, 1), (5, 4, 3), (1, 1, 1), (4, 3, 3), (3, 3, 2), (6, 5, 4), (7, 3, 3), (2, 2, 2)]


def extend_lds(nrhs):
    return (nrhs, nrhs + 3, 4 * ((nrhs + 4) // 4 + 1))


def proj_layouts(m):
    """(ld, slot): the block alone, and the X, W, P slots of the eigensolver's n x 3m array"""
    return ((m, 0), (3 * m, 0), (3 * m, 1), (3 * m, 2))


class Shapes:
    """the kernels and panels a call takes, from csr_mm_ld / ilu0_solve_multi_ld / ddm_harmonic_extend read as text"""

    @staticmethod
    def mm_kernel(w, ldx, ldy, x_offset, y_offset=0):
        quad = w % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and (8 * x_offset) % 32 == 0 and (8 * y_offset) % 32 == 0
        return "k_spmm_rowmajor4" if quad else "k_spmm_rowmajor"

    @staticmethod
    def panels(w, engine):
        p = PANEL if engine == "device" else HOST_PANEL
        return [min(p, w - c) for c in range(0, w, p)]

    @classmethod
    def extend_calls(cls, nrhs, ldx):
        """[(c0, w, product kernel)] of ddm_harmonic_extend"""
        return [(c0, min(PANEL, nrhs - c0), cls.mm_kernel(min(PANEL, nrhs - c0), ldx, min(PANEL, nrhs - c0), c0)) for c0 in range(0, nrhs, PANEL)]

    @classmethod
    def proj_kernel(cls, m, ld, slot):
        return cls.mm_kernel(m, ld, m, slot * m)


# ---- matrices ------------------------------------------------------------------------------------------------------------------------
def _boxes(boxes):
    """(n, block_ptr, ei, ej, pos): the edges i < j of the block-diagonal 7-point pattern, pos[r] = (block, x, y, z, nx, ny, nz)"""
    ei, ej, pos, bp = [], [], [], [0]
    for b, (nx, ny, nz) in enumerate(boxes):
        idx = bp[-1] + np.arange(nx * ny * nz).reshape(nz, ny, nx)
        for a, c in ((idx[:, :, :-1], idx[:, :, 1:]), (idx[:, :-1, :], idx[:, 1:, :]), (idx[:-1, :, :], idx[1:, :, :])):
            ei.append(a.ravel())
            ej.append(c.ravel())
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        pos.append(np.stack([np.full(x.size, b), x.ravel(), y.ravel(), z.ravel(), np.full(x.size, nx), np.full(x.size, ny), np.full(x.size, nz)], axis=1))
        bp.append(bp[-1] + nx * ny * nz)
    return bp[-1], np.array(bp, dtype=np.int64), np.concatenate(ei), np.concatenate(ej), np.concatenate(pos)


def _assemble(n, ei, ej, up, lo, diag):
    """a_ij = up, a_ji = lo for the edges i < j"""
    d = np.arange(n)
    M = sp.csr_matrix((np.concatenate([up, lo, diag]), (np.concatenate([ei, ej, d]), np.concatenate([ej, ei, d]))), shape=(n, n))
    M.sort_indices()
    assert M.nnz == 2 * len(ei) + n
    return M


def _matrix(kind, boxes, seed):
    n, bp, ei, ej, pos = _boxes(boxes)
    rng = np.random.default_rng(seed)
    ne = len(ei)
    if kind == "poisson":
        return _assemble(n, ei, ej, -np.ones(ne), -np.ones(ne), np.full(n, 6.0)), bp, pos
    if kind == "sym":
        w = -(0.2 + 0.8 * rng.random(ne))
        s = np.bincount(ei, np.abs(w), n) + np.bincount(ej, np.abs(w), n)
        return _assemble(n, ei, ej, w, w, np.maximum(s, 1.0) * (1.05 + 0.1 * rng.random(n))), bp, pos
    assert kind == "gen"
    up = (0.2 + 0.8 * rng.random(ne)) * np.where(rng.random(ne) < 0.7, -1.0, 1.0)
    lo = (0.2 + 0.8 * rng.random(ne)) * np.where(rng.random(ne) < 0.7, -1.0, 1.0)
    s = np.bincount(ej, np.abs(up), n) + np.bincount(ei, np.abs(lo), n)       # column sums: a_ij lies in column j, a_ji in column i
    return _assemble(n, ei, ej, up, lo, np.maximum(s, 1.0) * (1.1 + 0.2 * rng.random(n))), bp, pos


def _shell(pos, dirichlet_face=True):
    b, x, y, z, nx, ny, nz = pos.T
    face = (x == 0) | (x == nx - 1) | (y == 0) | (y == ny - 1) | (z == 0) | (z == nz - 1)
    cls = np.where(face, BOUNDARY, INTERIOR)
    if dirichlet_face:
        cls[x == 0] = NEITHER
    return cls.astype(np.uint8)


def perturbed_pair(pos):
    """(i, j): two interior rows of the shell classification that are neighbours in x, in the middle of block 0"""
    b, x, y, z, nx, ny, nz = pos.T
    i = int(np.nonzero((b == 0) & (x == nx // 2) & (y == ny // 2) & (z == nz // 2))[0][0])
    return i, i + 1


def _perturb(M, pos, rel):
    i, j = perturbed_pair(pos)
    M = M.copy()
    k = M.indptr[i] + int(np.searchsorted(M.indices[M.indptr[i]:M.indptr[i + 1]], j))
    assert M.indices[k] == j
    M.data[k] *= 1.0 + rel
    return M


@dataclass(frozen=True)
class Spec:
    matrix: str
    classes: str
    symmetric: bool            # what csr_values_symmetric must find in A^
    lists: bool = False        # through ddm_harmonic_create (index lists; no G_bi)


SPECS = {
    "poisson-shell": Spec("poisson", "shell", True),
    "poisson-all": Spec("poisson", "all", True),
    "poisson-random": Spec("poisson", "random", True),
    "poisson-dup": Spec("poisson", "dup", True, lists=True),
    "poisson-no_boundary": Spec("poisson", "no_boundary", True),
    "dominant_sym-shell": Spec("dominant_sym", "shell", True),
    "dominant_sym-random": Spec("dominant_sym", "random", True),
    "dominant_gen-shell": Spec("dominant_gen", "shell", False),
    "dominant_gen-random": Spec("dominant_gen", "random", False),
    "nearly_sym_lo-shell": Spec("nearly_sym_lo", "shell", True),
    "nearly_sym_hi-shell": Spec("nearly_sym_hi", "shell", False),
    "uneven9-blocks": Spec("uneven9", "blocks", True),
}
NAMES = tuple(SPECS)
SYMMETRIC = tuple(k for k, s in SPECS.items() if s.symmetric and not s.lists)      # P^T and T T^T run here
GENERAL = tuple(k for k, s in SPECS.items() if not s.symmetric)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(A, block_ptr, pos), A read-only"""
    if name == "poisson":
        M, bp, pos = _matrix("poisson", SLABS, 0)
    elif name == "dominant_gen":
        M, bp, pos = _matrix("gen", SLABS, 11)
    elif name == "uneven9":
        M, bp, pos = _matrix("sym", NINE, 13)
    else:
        M, bp, pos = _matrix("sym", SLABS, 7)
        if name != "dominant_sym":
            M = _perturb(M, pos, {"nearly_sym_lo": 1e-13, "nearly_sym_hi": 1e-9}[name])
    for a in (M.data, M.indices, M.indptr, bp, pos):
        a.setflags(write=False)
    return M, bp, pos


def classes(name, mname):
    M, bp, pos = matrix(mname)
    if name in ("shell", "dup"):
        return _shell(pos)
    if name == "all":
        return _shell(pos, dirichlet_face=False)
    if name == "no_boundary":
        c = _shell(pos)
        c[c == BOUNDARY] = NEITHER
        return c
    if name == "random":
        c = np.random.default_rng(5).choice(np.array([INTERIOR, BOUNDARY, NEITHER], dtype=np.uint8), size=M.shape[0], p=[0.65, 0.25, 0.10])
        c[(c == INTERIOR) & (M.diagonal() == 0.0)] = NEITHER                # the repair (no row of these matrices needs it)
        return c
    assert name == "blocks"
    c = _shell(pos)
    b = pos[:, 0]
    c[b == 1] = INTERIOR
    c[b == 3] = BOUNDARY
    c[b == 4] = INTERIOR
    c[b == 5] = BOUNDARY
    return c


def index_lists(cls, every=5):
    """(interior, boundary) for ddm_harmonic_create; every fifth boundary index is listed twice (the copy right behind it)"""
    bb = np.nonzero(cls == BOUNDARY)[0]
    rep = np.ones(len(bb), dtype=np.int64)
    rep[::every] = 2
    return np.nonzero(cls == INTERIOR)[0].astype(np.int64), np.repeat(bb, rep).astype(np.int64)


def error_case():
    """(A, block_ptr, classes, row): poisson / shell with the diagonal of interior row `row` removed and its six neighbours made
    boundary, so that no stored entry of the row lies in an interior column"""
    M, bp, pos = matrix("poisson")
    c = _shell(pos)
    row, _ = perturbed_pair(pos)
    nb = M.indices[M.indptr[row]:M.indptr[row + 1]]
    c[nb[nb != row]] = BOUNDARY
    A = sp.coo_matrix(M)
    keep = ~((A.row == row) & (A.col == row))
    A = sp.csr_matrix((A.data[keep], (A.row[keep], A.col[keep])), shape=M.shape)
    A.sort_indices()
    assert c[row] == INTERIOR and A.nnz == M.nnz - 1 and np.all(c[A.indices[A.indptr[row]:A.indptr[row + 1]]] != INTERIOR)
    return A, bp, c, row


# ---- reference -----------------------------------------------------------------------------------------------------------------------
def spmm_ld(M, Z):
    """M Z with the products and the row sums in numpy.longdouble"""
    M = sp.csr_matrix(M)
    Z = np.asarray(Z, dtype=LD)
    out = np.zeros((M.shape[0], Z.shape[1]), dtype=LD)
    if M.nnz:
        prod = M.data.astype(LD)[:, None] * Z[M.indices]
        filled = np.diff(M.indptr) > 0
        out[filled] = np.add.reduceat(prod, M.indptr[:-1][filled], axis=0)
    return out


def refined_solve(M, lu, B):
    """M Z = B (B longdouble) from the float64 factor lu, refined on longdouble residuals until the correction of every column is at the
    rounding level of float64 (4 eps of the column's largest entry); returns (Z longdouble, steps)"""
    B = np.asarray(B, dtype=LD)
    if M.shape[0] == 0 or B.shape[1] == 0:
        return np.zeros(B.shape, dtype=LD), 0
    Z = lu.solve(np.asarray(B, dtype=np.float64)).astype(LD)
    for step in range(1, 9):
        dz = lu.solve(np.asarray(B - spmm_ld(M, Z), dtype=np.float64))
        Z += dz
        if np.all(np.abs(dz).max(axis=0) <= 4 * np.finfo(np.float64).eps * np.abs(Z).max(axis=0)):
            return Z, step
    raise AssertionError("the refinement did not settle")


class Case:
    """one (matrix, classification) pair with its inputs and references; everything float64 unless said"""

    def __init__(self, name):
        s = SPECS[name]
        self.name, self.spec = name, s
        self.A, self.block_ptr, self.pos = matrix(s.matrix)
        self.n = self.A.shape[0]
        self.cls = classes(s.classes, s.matrix)
        self.ii, self.bb, self.nn = (np.nonzero(self.cls == k)[0] for k in (INTERIOR, BOUNDARY, NEITHER))
        self.Aii = self.A[self.ii][:, self.ii].tocsr()
        self.Aib = self.A[self.ii][:, self.bb].tocsr()
        rng = np.random.default_rng(sum(map(ord, name)))
        self.X = rng.standard_normal((self.n, WMAX))                      # every width reads its leading columns
        self.R = rng.standard_normal((self.n, max(PROJ_WIDTHS)))
        self.d = np.where(self.cls == INTERIOR, 0.5 + rng.random(self.n), 0.0)   # pou_int: zero outside the interior
        for a in (self.cls, self.X, self.R, self.d):
            a.setflags(write=False)

    # -- structure
    def embedded(self, transpose):
        """G_ib (or its transpose G_bi) as n x n CSR with sorted columns, sliced from A"""
        A = sp.coo_matrix(self.A)
        k = (self.cls[A.row] == INTERIOR) & (self.cls[A.col] == BOUNDARY)
        r, c = (A.col[k], A.row[k]) if transpose else (A.row[k], A.col[k])
        G = sp.csr_matrix((A.data[k], (r, c)), shape=self.A.shape)
        G.sort_indices()
        assert G.nnz == int(k.sum())
        return G.indptr.astype(np.int64), G.indices.astype(np.int32), G.data.copy()

    def Ahat(self):
        """A^ = [A_ii 0; 0 I] in the numbering of A: the direct solver's input"""
        A = sp.coo_matrix(self.A)
        k = (self.cls[A.row] == INTERIOR) & (self.cls[A.col] == INTERIOR)
        o = np.nonzero(self.cls != INTERIOR)[0]
        M = sp.csr_matrix((np.concatenate([A.data[k], np.ones(len(o))]), (np.concatenate([A.row[k], o]), np.concatenate([A.col[k], o]))), shape=self.A.shape)
        M.sort_indices()
        return M

    def values_symmetric(self, extra=None):
        """csr_values_symmetric restated on A^ = [A_ii 0; 0 I]; extra: entries (i, j, v) a fault leaves in A^"""
        Ah = sp.lil_matrix((self.n, self.n))
        Ah[np.ix_(self.ii, self.ii)] = self.Aii
        for i, j, v in extra or ():
            Ah[i, j] = v
        Ah = sp.csr_matrix(Ah)
        D = abs(Ah - Ah.T)
        S = abs(Ah) + abs(Ah.T)
        return not (D > 1e-12 * S).nnz

    # -- solves
    @functools.cached_property
    def lu(self):
        return spl.splu(self.Aii.tocsc()) if len(self.ii) else None

    @functools.cached_property
    def lut(self):
        return spl.splu(self.Aii.T.tocsc()) if len(self.ii) else None

    @functools.cached_property
    def E(self):
        """-A_ii^-1 A_ib X_b (n_i x WMAX), refined"""
        Z, self.steps = refined_solve(self.Aii, self.lu, -spmm_ld(self.Aib, self.X[self.bb]))
        return np.asarray(Z, dtype=np.float64)

    def extend_ref(self, nrhs):
        return self.E[:, :nrhs]

    def P_ref(self, m):
        """P X on all rows: interior E, boundary X, neither 0"""
        out = np.zeros((self.n, m))
        out[self.ii] = self.E[:, :m]
        out[self.bb] = self.X[self.bb, :m]
        return out

    @functools.cached_property
    def PtR(self):
        """P^T R = [0; R_b - A_ib^T A_ii^-T R_i; 0] from the definition, refined"""
        out = np.zeros(self.R.shape)
        Z, _ = refined_solve(self.Aii.T.tocsr(), self.lut, self.R[self.ii].astype(LD))
        out[self.bb] = np.asarray(self.R[self.bb].astype(LD) - spmm_ld(self.Aib.T.tocsr(), Z), dtype=np.float64)
        return out

    def Pt_ref(self, m):
        return self.PtR[:, :m]

    @functools.cached_property
    def T(self):
        """dense T = D A_ii^-1 A_ib (n_i x n_b) in longdouble, every column refined"""
        Z, _ = refined_solve(self.Aii, self.lu, self.Aib.toarray().astype(LD))
        return self.d[self.ii].astype(LD)[:, None] * Z

    @functools.cached_property
    def TTtX(self):
        out = np.zeros(self.R.shape)
        out[self.ii] = np.asarray(self.T @ (self.T.T @ self.R[self.ii].astype(LD)), dtype=np.float64)
        return out

    def TTt_ref(self, m):
        return self.TTtX[:, :m]

    # -- float64 model of the library's steps, with seeded faults (tests/test_harmonic_cases_reference.py)
    def model(self, op, m, fault=None):
        """what the library computes for op in ("extend", "P", "Pt") on the leading m columns, in float64 (splu), as an n x m block;
        fault: None or one of FAULTS"""
        cls, n = self.cls, self.n
        A = sp.coo_matrix(self.A)
        isint, isb = cls == INTERIOR, cls == BOUNDARY
        k = isint[A.row] & isb[A.col]
        gr, gc_, gv = A.row[k], A.col[k], A.data[k]
        if fault == "gib_entry_dropped":
            sel = np.arange(len(gv)) != len(gv) // 2
            gr, gc_, gv = gr[sel], gc_[sel], gv[sel]
        if fault == "gib_keeps_neither":
            k2 = isint[A.row] & (cls[A.col] == NEITHER)
            gr, gc_, gv = np.concatenate([gr, A.row[k2]]), np.concatenate([gc_, A.col[k2]]), np.concatenate([gv, A.data[k2]])
        Gib = sp.csr_matrix((gv, (gr, gc_)), shape=(n, n))
        tr, tc = gc_.copy(), gr.copy()
        if fault == "gbi_entry_untransposed" and len(gv):
            q = len(gv) // 2
            tr[q], tc[q] = gr[q], gc_[q]                                     # left at (i, j)
        Gbi = sp.csr_matrix((gv, (tr, tc)), shape=(n, n))
        ka = isint[A.row] & isint[A.col]
        if fault == "ahat_keeps_neither":
            ka = isint[A.row] & (isint[A.col] | (cls[A.col] == NEITHER))
        out_ = ~isint
        Ah = sp.csr_matrix((np.concatenate([A.data[ka], np.ones(out_.sum())]), (np.concatenate([A.row[ka], np.nonzero(out_)[0]]), np.concatenate([A.col[ka], np.nonzero(out_)[0]]))), shape=(n, n))
        lu = spl.splu(Ah.tocsc())
        keep, keep_b = (~isint).astype(np.float64), isb.astype(np.float64)
        if op in ("extend", "P"):
            X = self.X[:, :m]
            k_ = keep if op == "extend" or fault == "keep_for_keep_b" else keep_b
            out = np.empty((n, m))
            for c0 in range(0, m, PANEL if op == "extend" else m):
                w = min(PANEL, m - c0) if op == "extend" else m
                src = X[:, 0:w] if (fault == "chunk_reads_first" and c0 > 0) else X[:, c0:c0 + w]
                out[:, c0:c0 + w] = k_[:, None] * X[:, c0:c0 + w] - lu.solve(np.ascontiguousarray((Gib @ src)))
            return out
        assert op == "Pt"
        R = self.R[:, :m]
        solve = lu.solve if (self.spec.symmetric or fault == "inverse_for_transposed_inverse") else (lambda B: lu.solve(B, trans="T"))
        k_ = keep if fault == "keep_for_keep_b" else keep_b
        return k_[:, None] * R - Gbi @ solve(np.ascontiguousarray(isint[:, None] * R))


FAULTS = ("gib_entry_dropped", "gbi_entry_untransposed", "gib_keeps_neither", "keep_for_keep_b", "inverse_for_transposed_inverse", "chunk_reads_first")
# A neither column kept in A^ alone moves NO result: the row of A^ that belongs to it is an identity row and its right-hand side is
# zero in every operation (G_ib X, interior .* R and D X vanish outside the interior), so the unknown it multiplies is zero.  What it
# changes is the symmetry of A^ (Case.values_symmetric), hence the factor kind and whether P^T is offered.
FAULT_WITHOUT_EFFECT = "ahat_keeps_neither"


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def column_ratio(got, ref, rows=None):
    """per column: max |got - ref| over `rows` / (TOL max |ref| over `rows`); a column whose reference is zero must be met exactly
    (ratio 0 or inf)"""
    g, r = (np.asarray(a)[rows] if rows is not None else np.asarray(a) for a in (got, ref))
    if g.shape[0] == 0:
        return np.zeros(g.shape[1])
    err, big = np.abs(g - r).max(axis=0), np.abs(r).max(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, err / (TOL * big))
