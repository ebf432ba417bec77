"""CPU (-m "not gpu"): the problems of tests/test_gpu_apply_shapes.py and the sharpness of the reference those tests compare with.

The GPU module runs the block and the coarse applies at the shapes their kernels branch on: subdomains of more than one 8192-row
chunk, uneven numbers of coarse vectors per subdomain with kmax = 12, every block width 1..32, n * m beyond one pass of the
element-wise grids.  It compares the device with the float64 CPU oracle (oracle/apply_oracle.py) under the project's fixed rules:
RTOL_VEC = 1e-12 of the largest entry for one operator application, 1e-10 of the largest entry for a preconditioner apply.  Those
rules only mean something if the oracle itself is much closer than that to the exact value on these inputs.  This module measures it:
the oracle's operator applies and its GalerkinPreconditioner.apply against restatements in extended precision (numpy.longdouble:
global scatter-add of the local CSR products; R d, R A R^T and R^T x0 accumulated in longdouble, the K x K solve in float64 with
residual refinement in longdouble).  The reference envelope E_ref of an operation is the largest column-relative deviation
max|oracle - extended| / max|extended| over the checked columns, and the condition asserted is 4 E_ref <= project rule (the device may
be as far from the exact value as the oracle is, on the other side, times two for reduction trees of another depth than numpy's).

The helpers `build_case`, `uneven_basis`, `consistent_columns` and `split_novlp` are the GPU module's inputs as well.

Measured (x86-64, 80-bit longdouble; 4 columns per grid, the applies act on consistent standard-normal vectors):

  grid        n_o     n        rows / subdomain   K    cond(R A R^T)   E_ref A x   E_ref y - A x / 2   E_ref Galerkin   a0 vs extended
  (13,12,11)  2184    4896     576..648           43   96.0            2.8e-16     2.7e-16             6.8e-15          1.2e-15
  (44,42,40)  79335   103635   12144..13800       43   15.1            4.8e-16     4.6e-16             6.5e-14          4.1e-14

so 4 E_ref is 1.9e-15 against 1e-12 for the operator and 2.6e-13 against 1e-10 for the coarse level.  (The Schwarz level has no
extended-precision restatement here: its local ILU(0) solve is pinned bit for bit by tests/test_gpu_parity.py and the pipe / box tests.)
"""
import numpy as np
import pytest

from tests.test_gpu_parity import RTOL_VEC, _build

RTOL_PREC = 1e-10                      # a preconditioner apply against the oracle (tests/test_gpu_parity.py, relative to the largest entry)
CHUNK_ROWS = 8192                      # COARSE_CHUNK_ROWS of csrc/preconditioners.hpp: rows of one coarse restriction / prolongation chunk
GRID_PASS = 2048 * 256                 # entries that one pass of an element-wise kernel covers (grid_for caps the grid at 2048 workgroups)
PARTS = (2, 2, 2)
SMALL, LARGE = (13, 12, 11), (44, 42, 40)
K_S = (1, 2, 4, 5, 7, 9, 12, 3)        # coarse vectors per subdomain: kmax = 12 (three passes of the j += 4 loop), K = 43
# (a, b, c) of cos(pi a x) cos(pi b y) cos(pi c z) on the subdomain's bounding box scaled to [0, 1]^3, lowest orders first
MODES = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1), (2, 0, 0), (0, 2, 0), (0, 0, 2), (2, 1, 0))
LD = np.longdouble


def build_case(ddm, N):
    """(decomposition, basis): structured Poisson on N nodes, 2 x 2 x 2 subdomains, overlap 2, with the hand-made uneven coarse basis"""
    dec = _build(ddm, N, PARTS)
    return dec, uneven_basis(dec, N)


def uneven_basis(dec, N):
    """{subdomain: (k_s, n_s) array}, k_s = K_S[s]: partition of unity times the lowest k_s cosine modes of the subdomain's box,
    normalised, zero on Dirichlet rows (what solver.pou_basis does with its template vectors).  Smooth, linearly independent and close
    to orthogonal per subdomain, so that R A R^T stays well conditioned."""
    from dune_ddm_amd import synth
    grid = synth.StructuredPoisson(N, PARTS)
    assert len(dec.subs) == len(K_S)
    basis = {}
    for sd in dec.subs:
        X = grid.node_coords(sd.glob).astype(np.float64)
        lo, hi = X.min(axis=0), X.max(axis=0)
        T = (X - lo) / (hi - lo)
        vecs = []
        for a, b, c in MODES[:K_S[sd.id]]:
            v = sd.pou * np.cos(np.pi * a * T[:, 0]) * np.cos(np.pi * b * T[:, 1]) * np.cos(np.pi * c * T[:, 2])
            v = v * (1.0 / np.sqrt(float(np.dot(v, v))))
            v[sd.dirichlet_ovlp > 0] = 0.0
            vecs.append(v)
        basis[sd.id] = np.array(vecs)
    return basis


def consistent_columns(dec, m, seed):
    """(n_o, m) block of consistent vectors (the same value on every holder of a DoF) in the single-rank layout"""
    rng = np.random.default_rng(seed)
    cols = []
    for _ in range(m):
        xg = rng.standard_normal(dec.nglobal)
        cols.append(np.concatenate([xg[sd.glob[:sd.n_o]] for sd in dec.subs]))
    return np.stack(cols, axis=1)


def split_novlp(dec, v):
    """the per-subdomain pieces (copies) of a vector in the single-rank non-overlapping layout"""
    out, o = [], 0
    for sd in dec.subs:
        out.append(np.array(v[o:o + sd.n_o], dtype=np.float64))
        o += sd.n_o
    return out


def check_sizes(dec, basis, large):
    """The size conditions the GPU tests rely on, asserted on the decomposition that was built.  Returns (n_o, n, rows per subdomain)."""
    rows = [sd.n for sd in dec.subs]
    n_o, n = sum(sd.n_o for sd in dec.subs), sum(rows)
    assert tuple(len(basis[s]) for s in range(dec.nsub)) == K_S and sum(K_S) == 43 and max(K_S) == 12
    if large:
        assert all(r > CHUNK_ROWS and r % CHUNK_ROWS != 0 for r in rows), rows      # several chunks per subdomain, a ragged last one
        assert n_o * 8 > GRID_PASS and n * 8 > GRID_PASS, (n_o, n)                  # m >= 8: the element-wise kernels stride their grid
    else:
        assert all(r < CHUNK_ROWS for r in rows), rows
    return n_o, n, rows


# ---- extended precision restatements ------------------------------------------------------------------------------------------------
def _csr_mv_ld(M, x):
    """M x with the products and the row sums in longdouble (every row of the matrices here has entries)"""
    assert (np.diff(M.indptr) > 0).all()
    return np.add.reduceat(M.data.astype(LD) * x[M.indices], M.indptr[:-1])


def _global_ld(dec, v):
    """the global vector of a consistent non-overlapping one"""
    g = np.zeros(dec.nglobal, dtype=LD)
    for sd, p in zip(dec.subs, split_novlp(dec, v)):
        g[sd.glob[:sd.n_o]] = p
    return g


def operator_ld(dec, x):
    """A x in the non-overlapping layout: the additive local products summed over all holders of a DoF"""
    xg = _global_ld(dec, x)
    yg = np.zeros(dec.nglobal, dtype=LD)
    for sd in dec.subs:
        np.add.at(yg, sd.glob[:sd.n_o], _csr_mv_ld(sd.A.tocsr(), xg[sd.glob[:sd.n_o]]))
    return np.concatenate([yg[sd.glob[:sd.n_o]] for sd in dec.subs])


class GalerkinLD:
    """x = R^T (R A R^T)^-1 R d restated densely: G holds every basis vector as a global vector (zero outside its subdomain);
    row block s of R A R^T is V_s A_dir,s G[glob_s] (galerkin_preconditioner.hh:292-327: the neighbours' vectors on the shared
    indices, zero elsewhere)."""

    def __init__(self, dec, basis):
        self.dec = dec
        self.V = [np.asarray(basis[s], dtype=np.float64).astype(LD) for s in range(dec.nsub)]
        K = sum(len(v) for v in self.V)
        G = np.zeros((dec.nglobal, K), dtype=LD)
        off = 0
        for sd, V in zip(dec.subs, self.V):
            G[sd.glob, off:off + len(V)] = V.T
            off += len(V)
        A0 = np.zeros((K, K), dtype=LD)
        off = 0
        for sd, V in zip(dec.subs, self.V):
            M = sd.A_dir.tocsr()
            Gs = G[sd.glob]
            Y = np.stack([_csr_mv_ld(M, Gs[:, c]) for c in range(K)], axis=1)      # A_dir,s G[glob_s]
            A0[off:off + len(V)] = V @ Y
            off += len(V)
        self.K, self.A0 = K, A0
        self.A0_f64 = A0.astype(np.float64)

    def solve(self, d0):
        x = np.zeros(self.K, dtype=LD)
        for _ in range(4):                                        # float64 solves, residuals in longdouble
            r = d0 - self.A0 @ x
            x = x + np.linalg.solve(self.A0_f64, r.astype(np.float64)).astype(LD)
        return x

    def apply(self, d):
        dec = self.dec
        dg = _global_ld(dec, d)                                   # d extended to the overlap: the owner's value on every holder
        d0 = np.concatenate([V @ dg[sd.glob] for sd, V in zip(dec.subs, self.V)])
        x0 = self.solve(d0)
        xg = np.zeros(dec.nglobal, dtype=LD)
        off = 0
        for sd, V in zip(dec.subs, self.V):
            np.add.at(xg, sd.glob, x0[off:off + len(V)] @ V)      # addOwnerCopyToAll: the sum over all holders
            off += len(V)
        return np.concatenate([xg[sd.glob[:sd.n_o]] for sd in dec.subs])


def _dev(a, ref):
    return float(np.max(np.abs(a.astype(LD) - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("N", [SMALL, LARGE], ids=["small", "large"])
def test_reference_envelope_fits_the_project_rules(ddm, N):
    """Sizes of the decomposition, cond(R A R^T) of the hand-made basis and E_ref of the oracle's operator and Galerkin applies;
    4 E_ref <= RTOL_VEC (operator) and <= 1e-10 (preconditioner).  The figures are printed (pytest -s) and recorded in the module
    docstring and DESIGN.md section 9."""
    from tests.oracle_bridge import oracle_objects
    assert np.finfo(LD).eps < 1e-18, "numpy.longdouble is not an extended format on this machine"
    dec, basis = build_case(ddm, N)
    n_o, n, rows = check_sizes(dec, basis, large=N == LARGE)
    op, sp_, prec, sch, gal = oracle_objects(dec, coarse=basis)
    ref = GalerkinLD(dec, basis)
    cond = float(np.linalg.cond(ref.A0_f64))
    e_a0 = _dev(gal.a0.toarray(), ref.A0)
    ncol = 4
    X, Y0 = consistent_columns(dec, ncol, seed=11), consistent_columns(dec, ncol, seed=97)
    e_apply = e_usmv = e_gal = 0.0
    for j in range(ncol):
        xs, ys = split_novlp(dec, X[:, j]), split_novlp(dec, Y0[:, j])
        yo = [np.zeros(sd.n_o) for sd in dec.subs]
        op.apply(xs, yo)
        ax = operator_ld(dec, X[:, j])
        e_apply = max(e_apply, _dev(np.concatenate(yo), ax))
        op.applyscaleadd(-0.5, xs, ys)
        e_usmv = max(e_usmv, _dev(np.concatenate(ys), Y0[:, j].astype(LD) - LD(0.5) * ax))
        zo = [np.zeros(sd.n_o) for sd in dec.subs]
        gal.apply(zo, split_novlp(dec, Y0[:, j]))
        e_gal = max(e_gal, _dev(np.concatenate(zo), ref.apply(Y0[:, j])))
    print(f"\napply-shapes reference {N}: n_o = {n_o}, n = {n}, rows per subdomain {min(rows)}..{max(rows)}, K = {ref.K}, "
          f"cond(R A R^T) = {cond:.3e}, E_ref: A x {e_apply:.2e}, y - A x / 2 {e_usmv:.2e}, Galerkin apply {e_gal:.2e}, a0 {e_a0:.2e}")
    assert 4 * e_apply <= RTOL_VEC and 4 * e_usmv <= RTOL_VEC
    assert 4 * e_gal <= RTOL_PREC
    assert 4 * e_a0 <= 1e-12                                    # the tl.a0 against gal.a0 rule of test_operator_dot_and_preconditioner_applies
    assert cond < 1e5                                           # cond * 2^-53 stays two orders below the 1e-10 rule


def test_extended_restatement_is_not_the_oracle_restated(ddm):
    """The restatement must be able to disagree with the oracle: with one coarse vector dropped from a subdomain, or one local product
    left out, it moves by far more than the envelope (a reference that follows the oracle into its mistakes measures nothing)."""
    from tests.oracle_bridge import oracle_objects
    dec, basis = build_case(ddm, SMALL)
    op, sp_, prec, sch, gal = oracle_objects(dec, coarse=basis)
    d = consistent_columns(dec, 1, seed=3)[:, 0]
    zo = [np.zeros(sd.n_o) for sd in dec.subs]
    gal.apply(zo, split_novlp(dec, d))
    fewer = dict(basis)
    fewer[6] = basis[6][:-1]
    assert _dev(np.concatenate(zo), GalerkinLD(dec, fewer).apply(d)) > 1e-6
    yo = [np.zeros(sd.n_o) for sd in dec.subs]
    op.apply(split_novlp(dec, d), yo)
    assert _dev(np.concatenate(yo), operator_ld(dec, d)) < 1e-14
    dec.subs[3].A = dec.subs[3].A * 0.0
    assert _dev(np.concatenate(yo), operator_ld(dec, d)) > 1e-3
