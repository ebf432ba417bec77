"""Numpy restatement of block CG as include/ddm_hip.h states it for ddm_bcg_solve_multi (O'Leary's block CG with a pseudo-inverse in the
m x m coupling), on the CPU oracle's operator, scalar product and preconditioner (tests/oracle_bridge.py: lists of per-rank vectors; a
block is a list of m such columns).  Test-side only.

  1. R = B - A X; def0_c = ||R_c||; a column with def0_c < 1e-30 has converged with 0 iterations and stays in the block.
  2. Z = M^-1 R; P = Z.
  3. k = 1 .. maxit while some column fails: Q = A P; W = P^T Q; S = P^T R; W^+ = sym_pinv(W, rank_tol); alpha = W^+ S; X += P alpha;
     R -= Q alpha; def_c = ||R_c||; Z = M^-1 R; (stop if every column passes) beta = -W^+ (Q^T Z); P = Z + P beta.
  4. column c passes when def_c < reduction def0_c or def_c < 1e-30; iterations_c = the first k at which it passed."""
import numpy as np

from tests.oracle_bridge import oracle_objects


def sym_pinv(W, tol):
    """pseudo-inverse of (W + W^T) / 2: Jacobi scaling d_i = sqrt(|W_ii|) (1 where W_ii = 0), eigen-decomposition of the scaled matrix,
    eigenvalues <= tol lambda_max dropped, the rest inverted, scaled back.  Returns (W^+, rank)."""
    W = np.asarray(W, dtype=float)
    d = np.sqrt(np.abs(np.diag(W)))
    d[d == 0.0] = 1.0
    G = 0.5 * (W + W.T) / d[:, None] / d[None, :]
    lam, Q = np.linalg.eigh(G)
    keep = lam > tol * lam[-1] if lam[-1] > 0.0 else np.zeros(len(lam), dtype=bool)
    Wp = (Q[:, keep] / lam[keep]) @ Q[:, keep].T
    return Wp / d[:, None] / d[None, :], int(keep.sum())


def bcg_solve(op, sp_, prec, X, B, reduction=1e-10, maxit=1000, rank_tol=1e-12, trace=None):
    """X, B: lists of m columns, each a list of per-rank vectors; both overwritten (X: solutions, B: defects).  trace (optional list):
    receives W of every iteration.  Returns (per-column iterations, per-column converged flags, history (k_end + 1) x m, ranks per
    iteration)."""
    m, nr = len(X), len(X[0])

    def zeros():
        return [np.zeros_like(v) for v in X[0]]

    def gram(U, V):
        return np.array([[sp_.dot(U[i], V[j]) for j in range(m)] for i in range(m)])

    def combine(U, C, j):
        """sum_i U_i C[i, j], the products added in ascending i"""
        out = zeros()
        for i in range(m):
            for r in range(nr):
                out[r] = out[r] + U[i][r] * C[i, j] if i else U[i][r] * C[i, j]
        return out

    def precondition():
        Z = []
        for c in range(m):
            z = zeros()
            prec.apply(z, B[c])
            Z.append(z)
        return Z

    for c in range(m):
        op.applyscaleadd(-1.0, X[c], B[c])
    def0 = np.array([sp_.norm(B[c]) for c in range(m)])
    if np.isnan(def0).any():
        raise FloatingPointError("initial defect is NaN")
    hist = [def0.copy()]
    first = np.where(def0 < 1e-30, 0, -1)
    ranks = []

    def passes(d):
        return (d < reduction * def0) | (d < 1e-30)

    k = 0
    failing = ~passes(def0)
    if failing.any() and maxit > 0:
        Z = precondition()
        P = [[v.copy() for v in z] for z in Z]
    while failing.any() and k < maxit:
        k += 1
        Q = []
        for c in range(m):
            q = zeros()
            op.apply(P[c], q)
            Q.append(q)
        W, S = gram(P, Q), gram(P, B)
        if trace is not None:
            trace.append(W.copy())
        Wp, rank = sym_pinv(W, rank_tol)
        ranks.append(rank)
        if rank == 0:
            raise ZeroDivisionError("breakdown in block CG - P^T A P has rank 0")
        alpha = Wp @ S
        for c in range(m):
            dx, dr = combine(P, alpha, c), combine(Q, alpha, c)
            for r in range(nr):
                X[c][r] += dx[r]
                B[c][r] -= dr[r]
        d = np.array([sp_.norm(B[c]) for c in range(m)])
        hist.append(d.copy())
        if np.isnan(d).any():
            raise FloatingPointError("defect is NaN")
        Z = precondition()
        ok = passes(d)
        first = np.where(ok & (first < 0), k, first)
        failing = ~ok
        if not failing.any():
            break
        beta = -Wp @ gram(Q, Z)
        Pn = []
        for c in range(m):
            pb = combine(P, beta, c)
            Pn.append([Z[c][r] + pb[r] for r in range(nr)])
        P = Pn
    its = np.where(first >= 0, first, k)
    return [int(i) for i in its], [bool(v) for v in passes(hist[-1])], np.array(hist), ranks


def reference_solve(dec, Bcols=None, reduction=1e-10, maxit=1000, rank_tol=1e-12, trace=None, **kw):
    """the restatement on a Decomposition from a zero start (kw: oracle_objects' configuration).  Bcols: list of m columns, each a list
    of per-rank vectors (default: the problem's right-hand side as one column).  Returns (iterations, converged, history, ranks, X as a
    list of m per-rank lists)."""
    op, sp_, prec, sch, gal = oracle_objects(dec, **kw)
    if Bcols is None:
        Bcols = [[sd.b.copy() for sd in dec.subs]]
    B = [[np.array(v, dtype=float) for v in col] for col in Bcols]
    X = [[np.zeros(sd.n_o) for sd in dec.subs] for _ in B]
    its, conv, hist, ranks = bcg_solve(op, sp_, prec, X, B, reduction, maxit, rank_tol, trace=trace)
    return its, conv, hist, ranks, X
