"""Numpy restatement of block GMRES as include/ddm_hip.h states it for ddm_bgmres_solve_multi (right-preconditioned block GMRES with a
fixed preconditioner, deflation of the block at every cycle start, block classical Gram-Schmidt applied twice), on the CPU oracle's
operator, scalar product and preconditioner (tests/oracle_bridge.py: lists of per-rank vectors; a block is a list of such columns).
Test-side only.

  1. R = B - A X; def0_c = ||R_c||; a column with def0_c < 1e-30 has converged with 0 iterations and is never touched.
  2. cycle start: G = R^T R over the running columns; (T, C0, p) = factor(G); V_0 = R C0 (n x p, orthonormal), R = V_0 T.
  3. step j: W = A M^-1 V_j; H1 = [V_0 .. V_j]^T W; W -= [V_0 .. V_j] H1; H2 and a second subtraction; G_W = W^T W;
     (S, C, rank) = factor(G_W, scaled by the column norms of W before the orthogonalisation); the block Hessenberg matrix gets the
     column block [H1 + H2; S]; per column the monitored defect is the residual of min ||E_1 T e_c - Hbar y||; rank = p: V_{j+1} = W C;
     rank < p: the cycle ends after this step.
  4. cycle end (restart, maxit, exhaustion, every running column passes): U = [V_0 .. V_{j-1}] Y; Z = M^-1 U; X += Z; R -= A Z; the
     norms are recomputed and replace the history row of the cycle's last step.
  5. iterations_c = the first block iteration at which c passed and stayed passed."""
import numpy as np

from tests.oracle_bridge import oracle_objects


def factor(G, scale2, tol):
    """G (p x p, symmetric positive semi-definite) = S^T S with S (rank x p), and C (p x rank) with C^T G C = I: Jacobi scaling
    d_c = sqrt(scale2_c) (1 where scale2_c = 0; scale2 None: the diagonal of G), eigen-decomposition of D^-1 (G + G^T)/2 D^-1, the
    eigenvalues above tol lambda_max kept (largest first): S = Lambda^1/2 U^T D, C = D^-1 U Lambda^-1/2.  Returns (S, C, rank)."""
    G = np.asarray(G, dtype=float)
    d = np.sqrt(np.abs(np.diag(G) if scale2 is None else np.asarray(scale2, dtype=float)))
    d[d == 0.0] = 1.0
    lam, U = np.linalg.eigh(0.5 * (G + G.T) / d[:, None] / d[None, :])
    keep = lam > tol * lam[-1] if lam[-1] > 0.0 else np.zeros(len(lam), dtype=bool)
    lam, U = lam[keep][::-1], U[:, keep][:, ::-1]
    sq = np.sqrt(lam)
    return (sq[:, None] * U.T) * d[None, :], (U / sq[None, :]) / d[:, None], int(keep.sum())


def bgmres_solve(op, sp_, prec, X, B, reduction=1e-10, maxit=1000, restart=100, rank_tol=1e-12, gaps=None):
    """X, B: lists of m columns, each a list of per-rank vectors; both overwritten (X: solutions, B: defects).  gaps (optional list):
    receives, per cycle, max_c |monitored - recomputed| / def0_c over the running columns.  Returns (per-column iterations, per-column
    converged flags, history (k_end + 1) x m, widths per block iteration)."""
    m, nr = len(X), len(X[0])

    def zeros():
        return [np.zeros_like(v) for v in X[0]]

    def gram(U, V):
        return np.array([[sp_.dot(u, v) for v in V] for u in U]).reshape(len(U), len(V))

    def combine(blocks, Cs, q):
        """sum_k blocks[k] Cs[k] (n x q): per entry the products added in ascending block and column index"""
        out = []
        for c in range(q):
            acc = zeros()
            first = True
            for Vk, Ck in zip(blocks, Cs):
                for i, v in enumerate(Vk):
                    for r in range(nr):
                        acc[r] = v[r] * Ck[i, c] if first else acc[r] + v[r] * Ck[i, c]
                    first = False
            out.append(acc)
        return out

    def apply_block(V):
        """A M^-1 V and M^-1 V"""
        Zs, Ws = [], []
        for v in V:
            z, w = zeros(), zeros()
            prec.apply(z, v)
            op.apply(z, w)
            Zs.append(z)
            Ws.append(w)
        return Zs, Ws

    for c in range(m):
        op.applyscaleadd(-1.0, X[c], B[c])
    def0 = np.array([sp_.norm(B[c]) for c in range(m)])
    if np.isnan(def0).any():
        raise FloatingPointError("initial defect is NaN")
    live = def0 >= 1e-30

    def passes(d):
        return (d < reduction * def0) | (d < 1e-30)

    hist = [def0.copy()]
    widths = []
    defect = def0.copy()
    first = np.where(live, -1, 0)
    k = 0
    while (first < 0).any() and k < maxit:
        run = first < 0
        idx = np.flatnonzero(run)
        G = np.zeros((m, m))
        G[np.ix_(idx, idx)] = gram([B[c] for c in idx], [B[c] for c in idx])
        T, C0, p = factor(G, None, rank_tol)
        T[:, ~run] = 0.0
        C0[~run, :] = 0.0
        if p == 0:
            raise ZeroDivisionError("breakdown in block GMRES - the running defects have rank 0")
        V = [combine([B], [C0], p)]
        Hbar = np.zeros((p, 0))
        rhs = np.zeros((p, m))
        rhs[:p] = T
        j, done = 0, False
        mon = defect.copy()
        while j < restart and k < maxit and not done:
            Zs, W = apply_block(V[j])
            Hsum = np.zeros(((j + 1) * p, p))
            for _ in range(2):
                Hc = np.vstack([gram(Vk, W) for Vk in V])
                upd = combine(V, [Hc[a * p:(a + 1) * p] for a in range(j + 1)], p)
                W = [[W[c][r] - upd[c][r] for r in range(nr)] for c in range(p)]
                Hsum += Hc
            GW = gram(W, W)
            S, C, rank = factor(GW, np.sum(Hsum * Hsum, axis=0) + np.diag(GW), rank_tol)
            new = np.zeros(((j + 2) * p, (j + 1) * p))
            new[:(j + 1) * p, :j * p] = Hbar
            new[:(j + 1) * p, j * p:] = Hsum
            new[(j + 1) * p:(j + 1) * p + rank, j * p:] = S
            Hbar = new
            rhs = np.vstack([rhs, np.zeros((p, m))])
            Q, Rf = np.linalg.qr(Hbar, mode="complete")
            g = Q.T @ rhs
            j += 1
            k += 1
            widths.append(p)
            mon = np.where(run, np.sqrt(np.sum(g[j * p:] ** 2, axis=0)), defect)
            hist.append(mon.copy())
            if np.isnan(mon).any():
                raise FloatingPointError("defect is NaN")
            ok = passes(mon)
            first = np.where(run & ok & (first < 0), k, first)
            first = np.where(run & ~ok, -1, first)
            if rank < p or not (run & ~ok).any():
                done = True
            else:
                V.append(combine([W], [C], p))
        Y = np.linalg.solve(Rf[:j * p, :j * p], g[:j * p]) if j else np.zeros((0, m))
        Y[:, ~run] = 0.0
        U = combine(V[:j], [Y[a * p:(a + 1) * p] for a in range(j)], m)
        for c in idx:
            z, w = zeros(), zeros()
            prec.apply(z, U[c])
            op.apply(z, w)
            for r in range(nr):
                X[c][r] += z[r]
                B[c][r] -= w[r]
        defect = np.where(run, np.array([sp_.norm(B[c]) for c in range(m)]), defect)
        if gaps is not None:
            gaps.append(float(np.max(np.abs(mon[run] - defect[run]) / def0[run])))
        hist[-1] = defect.copy()
        ok = passes(defect)
        first = np.where(run & ok & (first < 0), k, first)
        first = np.where(run & ~ok, -1, first)
    its = np.where(first >= 0, first, k)
    return [int(i) for i in its], [bool(v) for v in passes(defect)], np.array(hist), widths


def reference_solve(dec, Bcols=None, reduction=1e-10, maxit=1000, restart=100, rank_tol=1e-12, gaps=None, X0=None, **kw):
    """the restatement on a Decomposition (kw: oracle_objects' configuration), from X0 (list of m per-rank lists) or zero.  Bcols: list of
    m columns, each a list of per-rank vectors (default: the problem's right-hand side as one column).  Returns (iterations, converged,
    history, widths, X as a list of m per-rank lists)."""
    op, sp_, prec, sch, gal = oracle_objects(dec, **kw)
    if Bcols is None:
        Bcols = [[sd.b.copy() for sd in dec.subs]]
    B = [[np.array(v, dtype=float) for v in col] for col in Bcols]
    X = [[np.zeros(sd.n_o) for sd in dec.subs] for _ in B] if X0 is None else [[np.array(v, dtype=float) for v in col] for col in X0]
    its, conv, hist, widths = bgmres_solve(op, sp_, prec, X, B, reduction, maxit, restart, rank_tol, gaps=gaps)
    return its, conv, hist, widths, X
