"""Numpy restatement of flexible restarted GMRES as include/ddm_hip.h states it for ddm_fgmres_solve (dune-istl's
RestartedFlexibleGMResSolver: right preconditioning, the preconditioned directions are kept, the true defect is monitored), on the
CPU oracle's operator, scalar product and preconditioner (tests/oracle_bridge.py: lists of per-rank vectors).  Test-side only.

  1. b -= A x; beta = ||b||; def0 = beta; def0 < 1e-30: converged at once.
  2. per cycle: v_0 = b / beta; for i < restart: z_i = M^-1 v_i (kept); w = A z_i; modified Gram-Schmidt against v_0..v_i in the order
     k = 0..i; h_{i+1,i} = ||w||; v_{i+1} = w / h_{i+1,i}; Givens rotations on column i and on s; norm = |s_{i+1}|; stop when
     norm < reduction def0 or norm < 1e-30.  End of the cycle or stop: H y = s, x += sum_k y_k z_k; if not stopped: b -= A (sum_k y_k z_k),
     beta = ||b||.
  3. reduction = norm / def0, iterations = j."""
import numpy as np

from tests.oracle_bridge import oracle_objects


def generate_rotation(dx, dy):
    """the Givens rotation of dune-istl's GMRES (generatePlaneRotation), as gmres_generate_rotation in csrc/krylov_gmres.hpp"""
    ndx, ndy = abs(dx), abs(dy)
    if ndy < 1e-15:
        return 1.0, 0.0
    if ndx < 1e-15:
        return 0.0, 1.0
    if ndy > ndx:
        t = ndx / ndy
        cs = 1.0 / np.sqrt(1.0 + t * t)
        sn = cs
        cs *= t
        sn *= dx / ndx
        sn *= dy / ndy
        return cs, sn
    t = ndy / ndx
    cs = 1.0 / np.sqrt(1.0 + t * t)
    return cs, cs * (dy / dx)


def _back_substitute(H, s, cnt):
    y = np.zeros(cnt)
    for a in range(cnt - 1, -1, -1):
        t = s[a]
        for c in range(a + 1, cnt):
            t -= H[a, c] * y[c]
        y[a] = t / H[a, a]
    return y


def fgmres_solve(op, sp_, prec, x, b, reduction=1e-10, maxit=1000, restart=100, prec_apply=None, iterates=None):
    """x, b: lists of per-rank vectors, both overwritten (x: solution, b: defect).  prec_apply(j, z, v) (optional) replaces
    prec.apply(z, v) in global iteration j -- a preconditioner that changes from step to step.  iterates (optional list): receives a
    copy of the iterate x_j (per-rank list) after every iteration j = 1, 2, ..., formed from the part of the cycle computed so far.
    Returns (iterations, converged, [norm_0, norm_1, ...], norm / def0)."""
    P = len(x)
    R = restart

    def zeros():
        return [np.zeros_like(v) for v in x]

    def apply_prec(j, z, v):
        for r in range(P):
            z[r][:] = 0.0
        if prec_apply is not None:
            prec_apply(j, z, v)
        else:
            prec.apply(z, v)

    def combination(y, Z):
        upd = zeros()
        for a in range(len(y)):
            for r in range(P):
                upd[r] += y[a] * Z[a][r]
        return upd

    op.applyscaleadd(-1.0, x, b)
    norm = sp_.norm(b)
    def0 = norm
    hist = [def0]
    if def0 < 1e-30:
        return 0, True, hist, 0.0
    j, conv = 0, False
    while j < maxit and not conv:
        V = [[v * (1.0 / norm) for v in b]]
        Z = []
        s = np.zeros(R + 1)
        s[0] = norm
        H = np.zeros((R + 1, R))
        cs, sn = np.zeros(R), np.zeros(R)
        i = 0
        while i < R and j < maxit and not conv:
            Z.append(zeros())
            apply_prec(j, Z[i], V[i])
            w = zeros()
            op.apply(Z[i], w)
            for k in range(i + 1):
                H[k, i] = sp_.dot(V[k], w)
                for r in range(P):
                    w[r] -= H[k, i] * V[k][r]
            H[i + 1, i] = sp_.norm(w)
            if abs(H[i + 1, i]) < 1e-80:
                raise ZeroDivisionError("breakdown in GMRes - |w| == 0.0")
            V.append([v * (1.0 / H[i + 1, i]) for v in w])
            for k in range(i):
                t = cs[k] * H[k, i] + sn[k] * H[k + 1, i]
                H[k + 1, i] = -sn[k] * H[k, i] + cs[k] * H[k + 1, i]
                H[k, i] = t
            cs[i], sn[i] = generate_rotation(H[i, i], H[i + 1, i])
            t = cs[i] * H[i, i] + sn[i] * H[i + 1, i]
            H[i + 1, i] = -sn[i] * H[i, i] + cs[i] * H[i + 1, i]
            H[i, i] = t
            t = cs[i] * s[i] + sn[i] * s[i + 1]
            s[i + 1] = -sn[i] * s[i] + cs[i] * s[i + 1]
            s[i] = t
            norm = abs(s[i + 1])
            hist.append(norm)
            i += 1
            j += 1
            if iterates is not None:
                upd = combination(_back_substitute(H, s, i), Z)
                iterates.append([x[r] + upd[r] for r in range(P)])
            if norm < def0 * reduction or norm < 1e-30:
                conv = True
        upd = combination(_back_substitute(H, s, i), Z)
        for r in range(P):
            x[r] += upd[r]
        if not conv and j < maxit:
            op.applyscaleadd(-1.0, upd, b)
            norm = sp_.norm(b)
    return j, conv, hist, norm / def0


def reference_solve(dec, reduction=1e-10, maxit=1000, restart=100, b=None, iterates=None, **kw):
    """the restatement on a Decomposition from a zero start (kw: oracle_objects' configuration); b: per-rank list (default: the
    problem's).  Returns (iterations, converged, history array, reduction, x as a per-rank list)."""
    op, sp_, prec, sch, gal = oracle_objects(dec, **kw)
    x = [np.zeros(sd.n_o) for sd in dec.subs]
    bb = [sd.b.copy() for sd in dec.subs] if b is None else [np.array(v, dtype=float) for v in b]
    it, conv, hist, red = fgmres_solve(op, sp_, prec, x, bb, reduction, maxit, restart, iterates=iterates)
    return it, conv, np.asarray(hist, dtype=float), red, x
