"""Numpy restatement of flexible CG as include/ddm_hip.h states it for ddm_fcg_solve (dune-istl's RestartedFCGSolver and
CompleteFCGSolver: CG for a symmetric positive definite operator whose preconditioner is not symmetric or not fixed; the true defect
is tested), on the CPU oracle's operator, scalar product and preconditioner (tests/oracle_bridge.py: lists of per-rank vectors).
Test-side only.

  1. b -= A x; def0 = ||b||; def0 < 1e-30: converged at once.
  2. i = 1, s = 0, klimit = 0; while i <= maxit and not stopped: { while s <= mmax, i <= maxit and not stopped: d_s = M^-1 b;
     J = {0 .. s - 1} (restarted) or {k < klimit, k != s}, then if klimit <= s: ++klimit (complete); c_k = <Ad_k, d_s> / g_k for every
     k in J from the UNMODIFIED d_s; d_s -= c_k d_k in ascending k; Ad_s = A d_s; g_s = <d_s, Ad_s>; alpha = <d_s, b> / g_s;
     x += alpha d_s; b -= alpha Ad_s; def = ||b||; stop when def < reduction def0 or def < 1e-30; ++i; ++s.  End of a pass: slot 0 <->
     slot mmax and s = 1 (restarted); s = 0 and klimit = mmax + 1 (complete). }
  3. iterations = i - 1, reduction = def / def0."""
import numpy as np

from tests.oracle_bridge import oracle_objects


def fcg_solve(op, sp_, prec, x, b, reduction=1e-10, maxit=1000, mmax=10, complete=False, prec_apply=None, windows=None):
    """x, b: lists of per-rank vectors, both overwritten (x: solution, b: defect).  prec_apply(j, z, v) (optional) replaces
    prec.apply(z, v) in global iteration j = 0, 1, ... -- a preconditioner that changes from step to step.  windows (optional list):
    receives, per iteration, (d_s, Ad_s, g_s, [(d_k, Ad_k, g_k) for k in J]) with copies of the vectors: the fresh direction after its
    orthogonalisation and the slots it was orthogonalised against.
    Returns (iterations, converged, [def_0, def_1, ...], def / def0)."""
    P = len(x)

    def zeros():
        return [np.zeros_like(v) for v in x]

    op.applyscaleadd(-1.0, x, b)
    def0 = sp_.norm(b)
    hist = [def0]
    if def0 < 1e-30:
        return 0, True, hist, 0.0
    d = [None] * (mmax + 1)
    Ad = [None] * (mmax + 1)
    g = [0.0] * (mmax + 1)
    i, s, klimit = 1, 0, 0
    stop = False
    norm = def0
    while i <= maxit and not stop:
        while s <= mmax and i <= maxit and not stop:
            d[s] = zeros()
            if prec_apply is not None:
                prec_apply(i - 1, d[s], b)
            else:
                prec.apply(d[s], b)
            if complete:
                J = [k for k in range(klimit) if k != s]
                if klimit <= s:
                    klimit += 1
            else:
                J = list(range(s))
            c = [sp_.dot(Ad[k], d[s]) / g[k] for k in J]               # all from the unmodified d_s
            for ck, k in zip(c, J):
                for r in range(P):
                    d[s][r] -= ck * d[k][r]
            Ad[s] = zeros()
            op.apply(d[s], Ad[s])
            g[s] = sp_.dot(d[s], Ad[s])
            if g[s] == 0.0:
                raise ZeroDivisionError("breakdown in FCG - <d, A d> == 0.0")
            alpha = sp_.dot(d[s], b) / g[s]
            for r in range(P):
                x[r] += alpha * d[s][r]
                b[r] -= alpha * Ad[s][r]
            norm = sp_.norm(b)
            hist.append(norm)
            if windows is not None:
                windows.append(([v.copy() for v in d[s]], [v.copy() for v in Ad[s]], g[s],
                                [([v.copy() for v in d[k]], [v.copy() for v in Ad[k]], g[k]) for k in J]))
            if norm < def0 * reduction or norm < 1e-30:
                stop = True
            i += 1
            s += 1
        if s <= mmax:
            break
        if complete:
            s, klimit = 0, mmax + 1
        else:
            d[0], d[mmax] = d[mmax], d[0]
            Ad[0], Ad[mmax] = Ad[mmax], Ad[0]
            g[0], g[mmax] = g[mmax], g[0]
            s = 1
    return i - 1, stop, hist, norm / def0


def reference_solve(dec, reduction=1e-10, maxit=1000, mmax=10, complete=False, b=None, windows=None, **kw):
    """the restatement on a Decomposition from a zero start (kw: oracle_objects' configuration); b: per-rank list (default: the
    problem's).  Returns (iterations, converged, history array, reduction, x as a per-rank list)."""
    op, sp_, prec, sch, gal = oracle_objects(dec, **kw)
    x = [np.zeros(sd.n_o) for sd in dec.subs]
    bb = [sd.b.copy() for sd in dec.subs] if b is None else [np.array(v, dtype=float) for v in b]
    it, conv, hist, red = fcg_solve(op, sp_, prec, x, bb, reduction, maxit, mmax, complete, windows=windows)
    return it, conv, np.asarray(hist, dtype=float), red, x
