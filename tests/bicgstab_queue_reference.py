"""Plain numpy restatement of the queue protocol of ddm_bicgstab_solve_queue (csrc/krylov_bicgstab.hpp) beside the single loop it must reproduce
(the evaluation order of oracle/apply_oracle.py::bicgstab_solve), on a small dense system A with a fixed right preconditioner W^-1
given as a matrix.  tests/test_bicgstab_queue_cpu.py asserts on it what the device driver relies on:

  * a fresh slot (p = v = 0, rho = alpha = omega = 1) run through the GENERAL direction update gives p = r bit for bit, so the queue
    has no first step and the slots need not be aligned;
  * a column that passes the stop test after a first half step is masked out of the second: x, r and its scalars stay;
  * there is one boundary per iteration, after the second half step: store, release, refill in ascending slot order, a column with
    def0 < 1e-30 (or maxit = 0) finished at once and its slot refilled again;
  * the breakdown checks run on the operands the single loop checks: rho and omega as used by the direction update, h = <rt, v>.

Every sum is np.dot on contiguous float64 vectors in both loops, so equal operands give equal bits."""
import numpy as np

EPS = 1e-80


class Breakdown(ArithmeticError):
    def __init__(self, scalar, value, column=None):
        super().__init__(f"breakdown in BiCGSTAB: {scalar} = {value!r}" + ("" if column is None else f" in column {column}"))
        self.scalar, self.value, self.column = scalar, value, column


def dot(u, v):
    return float(np.dot(np.ascontiguousarray(u), np.ascontiguousarray(v)))


def direction(p, v, r, beta, omega):
    """p = r + beta (p - omega v) as the single loop evaluates it: p += (-omega) v; p *= beta; p += r"""
    p = p + (-omega) * v
    p = p * beta
    return p + r


def single(A, Winv, x0, b, reduction, maxit):
    """the single loop, with its `it < 1` branch.  Returns dict(x, hist, iterations, converged)."""
    x = np.array(x0, dtype=np.float64)
    r = np.array(b, dtype=np.float64) - A @ x
    rt = r.copy()
    def0 = np.sqrt(dot(r, r))
    hist = [def0]
    if def0 < 1e-30:
        return dict(x=x, hist=np.array(hist), iterations=0, converged=True)
    p, v = np.zeros_like(r), np.zeros_like(r)
    rho = alpha = omega = 1.0
    it, conv = 0.5, False
    while it < maxit:
        rho_new = dot(rt, r)
        if abs(rho) <= EPS:
            raise Breakdown("rho", rho)
        if abs(omega) <= EPS:
            raise Breakdown("omega", omega)
        if it < 1:
            p = r.copy()
        else:
            p = direction(p, v, r, (rho_new / rho) * (alpha / omega), omega)
        y = Winv @ p
        v = A @ y
        h = dot(rt, v)
        if abs(h) < EPS:
            raise Breakdown("h", h)
        alpha = rho_new / h
        x = x + alpha * y
        r = r + (-alpha) * v
        hist.append(np.sqrt(dot(r, r)))
        if hist[-1] <= def0 * reduction:
            conv = True
            break
        it += 0.5
        y = Winv @ r
        t = A @ y
        omega = dot(t, r) / dot(t, t)
        x = x + omega * y
        r = r + (-omega) * t
        rho = rho_new
        hist.append(np.sqrt(dot(r, r)))
        if hist[-1] <= def0 * reduction:
            conv = True
            break
        it += 0.5
    return dict(x=x, hist=np.array(hist), iterations=int(np.ceil(min(it, maxit))), converged=conv)


def queue(A, Winv, X0, B, width, reduction, maxit):
    """M columns through `width` slots.  Returns dict(X, hist ((2 maxit + 1) x M, NaN where not written), nhist, iterations, converged,
    frozen: [(column, iteration)] for every column that sat out a second half step while another slot ran it, and trace: per iteration
    the slot -> column table)."""
    B = np.asarray(B, dtype=np.float64)
    n, M = B.shape
    w = width
    X = np.array(X0, dtype=np.float64)
    hist = np.full((2 * maxit + 1, M), np.nan)
    nhist = np.zeros(M, dtype=np.int64)
    iterations = np.zeros(M, dtype=np.int64)
    converged = np.zeros(M, dtype=bool)
    x, r, rt, p, v = (np.zeros((n, w)) for _ in range(5))
    rho, alpha, omega, rho_new, def0 = (np.zeros(w) for _ in range(5))
    column = [-1] * w
    active = [False] * w
    nhalf = [0] * w
    conv = [False] * w
    nxt = 0
    frozen, trace = [], []

    def release(s):
        j = column[s]
        iterations[j] = (nhalf[s] + 1) // 2
        nhist[j] = nhalf[s] + 1
        converged[j] = conv[s]
        column[s] = -1

    def refill():
        nonlocal nxt
        while nxt < M:
            loaded = []
            for s in range(w):
                if column[s] < 0 and nxt < M:
                    column[s] = nxt
                    nxt += 1
                    loaded.append(s)
            if not loaded:
                break
            for s in loaded:
                j = column[s]
                x[:, s], r[:, s] = X[:, j], B[:, j]
                p[:, s] = v[:, s] = 0.0
                rho[s] = alpha[s] = omega[s] = 1.0
                r[:, s] = r[:, s] - A @ x[:, s]
                rt[:, s] = r[:, s]
                rho_new[s] = dot(r[:, s], r[:, s])          # <rt, r> = <r, r>: the sum the defect pass has formed
                def0[s] = np.sqrt(rho_new[s])
                hist[0, j] = def0[s]
                nhalf[s], conv[s] = 0, False
                if def0[s] < 1e-30 or maxit == 0:
                    conv[s] = def0[s] < 1e-30
                    release(s)
                else:
                    active[s] = True

    def record(s, norm):
        nhalf[s] += 1
        hist[nhalf[s], column[s]] = norm
        if norm <= def0[s] * reduction:
            conv[s] = True
            active[s] = False

    refill()
    it = 0
    while any(active):
        it += 1
        trace.append(list(column))
        y = np.zeros((n, w))
        for s in range(w):
            if not active[s]:
                continue
            if abs(rho[s]) <= EPS:
                raise Breakdown("rho", rho[s], column[s])
            if abs(omega[s]) <= EPS:
                raise Breakdown("omega", omega[s], column[s])
            beta = (rho_new[s] / rho[s]) * (alpha[s] / omega[s])
            p[:, s] = direction(p[:, s], v[:, s], r[:, s], beta, omega[s])     # the general step, also for a fresh slot
            y[:, s] = Winv @ p[:, s]
            v[:, s] = A @ y[:, s]
            h = dot(rt[:, s], v[:, s])
            if abs(h) < EPS:
                raise Breakdown("h", h, column[s])
            alpha[s] = rho_new[s] / h
            x[:, s] = x[:, s] + alpha[s] * y[:, s]
            r[:, s] = r[:, s] + (-alpha[s]) * v[:, s]
            record(s, np.sqrt(dot(r[:, s], r[:, s])))
        held = {s: (x[:, s].copy(), r[:, s].copy(), rho[s], alpha[s], omega[s]) for s in range(w) if column[s] >= 0 and not active[s]}
        if any(active):
            frozen += [(column[s], it) for s in held if nhalf[s] % 2 == 1]
            for s in range(w):
                if not active[s]:
                    continue
                y[:, s] = Winv @ r[:, s]
                t = A @ y[:, s]
                omega[s] = dot(t, r[:, s]) / dot(t, t)
                x[:, s] = x[:, s] + omega[s] * y[:, s]
                r[:, s] = r[:, s] + (-omega[s]) * t
                rho[s] = rho_new[s]
                rho_new[s] = dot(rt[:, s], r[:, s])
                record(s, np.sqrt(dot(r[:, s], r[:, s])))
                if active[s] and nhalf[s] >= 2 * maxit:
                    active[s] = False
        for s, (xs, rs, a, b_, c) in held.items():                             # a slot that sat out the second half step is as it was
            assert np.array_equal(x[:, s], xs) and np.array_equal(r[:, s], rs) and (rho[s], alpha[s], omega[s]) == (a, b_, c)
        stored = [s for s in range(w) if column[s] >= 0 and not active[s]]
        for s in stored:                                                         # the boundary
            X[:, column[s]] = x[:, s]
            release(s)
        if stored:
            refill()
    return dict(X=X, hist=hist, nhist=nhist, iterations=iterations, converged=converged, frozen=frozen, trace=trace)
