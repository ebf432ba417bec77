"""Block GMRES against independent recurrences on the same block (ddm_bgmres_solve_multi vs. ddm_gmres_solve_multi, ddm_fgmres_solve_multi and the
BiCGSTAB queue).

Workloads: `dg`, the bench_convdiff.py setup (Q1-DG convection-diffusion on 512 x 512 cells, 4x2 subdomains, overlap 2, direct local
solves, GenEO nev 16, standard Schwarz, additive, reduction 1e-8: a non-symmetric operator), and `poisson`, the bench.py setup (3-D Q1
Poisson on 216^3, 2x2x2 subdomains, overlap 2, ILU(0), GenEO nev 20) with RESTRICTED Schwarz (a non-symmetric preconditioner),
reduction 1e-10.  Right-hand sides: column 0 is the problem's, the others are seeded random consistent vectors.  For every width of
--m the same block is solved --runs times by solve_block_gmres, by solve_multi(solver="restartedgmressolver") (left-preconditioned: its
stop test is on the PRECONDITIONED defect, so its true reduction differs), by solve_multi(solver="restartedflexiblegmressolver") (the
true defect, as block GMRES; twice the basis memory -- recorded as refused where that does not fit) and by
solve_many(solver="bicgstabsolver", width=m) in turn, in one process, all with the same restart and maxit.  Per run: block iterations,
per-column iterations, seconds, ms per block iteration, the worst recomputed true reduction and the all-reduces issued.  One more run
each of block GMRES and of the independent GMRES block with the library's event timers on (ddm_timing_*) gives the split of an
iteration: applies, projection, combination, host algebra against applies, orthogonalisation, update.  The basis of both GMRES
drivers is allocated for min(restart, maxit) + 1 blocks of n x m doubles, so --maxit bounds the memory on the large workload.
Prints one JSON line.

    python tools/block_gmres_bench.py --workload dg|poisson [--m 8,32] [--restart 100] [--maxit N] [--runs 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TIMERS = ("Operator/apply", "CombinedPreconditioner/apply", "Schwarz/local solve", "BGMRES/project", "BGMRES/combine", "BGMRES/host",
          "GMRES/orthogonalisation", "GMRES/update")


def log(*a):
    print("[block_gmres_bench]", *a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="dg", choices=["dg", "poisson"])
    ap.add_argument("--cells", type=int, default=512, help="dg: cells per direction")
    ap.add_argument("--grid", type=int, default=216, help="poisson: grid points per direction")
    ap.add_argument("--m", default="8,32", help="block widths, comma separated (each <= 32)")
    ap.add_argument("--restart", type=int, default=100)
    ap.add_argument("--maxit", type=int, default=0, help="0: 1000 (dg), 60 (poisson: 61 basis blocks of 216^3 x 32 doubles are 156 GB)")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    widths = sorted({int(v) for v in args.m.split(",")})
    assert all(1 <= m <= 32 for m in widths) and args.runs >= 1

    import __graft_entry__ as ge
    ge.import_package()
    import torch
    from dune_ddm_amd import DdmError, synth
    from dune_ddm_amd.geneo import geneo_basis
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz

    t0 = time.perf_counter()
    if args.workload == "dg":
        C = args.cells
        dec = build_structured(synth.StructuredDG2D((C, C), (4, 2)), overlap=2, neumann=True)
        tl = TwoLevelSchwarz(dec, schwarz_type="standard", mode="additive", coarse="none", subdomain_solver="umfpack")
        tl.set_coarse_basis(geneo_basis(tl, nev=16, tol=1e-5))
        reduction, maxit = 1e-8, args.maxit or 1000
        workload = f"Q1-DG convection-diffusion {C}x{C} cells, 8 subdomains (4x2, overlap 2), direct local solves, GenEO nev 16, standard Schwarz, additive"
    else:
        G = args.grid
        dec = build_structured(synth.StructuredPoisson((G, G, G), (2, 2, 2)), overlap=2, pou_type="distance", shrink=0, neumann=True)
        tl = TwoLevelSchwarz(dec, schwarz_type="restricted", mode="additive", coarse="none")
        tl.set_coarse_basis(geneo_basis(tl, nev=20))
        reduction, maxit = 1e-10, args.maxit or 60
        workload = f"{G}^3 Q1 Poisson, 8 subdomains, overlap 2, ILU(0) restricted Schwarz + GenEO nev 20, additive"
    tl.rebuild_combined("additive")
    tl.schwarz.wait_setup()
    tl.ctx.sync()
    n = int(tl.rl.n_o)
    log(f"setup {time.perf_counter() - t0:.1f} s, n_o = {n}, local engine {tl.schwarz.engine()}")

    rng = np.random.default_rng(args.seed)
    cols = [np.asarray(tl.rl.b, dtype=np.float64)]
    for _ in range(max(widths) - 1):
        xg = rng.standard_normal(dec.nglobal)
        cols.append(tl.rl.cat_novlp([xg[sd.glob[:sd.n_o]] for sd in dec.subs]))
    Bd = tl.to_device(np.stack(cols, axis=1))
    del cols

    def true_reduction(B, X):
        R = B.clone()
        tl.op.applyscaleadd_multi(-1.0, X, R)
        return float(np.max(np.sqrt(tl.op.dot_multi(R, R) / tl.op.dot_multi(B, B))))

    def solve(name, B, m, mx, history=False):
        """-> (results, X, block iterations)"""
        if name == "block":
            res, _, X, w = tl.solve_block_gmres(B, reduction=reduction, maxit=mx, restart=args.restart, history=history)
            return res, X, len(w)
        if name in ("multi", "flexible"):
            res, _, X = tl.solve_multi(B, reduction=reduction, maxit=mx, restart=args.restart, history=history,
                                       solver="restartedgmressolver" if name == "multi" else "restartedflexiblegmressolver")
        else:
            res, _, X = tl.solve_many(B, width=m, reduction=reduction, maxit=mx, solver="bicgstabsolver", history=history)
        return res, X, max(int(x.iterations) for x in res)

    def timed(name, B, m):
        """one more run with the event timers on: ms per block iteration by timer, timer calls, all-reduces per block iteration"""
        tl.ctx.timing(True)
        tl.ctx.timing_reset()
        before = tl.ctx.comm_counts()
        res, X, k_end = solve(name, B, m, maxit)
        after = tl.ctx.comm_counts()
        tl.ctx.timing(False)
        k = max(k_end, 1)
        del X
        return {"block_iterations": k_end, "ms_per_block_iteration": {key: tl.ctx.timer(key)[0] / k for key in TIMERS if tl.ctx.timer(key)[1]},
                "calls": {key: int(tl.ctx.timer(key)[1]) for key in TIMERS if tl.ctx.timer(key)[1]},
                "allreduces_per_block_iteration": float(after[0] - before[0]) / k, "allreduce_doubles_per_block_iteration": float(after[1] - before[1]) / k}

    rows = []
    for m in widths:
        B = Bd[:, :m].contiguous()
        names, refused = [], {}
        for name in ("block", "multi", "flexible", "bicgstab_queue"):
            try:
                solve(name, B, m, 3)                                       # warm-up (graph capture, scratch)
                solve(name, B, m, min(maxit, args.restart + 1))            # ... and the basis of the timed runs fits
                names.append(name)
            except DdmError as e:
                refused[name] = str(e)
                log(f"m = {m} {name}: refused: {e}")
        runs = {name: [] for name in names}
        for r in range(args.runs):
            for name in names:
                before = tl.ctx.comm_counts()
                res, X, k_end = solve(name, B, m, maxit)
                after = tl.ctx.comm_counts()
                el = float(res[0].elapsed_s)
                run = {"block_iterations": k_end, "iterations": [int(x.iterations) for x in res], "converged": all(bool(x.converged) for x in res),
                       "seconds": el, "ms_per_block_iteration": 1e3 * el / max(k_end, 1), "worst_true_reduction": true_reduction(B, X),
                       "allreduces": int(after[0] - before[0])}
                runs[name].append(run)
                log(f"m = {m} run {r} {name}: {k_end} block iterations, {el:.3f} s ({run['ms_per_block_iteration']:.2f} ms each), converged "
                    f"{run['converged']}, worst true reduction {run['worst_true_reduction']:.2e}")
                del X
        prof = {name: timed(name, B, m) for name in ("block", "multi")}
        best = {name: min(x["seconds"] for x in runs[name]) for name in runs}
        rows.append({"m": m, "runs": runs, "refused": refused, "best_seconds": best, "winner_time_to_solution": min(best, key=best.get), "timers": prof})
        log(f"m = {m}: best {best}; timers {prof}")
    out = {"workload": f"{workload}, reduction {reduction:g}, restart {args.restart}, maxit {maxit}", "n_o": n, "device": torch.cuda.get_device_name(0),
           "rows": rows,
           "what": "block = ddm_bgmres_solve_multi (solve_block_gmres), multi = ddm_gmres_solve_multi (solve_multi, left-preconditioned restarted GMRES, "
                   "independent columns, stop test on the preconditioned defect), flexible = ddm_fgmres_solve_multi (true defect), bicgstab_queue = ddm_bicgstab_solve_queue (solve_many, width m) on the same block, in turn; seconds = wall time "
                   "of the loop; block_iterations of bicgstab_queue = the largest per-column count (two applies each); timers: ms per block iteration "
                   "of one more run with the event timers on"}
    print(json.dumps(out))
    tl.ctx.close()


if __name__ == "__main__":
    main()
