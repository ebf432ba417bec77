"""Restarted GMRES for several right-hand sides at once against sequential solves (ddm_gmres_solve_multi vs. m calls of ddm_gmres_solve).

Problems, built as bench_convdiff.py builds them: BASELINE configs[3] (Q1-DG convection-diffusion 512^2, 8 subdomains, `umfpack` local
solves, GenEO, additive, GMRES(100) to 1e-8; the default) and --problem elasticity (configs[4]: P1 elasticity bar, `cholmod`, restricted
Schwarz, multiplicative GenEO level, GMRES(100) to 1e-6).  Right-hand sides: column 0 is the problem's, the others are seeded random
consistent vectors.  For every m of --m the same m right-hand sides are solved (a) as one block and (b) one after the other (each column
once; the sequential time of m columns is the sum over the first m).  Prints a table and one JSON line: RHS-iterations per second of
both, their ratio, and the per-iteration breakdown of a --profile-iters run with the library's event timers (local solve, coarse level,
operator, orthogonalisation; the single-vector loop has no orthogonalisation timer: its share is the rest of the wall time).
--solver restartedflexiblegmressolver measures ddm_fgmres_solve_multi / ddm_fgmres_solve instead; restartedfcgsolver and
completefcgsolver measure flexible CG with --mmax + 1 slots (ddm_fcg_solve_multi / ddm_fcg_solve), cgsolver the block CG they are
compared with (ddm_cg_solve_multi / ddm_cg_solve).  The CG family needs a symmetric positive definite operator: --problem poisson (Q1
Poisson --cells^3, 8 subdomains, ILU(0), restricted Schwarz, POU coarse space, additive, to 1e-10; restricted Schwarz is not symmetric,
so cgsolver is there for its cost per iteration, not for its convergence).  Every row also carries the largest
reported and the largest recomputed true reduction ||b - A x|| / ||b|| of its columns and the bytes of the Krylov bases.

The measurement runs in a child process under `timeout -k 10 --step-timeout`; the parent only starts it and passes its exit code on.

    python tools/multi_gmres_bench.py [--problem dg|elasticity|poisson] [--solver ...] [--mmax 3] [--m 1,4,8,16]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TIMERS = {"local solve": "Schwarz/local solve", "coarse": "GalerkinPrec/apply", "operator": "Operator/apply",
          "orthogonalisation": "GMRES/orthogonalisation", "update": "GMRES/update", "preconditioner": "CombinedPreconditioner/apply"}


def log(*a):
    print("[multi_gmres_bench]", *a, file=sys.stderr, flush=True)


FCG = ("restartedfcgsolver", "completefcgsolver")


def solver_name(args):
    if args.solver in FCG:
        return f"{'restarted' if args.solver == FCG[0] else 'complete'} flexible CG(mmax = {args.mmax})"
    if args.solver == "cgsolver":
        return "CG"
    return ("flexible GMRES" if args.solver == "restartedflexiblegmressolver" else "GMRES") + f"({args.restart})"


def krylov_blocks(args):
    """n x m blocks the driver keeps next to x and b"""
    if args.solver in FCG:
        return 2 * (min(args.mmax, args.maxit) + 1)
    if args.solver == "cgsolver":
        return 2
    return (2 if args.solver == "restartedflexiblegmressolver" else 1) * min(args.restart, args.maxit) + 2


def build(args):
    from dune_ddm_amd import synth
    from dune_ddm_amd.geneo import geneo_basis
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz
    if args.problem == "poisson":
        cells = args.cells or 128
        grid = synth.StructuredPoisson((cells, cells, cells), (2, 2, 2))
        dec = build_structured(grid, overlap=2, pou_type="distance")
        cfg = dict(schwarz_type="restricted", mode="additive", reduction=1e-10)
        tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type=cfg["schwarz_type"], mode=cfg["mode"])
        tl.schwarz.wait_setup()
        tl.ctx.sync()
        return dec, tl, cfg, f"Q1 Poisson {cells}^3 = {grid.nglobal} DoF, 8 subdomains (overlap 2), ILU(0), restricted, POU coarse space, additive, {solver_name(args)} to 1e-10"
    if args.problem == "dg":
        cells = args.cells or 512
        grid = synth.StructuredDG2D((cells, cells), (4, 2))
        dec = build_structured(grid, overlap=2, neumann=True)
        cfg = dict(schwarz_type="standard", mode="additive", reduction=1e-8, tol=1e-5, nev=args.nev, local="umfpack")
        workload = f"Q1-DG convection-diffusion {cells}^2 cells = {grid.nglobal} DoF, 8 subdomains (overlap 2), umfpack, GenEO nev {args.nev}, additive"
    else:
        grid = synth.StructuredElasticity(refine=args.refine, parts=8)
        dec = build_structured(grid, overlap=1, neumann=True, second_region="all")
        cfg = dict(schwarz_type="restricted", mode="multiplicative", reduction=1e-6, tol=1e-6, nev=min(args.nev, 12), local="cholmod")
        workload = f"P1 elasticity bar, refine {args.refine} = {grid.nglobal} DoF, 8 subdomains (overlap 1), cholmod, GenEO nev {cfg['nev']}, restricted, multiplicative"
    tl = TwoLevelSchwarz(dec, schwarz_type=cfg["schwarz_type"], mode=cfg["mode"], coarse="none", subdomain_solver=cfg["local"])
    tl.set_coarse_basis(geneo_basis(tl, nev=cfg["nev"], tol=cfg["tol"]))
    tl.rebuild_combined(cfg["mode"])
    tl.schwarz.wait_setup()
    tl.ctx.sync()
    return dec, tl, cfg, workload + f", {solver_name(args)} to {cfg['reduction']:g}"


def timers_per_iteration(tl, iters):
    return {k: tl.ctx.timer(name)[0] / iters for k, name in TIMERS.items()}


def worker(args):
    import __graft_entry__ as ge
    ge.import_package()
    import torch
    ms_ = sorted({int(v) for v in args.m.split(",")})
    if args.solver in FCG:
        TIMERS["orthogonalisation"] = "FCG/orthogonalisation"
    assert all(1 <= m <= 32 for m in ms_)
    t0 = time.perf_counter()
    dec, tl, cfg, workload = build(args)
    log(f"setup {time.perf_counter() - t0:.1f} s, n_o = {tl.rl.n_o}, local engine {tl.schwarz.engine()}")
    kw = dict(solver=args.solver, restart=args.restart, mmax=args.mmax)

    def true_reductions(X, B0):
        """||b - A x|| / ||b|| per column, recomputed"""
        Y = torch.zeros_like(X)
        tl.op.apply_multi(X, Y)
        R = B0 - Y
        return np.sqrt(tl.op.dot_multi(R, R) / tl.op.dot_multi(B0, B0))
    mmax = max(ms_)
    rng = np.random.default_rng(args.seed)
    cols = [np.asarray(tl.rl.b, dtype=np.float64)]
    for _ in range(mmax - 1):
        xg = rng.standard_normal(dec.nglobal)
        cols.append(tl.rl.cat_novlp([xg[sd.glob[:sd.n_o]] for sd in dec.subs]))
    Bh = np.stack(cols, axis=1)
    Bd = tl.to_device(Bh)
    P = args.profile_iters

    # (b) sequential single-vector solves, each column once
    tl.solve(reduction=0.0, maxit=5, history=False, b=Bh[:, 0], **kw)          # warm-up
    seq = []
    for c in range(max(ms_)):
        res, _, _ = tl.solve(reduction=cfg["reduction"], maxit=args.maxit, history=False, b=Bh[:, c], **kw)
        seq.append((int(res.iterations), float(res.elapsed_s), bool(res.converged)))
        log(f"single column {c}: {res.iterations} iterations, {res.elapsed_s * 1e3:.1f} ms")
    tl.ctx.timing(True)
    tl.ctx.timing_reset()
    res, _, _ = tl.solve(reduction=0.0, maxit=P, history=False, b=Bh[:, 0], **kw)
    tl.ctx.timing(False)
    single_prof = timers_per_iteration(tl, P)
    single_prof["wall"] = 1e3 * float(res.elapsed_s) / P

    # (a) one block solve per width
    rows = []
    for m in ms_:
        B = Bd[:, :m].contiguous()
        tl.ctx.timing(True)
        tl.ctx.timing_reset()
        res, _, _ = tl.solve_multi(B, reduction=0.0, maxit=P, history=False, **kw)   # (also the warm-up of this width)
        tl.ctx.timing(False)
        prof = timers_per_iteration(tl, P)
        prof["wall"] = 1e3 * float(res[0].elapsed_s) / P
        res, _, X = tl.solve_multi(B, reduction=cfg["reduction"], maxit=args.maxit, history=False, **kw)
        its = [int(r.iterations) for r in res]
        el = float(res[0].elapsed_s)
        true_red = true_reductions(X, B)
        seq_its = [s[0] for s in seq[:m]]
        seq_el = sum(s[1] for s in seq[:m])
        row = {"m": m, "iterations": its, "sequential_iterations": seq_its, "converged": all(r.converged for r in res),
               "block_s": el, "sequential_s": seq_el, "ms_per_block_iteration": 1e3 * el / max(its),
               "rhs_iterations_per_s": sum(its) / el, "sequential_rhs_iterations_per_s": sum(seq_its) / seq_el,
               "ms_per_block_iteration_by_timer": prof, "reported_reduction_max": max(float(r.reduction) for r in res),
               "true_reduction_max": float(np.max(true_red)),
               "basis_bytes": krylov_blocks(args) * int(tl.rl.n_o) * m * 8}
        row["ratio"] = row["rhs_iterations_per_s"] / row["sequential_rhs_iterations_per_s"]
        rows.append(row)
        del X
    tl.prec.check_status()

    hdr = f"{'m':>3} {'block it':>8} {'ms/it':>8} {'RHS-it/s':>10} {'seq RHS-it/s':>12} {'ratio':>6} | " + " ".join(f"{k[:9]:>9}" for k in TIMERS)
    print(hdr)
    print(f"{'seq':>3} {seq[0][0]:>8} {single_prof['wall']:>8.2f} {'':>10} {'':>12} {'':>6} | " + " ".join(f"{single_prof[k]:>9.3f}" for k in TIMERS))
    for r in rows:
        p = r["ms_per_block_iteration_by_timer"]
        print(f"{r['m']:>3} {max(r['iterations']):>8} {r['ms_per_block_iteration']:>8.2f} {r['rhs_iterations_per_s']:>10.0f} "
              f"{r['sequential_rhs_iterations_per_s']:>12.0f} {r['ratio']:>6.2f} | " + " ".join(f"{p[k]:>9.3f}" for k in TIMERS))
    for r in rows:
        print(f"m = {r['m']}: reported reduction (max over the columns) {r['reported_reduction_max']:.3e}, recomputed true reduction {r['true_reduction_max']:.3e}, "
              f"basis and work blocks {r['basis_bytes'] / 2**20:.1f} MiB")
    out = {"workload": workload, "solver": args.solver, "problem": args.problem, "n_o": int(tl.rl.n_o), "device": torch.cuda.get_device_name(0), "restart": args.restart,
           "mmax": args.mmax if args.solver in FCG else None, "profile_iters": P, "single_ms_per_iteration_by_timer": single_prof, "rows": rows,
           "what": "rhs_iterations_per_s = sum of the columns' iterations / wall time of the solve; sequential = the same columns solved one by one "
                   "with the single-vector driver; *_by_timer: ms per (block) iteration of a run of profile_iters iterations (reduction 0) with the event timers on"}
    print(json.dumps(out))
    tl.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", default="dg", choices=["dg", "elasticity", "poisson"])
    ap.add_argument("--cells", type=int, default=None, help="cells per direction (default: dg 512, poisson 128)")
    ap.add_argument("--refine", type=int, default=1)
    ap.add_argument("--nev", type=int, default=16)
    ap.add_argument("--restart", type=int, default=100)
    ap.add_argument("--solver", default="restartedgmressolver",
                    choices=["restartedgmressolver", "restartedflexiblegmressolver", "restartedfcgsolver", "completefcgsolver", "cgsolver"],
                    help="restartedflexiblegmressolver: ddm_fgmres_solve(_multi), right-preconditioned, two bases; restartedfcgsolver / completefcgsolver: "
                         "ddm_fcg_solve(_multi) with --mmax; cgsolver: ddm_cg_solve(_multi)")
    ap.add_argument("--mmax", type=int, default=10, help="flexible CG: slots 0 .. mmax")
    ap.add_argument("--m", default="1,4,8,16", help="block widths, comma separated (each <= 32)")
    ap.add_argument("--maxit", type=int, default=1000)
    ap.add_argument("--profile-iters", type=int, default=20, help="iterations of the timer runs")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=540, help="seconds the measuring child process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, cwd=ROOT))


if __name__ == "__main__":
    main()
