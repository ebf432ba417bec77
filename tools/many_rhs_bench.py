"""Many right-hand sides through a CG block of fixed width against the chunked block call (ddm_cg_solve_queue vs. ddm_cg_solve_multi on
w columns at a time, which is what a caller with more than 32 right-hand sides had to do before).

Workload: the bench.py setup (BASELINE configs[2]: 3-D Q1 Poisson on 216^3, 2x2x2 subdomains, overlap 2, ILU(0) Schwarz, GenEO coarse
space with nev = 20, additive, CG to 1e-10).  Right-hand sides: column 0 is the problem's, the others are seeded random consistent
vectors.  The M columns are solved (a) by TwoLevelSchwarz.solve_many through w slots and (b) by solve_multi in chunks of w, once as
they are ("even": every column needs about the same number of iterations) and once with every third right-hand side scaled by 2^-83
("mixed": such a column runs the same recurrence exactly scaled and stops on the absolute test def < 1e-30, well before the others
reach 1e-10 def0.  A warm start does not give columns that finish early: the stop test is relative to the column's own def0 and CG
needs as many iterations from a converged X0 as from zero, tests/test_gpu_queue.py).  Prints one
JSON line: per run the wall time, RHS-iterations per second, the number of block iterations and the fraction of slot-iterations that ran
frozen (a slot-iteration: one slot of the block through one block iteration; frozen: the slot held no running column, either done and
waiting for the slowest column of its chunk, or never filled).  The block iterations of the queued run are not reported by the
library: they are the refill protocol replayed on the columns' iteration counts (schedule()).

    python tools/many_rhs_bench.py [--grid 216] [--ncols 24] [--width 8] [--coarse geneo|pou] [--out profiles/many_rhs_bench.json]

With --solver bicgstabsolver the queue is the BiCGSTAB one (ddm_bicgstab_solve_queue) and the problem is the non-symmetric one of
--problem dg (BASELINE configs[3], the bench_convdiff.py setup: Q1-DG convection-diffusion on --cells^2 cells, 4 x 2 subdomains,
overlap 2, `umfpack`-type local solves, GenEO on the symmetric part, additive).  The M seeded random columns are solved (a) queued
through w slots, (b) by M consecutive single-vector BiCGSTAB solves (ddm_bicgstab_solve) and (c) by solve_multi(solver=
"restartedgmressolver") in chunks of w, --repeat times each, alternating.  Per variant: seconds per column, column-half-steps (or
column-iterations) per second, and the device memory of its work blocks computed from the shapes; for the queue also the share of
slot-half-steps that sat frozen (1 - sum of half steps / (2 w block iterations), the block iterations replayed by schedule()).

    python tools/many_rhs_bench.py --solver bicgstabsolver --problem dg --cells 512 --ncols 24 --width 8 --reduction 1e-8 [--out ...]
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


def log(*a):
    print("[many_rhs_bench]", *a, file=sys.stderr, flush=True)


def schedule(its, w):
    """block iterations of the queued loop for columns needing its[j] iterations each, in queue order through w slots: a column with 0
    iterations never holds a slot, freed slots take the queue head at the iteration boundary"""
    slots, nxt, blocks = [], 0, 0
    while True:
        while len(slots) < w and nxt < len(its):
            if its[nxt] > 0:
                slots.append(its[nxt])
            nxt += 1
        if not slots:
            return blocks
        blocks += 1
        slots = [r - 1 for r in slots if r > 1]


def summary(its, seconds, blocks, w):
    total = int(sum(its))
    return {"iterations": [int(i) for i in its], "seconds": seconds, "rhs_iterations_per_s": total / seconds, "block_iterations": int(blocks),
            "ms_per_block_iteration": 1e3 * seconds / max(blocks, 1), "frozen_fraction": 1.0 - total / max(blocks * w, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=216)
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--overlap", type=int, default=2)
    ap.add_argument("--coarse", default="geneo", choices=["geneo", "pou"])
    ap.add_argument("--nev", type=int, default=20)
    ap.add_argument("--ncols", type=int, default=24, help="right-hand sides M")
    ap.add_argument("--width", type=int, default=8, help="block width w (<= 32)")
    ap.add_argument("--reduction", type=float, default=1e-10)
    ap.add_argument("--maxit", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--solver", default="cgsolver", choices=["cgsolver", "bicgstabsolver"])
    ap.add_argument("--problem", default="poisson", choices=["poisson", "dg"], help="dg: BASELINE configs[3] (with --solver bicgstabsolver)")
    ap.add_argument("--cells", type=int, default=512, help="--problem dg: cells per direction")
    ap.add_argument("--local-solver", default="umfpack", choices=["umfpack", "ilu0"], help="--problem dg")
    ap.add_argument("--restart", type=int, default=100, help="--solver bicgstabsolver: restart of the block GMRES it is compared with")
    ap.add_argument("--repeat", type=int, default=3, help="--solver bicgstabsolver: timed repetitions of every variant")
    args = ap.parse_args()
    M, w = args.ncols, args.width
    assert M >= 1 and 1 <= w <= 32
    if (args.solver == "bicgstabsolver") != (args.problem == "dg"):
        ap.error("--solver bicgstabsolver goes with --problem dg (and cgsolver with poisson)")
    if args.solver == "bicgstabsolver":
        return main_bicgstab(args)

    import __graft_entry__ as ge
    ge.import_package()
    import torch
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz

    t0 = time.perf_counter()
    G, P = args.grid, args.parts
    dec = build_structured(synth.StructuredPoisson((G, G, G), (P, P, P)), overlap=args.overlap, pou_type="distance", shrink=0,
                           neumann=(args.coarse == "geneo"))
    if args.coarse == "geneo":
        from dune_ddm_amd.geneo import geneo_basis
        tl = TwoLevelSchwarz(dec, schwarz_type="standard", mode="additive", coarse="none")
        tl.set_coarse_basis(geneo_basis(tl, nev=args.nev))
        tl.rebuild_combined("additive")
    else:
        tl = TwoLevelSchwarz(dec, schwarz_type="standard", mode="additive", coarse="pou")
    tl.schwarz.wait_setup()
    tl.ctx.sync()
    log(f"setup {time.perf_counter() - t0:.1f} s, n_o = {tl.rl.n_o}, local engine {tl.schwarz.engine()}")

    rng = np.random.default_rng(args.seed)
    cols = [np.asarray(tl.rl.b, dtype=np.float64)]
    for _ in range(M - 1):
        xg = rng.standard_normal(dec.nglobal)
        cols.append(tl.rl.cat_novlp([xg[sd.glob[:sd.n_o]] for sd in dec.subs]))
    Bd = tl.to_device(np.stack(cols, axis=1))
    del cols
    kw = dict(reduction=args.reduction, maxit=args.maxit, history=False)
    tl.solve_many(Bd[:, :w].contiguous(), width=w, reduction=args.reduction, maxit=3, history=False)   # warm-up (the block solves' graphs)

    def queued(B):
        res, _, _ = tl.solve_many(B, width=w, **kw)
        its = [r.iterations for r in res]
        return summary(its, float(res[0].elapsed_s), schedule(its, w), w), all(r.converged for r in res)

    def chunked(B):
        its, seconds, blocks, conv = [], 0.0, 0, True
        for c0 in range(0, M, w):
            c1 = min(c0 + w, M)
            res, _, _ = tl.solve_multi(B[:, c0:c1].contiguous(), **kw)
            its += [r.iterations for r in res]
            seconds += float(res[0].elapsed_s)
            blocks += max(r.iterations for r in res)
            conv = conv and all(r.converged for r in res)
        # (a ragged last chunk runs c1 - c0 < w columns wide: its missing slots count as frozen, as the queue's never-filled ones do)
        return summary(its, seconds, blocks, w), conv

    runs = {}
    for name in ("even", "mixed"):
        B = Bd
        if name == "mixed":
            B = Bd.clone()
            B[:, ::3] *= 2.0 ** -83
        q, qconv = queued(B)
        c, cconv = chunked(B)
        runs[name] = {"queued": q, "chunked": c, "converged": bool(qconv and cconv), "ratio": q["rhs_iterations_per_s"] / c["rhs_iterations_per_s"]}
        for tag, r in (("queued", q), ("chunked", c)):
            log(f"{name} {tag}: {sum(r['iterations'])} RHS-iterations in {r['seconds']:.2f} s = {r['rhs_iterations_per_s']:.0f} RHS-it/s, "
                f"{r['block_iterations']} block iterations ({r['ms_per_block_iteration']:.1f} ms each), frozen {100 * r['frozen_fraction']:.1f} %")
    out = {"workload": f"{G}^3 Q1 Poisson, {P ** 3} subdomains, overlap {args.overlap}, ILU(0) Schwarz + {args.coarse} coarse space, additive, CG to {args.reduction:g}",
           "n_o": int(tl.rl.n_o), "device": torch.cuda.get_device_name(0), "ncols": M, "width": w, "runs": runs,
           "what": "queued = solve_many (ddm_cg_solve_queue), chunked = solve_multi on w columns at a time; even: the columns as they are; mixed: every "
                   "third right-hand side scaled by 2^-83 (stops on def < 1e-30); rhs_iterations_per_s = sum of the columns' CG iterations / time inside the "
                   "solves; frozen_fraction = 1 - sum of iterations / (block iterations x w)"}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    tl.ctx.close()


def main_bicgstab(args):
    M, w = args.ncols, args.width
    import __graft_entry__ as ge
    ge.import_package()
    import torch
    from dune_ddm_amd import synth
    from dune_ddm_amd.geneo import geneo_basis
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz

    t0 = time.perf_counter()
    C = args.cells
    grid = synth.StructuredDG2D((C, C), (4, 2))
    dec = build_structured(grid, overlap=args.overlap, neumann=True)
    tl = TwoLevelSchwarz(dec, schwarz_type="standard", mode="additive", coarse="none", subdomain_solver=args.local_solver)
    tl.set_coarse_basis(geneo_basis(tl, nev=args.nev, tol=1e-5))
    tl.rebuild_combined("additive")
    tl.schwarz.wait_setup()
    tl.ctx.sync()
    n = int(tl.rl.n_o)
    log(f"setup {time.perf_counter() - t0:.1f} s, n_o = {n}, local engine {tl.schwarz.engine()}, K = {tl.K}")

    rng = np.random.default_rng(args.seed)
    free = tl.rl.cat_novlp([(sd.dirichlet_ovlp[:sd.n_o] == 0).astype(np.float64) for sd in dec.subs])
    cols = []
    for _ in range(M):
        xg = rng.standard_normal(dec.nglobal)
        cols.append(tl.rl.cat_novlp([xg[sd.glob[:sd.n_o]] for sd in dec.subs]) * free)
    Bh = np.stack(cols, axis=1)
    Bd = tl.to_device(Bh)
    del cols
    red, maxit, R = args.reduction, args.maxit, args.restart

    def queued():
        res, hist, _ = tl.solve_many(Bd, width=w, reduction=red, maxit=maxit, solver="bicgstabsolver")
        half = [int(np.sum(~np.isnan(hist[:, j]))) - 1 for j in range(M)]
        blocks = schedule([r.iterations for r in res], w)
        return {"seconds": float(res[0].elapsed_s), "half_steps": half, "block_iterations": int(blocks), "converged": all(r.converged for r in res),
                "frozen_fraction": 1.0 - sum(half) / max(2 * w * blocks, 1)}

    def singles():
        half, seconds, conv = [], 0.0, True
        for j in range(M):
            res, hist, _ = tl.solve(reduction=red, maxit=maxit, b=Bh[:, j], solver="bicgstabsolver")   # (uploads a copy: the driver overwrites b)
            half.append(len(hist) - 1)
            seconds += float(res.elapsed_s)
            conv = conv and bool(res.converged)
        return {"seconds": seconds, "half_steps": half, "converged": conv}

    def gmres_chunks():
        its, seconds, conv = [], 0.0, True
        for c0 in range(0, M, w):
            res, _, _ = tl.solve_multi(Bd[:, c0:min(c0 + w, M)].contiguous(), reduction=red, maxit=maxit, history=False, solver="restartedgmressolver", restart=R)
            its += [r.iterations for r in res]
            seconds += float(res[0].elapsed_s)
            conv = conv and all(r.converged for r in res)
        return {"seconds": seconds, "iterations": [int(i) for i in its], "converged": conv}

    variants = {"queued_bicgstab": queued, "single_bicgstab": singles, "chunked_gmres": gmres_chunks}
    tl.solve_many(Bd[:, :w].contiguous(), width=w, reduction=red, maxit=2, history=False, solver="bicgstabsolver")    # warm-up of every shape
    tl.solve(reduction=red, maxit=2, b=Bh[:, 0], solver="bicgstabsolver")
    tl.solve_multi(Bd[:, :w].contiguous(), reduction=red, maxit=2, history=False, solver="restartedgmressolver", restart=R)
    runs = {k: [] for k in variants}
    for _ in range(args.repeat):                       # alternating, so that a drift of the machine hits every variant alike
        for k, fn in variants.items():
            runs[k].append(fn())
    tl.prec.check_status()
    out_runs = {}
    for k, rr in runs.items():
        secs = sorted(r["seconds"] for r in rr)
        med = secs[len(secs) // 2]
        work = sum(rr[0].get("half_steps", rr[0].get("iterations")))
        e = {"seconds_all": [r["seconds"] for r in rr], "seconds_median": med, "seconds_per_column": med / M, "converged": all(r["converged"] for r in rr)}
        if "half_steps" in rr[0]:
            e["half_steps"] = rr[0]["half_steps"]
            e["column_half_steps_per_s"] = work / med
        else:
            e["iterations"] = rr[0]["iterations"]
            e["column_iterations_per_s"] = work / med
        if k == "queued_bicgstab":
            e["block_iterations"] = rr[0]["block_iterations"]
            e["frozen_fraction"] = rr[0]["frozen_fraction"]
        out_runs[k] = e
        log(f"{k}: median {med:.3f} s of {[round(x, 3) for x in e['seconds_all']]} = {1e3 * med / M:.1f} ms per column, work {work}")
    Rg = min(R, max(maxit, 1))
    mem = {"queued_bicgstab_bytes": 7 * n * w * 8, "single_bicgstab_bytes": 5 * n * 8, "chunked_gmres_bytes": (Rg + 2) * n * w * 8,
           "what": "work blocks from the shapes: 7 blocks of n x w (x, r, rt, p, v, y, t); 5 vectors beside the caller's x and b; (R + 2) blocks of n x w (basis, w)"}
    out = {"workload": f"Q1-DG convection-diffusion {C}x{C} cells = {grid.nglobal} DoF, 8 subdomains (4x2), overlap {args.overlap}, '{args.local_solver}' local "
                       f"solves, GenEO nev {args.nev}, additive, to {red:g}; GMRES restart {R}",
           "n_o": n, "device": torch.cuda.get_device_name(0), "ncols": M, "width": w, "repeat": args.repeat, "runs": out_runs, "memory": mem}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    tl.ctx.close()


if __name__ == "__main__":
    main()
