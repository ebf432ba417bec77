"""Block CG against independent CG recurrences on the same block (ddm_bcg_solve_multi vs. ddm_cg_solve_multi).

Workload: the bench.py setup (3-D Q1 Poisson on 216^3, 2x2x2 subdomains, overlap 2, ILU(0) standard Schwarz, GenEO coarse space with
nev = 20, additive, reduction 1e-10).  Right-hand sides: column 0 is the problem's, the others are seeded random consistent vectors.
For every width of --m the same block is solved --runs times by solve_block and by solve_multi in turn, in one process.  Per run: block
iterations, per-column iterations, ms per block iteration, time to solution and the worst recomputed true reduction; for block CG also
the shares of its three kernels per iteration from one more run with the library's event timers on (ddm_timing_*), with the bytes
each pass has to move (Gram 24 m n per product pair, update 40 m n, direction 24 m n) over its time.  Prints one JSON line.

    python tools/block_cg_bench.py [--grid 216] [--m 8,32] [--coarse geneo|pou] [--runs 3]
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

TIMERS = ("BCG/gram", "BCG/update", "BCG/direction", "Operator/apply", "Schwarz/local solve", "CombinedPreconditioner/apply")


def log(*a):
    print("[block_cg_bench]", *a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=216)
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--overlap", type=int, default=2)
    ap.add_argument("--coarse", default="geneo", choices=["geneo", "pou"])
    ap.add_argument("--nev", type=int, default=20)
    ap.add_argument("--m", default="8,32", help="block widths, comma separated (each <= 32)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reduction", type=float, default=1e-10)
    ap.add_argument("--maxit", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    widths = sorted({int(v) for v in args.m.split(",")})
    assert all(1 <= m <= 32 for m in widths) and args.runs >= 1

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

    rows = []
    for m in widths:
        B = Bd[:, :m].contiguous()
        tl.solve_block(B, reduction=args.reduction, maxit=3, history=False)           # warm-up of both drivers (graph capture, scratch)
        tl.solve_multi(B, reduction=args.reduction, maxit=3, history=False)
        runs = {"block": [], "multi": []}
        for r in range(args.runs):
            for name in ("block", "multi"):
                if name == "block":
                    res, _, X, ranks = tl.solve_block(B, reduction=args.reduction, maxit=args.maxit, history=False)
                    k_end = len(ranks)
                else:
                    res, _, X = tl.solve_multi(B, reduction=args.reduction, maxit=args.maxit, history=False)
                    k_end = max(int(x.iterations) for x in res)
                el = float(res[0].elapsed_s)
                run = {"block_iterations": k_end, "iterations": [int(x.iterations) for x in res], "converged": all(x.converged for x in res),
                       "seconds": el, "ms_per_block_iteration": 1e3 * el / max(k_end, 1), "worst_true_reduction": true_reduction(B, X)}
                if name == "block":
                    run["min_rank"] = int(ranks.min()) if k_end else 0
                runs[name].append(run)
                log(f"m = {m} run {r} {name}: {k_end} block iterations, {el:.3f} s ({run['ms_per_block_iteration']:.2f} ms each), "
                    f"worst true reduction {run['worst_true_reduction']:.2e}")
                del X
        tl.ctx.timing(True)
        tl.ctx.timing_reset()
        res, _, X, ranks = tl.solve_block(B, reduction=args.reduction, maxit=args.maxit, history=False)
        tl.ctx.timing(False)
        k = max(len(ranks), 1)
        prof = {key: tl.ctx.timer(key)[0] / k for key in TIMERS}
        calls = {key: tl.ctx.timer(key)[1] for key in ("BCG/gram", "BCG/update", "BCG/direction")}
        # per pass: the two-product Gram reads 3 blocks, the one-product Gram 2 (both under BCG/gram: 5 blocks per iteration)
        bytes_per_iteration = {"BCG/gram": 40 * m * n, "BCG/update": 40 * m * n, "BCG/direction": 24 * m * n}
        gbs = {key: bytes_per_iteration[key] / (prof[key] * 1e-3) / 1e9 for key in bytes_per_iteration if prof[key] > 0}
        del X
        best = {name: min(x["seconds"] for x in runs[name]) for name in runs}
        rows.append({"m": m, "runs": runs, "best_seconds": best, "winner_time_to_solution": min(best, key=best.get),
                     "block_cg_ms_per_iteration_by_timer": prof, "block_cg_timer_calls": calls, "block_cg_kernel_GB_per_s": gbs})
        log(f"m = {m}: best block CG {best['block']:.3f} s, best independent CG {best['multi']:.3f} s; kernels per iteration {prof}; GB/s {gbs}")
    out = {"workload": f"{G}^3 Q1 Poisson, {P ** 3} subdomains, overlap {args.overlap}, ILU(0) standard Schwarz + {args.coarse} coarse space, additive, reduction {args.reduction:g}",
           "n_o": n, "device": torch.cuda.get_device_name(0), "rows": rows,
           "what": "block = ddm_bcg_solve_multi (solve_block), multi = ddm_cg_solve_multi (solve_multi) on the same block, in turn; seconds = wall time of the "
                   "loop; *_by_timer: ms per block iteration of one more block CG run with the event timers on (BCG/gram covers both Gram passes of an "
                   "iteration: 40 m n bytes); GB/s = the bytes the pass must move / its time"}
    print(json.dumps(out))
    tl.ctx.close()


if __name__ == "__main__":
    main()
