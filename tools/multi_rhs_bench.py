"""Several right-hand sides at once against sequential solves (ddm_cg_solve_multi vs. m calls of ddm_cg_solve).

Workload: the bench.py setup (BASELINE configs[2]: 3-D Q1 Poisson on 216^3, 2x2x2 subdomains, overlap 2, ILU(0) Schwarz, GenEO coarse
space with nev = 20, additive, CG to 1e-10).  Right-hand sides: column 0 is the problem's, the others are seeded random consistent
vectors.  For every m of --m the same m right-hand sides are solved (a) as one block by ddm_cg_solve_multi and (b) one after the other by
ddm_cg_solve (each column is solved once; the sequential time of m columns is the sum over the first m).  Prints one JSON line:
RHS-iterations per second of both, their ratio, ms per block iteration, the iteration counts, and the per-block breakdown of a
--profile-iters run with the library's event timers (ddm_timing_*).

    python tools/multi_rhs_bench.py [--grid 216] [--m 1,4,8,16] [--coarse geneo|pou] [--multi-engine levels|xcd]
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

TIMERS = ("Operator/apply", "Schwarz/get defect", "Schwarz/local solve", "Schwarz/add solution", "GalerkinPrec/apply", "CombinedPreconditioner/apply")


def log(*a):
    print("[multi_rhs_bench]", *a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=216)
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--overlap", type=int, default=2)
    ap.add_argument("--coarse", default="geneo", choices=["geneo", "pou"])
    ap.add_argument("--nev", type=int, default=20)
    ap.add_argument("--m", default="1,4,8,16", help="block widths, comma separated (each <= 32)")
    ap.add_argument("--reduction", type=float, default=1e-10)
    ap.add_argument("--maxit", type=int, default=1000)
    ap.add_argument("--profile-iters", type=int, default=20, help="iterations of the timer run per block width (0 = none)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--multi-engine", default="levels", choices=["levels", "xcd"], help="engine of the local solves of the block applies")
    args = ap.parse_args()
    ms_ = sorted({int(v) for v in args.m.split(",")})
    assert all(1 <= m <= 32 for m in ms_)

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
    tl.schwarz.set_multi_engine(args.multi_engine)
    tl.schwarz.wait_setup()
    tl.ctx.sync()
    log(f"setup {time.perf_counter() - t0:.1f} s, n_o = {tl.rl.n_o}, local engine {tl.schwarz.engine()}")

    mmax = max(ms_)
    rng = np.random.default_rng(args.seed)
    cols = [np.asarray(tl.rl.b, dtype=np.float64)]
    for _ in range(mmax - 1):
        xg = rng.standard_normal(dec.nglobal)
        cols.append(tl.rl.cat_novlp([xg[sd.glob[:sd.n_o]] for sd in dec.subs]))
    Bh = np.stack(cols, axis=1)
    Bd = tl.to_device(Bh)

    # (b) sequential single-vector solves, each column once
    tl.solve(reduction=args.reduction, maxit=5, history=False, b=Bh[:, 0])          # warm-up (graph capture)
    seq = []
    for c in range(mmax):
        res, _, _ = tl.solve(reduction=args.reduction, maxit=args.maxit, history=False, b=Bh[:, c])
        seq.append((int(res.iterations), float(res.elapsed_s), bool(res.converged)))
        log(f"single column {c}: {res.iterations} iterations, {res.elapsed_s * 1e3:.1f} ms")
    single_prof = None
    if args.profile_iters > 0:
        tl.ctx.timing(True)
        tl.ctx.timing_reset()
        tl.solve(reduction=0.0, maxit=args.profile_iters, history=False, b=Bh[:, 0])
        tl.ctx.timing(False)
        single_prof = {k: tl.ctx.timer(k)[0] / args.profile_iters for k in TIMERS}

    # (a) one block solve per width
    rows = []
    for m in ms_:
        B = Bd[:, :m].contiguous()
        prof = None
        if args.profile_iters > 0:   # (also the warm-up: the block solves' graphs are captured here)
            tl.ctx.timing(True)
            tl.ctx.timing_reset()
            tl.solve_multi(B, reduction=0.0, maxit=args.profile_iters, history=False)
            tl.ctx.timing(False)
            prof = {k: tl.ctx.timer(k)[0] / args.profile_iters for k in TIMERS}
        res, _, X = tl.solve_multi(B, reduction=args.reduction, maxit=args.maxit, history=False)
        its = [int(r.iterations) for r in res]
        el = float(res[0].elapsed_s)
        seq_its = [s[0] for s in seq[:m]]
        seq_el = sum(s[1] for s in seq[:m])
        row = {"m": m, "iterations": its, "sequential_iterations": seq_its, "converged": all(r.converged for r in res),
               "block_s": el, "sequential_s": seq_el, "ms_per_block_iteration": 1e3 * el / max(its),
               "rhs_iterations_per_s": sum(its) / el, "sequential_rhs_iterations_per_s": sum(seq_its) / seq_el,
               "ms_per_block_iteration_by_timer": prof}
        row["ratio"] = row["rhs_iterations_per_s"] / row["sequential_rhs_iterations_per_s"]
        rows.append(row)
        log(f"m = {m}: {max(its)} block iterations in {el:.3f} s ({row['ms_per_block_iteration']:.2f} ms each), "
            f"{row['rhs_iterations_per_s']:.0f} RHS-it/s against {row['sequential_rhs_iterations_per_s']:.0f} sequential: x{row['ratio']:.2f}")
        del X
    out = {"workload": f"{G}^3 Q1 Poisson, {P ** 3} subdomains, overlap {args.overlap}, ILU(0) Schwarz + {args.coarse} coarse space, additive, CG to {args.reduction:g}",
           "n_o": int(tl.rl.n_o), "multi_engine": args.multi_engine, "device": torch.cuda.get_device_name(0), "single_ms_per_iteration_by_timer": single_prof, "rows": rows,
           "what": "rhs_iterations_per_s = sum of the columns' CG iterations / wall time of the solve; sequential = the same columns solved one by one with "
                   "ddm_cg_solve; *_by_timer: ms per (block) iteration of a fixed-length run with the library's event timers on"}
    print(json.dumps(out))
    tl.ctx.close()


if __name__ == "__main__":
    main()
