"""The block solve of the ILU(0) local solver on its two engines: `levels` (one launch per dependency level and sweep) against `xcd`
(one persistent launch, csrc/engine_multi_xcd.hpp), in ONE process, alternating.

Workloads: the bench.py setup (3-D Q1 Poisson on 216^3, 2x2x2 subdomains, overlap 2: the block-diagonal ILU(0) factor of the 8
overlapping subdomain matrices) and the Q1-DG problem of bench_convdiff.py (512 x 512 cells, 4x2 subdomains, overlap 2) with the ILU(0)
local solver.  Timed: ddm_ilu0_solve_multi at m = 8 and 32 (double sweeps) and ddm_ilu0_solve_multi_f32 at m = 24, between two HIP
events on the library's stream, after a warm-up (the graph capture and --warmup replays), --reps times per engine with the engine
switched after every solve; reported are the median and the spread (min, max) in ms and whether the two engines' results are
bit-identical.  With --block-iteration: one CG block solve at m = 8 (pou coarse space, 30 iterations) per engine, ms per block
iteration.  With --geneo (216^3 only): the wall time of geneo_basis (nev = 20, ILU(0) preconditioner) with DDM_TRSV_MULTI_MODE unset and
set to xcd, and whether the two bases are bit-identical.  Prints one JSON line.

    python tools/multi_trsv_bench.py [--workload poisson216|dg512] [--grid 216] [--cells 512] [--reps 21] [--block-iteration] [--geneo]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ((8, False), (32, False), (24, True))   # (m, single precision)


def log(*a):
    print("[multi_trsv_bench]", *a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="poisson216", choices=["poisson216", "dg512"])
    ap.add_argument("--grid", type=int, default=216)
    ap.add_argument("--cells", type=int, default=512)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-iteration", action="store_true")
    ap.add_argument("--geneo", action="store_true")
    args = ap.parse_args()
    assert args.reps >= 20

    import __graft_entry__ as ge
    ddm = ge.import_package()
    import torch
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz

    os.environ.pop("DDM_TRSV_MULTI_MODE", None)
    t0 = time.perf_counter()
    if args.workload == "poisson216":
        G = args.grid
        dec = build_structured(synth.StructuredPoisson((G, G, G), (2, 2, 2)), overlap=2, pou_type="distance", shrink=0, neumann=args.geneo)
        workload = f"{G}^3 Q1 Poisson, 8 subdomains, overlap 2, ILU(0)"
        tl = TwoLevelSchwarz(dec, schwarz_type="standard", mode="additive", coarse="pou")
    else:
        C = args.cells
        dec = build_structured(synth.StructuredDG2D((C, C), (4, 2)), overlap=2, neumann=False)
        workload = f"Q1-DG convection-diffusion {C}x{C} cells, 8 subdomains (4x2), overlap 2, ILU(0)"
        tl = TwoLevelSchwarz(dec, schwarz_type="standard", mode="additive", coarse="pou", subdomain_solver="ilu0")
    tl.schwarz.wait_setup()
    ctx, lib = tl.ctx, tl.ctx.lib
    F = ctypes.c_void_p(tl.schwarz.local_solver())
    n = int(tl.rl.n)
    nlev = tl.schwarz.num_levels()
    log(f"setup {time.perf_counter() - t0:.1f} s: {workload}, {n} overlapping rows, levels {nlev}")

    def info():
        ctx.sync()
        out = np.zeros(14, dtype=np.int64)
        cnt = ctypes.c_int64()
        ctx.check(lib.ddm_ilu0_multi_info(F, out.ctypes.data_as(ctypes.c_void_p), 14, ctypes.byref(cnt)))
        return out

    rng = np.random.default_rng(5)
    rows = []
    for m, f32 in CONFIGS:
        D = torch.tensor(rng.standard_normal((n, m))).cuda()
        X = {e: torch.full_like(D, float("nan")) for e in (0, 1)}
        fn = lib.ddm_ilu0_solve_multi_f32 if f32 else lib.ddm_ilu0_solve_multi

        def solve(e):
            ctx.check(lib.ddm_ilu0_set_multi_engine(ctx.h, F, e))
            ctx.check(fn(ctx.h, F, m, ctypes.c_void_p(D.data_ptr()), ctypes.c_void_p(X[e].data_ptr())))
        ran = {}
        for e in (0, 1):                       # warm-up: capture, replays
            for _ in range(1 + args.warmup):
                solve(e)
            ran[e] = int(info()[1])
        ms = {0: [], 1: []}
        for _ in range(args.reps):             # alternating: every solve is a new capture, as after any engine switch ...
            for e in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ctx.check(lib.ddm_ilu0_set_multi_engine(ctx.h, F, e))
                ctx.check(fn(ctx.h, F, m, ctypes.c_void_p(D.data_ptr()), ctypes.c_void_p(X[e].data_ptr())))   # (capture, not timed)
                ctx.sync()
                e0.record()
                ctx.check(fn(ctx.h, F, m, ctypes.c_void_p(D.data_ptr()), ctypes.c_void_p(X[e].data_ptr())))   # ... so the REPLAY is timed
                e1.record()
                ctx.sync()
                ms[e].append(e0.elapsed_time(e1))
        st = ctypes.c_int()
        ctx.check(lib.ddm_ilu0_status(ctx.h, F, ctypes.byref(st)))
        row = {"m": m, "f32": f32, "engine_ran": {"levels": ran[0], "xcd": ran[1]}, "status": st.value, "bit_identical": bool(torch.equal(X[0], X[1])),
               "finite": bool(torch.isfinite(X[1]).all())}
        for e, name in ((0, "levels"), (1, "xcd")):
            a = np.asarray(ms[e])
            row[name + "_ms"] = {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()), "reps": int(a.size)}
        row["xcd_over_levels"] = row["xcd_ms"]["median"] / row["levels_ms"]["median"]
        rows.append(row)
        log(f"m = {m}{' f32' if f32 else ''}: levels {row['levels_ms']['median']:.3f} ms ({row['levels_ms']['min']:.3f}..{row['levels_ms']['max']:.3f}), "
            f"xcd {row['xcd_ms']['median']:.3f} ms ({row['xcd_ms']['min']:.3f}..{row['xcd_ms']['max']:.3f}), bit-identical {row['bit_identical']}")
        del D, X
    out = {"workload": workload, "rows_overlapping": n, "levels": list(nlev), "device": torch.cuda.get_device_name(0), "multi_info_xcd": [int(v) for v in info()],
           "block_solve": rows,
           "what": "ms of one replayed block solve X = (LU)^-1 D between HIP events on the library's stream, engines alternating in one process; "
                   "median (min, max) over reps"}

    if args.block_iteration:
        m = 8
        cols = [np.asarray(tl.rl.b, dtype=np.float64)]
        for _ in range(m - 1):
            xg = rng.standard_normal(dec.nglobal)
            cols.append(tl.rl.cat_novlp([xg[sd.glob[:sd.n_o]] for sd in dec.subs]))
        B = tl.to_device(np.stack(cols, axis=1))
        solver = "cgsolver" if args.workload == "poisson216" else "restartedgmressolver"
        it = {}
        for name in ("levels", "xcd", "levels", "xcd"):
            tl.schwarz.set_multi_engine(name)
            tl.solve_multi(B, reduction=0.0, maxit=3, history=False, solver=solver, restart=30)          # warm-up: capture
            res, _, X = tl.solve_multi(B, reduction=0.0, maxit=30, history=False, solver=solver, restart=30)
            it.setdefault(name, []).append(1e3 * float(res[0].elapsed_s) / 30)
            del X
        tl.prec.check_status()
        out["block_iteration_m8"] = {"solver": solver, "coarse": "pou", "iterations": 30, "ms_per_block_iteration": it}
        log(f"block iteration (m = 8, {solver}, pou): {it}")
    tl.ctx.close()
    del tl

    if args.geneo and args.workload == "poisson216":
        from dune_ddm_amd.geneo import geneo_basis
        g = {}
        bases = {}
        for mode in ("levels", "xcd"):
            os.environ["DDM_TRSV_MULTI_MODE"] = mode
            t2 = TwoLevelSchwarz(dec, schwarz_type="standard", mode="additive", coarse="none")
            t2.ctx.sync()
            t1 = time.perf_counter()
            basis, gi = geneo_basis(t2, nev=20, return_info=True, preconditioner="ilu0")
            t2.ctx.sync()
            g[mode] = {"wall_s": time.perf_counter() - t1, "iterations": gi["iterations"], "converged": bool(gi["converged"]),
                       "setup_s": gi.get("setup_s"), "iterate_s": gi.get("iterate_s")}
            bases[mode] = basis
            t2.ctx.close()
            log(f"geneo_basis with DDM_TRSV_MULTI_MODE={mode}: {g[mode]}")
        os.environ.pop("DDM_TRSV_MULTI_MODE", None)
        g["bit_identical"] = all(np.array_equal(np.asarray(bases["levels"][s]), np.asarray(bases["xcd"][s])) for s in bases["levels"])
        out["geneo_basis_nev20_ilu0"] = g
    print(json.dumps(out))


if __name__ == "__main__":
    main()
