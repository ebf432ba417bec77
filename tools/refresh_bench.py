"""Times TwoLevelSchwarz.update_values (new matrix values, everything symbolic and the coarse basis kept) against constructing the
object anew on the same values.

    python tools/refresh_bench.py [--workload poisson] [--grid 216] [--parts 2] [--overlap 2] [--coarse geneo|pou] [--nev 20]
    python tools/refresh_bench.py --workload dg [--cells 512] [--coarse pou|geneo]
    python tools/refresh_bench.py --workload elasticity [--refine 1] [--coarse pou|geneo]

poisson: the headline problem (216^3 nodes, 2 x 2 x 2 subdomains, overlap 2, ILU(0) local solves, GenEO basis kept), and the device
ILU(0) factorisation of the refresh against the host factorisation that DDM_PIPE_VERBOSE reports at creation.
dg / elasticity: the problems of bench_convdiff.py (configs[3]: Q1-DG convection-diffusion on 512^2 cells, `umfpack`; configs[4]:
P1 elasticity on the 80 x 8 x 12 bar, `cholmod`) with the DIRECT local solver on the device engine (DDM_DIRECT_ENGINE=device): the
local-solver phase of update_values -- the in-place refresh of the supernodal factor, split into numeric factorisation, chain
inverses and refinement probe as the library reports them -- against the same phase of a build that creates the level anew, and
against the local-solver share of a new object.

The new values are a changed coefficient: a_ij c_i c_j with one factor c in [0.7, 1.3] per global unknown (a congruence: symmetric
matrices stay symmetric positive definite, the DG operator keeps its positive definite symmetric part; consistent between the
additive matrix and the overlapping matrices).  Prints the phases and one JSON line; exits 1 when the refreshed object and the new
one disagree in iterations or in a bit of the solution."""
import argparse
import dataclasses
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def changed_coefficient(dec, seed):
    import numpy as np
    import scipy.sparse as sp
    c = np.random.default_rng(seed).uniform(0.7, 1.3, dec.nglobal)
    subs = []
    for sd in dec.subs:
        g = np.asarray(sd.glob, dtype=np.int64)
        out = {}
        for key in ("A", "A_dir"):
            M = sp.csr_matrix(getattr(sd, key))
            cg = c[g[:M.shape[0]]]
            rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
            out[key] = sp.csr_matrix((M.data * cg[rows] * cg[M.indices], M.indices, M.indptr), shape=M.shape)
        subs.append(dataclasses.replace(sd, **out))
    return dataclasses.replace(dec, subs=subs, meta=dict(dec.meta))


def sorted_data(M):
    import scipy.sparse as sp
    M = sp.csr_matrix(M)
    return (M if M.has_sorted_indices else M.sorted_indices()).data


class CaptureStderr:
    """the C library's stderr (file descriptor 2) into a temporary file"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        sys.stderr.write(self.text)


def problem(args):
    """(decomposition, keyword arguments of TwoLevelSchwarz, of tl.solve, GenEO settings) of the workload"""
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    geneo = args.coarse == "geneo"
    if args.workload == "poisson":
        G, P = args.grid, args.parts
        dec = build_structured(synth.StructuredPoisson((G, G, G), (P, P, P)), overlap=args.overlap, pou_type="distance", shrink=0, neumann=geneo)
        return dec, {}, dict(reduction=args.reduction, maxit=1000, history=False), dict(nev=args.nev)
    os.environ["DDM_DIRECT_ENGINE"] = "device"
    if args.workload == "dg":                                    # bench_convdiff.py --problem dg
        dec = build_structured(synth.StructuredDG2D((args.cells, args.cells), (4, 2)), overlap=2, neumann=geneo)
        return (dec, dict(schwarz_type="standard", mode="additive", subdomain_solver="umfpack"),
                dict(reduction=1e-8, maxit=1000, history=False, solver="restartedgmressolver", restart=100), dict(nev=16, tol=1e-5))
    dec = build_structured(synth.StructuredElasticity(refine=args.refine, parts=8), overlap=1, neumann=geneo, second_region="all")   # --problem elasticity
    return (dec, dict(schwarz_type="restricted", mode="multiplicative", subdomain_solver="cholmod"),
            dict(reduction=1e-6, maxit=1000, history=False, solver="restartedgmressolver", restart=100), dict(nev=12, tol=1e-6))


LOCAL_KEYS = ("local solver (device factorisation, scatter)", "local solver (created anew)")
SN_LINE = re.compile(r"device supernodal (?:L U|Cholesky) refresh: numeric factorisation ([0-9.]+) s \(chain inverses ([0-9.]+) s of it\), probe ([0-9.]+) s: (\d+) refinement")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="poisson", choices=["poisson", "dg", "elasticity"])
    ap.add_argument("--grid", type=int, default=216)
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--overlap", type=int, default=2)
    ap.add_argument("--cells", type=int, default=512)
    ap.add_argument("--refine", type=int, default=1)
    ap.add_argument("--coarse", default=None, choices=["geneo", "pou"], help="default: geneo for poisson, pou for the direct workloads (the basis is kept either way)")
    ap.add_argument("--nev", type=int, default=20)
    ap.add_argument("--reduction", type=float, default=1e-10)
    args = ap.parse_args()
    direct = args.workload != "poisson"
    if args.coarse is None:
        args.coarse = "pou" if direct else "geneo"
    import numpy as np
    import __graft_entry__ as ge
    ge.import_package()
    from dune_ddm_amd.problem import RankLocal
    from dune_ddm_amd.solver import TwoLevelSchwarz
    os.environ["DDM_PIPE_VERBOSE"] = "1"

    dec, tl_kw, solve_kw, geneo_kw = problem(args)
    t0 = time.perf_counter()
    if args.coarse == "geneo":
        from dune_ddm_amd.geneo import geneo_basis
        tl = TwoLevelSchwarz(dec, coarse="none", **tl_kw)
        tl.set_coarse_basis(geneo_basis(tl, **geneo_kw))
        tl.rebuild_combined(tl_kw.get("mode", "additive"))
    else:
        tl = TwoLevelSchwarz(dec, coarse="pou", **tl_kw)
    tl.schwarz.wait_setup()
    tl.ctx.sync()
    t_first = time.perf_counter() - t0
    res0, _, _ = tl.solve(**solve_kw)
    print(f"first object: {t_first:.2f} s of device setup (coarse space '{args.coarse}' included), engine {tl.schwarz.engine()}, {res0.iterations} iterations, "
          f"{res0.elapsed_s:.3f} s", flush=True)

    dec2 = changed_coefficient(dec, 5)
    rl2 = RankLocal(dec2)
    va, vd = sorted_data(rl2.A).copy(), sorted_data(rl2.A_dir).copy()
    del rl2

    schwarz_before = tl.schwarz
    tl.ctx.timing(True)
    tl.ctx.timing_reset()
    with CaptureStderr() as cap_refresh:
        t0 = time.perf_counter()
        tl.update_values(va, vd)
        tl.ctx.sync()
        t_refresh = time.perf_counter() - t0
    timers = {name: tl.ctx.timer(name)[0] * 1e-3 for name in ("Refresh/factor", "Refresh/scatter", "Refresh/sn factor", "Refresh/sn probe")}
    tl.ctx.timing(False)
    phases = {k[len("refresh: "):]: v for k, v in tl.setup_times.items() if k.startswith("refresh: ")}
    local_key = next((k for k in LOCAL_KEYS if k in phases), None)
    count = getattr(tl.schwarz, "refresh_count", lambda: None)()        # (None: a build without the counter)
    in_place = tl.schwarz is schwarz_before
    res1, _, x1 = tl.solve(**solve_kw)
    print(f"update_values: {t_refresh:.3f} s; phases (s): " + ", ".join(f"{k} {v:.4f}" for k, v in phases.items()), flush=True)
    sn = None
    if direct:
        m = SN_LINE.search(cap_refresh.text)
        if m:
            sn = {"numeric_factorisation_s": float(m.group(1)), "chain_inverses_s": float(m.group(2)), "probe_s": float(m.group(3)), "refinement_steps": int(m.group(4))}
        print(f"  local solver: '{local_key}' {phases.get(local_key, float('nan')):.4f} s, the same object: {in_place}, in-place refreshes counted: {count}; "
              f"engine {tl.schwarz.engine()}; split reported by the library: {sn}; solve: {res1.iterations} iterations, {res1.elapsed_s:.3f} s", flush=True)
    else:
        print(f"  device ILU(0) factorisation {timers['Refresh/factor']:.3f} s, scatter into the engines {timers['Refresh/scatter']:.3f} s; solve: {res1.iterations} iterations, "
              f"{res1.elapsed_s:.3f} s", flush=True)

    basis = tl.host_basis()
    with CaptureStderr() as cap:
        t0 = time.perf_counter()
        new = TwoLevelSchwarz(dec2, coarse=basis, **tl_kw)
        new.schwarz.wait_setup()
        new.ctx.sync()
        t_new = time.perf_counter() - t0
    m = re.search(r"factorisation \(host, one thread per block\) ([0-9.]+) s", cap.text)
    host_factor_s = float(m.group(1)) if m else None
    res2, _, x2 = new.solve(**solve_kw)
    same = bool(res1.iterations == res2.iterations and (x1 == x2).all().item())
    print(f"new object on the same values (basis handed over): {t_new:.2f} s; phases (s): " + ", ".join(f"{k} {v:.2f}" for k, v in new.setup_times.items()), flush=True)
    print(f"  host ILU(0) factorisation at creation {host_factor_s} s; solve: {res2.iterations} iterations; refreshed and new object agree bit for bit: {same}", flush=True)
    print(json.dumps({"workload": args.workload, "grid": args.grid if not direct else None, "parts": args.parts if not direct else None,
                      "cells": args.cells if args.workload == "dg" else None, "refine": args.refine if args.workload == "elasticity" else None,
                      "coarse": args.coarse, "engine": tl.schwarz.engine(), "refresh_s": t_refresh, "refresh_phases_s": phases,
                      "local_solver_phase": local_key, "local_solver_phase_s": phases.get(local_key), "local_solver_in_place": in_place, "refresh_count": count,
                      "supernodal_refresh_split_s": sn, "device_timers_s": timers,
                      "device_factorisation_s": timers["Refresh/factor"], "device_scatter_s": timers["Refresh/scatter"], "reconstruction_s": t_new,
                      "reconstruction_phases_s": new.setup_times, "host_factorisation_s": host_factor_s,
                      "iterations": [int(res0.iterations), int(res1.iterations), int(res2.iterations)], "bit_identical": same}), flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
