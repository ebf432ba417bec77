"""Times the kept GenEO eigensolver (GeneoSolver: update + compute("kept")) against geneo_basis anew on the same new values, and counts
what either basis, and the stale one, cost the outer CG.

    python tools/geneo_refresh_bench.py [--grid 216] [--parts 2] [--overlap 2] [--nev 20] [--repeat 3] [--spreads 0.3,0.05]
    python tools/geneo_refresh_bench.py --cold-only        # geneo_basis on the new values only: runs on a commit without GeneoSolver

The headline problem (216^3 nodes, 2 x 2 x 2 subdomains, overlap 2, nev 20).  The coefficient is changed per cell by a factor in
[1 - s, 1 + s] for every spread s (default 0.3 and 0.05); the patterns stay.  Per spread, --repeat times, taken in turn:
  (i)  geneo_basis anew on the new values (inputs, pencil, preconditioner, iteration, download): seconds, block iterations;
  (ii) GeneoSolver.update (values, pencil and preconditioner refreshed on the device) + compute("kept"): seconds, block iterations --
       the solver is put back to the old values and a cold compute before every repetition, so that each starts from the same block;
then one outer CG solve on the new matrices with the basis of (i), of (ii) and with the stale basis of the old values.
--cold-only does (i) alone, for the comparison of the cold path with the commit it replaces.  Prints one JSON line per spread with
medians and ranges."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sorted_data(M):
    import scipy.sparse as sp
    M = sp.csr_matrix(M)
    return (M if M.has_sorted_indices else M.sorted_indices()).data


def med(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=216)
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--overlap", type=int, default=2)
    ap.add_argument("--nev", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--spreads", default="0.3,0.05")
    ap.add_argument("--reduction", type=float, default=1e-10)
    ap.add_argument("--cold-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import __graft_entry__ as ge
    ge.import_package()
    from dune_ddm_amd import synth
    from dune_ddm_amd.geneo import geneo_basis
    from dune_ddm_amd.problem import RankLocal, build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz
    G, P = args.grid, args.parts

    def decomposition(kappa):
        t0 = time.perf_counter()
        dec = build_structured(synth.StructuredPoisson((G, G, G), (P, P, P), kappa), overlap=args.overlap, pou_type="distance", shrink=0, neumann=True)
        print(f"decomposition: {time.perf_counter() - t0:.1f} s", flush=True)
        return dec
    ones = np.ones((G - 1, G - 1, G - 1))
    dec_old = None
    for spread in (float(s) for s in args.spreads.split(",")):
        kappa = ones * np.random.default_rng(7).uniform(1.0 - spread, 1.0 + spread, ones.shape)
        dec_new = decomposition(kappa)
        tl_new = TwoLevelSchwarz(dec_new, coarse="none")
        tl_new.schwarz.wait_setup()
        cold_s, cold_it = [], []
        basis_cold = None
        if args.cold_only:
            for _ in range(args.repeat):
                tl_new.ctx.sync()
                t0 = time.perf_counter()
                basis_cold, info = geneo_basis(tl_new, nev=args.nev, return_info=True)
                cold_s.append(time.perf_counter() - t0)
                cold_it.append(info["iterations"])
                print(f"spread {spread}: geneo_basis anew {cold_s[-1]:.2f} s, {cold_it[-1]} block iterations (direct {info['used_direct']})", flush=True)
            print(json.dumps({"grid": G, "parts": P, "nev": args.nev, "spread": spread, "cold_only": True, "cold_s": med(cold_s), "cold_block_iterations": med(cold_it)}), flush=True)
            tl_new.ctx.close()
            continue
        from dune_ddm_amd.geneo import GeneoSolver
        if dec_old is None:
            dec_old = decomposition(ones)
        tl = TwoLevelSchwarz(dec_old, coarse="none")
        tl.schwarz.wait_setup()
        old_vals = ({sd.id: sorted_data(sd.A_neu) for sd in dec_old.subs}, {sd.id: sorted_data(sd.B_neu) for sd in dec_old.subs})
        new_vals = ({sd.id: sorted_data(sd.A_neu) for sd in dec_new.subs}, {sd.id: sorted_data(sd.B_neu) for sd in dec_new.subs})
        b_is_a = all(sd.B_neu is sd.A_neu for sd in dec_old.subs)
        import torch

        def used():
            tl.ctx.sync()
            free, total = torch.cuda.mem_get_info()
            return total - free
        held = [used()]
        t0 = time.perf_counter()
        S = GeneoSolver(tl, nev=args.nev)
        t_create = time.perf_counter() - t0
        held.append(used())
        basis_old, info_old = S.compute("random", return_info=True)
        held.append(used())
        print(f"spread {spread}: kept eigensolver created in {t_create:.2f} s, first compute {info_old['iterations']} block iterations (direct {info_old['used_direct']}); "
              f"device memory held: {(held[1] - held[0]) / 1e9:.2f} GB after create, {(held[2] - held[0]) / 1e9:.2f} GB after the first compute", flush=True)
        upd_s, warm_s, warm_it = [], [], []
        basis_warm = None
        for r in range(args.repeat):
            tl_new.ctx.sync()
            t0 = time.perf_counter()
            basis_cold, info = geneo_basis(tl_new, nev=args.nev, return_info=True)
            cold_s.append(time.perf_counter() - t0)
            cold_it.append(info["iterations"])
            if r:                                                   # back to the state before the first update
                S.update(old_vals[0], None if b_is_a else old_vals[1])
                S.compute("random")
            tl.ctx.sync()
            t0 = time.perf_counter()
            S.update(new_vals[0], None if b_is_a else new_vals[1])
            t1 = time.perf_counter()
            basis_warm, winfo = S.compute("kept", return_info=True)
            t2 = time.perf_counter()
            upd_s.append(t1 - t0)
            warm_s.append(t2 - t0)
            warm_it.append(winfo["iterations"])
            held.append(used())
            print(f"spread {spread}: device memory held after the update and the warm compute: {(held[-1] - held[0]) / 1e9:.2f} GB", flush=True)
            print(f"spread {spread}: geneo_basis anew {cold_s[-1]:.2f} s, {cold_it[-1]} block iterations; update {upd_s[-1]:.2f} s + compute(kept) {t2 - t1:.2f} s = "
                  f"{warm_s[-1]:.2f} s, {warm_it[-1]} block iterations; state {S.state()}", flush=True)
        S.close()
        tl.ctx.close()
        del tl, S
        cg = {}
        b = np.asarray(RankLocal(dec_new, 0, 1).b, dtype=np.float64)
        for name, basis in (("new", basis_cold), ("kept", basis_warm), ("stale", basis_old)):
            tl_new.set_coarse_basis(basis)
            tl_new.rebuild_combined("additive")
            res, _, _ = tl_new.solve(reduction=args.reduction, maxit=1000, history=False, b=b)
            cg[name] = int(res.iterations) if res.converged else None
            print(f"spread {spread}: outer CG with the {name} basis: {cg[name]} iterations, {res.elapsed_s:.3f} s", flush=True)
        print(json.dumps({"grid": G, "parts": P, "overlap": args.overlap, "nev": args.nev, "spread": spread, "create_s": t_create, "held_gb": [(h - held[0]) / 1e9 for h in held[1:]], "cold_s": med(cold_s),
                          "cold_block_iterations": med(cold_it), "update_s": med(upd_s), "update_plus_warm_s": med(warm_s), "warm_block_iterations": med(warm_it),
                          "cg_iterations": cg}), flush=True)
        tl_new.ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
