"""Times TwoLevelSchwarz.update_values (new matrix values, everything symbolic and the coarse basis kept) against constructing the
object anew on the same values, on the headline problem (216^3 nodes, 2 x 2 x 2 subdomains, overlap 2, GenEO basis kept), and the
device ILU(0) factorisation of the refresh against the host factorisation that DDM_PIPE_VERBOSE reports at creation.

    python tools/refresh_bench.py [--grid 216] [--parts 2] [--overlap 2] [--coarse geneo|pou] [--nev 20]

The new values are a changed coefficient: a_ij c_i c_j with one factor c in [0.7, 1.3] per global unknown (symmetric, positive
definite, consistent between the additive matrix and the overlapping matrices).  Prints the phases and one JSON line; exits 1 when
the refreshed object and the new one disagree in iterations or in a bit of the solution."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=216)
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--overlap", type=int, default=2)
    ap.add_argument("--coarse", default="geneo", choices=["geneo", "pou"])
    ap.add_argument("--nev", type=int, default=20)
    ap.add_argument("--reduction", type=float, default=1e-10)
    args = ap.parse_args()
    import numpy as np
    import __graft_entry__ as ge
    ge.import_package()
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import RankLocal, build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz
    os.environ["DDM_PIPE_VERBOSE"] = "1"

    G, P = args.grid, args.parts
    dec = build_structured(synth.StructuredPoisson((G, G, G), (P, P, P)), overlap=args.overlap, pou_type="distance", shrink=0, neumann=(args.coarse == "geneo"))
    t0 = time.perf_counter()
    if args.coarse == "geneo":
        from dune_ddm_amd.geneo import geneo_basis
        tl = TwoLevelSchwarz(dec, coarse="none")
        tl.set_coarse_basis(geneo_basis(tl, nev=args.nev))
        tl.rebuild_combined("additive")
    else:
        tl = TwoLevelSchwarz(dec, coarse="pou")
    tl.schwarz.wait_setup()
    tl.ctx.sync()
    t_first = time.perf_counter() - t0
    res0, _, _ = tl.solve(reduction=args.reduction, maxit=1000, history=False)
    print(f"first object: {t_first:.2f} s of device setup (coarse space '{args.coarse}' included), engine {tl.schwarz.engine()}, {res0.iterations} iterations, "
          f"{res0.elapsed_s:.3f} s", flush=True)

    dec2 = changed_coefficient(dec, 5)
    rl2 = RankLocal(dec2)
    va, vd = sorted_data(rl2.A).copy(), sorted_data(rl2.A_dir).copy()
    del rl2

    tl.ctx.timing(True)
    tl.ctx.timing_reset()
    t0 = time.perf_counter()
    tl.update_values(va, vd)
    tl.ctx.sync()
    t_refresh = time.perf_counter() - t0
    dev_factor_ms, _ = tl.ctx.timer("Refresh/factor")
    dev_scatter_ms, _ = tl.ctx.timer("Refresh/scatter")
    tl.ctx.timing(False)
    phases = {k[len("refresh: "):]: v for k, v in tl.setup_times.items() if k.startswith("refresh: ")}
    res1, _, x1 = tl.solve(reduction=args.reduction, maxit=1000, history=False)
    print(f"update_values: {t_refresh:.2f} s; phases (s): " + ", ".join(f"{k} {v:.3f}" for k, v in phases.items()), flush=True)
    print(f"  device ILU(0) factorisation {dev_factor_ms * 1e-3:.3f} s, scatter into the engines {dev_scatter_ms * 1e-3:.3f} s; solve: {res1.iterations} iterations, "
          f"{res1.elapsed_s:.3f} s", flush=True)

    basis = tl.host_basis()
    with CaptureStderr() as cap:
        t0 = time.perf_counter()
        new = TwoLevelSchwarz(dec2, coarse=basis)
        new.schwarz.wait_setup()
        new.ctx.sync()
        t_new = time.perf_counter() - t0
    m = re.search(r"factorisation \(host, one thread per block\) ([0-9.]+) s", cap.text)
    host_factor_s = float(m.group(1)) if m else None
    res2, _, x2 = new.solve(reduction=args.reduction, maxit=1000, history=False)
    same = bool(res1.iterations == res2.iterations and (x1 == x2).all().item())
    print(f"new object on the same values (basis handed over): {t_new:.2f} s; phases (s): " + ", ".join(f"{k} {v:.2f}" for k, v in new.setup_times.items()), flush=True)
    print(f"  host ILU(0) factorisation at creation {host_factor_s} s; solve: {res2.iterations} iterations; refreshed and new object agree bit for bit: {same}", flush=True)
    print(json.dumps({"grid": G, "parts": P, "coarse": args.coarse, "engine": tl.schwarz.engine(), "refresh_s": t_refresh, "refresh_phases_s": phases,
                      "device_factorisation_s": dev_factor_ms * 1e-3, "device_scatter_s": dev_scatter_ms * 1e-3, "reconstruction_s": t_new,
                      "reconstruction_phases_s": new.setup_times, "host_factorisation_s": host_factor_s,
                      "iterations": [int(res0.iterations), int(res1.iterations), int(res2.iterations)], "bit_identical": same}), flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
