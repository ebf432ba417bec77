"""Worker of tests/test_gpu_multi_gmres.py, launched by torch.distributed.run (backend gloo): the ranks share cuda:0 (`levels` engine)
and exchange through the alltoall / allreduce callbacks.  Block GMRES with m = 4 right-hand sides (ddm_gmres_solve_multi): the halo
blocks go column by column through the callback, the Gram-Schmidt coefficients of one step in one all-reduce of m doubles.  Rank 0
compares with the same block solve on a single-rank context and prints MULTI_GMRES_RANKS_OK <world>."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from dune_ddm_amd import synth  # noqa: E402
from dune_ddm_amd.problem import build_structured  # noqa: E402

TOL_REL, TOL_ABS = 1e-7, 1e-11     # |h - h'| <= 1e-7 |r_k| + 1e-11 |r_0| for GMRES histories


def rhs_block(dec, tl, m, seed=17):
    rng = np.random.default_rng(seed)
    cols = [np.asarray(tl.rl.b, dtype=np.float64)]
    for _ in range(m - 1):
        xg = rng.standard_normal(dec.nglobal)           # the same global vectors on every rank
        cols.append(tl.rl.cat_novlp([xg[sd.glob[:sd.n_o]] for sd in dec.subs]))
    return np.stack(cols, axis=1)


def ranks():
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from dune_ddm_amd.solver import TorchComm, TwoLevelSchwarz
    m = 4
    kw = dict(schwarz_type="restricted", mode="additive", coarse="pou")
    solve = dict(reduction=1e-10, maxit=300, solver="restartedgmressolver", restart=6)
    dec = build_structured(synth.StructuredPoisson((15, 14, 13), (2, 2, 2)), overlap=2, pou_type="distance")
    tl = TwoLevelSchwarz(dec, rank, world, 0, TorchComm(), **kw)
    res, hist, X = tl.solve_multi(rhs_block(dec, tl, m), **solve)
    its = [r.iterations for r in res]
    assert all(r.converged for r in res), its
    parts = [None] * world
    dist.all_gather_object(parts, (tl.rl.local, X.cpu().numpy()))
    if rank == 0:
        ref = TwoLevelSchwarz(dec, **kw)   # single rank, all subdomains local
        res1, hist1, X1 = ref.solve_multi(rhs_block(dec, ref, m), **solve)
        its1 = [r.iterations for r in res1]
        print("iterations", its, its1, flush=True)
        assert its == its1, (its, its1)
        for c in range(m):
            h, h1 = hist[:its[c] + 1, c], hist1[:its[c] + 1, c]
            dev = np.abs(h - h1) - (TOL_REL * h1 + TOL_ABS * h1[0])
            print("column", c, "largest history excess over the tolerance", float(dev.max()), flush=True)
            assert (dev <= 0).all(), c
        X1 = X1.cpu().numpy()
        off = {}
        o = 0
        for sd in ref.rl.subs:
            off[sd.id] = o
            o += sd.n_o
        got = np.zeros_like(X1)
        for local, Xr in parts:
            p = 0
            for s in local:
                n_o = dec.subs[s].n_o
                got[off[s]:off[s] + n_o] = Xr[p:p + n_o]
                p += n_o
        err = np.max(np.abs(got - X1)) / np.max(np.abs(X1))
        print("x", err, flush=True)
        assert err <= 1e-8, err
        print("MULTI_GMRES_RANKS_OK", world, its, flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    ranks()
