"""Worker of tests/test_gpu_bicgstab_queue.py, launched by torch.distributed.run (backend gloo): the ranks share cuda:0 and exchange
through the alltoall / allreduce callbacks.  M = 6 right-hand sides through w = 4 BiCGSTAB slots (ddm_bicgstab_solve_queue): the halo
blocks go column by column through the callback, the sums of one block dot in one all-reduce of w doubles.  Rank 0 compares with the
same call on a single-rank context and prints BICGSTAB_QUEUE_RANKS_OK <world>.  The test module takes its two problems from here."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from dune_ddm_amd import synth  # noqa: E402
from dune_ddm_amd.problem import build_structured  # noqa: E402

RED, MAXIT = 1e-9, 200
CONFIGS = {
    "poisson": dict(schwarz_type="restricted", mode="multiplicative", subdomain_solver="ilu0"),     # non-symmetric preconditioner
    "dg": dict(schwarz_type="standard", mode="additive", subdomain_solver="umfpack"),               # non-symmetric operator
}


def decomposition(name):
    if name == "poisson":
        return build_structured(synth.StructuredPoisson((17, 16, 15), (2, 2, 2)), overlap=2, pou_type="distance", shrink=0)
    return build_structured(synth.StructuredDG2D((24, 24), (2, 2)), overlap=2)


def rhs_block(dec, tl, m, seed):
    """m consistent seeded random columns, zero on the Dirichlet rows (the same global vectors on every rank)"""
    rng = np.random.default_rng(seed)
    free = tl.rl.cat_novlp([(sd.dirichlet_ovlp[:sd.n_o] == 0).astype(np.float64) for sd in dec.subs])
    cols = []
    for _ in range(m):
        xg = rng.standard_normal(dec.nglobal)
        cols.append(tl.rl.cat_novlp([xg[sd.glob[:sd.n_o]] for sd in dec.subs]) * free)
    return np.stack(cols, axis=1)


def ranks():
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from dune_ddm_amd.solver import TorchComm, TwoLevelSchwarz
    M, w = 6, 4
    kw = dict(coarse="pou", **CONFIGS["poisson"])
    dec = decomposition("poisson")
    tl = TwoLevelSchwarz(dec, rank, world, 0, TorchComm(), **kw)
    res, hist, X = tl.solve_many(rhs_block(dec, tl, M, 21), width=w, reduction=RED, maxit=MAXIT, solver="bicgstabsolver")
    nh = [int(np.sum(~np.isnan(hist[:, j]))) for j in range(M)]
    assert all(r.converged for r in res), nh
    parts = [None] * world
    dist.all_gather_object(parts, (tl.rl.local, X.cpu().numpy()))
    if rank == 0:
        ref = TwoLevelSchwarz(dec, **kw)   # single rank, all subdomains local
        res1, hist1, X1 = ref.solve_many(rhs_block(dec, ref, M, 21), width=w, reduction=RED, maxit=MAXIT, solver="bicgstabsolver")
        nh1 = [int(np.sum(~np.isnan(hist1[:, j]))) for j in range(M)]
        print("half steps + 1", nh, nh1, flush=True)
        assert nh == nh1, (nh, nh1)
        X1 = X1.cpu().numpy()
        off, o = {}, 0
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
        err = np.max(np.abs(got - X1), axis=0) / np.max(np.abs(X1), axis=0)
        print("x", err, flush=True)
        assert (err <= 1e-7).all(), err
        print("BICGSTAB_QUEUE_RANKS_OK", world, nh, flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    ranks()
