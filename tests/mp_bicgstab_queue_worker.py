"""Worker of tests/test_gpu_bicgstab_queue.py, two modes.

  ranks            launched by torch.distributed.run (backend gloo): the ranks share cuda:0 and exchange through the alltoall /
                   allreduce callbacks.  M = 6 right-hand sides through w = 4 BiCGSTAB slots (ddm_bicgstab_solve_queue): the halo blocks
                   go column by column through the callback, the pairs of sums of one half step in one all-reduce of 2 w doubles.
                   Rank 0 compares with the same call on a single-rank context and prints BICGSTAB_QUEUE_RANKS_OK <world>.
  dump <out.npz>   a fresh single process (the environment switch DDM_BICGSTAB_QUEUE_FUSED is read by the library, once, from ITS
                   environment): queued solves with w = 1, 3, 8, 13 slots and M = w + 2 columns on the two problems of the test,
                   iterations, histories and solutions written to <out.npz> for a bitwise comparison by the parent."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from dune_ddm_amd import synth  # noqa: E402
from dune_ddm_amd.problem import build_structured  # noqa: E402

DUMP_W = (1, 3, 8, 13)
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


def dump(path):
    from dune_ddm_amd.solver import TwoLevelSchwarz
    out = {}
    for name, kw in CONFIGS.items():
        dec = decomposition(name)
        tl = TwoLevelSchwarz(dec, coarse="pou", **kw)
        for w in DUMP_W:
            res, hist, X = tl.solve_many(rhs_block(dec, tl, w + 2, seed=60 + w), width=w, reduction=RED, maxit=MAXIT, solver="bicgstabsolver")
            assert all(r.converged for r in res), (name, w)
            out[f"{name}_hist{w}"] = hist
            out[f"{name}_x{w}"] = X.cpu().numpy()
            out[f"{name}_it{w}"] = np.array([r.iterations for r in res])
        tl.prec.check_status()
        tl.ctx.close()
    np.savez(path, **out)
    print("BICGSTAB_QUEUE_DUMP_OK", os.environ.get("DDM_BICGSTAB_QUEUE_FUSED", "(unset)"), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "ranks":
        ranks()
    else:
        dump(sys.argv[2])
