"""Worker of tests/test_multi_rhs_ranks.py (launched by torch.distributed.run, backend gloo): the ranks share cuda:0 and exchange through
the alltoall / allreduce callbacks (staged through the host).  Block CG with m = 4 right-hand sides (ddm_cg_solve_multi): the halo blocks
go column by column through the callback, the coarse defect block (K x m) in one all-reduce.  Rank 0 compares with the same block solve
on a single-rank context (all subdomains local) and prints MULTI_RANKS_OK <world>."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from dune_ddm_amd import synth  # noqa: E402
from dune_ddm_amd.problem import build_structured  # noqa: E402


def rhs_block(dec, tl, m):
    rng = np.random.default_rng(17)
    cols = [np.asarray(tl.rl.b, dtype=np.float64)]
    for _ in range(m - 1):
        xg = rng.standard_normal(dec.nglobal)           # the same global vectors on every rank
        cols.append(tl.rl.cat_novlp([xg[sd.glob[:sd.n_o]] for sd in dec.subs]))
    return np.stack(cols, axis=1)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from dune_ddm_amd.solver import TorchComm, TwoLevelSchwarz
    m = 4
    dec = build_structured(synth.StructuredPoisson((15, 14, 13), (2, 2, 2)), overlap=2, pou_type="distance")
    tl = TwoLevelSchwarz(dec, rank, world, 0, TorchComm(), schwarz_type="standard", mode="additive", coarse="pou")
    res, hist, X = tl.solve_multi(rhs_block(dec, tl, m), reduction=1e-10, maxit=300)
    its = [r.iterations for r in res]
    assert all(r.converged for r in res), its
    parts = [None] * world
    dist.all_gather_object(parts, (tl.rl.local, X.cpu().numpy()))
    if rank == 0:
        ref = TwoLevelSchwarz(dec, schwarz_type="standard", mode="additive", coarse="pou")   # single rank, all subdomains local
        res1, hist1, X1 = ref.solve_multi(rhs_block(dec, ref, m), reduction=1e-10, maxit=300)
        assert its == [r.iterations for r in res1], (its, [r.iterations for r in res1])
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
        assert np.max(np.abs(got - X1)) <= 1e-8 * np.max(np.abs(X1)), np.max(np.abs(got - X1))
        print("MULTI_RANKS_OK", world, its, flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
