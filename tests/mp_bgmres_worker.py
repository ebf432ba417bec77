"""Worker of tests/test_bgmres_ranks.py (launched by torch.distributed.run, backend gloo): the ranks share cuda:0 (`levels` engine) and
exchange through the alltoall / allreduce callbacks.  Block GMRES with m = 4 right-hand sides (ddm_bgmres_solve_multi) on restricted
Schwarz with the multiplicative coarse level, restart 6: the halo blocks go column by column through the callback, the Gram matrix of
the defects, the two projections and the Gram matrix of the new block as one all-reduce each.  Every rank must form the same factors
and the same least-squares solution from the reduced numbers, or the ranks' columns drift apart.  Rank 0 compares with the same block
solve on a single-rank context (all subdomains local) and prints BGMRES_RANKS_OK <world>."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from dune_ddm_amd import synth  # noqa: E402
from dune_ddm_amd.problem import build_structured  # noqa: E402

XTOL = 1e-8     # the bound of tests/test_gpu_bgmres.py for x against another summation order, relative to the largest entry of the column


def rhs_block(dec, tl, m, seed=17):
    rng = np.random.default_rng(seed)
    cols = [np.asarray(tl.rl.b, dtype=np.float64)]
    for _ in range(m - 1):
        xg = rng.standard_normal(dec.nglobal)           # the same global vectors on every rank
        cols.append(tl.rl.cat_novlp([xg[sd.glob[:sd.n_o]] for sd in dec.subs]))
    return np.stack(cols, axis=1)


def main():
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from dune_ddm_amd.solver import TorchComm, TwoLevelSchwarz
    m = 4
    kw = dict(schwarz_type="restricted", mode="multiplicative", coarse="pou")
    dec = build_structured(synth.StructuredPoisson((15, 14, 13), (2, 2, 2)), overlap=2, pou_type="distance")
    tl = TwoLevelSchwarz(dec, rank, world, 0, TorchComm(), **kw)
    ref = TwoLevelSchwarz(dec, **kw) if rank == 0 else None   # single rank, all subdomains local
    before = tl.ctx.comm_counts()
    res, hist, X, ranks = tl.solve_block_gmres(rhs_block(dec, tl, m), reduction=1e-10, maxit=300, restart=6)
    after = tl.ctx.comm_counts()
    its = [r.iterations for r in res]
    assert all(r.converged for r in res), its
    parts = [None] * world
    dist.all_gather_object(parts, (tl.rl.local, X.cpu().numpy(), its, ranks.tolist(), hist.tolist()))
    ok = True
    if rank == 0:
        res1, hist1, X1, ranks1 = ref.solve_block_gmres(rhs_block(dec, ref, m), reduction=1e-10, maxit=300, restart=6)
        its1 = [r.iterations for r in res1]
        print("iterations", its, its1, "widths", sorted(set(ranks.tolist())), "all-reduces", [int(a - b) for a, b in zip(after, before)], flush=True)
        X1 = X1.cpu().numpy()
        off = {}
        o = 0
        for sd in ref.rl.subs:
            off[sd.id] = o
            o += sd.n_o
        got = np.zeros_like(X1)
        for local, Xr, its_r, ranks_r, hist_r in parts:
            ok = ok and its_r == its and ranks_r == ranks.tolist() and hist_r == hist.tolist()   # every rank reports the same run
            p = 0
            for s in local:
                n_o = dec.subs[s].n_o
                got[off[s]:off[s] + n_o] = Xr[p:p + n_o]
                p += n_o
        err = [float(np.max(np.abs(got[:, c] - X1[:, c])) / np.max(np.abs(X1[:, c]))) for c in range(m)]
        print("x deviation per column", err, flush=True)
        ok = ok and its == its1 and ranks.tolist() == ranks1.tolist() and ranks[0] == m and len(ranks) > 6 and max(err) <= XTOL
    if rank == 0 and ok:
        print("BGMRES_RANKS_OK", world, flush=True)
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0 and not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
