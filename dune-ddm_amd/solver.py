"""High-level driver mirroring the call order of examples/poisson.cc:198-321 on one rank:

    A_dir, pou, interfaces  ->  SchwarzPreconditioner  ->  coarse basis (POU / GenEO / given)
    -> zero_at_dirichlet -> GalerkinPreconditioner (R A R^T assembled on the device)
    -> NonOverlappingOperator -> CombinedPreconditioner -> CG.

torch is used for device memory, the stream and torch.distributed (RCCL over xGMI); all compute
goes through the C ABI of libddm_hip.so.
"""
from __future__ import annotations

import numpy as np

from . import (BCG_RANK_TOL, BGMRES_RANK_TOL, bcg_solve_multi, bgmres_solve_multi, CombinedPreconditioner, Context, torch_context, gmres_solve, bicgstab_solve, CsrMatrix, GalerkinPreconditioner, Halo, NonOverlappingOperator,
               SchwarzPreconditioner, bicgstab_solve_queue, cg_solve, cg_solve_multi, cg_solve_queue, fcg_solve, fcg_solve_multi, fgmres_solve, fgmres_solve_multi, galerkin_products, gmres_solve_multi)
from .problem import Decomposition, RankLocal


class _DevView:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f8", "data": (int(ptr), False), "version": 2}


class TorchComm:
    """Inter-rank exchange over torch.distributed.  backend 'nccl' (= RCCL over xGMI) moves device
    buffers directly; with 'gloo' (CPU rehearsal of the N>1 path) buffers are staged through the host."""

    def __init__(self):
        import torch
        import torch.distributed as dist
        self.torch, self.dist = torch, dist
        self.rank, self.nranks = dist.get_rank(), dist.get_world_size()
        self.backend = dist.get_backend()
        self.halos = {}
        self._views = {}

    def view(self, ptr, n):
        key = (int(ptr), int(n))
        if key not in self._views:
            self._views[key] = self.torch.as_tensor(_DevView(ptr, n), device="cuda")
        return self._views[key]

    def register(self, halo: Halo):
        self.halos[halo.tag] = halo

    def alltoall(self, tag, sptr, rptr):
        h = self.halos[tag]
        ns, nr = sum(h.send_counts), sum(h.recv_counts)
        send = self.view(sptr, max(ns, 1))
        recv = self.view(rptr, max(nr, 1))
        staged = self.backend != "nccl"
        s_host = send.cpu() if staged else send
        r_host = self.torch.empty(max(nr, 1), dtype=self.torch.float64) if staged else recv
        ops = []
        so = ro = 0
        for r in range(self.nranks):
            sc, rc = h.send_counts[r], h.recv_counts[r]
            if r == self.rank:
                if sc:
                    r_host[ro:ro + rc].copy_(s_host[so:so + sc])
            else:
                if sc:
                    ops.append(self.dist.P2POp(self.dist.isend, s_host[so:so + sc], r))
                if rc:
                    ops.append(self.dist.P2POp(self.dist.irecv, r_host[ro:ro + rc], r))
            so += sc
            ro += rc
        if ops:
            for w in self.dist.batch_isend_irecv(ops):
                w.wait()
        if staged:
            recv[:max(nr, 1)].copy_(r_host)
        return 0

    def allreduce(self, ptr, n):
        t = self.view(ptr, n)
        if self.backend == "nccl":
            self.dist.all_reduce(t)
        else:
            h = t.cpu()
            self.dist.all_reduce(h)
            t.copy_(h)
        return 0


def pou_basis(rl: RankLocal, template_vecs=None):
    """POUCoarseSpace (coarse_spaces.hh:1175-1231): 1 * pou / ||pou||_2 per subdomain -- or, with
    ``template_vecs`` = {sub id: (t, n_s)}, the POU-scaled template vectors of the second constructor
    (:1226-1230, used by TwoLevelSchwarzSolver with 1, x, y, xy, twolevel_schwarz.hh:68-107) -- then
    zero_at_dirichlet (examples/poisson.cc:235-238,282).  Returns {sub id: (k, n_s) array}."""
    out = {}
    for sd in rl.subs:
        T = np.ones((1, sd.n)) if template_vecs is None else np.asarray(template_vecs[sd.id], dtype=np.float64)
        vecs = []
        for t in T:
            v = t * sd.pou                                          # finalize_eigenvectors (:52-61)
            v = v * (1.0 / np.sqrt(float(np.dot(v, v))))
            v[sd.dirichlet_ovlp > 0] = 0.0
            vecs.append(v)
        out[sd.id] = np.array(vecs)
    return out


class TwoLevelSchwarz:
    def __init__(self, dec: Decomposition, rank=0, nranks=1, device=0, comm: TorchComm | None = None,
                 schwarz_type="standard", mode="additive", coarse="pou", use_pou_in_schwarz=True, subdomain_solver="ilu0", multi_engine="levels"):
        import torch
        self.torch = torch
        torch.cuda.set_device(device)
        self.dev = torch.device("cuda", device)
        self.dec = dec
        self.comm = comm
        self.ctx = torch_context(device)
        import os
        self.exchange = "none"
        if nranks > 1 or os.environ.get("DDM_RCCL_SELFTEST") == "1":
            # inter-rank exchange: inside the library over RCCL / xGMI when the job runs on the nccl backend (one process per
            # GPU), else the callbacks over torch.distributed (gloo rehearsal: staged through the host; DDM_EXCHANGE=callback
            # forces them on nccl too).  torch.distributed only distributes the 128-byte communicator id.
            in_library = (comm is not None and comm.backend == "nccl" and os.environ.get("DDM_EXCHANGE", "rccl") != "callback") or nranks == 1
            if in_library:
                uid = [self.ctx.rccl_unique_id() if rank == 0 else None]
                if nranks > 1:
                    comm.dist.broadcast_object_list(uid, src=0)
                self.ctx.set_rccl(rank, nranks, uid[0], self_test=(nranks == 1))
                self.exchange = "rccl"
            else:
                assert comm is not None
                self.ctx.set_comm(rank, nranks, comm.alltoall, comm.allreduce)
                self.exchange = "callback"
        import time
        self.setup_times = {}                                          # seconds per phase of the device setup (diagnostics: bench.py logs them)
        _t = [time.perf_counter()]

        def lap(name):
            now = time.perf_counter()
            self.setup_times[name] = self.setup_times.get(name, 0.0) + now - _t[0]
            _t[0] = now
        self._lap = lap
        rl = self.rl = RankLocal(dec, rank, nranks)
        lap("rank-local numbering")
        ctx = self.ctx
        if comm is not None and comm.backend != "nccl":
            # gloo rehearsal: several ranks share one GPU.  The single-launch triangular solves need all
            # their workgroups co-resident (one process per GPU); fall back to one launch per level.
            os.environ["DDM_TRSV_MODE"] = "levels"
            os.environ["DDM_TRSV_MULTI_MODE"] = "levels"
            multi_engine = "levels"
        self.A = CsrMatrix(ctx, rl.A)
        self.A_dir = CsrMatrix(ctx, rl.A_dir)
        lap("matrix upload (A, A_dir)")
        self.h_novlp = Halo(ctx, 1, Halo.ADD, rl.plan_novlp_add)
        self.h_copy = Halo(ctx, 2, Halo.COPY, rl.plan_ovlp_copy)
        self.h_add = Halo(ctx, 3, Halo.ADD, rl.plan_ovlp_add)
        if comm is not None:
            for h in (self.h_novlp, self.h_copy, self.h_add):
                comm.register(h)
        self.op = NonOverlappingOperator(ctx, self.A, self.h_novlp, rl.owner_novlp)
        self.schwarz = SchwarzPreconditioner(ctx, self.A_dir, rl.block_ptr, rl.n_o, rl.ext_map,
                                             rl.pou if use_pou_in_schwarz else None, schwarz_type, self.h_copy, self.h_add,
                                             subdomain_solver=subdomain_solver)   # [schwarz.subdomain_solver] type (schwarz.hh:85-92)
        self._schwarz_args = (rl.pou if use_pou_in_schwarz else None, schwarz_type, subdomain_solver)   # (update_values may build the level anew)
        self._mode = mode
        self.multi_engine = multi_engine          # engine of the local solves of the block applies: 'levels' | 'xcd' (same bits)
        if multi_engine != "levels":
            self.schwarz.set_multi_engine(multi_engine)
        lap("halo plans, operator, local solver (factorisation, schedules)")
        self.galerkin = None
        self.a0 = None
        if coarse is not None and coarse != "none":
            basis = pou_basis(rl) if isinstance(coarse, str) and coarse == "pou" else coarse
            self.set_coarse_basis(basis)
        self.prec = CombinedPreconditioner(ctx, mode, self.op, self.schwarz, self.galerkin)

    def schwarz_levels(self):
        return self.schwarz.num_levels()

    def rebuild_combined(self, mode="additive"):
        self._mode = mode
        self.prec = CombinedPreconditioner(self.ctx, mode, self.op, self.schwarz, self.galerkin)

    def host_basis(self):
        """coarse basis as {sub id: [vectors]} for every subdomain (single-rank runs; checker input)"""
        return {s: [v.copy() for v in self.basis_by_sub[s]] for s in self.rl.local}

    # -- device vectors
    def zeros(self, n):
        return self.torch.zeros(int(n), dtype=self.torch.float64, device=self.dev)

    def to_device(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    # -- coarse level -------------------------------------------------------------------------
    def set_coarse_basis(self, basis_by_sub):
        """basis_by_sub: {local sub id: (k_s, n_s) array}; builds R A R^T and the Galerkin level."""
        rl, dec, torch = self.rl, self.dec, self.torch
        P = dec.nsub
        self.basis_by_sub = {s: np.asarray(basis_by_sub[s], dtype=np.float64) for s in rl.local}
        basis_by_sub = self.basis_by_sub                       # (arrays, also where the caller passed lists of vectors: host_basis())
        k_local = {s: int(basis_by_sub[s].shape[0]) for s in rl.local}
        k_all = self._allgather_small(k_local, P)              # MPI_Allgather of num_t (galerkin_preconditioner.hh:248)
        kmax = max(k_all)
        offset = np.concatenate([[0], np.cumsum(k_all)[:-1]]).astype(np.int64)   # offset_per_rank (:256)
        K = int(sum(k_all))
        basis = np.zeros((kmax, rl.n))
        coarse_index = np.full((len(rl.local), kmax), -1, dtype=np.int64)
        for li, s in enumerate(rl.local):
            basis[:k_all[s], rl.off[s]:rl.off[s] + dec.subs[s].n] = basis_by_sub[s]
            coarse_index[li, :k_all[s]] = offset[s] + np.arange(k_all[s])
        self.k_all, self.coarse_offset, self.K = k_all, offset, K
        import time
        t0 = time.perf_counter()
        A0 = self._build_coarse_matrix(basis, k_all, offset, K)
        t1 = time.perf_counter()
        self.a0 = A0
        a0inv = np.linalg.inv(A0)
        self.galerkin = GalerkinPreconditioner(self.ctx, rl.n, rl.n_o, rl.ext_map, rl.block_ptr, basis, coarse_index.reshape(-1),
                                               a0inv, self.h_copy, self.h_add)
        self.setup_times["coarse matrix R A R^T"] = t1 - t0
        self.setup_times["coarse inverse, basis upload"] = time.perf_counter() - t1

    def update_values(self, A_values, A_dir_values, *, A_neu_values=None, B_neu_values=None, coarse="keep"):
        """New matrix values in the patterns the object was built on (a Newton step, a time step with a changing coefficient):
        A_values / A_dir_values are the ``data`` arrays of the rank-local A and A_dir in CSR order with sorted column indices.  The
        decomposition, the halo plans, the schedules of the local solver and the coarse basis are kept; refreshed are the two matrices,
        the operator's storage, the local factor -- ILU(0) or the device supernodal direct factor -- on the device
        (SchwarzPreconditioner.refresh: ``schwarz`` stays the same object, schwarz.refresh_count() counts), R A R^T with the existing
        basis and its inverse.  A local solver that cannot be refreshed in place (the host-engine direct factor, the box engine, a
        device direct factor whose new values belong to the host engine: DDM_ENOTIMPL) is built anew, that level only.  The result is bit for bit what a new TwoLevelSchwarz on the new matrices with ``coarse=host_basis()`` gives.
        coarse="keep" (default) keeps the basis.  coarse="refresh" makes the coarse space follow as well: it needs the kept eigensolver
        ``self.geneo`` (geneo_basis(..., keep=True)) and A_neu_values (B_neu_values where B_neu is its own matrix), per subdomain as
        GeneoSolver.update takes them; the eigensolver's pencil and preconditioner are refreshed on the device, the basis is recomputed
        from the kept eigenvectors and handed to set_coarse_basis (the number of vectors may change in threshold mode).
        The phases add to setup_times under "refresh: ..."."""
        va, vd = np.ascontiguousarray(A_values, dtype=np.float64), np.ascontiguousarray(A_dir_values, dtype=np.float64)
        if va.shape != (self.A.nnz,) or vd.shape != (self.A_dir.nnz,):       # (before anything is touched)
            raise ValueError(f"update_values: {va.size} and {vd.size} values for patterns of {self.A.nnz} (A) and {self.A_dir.nnz} (A_dir) entries")
        if coarse not in ("keep", "refresh"):
            raise ValueError(f"update_values: coarse = {coarse!r} (keep or refresh)")
        if coarse == "refresh":
            geneo = getattr(self, "geneo", None)
            if geneo is None or geneo.h is None:
                raise ValueError("update_values(coarse='refresh') needs the kept eigensolver: geneo_basis(tl, ..., keep=True)")
            if A_neu_values is None:
                raise ValueError("update_values(coarse='refresh') needs A_neu_values")
            if B_neu_values is not None and geneo.dB is geneo.dA:
                raise ValueError("update_values: B_neu is A_neu in the kept eigensolver; pass its values as A_neu_values only")
            geneo._values(A_neu_values, geneo._nnz_A, "A_neu")                # (lengths, before anything is touched)
            if B_neu_values is not None:
                geneo._values(B_neu_values, geneo._nnz_B, "B_neu")
        import time
        from . import DDM_ENOTIMPL, DdmError
        t = [time.perf_counter()]

        def lap(name):
            self.ctx.sync()
            now = time.perf_counter()
            self.setup_times["refresh: " + name] = now - t[0]
            t[0] = now
        recreated = False
        self.A.set_values(va)
        self.A_dir.set_values(vd)
        for M, v in ((self.rl.A, va), (self.rl.A_dir, vd)):                 # (the host copies, where they are in the same order)
            if getattr(M, "has_sorted_indices", False) and M.data.shape == v.shape:
                M.data[:] = v
        lap("matrix values (A, A_dir)")
        self.op.refresh()
        lap("operator storage")
        try:
            self.schwarz.refresh()
            lap("local solver (device factorisation, scatter)")
        except DdmError as e:
            if e.code != DDM_ENOTIMPL:
                raise
            self.schwarz = SchwarzPreconditioner(self.ctx, self.A_dir, self.rl.block_ptr, self.rl.n_o, self.rl.ext_map, self._schwarz_args[0],
                                                 self._schwarz_args[1], self.h_copy, self.h_add, subdomain_solver=self._schwarz_args[2])
            if self.multi_engine != "levels":
                self.schwarz.set_multi_engine(self.multi_engine)
            lap("local solver (created anew)")
            recreated = True
        if coarse == "refresh":
            self.geneo.update(A_neu_values, B_neu_values)
            lap("GenEO pencil and preconditioner")
            basis = self.geneo.compute("kept")
            lap("GenEO basis from the kept block")
            self.set_coarse_basis(basis)
            lap("GenEO coarse matrix, inverse, basis upload")
            recreated = True                                                  # (a new Galerkin level: the combination is rebuilt)
        elif self.galerkin is not None:
            kmax = max(self.k_all)
            basis = np.zeros((kmax, self.rl.n))
            for s in self.rl.local:
                basis[:self.k_all[s], self.rl.off[s]:self.rl.off[s] + self.dec.subs[s].n] = self.basis_by_sub[s]
            self.a0 = self._build_coarse_matrix(basis, self.k_all, self.coarse_offset, self.K)
            lap("coarse matrix R A R^T")
            self.galerkin.set_inverse(np.linalg.inv(self.a0))
            lap("coarse inverse")
        if recreated:                                                        # (the combination holds the level it was built with)
            self.prec = CombinedPreconditioner(self.ctx, self._mode, self.op, self.schwarz, self.galerkin)

    def _allgather_small(self, local: dict, P):
        if self.comm is None:
            return [local[s] for s in range(P)]
        objs = [None] * self.comm.nranks
        self.comm.dist.all_gather_object(objs, local)
        merged = {}
        for o in objs:
            merged.update(o)
        return [merged[s] for s in range(P)]

    def _build_coarse_matrix(self, basis, k_all, offset, K):
        """GalerkinPreconditioner::build_solver (galerkin_preconditioner.hh:219-349) on the device:
        local x local blocks from Y = A_dir R^T, local x neighbour blocks from the neighbours' vectors
        restricted to the shared indices (CopyGatherScatterWithRank, :66-103), one neighbour slot
        at a time for all local subdomains at once (A_dir is block diagonal)."""
        rl, dec, torch, ctx = self.rl, self.dec, self.torch, self.ctx
        kmax = basis.shape[0]
        R = self.to_device(basis)                                   # (kmax, n)
        A0 = np.zeros((K, K))
        for s in rl.local:                                           # :292-295
            blk = galerkin_products(ctx, self.A_dir, R, R, rl.off[s], rl.off[s] + dec.subs[s].n)   # [i, j] = <r_i, A r_j>
            ks = k_all[s]
            A0[offset[s]:offset[s] + ks, offset[s]:offset[s] + ks] = blk[:ks, :ks]
        nbrs = {s: sorted({a for (a, b) in dec.ovlp_all if b == s}) for s in rl.local}
        nslots = max([len(v) for v in nbrs.values()] + [0])
        if self.comm is not None:
            nslots = max(self._allgather_small({s: len(nbrs[s]) for s in rl.local}, dec.nsub) + [0])
        from .problem import halo_plan
        offs = {s: rl.off.get(s, 0) for s in range(dec.nsub)}
        for t in range(nslots):                                      # :298-309, 321-327
            pairs_t = {(a, b): v for (a, b), v in dec.ovlp_all.items()
                       if self._slot_of(dec, a, b) == t}
            plan = halo_plan(pairs_t, rl.local, rl.sub2rank, offs, rl.rank, rl.nranks)
            halo = Halo(ctx, 100 + t, Halo.COPY, plan)
            if self.comm is not None:
                self.comm.register(halo)
            V = torch.zeros_like(R)         # the neighbours' vectors restricted to the shared indices, zero elsewhere (:96-101)
            for j in range(kmax):
                halo.exchange_to(R[j], V[j])
            for s in rl.local:
                if t >= len(nbrs[s]):
                    continue
                src = nbrs[s][t]
                blk = galerkin_products(ctx, self.A_dir, R, V, rl.off[s], rl.off[s] + dec.subs[s].n)
                A0[offset[s]:offset[s] + k_all[s], offset[src]:offset[src] + k_all[src]] = blk[:k_all[s], :k_all[src]]
            self.ctx.sync()
        if self.comm is not None:                                    # gatherMatrixFromRowsFlat (helpers.hh:204-339), replicated
            t_ = torch.as_tensor(A0)
            if self.comm.backend == "nccl":
                t_ = t_.to(self.dev)
            self.comm.dist.all_reduce(t_)
            A0 = t_.cpu().numpy()
        return A0

    @staticmethod
    def _slot_of(dec, src, dst):
        cache = dec.meta.setdefault("_nbr_slots", {})
        if dst not in cache:
            cache[dst] = {a: i for i, a in enumerate(sorted({a for (a, b) in dec.ovlp_all if b == dst}))}
        return cache[dst][src]

    # -- solve -------------------------------------------------------------------------------
    SOLVERS = ("cgsolver", "restartedgmressolver", "restartedflexiblegmressolver", "restartedfcgsolver", "completefcgsolver", "bicgstabsolver")
    SOLVERS_MULTI = SOLVERS[:5]   # (the block BiCGSTAB loop is the queued one: solve_many with M <= width)

    def solve(self, reduction=1e-10, maxit=1000, fixed_iterations=0, history=True, x0=None, b=None, solver="cgsolver", restart=100, mmax=10):
        """v = 0; solver->apply(v, b, res)  (examples/poisson.cc:318-319).  solver: "cgsolver", "restartedgmressolver",
        "restartedflexiblegmressolver", "restartedfcgsolver", "completefcgsolver" (flexible CG with mmax + 1 slots) or "bicgstabsolver"
        (the [solver] type keys of dune-istl's solver factory).  Returns (res, hist, x)."""
        if solver not in self.SOLVERS:
            raise NotImplementedError("solver type '" + str(solver) + "' (" + ", ".join(self.SOLVERS[:-1]) + " and " + self.SOLVERS[-1]
                                      + " are available on the device)")
        x = self.zeros(self.rl.n_o) if x0 is None else self.to_device(x0)
        bd = self.to_device(self.rl.b if b is None else b)
        if solver == "restartedflexiblegmressolver":
            res, hist = fgmres_solve(self.ctx, self.op, self.prec, x, bd, reduction, maxit, restart, history)
            return res, hist, x
        if solver in ("restartedfcgsolver", "completefcgsolver"):
            res, hist = fcg_solve(self.ctx, self.op, self.prec, x, bd, reduction, maxit, mmax, solver == "completefcgsolver", history)
            return res, hist, x
        if solver == "restartedgmressolver":
            res, hist = gmres_solve(self.ctx, self.op, self.prec, x, bd, reduction, maxit, restart, history)
            return res, hist, x
        if solver == "bicgstabsolver":
            res, hist = bicgstab_solve(self.ctx, self.op, self.prec, x, bd, reduction, maxit, history)
            return res, hist, x
        res, hist = cg_solve(self.ctx, self.op, self.prec, x, bd, reduction, maxit, fixed_iterations, history)
        return res, hist, x

    def _blocks(self, B, X0):
        """device copies of the right-hand sides and the initial guesses (zero without X0) as (n_o, m) row-major blocks"""
        torch = self.torch
        n_o = self.rl.n_o

        def block(a):
            t = a.to(self.dev, torch.float64) if isinstance(a, torch.Tensor) else self.to_device(np.asarray(a, dtype=np.float64))
            t = t.reshape(n_o, 1) if t.dim() == 1 else t
            if t.dim() != 2 or t.shape[0] != n_o:
                raise ValueError(f"expected an (n_o, m) block with n_o = {n_o}, got {tuple(t.shape)}")
            return t.contiguous().clone()
        Bd = block(B)
        X = torch.zeros_like(Bd) if X0 is None else block(X0)
        if X.shape != Bd.shape:
            raise ValueError(f"X0 {tuple(X.shape)} and B {tuple(Bd.shape)} differ")
        return Bd, X

    def solve_multi(self, B=None, reduction=1e-10, maxit=1000, history=True, X0=None, solver="cgsolver", restart=100, mmax=10):
        """m right-hand sides at once: m independent CG solves (ddm_cg_solve_multi) or, with solver="restartedgmressolver" /
        "restartedflexiblegmressolver", m independent (flexible) restarted GMRES solves with aligned restart cycles
        (ddm_gmres_solve_multi / ddm_fgmres_solve_multi), or, with "restartedfcgsolver" / "completefcgsolver", m independent flexible CG
        solves that share the slot index (ddm_fcg_solve_multi), each column as ``solve`` would run it.
        B, X0: (n_o, m) arrays or tensors (B=None: the problem's right-hand side as one column).  Returns (list of m SolveResult,
        (iters + 1) x m history or None, X as an (n_o, m) device tensor)."""
        if solver not in self.SOLVERS_MULTI:
            raise NotImplementedError("solver type '" + str(solver) + "' (of the six device solvers " + ", ".join(self.SOLVERS)
                                      + ", all but bicgstabsolver are available for several right-hand sides)")
        n_o = self.rl.n_o
        if B is None:
            B = np.asarray(self.rl.b, dtype=np.float64).reshape(n_o, 1)
        Bd, X = self._blocks(B, X0)
        if solver == "restartedgmressolver":
            res, hist = gmres_solve_multi(self.ctx, self.op, self.prec, X, Bd, reduction, maxit, restart, history)
        elif solver == "restartedflexiblegmressolver":
            res, hist = fgmres_solve_multi(self.ctx, self.op, self.prec, X, Bd, reduction, maxit, restart, history)
        elif solver in ("restartedfcgsolver", "completefcgsolver"):
            res, hist = fcg_solve_multi(self.ctx, self.op, self.prec, X, Bd, reduction, maxit, mmax, solver == "completefcgsolver", history)
        else:
            res, hist = cg_solve_multi(self.ctx, self.op, self.prec, X, Bd, reduction, maxit, history)
        return res, hist, X

    def solve_block(self, B, reduction=1e-10, maxit=1000, history=True, X0=None, rank_tol=BCG_RANK_TOL):
        """m right-hand sides through ONE shared search space: block CG (ddm_bcg_solve_multi), a true block-Krylov method -- every
        column's error is minimised over the span of all columns' Krylov spaces, so it needs fewer iterations than ``solve_multi`` on
        the same block, the more the harder the operator.  For a symmetric positive definite preconditioner only (standard Schwarz,
        additive combination), as CG.  Dependent or duplicate columns and zero columns are safe (the m x m coupling is solved with a
        pseudo-inverse; rank_tol: relative eigenvalue below which a direction counts as dependent).  B, X0: (n_o, m) arrays or tensors,
        m <= 32.  Returns (list of m SolveResult -- iterations: the first iteration at which the column passed its test --, the
        (k_end + 1) x m history or None, X as an (n_o, m) device tensor, the k_end ranks of the coupling matrix)."""
        Bd, X = self._blocks(B, X0)
        res, hist, ranks = bcg_solve_multi(self.ctx, self.op, self.prec, X, Bd, reduction, maxit, rank_tol, history)
        return res, hist, X, ranks

    def solve_block_gmres(self, B, reduction=1e-10, maxit=1000, restart=100, history=True, X0=None, rank_tol=BGMRES_RANK_TOL):
        """m right-hand sides through ONE shared Krylov space: block GMRES (ddm_bgmres_solve_multi), the companion of ``solve_block``
        for a preconditioner that is not symmetric (restricted Schwarz, the multiplicative combination, a non-symmetric operator).
        Right preconditioning with a fixed preconditioner; the true defect is monitored and recomputed at every cycle end.  The block is
        deflated at every cycle start, so dependent, duplicate and zero columns are safe and cost no width (rank_tol: relative
        eigenvalue below which a direction counts as dependent).  maxit counts block iterations; restart: block iterations per cycle
        (the basis takes (restart + 1) n_o m doubles).  B, X0: (n_o, m) arrays or tensors, m <= 32.  Returns (list of m SolveResult --
        iterations: the first block iteration at which the column passed its test and stayed passed --, the (k_end + 1) x m history or
        None, X as an (n_o, m) device tensor, the k_end cycle widths)."""
        Bd, X = self._blocks(B, X0)
        res, hist, widths = bgmres_solve_multi(self.ctx, self.op, self.prec, X, Bd, reduction, maxit, restart, rank_tol, history)
        return res, hist, X, widths

    def solve_many(self, B, width=8, reduction=1e-10, maxit=1000, history=True, X0=None, solver="cgsolver"):
        """Any number M of right-hand sides, M independent solves through one block loop of ``width`` <= 32 slots: a slot whose column
        has stopped takes the next pending column, so no slot idles while columns wait.  solver="cgsolver" (ddm_cg_solve_queue): each
        column is what ``solve_multi`` computes on it.  solver="bicgstabsolver" (ddm_bicgstab_solve_queue), for the non-symmetric
        configurations: each column is what ``solve(solver="bicgstabsolver")`` computes on it, and with M <= width this is the block
        BiCGSTAB solve.  B, X0: (n_o, M) arrays or tensors, M may be smaller than ``width``.  Returns (list of M SolveResult, history or
        None -- row k of column j: its defect after its own k-th iteration (cgsolver) or half step (bicgstabsolver), NaN after its last
        --, X as an (n_o, M) device tensor)."""
        if solver not in ("cgsolver", "bicgstabsolver"):
            raise NotImplementedError("solver type '" + str(solver) + "' (cgsolver and bicgstabsolver take any number of right-hand sides "
                                      "through a block of fixed width)")
        if not 1 <= int(width) <= 32:
            raise ValueError(f"width = {width} outside [1, 32]")
        if int(maxit) < 0:
            raise ValueError(f"maxit = {maxit} is negative")
        Bd, X = self._blocks(B, X0)
        queue = bicgstab_solve_queue if solver == "bicgstabsolver" else cg_solve_queue
        res, hist = queue(self.ctx, self.op, self.prec, X, Bd, int(width), reduction, maxit, history)
        return res, hist, X


class TwoLevelSchwarzSolver:
    """Host mirror of the PDELab linear-solver backend ``TwoLevelSchwarzSolver`` (dune/ddm/twolevel_schwarz.hh:27-174), the class
    examples/convectiondiffusiondg.cc:75-78 and nonlinearpoisson.cc:151-154 hand to StationaryLinearProblemSolver / Newton:

      ctor   : non-overlapping communication + the four template vectors 1, x, y, xy with constrained DoFs zeroed (:58-81)
      apply  : (first call) overlap extension by ``overlap`` layers, overlapping matrix, PartitionOfUnity from the ``pou`` sub-tree,
               template vectors extended by copyOwnerToAll (:93-128); (every call) POUCoarseSpace(template vectors, pou) ->
               SchwarzPreconditioner (sub-tree "fine") + GalerkinPreconditioner ("coarse") in a CombinedPreconditioner whose mode
               key sits in the sub-tree itself (:131-142), solver from the "solver" sub-tree or restarted GMRES(30), maxit 1000
               (:146-160), right-hand side made consistent (:163-164), solve (:167-168).

    ``problem`` is one of the synth problems (it plays the role of the grid function space + assembled matrix); ``ptree`` the
    ``twolevelschwarz`` sub-tree as a nested dict (the keys of examples/convectiondiffusiondg.ini)."""

    def __init__(self, problem, ptree=None, coords=None, device=0):
        from .problem import build_structured
        self.ptree = dict(ptree or {})
        self.problem = problem
        overlap = int(self.ptree.get("overlap", 1))                                                    # :95
        pou = dict(self.ptree.get("pou", {}))
        self.dec = build_structured(problem, overlap=overlap, pou_type=pou.get("type", "distance"), shrink=int(pou.get("shrink", 0)))
        fine = dict(self.ptree.get("fine", {}))
        solver_type = dict(fine.get("subdomain_solver", {})).get("type")
        if solver_type is None:
            raise ValueError("You must specify the solver in the subtree fine.subdomain_solver using the key 'type'")   # schwarz.hh:89-91
        self.tl = TwoLevelSchwarz(self.dec, device=device, coarse="none", schwarz_type=fine.get("type", "restricted"),
                                  mode=self.ptree.get("mode", "additive"), subdomain_solver=solver_type)
        # template vectors 1, x, y, xy on the overlapping index sets (interpolation at the DoF positions, constrained DoFs zeroed)
        coords = coords if coords is not None else problem.dof_coords
        basis = {}
        for sd in self.tl.rl.subs:
            X = coords(sd.glob)
            T = np.stack([np.ones(sd.n), X[:, 0], X[:, 1], X[:, 0] * X[:, 1]])
            T[:, sd.dirichlet_ovlp > 0] = 0.0                                                          # set_constrained_dofs(cc, 0., v) (:75)
            V = T * sd.pou[None, :]                                                                    # POUCoarseSpace (coarse_spaces.hh:1226-1230)
            basis[sd.id] = V / np.linalg.norm(V, axis=1)[:, None]
        self.template_basis = basis
        self.tl.set_coarse_basis(basis)
        self.tl.rebuild_combined(self.ptree.get("mode", "additive"))
        self.result = None

    def apply(self, reduction, b=None):
        """solve A z = r to the given reduction (twolevel_schwarz.hh:84-169); returns (SolveResult, history, z)"""
        sol = dict(self.ptree.get("solver", {"type": "restartedgmressolver", "restart": 30, "maxit": 1000}))   # :146-153
        res, hist, z = self.tl.solve(reduction=reduction, maxit=int(sol.get("maxit", 1000)), solver=sol.get("type", "restartedgmressolver"),
                                     restart=int(sol.get("restart", 30)), mmax=int(sol.get("mmax", 10)), b=b)
        self.tl.prec.check_status()
        self.result = res                                                                              # LinearResultStorage (:170-174)
        return res, hist, z
