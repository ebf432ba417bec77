// C-ABI implementation of include/ddm_hip.h, one translation unit, gfx950 only, no fallback path.  This file is the table of
// contents: every object of the library lives in one header below, included once, in dependency order.  Only the two small export
// groups at the end (dense host helpers, input synthesis) have their bodies here.
#include "../../include/ddm_hip.h"

#include <dlfcn.h>
#include <rccl/rccl.h> // types and enums only: the library is opened with dlopen when ddm_ctx_set_rccl is called

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

// ---- building blocks without a context ------------------------------------------------------------
#include "host_vec.hpp"         // hvec<T>: host arrays without value initialisation.  Needs nothing.
#include "device_buffer.hpp"    // dbuf<T>, reserve_cols: the one owner of a device allocation.  Needs nothing.
#include "trsv_multi_plan.hpp" // namespace multi_xcd: levels, per-block plan tables and team arithmetic of the single-launch block solve (host; team_of also device).  Needs nothing.
#include "kernels.hpp"          // namespace ddm: single-vector kernels, WG, RED_MAX_BLOCKS, RowChunk, level descriptors.  Needs nothing.
#include "multi_kernels.hpp"    // kernels of the m-column paths, MULTI_MAX, MultiCoef.  Needs kernels.hpp.
#include "trsv_pipe.hpp"        // pipe engine of the ILU(0) solve: kernels and host schedule.  Needs host_vec.hpp.
#include "trsv_box.hpp"         // box engine of the ILU(0) solve: kernels and host schedule.  Needs nothing.
#include "sparse_chol_host.hpp" // namespace chol: host sparse Cholesky / LU (ordering, symbolic, numeric).  Needs nothing.
#include "sn_chol.hpp"          // namespace sn: supernodal factor on the device, factorisation and block-solve kernels (pulls in sn_chol_host.hpp).  Needs device_buffer.hpp, sparse_chol_host.hpp.
#include "sn_solve1.hpp"        // namespace sn: its single-vector solve kernels, TopPlan, ChainDev.  Needs sn_chol.hpp.
#include "sn_factor.hpp"        // namespace sn: its host driver: Factor, build, factorize, reserve, solve.  Needs sn_chol.hpp, sn_solve1.hpp.
#include "synth_host.hpp"       // namespace synth: Q1 matrix rows on the host.  Needs nothing.

using namespace ddm;

// ---- the objects of include/ddm_hip.h --------------------------------------------------------------
#include "context.hpp"          // ddm_ctx, fail and the *CHECK macros, grid sizes, upload, timers, RCCL plumbing, all-reduce, ddm_ctx_* / malloc / memcpy / timing.  Needs the building blocks.
#include "csr.hpp"              // ddm_csr, host_threads, row blocks, tiled row order, csr_adopt, products up to ddm_csr_mm.  Needs context.hpp.
#include "local_factor.hpp"     // ddm_ilu0 and its engine parts, SolveKey / GraphCache, engine choice, join of the background build.  Needs csr.hpp, trsv_*.hpp, sn_factor.hpp.
#include "tri_levels.hpp"       // sliced-ELL level schedules of ILU(0): build_schedule, enqueue_tri, enqueue_multi_levels(_f32).  Needs local_factor.hpp.
#include "tri_csr.hpp"          // CSR level schedules of the host direct factor: supernodes, build_csr_schedule, enqueue_tri_csr, enqueue_multi_levels_csr.  Needs local_factor.hpp.
#include "engine_xcd2.hpp"      // xcd2 engine: build_xcd_schedule, enqueue_xcd2.  Needs local_factor.hpp.
#include "engine_pipe.hpp"      // pipe engine: build_pipe_schedule, enqueue_pipe.  Needs local_factor.hpp, trsv_pipe.hpp.
#include "engine_multi_xcd.hpp" // engine `xcd` of the block solve: build_multi_xcd, enqueue_multi_xcd, ddm_ilu0_set_multi_engine / _multi_info, ddm_trsv_multi_*_host.  Needs local_factor.hpp.
#include "ilu0_refactor.hpp"    // value refresh of an ILU(0) factor: device factorisation, scatter into the engines, ddm_ilu0_refresh.  Needs tri_levels.hpp, engine_xcd2.hpp, engine_pipe.hpp.
#include "engine_box.hpp"       // box engine: build_box_engine, enqueue_box, ddm_ilu0_box_check.  Needs local_factor.hpp, trsv_box.hpp.
#include "local_solve.hpp"      // the solves: ilu0_enqueue, graph capture, ilu0_solve_epilogue, ilu0_solve_multi_ld, ddm_ilu0_solve*.  Needs tri_*.hpp, engine_*.hpp.
#include "local_solver.hpp"     // creation: ilu0_create_impl, direct_create_impl, ddm_ilu0_* / ddm_chol_* / ddm_direct_* / ddm_sn_host_*.  Needs local_solve.hpp.
#include "sn_refresh.hpp"       // value refresh of a device supernodal factor: sn_refresh (behind ddm_ilu0_refresh).  Needs local_solver.hpp.
#include "geneo.hpp"            // GeneoProblem, GeneoSetup, GeneoRun, ddm_geneo_basis / ddm_msgfem_basis / ddm_svd_basis, ddm_harmonic (pulls in dense_host.hpp, geneo_blocks.hpp: GeneoWork over geneo_kernels.hpp, ddm_blockvec_*, and geneo_solver.hpp: the kept eigensolver ddm_geneo_*).  Needs csr.hpp, local_solver.hpp.
#include "halo.hpp"             // ddm_halo: single-vector and m-column exchange over one RCCL wire function.  Needs context.hpp.
#include "krylov_work.hpp"      // KrylovWork: the block Krylov drivers' work blocks, one pool per ddm_combined.  Needs device_buffer.hpp, multi_kernels.hpp.
#include "preconditioners.hpp"  // dot products, ddm_op, ddm_schwarz, ddm_galerkin, ddm_combined: single and m-column applies side by side.  Needs halo.hpp, local_solver.hpp, krylov_work.hpp.
#include "krylov_frame.hpp"     // what the drivers share: StreamDrain, the frame around a loop, MultiFrame, launch_check, defect_norm_multi, gmres_memory_check.  Needs preconditioners.hpp.
#include "krylov_cg.hpp"        // CG: begin / steps / defect / solve, m columns at once, queued (ddm_cg_solve_queue).  Needs krylov_frame.hpp.
#include "krylov_bicgstab.hpp"  // BiCGSTAB: single, queued (ddm_bicgstab_solve_queue).  Needs krylov_frame.hpp.
#include "krylov_gmres.hpp"     // restarted GMRES, left and flexible: GmresColumn, gmres_loop, gmres_loop_multi and their four exports.  Needs krylov_frame.hpp.
#include "krylov_fcg.hpp"       // flexible CG, restarted and complete: fcg_loop, fcg_loop_multi, ddm_fcg_orth_multi.  Needs krylov_frame.hpp.
#include "krylov_bcg.hpp"       // block CG (ddm_bcg_solve_multi) and its three pass exports.  Needs krylov_frame.hpp.
#include "krylov_bgmres.hpp"    // block GMRES (ddm_bgmres_solve_multi) and its three pass exports.  Needs krylov_frame.hpp.

// ---- dense host helpers exposed for the CPU tests (host logic of the GenEO Rayleigh-Ritz step) -------------------------
extern "C" int ddm_dense_sym_eig_host(int n, double *V, double *w) { return dense::sym_eig(n, V, w) ? DDM_OK : DDM_ENUMERIC; }
extern "C" int ddm_dense_rayleigh_ritz_host(int p, const double *gA, const double *gC, int keep, double tau, double *mu, double *Y)
{
  return dense::rayleigh_ritz(p, gA, gC, keep, tau, mu, Y);
}
// ... and of block CG: the pseudo-inverse of the m x m coupling matrix
extern "C" int ddm_dense_sym_pinv_host(int m, const double *W, double tol, double *Wpinv, int *rank)
{
  if (m < 1 || !W || !Wpinv || !rank || W == Wpinv || !(tol > 0.0 && tol < 1.0)) return fail(nullptr, DDM_EINVAL, "ddm_dense_sym_pinv_host: bad arguments");
  return dense::sym_pinv(m, W, tol, Wpinv, rank) ? DDM_OK : DDM_ENUMERIC;
}
// ... and of block GMRES: the factor of the p x p Gram matrix of a block (scale2 may be NULL: the diagonal of G)
extern "C" int ddm_dense_bgmres_factor_host(int p, const double *G, const double *scale2, double tol, double *S, double *C, int *rank)
{
  if (p < 1 || !G || !S || !C || !rank || S == C || G == S || G == C || !(tol > 0.0 && tol < 1.0))
    return fail(nullptr, DDM_EINVAL, "ddm_dense_bgmres_factor_host: bad arguments");
  return dense::bgmres_factor(p, G, scale2, tol, S, C, rank) ? DDM_OK : DDM_ENUMERIC;
}

// ---- input synthesis on the host (bench.py / tests: the matrices PDELab's assembler hands to the reference) ----------------------
extern "C" int ddm_synth_q1_matrix(int dim, const int64_t *bshape, const double *ke, const int64_t *eshape, const int64_t *eoff, const double *K,
                                   const uint8_t *inset, const int64_t *loc_of_box, int64_t n, const int64_t *box_index, const uint8_t *dmask,
                                   const double *diag, int64_t *indptr, int32_t *indices, double *data, int nthreads)
{
    if ((dim != 2 && dim != 3) || !bshape || !ke || !eshape || !eoff || !K || !indptr || n < 0 || (indices && !data))
        return fail(nullptr, DDM_EINVAL, "ddm_synth_q1_matrix: bad arguments");
    int64_t nbox = 1;
    for (int d = 0; d < dim; ++d) {
        if (bshape[d] < 1 || eshape[d] < 0 || eoff[d] < 0) return fail(nullptr, DDM_EINVAL, "ddm_synth_q1_matrix: bad box");
        nbox *= bshape[d];
    }
    if (nbox >= INT32_MAX || (!box_index && n != nbox)) return fail(nullptr, DDM_EINVAL, "ddm_synth_q1_matrix: box too large or row count does not match the box");
    synth::Q1Args A{dim, bshape, ke, eshape, eoff, K, inset, loc_of_box, n, box_index, dmask, diag};
    synth::q1_rows(A, indptr, indices, data, nthreads);
    return DDM_OK;
}
