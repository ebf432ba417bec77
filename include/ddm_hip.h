/* ddm_hip.h -- C ABI of the MI355X-native two-level Schwarz + GenEO hot path.
 *
 * This is the drop-in boundary: a DUNE-side adaptor (header-only classes with the reference's
 * names, see dune-ddm_amd/dune/ddm/ and INTEGRATION.md) flattens its BCRSMatrix / BlockVector /
 * Interface objects once and then only calls the entry points below.  Plain pointers and sizes,
 * no C++ or torch types.  Citations are file:line in nilsfriess/dune-ddm (the reference).
 *
 * Conventions
 *   - All arithmetic FP64; column indices int32; row pointers / sizes int64.
 *   - "rank-local" vectors are the concatenation of the rank's subdomains (one subdomain per rank
 *     in the reference; several per GPU are allowed here so that the 8-subdomain problem also
 *     runs on 1, 2 or 4 GPUs).  n_o = non-overlapping size, n = overlapping size.
 *   - Vector arguments are DEVICE pointers unless the function name ends in _host.
 *   - Every call returns 0 on success or a negative DDM_E* code; ddm_last_error() gives the text
 *     (the adaptor turns it into DUNE_THROW, cf. dune/ddm/schwarz.hh:83,91,190,193).
 *   - All work is enqueued on the context's HIP stream; calls are asynchronous unless stated.
 *   - There is NO CPU fallback: without a HIP device every compute entry point fails.
 */
#ifndef DDM_HIP_H
#define DDM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDM_OK 0
#define DDM_EINVAL (-1)   /* bad argument / size mismatch (Dune::Exception, InvalidStateException) */
#define DDM_EHIP (-2)     /* HIP runtime error */
#define DDM_ENOTIMPL (-3) /* Dune::NotImplemented */
#define DDM_ENUMERIC (-4) /* zero pivot, singular coarse matrix, eigensolver failure */
#define DDM_ECOMM (-5)    /* exchange callback failed (MPI_Abort in the reference) */

typedef struct ddm_ctx ddm_ctx;
typedef struct ddm_csr ddm_csr;
typedef struct ddm_ilu0 ddm_ilu0;
typedef struct ddm_halo ddm_halo;
typedef struct ddm_op ddm_op;
typedef struct ddm_schwarz ddm_schwarz;
typedef struct ddm_galerkin ddm_galerkin;
typedef struct ddm_combined ddm_combined;

/* ---- context ---------------------------------------------------------------------------- */
/* One context per process/GPU.  stream == NULL: the library creates its own stream. */
int ddm_ctx_create(int device, void *hip_stream, ddm_ctx **out);
void ddm_ctx_destroy(ddm_ctx *ctx);
const char *ddm_last_error(const ddm_ctx *ctx); /* ctx == NULL: the calling thread's last failure of a context-free entry point */
int ddm_ctx_sync(ddm_ctx *ctx); /* hipStreamSynchronize */
/* the host waits for the work enqueued on the context's stream so far (event record + wait; later work is not waited for):
 * what an exchange callback of a host-driven transport (MPI) calls before it touches the packed send buffer */
int ddm_ctx_fence(ddm_ctx *ctx);
void *ddm_ctx_stream(ddm_ctx *ctx);

/* Inter-rank exchange is delegated to the host program (MPI in a DUNE build, torch.distributed
 * over RCCL in bench.py).  Both callbacks are invoked with the data already produced on the
 * context's stream; they must enqueue on (or synchronise with) that stream.
 *   alltoall: send/recv buffers are device pointers with the per-peer layout fixed at
 *             ddm_halo_create time; `tag` is the halo's id.
 *   allreduce_sum: in-place sum over all ranks of n doubles at a device pointer.
 * With no callbacks installed the context is single-rank (all subdomains local). */
typedef int (*ddm_alltoall_fn)(void *user, int tag, const double *sendbuf, double *recvbuf);
typedef int (*ddm_allreduce_fn)(void *user, double *buf, int64_t n);
int ddm_ctx_set_comm(ddm_ctx *ctx, int rank, int nranks, ddm_alltoall_fn a2a, ddm_allreduce_fn allreduce, void *user);

/* The same exchange INSIDE the library over RCCL (xGMI): grouped ncclSend / ncclRecv per halo and ncclAllReduce for the dots and the
 * coarse defect, all enqueued on the context's stream -- no callback round trip through the host program.  librccl is opened with
 * dlopen (a copy the host program already loaded is reused).  ddm_rccl_unique_id fills 128 bytes on ONE rank; the host program
 * distributes them (MPI_Bcast / torch.distributed.broadcast) and every rank calls ddm_ctx_set_rccl (collective: ncclCommInitRank).
 * self_test != 0: also route the rank's own halo segment and all reductions through RCCL (exercises the path on a single GPU). */
int ddm_rccl_unique_id(void *id128);
int ddm_ctx_set_rccl(ddm_ctx *ctx, int rank, int nranks, const void *id128, int self_test);
/* *count = number of ranks RCCL itself reports for the context's communicator (ncclCommCount), 0 without ddm_ctx_set_rccl:
 * lets a launcher check that the exchange really spans the ranks it started (bench.py prints it next to n_gpus). */
int ddm_ctx_rccl_size(ddm_ctx *ctx, int *count);
/* counts[3] = {all-reduces, doubles they carried, grouped halo exchanges} issued through this context so far, counted as a run over
 * several ranks launches them (one all-reduce / one send-receive group = one RCCL launch), also on a single rank where nothing is
 * sent: lets a benchmark report collectives per iteration.  In ddm_cg_steps the squared defect norm of an iteration rides on the
 * coarse-defect all-reduce of the next one (K + 1 doubles, galerkin_preconditioner.hh:170-183): per CG iteration 3 all-reduces
 * (<p, q>, <r, z>, coarse defect + norm) and 3 halo groups instead of 4 + 3. */
int ddm_ctx_comm_counts(ddm_ctx *ctx, int64_t *counts);

/* raw device memory helpers for callers that do not bring their own allocator */
int ddm_malloc(ddm_ctx *ctx, int64_t bytes, void **dptr);
int ddm_free(ddm_ctx *ctx, void *dptr);
int ddm_memset_zero(ddm_ctx *ctx, void *dptr, int64_t bytes);                 /* enqueued on the context's stream */
int ddm_memcpy_h2d(ddm_ctx *ctx, void *dst, const void *src, int64_t bytes); /* synchronous */
int ddm_memcpy_d2h(ddm_ctx *ctx, void *dst, const void *src, int64_t bytes); /* synchronous */

/* ---- CSR matrix (flattened Dune::BCRSMatrix<FieldMatrix<double,1,1>>; cf. the in-tree
 *      precedent dune/ddm/strumpack.hh:36-62) ---------------------------------------------- */
int ddm_csr_create(ddm_ctx *ctx, int64_t nrows, int64_t ncols, const int64_t *rowptr, const int32_t *col,
                   const double *val, ddm_csr **out);
/* The same object without device arrays, for matrices the library only reads on the host: A_neu / B_neu of ddm_geneo_basis (the
 * pencil A_neu + sigma D B D is assembled from the host arrays; at 216^3 the two device copies were 7 GB and 0.6 s for nothing).
 * Entry points that need the device arrays (products, factorisations) return DDM_EINVAL for it. */
int ddm_csr_create_host(ddm_ctx *ctx, int64_t nrows, int64_t ncols, const int64_t *rowptr, const int32_t *col, const double *val, ddm_csr **out); /* host arrays are copied */
/* New values in the pattern of A (nnz doubles, copied): the host copy and, unless A came from ddm_csr_create_host, the device
 * values on the context's stream.  Objects built on A keep what they made of the old values until they are refreshed
 * (ddm_op_refresh, ddm_ilu0_refresh, ddm_schwarz_refresh).  Synchronous. */
int ddm_csr_set_values(ddm_ctx *ctx, ddm_csr *A, const double *val_host);
void ddm_csr_destroy(ddm_csr *A);
int64_t ddm_csr_rows(const ddm_csr *A);
int64_t ddm_csr_nnz(const ddm_csr *A);
/* y = A x  (BCRSMatrix::mv, dune/ddm/nonoverlapping_operator.hh:37) */
int ddm_csr_mv(ddm_ctx *ctx, const ddm_csr *A, const double *x, double *y);
/* y += alpha A x  (BCRSMatrix::usmv, nonoverlapping_operator.hh:47) */
int ddm_csr_usmv(ddm_ctx *ctx, const ddm_csr *A, double alpha, const double *x, double *y);

/* Y = A X for row-major n x nrhs block vectors (the B*x / A*x products of the GenEO eigensolver,
 * eigensolvers/spectra.hh:100-105, on a block of vectors) */
int ddm_csr_mm(ddm_ctx *ctx, const ddm_csr *A, int nrhs, const double *X, double *Y);

/* Host-only (no device): the cache-blocked processing order the library uses for the block products A~ X, C~ X of the GenEO
 * eigensolver when the diagonal blocks of the matrix come from a structured grid in lexicographic numbering (strides read off the
 * column offsets most rows share; 16 x 4 x 4 bricks).  order_out[n] is always a permutation of the rows; returns 1 when a grid
 * structure was found, 0 when not (identity), < 0 on bad arguments.  A performance hint only: every row is computed as before. */
int ddm_csr_row_order_tiled_host(int64_t nblocks, const int64_t *block_ptr, const int64_t *rowptr, const int32_t *col, int32_t *order_out);
/* Host only (no device needed; for tests): the diagonal-row-block layout that ddm_op_create builds of its matrix (blocks of at most 256
 * consecutive rows on at most 32 diagonals col - row: offset table, one value slab per diagonal, a presence mask per row; rows that fit
 * none stay CSR-stream blocks; consecutive blocks with one table form a segment, which keeps only the slabs of the offsets >= 0 when
 * it is symmetric bit for bit), built for the square matrix given and applied to x on the host with the indexing of the device kernel.
 * kinds_out (may be NULL) receives (first row, end row, diagonals; 0 = CSR-stream, slabs stored) of the first max_blocks blocks;
 * counts_out[7] = {blocks, diagonal blocks, CSR-stream blocks, rows in diagonal blocks, value slots, segments, symmetric segments}. */
int ddm_dia_build_and_apply_host(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, const double *x, double *y,
                                 int64_t max_blocks, int32_t *kinds_out, int64_t *counts_out);
/* Host only (for tests): the x windows of the same layout.  The ascending offsets of a segment form runs (an offset joins the run of
 * the one before when they are at most 256 apart); a block reads one window of 256 + (last - first offset) consecutive doubles of x
 * per run, and a segment whose windows fit the capacity is staged: its blocks load the windows into LDS once (none is with
 * DDM_SPMV_STAGE_X=0 in the environment, which ddm_op_create reads as well).  segs_out: (staged, runs, window doubles, place of the
 * first run in runs_out) of the first max_segments segments; runs_out: (first offset, doubles, window position) of the first max_runs
 * runs, segment after segment; counts_out[4] = {segments, runs, capacity in doubles, rows of a full block}. */
int ddm_dia_windows_host(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int64_t max_segments, int32_t *segs_out,
                         int64_t max_runs, int32_t *runs_out, int64_t *counts_out);
/* Host only (for tests): the coded blocks of the same layout.  A block of a staged segment whose rows read at most 16 distinct
 * values (compared bit for bit) keeps them in a dictionary of 16 doubles, in order of first appearance and padded with +0.0, and
 * a 128-bit word of 4-bit codes per row, nibble k for diagonal k of the segment's table; a segment whose blocks are all coded
 * builds no value slabs (no block is coded with DDM_SPMV_CODE=0 in the environment, which ddm_op_create reads as well).  The
 * layout is built on `threads` host workers (0: the library's own number) and does not depend on them.  blocks_out (may be
 * NULL): (number of the block's dictionary or -1, dictionary entries in use, 1 when the block's segment has slabs) of the first
 * max_blocks blocks; dict_out (may be NULL): the 16 doubles of every dictionary whose number is below max_blocks, one after the
 * other; code_out (may be NULL): 4 words per row, 0 for the rows of blocks that are not coded; counts_out[5] = {blocks, coded
 * blocks, value slots of the slabs that were built, entries of a dictionary, words per row}.  The "value slots" that
 * ddm_dia_build_and_apply_host reports stay those of the slab layout, coded or not. */
int ddm_dia_codes_host(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int threads, int64_t max_blocks,
                       int32_t *blocks_out, double *dict_out, uint32_t *code_out, int64_t *counts_out);

/* ---- local subdomain solver: ILU(0), natural row order ------------------------------------
 * The InverseOperator behind schwarz.hh:57,92,133 for [subdomain_solver] type=loopsolver maxit=1,
 * preconditioner type=ilu n=0.  block_ptr[0..nblocks] = row ranges of the independent diagonal
 * blocks (subdomains) of A; pass nblocks=1, block_ptr={0,n} for one subdomain. */
int ddm_ilu0_create(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, ddm_ilu0 **out);
void ddm_ilu0_destroy(ddm_ilu0 *F);
/* Refactorises from the CURRENT values of the matrix the factor was created on (ddm_csr_set_values; A outlives the factor): the
 * numeric ILU(0) runs on the device along the factor's own L level schedule, then the new factor is scattered into the engines'
 * layouts.  Same pattern, same blocks, same schedules.  Afterwards every solve and ddm_ilu0_get_factors_host give bit for bit what
 * a factor created on the new values gives.  The level and pipe engines are rewritten in place (their buffers keep their addresses,
 * so solves captured before the refresh stay valid); a built xcd2 part is dropped and rebuilt by the next solve.
 * DDM_ENOTIMPL (nothing touched) for the HOST-engine sparse direct factor and for the box engine: create a new factor.
 * DDM_ENUMERIC for a zero or non-finite pivot (the message names the block, as at creation): the factor still is the previous one.
 * A DEVICE supernodal direct factor (ddm_ilu0_engine == 16) is refreshed too: the numeric factorisation runs again on the kept
 * supernodes, colours and solve plans, the refinement steps are decided again by the probe of the creation; its captured solves are
 * dropped and captured again by the next solve.  Its panels are overwritten in place, so a failure leaves NO factor: the object is
 * invalid and every solve through it (ddm_ilu0_solve*, the Schwarz applies) returns DDM_ENUMERIC ("the factor is invalid after a
 * failed refresh") until a later refresh succeeds.  Return codes as a creation on the same values: DDM_ENUMERIC where it fails (not
 * positive definite; with DDM_DIRECT_ENGINE=device also a vanishing pivot column or a probe above 1e-9), DDM_ENOTIMPL ("create a new
 * factor") where an unforced creation hands the matrix to the host engine.  See the sparse direct block below.
 * Synchronous; not to be called while the context's stream is being captured. */
int ddm_ilu0_refresh(ddm_ctx *ctx, ddm_ilu0 *F);
/* successful in-place refreshes of F since its creation, for every kind of factor: 0 after creation, unchanged by a failed or
 * refused ddm_ilu0_refresh -- tells "refreshed" from "built anew".  NULL: 0. */
int ddm_ilu0_refresh_count(const ddm_ilu0 *F);
/* x = (LU)^-1 d ; d and x must not alias */
int ddm_ilu0_solve(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x);
/* x = ((LU)^-1 d) * scale + add, entry by entry with two roundings; scale and add are device vectors of n doubles, either may be
 * NULL.  The tail of a Schwarz level (partition of unity, coarse correction) as the applies enqueue it: folded into the output pass
 * by the pipe and box engines, two more kernels on the others.  d and x must not alias. */
int ddm_ilu0_solve_tail(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, const double *scale, const double *add);
/* X = (LU)^-1 D for row-major n x nrhs block vectors (cf. the reference's multi-RHS triangular
 * solve eigensolvers/umfpack.hh:131-197); D and X must not alias */
int ddm_ilu0_solve_multi(ddm_ctx *ctx, ddm_ilu0 *F, int nrhs, const double *D, double *X);
/* the same with SINGLE-PRECISION sweeps (factor entries and the work block in float; D is read and X written in double): preconditioner
 * grade, relative error ~1e-6 x the growth of the triangular solves -- what the GenEO block iteration applies as W = T r (its eigenpairs
 * and residuals are computed in double).  nrhs % 4 != 0 or a sparse direct factor: the double sweeps. */
int ddm_ilu0_solve_multi_f32(ddm_ctx *ctx, ddm_ilu0 *F, int nrhs, const double *D, double *X);
int64_t ddm_ilu0_num_levels(const ddm_ilu0 *F, int upper);
/* status of the persistent (single-launch) triangular solve: 0 ok, 1 = a wave timed out waiting for a
 * dependency level (results invalid).  Synchronous.  DDM_TRSV_MODE=levels selects one launch per level. */
int ddm_ilu0_status(ddm_ctx *ctx, const ddm_ilu0 *F, int *status);
/* The same status word WITHOUT synchronising (it lives in pinned host memory the kernel writes to): non-zero as soon as a solve
 * that has finished gave up.  ddm_schwarz_apply / ddm_combined_apply (and with them the Krylov drivers) look at it on entry and
 * return DDM_ENUMERIC -- a time-out surfaces at the NEXT apply, not only in post().
 * Co-residency: the single-launch engines (`pipe`, `xcd2`) spin-wait on other workgroups of the same launch, so all their
 * workgroups (2 per CU) must be resident at once: ONE process per GPU, no other kernel holding CUs for the duration of a solve.
 * Every spin is bounded (it ends with the status word set, never in a hang); DDM_TRSV_MODE=levels (one launch per dependency
 * level, no spinning) is the engine for a GPU that is shared with other processes. */
int ddm_ilu0_peek_status(const ddm_ilu0 *F);
/* diagnostic: overwrite that status word (0 clears it), so that a caller can exercise the fail-fast path of the applies */
int ddm_ilu0_set_status(ddm_ilu0 *F, int status);
/* Engine of the BLOCK solves (ddm_ilu0_solve_multi*, and with them every block apply and the GenEO / harmonic-extension setup) of a plain
 * ILU(0) factor: mode 0 = levels (one launch per dependency level and sweep; the default), 1 = xcd (both sweeps of all diagonal blocks
 * in ONE persistent launch: teams of XCDs take the blocks in turn, a flag barrier separates the levels; the results are the bits of
 * mode 0), 2 = xcd with all workgroups in one team (the path taken when an XCD received no workgroup; for tests).  Other values:
 * DDM_EINVAL.  A direct factor: DDM_OK, no effect.  A factor with a level of 96 or more entries per row keeps the level launches
 * (ddm_ilu0_multi_info says so).  DDM_TRSV_MULTI_MODE=levels|xcd, read when a factor is created, sets the initial mode -- also of the
 * factors the GenEO and harmonic-extension setups create internally.  The co-residency rule of ddm_ilu0_peek_status holds for mode
 * 1 and 2 (one workgroup per CU); a time-out leaves 12 (grid barrier), 13 (level barrier) or 14 in the status word. */
int ddm_ilu0_set_multi_engine(ddm_ctx *ctx, ddm_ilu0 *F, int mode);
/* What the block solves of F run on.  *count = 14 values; out (capacity cap >= 14, or NULL to query the count): [0] requested mode,
 * [1] engine of the last block solve (-1 none yet, 0 levels, 1 xcd), [2] why xcd did not run (0 it ran, 1 not requested, 2 direct
 * factor, 3 a level of w >= 96), and of the last xcd launch [3] workgroups, [4] teams, [5] 1 if all workgroups formed one team,
 * [6..13] workgroups per XCD.  [4..13] are written by the kernel: synchronise first. */
int ddm_ilu0_multi_info(const ddm_ilu0 *F, int64_t *out, int64_t cap, int64_t *count);
/* Host only (tests): the plan of mode xcd for one triangle (upper = 0 / 1) of a CSR pattern with sorted rows and a full diagonal, as the
 * factor computes it: *nlev dependency levels; off[l (nblocks + 1) + b] = first position of diagonal block b among the ascending rows
 * of level l (off[l (nblocks + 1) + nblocks] = rows of the level); blk_nlev[b] = levels of block b.  off == NULL: only *nlev; otherwise
 * cap >= *nlev (nblocks + 1).  DDM_EINVAL for a malformed pattern. */
int ddm_trsv_multi_plan_host(int64_t n, const int64_t *rp, const int32_t *ci, int64_t nblocks, const int64_t *block_ptr, int upper, int32_t *off, int64_t cap,
                             int32_t *blk_nlev, int64_t *nlev);
/* Host only (tests): the team arithmetic of mode xcd for the workgroup that drew xcd_ticket on XCD xcc and global_ticket overall, from
 * the workgroups per XCD tickets8: out5 = {teams T = min(nblocks, 8), team = xcc % T, rank within the team, workgroups of the team,
 * 0}, or {1, 0, global_ticket, grid, 1} when a team would be empty or force_one is set. */
int ddm_trsv_multi_team_host(const uint32_t *tickets8, int nblocks, int force_one, int xcc, uint32_t xcd_ticket, uint32_t global_ticket, uint32_t grid, int32_t *out5);
/* engine the next ddm_ilu0_solve uses: 8 = pipe, 4 = xcd2 (also when pipe declined the matrix), 0 = one launch per level (also the
 * host sparse direct factor), 16 = device supernodal factor, 32 = box (DDM_TRSV_MODE=box; pipe when box declined the matrix) */
int ddm_ilu0_engine(const ddm_ilu0 *F);
/* ddm_ilu0_create returns while the schedule of the single-launch engine is still being built on host threads (2.6 s at 216^3; the
 * first ddm_ilu0_solve waits for it, so does ddm_ilu0_engine).  ddm_ilu0_wait joins that work now and returns its error, so that a
 * caller can account the whole setup before it starts its clock.  DDM_PIPE_ASYNC=0: everything inside ddm_ilu0_create.  The matrix
 * handed to ddm_ilu0_create must stay alive as long as the factor (it always had to: the factor borrows its pattern). */
int ddm_ilu0_wait(ddm_ctx *ctx, ddm_ilu0 *F);
/* Diagnostic of the box engine (structured blocks; csrc/trsv_box.hpp): with DDM_BOX_CHECK=1 in the environment at creation its sweep
 * kernels stamp every plane of block 0; out1024 = [2 sweeps][128 planes][4] = {start, end (100 MHz clock), polls of the previous plane's
 * progress word, XCC id} of the last solve (zeros without the switch). */
int ddm_ilu0_box_check(const ddm_ilu0 *F, unsigned long long *out1024);
/* Read-only, for tests: what the box engine's builder made of the matrix.  out = {blocks, workgroups of a sweep launch, engine of the
 * nested factor that solves the rows behind the boxes (the codes of ddm_ilu0_engine, settled; -1 when there are no such rows)}, then
 * per block {nx, ny, nz, steps per plane, rows behind the box}.  *count = 3 + 5 blocks is always set; out may be NULL to ask for it,
 * otherwise capacity >= *count.  A factor that is not on the box engine reports 0 blocks.  Waits for the background builder. */
int ddm_ilu0_box_info(const ddm_ilu0 *F, int64_t *out, int64_t capacity, int64_t *count);
/* diagnostic: one solve with in-kernel cycle stamps of one compute wave */
int ddm_ilu0_debug_stamps(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, unsigned long long *out6_host);
/* diagnostic: one solve with the stamped build of the pipe engine's kernel (DDM_TRSV_MODE=pipe, the default); per task 272
 * words, the first 16: start / first step / end (100 MHz ticks), cycles waiting for tiles / for producer tasks, an unused word (0),
 * steps, XCC id, segment sums of the compute wave's step (layout: csrc/trsv_pipe.hpp, STAMP), then the time of each of the first 256
 * steps' result stores; meta_host (optional) receives group and
 * sweep per task.  out_host == NULL queries *ntasks. */
int ddm_ilu0_pipe_trace(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, unsigned long long *out_host, int32_t *meta_host,
                        int64_t capacity_tasks, int64_t *ntasks);
/* diagnostic of the pipe engine's queue order (csrc/trsv_pipe_host.hpp, "Queue order"): out = {workgroups of the launch, spread mode,
 * most tasks a queue may hold in front of producers (0: creation order), tasks moved in the forward sweeps, in the backward sweeps,
 * most in one queue, gap in levels, tasks}, then per task {start level, moved}.  *count = 8 + 2 tasks is always set; out may be NULL to
 * ask for it, otherwise capacity >= *count.  A factor that is not on the pipe engine reports 0 tasks.  Waits for the background builder. */
int ddm_ilu0_pipe_info(ddm_ctx *ctx, ddm_ilu0 *F, int64_t *out, int64_t capacity, int64_t *count);
/* factor values in the pattern of A (inverse pivots on the diagonal), for parity tests */
int ddm_ilu0_get_factors_host(ddm_ctx *ctx, const ddm_ilu0 *F, double *lu_host);

/* ---- sparse direct local solver -------------------------------------------------------------
 * What the reference gets from SuiteSparse through the solver factory: [subdomain_solver] type = cholmod / umfpack
 * (schwarz.hh:85-92, examples/poisson.ini:23,26) and the factorisation of A - sigma B inside the GenEO eigensolver
 * (eigensolvers/spectra.hh:28-89).  Sparse Cholesky of a symmetric positive definite block-diagonal matrix: nested-dissection
 * ordering, symbolic analysis and numeric factorisation on host threads (setup work, one thread per block, like the ILU(0)
 * factorisation); the factor is handed to the same device triangular-solve engines as an ILU(0) factor (the returned object IS a
 * ddm_ilu0: ddm_ilu0_solve / _solve_multi / _destroy apply), solves run in the fill-reducing order with a permutation on either side.
 * max_flops > 0: analyse first and return DDM_ENOTIMPL without factorising if the factorisation needs more floating-point
 * operations (sum of squared column counts) -- the caller then stays with ILU(0).  DDM_ENUMERIC: not positive definite. */
int ddm_chol_create(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, double max_flops, ddm_ilu0 **out);
/* general != 0: L U on the pattern of A + A^T, for non-symmetric matrices (the DG convection-diffusion operator; `type = umfpack`):
 * the host engine eliminates WITHOUT pivoting (matrices whose symmetric part is positive definite; DDM_ENUMERIC on a vanishing
 * pivot), the device engine with threshold partial pivoting inside the diagonal block of a supernode (below).  general == 0 =
 * ddm_chol_create. */
int ddm_direct_create(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, int general, double max_flops, ddm_ilu0 **out);
/* Engines of ddm_chol_create / ddm_direct_create, environment DDM_DIRECT_ENGINE = device | host.  Default: the device engine when the
 * factorisation needs at least DDM_DIRECT_DEVICE_MIN_FLOPS multiply-adds -- 2e10 for ddm_direct_create / the Schwarz local solver
 * (the host engine's CSR level solves are the faster single-vector solves, 1.31 against 1.75 ms on configs[4], but its factorisation
 * takes ~1 s per 1e10 multiply-adds: above 2e10 the device engine wins the time to solution), 1e10 for the factors the library
 * builds for a handful of block solves (GenEO preconditioner, harmonic extensions):
 *   device  SUPERNODAL Cholesky (general = 0) or L U (general = 1) with numeric factorisation AND solves on the GPU (csrc/sn_chol.hpp):
 *           nested-dissection supernodes of at most 128 columns, dense panels, FP64-MFMA updates, level by level of the supernodal
 *           elimination tree; the host only orders and analyses.  L U: threshold partial pivoting (0.1, UMFPACK's default) INSIDE the
 *           diagonal block of a supernode; rows are never exchanged between supernodes; a pivot column that vanishes inside its block
 *           is replaced by sqrt(eps) max|a_ij| (static perturbation).  ITERATIVE REFINEMENT as dune/ddm/eigensolvers/umfpack.hh:42-129
 *           (and as UMFPACK's own solve): backward error omega = ||b - A x|| / (||A||_inf ||x|| + ||b||), stop below 1e-14 or when a
 *           step does not halve it, at most 3 steps -- decided ONCE per factor on a probe right-hand side (the solves stay captured HIP
 *           graphs), then applied in every single- and multi-vector solve (ddm_ilu0_refinement reports it; DDM_DIRECT_REFINE = off |
 *           <steps> overrides).  A factor whose probe stays above 1e-9 is refused (DDM_ENUMERIC when the engine was forced, else the
 *           host engine takes over).  Results are bitwise REPRODUCIBLE since round 4: supernodes of one tree level whose updates would
 *           meet in an ancestor entry are coloured apart and the colours run one after the other; the forward sweeps write into one
 *           slot per (supernode, row) and the row's owner adds its slots in a fixed order -- no atomics anywhere.  DDM_ENOTIMPL if the
 *           panels do not fit into the free device memory.
 *   host    up-looking factorisation on host threads (L U without pivoting for general = 1), CSR level solves on the device
 *           (bitwise reproducible).
 * New values in the old pattern (ddm_csr_set_values + ddm_ilu0_refresh / ddm_schwarz_refresh): the DEVICE engine's factor is
 * refreshed in place -- ordering, analysis, colours, plans and uploads are kept, sn::factorize and the refinement probe run again,
 * bit for bit a factor created on the new values; the matrix must outlive the factor (it is read again).  No second panel array
 * is held: a failed refresh leaves the factor INVALID (see ddm_ilu0_refresh).  The HOST engine's factor is refused (DDM_ENOTIMPL).
 * The host half of the device engine alone (no device needed; CPU tests): */
typedef struct ddm_sn_host ddm_sn_host;
int ddm_sn_host_create(int64_t n, const int64_t *rowptr, const int32_t *col, int64_t nblocks, const int64_t *block_ptr, ddm_sn_host **out);
void ddm_sn_host_destroy(ddm_sn_host *H);
/* sizes[4] = {supernodes, length of `rows`, panel entries (doubles), tree levels} of one block; *flops = multiply-adds */
int ddm_sn_host_sizes(const ddm_sn_host *H, int64_t block, int64_t *sizes, double *flops);
/* perm[n_b] (perm[new] = old, block-local), first[nsn + 1], rptr[nsn + 1], rows[], parent[nsn], level[nsn]; any pointer may be NULL */
int ddm_sn_host_get(const ddm_sn_host *H, int64_t block, int32_t *perm, int32_t *first, int64_t *rptr, int32_t *rows, int32_t *parent, int32_t *level);
int ddm_ilu0_is_direct(const ddm_ilu0 *F); /* 1 for a ddm_chol_create / ddm_direct_create factor */
int64_t ddm_ilu0_nnz(const ddm_ilu0 *F);   /* stored factor entries (L + D + U) */
/* iterative refinement of a device factor: returns the steps every solve performs; omega[5] (may be NULL) = backward error of the probe
 * right-hand side after 0, 1, .. steps (0 where not run) */
int ddm_ilu0_refinement(const ddm_ilu0 *F, double *omega);
/* read-only, for tests: the row order the threshold pivoting of a DEVICE L U factor chose, copied to the host after a
 * synchronisation of the context's stream.  out_n[n] in the permuted numbering: entry first[s] + k is the row of the diagonal block
 * of supernode s (block-local, before pivoting) that ended in position k; the identity where no row was exchanged.  DDM_EINVAL for
 * any other factor (ILU(0), the host engine, the device Cholesky). */
int ddm_ilu0_sn_pivots(ddm_ctx *ctx, const ddm_ilu0 *F, int32_t *out_n);
/* The host part alone (no device needed; used by the CPU tests): va == NULL stops after the symbolic analysis.
 * get: perm[n] (perm[new] = old), and the factor in the storage convention of ddm_ilu0_get_factors_host -- CSR over the
 * PERMUTED indices with pattern L + D + L^T: unit lower factor, inverse pivots on the diagonal, D L^T above. */
typedef struct ddm_chol_host ddm_chol_host;
int ddm_chol_host_create(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int64_t nblocks,
                         const int64_t *block_ptr, ddm_chol_host **out);
int ddm_direct_host_create(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int64_t nblocks,
                           const int64_t *block_ptr, int general, ddm_chol_host **out);
void ddm_chol_host_destroy(ddm_chol_host *H);
int64_t ddm_chol_host_nnz(const ddm_chol_host *H);        /* entries of the factor CSR (0 after a symbolic-only run) */
int64_t ddm_chol_host_nnz_factor(const ddm_chol_host *H); /* nnz(L) from the symbolic analysis */
double ddm_chol_host_flops(const ddm_chol_host *H);       /* sum of squared column counts */
int ddm_chol_host_get(const ddm_chol_host *H, int32_t *perm, int64_t *rowptr, int32_t *col, double *lu);

/* ---- halo exchange plan: one per DUNE interface -------------------------------------------
 * (copyOwnerToAll: schwarz.hh:125, galerkin_preconditioner.hh:162;
 *  addOwnerCopyToOwnerCopy: nonoverlapping_operator.hh:38,48, schwarz.hh:138,142;
 *  addOwnerCopyToAll: galerkin_preconditioner.hh:190.)
 * send side : sendbuf[k] = v[send_idx[k]], k < nsend, grouped by destination rank
 *             (send_counts[nranks]); the segment for this rank itself is delivered locally.
 * recv side : recvbuf is the concatenation of the peers' segments (recv_counts[nranks]).
 *             For entry t < ndst:  v[dst_idx[t]] (=|+=) sum_{k=dst_ptr[t]}^{dst_ptr[t+1]-1} recvbuf[src_pos[k]]
 *             contributions are added in list order (the adaptor lists them by ascending source
 *             rank, which is the order DUNE's BufferedCommunicator scatters them).
 * mode      : 0 = copy (overwrite), 1 = add. */
int ddm_halo_create(ddm_ctx *ctx, int tag, int mode, int64_t nsend, const int64_t *send_idx,
                    const int64_t *send_counts, const int64_t *recv_counts, int64_t ndst, const int64_t *dst_idx,
                    const int64_t *dst_ptr, const int64_t *src_pos, ddm_halo **out);
void ddm_halo_destroy(ddm_halo *H);
int ddm_halo_exchange(ddm_ctx *ctx, ddm_halo *H, double *v); /* pack -> (callback) -> unpack, in place */
/* pack from src, unpack into dst (entries of dst outside dst_idx are left alone).  With a copy-mode halo that carries ONE
 * neighbour's index lists and dst zeroed beforehand this is CopyGatherScatterWithRank (galerkin_preconditioner.hh:66-103): the
 * neighbour's vector restricted to the shared indices, zero elsewhere -- no mask, no host round trip. */
int ddm_halo_exchange_to(ddm_ctx *ctx, ddm_halo *H, const double *src, double *dst);
/* Buffers the alltoall callback is handed (device pointers; stable for the halo's lifetime). */
double *ddm_halo_sendbuf(ddm_halo *H);
double *ddm_halo_recvbuf(ddm_halo *H);

/* ---- NonOverlappingOperator + NonOverlappingScalarProduct (nonoverlapping_operator.hh) ---- */
int ddm_op_create(ddm_ctx *ctx, const ddm_csr *A, ddm_halo *novlp_add, const uint8_t *owner_mask_host, ddm_op **out);
/* the operator's diagonal-block storage again from A's current values (ddm_csr_set_values): what ddm_op_create builds on them */
int ddm_op_refresh(ddm_ctx *ctx, ddm_op *op);
void ddm_op_destroy(ddm_op *op);
int ddm_op_apply(ddm_ctx *ctx, ddm_op *op, const double *x, double *y);                       /* :34-39 */
int ddm_op_applyscaleadd(ddm_ctx *ctx, ddm_op *op, double alpha, const double *x, double *y); /* :41-50 */
int ddm_dot(ddm_ctx *ctx, ddm_op *op, const double *x, const double *y, double *result_host); /* :76-81, synchronous */
int ddm_norm(ddm_ctx *ctx, ddm_op *op, const double *x, double *result_host);                 /* :83, synchronous */

/* ---- SchwarzPreconditioner (schwarz.hh:54-220) --------------------------------------------
 * type: 0 = standard, 1 = restricted (schwarz.hh:80-83).  pou may be NULL (schwarz.hh:140).
 * ext_map[n]  : index into the non-overlapping vector or -1  ("extend": schwarz.hh:121-122)
 * A_dir is only read during creation (factorisation) and by ddm_schwarz_refresh. */
int ddm_schwarz_create(ddm_ctx *ctx, const ddm_csr *A_dir, int64_t nblocks, const int64_t *block_ptr, int64_t n_novlp,
                       const int32_t *ext_map_host, const double *pou_host, int type, ddm_halo *ovlp_copy,
                       ddm_halo *ovlp_add, ddm_schwarz **out);
/* the same with the `type` key of [schwarz.subdomain_solver] (schwarz.hh:85-92): "ilu0" (default of ddm_schwarz_create) or
 * "cholmod" / "ldl" = this library's sparse Cholesky (SPD input; DDM_ENUMERIC otherwise), "umfpack" = its L U without pivoting,
 * "direct" = Cholesky if the values are symmetric, else L U */
int ddm_schwarz_create_ex(ddm_ctx *ctx, const ddm_csr *A_dir, int64_t nblocks, const int64_t *block_ptr, int64_t n_novlp,
                          const int32_t *ext_map_host, const double *pou_host, int type, const char *subdomain_solver,
                          ddm_halo *ovlp_copy, ddm_halo *ovlp_add, ddm_schwarz **out);
/* the local solver again from A_dir's current values: ddm_ilu0_refresh on it, with its return codes.  ILU(0) and the device
 * supernodal direct factor are refreshed in place; DDM_ENOTIMPL for the host-engine direct factor, for the box engine and for a
 * device factor whose new values an unforced creation would hand to the host engine: create a new level.  After a failed refresh
 * of a device direct factor the applies return DDM_ENUMERIC until a refresh succeeds (or the level is created anew). */
int ddm_schwarz_refresh(ddm_ctx *ctx, ddm_schwarz *S);
void ddm_schwarz_destroy(ddm_schwarz *S);
int ddm_schwarz_apply(ddm_ctx *ctx, ddm_schwarz *S, double *x, const double *d); /* :115-149 */
int64_t ddm_schwarz_num_levels(const ddm_schwarz *S, int upper); /* dependency levels of the local L / U solve */
int64_t ddm_schwarz_factor_nnz(const ddm_schwarz *S); /* stored entries of the local solver's factor (ILU(0): nnz(A_dir); direct: nnz(L + U)) */
int ddm_schwarz_engine(const ddm_schwarz *S);                    /* ddm_ilu0_engine of the local solver */
/* Synchronous: DDM_OK, or DDM_ENUMERIC if a local solve since creation gave up waiting (results invalid).  apply has no
 * error return in the reference (schwarz.hh:131 discards the InverseOperatorResult); adaptors call this in post(). */
int ddm_schwarz_status(ddm_ctx *ctx, const ddm_schwarz *S);
/* the local solver object behind `solver->apply` (schwarz.hh:57,133; returned by SchwarzPreconditioner::getSolver(), :155):
 * borrowed, owned by S; ddm_ilu0_solve / _solve_multi / _status apply */
ddm_ilu0 *ddm_schwarz_local_solver(ddm_schwarz *S);

/* ---- GalerkinPreconditioner (galerkin_preconditioner.hh:40-363) ---------------------------
 * basis_host: kmax x n row-major (vector j contiguous), zero rows where a subdomain has fewer
 * vectors; sub_ptr[nsub+1]: overlapping row ranges of the rank's subdomains; coarse_index[nsub*kmax]:
 * global coarse row of (subdomain, vector) or -1; K = total coarse dimension;
 * a0inv_host: K x K row-major inverse of the coarse matrix R A R^T (every rank solves the
 * replicated coarse problem instead of the rank-0 gather/solve/scatter of :170-183).
 * Shares the ext_map / halos of the Schwarz object. */
int ddm_galerkin_create(ddm_ctx *ctx, int64_t n, int64_t n_novlp, const int32_t *ext_map_host, int64_t nsub,
                        const int64_t *sub_ptr, int64_t kmax, const double *basis_host, const int64_t *coarse_index,
                        int64_t K, const double *a0inv_host, ddm_halo *ovlp_copy, ddm_halo *ovlp_add,
                        ddm_galerkin **out);
/* a new inverse of the coarse matrix (K x K doubles, row-major) into the buffer the applies read; basis and layout stay */
int ddm_galerkin_set_inverse(ddm_ctx *ctx, ddm_galerkin *G, const double *a0inv_host);
void ddm_galerkin_destroy(ddm_galerkin *G);
int ddm_galerkin_apply(ddm_ctx *ctx, ddm_galerkin *G, double *x, const double *d); /* :151-194 */
/* Local slab of the Galerkin product (build_solver, :219-349; layout helpers.hh:252):
 * Y = A_dir * V for nvec device vectors V (nvec x n row-major) then out[i*nvec_r + j] = <R_i, Y_j>
 * restricted to the subdomain row range [row0,row1).  Used by the host to assemble R A R^T. */
int ddm_galerkin_products(ddm_ctx *ctx, const ddm_csr *A_dir, int64_t nleft, const double *left, int64_t nright,
                          const double *right, int64_t row0, int64_t row1, double *out_host);
/* Diagnostic: the coarse chain (restrict, all-reduce, A0^-1, prolong) alone on an overlapping defect on the device (n doubles), with the
 * full-grid passes over the basis (spread_grid = 0) or the spread ones on spread_grid one-wave workgroups (what the chain uses beside
 * the local solve).  Device outputs: the chunk partials (*npartial doubles), the coarse defect (K) and the prolonged correction (n);
 * all three NULL only queries *npartial.  Synchronous. */
int ddm_galerkin_debug_chain(ddm_ctx *ctx, ddm_galerkin *G, const double *d_ovlp, int spread_grid, double *partial_out, double *d0_out,
                             double *x_ovlp_out, int64_t *npartial);

/* ---- rank-local Schwarz passes and self-finishing reductions: tables and diagnostics -----------------------------------------------
 * Where both plans of a Schwarz level are rank-local (single rank, or an in-library exchange with no off-rank pair) and
 * DDM_FUSE_LOCAL is not "0" when the objects are created, the single-vector apply gathers the overlapping defect in one pass and sums,
 * restricts (and, for ddm_cg_steps, takes <z, r> of) the overlapping result in one pass, and ddm_cg_steps runs without its
 * one-workgroup launches; every result is bit-identical to the general path.
 * ddm_local_maps_host: the index tables of those passes from an extension map (n overlapping rows -> n_novlp non-overlapping rows or
 * -1) and the two plans as ddm_halo_create takes them (a plan with nsend = ndst = 0 and null arrays: no exchange).  src_of[n],
 * own_of[n_novlp], cp_ptr[n_novlp + 1], cp_idx[at most max_cp]; counts[2] = {1 if the tables exist else 0, entries of cp_idx}.
 * Host only, no device needed. */
int ddm_local_maps_host(int64_t n, int64_t n_novlp, const int32_t *ext_map, int64_t copy_nsend, const int64_t *copy_send_idx, int64_t copy_ndst,
                        const int64_t *copy_dst_idx, const int64_t *copy_dst_ptr, const int64_t *copy_src_pos, int64_t add_nsend,
                        const int64_t *add_send_idx, int64_t add_ndst, const int64_t *add_dst_idx, const int64_t *add_dst_ptr,
                        const int64_t *add_src_pos, int32_t *src_of, int32_t *own_of, int32_t *cp_ptr, int64_t max_cp, int32_t *cp_idx, int64_t *counts);
/* Diagnostics (device pointers; nothing synchronises unless said): whether S applies through the tables and its overlapping work
 * vectors; the context's device scalars; the second half of a Schwarz apply on a supplied overlapping vector (general != 0: add
 * exchange + restriction + dot product as separate kernels); one reduction of the CG loop alone (kinds: csrc/preconditioners.hpp). */
int ddm_schwarz_debug_local(ddm_ctx *ctx, ddm_schwarz *S, int *local, double **d_ovlp, double **x_ovlp);
double *ddm_ctx_scalars(ddm_ctx *ctx);
int ddm_schwarz_debug_sum_restrict(ddm_ctx *ctx, ddm_schwarz *S, const double *x_ovlp, int general, const uint8_t *mask, const double *r, double *z, double *out);
int ddm_debug_reduction(ddm_ctx *ctx, int kind, int fin, int64_t n, const uint8_t *mask, double *a, double *b, const double *c, const double *d,
                        int first, const int32_t *own_of, const int32_t *cp_ptr, const int32_t *cp_idx, double *out);

/* ---- GenEO coarse-basis builder ---------------------------------------------------------------
 * GenEOCoarseSpace(A, B, pou, ptree, taskflow, prefix) -> get_basis() (dune/ddm/coarsespaces/coarse_spaces.hh:219-256, 286-331):
 * C = D B_neu D, the lowest nev eigenpairs of A_neu x = lambda C x per subdomain, v <- D v / ||D v||_2, entries of Dirichlet
 * DoFs zeroed (the caller's zero_at_dirichlet, examples/poisson.cc:235-238).  The fields of ddm_geneo_params are the keys of the
 * `<prefix>.eigensolver` sub-tree (dune/ddm/eigensolvers/eigensolver_params.hh:8-62); the block method behind it is described
 * in csrc/geneo.hpp (ncv / blocksize / maxit of the reference's single-vector Lanczos have no meaning for it).
 *   A_neu, B_neu : block-diagonal over the rank's subdomains (sub_ptr[nsub+1] row ranges), B_neu may be the same object as A_neu
 *   pou_host[n], dirichlet_host[n] (may be NULL)
 *   basis_host   : kmax x n row-major (vector j of every subdomain in row j, zero outside the subdomain's rows is NOT implied:
 *                  row j holds vector j of ALL local subdomains side by side); info->nev rows are written
 *   nconv[nsub]  : vectors to use per subdomain (= nev, or the count below `threshold` in threshold mode, spectra.hh:157-163)
 *   eigenvalues_host : nsub x kmax, ascending
 * Synchronous.  DDM_ENUMERIC if a projected eigenproblem breaks down; not converged within maxit is reported in info only. */
typedef struct {
  int32_t nev;             /* eigensolver.nev (default 16) */
  int32_t nev_max;         /* upper bound of the threshold mode (default 2 nev) */
  double tolerance;        /* eigensolver.tolerance (1e-5) */
  double shift;            /* eigensolver.shift (1e-3) */
  double threshold;        /* eigensolver.threshold (-0.5 = off) */
  int32_t maxit;           /* block iterations (400) */
  int32_t extra;           /* guard vectors iterated beyond nev (4); nev + extra <= 132 */
  int32_t seed;            /* start block */
  int32_t preconditioner;  /* 0 = sparse Cholesky of A + shift C if its flop count <= max_direct_flops, else ILU(0); 1 = ILU(0); 2 = Cholesky */
  double max_direct_flops; /* default: a per-rank TIME budget (DDM_GENEO_DIRECT_SECONDS, 6 s) x the measured factorisation rate (1.1e13 multiply-adds / s);
                            * the panels must also fit into 85 % of the free device memory */
  int32_t verbose;
  int32_t raw;             /* 1: return the eigenvectors normalised to ||v||_2 = 1 without the "v <- D v" of finalize_eigenvectors
                            * (the ring coarse spaces extend the ring eigenvectors first, coarse_spaces.hh:612-627) */
} ddm_geneo_params;
typedef struct {
  int32_t iterations, converged, used_direct, nev;
  double worst_residual, setup_s, iterate_s, direct_flops;
} ddm_geneo_info;
int ddm_geneo_params_default(ddm_geneo_params *p);
int ddm_geneo_basis(ddm_ctx *ctx, const ddm_csr *A_neu, const ddm_csr *B_neu, int64_t nsub, const int64_t *sub_ptr, const double *pou_host,
                    const uint8_t *dirichlet_host, const ddm_geneo_params *params, int64_t kmax, double *basis_host, int32_t *nconv,
                    double *eigenvalues_host, ddm_geneo_info *info);
/* The same eigensolver as an object that outlives one call, for matrices whose values change in an unchanged pattern (a Newton step,
 * a time step with a changing coefficient).  ddm_geneo_basis is create + compute(0) + destroy.
 *   create  : assembles the pencil A~ = A_neu + shift C~, C~ = D B_neu D and chooses and builds the preconditioner; nothing else.  The
 *             object owns the pencil, the preconditioner, the Dirichlet mask and the POU on the device, and a map from every pencil entry
 *             to its place in A_neu and B_neu (4 bytes per entry).  A_neu, B_neu (which must outlive it, as a factor's matrix must) and
 *             *params are BORROWED: params is read again by every compute, so nev, nev_max, extra, threshold, tolerance, maxit and seed
 *             may change between two of them; shift, preconditioner and max_direct_flops are those of the creation.  sub_ptr, pou_host
 *             and dirichlet_host are copied.
 *   compute : allocates the work space (six n x 3 (nev + extra) blocks), iterates, writes basis_host / nconv / eigenvalues_host / info
 *             as ddm_geneo_basis does, frees the work space.  Kept on the device afterwards: the raw block X of the last run
 *             (n x (nev + extra) doubles, before v <- D v).  start = 0: random start block -- bit for bit ddm_geneo_basis.  start = 1:
 *             the run begins at nev = max(params->nev, nev of the kept block) from the kept block, further columns drawn as in the cold
 *             start; a doubling of the threshold mode starts from the block just converged.  Without a kept block start = 1 is start = 0.
 *             kmax must not be smaller than the nev the run begins at: info->nev of the last compute is the nev of the kept block.
 *             info->setup_s: the seconds of setup since the last compute -- the creation, or the last successful refresh; 0 for a
 *             compute that follows another without a refresh.
 *   refresh : after ddm_csr_set_values on A_neu and / or B_neu: both value arrays of the pencil are recomputed on the device, in place,
 *             bit for bit what an assembly on the new values gives; the preconditioner is refreshed in place (ILU(0): ddm_ilu0_refresh's
 *             machinery; device supernodal factor: same plans) or, where that is not possible (host-engine direct factor), chosen and
 *             built anew by the rules of the creation.  X is kept.  Synchronous, not to be called under stream capture.  A failure
 *             (DDM_ENUMERIC from the factor, ...) is returned, and compute then answers the same code until a refresh succeeds; that
 *             refresh builds the preconditioner anew where the failed one left none.  A refusal that touched nothing leaves the
 *             object as it was: DDM_ENOTIMPL for a row of A_neu or B_neu of more than 65535 entries, DDM_EINVAL for other matrices.
 *   state   : out = {width of the kept block (0: none), pencil refreshes, preconditioner refreshed in place (count), built anew (count)} */
typedef struct ddm_geneo ddm_geneo;
int ddm_geneo_create(ddm_ctx *ctx, const ddm_csr *A_neu, const ddm_csr *B_neu, int64_t nsub, const int64_t *sub_ptr, const double *pou_host,
                     const uint8_t *dirichlet_host, const ddm_geneo_params *params, ddm_geneo **out);
int ddm_geneo_compute(ddm_ctx *ctx, ddm_geneo *G, int start, int64_t kmax, double *basis_host, int32_t *nconv, double *eigenvalues_host,
                      ddm_geneo_info *info);
int ddm_geneo_refresh(ddm_ctx *ctx, ddm_geneo *G);
int ddm_geneo_state(const ddm_geneo *G, int32_t out[4]);
void ddm_geneo_destroy(ddm_geneo *G);
/* Host twins of the pencil assembly and of its value refresh (no device, no context; for tests).  pencil_host: the pencil of (A, B) on
 * the union pattern and its origin map -- per entry, low 16 bits: 1 + offset inside A's row, high 16 bits: 1 + offset inside B's row,
 * 0 = absent.  rowptr_out: n + 1; col_out, val_At_out, val_C_out, origin_out: room for nnz(A) + nnz(B) entries, *nnz_out are used.
 * pencil_refresh_host: val_At / val_C from new a_val / b_val through the map.  dirichlet may be NULL. */
int ddm_geneo_pencil_host(int64_t n, const int64_t *a_rowptr, const int32_t *a_col, const double *a_val, const int64_t *b_rowptr, const int32_t *b_col,
                          const double *b_val, const double *pou, const uint8_t *dirichlet, double sigma, int64_t *rowptr_out, int32_t *col_out,
                          double *val_At_out, double *val_C_out, uint32_t *origin_out, int64_t *nnz_out);
int ddm_geneo_pencil_refresh_host(int64_t n, const int64_t *rowptr, const int32_t *col, const uint32_t *origin, const int64_t *a_rowptr, const double *a_val,
                                  const int64_t *b_rowptr, const double *b_val, const double *pou, const uint8_t *dirichlet, double sigma, double *val_At,
                                  double *val_C);
/* MsGFEMCoarseSpace(A_neu, A_dir, pou, dirichlet_mask, subdomain_boundary_mask, ptree, taskflow, prefix = "msgfem")
 * (coarse_spaces.hh:663-831; the default coarse space of examples/poisson.ini:36): GenEO's eigenproblem with right-hand side
 * D A_neu D on the interior DoFs, restricted to the a-harmonic functions (A_dir u = 0 in interior rows); Dirichlet DoFs are left
 * out and get zero entries.  Arguments as ddm_geneo_basis plus boundary_host[n] (the subdomain boundary mask); A_dir must be
 * symmetric in its interior block (DDM_ENOTIMPL otherwise).  csrc/geneo.hpp describes how the saddle-point pencil of the
 * reference is replaced by an iteration inside the constrained subspace. */
int ddm_msgfem_basis(ddm_ctx *ctx, const ddm_csr *A_neu, const ddm_csr *A_dir, int64_t nsub, const int64_t *sub_ptr, const double *pou_host,
                     const uint8_t *dirichlet_host, const uint8_t *boundary_host, const ddm_geneo_params *params, int64_t kmax, double *basis_host,
                     int32_t *nconv, double *eigenvalues_host, ddm_geneo_info *info);
/* SVDCoarseSpace(A_ovlp, pou, subdomain_boundary_mask, dirichlet_boundary_mask, ptree, taskflow, prefix = "svd_coarse_space")
 * (coarse_spaces.hh:1268-1407): the n_vectors leading left singular vectors of T = D A_ii^-1 A_{i,Gamma}, zero outside the interior
 * DoFs; with mult_pou != 0 followed by finalize_eigenvectors (:1403).  basis_host: n_vectors x n row-major;
 * singular_values_host: nsub x n_vectors, descending.  T is never formed (csrc/geneo.hpp). */
int ddm_svd_basis(ddm_ctx *ctx, const ddm_csr *A_dir, int64_t nsub, const int64_t *sub_ptr, const double *pou_host, const uint8_t *dirichlet_host,
                  const uint8_t *boundary_host, int n_vectors, int mult_pou, double tolerance, int maxit, double *basis_host, double *singular_values_host,
                  ddm_geneo_info *info);
/* EnergyMinimalExtension(A, interior_indices, boundary_indices) (coarsespaces/energy_minimal_extension.hh:36-229), the building
 * block of the ring and harmonic-extension coarse spaces (coarse_spaces.hh:598, 1097, 1250): u_i = -A_ii^-1 (A [0; u_b])_i.
 * A may be block diagonal (block_ptr[nblocks+1]: one sparse direct factor per block; Cholesky if the interior block is symmetric,
 * LU without pivoting otherwise).  extend works IN PLACE on a row-major DEVICE block X (n x nrhs, leading dimension ldx) that
 * holds the boundary values: interior rows are overwritten, every other row is left alone; values in rows that are neither
 * interior nor boundary do not enter (they count as zero, :109-118). */
typedef struct ddm_harmonic ddm_harmonic;
int ddm_harmonic_create(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, int64_t n_interior, const int64_t *interior_host,
                        int64_t n_boundary, const int64_t *boundary_host, ddm_harmonic **out);
void ddm_harmonic_destroy(ddm_harmonic *H);
int ddm_harmonic_extend(ddm_ctx *ctx, ddm_harmonic *H, int nrhs, double *X, int64_t ldx);
/* The same object read-only and step by step (for tests): each forwards to the function ddm_harmonic_extend, ddm_msgfem_basis and
 * ddm_svd_basis call, with the caller's DEVICE pointers, widths and leading dimensions; nothing is chunked.
 *   ddm_harmonic_create_classes  the object from row classes cls_host[n] (0 = interior, 1 = boundary, anything else = neither), as
 *                            ddm_msgfem_basis and ddm_svd_basis make it; want_transpose != 0: with G_bi = G_ib^T.  DDM_ENUMERIC for an
 *                            interior row without interior entries.
 *   ddm_harmonic_debug_apply op 0: X <- the extension of at most 48 columns (interior rows overwritten, every other row kept);
 *                            op 1: X <- P X (interior rows overwritten, boundary rows kept, every other row zero);
 *                            op 2: X <- P^T X (boundary rows R_b - G_bi A_ii^-T R_i, every other row zero);
 *                            op 3: Y = T T^T X, T = D A_ii^-1 A_{i,Gamma} with D = pou_int (HOST, n entries, zero outside the
 *                                  interior); synchronous.
 *                            Ops 0 .. 2 work in place and ignore pou_int, Y, ldy.  Ops 2 and 3: DDM_ENOTIMPL when the interior block
 *                            is not symmetric, DDM_EINVAL when the object has no G_bi.
 *   ddm_harmonic_info        out[8] = n, symmetric (0 / 1), nnz(G_ib), nnz(G_bi) (-1: absent), 1 when the factor is the device
 *                            supernodal one, the factor's stored entries, its refinement steps, columns the work blocks hold
 *   ddm_harmonic_get_host    the host arrays of G_ib (which = 0) or G_bi (which = 1): rowptr[n + 1], col[nnz], val[nnz], each where
 *                            not NULL */
int ddm_harmonic_create_classes(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, const uint8_t *cls_host, int want_transpose,
                                ddm_harmonic **out);
int ddm_harmonic_debug_apply(ddm_ctx *ctx, ddm_harmonic *H, int op, int nrhs, double *X, int64_t ldx, const double *pou_int, double *Y, int64_t ldy);
int ddm_harmonic_info(const ddm_harmonic *H, int64_t *out);
int ddm_harmonic_get_host(const ddm_harmonic *H, int which, int64_t *rowptr, int32_t *col, double *val);
/* The two dense contractions of the block eigensolver on their own (FP64 MFMA, csrc/geneo_kernels.hpp), for row-major DEVICE
 * blocks split into subdomain row ranges sub_ptr[nsub+1]:
 *   gram  : G_host[s] = U[rows of s]^T V[rows of s]   (nsub matrices pu x pv, row-major; split-K over 2048-row chunks, summed in
 *           chunk order)                              -- Spectra's V^T B f / Gram products
 *   rotate: Out[rows of s, 0:q) = (Base[rows of s, 0:q) -) U[rows of s, 0:p) Y_host[s]   (Y: nsub matrices p x q; more than 48 output
 *           or 80 inner columns run as panels)
 *                                                     -- Spectra's compress_V (Arnoldi.h:310-329)
 * Synchronous. */
int ddm_blockvec_gram(ddm_ctx *ctx, int64_t nsub, const int64_t *sub_ptr, const double *U, int64_t ldu, int pu, const double *V, int64_t ldv,
                      int pv, double *G_host);
/* gram2_sym: G1_host[s] = U^T V1, G2_host[s] = U^T V2 (p x p) for products that are SYMMETRIC by construction (V1 = A~ U, V2 = C~ U:
 * the two projected matrices of the Rayleigh-Ritz step) -- one pass over U, upper tiles only, the lower triangle is the mirrored
 * upper one. */
int ddm_blockvec_gram2_sym(ddm_ctx *ctx, int64_t nsub, const int64_t *sub_ptr, const double *U, int64_t ldu, const double *V1, const double *V2, int64_t ldv, int p,
                           double *G1_host, double *G2_host);
int ddm_blockvec_rotate(ddm_ctx *ctx, int64_t nsub, const int64_t *sub_ptr, const double *U, int64_t ldu, int p, const double *Y_host, int q,
                        const double *Base, int64_t ldb, double *Out, int64_t ldo);
/* The device steps of the block eigensolver on their own (for tests): each forwards to the function the eigensolver calls, with the
 * caller's DEVICE pointers and leading dimensions, so that blocks can be passed as the eigensolver passes them -- slots of an
 * n x 3m array S = [X | W | P] with ld = 3m.  Nothing synchronises unless said.
 *   ddm_csr_mm_ld            Y = A X with leading dimensions (ddm_csr_mm is the case ldx == ldy == nrhs)
 *   ddm_csr_pair_create      two matrices on ONE pattern the way the eigensolver makes its pencil: host arrays adopted, uploaded by a
 *                            helper thread (joined before the call returns); nblocks > 0: the cache-blocked row order of the block
 *                            products is looked for (not when DDM_SPMM_NATURAL_ORDER is set).  *companion holds values only and views
 *                            the pattern of *out; both are destroyed with ddm_csr_destroy, *companion first.
 *   ddm_csr_has_row_order    1 when the matrix carries such a row order (its two-matrix products of at most 32 columns then run
 *                            the cache-blocked kernel)
 *   ddm_csr_mm2_ld           Y1 = A1 X, Y2 = A2 X in one pass for such a pair
 *   ddm_ilu0_solve_multi_ld  ddm_ilu0_solve_multi(_f32) with leading dimensions
 *   ddm_blockvec_rotate_multi  Out_k[rows of s, c(j)] = (Base_k[rows of s, j] -) U_k[rows of s, 0:p) Y_host[s][:, j] for k < narr <= 3 arrays
 *                            that share Y, j < q, c(j) = j for j < gap_from and j + gap from there on; Base: NULL or narr pointers.
 *                            Synchronous.
 *   ddm_geneo_debug_helper   one of the column-wise helper kernels (op 0 .. 5: random start block, residual, column copy, row scaling,
 *                            inverse square roots of Gram diagonals, finalisation with transpose; the arguments per op are listed at
 *                            its definition in csrc/geneo.hpp).  Synchronous. */
int ddm_csr_mm_ld(ddm_ctx *ctx, const ddm_csr *A, int nrhs, const double *X, int64_t ldx, double *Y, int64_t ldy);
int ddm_csr_pair_create(ddm_ctx *ctx, int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, const double *val2, int64_t nblocks,
                        const int64_t *block_ptr, ddm_csr **out, ddm_csr **companion);
int ddm_csr_has_row_order(const ddm_csr *A);
int ddm_csr_mm2_ld(ddm_ctx *ctx, const ddm_csr *A1, const ddm_csr *A2, int nrhs, const double *X, int64_t ldx, double *Y1, double *Y2, int64_t ldy);
int ddm_ilu0_solve_multi_ld(ddm_ctx *ctx, ddm_ilu0 *F, int nrhs, const double *D, int64_t ldd, double *X, int64_t ldx, int f32);
int ddm_blockvec_rotate_multi(ddm_ctx *ctx, int64_t nsub, const int64_t *sub_ptr, int narr, const double *const *U, int64_t ldu, int p, const double *Y_host,
                              int q, const double *const *Base, int64_t ldb, double *const *Out, int64_t ldo, int gap_from, int gap);
int ddm_geneo_debug_helper(ddm_ctx *ctx, int op, int64_t nsub, const int64_t *sub_ptr, int m, int nev, uint64_t seed, const double *a, int64_t lda,
                           const double *b, int64_t ldb, const double *s, double *out, int64_t ldo);
/*   ddm_geneo_debug_start_block  the start block of a warm run: S (n x 3m, DEVICE) from the first min(m_kept, m) columns of kept (n x m_kept,
 *                            DEVICE), the generator of op 0 for the other columns of the X slot, zero W and P slots, zero rows where
 *                            mask (n, DEVICE) is 0.  Synchronous.
 *   ddm_geneo_debug_pencil   the pencil a ddm_geneo holds on the device: *nnz always, the arrays (host) where not NULL.  Synchronous. */
int ddm_geneo_debug_start_block(ddm_ctx *ctx, int64_t n, int m, int m_kept, uint64_t seed, const double *mask, const double *kept, double *S);
int ddm_geneo_debug_pencil(ddm_ctx *ctx, const ddm_geneo *G, int64_t *nnz, int64_t *rowptr, int32_t *col, double *val_At, double *val_C);
/* host logic of the Rayleigh-Ritz step, exposed for the CPU tests: symmetric eigen-decomposition (V: matrix in, eigenvectors as
 * columns out; w ascending) and the rank-revealing Rayleigh-Ritz of gC y = mu gA y (returns the rank used, < 0 on failure) */
int ddm_dense_sym_eig_host(int n, double *V, double *w);
int ddm_dense_rayleigh_ritz_host(int p, const double *gA, const double *gC, int keep, double tau, double *mu, double *Y);

/* ---- CombinedPreconditioner (combined_preconditioner.hh:39-180) --------------------------- */
/* mode 0 = additive, 1 = multiplicative (:56-69).  galerkin may be NULL (one-level). */
int ddm_combined_create(ddm_ctx *ctx, int mode, ddm_op *op, ddm_schwarz *schwarz, ddm_galerkin *galerkin,
                        ddm_combined **out);
void ddm_combined_destroy(ddm_combined *C);
int ddm_combined_status(ddm_ctx *ctx, const ddm_combined *C); /* ddm_schwarz_status of the fine level */
int ddm_combined_apply(ddm_ctx *ctx, ddm_combined *C, double *x, const double *d); /* :127-163 */

/* ---- outer Krylov loop: dune-istl CGSolver::apply as driven by examples/poisson.cc:311-319 -- */
typedef struct {
  int32_t iterations;
  int32_t converged;
  double def0;        /* initial defect norm */
  double reduction;   /* achieved ||r_k|| / ||r_0|| */
  double elapsed_s;   /* wall time of the loop (host clock, stream synchronised) */
} ddm_solve_result;
/* x: initial guess / solution; b: right-hand side, overwritten by the defect (as in dune-istl).
 * hist_host (may be NULL): maxit+1 doubles receiving ||r_0||, ||r_1||, ...
 * fixed_iterations > 0: run exactly that many iterations without testing convergence (bench). */
int ddm_cg_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit,
                 int fixed_iterations, double *hist_host, ddm_solve_result *res);

/* dune-istl RestartedGMResSolver::apply (left-preconditioned, modified Gram-Schmidt, Givens rotations; the
 * monitored norm is that of the preconditioned defect): [solver] type = restartedgmressolver,
 * examples/poisson.ini:12-17; default of dune/ddm/twolevel_schwarz.hh:121-130.  Needed for the
 * non-symmetric preconditioners (restricted Schwarz, multiplicative combination) and operators.
 * Errors and memory as ddm_fgmres_solve below, with ONE basis: min(restart, maxit) + 1 vectors plus one work vector.
 * hist_host (may be NULL): maxit+1 doubles. */
int ddm_gmres_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit,
                    int restart, double *hist_host, ddm_solve_result *res);

/* dune-istl RestartedFlexibleGMResSolver::apply ([solver] type = restartedflexiblegmressolver; DUNE 2.10 solvers.hh, not in the
 * reference snapshot, restated here): RIGHT-preconditioned restarted GMRES that keeps the preconditioned directions.  The monitored
 * norm estimates the TRUE defect ||b - A x|| -- the quantity ddm_cg_solve and ddm_bicgstab_solve test, not the preconditioned defect
 * of ddm_gmres_solve -- and the preconditioner may be a different operator in every iteration.
 *   1. b -= A x; beta = ||b|| (the owner-masked norm of ddm_norm); def0 = beta; def0 < 1e-30: converged at once, x untouched.
 *   2. per restart cycle: v_0 = b / beta; for i = 0 .. restart - 1:
 *        z_i = M^-1 v_i (ddm_combined_apply; z_i is STORED); w = A z_i;
 *        modified Gram-Schmidt against v_0 .. v_i in the order k = 0 .. i: h_{k,i} = <v_k, w>, w -= h_{k,i} v_k;
 *        h_{i+1,i} = ||w||; v_{i+1} = w / h_{i+1,i};
 *        the Givens rotations of ddm_gmres_solve applied to column i of H and to s (s = beta e_0 at the start of the cycle);
 *        norm = |s_{i+1}|, written to hist_host[j] (j = global iteration); the column stops when norm < reduction def0 or norm < 1e-30.
 *      at the end of the cycle, or at the stop: H y = s solved by back substitution, x += sum_{k < i} y_k z_k (no preconditioner apply);
 *      if the solve has not stopped: b -= A (sum_k y_k z_k), beta = ||b||.
 *   3. res->reduction = norm / def0 (after a restart: the recomputed beta / def0), res->iterations = j.
 * DDM_EINVAL (before any device work) for NULL pointers, x == b, restart < 1 or maxit < 0; DDM_ENUMERIC for |w| == 0 before the
 * normalisation, a NaN norm, and when a local solve gave up (ddm_ilu0_peek_status on entry, ddm_ilu0_status at the end).
 * Memory: TWO bases, V of min(restart, maxit) + 1 and Z of min(restart, maxit) vectors, plus one work vector, allocated per call and
 * freed on every return path; DDM_ENOTIMPL (the byte count is in the message) before anything is allocated when they exceed the free
 * device memory.  hist_host (may be NULL): maxit + 1 doubles. */
int ddm_fgmres_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit, int restart,
                     double *hist_host, ddm_solve_result *res);

/* dune-istl BiCGSTABSolver::apply ([solver] type = bicgstabsolver): right-preconditioned, two half steps per iteration, the defect norm
 * is tested after each half step.  hist_host (may be NULL): up to 2 maxit + 1 doubles (one per half step), *nhist receives the count;
 * res->iterations = ceil of the half-step counter (what dune-istl reports).  DDM_ENUMERIC on the breakdowns dune-istl aborts on. */
int ddm_bicgstab_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit, double *hist_host,
                       int32_t *nhist, ddm_solve_result *res);

/* The same loop in pieces, so that a caller can bracket an exact number of iterations
 * (bench.py): begin = "b -= A x; def0 = ||b||" (synchronous); steps = k iterations enqueued
 * without host synchronisation; defect = ||b|| of the last enqueued iteration (synchronous). */
typedef struct ddm_cg ddm_cg;
int ddm_cg_begin(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, ddm_cg **out);
int ddm_cg_steps(ddm_ctx *ctx, ddm_cg *cg, int k);
int ddm_cg_defect(ddm_ctx *ctx, ddm_cg *cg, double *def_host);
double ddm_cg_def0(const ddm_cg *cg);
void ddm_cg_end(ddm_ctx *ctx, ddm_cg *cg);

/* ---- several right-hand sides at once --------------------------------------------------------------------------------------
 * Block vectors are DEVICE pointers to row-major n x nrhs blocks (entry (i, c) at i * nrhs + c: the layout of ddm_csr_mm and
 * ddm_ilu0_solve_multi), 1 <= nrhs <= 32 (DDM_EINVAL outside).  Every column is what the single-vector entry point computes on it;
 * summation orders are kept where that costs nothing (halo exchanges, dots, prolongation: bit-identical per column), elsewhere the
 * columns differ from the single-vector results by rounding only.  Each object allocates its block scratch on first use for the widest
 * nrhs seen and reuses it.  With the alltoall callback (ddm_ctx_set_comm) a halo block is exchanged column by column through the
 * unchanged callback; in-library (RCCL) and single-rank exchanges send one message of nrhs x count doubles per peer. */
int ddm_op_apply_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, const double *X, double *Y);                       /* nonoverlapping_operator.hh:34-39 */
int ddm_op_applyscaleadd_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, double alpha, const double *X, double *Y); /* :41-50 */
/* result_host[c] = <X_c, Y_c> (owner-masked, :76-81): one reduction kernel, one all-reduce of nrhs doubles; synchronous */
int ddm_dot_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, const double *X, const double *Y, double *result_host);
int ddm_schwarz_apply_multi(ddm_ctx *ctx, ddm_schwarz *S, int nrhs, double *X, const double *D);   /* schwarz.hh:115-149 */
/* Precision of the local solve inside the BLOCK applies of S (ddm_schwarz_apply_multi, ddm_combined_apply_multi and the block Krylov
 * drivers): f32 = 0 (the default) double sweeps, f32 = 1 the single-precision sweeps of ddm_ilu0_solve_multi_f32 (preconditioner grade,
 * relative error ~1e-6; double sweeps all the same when nrhs % 4 != 0 or the local solver is a sparse direct factor -- the conditions
 * of ddm_ilu0_solve_multi_f32).  May be switched between two applies, also inside a solve: the preconditioner is then no longer one
 * fixed linear operator, and with f32 = 1 it differs from the single-vector apply.  Only the flexible drivers (ddm_fgmres_solve_multi)
 * are meant to be combined with it: they keep M^-1 v and test the true defect; CG and left-preconditioned GMRES assume a fixed M^-1 and
 * would report the defect of a system preconditioned in single precision.  The single-vector apply never changes.  DDM_EINVAL for S == NULL. */
int ddm_schwarz_set_multi_precision(ddm_schwarz *S, int f32);
/* ddm_ilu0_set_multi_engine on the local solver of S: the engine of the local solves of the block applies (0 levels, 1 xcd, 2 xcd with
 * one team); same results, bit for bit.  DDM_EINVAL for another mode or a null S. */
int ddm_schwarz_set_multi_engine(ddm_schwarz *S, int mode);
int ddm_galerkin_apply_multi(ddm_ctx *ctx, ddm_galerkin *G, int nrhs, double *X, const double *D); /* galerkin_preconditioner.hh:151-194 */
int ddm_combined_apply_multi(ddm_ctx *ctx, ddm_combined *C, int nrhs, double *X, const double *D); /* combined_preconditioner.hh:127-163 */
/* nrhs INDEPENDENT dune-istl CGSolver::apply recurrences (the loop of ddm_cg_solve per column; not a block-Krylov method).  X: initial
 * guesses / solutions, B: right-hand sides, overwritten by the defects.  Column c stops on its own test (def < reduction def0 or
 * def < 1e-30; def0 < 1e-30: converged at once) and is then frozen -- its x, defect and history stop changing -- while the others go on;
 * the loop ends when every column has converged or after maxit iterations.  hist_host (may be NULL): (maxit + 1) x nrhs row-major, entry
 * (i, c) = ||r_i|| of column c for i <= res[c].iterations (later entries are not written).  res: nrhs entries.  DDM_ENUMERIC on a NaN
 * defect and when a local solve gave up (ddm_ilu0_peek_status), as ddm_cg_solve. */
int ddm_cg_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit,
                       double *hist_host, ddm_solve_result *res);
/* Any number of right-hand sides through a CG block of fixed width: ncols >= 1 columns queue for the 1 <= width <= 32 slots of one block
 * loop (ncols may be smaller than width; DDM_EINVAL outside these ranges).  When a slot's column stops, its solution is written out and
 * the next pending column takes the slot at the iteration boundary, so the block stays full until the queue is empty.
 *   X, B: DEVICE blocks, n x ncols row-major (entry (i, j) at i * ncols + j).  X: initial guesses on entry, solutions on exit.  B is NOT
 *     modified: the defects live in the width-wide work block of the preconditioner object.
 *   Column j is what ddm_cg_solve_multi computes on it: its own def0, stop test (def < reduction def0 or def < 1e-30; def0 < 1e-30:
 *     converged with 0 iterations), iteration counter and maxit.  A column that reaches maxit leaves its slot with converged = 0, and its x
 *     is still written to X.
 *   hist_host (may be NULL): (maxit + 1) x ncols row-major, entry (k, j) = the defect of column j after ITS OWN k-th iteration, for
 *     k <= res[j].iterations (later entries are not written).  res: ncols entries; elapsed_s is that of the whole call in every entry.
 *   DDM_ENUMERIC on a NaN defect (the message names the column) and when a local solve gave up, as ddm_cg_solve_multi: the columns
 *     stored before keep their results, X[:, j] of every other column is as on entry and its res entry is reset. */
int ddm_cg_solve_queue(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int64_t ncols, int width, double *X, double *B, double reduction,
                       int maxit, double *hist_host, ddm_solve_result *res);

/* BiCGSTAB for any number of right-hand sides through a block of fixed width: the queue protocol of ddm_cg_solve_queue over the
 * recurrence of ddm_bicgstab_solve.  X, B: the caller's row-major n x ncols device blocks (B is only read); width in [1, 32] slots;
 * res: ncols entries.  Every column is what ddm_bicgstab_solve computes on it (right-preconditioned, two half steps per iteration,
 * norm <= def0 * reduction tested after each, iterations = ceil(half steps / 2), maxit full iterations per column).  A column that
 * stops after a first half step sits out the second; there is one boundary per iteration, after the second half step, at which the
 * stopped columns are stored and the freed slots take the next columns in ascending slot order.  With ncols <= width this is the
 * plain block solve.  hist_host: (2 maxit + 1) x ncols, row-major, or NULL -- row k of column j is its defect after its own k-th
 * half step, rows a column never reaches are left as passed; nhist (may be NULL): entries written per column.  A breakdown (the
 * checks of ddm_bicgstab_solve on rho, omega and h) or a NaN in a running column ends the call with DDM_ENUMERIC, the message naming
 * the column and the scalar: the columns stored before keep their results, X[:, j] of the others is as on entry. */
int ddm_bicgstab_solve_queue(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int64_t ncols, int width, double *X, double *B, double reduction,
                             int maxit, double *hist_host, int32_t *nhist, ddm_solve_result *res);
/* nrhs INDEPENDENT dune-istl RestartedGMResSolver::apply recurrences in one loop (the loop of ddm_gmres_solve per column: left
 * preconditioning, modified Gram-Schmidt in the order k = 0..i, the same Givens rotations, the monitored norm is that of the
 * preconditioned defect; not a block-Krylov method).  X, B, hist_host ((maxit + 1) x nrhs, entries after a column's last iteration are
 * not written) and res (nrhs entries) as in ddm_cg_solve_multi.
 *   Restart cycles are aligned: every column restarts at the iterations restart, 2 restart, ..., exactly where ddm_gmres_solve restarts it.
 *   Stopping: column c stops on its own test (norm < reduction def0 or norm < 1e-30; def0 < 1e-30: converged at once, x untouched); its
 *     solution update is formed from its own Hessenberg columns of the current cycle, at the end of that cycle.
 *   Frozen columns: after a column stopped, its x, its history, its res entry and its column of B do not change any more (as the
 *     single-vector solver does not apply b -= A w after the cycle in which it converged).  A frozen column is skipped by mask, never
 *     multiplied by a zero coefficient: its basis entries may hold anything.
 *   Errors: DDM_EINVAL (before any device work) for nrhs outside 1..32, restart < 1, maxit < 0, NULL pointers or X == B; DDM_ENUMERIC,
 *     naming column and iteration, for a NaN norm or the |w| == 0 breakdown in an active column, and when a local solve gave up
 *     (ddm_ilu0_peek_status on entry, ddm_ilu0_status at the end).
 *   Memory: the Krylov basis is min(restart, maxit) + 1 blocks of n x nrhs doubles plus one work block, allocated per call and freed on
 *     every return path.  When that exceeds the free device memory the call returns DDM_ENOTIMPL (the byte count is in the message)
 *     before it allocates anything.
 *   Host traffic: one read-back per iteration (the (i + 2) x nrhs fresh Hessenberg entries); the dots of one orthogonalisation step
 *     travel as one all-reduce of nrhs doubles. */
int ddm_gmres_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit,
                          int restart, double *hist_host, ddm_solve_result *res);
/* nrhs INDEPENDENT ddm_fgmres_solve recurrences in one loop (flexible restarted GMRES: right preconditioning, the true defect is
 * monitored; not a block-Krylov method), under every rule of ddm_gmres_solve_multi: aligned restart cycles; a column stops on its own
 * test and is then frozen by mask (its x, history, res entry and column of B do not change any more; it is never multiplied by a zero
 * coefficient); one read-back of the (i + 2) x nrhs fresh Hessenberg entries per iteration; one all-reduce of nrhs doubles per
 * orthogonalisation step; DDM_EINVAL before any device work for nrhs outside 1..32, restart < 1,
 * maxit < 0, NULL pointers or X == B; DDM_ENUMERIC, naming column and iteration, for a NaN norm or |w| == 0 in an active column and
 * when a local solve gave up.  X, B, hist_host ((maxit + 1) x nrhs) and res as in ddm_cg_solve_multi.
 *   Memory: two bases, min(restart, maxit) + 1 and min(restart, maxit) blocks of n x nrhs doubles, plus one work block -- twice what
 *     ddm_gmres_solve_multi needs -- allocated per call and freed on every return path; DDM_ENOTIMPL (byte count in the message) before
 *     anything is allocated when that exceeds the free device memory.
 *   The restart (B -= A W with the new defect norms) is one operator apply and ONE element-wise kernel that also forms the partial sums
 *     of the norms, in the summation order of ddm_dot_multi.
 *   With ddm_schwarz_set_multi_precision(S, 1) the local solves run in single precision; the test is still on the true defect. */
int ddm_fgmres_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit,
                           int restart, double *hist_host, ddm_solve_result *res);
/* The restart step of ddm_fgmres_solve_multi on its own (for tests): B -= T in the columns with active_host[c] != 0 (the others are not
 * written), norm2_host[c] = <B_c, B_c> (owner-masked, summed over the ranks) of EVERY column afterwards.  fused != 0: the kernel the
 * driver uses; fused == 0: the kernels it replaces (an AXPY with unit coefficients over the active columns, then the block dot of
 * ddm_dot_multi); the results are bit-identical.  Synchronous. */
int ddm_fgmres_defect_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, const int32_t *active_host, const double *T, double *B, int fused,
                            double *norm2_host);

/* ---- flexible CG ---------------------------------------------------------------------------------------------------------------
 * dune-istl RestartedFCGSolver::apply (complete = 0; [solver] type = restartedfcgsolver) and CompleteFCGSolver::apply (complete != 0;
 * completefcgsolver), DUNE 2.10 solvers.hh, not in the reference snapshot, restated here: CG for a symmetric positive definite
 * operator with a preconditioner that is not symmetric or not fixed.  Like CG it tests the TRUE defect; it keeps 2 (mmax + 1) vectors.
 * Slots 0 .. mmax hold a direction d_s, its image Ad_s and g_s = <d_s, Ad_s>; dots and norms are those of ddm_dot / ddm_norm.
 *   1. b -= A x; def0 = ||b||; hist_host[0] = def0; def0 < 1e-30: converged with 0 iterations, x untouched.
 *   2. i = 1 (global iteration), s = 0 (slot), klimit = 0; while i <= maxit and not stopped:
 *        while s <= mmax, i <= maxit and not stopped:
 *          d_s = M^-1 b (ddm_combined_apply);
 *          J = {0 .. s - 1} (restarted) or {k < klimit, k != s}, then if (klimit <= s) ++klimit (complete);
 *          c_k = <Ad_k, d_s> / g_k for every k in J, ALL from the unmodified d_s (classical Gram-Schmidt); d_s -= c_k d_k, k ascending;
 *          Ad_s = A d_s; g_s = <d_s, Ad_s>; alpha = <d_s, b> / g_s; x += alpha d_s; b -= alpha Ad_s; def = ||b||; hist_host[i] = def;
 *          stop when def < reduction def0 or def < 1e-30; ++i; ++s.
 *        end of a pass: slot 0 <-> slot mmax (d, Ad, g) and s = 1 (restarted); s = 0 and klimit = mmax + 1 (complete).
 *   3. res->iterations = i - 1, res->reduction = def / def0.
 * The orthogonalisation is two kernels around ONE all-reduce of the |J| numerators: a projection that reads d_s once per 8 slots and
 * gives every <Ad_k, d_s> bit-identical to ddm_dot, and one read-modify-write of d_s.  alpha and g_s stay on the device; the host reads
 * one squared defect per iteration.
 * DDM_EINVAL (before any device work) for NULL pointers, x == b, mmax < 1 or maxit < 0; DDM_ENUMERIC for g_s == 0 or a NaN defect
 * (g_s == 0 turns the defect into NaN, one message covers both) and when a local solve gave up (ddm_ilu0_peek_status on entry,
 * ddm_ilu0_status at the end).  Memory: 2 (min(mmax, maxit) + 1) vectors, allocated per call and freed on every return path;
 * DDM_ENOTIMPL (the byte count is in the message) before anything is allocated when they exceed the free device memory.
 * hist_host (may be NULL): maxit + 1 doubles. */
int ddm_fcg_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit, int mmax, int complete,
                  double *hist_host, ddm_solve_result *res);
/* nrhs INDEPENDENT ddm_fcg_solve recurrences in one loop (not a block-Krylov method).  All columns share the slot index s and the
 * window J, which do not depend on data; a column stops on its own test and is then frozen by mask: no kernel writes its x, its column
 * of B, its g or its history afterwards.  Per iteration: one all-reduce of |J| x nrhs numerators (projection: one pass over d_s per
 * 4 slots, every sum bit-identical to ddm_dot_multi), one of 2 nrhs (<d, Ad> and <d, b>, one pass), one of nrhs defect norms, and one
 * read-back of nrhs doubles.  X, B, hist_host ((maxit + 1) x nrhs) and res (nrhs entries) as in ddm_cg_solve_multi; errors and memory
 * (2 (min(mmax, maxit) + 1) blocks of n x nrhs doubles) as in ddm_fcg_solve, DDM_EINVAL also for nrhs outside 1..32.  With
 * ddm_schwarz_set_multi_precision(S, 1) the local solves run in single precision; the test is still on the true defect. */
int ddm_fcg_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit, int mmax,
                        int complete, double *hist_host, ddm_solve_result *res);
/* One orthogonalisation of ddm_fcg_solve_multi on its own (for tests): the n x nrhs block W against nslots >= 0 stored slots -- DS the
 * directions and AD their images, nslots consecutive n x nrhs blocks each, g_host[k * nrhs + c] = <d_k, Ad_k>.  In the columns with
 * active_host[c] != 0: W -= sum_k coef_k d_k with coef_k = <Ad_k, W> / g_k, every coefficient from the W passed in, the terms in
 * ascending k; the other columns of W are not written.  coef_host (nslots x nrhs) receives the coefficients (0 in the other columns).
 * fused != 0: the projection and update kernels the driver uses; fused == 0: the composition they replace (the block dot of
 * ddm_dot_multi per slot on the unmodified W, then one AXPY per slot); the results are bit-identical.  Synchronous. */
int ddm_fcg_orth_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, int nslots, const int32_t *active_host, const double *AD, const double *DS,
                       const double *g_host, double *W, int fused, double *coef_host);

/* ---- block CG --------------------------------------------------------------------------------------------------------------------
 * A TRUE block-Krylov method (O'Leary 1980), unlike every *_multi driver above: the nrhs columns share one search space, each column's
 * error is minimised over the span of ALL columns' Krylov spaces, so the iteration count falls as nrhs grows.  The operator and the
 * preconditioner must be symmetric positive definite, as for CG (standard Schwarz with the additive combination; not restricted
 * Schwarz, not the multiplicative combination); this is not tested.  Blocks are n x nrhs row-major, 1 <= nrhs <= 32; <.,.> is the
 * owner-masked scalar product summed over the ranks and U^T V the nrhs x nrhs matrix of those products.
 *   1. R = B - A X (in B); def0_c = ||R_c||; hist row 0.  def0_c < 1e-30: column c is converged with 0 iterations; it STAYS in the
 *      block (a zero right-hand side gives exactly zero coefficients: its x is not changed).  NaN: DDM_ENUMERIC.
 *   2. Z = M^-1 R; P = Z.
 *   3. k = 1 .. maxit, while some column fails its test:
 *        Q = A P;  W = P^T Q, S = P^T R (one pass over P, Q, R; one all-reduce of 2 nrhs^2 doubles; host read-back 1);
 *        W^+ = pseudo-inverse of (W + W^T) / 2 on the host (ddm_dense_sym_pinv_host with rank_tol), rank_k = eigenvalues kept;
 *        alpha = W^+ S;  X += P alpha;  R -= Q alpha;  def_c = ||R_c|| (the norms come from the pass of the two updates);
 *        Z = M^-1 R;  Q^T Z (one pass; ONE all-reduce of nrhs^2 + nrhs doubles takes it and the squared norms; host read-back 2);
 *        the test; if some column still fails: beta = -W^+ (Q^T Z);  P = Z + P beta.
 *   4. Column c passes when def_c < reduction def0_c or def_c < 1e-30.  The loop ends at the first k at which EVERY column passes.  No
 *      column is frozen: one that has passed goes on being improved.  res[c].iterations = the first k at which c passed (k_end if it
 *      never did); res[c].converged and res[c].reduction describe the state at the end.  hist_host (may be NULL; (maxit + 1) x nrhs):
 *      rows 0 .. k_end are written for EVERY column.  rank_hist_host (may be NULL; maxit + 1 int32): entry k = rank_k, entry 0 = 0.
 * The pseudo-inverse is what makes the method safe with duplicate or dependent right-hand sides, a zero column, and columns that
 * converge at very different speeds; with nrhs = 1 the algorithm is CG.
 * DDM_EINVAL (before any device work; the message names the function) for NULL pointers, X == B, nrhs outside 1..32, maxit < 0 or
 * rank_tol outside (0, 1); DDM_ENUMERIC for a NaN defect (the message names the column), a coupling matrix that is not finite, rank_k = 0
 * while a column still fails, and when a local solve gave up.  Nothing outlives the call on the device but three n x nrhs work blocks
 * of the preconditioner object (P and Q are those of ddm_cg_solve_multi); the active-column mask of the other drivers is not used. */
#define DDM_BCG_RANK_TOL_DEFAULT 1e-12
int ddm_bcg_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit,
                        double rank_tol, double *hist_host, int32_t *rank_hist_host, ddm_solve_result *res);
/* Its three passes over the blocks on their own (for tests; synchronous; no atomics: two identical calls give identical bits).
 *   gram:      G_host = [U^T V1 | U^T V2] (nrhs^2 doubles each, row-major; V2 may be NULL: U^T V1 only), owner-masked, all ranks.
 *   update:    X += P alpha; R -= Q alpha (alpha_host: nrhs x nrhs row-major; per entry the nrhs products are summed in ascending
 *              index and the sum is then applied); norm2_host[c] = <R_c, R_c> afterwards.  The four blocks must be distinct.
 *   direction: P = Z + P beta, in place. */
int ddm_bcg_gram_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, const double *U, const double *V1, const double *V2, double *G_host);
int ddm_bcg_update_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, const double *alpha_host, const double *P, const double *Q, double *X, double *R,
                         double *norm2_host);
int ddm_bcg_direction_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, const double *beta_host, const double *Z, double *P);
/* host logic of the coupling, exposed for the CPU tests: Wpinv = pseudo-inverse of (W + W^T) / 2 (m x m row-major) -- Jacobi scaling
 * d_i = sqrt(|W_ii|) (1 where W_ii = 0), symmetric eigen-decomposition of the scaled matrix, eigenvalues <= tol lambda_max dropped,
 * the rest inverted, scaled back; *rank = eigenvalues kept.  DDM_EINVAL for m < 1, NULL, W == Wpinv, tol outside (0, 1); DDM_ENUMERIC
 * for an entry that is not finite. */
int ddm_dense_sym_pinv_host(int m, const double *W, double tol, double *Wpinv, int *rank);

/* ---- block GMRES -----------------------------------------------------------------------------------------------------------------
 * The non-symmetric companion of block CG: right-preconditioned block GMRES with a FIXED preconditioner (any linear map that does not
 * change within the call: restricted Schwarz, the multiplicative combination, single-precision local solves).  The nrhs columns share
 * one Krylov space; the true defect is monitored, as by CG and flexible GMRES; the basis is that of ddm_gmres_solve_multi, restart + 1
 * blocks of n x nrhs doubles (half of the flexible variant's).  Blocks are n x nrhs row-major, 1 <= nrhs <= 32; <.,.> is the
 * owner-masked scalar product summed over the ranks, U^T V the matrix of those products; maxit counts block iterations.
 *   1. R = B - A X (in B); def0_c = ||R_c||; hist row 0.  def0_c < 1e-30: column c has converged with 0 iterations and is never
 *      touched.  NaN: DDM_ENUMERIC naming the column.
 *   2. Cycle start (deflation).  The running columns are those that have not passed their test.  G = R^T R over the running columns
 *      (rows and columns of the others zero); on the host (ddm_dense_bgmres_factor_host) scaled with d_c = sqrt(G_cc) (1 where
 *      G_cc = 0), eigen-decomposition of the scaled matrix, the p eigenvalues above rank_tol lambda_max kept:
 *      T = Lambda^1/2 U^T D (p x nrhs), C0 = D^-1 U Lambda^-1/2 (nrhs x p); V_0 = R C0 is n x p with orthonormal columns, R = V_0 T.
 *      The width p is fixed for the cycle; duplicate, dependent and zero columns cost no width.  p = 0 while a column runs: DDM_ENUMERIC.
 *   3. Step j of the cycle (j < restart, k < maxit; k counts block iterations):
 *        W = A M^-1 V_j (the block applies at width p);
 *        H1 = [V_0 .. V_j]^T W;  W -= [V_0 .. V_j] H1;  H2 and a second subtraction the same way (block classical Gram-Schmidt twice);
 *        G_W = W^T W from the pass of the second subtraction: four passes over the basis, three all-reduces, one host read-back;
 *        H1 + H2 is column block j of the block Hessenberg matrix; G_W is factored as in 2., but scaled with
 *        d_c^2 = sum_rows (H1 + H2)^2_{.c} + (G_W)_cc, the squared norm of W_c BEFORE the orthogonalisation (scaled by its own diagonal
 *        a column of rounding noise would be a unit column and a rank drop would never be seen): S (rank x p) with S^T S = G_W,
 *        C (p x rank); S, padded with zero rows to p x p, is the sub-diagonal block;
 *        per running column c the monitored defect is the least-squares residual of min || E_1 T e_c - Hbar y || (incremental Householder
 *        QR of the block Hessenberg matrix on the host; every rank computes the same numbers from the all-reduced coefficients);
 *        rank = p: V_{j+1} = W C, the cycle goes on;  rank < p: the space is exhausted -- the step counts and enters the least squares,
 *        the cycle ends after it.
 *   4. Cycle end (restart, maxit, exhaustion, or every running column passes): U = [V_0 .. V_{j-1}] Y, Y one column per block column,
 *      zero for the columns that do not run; Z = M^-1 U; X += Z; R -= A Z; the defect norms are recomputed (one block preconditioner
 *      apply and one block operator apply at width nrhs per cycle) and overwrite the history row of the cycle's last step.  A column
 *      that passed on the monitored value but fails on the recomputed one runs again.
 *   5. Column c passes when def_c < reduction def0_c or def_c < 1e-30.  res[c].iterations = the first block iteration at which c
 *      passed and stayed passed (the final k otherwise); converged and reduction come from the last recomputed defect.
 *      hist_host (may be NULL; (maxit + 1) x nrhs): hist[k nrhs + c] = the monitored defect after block iteration k, recomputed at cycle
 *      ends; a column that does not run repeats its last value, a zero column has zeros throughout.  width_hist_host (may be NULL;
 *      maxit + 1 int32): entry k = the cycle width p of iteration k, entry 0 = 0.
 * With nrhs = 1 the algorithm is right-preconditioned restarted GMRES.  At short restarts a single column can need an iteration more
 * than its independent recurrence.
 * DDM_EINVAL (before any device work; the message names the function) for NULL pointers, X == B, nrhs outside 1..32, maxit < 0,
 * restart < 1 or rank_tol outside (0, 1); DDM_ENOTIMPL when the basis does not fit the free device memory; DDM_ENUMERIC for a NaN
 * defect, coefficients that are not finite, width 0 while a column runs, a singular block Hessenberg matrix, and when a local solve
 * gave up.  Nothing outlives the call on the device but the three n x nrhs work blocks of block CG in the preconditioner object; the
 * active-column mask of the other drivers is not used. */
#define DDM_BGMRES_RANK_TOL_DEFAULT 1e-12
int ddm_bgmres_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit,
                           int restart, double rank_tol, double *hist_host, int32_t *width_hist_host, ddm_solve_result *res);
/* Its three passes over the blocks on their own (for tests; synchronous; no atomics: two identical calls give identical bits).  V: K
 * stored blocks of n x p (combine: n x pin) doubles one after the other; 1 <= p, pin, q <= 32, K >= 1.
 *   project:      H_host (K p^2 doubles, block k row-major) = V_k^T W, owner-masked, all ranks.
 *   combine:      Out (n x q) = (mode 0) / += (1) / -= (2) sum_k V_k C_k with coef_host = the K blocks C_k (pin x q row-major) one
 *                 after the other; per entry the products are summed in ascending k, then ascending row of C_k, and the sum is then
 *                 applied.  Out must not be V.
 *   combine_gram: W (n x p) -= sum_k V_k C_k and G_host (p^2 doubles) = W^T W afterwards, owner-masked, all ranks, in one pass. */
int ddm_bgmres_project_multi(ddm_ctx *ctx, ddm_op *op, int p, int K, const double *V, const double *W, double *H_host);
int ddm_bgmres_combine_multi(ddm_ctx *ctx, ddm_op *op, int mode, int pin, int q, int K, const double *V, const double *coef_host, double *Out);
int ddm_bgmres_combine_gram_multi(ddm_ctx *ctx, ddm_op *op, int p, int K, const double *V, const double *coef_host, double *W, double *G_host);
/* host logic of steps 2 and 3, exposed for the CPU tests: the symmetric positive semi-definite p x p matrix G = S^T S with S (rank x p)
 * and C (p x rank) with C^T G C = I -- scaling d_c = sqrt(|scale2_c|) (1 where 0; scale2 == NULL: the diagonal of G),
 * eigen-decomposition of D^-1 (G + G^T) / 2 D^-1, the eigenvalues above tol lambda_max kept, largest first.  S and C are p x p
 * row-major arrays: rows >= rank of S and columns >= rank of C are zero.  DDM_EINVAL for p < 1, NULL, overlapping arrays, tol outside
 * (0, 1); DDM_ENUMERIC for an entry that is not finite. */
int ddm_dense_bgmres_factor_host(int p, const double *G, const double *scale2, double tol, double *S, double *C, int *rank);

/* ---- instrumentation ---------------------------------------------------------------------
 * Named event timers mirroring the reference's Logger events ("Schwarz/local solve", ...,
 * dune/ddm/schwarz.hh:178-181).  Times are HIP-event milliseconds accumulated on the stream. */
int ddm_timing_enable(ddm_ctx *ctx, int on);
int ddm_timing_get(ddm_ctx *ctx, const char *name, double *total_ms, int64_t *count);
int ddm_timing_reset(ddm_ctx *ctx);

/* ---- input synthesis (host only; no ddm_ctx, no device) ------------------------------------
 * The Q1 diffusion matrix of a structured node box restricted to a node subset, in the caller's numbering, Dirichlet rows and columns
 * eliminated symmetrically: the matrices the reference receives from PDELab's assembler (A of make_communication,
 * A_dir / A_neu / B_neu of examples/pdelab_helper.hh:113-436) for the synthetic benchmark problem.  Row-by-row on host threads, bit for
 * bit what dune_ddm_amd/synth.py builds with numpy.  All shapes x first.  Two calls: indices == NULL fills indptr[n + 1] (row pointers),
 * the second call (same arguments, indptr kept) fills indices / data.  inset, loc_of_box, box_index, diag may be NULL (all nodes,
 * identity numbering, unit Dirichlet diagonal). */
int ddm_synth_q1_matrix(int dim, const int64_t *bshape, const double *ke, const int64_t *eshape, const int64_t *eoff, const double *K,
                        const uint8_t *inset, const int64_t *loc_of_box, int64_t n, const int64_t *box_index, const uint8_t *dmask,
                        const double *diag, int64_t *indptr, int32_t *indices, double *data, int nthreads);

#ifdef __cplusplus
}
#endif
#endif /* DDM_HIP_H */
