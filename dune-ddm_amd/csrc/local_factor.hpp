// The local solver of the Schwarz level, first of eight files: what a factor IS (included by ddm_hip.hip after context.hpp and csr.hpp; C ABI:
// the ddm_ilu0_* / ddm_chol_* / ddm_direct_* / ddm_sn_host_* functions of include/ddm_hip.h): ILU(0) and sparse direct factors and
// their triangular-solve engines.  ddm_hip.hip lists the other seven files of the local solver, local_solver.hpp (creation) last.
//
// A factor (struct ddm_ilu0) holds what all engines share and one part per engine it has: LevelEngine (one launch per level; every
// ILU(0) factor has it, the multi-RHS solves run on it), XcdEngine (xcd2), PipeEngine (pipe), BoxEngine (box), CsrDirect (host sparse
// direct factor, CSR level solves) and SnDirect (supernodal factor on the device).  F->engine is the one record of which engine the
// single-vector solve uses (requested_engine at creation, settle_engine after the background build).  The rest of the library
// reaches factors only through the ddm_ilu0_* entry points and ilu0_create_impl, direct_create_impl, ilu0_solve_epilogue,
// ilu0_solve_multi_ld, ilu0_peek_status and ilu0_direct_flops.

struct TriSchedule { // one triangular factor, level by level in sliced ELL
  int64_t nlev = 0;
  std::vector<LevelDesc> desc;        // per level
  dbuf<int32_t> rows;                 // [n] rows sorted by level
  dbuf<int32_t> cols;                 // sliced ELL columns
  dbuf<double> vals;                  // sliced ELL values
  dbuf<double> dinv;                  // upper only: inverse pivots in level order
  dbuf<float> vals_f32, dinv_f32;     // single-precision copies for the preconditioner sweeps (made on first use)
  dbuf<LevelDesc> d_desc;             // device copy (for the small-level kernel)
  struct Launch {                     // execution plan
    int first, count;                 // levels [first, first+count)
    bool small;                       // one workgroup loops over the levels
  };
  std::vector<Launch> plan;
  int64_t ell_entries = 0;
  // single-launch block solve (trsv_multi_plan.hpp): blk_off[l (nb + 1) + b] = first position of block b inside level l, blk_nlev[b]
  dbuf<int32_t> blk_off, blk_nlev;
  std::vector<int32_t> h_blk_nlev;
};

struct TriCsr { // one triangular factor of the sparse direct solver: rows in level order, CSR entries (kernels.hpp: CsrLevel)
  int64_t nlev = 0;
  std::vector<CsrLevel> desc;
  int64_t nrows = 0, entries = 0; // transformed rows (real + virtual unknowns of the supernodes), stored entries
  dbuf<int32_t> rows;             // destination unknown of a row
  dbuf<int32_t> rhs;              // index of its right-hand side (lower: in d, upper: in x) or -1 (none)
  dbuf<int64_t> lrp;
  dbuf<int32_t> cols;
  dbuf<double> vals;
  dbuf<double> dinv; // upper only
  dbuf<CsrLevel> d_desc;
  struct Launch {
    int first, count;
    bool fused;
  };
  std::vector<Launch> plan;
  // block-wise variant (rows ordered by (block, level)): one workgroup per block runs the block's whole solve
  int nblocks = 0;
  dbuf<int32_t> blk_lev_ptr;
};

// ---- the parts of a factor ----------------------------------------------------------------------
// Device arrays are dbuf members (device_buffer.hpp), so a part's destructor only says what is NOT memory, or an order that matters.

// Engine of the single-vector solve; the values are the codes ddm_ilu0_engine reports.
enum class Engine : int { Levels = 0, Xcd2 = 4, Pipe = 8, Supernodal = 16, Box = 32 };

struct MultiXcdSync { // what the single-launch block solve (engine_multi_xcd.hpp) adds to the level engine: flags and a report, no factor memory
  dbuf<unsigned long long> flags; // MULTI_XCD_TEAMS x grid flag slots, MULTI_XCD_FLAG_STRIDE words apart (zero-initialised; epochs separate launches)
  unsigned *report = nullptr;     // pinned, device-mapped host words the kernel's first workgroup writes: tickets[8], teams, one-team flag
  int grid = 0;
  ~MultiXcdSync() { if (report) (void)hipHostFree(report); }
};
struct LevelEngine { // one launch per level (runs of small levels in one workgroup); also the multi-RHS solves of every ILU(0) factor
  TriSchedule L, U;
  dbuf<float> xf; // n x xf_nrhs work block of the single-precision multi-RHS sweeps
  int xf_nrhs = 0;
  std::unique_ptr<MultiXcdSync> mx; // built by the first block solve on engine `xcd`
};

struct XcdEngine { // xcd2 (XCD-local + loader waves): per-block (subdomain) level schedules, built on first use (build_xcd_schedule)
  int ngroups = 0;
  dbuf<GroupDesc> groups;
  dbuf<LevelDesc> desc;
  dbuf<int64_t> flag_off;
  dbuf<int32_t> rows, cols;
  dbuf<double> vals, dinv;
  dbuf<unsigned> flags;
  dbuf<double> dperm; // right-hand side permuted into level order (loader engine)
  dbuf<int64_t> lpos; // positions of the L parts (only those need the permuted right-hand side)
};

struct PipeEngine { // pipe: chains x tasks, see trsv_pipe_host.hpp
  int ngroups = 0;
  dbuf<pipe::Group> groups;
  dbuf<pipe::Task> tasks;
  dbuf<unsigned char> stream;
  dbuf<int32_t> koff, posU, rowU; // rowU: natural row of every U position (-1: padding)
  dbuf<double> ypos, xpos;
  dbuf<unsigned long long> progress;
  dbuf<unsigned> queue;
  dbuf<int64_t> slot;             // [2 n] pipe::row_slot of every row's L entries, then of its U entries (the value refresh)
  int64_t nposU = 0;
  int spread = 0; // placement-independent mode (set when a subdomain has more work per level than one XCD's workgroups take)
  int grid = 0;
  int move_max = 0, move_gap = 0; // queue order the schedule was built with (pipe::Options)
  pipe::Stats stats;
};

struct BoxEngine { // box (trsv_box_host.hpp): structured leading box of every block + a nested factor for the rows behind it
  int nblocks = 0;
  int64_t nshell = 0, nprod = 0;
  dbuf<box::Block> blocks;
  dbuf<box::StepTab> steps;
  dbuf<double> stream;
  dbuf<unsigned long long> einfo;
  dbuf<double> E, ext_val;
  dbuf<int32_t> ext_col;
  dbuf<double> xs;
  dbuf<unsigned long long> prog;
  dbuf<unsigned> queue;
  unsigned long long *dbg = nullptr;    // DDM_BOX_CHECK: pinned host words of the kernels' address check (hipHostMalloc)
  int64_t n = 0, stream_len = 0, xs_len = 0, prog_len = 0, einfo_len = 0;
  // shell system
  dbuf<int64_t> srp;
  dbuf<int32_t> sci, srow;
  dbuf<double> sva, ds, xsol;
  ddm_csr *shell_csr = nullptr;
  ddm_ilu0 *shell = nullptr;
  int grid = 0;
  box::Stats stats;
  std::vector<box::Block> h_blocks;     // host copy of `blocks` (ddm_ilu0_box_info)
  ~BoxEngine() // the body runs before the members go: the nested factor (it reads shell_csr), then its matrix, then the arrays above
  {
    ddm_ilu0_destroy(shell);
    ddm_csr_destroy(shell_csr);
    if (dbg) (void)hipHostFree(dbg);
  }
};

struct CsrDirect { // host sparse direct factor (ddm_chol_create): lives in a fill-reducing order, d / x are permuted around the solve
  ddm_csr *pattern = nullptr; // host-only CSR pattern of L + D + L^T in the permuted order (owned)
  dbuf<int32_t> perm;         // device: perm[new] = old
  int64_t nvirt = 0;          // virtual unknowns of the supernodal transformation: the permuted solution holds n + nvirt entries
  TriCsr Lc, Uc;              // global levels: multi-RHS solves, one launch per level
  TriCsr Lb, Ub;              // the same factors ordered by (block, level): single right-hand side, one workgroup per block
  ~CsrDirect() { delete pattern; }
};

struct SnDirect { // supernodal factor computed ON THE DEVICE (sn_chol.hpp); solves run on its panels, in place in pd / pD
  std::unique_ptr<sn::Factor> f;
  // iterative refinement (dune/ddm/eigensolvers/umfpack.hh:42-129; UMFPACK refines inside its own solve too): the number of steps
  // is fixed when the factor is created, from the backward error of a probe solve (sn_direct_create), so that the solves stay
  // captured HIP graphs; the matrix is kept as device copies of its three arrays
  int refine_steps = 0;
  double refine_omega[5] = {0, 0, 0, 0, 0}; // backward error of the probe after 0, 1, .. steps
  dbuf<int64_t> ref_rp;
  dbuf<int32_t> ref_ci;
  dbuf<double> ref_va, pr; // pr: residual block (n x pr_cols)
  int pr_cols = 0;
  // a value refresh (sn_refresh.hpp) overwrites the panels in place: when it fails they hold no factor, and every solve entry
  // returns DDM_ENUMERIC until a later refresh succeeds
  bool invalid = false;
};

struct Refactor { // what ddm_ilu0_refresh keeps on the device (ilu0_refactor.hpp), allocated by the first refresh
  dbuf<double> lu;      // the factor in the pattern of A as the last successful refresh left it
  dbuf<double> scratch; // the factor being computed: exchanged with `lu` once the status word says that every pivot was fine
  dbuf<int64_t> diag;   // h_diag
  dbuf<unsigned> status;
  std::vector<TriSchedule::Launch> plan; // launches of the factorisation over the levels of F->lev->L
  bool host_stale = false; // h_lu is older than `lu`: ilu0_sync_host_factor brings it up to date for whoever reads it next
};

struct SolveKey { // the arguments a captured solve is bound to; the single-vector cache leaves nrhs, ldd, ldx, f32 as they stand here
  const double *d = nullptr, *scale = nullptr, *add = nullptr;
  double *x = nullptr;
  int64_t nrhs = 1, ldd = 1, ldx = 1;
  bool f32 = false; // the graph runs the single-precision sweeps
  int engine = 0;   // block solves: MULTI_LEVELS, MULTI_XCD or MULTI_XCD_ONE_TEAM, whichever the graph runs
  bool operator==(const SolveKey &o) const
  {
    return d == o.d && x == o.x && scale == o.scale && add == o.add && nrhs == o.nrhs && ldd == o.ldd && ldx == o.ldx && f32 == o.f32 && engine == o.engine;
  }
};
struct GraphCache { // one captured, instantiated solve and the key it was captured for (capture_and_launch sets both)
  hipGraphExec_t exec = nullptr;
  SolveKey key;
  bool hit(const SolveKey &k) const { return exec && key == k; }
  void reset() { if (exec) (void)hipGraphExecDestroy(exec); exec = nullptr; key = SolveKey{}; }
  ~GraphCache() { reset(); }
};

// Engine of the block solve of a plain ILU(0) factor (ddm_ilu0_set_multi_engine; DDM_TRSV_MULTI_MODE at creation) and why a request
// for `xcd` was not followed (ddm_ilu0_multi_info)
enum { MULTI_LEVELS = 0, MULTI_XCD = 1, MULTI_XCD_ONE_TEAM = 2 };
enum { MULTI_RAN_REQUESTED = 0, MULTI_NOT_REQUESTED = 1, MULTI_DIRECT_FACTOR = 2, MULTI_WIDE_LEVEL = 3 };

struct ddm_ilu0 {
  int64_t n = 0, nnz = 0;
  Engine engine = Engine::Levels;
  int multi_mode = MULTI_LEVELS;                                  // requested engine of the block solves
  int multi_last = -1, multi_decline = MULTI_NOT_REQUESTED;       // engine of the last block solve (-1: none yet), decline reason
  hvec<double> h_lu; // factor values in the pattern of A
  std::vector<int64_t> h_diag, h_block_ptr;
  const ddm_csr *A = nullptr;
  // status word of the single-launch engines in pinned, device-mapped HOST memory: a wave that gives up waiting writes its code
  // straight into it, so the host can look at it without synchronising the stream (ilu0_peek_status: every apply checks the
  // applies before it -- fail fast instead of returning stale results until somebody calls ddm_ilu0_status)
  unsigned *err = nullptr;
  dbuf<XcdState> xstate; // tickets and epoch of the persistent kernels (pipe, xcd2, box)
  // direct factors: right-hand side / solution permuted into the factor's order (n, n + nvirt doubles), the same for row-major blocks
  dbuf<double> pd, px;
  dbuf<double> pD, pX;
  int pm_nrhs = 0;
  double direct_flops = 0.0;
  int refresh_count = 0; // successful in-place value refreshes since creation (ddm_ilu0_refresh_count)
  // the pipe / box part is built in the background (its own host threads + uploads; 2.6 s at 216^3, nothing of it is needed before
  // the first single-vector solve): every reader of those parts or of `engine` joins first (ilu0_join)
  std::thread builder;
  int builder_rc = DDM_OK;
  std::string builder_err;
  std::unique_ptr<LevelEngine> lev;
  std::unique_ptr<XcdEngine> xcd;
  std::unique_ptr<PipeEngine> pipe;
  std::unique_ptr<BoxEngine> box;
  std::unique_ptr<CsrDirect> csr;
  std::unique_ptr<SnDirect> sn;
  std::unique_ptr<Refactor> refac;
  // HIP graph caches: the single-vector solve for one (d, x, scale, add), the multi-RHS solve for one (D, X, nrhs, ld, f32)
  GraphCache graph, mgraph;
  ~ddm_ilu0() // the body runs before any member goes: the builder thread writes the parts, the graph execs point into the arrays
  {
    if (builder.joinable()) builder.join();
    graph.reset();
    mgraph.reset();
    if (err) (void)hipHostFree(err);
  }
};
static inline double ilu0_direct_flops(const ddm_ilu0 *F) { return F->direct_flops; }
// the status word WITHOUT synchronising (ddm_ilu0_status synchronises): what the solves that have finished so far reported (0 = nothing wrong yet)
static inline unsigned ilu0_peek_status(const ddm_ilu0 *F) { return (F && F->err) ? *(volatile unsigned *)F->err : 0u; }

static int ilu0_alloc_status(ddm_ctx *ctx, ddm_ilu0 *F)
{
  if (hipHostMalloc((void **)&F->err, 128, hipHostMallocMapped) != hipSuccess) return fail(ctx, DDM_EHIP, "local solver: allocation failed");
  std::memset(F->err, 0, 128);
  return DDM_OK;
}
// the XcdState of a factor: allocated by the first builder of a persistent engine, shared by the others
static int ilu0_alloc_xstate(ddm_ctx *ctx, ddm_ilu0 *F)
{
  if (F->xstate) return DDM_OK;
  HIPCHECK(ctx, F->xstate.alloc(1));
  HIPCHECK(ctx, dev_memset(F->xstate, 0, sizeof(XcdState)));
  return DDM_OK;
}

// ---- engine choice ------------------------------------------------------------------------------
// At creation: DDM_TRSV_MODE = levels | xcd2 | box | pipe (the default; also any other value), the box engine only where allowed
// (not for its own nested factor); the level kernels for a factor that only sees multi-RHS solves.  Direct factors are created
// with theirs (levels for the host factor, supernodal for the device factor).  The box engine is opt-in: bit-exact, but at the
// benchmark's size still slower than pipe (4.4 against 3.25 ms per solve: DESIGN.md section 3d says what bounds it).
static Engine requested_engine(bool multi_rhs_only, bool box_allowed)
{
  if (multi_rhs_only) return Engine::Levels;
  const char *m = std::getenv("DDM_TRSV_MODE");
  if (!m) return Engine::Pipe;
  if (!std::strcmp(m, "levels")) return Engine::Levels;
  if (!std::strcmp(m, "xcd2")) return Engine::Xcd2;
  return box_allowed && !std::strcmp(m, "box") ? Engine::Box : Engine::Pipe;
}
// After the background build: an engine whose builder declined the matrix hands it on -- box to pipe, pipe to xcd2 (which takes
// any matrix; its schedules are built on first use).  A failed build leaves the choice alone: every call that needs it reports the
// failure.  Idempotent.
static void settle_engine(ddm_ilu0 *F)
{
  if (F->builder_rc) return;
  if (F->engine == Engine::Box && !F->box) F->engine = Engine::Pipe;
  if (F->engine == Engine::Pipe && !F->pipe && F->n > 0) F->engine = Engine::Xcd2;
}
static void ilu0_join_builder(ddm_ilu0 *F)
{
  if (F->builder.joinable()) F->builder.join();
  settle_engine(F);
}
// h_lu after a value refresh (ddm_ilu0_refresh leaves the new factor on the device): copied back when somebody reads it --
// ddm_ilu0_get_factors_host and the builders that run after creation (xcd2 on first use, the pipe trace).  Synchronous.
static int ilu0_sync_host_factor(ddm_ctx *ctx, ddm_ilu0 *F)
{
  if (!F->refac || !F->refac->host_stale) return DDM_OK;
  HIPCHECK(ctx, hipMemcpyAsync(F->h_lu.data(), F->refac->lu, sizeof(double) * (size_t)F->nnz, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  F->refac->host_stale = false;
  return DDM_OK;
}
// waits for the background part of the setup; its failure is reported by every call that needs the result
static int ilu0_join(ddm_ctx *ctx, ddm_ilu0 *F)
{
  ilu0_join_builder(F);
  if (F->builder_rc) return fail(ctx, F->builder_rc, "%s", F->builder_err.c_str());
  return DDM_OK;
}
