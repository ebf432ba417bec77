// The solves of a factor: what the settled engine still lacks (ilu0_prepare_engine), the enqueues of the two direct-factor kinds, the
// one single-vector dispatch (ilu0_enqueue), graph capture, the two solve entry points (ilu0_solve_epilogue, ilu0_solve_multi_ld)
// with their exports, and two diagnostics.  Needs tri_levels.hpp, tri_csr.hpp, engine_*.hpp.

// ---- single right-hand side ---------------------------------------------------------------------
// joins the background build and builds what the settled engine still lacks (the single-vector solve and the box engine's nested
// factor): xcd2 schedules are built on first use
static int ilu0_prepare_engine(ddm_ctx *ctx, ddm_ilu0 *F)
{
  DDMCHECK(ilu0_join(ctx, F));
  if (F->engine == Engine::Box && F->box->shell) return ilu0_prepare_engine(ctx, F->box->shell);
  if (F->engine == Engine::Xcd2 && !F->xcd) return build_xcd_schedule(ctx, F);
  return DDM_OK;
}

// Supernodal device factor, one panel of w <= 48 columns: gather into the permuted work block, solve in place on the panels, scatter;
// then the refinement steps.  The single vector is w = 1 with leading dimensions 1, work = F->pd, yvec = F->px (sn::solve then takes
// its single-vector kernels) and the status word in err; the block solves pass work = F->pD and neither yvec nor err.
static void enqueue_sn_panel(ddm_ctx *ctx, const ddm_ilu0 *F, int w, const double *D, int64_t ldd, double *X, int64_t ldx, double *work, double *yvec, unsigned *err)
{
  const SnDirect &S = *F->sn;
  const int64_t n = F->n;
  const dim3 grid(grid_for(n * w));
  hipLaunchKernelGGL(k_perm_gather, grid, dim3(WG), 0, ctx->stream, n, w, S.f->d_perm, D, ldd, work);
  sn::solve(*S.f, ctx->stream, w, work, w, yvec, err); // (a time-out of the persistent top kernel lands in the status word)
  hipLaunchKernelGGL(k_perm_scatter, grid, dim3(WG), 0, ctx->stream, n, w, S.f->d_perm, (const double *)work, X, ldx);
  for (int it = 0; it < S.refine_steps; ++it) { // X += A^-1 (D - A X)
    hipLaunchKernelGGL(k_residual_rowmajor, dim3((unsigned)((n * (int64_t)w + WG - 1) / WG)), dim3(WG), 0, ctx->stream, n, w, (const int64_t *)S.ref_rp, (const int32_t *)S.ref_ci,
                       (const double *)S.ref_va, (const double *)X, ldx, D, ldd, S.pr, (int64_t)w);
    hipLaunchKernelGGL(k_perm_gather, grid, dim3(WG), 0, ctx->stream, n, w, S.f->d_perm, (const double *)S.pr, (int64_t)w, work);
    sn::solve(*S.f, ctx->stream, w, work, w, yvec, err);
    hipLaunchKernelGGL(k_perm_scatter_add, grid, dim3(WG), 0, ctx->stream, n, w, S.f->d_perm, (const double *)work, X, ldx);
  }
}
// Host sparse direct factor: gather, the two level solves in the fill-reducing order, scatter.  block = false: the single vector
// (nrhs = 1) on F->pd / F->px with the single-vector kernels, one workgroup per block where the factor has that order (Lb / Ub);
// block = true: nrhs columns in panels of at most CSR_PANEL_COLS on the packed work blocks F->pD / F->pX (leading dimension: the
// panel's width), one launch per global level (Lc / Uc) and panel.
constexpr int CSR_PANEL_COLS = WG; // k_trsv_csr_level_multi gives every column of a row a thread of one workgroup
static int enqueue_csr_direct(ddm_ctx *ctx, const ddm_ilu0 *F, bool block, int nrhs, const double *D, int64_t ldd, double *X, int64_t ldx)
{
  const CsrDirect &C = *F->csr;
  double *wd = block ? F->pD : F->pd, *wx = block ? F->pX : F->px;
  for (int c0 = 0; c0 < nrhs; c0 += CSR_PANEL_COLS) {
    const int w = std::min(CSR_PANEL_COLS, nrhs - c0);
    const dim3 grid(grid_for(F->n * w));
    hipLaunchKernelGGL(k_perm_gather, grid, dim3(WG), 0, ctx->stream, F->n, w, C.perm, D + c0, ldd, wd);
    if (block) {
      enqueue_multi_levels_csr(ctx, C.Lc, false, w, wd, w, wx, w);
      enqueue_multi_levels_csr(ctx, C.Uc, true, w, wd, w, wx, w);
    } else {
      DDMCHECK(enqueue_tri_csr(ctx, C.Lb.nblocks ? C.Lb : C.Lc, false, wd, wx));
      DDMCHECK(enqueue_tri_csr(ctx, C.Ub.nblocks ? C.Ub : C.Uc, true, wd, wx));
    }
    hipLaunchKernelGGL(k_perm_scatter, grid, dim3(WG), 0, ctx->stream, F->n, w, C.perm, (const double *)wx, X + c0, ldx);
  }
  return DDM_OK;
}

// x = (LU)^-1 d on the settled engine (ilu0_prepare_engine); the single-launch kernels report time-outs into *err.  *folded: the
// engine applied x *= scale and x += add (either may be null) in its output pass (pipe, box); otherwise that is left to the caller.
static int ilu0_enqueue(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, const double *scale, const double *add, unsigned *err, bool *folded)
{
  *folded = F->engine == Engine::Box || F->engine == Engine::Pipe;
  switch (F->engine) {
  case Engine::Box: return enqueue_box(ctx, F, d, x, scale, add, err);
  case Engine::Pipe: (void)enqueue_pipe(ctx, F, d, x, err, nullptr, scale, add); return DDM_OK;
  case Engine::Xcd2: enqueue_xcd2(ctx, F, d, x, err, nullptr); return DDM_OK;
  case Engine::Supernodal: enqueue_sn_panel(ctx, F, 1, d, 1, x, 1, F->pd, F->px, err); return DDM_OK;
  case Engine::Levels: break;
  }
  if (F->csr) return enqueue_csr_direct(ctx, F, /*block=*/false, 1, d, 1, x, 1);
  DDMCHECK(enqueue_tri(ctx, F->lev->L, false, d, x));
  return enqueue_tri(ctx, F->lev->U, true, d, x);
}

// Captures what enqueue() puts on the context's stream into `cache` (replacing the graph it held), then launches it.  The cache
// answers to `key` once the graph is instantiated; after a failure it holds nothing.
template <class Enqueue>
static int capture_and_launch(ddm_ctx *ctx, GraphCache &cache, const SolveKey &key, Enqueue &&enqueue)
{
  cache.reset();
  hipGraph_t g = nullptr;
  HIPCHECK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue();
  hipError_t e = hipStreamEndCapture(ctx->stream, &g);
  if (rc || e != hipSuccess) {
    if (g) (void)hipGraphDestroy(g);
    return rc ? rc : fail(ctx, DDM_EHIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
  }
  e = hipGraphInstantiate(&cache.exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) {
    cache.exec = nullptr;
    return fail(ctx, DDM_EHIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
  }
  cache.key = key;
  HIPCHECK(ctx, hipGraphLaunch(cache.exec, ctx->stream));
  return DDM_OK;
}

// Diagnostic (not part of the product path): one solve with the loader engine and in-kernel cycle stamps of one
// compute wave.  out[0..5] = cycles waiting for the LDS tile, for the level flags, for the x gathers, for the
// store drain + flag; work items; total cycles (s_memtime ticks, 100 MHz constant clock on gfx9).
extern "C" int ddm_ilu0_debug_stamps(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, unsigned long long *out_host)
{
  dbuf<unsigned long long> st;
  HIPCHECK(ctx, st.alloc(8));
  HIPCHECK(ctx, hipMemset(st, 0, 64));
  DDMCHECK(ilu0_join(ctx, F));
  if (!F->xcd) DDMCHECK(build_xcd_schedule(ctx, F));
  enqueue_xcd2(ctx, F, d, x, F->err, st);
  return ddm_memcpy_d2h(ctx, out_host, st, 48);
}

// Diagnostic (not part of the product path): one solve with the stamped build of the pipe kernel.  Per task PIPE_STAMP_WORDS
// words (layout: trsv_pipe.hpp, STAMP); returns the number of tasks in *ntasks.  out_host may be null
// to query the size.  Also reports group / sweep of every task in meta_host[2 * ntasks] when given.
extern "C" int ddm_ilu0_pipe_trace(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, unsigned long long *out_host, int32_t *meta_host,
                                   int64_t capacity_tasks, int64_t *ntasks)
{
  if (!F || !ntasks) return fail(ctx, DDM_EINVAL, "ddm_ilu0_pipe_trace: bad arguments");
  DDMCHECK(ilu0_join(ctx, F));
  if (!F->pipe) DDMCHECK(build_pipe_schedule(ctx, F));
  if (!F->pipe) return fail(ctx, DDM_EINVAL, "pipe engine not applicable to this matrix");
  const int64_t nt = F->pipe->stats.ntasks[0] + F->pipe->stats.ntasks[1];
  *ntasks = nt;
  if (!out_host) return DDM_OK;
  if (capacity_tasks < nt || !d || !x || d == x) return fail(ctx, DDM_EINVAL, "ddm_ilu0_pipe_trace: bad arguments");
  dbuf<unsigned long long> st;
  HIPCHECK(ctx, st.alloc(PIPE_STAMP_WORDS * (nt + 1)));
  HIPCHECK(ctx, hipMemsetAsync(st, 0, sizeof(unsigned long long) * PIPE_STAMP_WORDS * (size_t)(nt + 1), ctx->stream));
  (void)enqueue_pipe(ctx, F, d, x, F->err, st);
  int rc = ddm_memcpy_d2h(ctx, out_host, st, (int64_t)sizeof(unsigned long long) * PIPE_STAMP_WORDS * nt);
  if (!rc && meta_host) {
    std::vector<pipe::Task> tasks((size_t)nt);
    rc = ddm_memcpy_d2h(ctx, tasks.data(), F->pipe->tasks, (int64_t)sizeof(pipe::Task) * nt);
    for (int64_t t = 0; t < nt && !rc; ++t) {
      meta_host[2 * t] = tasks[(size_t)t].group;
      meta_host[2 * t + 1] = tasks[(size_t)t].sweep;
    }
  }
  return rc;
}

// Diagnostic: what the builder did to the queue order (layout: ddm_hip.h).
extern "C" int ddm_ilu0_pipe_info(ddm_ctx *ctx, ddm_ilu0 *F, int64_t *out, int64_t capacity, int64_t *count)
{
  if (!F || !count) return fail(ctx, DDM_EINVAL, "ddm_ilu0_pipe_info: bad arguments");
  DDMCHECK(ilu0_join(ctx, F));
  PipeEngine *E = F->pipe.get();
  const int64_t nt = E ? E->stats.ntasks[0] + E->stats.ntasks[1] : 0;
  *count = 8 + 2 * nt;
  if (!out) return DDM_OK;
  if (capacity < *count) return fail(ctx, DDM_EINVAL, "ddm_ilu0_pipe_info: capacity too small");
  const int64_t v[8] = {E ? E->grid : 0, E ? E->spread : 0, E ? E->move_max : 0, E ? E->stats.moved[0] : 0, E ? E->stats.moved[1] : 0, E ? E->stats.max_moved : 0,
                        E ? E->move_gap : 0, nt};
  std::copy(v, v + 8, out);
  if (!nt) return DDM_OK;
  std::vector<pipe::Task> tasks((size_t)nt);
  DDMCHECK(ddm_memcpy_d2h(ctx, tasks.data(), E->tasks, (int64_t)sizeof(pipe::Task) * nt));
  for (int64_t t = 0; t < nt; ++t) {
    out[8 + 2 * t] = tasks[(size_t)t].start_level;
    out[9 + 2 * t] = tasks[(size_t)t].moved;
  }
  return DDM_OK;
}

// whether the settled engine of the factor is pipe (waits for the background builder)
static int ilu0_is_pipe(ddm_ctx *ctx, ddm_ilu0 *F, bool *yes)
{
  *yes = false;
  if (!F || F->n == 0) return DDM_OK;
  DDMCHECK(ilu0_prepare_engine(ctx, F));
  *yes = F->engine == Engine::Pipe;
  return DDM_OK;
}

// Both solve entry points start with this: the panels of a device supernodal factor whose last value refresh failed hold no factor
// (sn_refresh.hpp), and the captured graphs are gone with it.
static int sn_check_valid(ddm_ctx *ctx, const ddm_ilu0 *F)
{
  if (F->sn && F->sn->invalid) return fail(ctx, DDM_ENUMERIC, "sparse direct solver (device): the factor is invalid after a failed refresh");
  return DDM_OK;
}

// x = (LU)^-1 d, then optionally x *= scale and x += add (the tail of the Schwarz level: partition of unity of the restricted
// variant and the coarse correction); the pipe and box engines fold both into their output pass, the others append the two kernels.
// add_ready (pipe engine only, ilu0_is_pipe): `add` is being written on another stream and is complete when this event fires.  The
// solve kernel starts without waiting, only the output pass waits -- enqueued directly (three launches), not through the graph cache.
static int ilu0_solve_epilogue(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, const double *scale, const double *add, hipEvent_t add_ready = nullptr)
{
  if (F && F->n == 0) return DDM_OK;
  if (!F || !d || !x || d == x) return fail(ctx, DDM_EINVAL, "ddm_ilu0_solve: bad arguments (d and x must not alias)");
  DDMCHECK(sn_check_valid(ctx, F));
  if (add_ready) {
    bool pipe_engine = false;
    DDMCHECK(ilu0_is_pipe(ctx, F, &pipe_engine));
    if (!pipe_engine || !add) return fail(ctx, DDM_EINVAL, "ddm_ilu0_solve: only the pipe engine joins a side stream in front of its output pass");
    HIPCHECK(ctx, enqueue_pipe(ctx, F, d, x, F->err, nullptr, scale, add, add_ready));
    HIPCHECK(ctx, hipGetLastError());
    return DDM_OK;
  }
  SolveKey key;
  key.d = d, key.x = x, key.scale = scale, key.add = add;
  if (F->graph.hit(key)) {
    HIPCHECK(ctx, hipGraphLaunch(F->graph.exec, ctx->stream));
    return DDM_OK;
  }
  // (re)capture the ~2*nlev launches into a graph bound to this (d, x) pair
  F->graph.reset();
  if (F->sn && !sn::reserve(*F->sn->f, 1)) return fail(ctx, DDM_EHIP, "sparse direct solver: allocation failed");
  DDMCHECK(ilu0_prepare_engine(ctx, F));
  return capture_and_launch(ctx, F->graph, key, [&]() {
    bool folded = false;
    const int rc = ilu0_enqueue(ctx, F, d, x, scale, add, F->err, &folded);
    if (!folded) {
      if (scale) hipLaunchKernelGGL(k_scale, dim3(grid_for(F->n)), dim3(WG), 0, ctx->stream, F->n, scale, x);
      if (add) hipLaunchKernelGGL(k_axpy, dim3(grid_for(F->n)), dim3(WG), 0, ctx->stream, F->n, 1.0, add, x);
    }
    return rc;
  });
}

extern "C" int ddm_ilu0_solve(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x) { return ilu0_solve_epilogue(ctx, F, d, x, nullptr, nullptr); }
// the solve with the tail of a Schwarz level, x = (LU)^-1 d * scale + add entry by entry (either may be null), on whatever engine the
// factor has: what the Schwarz applies enqueue, reachable at row level (tests)
extern "C" int ddm_ilu0_solve_tail(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, const double *scale, const double *add)
{
  return ilu0_solve_epilogue(ctx, F, d, x, scale, add);
}

// Multi-RHS solve X = (LU)^-1 D for row-major n x nrhs block vectors with leading dimensions ldd / ldx (GenEO setup path).
// One launch per level (wide levels of direct factors: one workgroup per row); the launches of one (D, X, nrhs) combination are
// captured into a HIP graph on first use and replayed afterwards (the block eigensolver calls with the same buffers every iteration).
static int ilu0_solve_multi_ld(ddm_ctx *ctx, ddm_ilu0 *F, int nrhs, const double *D, int64_t ldd, double *X, int64_t ldx, bool f32 = false)
{
  if (!F || !D || !X || D == X || nrhs < 1 || ldd < nrhs || ldx < nrhs) return fail(ctx, DDM_EINVAL, "ddm_ilu0_solve_multi: bad arguments");
  if (F->n == 0) return DDM_OK;
  DDMCHECK(sn_check_valid(ctx, F));
  // single precision only for plain ILU(0) factors on aligned blocks of a multiple of 4 columns without wide levels
  f32 = f32 && F->lev && nrhs % 4 == 0 && ldd % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)D & 31) == 0 && ((uintptr_t)X & 31) == 0;
  if (f32)
    for (const TriSchedule *S : {&F->lev->L, &F->lev->U})
      for (const LevelDesc &L : S->desc) f32 = f32 && L.w < 96;
  // engine `xcd` (engine_multi_xcd.hpp) where it was requested and applies; otherwise what ran before it existed
  int why;
  const int engine = multi_xcd_applies(F, &why) ? F->multi_mode : MULTI_LEVELS;
  F->multi_last = engine != MULTI_LEVELS ? MULTI_XCD : MULTI_LEVELS, F->multi_decline = why;
  SolveKey key;
  key.d = D, key.x = X, key.nrhs = nrhs, key.ldd = ldd, key.ldx = ldx, key.f32 = f32, key.engine = engine;
  if (F->mgraph.hit(key)) {
    HIPCHECK(ctx, hipGraphLaunch(F->mgraph.exec, ctx->stream));
    return DDM_OK;
  }
  if (f32) {
    LevelEngine &E = *F->lev;
    for (TriSchedule *S : {&E.L, &E.U}) {
      if (!S->vals_f32 && S->ell_entries > 0) {
        HIPCHECK(ctx, S->vals_f32.alloc(S->ell_entries));
        hipLaunchKernelGGL(k_to_float, dim3((unsigned)((S->ell_entries + 255) / 256)), dim3(256), 0, ctx->stream, S->ell_entries, (const double *)S->vals, S->vals_f32);
      }
      if (S == &E.U && !S->dinv_f32) {
        HIPCHECK(ctx, S->dinv_f32.alloc(F->n));
        hipLaunchKernelGGL(k_to_float, dim3((unsigned)((F->n + 255) / 256)), dim3(256), 0, ctx->stream, F->n, (const double *)S->dinv, S->dinv_f32);
      }
    }
    HIPCHECK(ctx, reserve_cols(E.xf_nrhs, nrhs, E.xf, F->n));
    HIPCHECK(ctx, hipGetLastError());
  }
  F->mgraph.reset();
  if (engine != MULTI_LEVELS) DDMCHECK(build_multi_xcd(ctx, F));
  if (F->sn) {
    SnDirect &S = *F->sn;
    const int w = std::min(nrhs, 48); // the panel kernels take up to 48 columns: wider blocks are solved in column panels
    const double *partial_before = S.f->d_partial, *contrib_before = S.f->d_contrib;
    if (!sn::reserve(*S.f, w)) return fail(ctx, DDM_EHIP, "sparse direct solver: allocation failed");
    if (S.f->d_partial != partial_before || S.f->d_contrib != contrib_before) F->graph.reset(); // the single-vector graph's nodes hold the old scratch pointers
    HIPCHECK(ctx, reserve_cols(F->pm_nrhs, w, F->pD, F->n));
    if (S.refine_steps > 0 && S.pr_cols < w) {
      HIPCHECK(ctx, reserve_cols(S.pr_cols, w, S.pr, F->n));
      F->graph.reset(); // (the single-vector graph holds the old residual buffer)
    }
  }
  if (F->csr) HIPCHECK(ctx, reserve_cols<double>(F->pm_nrhs, std::min(nrhs, CSR_PANEL_COLS), {{F->pX, F->n + F->csr->nvirt}, {F->pD, F->n}})); // one panel
  return capture_and_launch(ctx, F->mgraph, key, [&]() {
    if (F->sn) {
      for (int c0 = 0; c0 < nrhs; c0 += 48) enqueue_sn_panel(ctx, F, std::min(48, nrhs - c0), D + c0, ldd, X + c0, ldx, F->pD, nullptr, nullptr);
    } else if (F->csr) {
      return enqueue_csr_direct(ctx, F, /*block=*/true, nrhs, D, ldd, X, ldx);
    } else if (engine != MULTI_LEVELS) {
      enqueue_multi_xcd(ctx, F, engine, f32, nrhs, D, ldd, X, ldx);
    } else if (f32) {
      // (Splitting the columns into two halves that run as two parallel chains of the captured graph -- a second stream joining the
      //  capture -- was measured and is slower: 6.8 against 5.6 s for the 109 block iterations of the headline GenEO run; every level
      //  kernel is latency-bound, so two half-width kernels cost two full ones and the chains do not overlap enough to pay for that.)
      enqueue_multi_levels_f32(*F->lev, ctx->stream, nrhs, 0, nrhs, D, ldd, X, ldx);
    } else {
      enqueue_multi_levels(ctx, *F->lev, nrhs, D, ldd, X, ldx);
    }
    return DDM_OK;
  });
}
extern "C" int ddm_ilu0_solve_multi(ddm_ctx *ctx, ddm_ilu0 *F, int nrhs, const double *D, double *X) { return ilu0_solve_multi_ld(ctx, F, nrhs, D, nrhs, X, nrhs); }
// the same solve with SINGLE-PRECISION sweeps (factor entries and work block in float, D read and X written in double): preconditioner
// grade -- what the GenEO block iteration applies.  Falls back to the double sweeps when nrhs is not a multiple of 4 or F is a sparse
// direct factor.
extern "C" int ddm_ilu0_solve_multi_f32(ddm_ctx *ctx, ddm_ilu0 *F, int nrhs, const double *D, double *X) { return ilu0_solve_multi_ld(ctx, F, nrhs, D, nrhs, X, nrhs, true); }
