// pipe engine of the ILU(0) solve (PipeEngine: local_factor.hpp; kernels and host schedule: trsv_pipe.hpp): builder and enqueue.
// Needs local_factor.hpp.

// Chain/task schedule of the pipe engine (F->pipe); left null when the builder reports that the matrix does not fit the tile
// format (settle_engine then hands the matrix to xcd2).
static int build_pipe_schedule(ddm_ctx *ctx, ddm_ilu0 *F)
{
  const ddm_csr *A = F->A;
  DDMCHECK(ilu0_sync_host_factor(ctx, F)); // (nothing to do at creation; the trace entry point may build after a value refresh)
  pipe::Options opt;
  if (const char *e = std::getenv("DDM_PIPE_DELTA")) opt.delta = std::atoi(e);
  if (const char *e = std::getenv("DDM_PIPE_SPAN")) opt.max_span = std::atoi(e);
  if (const char *e = std::getenv("DDM_PIPE_REUSE")) opt.vote = std::atoi(e);
  int spread_env = -1;
  if (const char *e = std::getenv("DDM_PIPE_SPREAD")) spread_env = std::atoi(e);
  pipe::Schedule S;
  const int nb = (int)F->h_block_ptr.size() - 1;
  // the grid first: it bounds how many tasks the builder may queue in front of producers
  HIPCHECK(ctx, hipFuncSetAttribute((const void *)k_trsv_pipe<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PIPE_LDS_BYTES));
  HIPCHECK(ctx, hipFuncSetAttribute((const void *)k_trsv_pipe<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PIPE_LDS_BYTES));
  int per_cu = 0;
  HIPCHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_trsv_pipe<false>, 64 * PIPE_WAVES, PIPE_LDS_BYTES));
  per_cu = std::max(1, std::min(per_cu, 2));
  if (const char *e = std::getenv("DDM_PIPE_WG_PER_CU")) per_cu = std::max(1, std::min(per_cu, std::atoi(e)));
  const int grid = per_cu * (ctx->num_cu / 8 * 8);
  // All workgroups of the grid are resident (the kernel starts with a barrier over them) and go round-robin over the XCDs.  A queue
  // is first served by the workgroups that start on its subdomain: in XCD-local mode the XCD's share of the grid over the
  // subdomains the XCD owns, in spread mode the grid over all subdomains (the kernel falls back to it by itself when an XCD hosts no
  // workgroup).  Half the smaller of the two may be moved, at most 32 -- "fewer than the queue has workgroups" with room to
  // spare (trsv_pipe_host.hpp, 5.) -- and none where that leaves a queue fewer than 8 slots for its other tasks.
  {
    const int per_queue = std::min((grid / 8) / ((nb + 7) / 8), grid / std::max(nb, 1));
    opt.move_max = std::min(per_queue / 2, 32);
    if (per_queue - opt.move_max < 8) opt.move_max = 0;
    if (const char *e = std::getenv("DDM_PIPE_MOVE")) opt.move_max = std::max(0, std::min(opt.move_max, std::atoi(e)));
    if (const char *e = std::getenv("DDM_PIPE_MOVE_GAP")) opt.move_gap = std::atoi(e);
  }
  if (!pipe::build(A->nrows, A->h_rp.data(), A->h_ci.data(), F->h_lu.data(), F->h_diag.data(), nb, F->h_block_ptr.data(), opt, S)) {
    if (std::getenv("DDM_PIPE_VERBOSE")) std::fprintf(stderr, "[ddm] pipe engine not applicable: %s\n", S.error.c_str());
    return DDM_OK;
  }
  auto E = std::make_unique<PipeEngine>();
  E->ngroups = nb;
  E->stats = S.stats;
  // one XCD hosts 64 workgroups (2 per CU): a subdomain whose sweeps are wider than ~48 wavefronts per level is spread over
  // all XCDs (write-through hand-overs); measured at 216^3: 1 subdomain 6.9 vs 9.2 ms, 2 subdomains 7.6 vs 8.3 ms
  E->spread = spread_env >= 0 ? spread_env : (nb < 8 && S.stats.max_rows_per_level > 48.0 * 64.0 ? 1 : 0);
  E->nposU = S.nposU;
  DDMCHECK(upload(ctx, S.groups.data(), (int64_t)S.groups.size(), E->groups));
  DDMCHECK(upload(ctx, S.tasks.data(), (int64_t)S.tasks.size(), E->tasks));
  DDMCHECK(upload(ctx, S.stream.data(), (int64_t)S.stream.size(), E->stream));
  DDMCHECK(upload(ctx, S.koff.data(), (int64_t)S.koff.size(), E->koff));
  DDMCHECK(upload(ctx, S.posU.data(), (int64_t)S.posU.size(), E->posU));
  {
    std::vector<int64_t> slot(S.slot[0]);
    slot.insert(slot.end(), S.slot[1].begin(), S.slot[1].end());
    DDMCHECK(upload(ctx, slot.data(), (int64_t)slot.size(), E->slot));
  }
  {
    std::vector<int32_t> rowU((size_t)std::max<int64_t>(S.nposU, 1), -1);
    for (size_t i = 0; i < S.posU.size(); ++i) rowU[(size_t)S.posU[i]] = (int32_t)i;
    DDMCHECK(upload(ctx, rowU.data(), (int64_t)rowU.size(), E->rowU));
  }
  HIPCHECK(ctx, E->ypos.alloc(S.nposL));
  HIPCHECK(ctx, E->xpos.alloc(S.nposU));
  HIPCHECK(ctx, dev_memset(E->ypos, 0, sizeof(double) * (size_t)std::max<int64_t>(S.nposL, 1)));
  HIPCHECK(ctx, dev_memset(E->xpos, 0, sizeof(double) * (size_t)std::max<int64_t>(S.nposU, 1)));
  const size_t pbytes = sizeof(unsigned long long) * 16 * std::max<size_t>(S.tasks.size(), 1);
  HIPCHECK(ctx, E->progress.alloc((int64_t)(pbytes / sizeof(unsigned long long))));
  HIPCHECK(ctx, dev_memset(E->progress, 0, pbytes));
  HIPCHECK(ctx, E->queue.alloc(32 * 4 * (int64_t)nb));
  HIPCHECK(ctx, dev_memset(E->queue, 0, sizeof(unsigned) * 32 * 4 * (size_t)nb));
  DDMCHECK(ilu0_alloc_xstate(ctx, F));
  E->grid = grid;
  E->move_max = opt.move_max;
  E->move_gap = opt.move_gap;
  if (std::getenv("DDM_PIPE_VERBOSE")) {
    const pipe::Stats &st = S.stats;
    std::fprintf(stderr,
                 "[ddm] pipe schedule: %lld rows, tasks %lld+%lld, steps %lld+%lld (lane occupancy %.3f / %.3f), entries %lld: local %.3f self-global %.3f remote %.3f, "
                 "stream %.1f MB (%.2fx of 12 B/entry), max producers %lld, max steps %lld, regrouped %lld, levels <= %lld, rows/level <= %.0f, spread %d, grid %d, "
                 "moved in the queues %lld+%lld (most in one %lld; at most %d, gap %d)\n",
                 (long long)st.rows, (long long)st.ntasks[0], (long long)st.ntasks[1], (long long)st.nsteps[0], (long long)st.nsteps[1],
                 (double)st.rows / (64.0 * std::max<int64_t>(st.nsteps[0], 1)), (double)st.rows / (64.0 * std::max<int64_t>(st.nsteps[1], 1)), (long long)st.entries,
                 (double)st.entries_local / std::max<int64_t>(st.entries, 1), (double)st.entries_self_global / std::max<int64_t>(st.entries, 1),
                 (double)st.entries_remote / std::max<int64_t>(st.entries, 1), S.stream.size() / 1e6, S.stream.size() / (12.0 * std::max<int64_t>(st.entries, 1)),
                 (long long)st.max_prod, (long long)st.max_steps, (long long)st.regrouped, (long long)st.max_levels, st.max_rows_per_level, E->spread, E->grid,
                 (long long)st.moved[0], (long long)st.moved[1], (long long)st.max_moved, opt.move_max, opt.move_gap);
  }
  F->pipe = std::move(E);
  return DDM_OK;
}

static unsigned perm_grid(ddm_ctx *ctx, int64_t npos) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((npos + PERM_TILE - 1) / PERM_TILE, (int64_t)ctx->num_cu * 16)); }
// add_ready: `add` is being written on another stream; only the output permutation waits for that event, the solve kernel does not
static hipError_t enqueue_pipe(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, unsigned *err, unsigned long long *stamps, const double *scale = nullptr,
                               const double *add = nullptr, hipEvent_t add_ready = nullptr)
{
  const PipeEngine &E = *F->pipe;
  PipeParams P;
  P.ngroups = E.ngroups;
  P.groups = E.groups;
  P.tasks = E.tasks;
  P.stream = E.stream;
  P.koff = E.koff;
  P.d = d;
  P.ypos = E.ypos;
  P.xpos = E.xpos;
  P.progress = E.progress;
  P.queue = E.queue;
  P.st = F->xstate;
  P.err = err;
  P.stamps = stamps;
  P.spread = E.spread;
  hipLaunchKernelGGL(k_pipe_prologue, dim3(1), dim3(64), 0, ctx->stream, F->xstate, E.queue, E.ngroups * 4);
  if (stamps) hipLaunchKernelGGL((k_trsv_pipe<true>), dim3(E.grid), dim3(64 * PIPE_WAVES), PIPE_LDS_BYTES, ctx->stream, P);
  else hipLaunchKernelGGL((k_trsv_pipe<false>), dim3(E.grid), dim3(64 * PIPE_WAVES), PIPE_LDS_BYTES, ctx->stream, P);
  const hipError_t e = add_ready ? hipStreamWaitEvent(ctx->stream, add_ready, 0) : hipSuccess;
  if (e != hipSuccess) return e; // (x stays unwritten: the caller fails)
  hipLaunchKernelGGL(k_pipe_permute_out, dim3(perm_grid(ctx, E.nposU)), dim3(PERM_WG), 0, ctx->stream, E.nposU, E.rowU, (const double *)E.xpos, x, scale, add);
  return hipSuccess;
}
