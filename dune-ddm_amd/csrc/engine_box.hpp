// box engine of the ILU(0) solve (BoxEngine: local_factor.hpp; kernels and host schedule: trsv_box.hpp): builder and enqueue.  The
// rows behind the boxes are a factor of their own (BoxEngine::shell) with the general engines, so both halves go back into the
// local solver.  Needs local_factor.hpp.

// (the recursion of the build: ilu0_build_engines, local_solver.hpp, starts this builder, and the nested factor is built by it)
static int ilu0_build_engines(ddm_ctx *ctx, ddm_ilu0 *F, const ddm_csr *A, const std::vector<int64_t> &diag, int64_t nblocks, const int64_t *block_ptr,
                              bool multi_rhs_only, bool box_allowed);
// Box engine part (F->box); left null when the builder declines the matrix (settle_engine then hands it to pipe).
static int build_box_engine(ddm_ctx *ctx, ddm_ilu0 *F)
{
  const ddm_csr *A = F->A;
  const int nb = (int)F->h_block_ptr.size() - 1;
  const auto t0 = std::chrono::steady_clock::now();
  box::Schedule S;
  if (!box::build(A->nrows, A->h_rp.data(), A->h_ci.data(), F->h_lu.data(), F->h_diag.data(), nb, F->h_block_ptr.data(), S)) {
    if (std::getenv("DDM_PIPE_VERBOSE")) std::fprintf(stderr, "[ddm] box engine not applicable: %s\n", S.error.c_str());
    return DDM_OK;
  }
  auto X = std::make_unique<BoxEngine>();
  X->nblocks = nb;
  X->nshell = (int64_t)S.srow.size();
  X->nprod = (int64_t)S.ext_val.size();
  X->stats = S.stats;
  X->h_blocks = S.blocks;
  int rc = upload(ctx, S.blocks.data(), (int64_t)S.blocks.size(), X->blocks);
  if (!rc) rc = upload(ctx, S.steps.data(), (int64_t)S.steps.size(), X->steps);
  if (!rc) rc = upload(ctx, S.stream.data(), (int64_t)S.stream.size(), X->stream);
  if (!rc) rc = upload(ctx, (const unsigned long long *)S.einfo.data(), (int64_t)S.einfo.size(), X->einfo);
  if (!rc) rc = upload(ctx, S.ext_val.data(), X->nprod, X->ext_val);
  if (!rc) rc = upload(ctx, S.ext_col.data(), X->nprod, X->ext_col);
  if (!rc) rc = upload(ctx, S.srp.data(), (int64_t)S.srp.size(), X->srp);
  if (!rc) rc = upload(ctx, S.sci.data(), (int64_t)S.sci.size(), X->sci);
  if (!rc) rc = upload(ctx, S.sva.data(), (int64_t)S.sva.size(), X->sva);
  if (!rc) rc = upload(ctx, S.srow.data(), X->nshell, X->srow);
  if (rc) return rc;
  auto zalloc = [&](auto &buf, int64_t count) {
    count = std::max<int64_t>(count, 1);
    if (buf.alloc(count) != hipSuccess) return fail(ctx, DDM_EHIP, "box engine: allocation failed");
    if (dev_memset(buf, 0, sizeof(*buf.get()) * (size_t)count) != hipSuccess) return fail(ctx, DDM_EHIP, "box engine: memset failed");
    return DDM_OK;
  };
  rc = zalloc(X->E, X->nprod);
  if (!rc) rc = zalloc(X->xs, S.xs_len);
  if (!rc) rc = zalloc(X->prog, S.prog_len);
  if (!rc) rc = zalloc(X->queue, 32 * 2 * (int64_t)nb);
  if (!rc) rc = zalloc(X->ds, X->nshell);
  if (!rc) rc = zalloc(X->xsol, X->nshell);
  if (!rc) rc = ilu0_alloc_xstate(ctx, F);
  if (rc) return rc;
  if (X->nshell > 0) { // the rows behind the boxes: a factor object of their own with the general engines
    rc = csr_create_impl(ctx, X->nshell, X->nshell, S.frp.data(), S.fci.data(), S.fva.data(), /*host_only=*/true, &X->shell_csr);
    if (rc) return rc;
    ddm_ilu0 *G = new ddm_ilu0;
    X->shell = G;
    G->n = X->nshell;
    G->nnz = (int64_t)S.fci.size();
    hvec_copy(G->h_lu, S.fva.data(), S.fva.size());
    rc = ilu0_build_engines(ctx, G, X->shell_csr, S.fdiag, nb, S.fblock_ptr.data(), /*level kernels only=*/std::getenv("DDM_BOX_SHELL_LEVELS") != nullptr,
                            /*box_allowed=*/false);
    if (rc) return rc;
  }
  X->n = A->nrows;
  X->stream_len = (int64_t)S.stream.size();
  X->xs_len = S.xs_len;
  X->prog_len = S.prog_len;
  X->einfo_len = (int64_t)S.einfo.size();
  if (std::getenv("DDM_BOX_CHECK")) {
    if (hipHostMalloc((void **)&X->dbg, 8192, hipHostMallocMapped) != hipSuccess) return fail(ctx, DDM_EHIP, "box engine: allocation failed");
    std::memset(X->dbg, 0, 8192);
  }
  X->grid = 2 * (ctx->num_cu / 8 * 8);
  if (const char *e = std::getenv("DDM_BOX_GRID")) X->grid = std::max(8, std::atoi(e) / 8 * 8);
  if (std::getenv("DDM_PIPE_VERBOSE")) {
    const box::Block &B0 = S.blocks[0];
    std::fprintf(stderr, "[ddm] box engine: %d blocks, box rows %lld (block 0: %d x %d x %d, %d steps per plane), rows behind the boxes %lld (nested factor: %lld entries), "
                 "streams %.1f MB (%.2f B per factor entry of the boxes), shell products %lld, grid %d, built in %.2f s\n",
                 nb, (long long)S.stats.box_rows, B0.nx, B0.ny, B0.nz, B0.nsteps, (long long)X->nshell, (long long)S.fci.size(), S.stats.stream_bytes / 1e6,
                 (double)S.stats.stream_bytes / (27.0 * std::max<int64_t>(S.stats.box_rows, 1)), (long long)X->nprod, X->grid,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  F->box = std::move(X);
  return DDM_OK;
}

// (the recursion of the solve: ilu0_enqueue, local_solve.hpp, dispatches to enqueue_box, and the nested factor is solved through it)
static int ilu0_enqueue(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, const double *scale, const double *add, unsigned *err, bool *folded);
static int enqueue_box(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, const double *scale, const double *add, unsigned *err)
{
  BoxEngine *X = F->box.get();
  BoxParams P;
  P.nblocks = X->nblocks;
  P.blocks = X->blocks;
  P.steps = X->steps;
  P.stream = X->stream;
  P.einfo = X->einfo;
  P.E = X->E;
  P.xs = X->xs;
  P.prog = X->prog;
  P.queue = X->queue;
  P.st = F->xstate;
  P.err = err;
  P.spread = 0;
  if (const char *e = std::getenv("DDM_BOX_SPREAD")) P.spread = std::atoi(e);
  P.dbg = X->dbg;
  P.n = X->n;
  P.stream_len = X->stream_len;
  P.xs_len = X->xs_len;
  P.prog_len = X->prog_len;
  P.einfo_len = X->einfo_len;
  P.e_len = X->nprod;
  // forward sweep of the boxes: y into x
  P.rhs = d;
  P.out = x;
  P.scale = P.add = nullptr;
  int dbg = 0;   // diagnostic: DDM_BOX_DEBUG bit mask switches phases off (1 forward boxes, 2 nested solve, 4 products, 8 backward boxes, 16 shell rhs / out)
  if (const char *e = std::getenv("DDM_BOX_DEBUG")) dbg = std::atoi(e);
  hipLaunchKernelGGL(k_pipe_prologue, dim3(1), dim3(64), 0, ctx->stream, F->xstate, X->queue, X->nblocks * 2);
  hipLaunchKernelGGL(k_box_fill, dim3(grid_for(X->xs_len, WG, 4096)), dim3(WG), 0, ctx->stream, X->xs_len, (unsigned long long *)X->xs.get());   // "not written yet"
  if (!(dbg & 1)) hipLaunchKernelGGL((k_box_sweep<false>), dim3(X->grid), dim3(BOX_WG), 0, ctx->stream, P);
  if (X->nshell > 0 && !(dbg & 2)) {
    if (!(dbg & 16))
      hipLaunchKernelGGL(k_box_shell_rhs, dim3(grid_for(X->nshell)), dim3(WG), 0, ctx->stream, X->nshell, (const int64_t *)X->srp, (const int32_t *)X->sci, (const double *)X->sva,
                         (const int32_t *)X->srow, d, (const double *)x, X->ds);
    bool folded = false; // (nothing to fold: no scale / add)
    DDMCHECK(ilu0_enqueue(ctx, X->shell, X->ds, X->xsol, nullptr, nullptr, err, &folded)); // the nested solve reports into this factor's status word
  }
  // products of the box rows' shell entries, then the backward sweep of the boxes (with the level's tail) and the shell rows of x
  if (!(dbg & 4))
    hipLaunchKernelGGL(k_box_products, dim3(grid_for(X->nprod)), dim3(WG), 0, ctx->stream, X->nprod, (const double *)X->ext_val, (const int32_t *)X->ext_col, (const double *)X->xsol, X->E);
  P.rhs = x;
  P.scale = scale;
  P.add = add;
  hipLaunchKernelGGL(k_pipe_prologue, dim3(1), dim3(64), 0, ctx->stream, F->xstate, X->queue, X->nblocks * 2);
  hipLaunchKernelGGL(k_box_fill, dim3(grid_for(X->xs_len, WG, 4096)), dim3(WG), 0, ctx->stream, X->xs_len, (unsigned long long *)X->xs.get());
  if (!(dbg & 8)) hipLaunchKernelGGL((k_box_sweep<true>), dim3(X->grid), dim3(BOX_WG), 0, ctx->stream, P);
  if (X->nshell > 0 && !(dbg & 16))
    hipLaunchKernelGGL(k_box_shell_out, dim3(grid_for(X->nshell)), dim3(WG), 0, ctx->stream, X->nshell, (const int32_t *)X->srow, (const double *)X->xsol, x, scale, add);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}

// diagnostic: the stamps of the box engine's last solve (DDM_BOX_CHECK=1 at creation): out[2][128][4] = per sweep and plane of block 0
// {start, end (100 MHz clock), polls of the previous plane's progress word, XCC}; zeros without the switch
extern "C" int ddm_ilu0_box_check(const ddm_ilu0 *F, unsigned long long *out1024)
{
  if (!F || !out1024) return DDM_EINVAL;
  for (int k = 0; k < 1024; ++k) out1024[k] = (F->box && F->box->dbg) ? F->box->dbg[k] : 0ull;
  return DDM_OK;
}

// read-only (tests): what the builder made of the matrix and how the solve is launched.  out = {blocks, workgroups of a sweep launch,
// engine code of the nested factor once settled (ddm_ilu0_engine; -1: no rows behind the boxes)}, then per block {nx, ny, nz, steps
// per plane, rows behind the box}.  *count = 3 + 5 blocks; out may be null to ask for it.  A factor that is not on the box engine
// reports 0 blocks.
extern "C" int ddm_ilu0_box_info(const ddm_ilu0 *F, int64_t *out, int64_t capacity, int64_t *count)
{
  if (!F || !count) return DDM_EINVAL;
  ilu0_join_builder(const_cast<ddm_ilu0 *>(F));
  const BoxEngine *X = F->engine == Engine::Box ? F->box.get() : nullptr;
  const int64_t nb = X ? (int64_t)X->h_blocks.size() : 0;
  *count = 3 + 5 * nb;
  if (!out) return DDM_OK;
  if (capacity < *count) return DDM_EINVAL;
  out[0] = nb;
  out[1] = X ? X->grid : 0;
  out[2] = X && X->shell ? ddm_ilu0_engine(X->shell) : -1;
  for (int64_t b = 0; b < nb; ++b) {
    const box::Block &B = X->h_blocks[(size_t)b];
    const int64_t v[5] = {B.nx, B.ny, B.nz, B.nsteps, B.nloc - B.nb};
    std::copy(v, v + 5, out + 3 + 5 * b);
  }
  return DDM_OK;
}
