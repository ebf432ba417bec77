// CG: one right-hand side (begin / steps / defect / end / solve), m right-hand sides at once, and any number of them queued through a
// block of fixed width.  Needs krylov_frame.hpp.
#pragma once

// ---- CG ----------------------------------------------------------------------------------------
// dune-istl CGSolver::apply, split so that a caller can time an exact number of
// iterations: begin = "b -= A x; def0 = ||b||", one step = "prec.apply; rho; [beta; p = beta p + q];
// q = A p; alpha; lambda; x += lambda p; b -= lambda q; def = ||b||".
struct ddm_cg {
  ddm_op *op = nullptr;
  ddm_combined *prec = nullptr;
  double *x = nullptr, *b = nullptr; // the caller's
  dbuf<double> p, q;
  int64_t n = 0;
  int it = 0;
  double def0 = 0.0;
  // The loop without its one-workgroup launches (self-finishing reductions, quotients formed by their consumers: kernels.hpp) and
  // with <q, b> taken by the apply's last pass: where the Schwarz level applies through its rank-local tables (ddm_schwarz::local).
  bool fuse = false;
};
extern "C" int ddm_cg_begin(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, ddm_cg **out)
{
  if (!ctx || !op || !prec || !x || !b || !out) return fail(ctx, DDM_EINVAL, "ddm_cg_begin: bad arguments");
  auto S = std::make_unique<ddm_cg>();
  S->op = op;
  S->prec = prec;
  S->x = x;
  S->b = b;
  S->n = op->n;
  if (S->p.alloc(S->n) != hipSuccess || S->q.alloc(S->n) != hipSuccess) return fail(ctx, DDM_EHIP, "ddm_cg_begin: allocation failed");
  S->fuse = prec->schwarz && schwarz_is_local(ctx, prec->schwarz); // (the Schwarz level read the switch when it was created)
  DDMCHECK(ddm_op_applyscaleadd(ctx, op, -1.0, x, b)); // prec.pre(x,b); b -= A x
  double bb = 0.0;
  DDMCHECK(dot_device(ctx, S->n, op->owner, b, b, ctx->scal + SCAL_DEF2));
  DDMCHECK(ddm_memcpy_d2h(ctx, &bb, ctx->scal + SCAL_DEF2, sizeof(double)));
  S->def0 = std::sqrt(bb);
  *out = S.release();
  return DDM_OK;
}
extern "C" void ddm_cg_end(ddm_ctx *ctx, ddm_cg *S)
{
  if (!S) return;
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  delete S;
}
extern "C" double ddm_cg_def0(const ddm_cg *S) { return S->def0; }
// Enqueues k iterations without synchronising; the squared defect of the last one is left in
// device scalar SCAL_DEF2 (read it with ddm_cg_defect).
extern "C" int ddm_cg_steps(ddm_ctx *ctx, ddm_cg *S, int k)
{
  double *scal = ctx->scal;
  double *rider = nullptr; // the previous iteration's squared defect norm, not yet summed over the ranks: handed to the next apply
  const int G = grid_for(S->n);
  for (int i = 0; i < k && S->fuse; ++i) { // the same iteration in fewer launches: every scalar and vector bit for bit what the loop below leaves
    const bool first = S->it == 0;
    double *z = first ? S->p : S->q, *rho = scal + (first ? SCAL_RHOLAST : SCAL_RHO);
    ApplyDot dot{S->op->owner, S->b, rho, false};
    DDMCHECK(combined_apply_impl(ctx, S->prec, z, S->b, rider, &dot));                      // q = M^-1 b and rho = <q, b> where the apply can take it
    if (!dot.done) DDMCHECK(dot_device_fin(ctx, S->n, S->op->owner, z, S->b, rho));
    if (!first) hipLaunchKernelGGL(k_cg_direction_beta, dim3(G), dim3(WG), 0, ctx->stream, S->n, scal, S->q, S->p); // beta = rho / rholast; p = beta p + q
    DDMCHECK(ddm_op_apply(ctx, S->op, S->p, S->q));                                          // q = A p
    DDMCHECK(dot_device_fin(ctx, S->n, S->op->owner, S->p, S->q, scal + SCAL_PQ));           // alpha = <p, q>
    const int nb = grid_for(S->n, WG * 4, RED_MAX_BLOCKS);
    const int num = first ? SCAL_RHOLAST : SCAL_RHO; // lambda = rholast / alpha; rholast = rho; x += lambda p; b -= lambda q; def^2 = <b, b>
    if (S->op->owner)
      hipLaunchKernelGGL(k_cg_update_norm_fin<true>, dim3(nb), dim3(WG), 0, ctx->stream, S->n, scal, num, S->op->owner, S->p, S->q, S->x, S->b, ctx->partial, ctx->ticket, scal + SCAL_DEF2);
    else
      hipLaunchKernelGGL(k_cg_update_norm_fin<false>, dim3(nb), dim3(WG), 0, ctx->stream, S->n, scal, num, S->op->owner, S->p, S->q, S->x, S->b, ctx->partial, ctx->ticket, scal + SCAL_DEF2);
    rider = i + 1 < k && S->prec->galerkin ? scal + SCAL_DEF2 : nullptr; // (as below)
    if (!rider) DDMCHECK(ctx_allreduce(ctx, scal + SCAL_DEF2, 1, "scalar product"));
    S->it += 1;
  }
  for (int i = 0; i < k && !S->fuse; ++i) {
    const bool first = S->it == 0;
    DDMCHECK(combined_apply_impl(ctx, S->prec, first ? S->p : S->q, S->b, rider));         // q = M^-1 b  (p on the first step)
    DDMCHECK(dot_device(ctx, S->n, S->op->owner, first ? S->p : S->q, S->b, scal + (first ? SCAL_RHOLAST : SCAL_RHO))); // rho = <q, b>
    if (!first) {
      hipLaunchKernelGGL(k_cg_beta, dim3(1), dim3(1), 0, ctx->stream, scal);                 // beta = rho / rholast; rholast = rho
      hipLaunchKernelGGL(k_cg_direction, dim3(G), dim3(WG), 0, ctx->stream, S->n, scal, S->q, S->p); // p = beta p + q
    }
    DDMCHECK(ddm_op_apply(ctx, S->op, S->p, S->q));                                          // q = A p
    DDMCHECK(dot_device(ctx, S->n, S->op->owner, S->p, S->q, scal + SCAL_PQ));               // alpha = <p, q>
    hipLaunchKernelGGL(k_cg_lambda, dim3(1), dim3(1), 0, ctx->stream, scal);                 // lambda = rholast / alpha
    { // x += lambda p; b -= lambda q; def^2 = <b, b> (partial sums in the same kernel)
      const int nb = grid_for(S->n, WG * 4, RED_MAX_BLOCKS);
      if (S->op->owner)
        hipLaunchKernelGGL(k_cg_update_norm<true>, dim3(nb), dim3(WG), 0, ctx->stream, S->n, scal, S->op->owner, S->p, S->q, S->x, S->b, ctx->partial);
      else
        hipLaunchKernelGGL(k_cg_update_norm<false>, dim3(nb), dim3(WG), 0, ctx->stream, S->n, scal, S->op->owner, S->p, S->q, S->x, S->b, ctx->partial);
      hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(WG), 0, ctx->stream, nb, ctx->partial, scal + SCAL_DEF2);
      // The rank-local sum is complete; its all-reduce rides on the coarse-defect all-reduce of the NEXT iteration's preconditioner
      // (one RCCL launch saved per iteration) unless this is the chunk's last iteration -- whoever reads the defect (ddm_cg_defect)
      // needs it now -- or there is no coarse level to ride on.
      rider = i + 1 < k && S->prec->galerkin ? scal + SCAL_DEF2 : nullptr;
      if (!rider) DDMCHECK(ctx_allreduce(ctx, scal + SCAL_DEF2, 1, "scalar product"));
    }
    S->it += 1;
  }
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_cg_defect(ddm_ctx *ctx, ddm_cg *S, double *def_host) // synchronous
{
  double bb = 0.0;
  DDMCHECK(ddm_memcpy_d2h(ctx, &bb, ctx->scal + SCAL_DEF2, sizeof(double)));
  *def_host = std::sqrt(bb);
  (void)S;
  return DDM_OK;
}

extern "C" int ddm_cg_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit,
                            int fixed_iterations, double *hist_host, ddm_solve_result *res)
{
  if (!res) return fail(ctx, DDM_EINVAL, "ddm_cg_solve: bad arguments");
  ddm_cg *S = nullptr;
  DDMCHECK(ddm_cg_begin(ctx, op, prec, x, b, &S));
  const double def0 = S->def0;
  solve_result_reset(res);
  res->def0 = def0;
  if (hist_host) hist_host[0] = def0;
  if (const Defect0 d = classify_initial_defect(def0); d != Defect0::Go) {
    ddm_cg_end(ctx, S);
    if (d == Defect0::NaN) return fail(ctx, DDM_ENUMERIC, "initial defect is NaN");
    res->converged = 1;
    return DDM_OK;
  }
  (void)hipStreamSynchronize(ctx->stream);
  const auto t0 = std::chrono::steady_clock::now();
  int rc = DDM_OK;
  double deff = def0;
  if (fixed_iterations > 0 && !hist_host) {
    rc = ddm_cg_steps(ctx, S, fixed_iterations);
    if (!rc) rc = ddm_cg_defect(ctx, S, &deff);
    res->iterations = fixed_iterations;
  } else {
    const int iters = fixed_iterations > 0 ? fixed_iterations : maxit;
    for (int i = 1; i <= iters && !rc; ++i) {
      rc = ddm_cg_steps(ctx, S, 1);
      if (!rc) rc = ddm_cg_defect(ctx, S, &deff); // the Krylov loop tests the defect every iteration
      if (rc) break;
      res->iterations = i;
      if (hist_host) hist_host[i] = deff;
      if (!(deff == deff)) {
        rc = fail(ctx, DDM_ENUMERIC, "defect is NaN in iteration %d", i);
        break;
      }
      if (fixed_iterations <= 0 && (deff < def0 * reduction || deff < 1e-30)) {
        res->converged = 1;
        break;
      }
    }
  }
  rc = krylov_finish(ctx, prec, rc, t0, &res->elapsed_s);
  res->reduction = deff / def0;
  ddm_cg_end(ctx, S);
  return rc;
}

// ---- CG for m right-hand sides ---------------------------------------------------------------------------------------------------------
// m independent CGSolver::apply recurrences (the loop of ddm_cg_solve per column).  A column whose defect passed the test is frozen by
// the device-side mask ctx->mactive: its x, defect, scalars and history stop changing while the other columns go on.  Per iteration
// the host reads the m squared defects once (one all-reduce of m doubles each for <q, b>, <p, q> and <b, b>; no deferred norm).
static int cg_multi_step(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int m, bool first, double *X, double *B, double *P, double *Q)
{
  double *scal = ctx->mscal;
  const int64_t n = op->n;
  DDMCHECK(combined_apply_multi_impl(ctx, prec, m, first ? P : Q, B));                                       // q = M^-1 b (p on the first step)
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, first ? P : Q, B, scal + (first ? SCAL_RHOLAST : SCAL_RHO) * MULTI_MAX)); // rho = <q, b>
  if (!first) {
    hipLaunchKernelGGL(k_cg_beta_multi, dim3(1), dim3(64), 0, ctx->stream, m, (const int32_t *)ctx->mactive, scal); // beta = rho / rholast
    hipLaunchKernelGGL(k_cg_direction_multi, dim3(grid_for(n * m)), dim3(WG), 0, ctx->stream, n, m, (const int32_t *)ctx->mactive, (const double *)scal,
                       (const double *)Q, P); // p = beta p + q
  }
  DDMCHECK(op_apply_multi(ctx, op, m, P, Q));                                           // q = A p
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, P, Q, scal + SCAL_PQ * MULTI_MAX)); // alpha = <p, q>
  hipLaunchKernelGGL(k_cg_lambda_multi, dim3(1), dim3(64), 0, ctx->stream, m, (const int32_t *)ctx->mactive, scal); // lambda = rholast / alpha
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  for_column_groups(m, [&](int c0, int cb) { // x += lambda p; b -= lambda q; <b, b> partials
    DDM_MULTI_CB_DISPATCH(k_cg_update_norm_multi, op->owner != nullptr, cb, dim3(nb), dim3(WG), 0, ctx->stream, n, m, c0, (const int32_t *)ctx->mactive,
                          (const double *)scal, SCAL_STEP, (const uint8_t *)op->owner, (const double *)P, (const double *)Q, X, B, ctx->mpartial);
  });
  hipLaunchKernelGGL(k_reduce_final_multi, dim3(m), dim3(WG), 0, ctx->stream, nb, (const double *)ctx->mpartial, scal + SCAL_DEF2 * MULTI_MAX);
  HIPCHECK(ctx, hipGetLastError());
  return ctx_allreduce(ctx, scal + SCAL_DEF2 * MULTI_MAX, m, "defect norms");
}
extern "C" int ddm_cg_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit,
                                  double *hist_host, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !X || !B || !res || X == B || maxit < 0) return fail(ctx, DDM_EINVAL, "ddm_cg_solve_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_cg_solve_multi"));
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  const int m = nrhs;
  const int64_t n = op->n;
  for (int c = 0; c < m; ++c) solve_result_reset(&res[c]);
  DDMCHECK(ctx_multi_scratch(ctx));
  HIPCHECK(ctx, prec->work.reserve(m, n, 2));
  double *P = prec->work.block[0], *Q = prec->work.block[1]; // search directions p, q
  double bb[MULTI_MAX];
  MultiFrame f{ctx, "ddm_cg_solve_multi", m, reduction, hist_host, res};
  DDMCHECK(op_applyscaleadd_multi(ctx, op, m, -1.0, X, B)); // prec.pre(x, b); b -= A x
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, B, B, ctx->mscal + SCAL_DEF2 * MULTI_MAX));
  DDMCHECK(ddm_memcpy_d2h(ctx, bb, ctx->mscal + SCAL_DEF2 * MULTI_MAX, sizeof(double) * (size_t)m));
  DDMCHECK(multi_start(f, bb));
  (void)hipStreamSynchronize(ctx->stream);
  const auto t0 = std::chrono::steady_clock::now();
  int rc = DDM_OK;
  for (int i = 1; i <= maxit && f.nactive > 0 && !rc; ++i) {
    rc = cg_multi_step(ctx, op, prec, m, i == 1, X, B, P, Q);
    if (!rc) rc = ddm_memcpy_d2h(ctx, bb, ctx->mscal + SCAL_DEF2 * MULTI_MAX, sizeof(double) * (size_t)m); // the defects are tested every iteration
    for (int c = 0; c < m && !rc; ++c)
      if (f.active[c]) rc = multi_record(f, c, i, std::sqrt(bb[c]));
    if (!rc && f.nactive > 0) rc = multi_upload_mask(f);
  }
  return multi_finish(f, prec, rc, t0);
}

// ---- CG for any number of right-hand sides through a block of fixed width ------------------------------------------------------------
// ncols columns queue for the `width` slots of one block loop: the loop of ddm_cg_solve_multi (cg_multi_step, MultiFrame, the mask)
// with a slot -> column table beside it.  Every column is what ddm_cg_solve_multi computes on it -- its own def0, stop test, iteration
// counter and maxit.  X and B are the caller's n x ncols blocks; the recurrences run in n x width work blocks (x, defect, p, q), so B
// is only read.  After the defects of an iteration are read, at the iteration boundary:
//   store   every slot whose column stopped (converged, or maxit reached) scatters its x into X[:, column] (k_column_store_multi);
//   refill  the slots freed in this iteration take the next columns of the queue, in ascending slot order, in one launch of
//           k_column_load_multi (x = X[:, j], defect = B[:, j], p = 0, rholast = 1: the slot's next direction is p = beta * 0 + q = q);
//   defect  one block operator apply T = A x and k_defect_norm_multi (defect -= T and its norms) under a mask of the refilled slots
//           only: the running slots' defects are not touched.  A refilled column with def0 < 1e-30 (or maxit = 0) is finished at
//           once and its slot refilled again at the same boundary (at most ncols passes); then the loop mask is restored.
// With the queue empty a freed slot is frozen as in ddm_cg_solve_multi.  Every step is the "not first" step of cg_multi_step: a fresh
// slot has p = 0 and a finite beta, so no step is special and the slots need not be aligned.  A NaN ends the call with DDM_ENUMERIC:
// the columns stored before keep their results, X[:, j] of the others is as on entry.
extern "C" int ddm_cg_solve_queue(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int64_t ncols, int width, double *X, double *B, double reduction,
                                  int maxit, double *hist_host, ddm_solve_result *res)
{
  const char *what = "ddm_cg_solve_queue";
  if (width < 1 || width > MULTI_MAX) return fail(ctx, DDM_EINVAL, "%s: width = %d outside [1, %d]", what, width, MULTI_MAX);
  if (ncols < 1) return fail(ctx, DDM_EINVAL, "%s: ncols = %lld, at least one column is needed", what, (long long)ncols);
  if (!ctx || !op || !prec || !X || !B || !res || X == B || maxit < 0) return fail(ctx, DDM_EINVAL, "%s: bad arguments", what);
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  const int w = width;
  const int64_t n = op->n;
  for (int64_t j = 0; j < ncols; ++j) solve_result_reset(&res[j]);
  DDMCHECK(ctx_multi_scratch(ctx));
  HIPCHECK(ctx, prec->work.reserve(w, n, 4));
  StreamDrain drain{ctx}; // every return waits for the kernels that read the caller's blocks
  double *P = prec->work.block[0], *Q = prec->work.block[1], *XW = prec->work.block[2], *BW = prec->work.block[3]; // directions p, q; the slots' x and defect
  int64_t *tabdev = prec->work.tab; // (slot, column) pairs of one load or store launch
  if (n > 0) // a slot that never holds a column stays zero
    for (double *blk : {P, XW, BW}) HIPCHECK(ctx, hipMemsetAsync(blk, 0, sizeof(double) * (size_t)(n * w), ctx->stream));
  double *bbdev = ctx->mscal + SCAL_DEF2 * MULTI_MAX;
  double bb[MULTI_MAX];
  ddm_solve_result sres[MULTI_MAX]; // the slots' results: MultiFrame works on these, a stored column's entry is copied to res
  int64_t column[MULTI_MAX], tab[2 * MULTI_MAX];
  int32_t mask[MULTI_MAX];
  for (int s = 0; s < w; ++s) solve_result_reset(&sres[s]), column[s] = -1;
  MultiFrame f{ctx, what, w, reduction, nullptr, sres};
  f.column = column;
  std::fill(f.active, f.active + w, 0);
  int64_t next = 0; // head of the queue
  auto hist = [&](int64_t j, int it, double def) {
    if (hist_host) hist_host[(int64_t)it * ncols + j] = def;
  };
  auto upload_table = [&](int npairs) { return ddm_memcpy_h2d(ctx, tabdev, tab, sizeof(int64_t) * 2 * (size_t)npairs); };
  // slot s is done with its column: the result entry goes to the caller (x has been stored, or never changed)
  auto release = [&](int s) {
    ddm_solve_result &r = res[column[s]] = sres[s];
    if (r.def0 >= 1e-30) r.reduction = f.def[s] / r.def0;
    column[s] = -1;
  };
  // the free slots take the next columns of the queue; leaves the loop mask on the device
  auto refill = [&]() -> int {
    for (int64_t pass = 0; pass < ncols && next < ncols; ++pass) {
      int nload = 0;
      std::fill(mask, mask + w, 0);
      for (int s = 0; s < w && next < ncols; ++s) {
        if (column[s] >= 0) continue;
        tab[2 * nload] = s, tab[2 * nload + 1] = column[s] = next++;
        mask[s] = 1;
        ++nload;
      }
      if (nload == 0) break;
      DDMCHECK(upload_table(nload));
      hipLaunchKernelGGL(k_column_load_multi, dim3(grid_for(n * nload)), dim3(WG), 0, ctx->stream, n, w, nload, (const int64_t *)tabdev, ncols, (const double *)X,
                         (const double *)B, XW, BW, P, ctx->mscal);
      HIPCHECK(ctx, hipGetLastError());
      DDMCHECK(ddm_memcpy_h2d(ctx, ctx->mactive, mask, sizeof(int32_t) * (size_t)w)); // the defect pass writes the loaded slots only
      DDMCHECK(op_apply_multi(ctx, op, w, XW, Q));                                     // t = A x (q is free between two iterations)
      DDMCHECK(defect_norm_multi(ctx, op, w, Q, BW, bbdev));                         // prec.pre(x, b); b -= t; <b, b>
      DDMCHECK(ddm_memcpy_d2h(ctx, bb, bbdev, sizeof(double) * (size_t)w));
      for (int k = 0; k < nload; ++k) {
        const int s = (int)tab[2 * k];
        solve_result_reset(&sres[s]);
        const double def0 = f.def[s] = std::sqrt(bb[s]);
        sres[s].def0 = def0;
        hist(column[s], 0, def0);
        const Defect0 d = classify_initial_defect(def0);
        if (d == Defect0::NaN) return fail(ctx, DDM_ENUMERIC, "%s: initial defect is NaN in column %lld", what, (long long)column[s]);
        if (d == Defect0::Zero) sres[s].converged = 1;
        if (d == Defect0::Zero || maxit == 0) { // needs no iteration, or gets none: x stays as it is in X
          release(s);
          continue;
        }
        f.active[s] = 1;
        f.nactive += 1;
      }
    }
    f.changed = true;
    return multi_upload_mask(f);
  };
  int rc = refill();
  (void)hipStreamSynchronize(ctx->stream);
  const auto t0 = std::chrono::steady_clock::now();
  while (f.nactive > 0 && !rc) {
    rc = cg_multi_step(ctx, op, prec, w, false, XW, BW, P, Q);
    if (!rc) rc = ddm_memcpy_d2h(ctx, bb, bbdev, sizeof(double) * (size_t)w); // the defects are tested every iteration
    int nstore = 0;
    for (int s = 0; s < w && !rc; ++s) {
      if (!f.active[s]) continue;
      const int it = sres[s].iterations + 1;
      rc = multi_record(f, s, it, std::sqrt(bb[s]));
      hist(column[s], it, f.def[s]);
      if (!rc && f.active[s] && it >= maxit) { // out of iterations: leaves its slot unconverged
        f.active[s] = 0;
        f.nactive -= 1;
        f.changed = true;
      }
      if (!rc && !f.active[s]) tab[2 * nstore] = s, tab[2 * nstore + 1] = column[s], ++nstore;
    }
    if (rc) break;
    if (nstore > 0) {
      rc = upload_table(nstore);
      if (rc) break;
      hipLaunchKernelGGL(k_column_store_multi, dim3(grid_for(n * nstore)), dim3(WG), 0, ctx->stream, n, w, nstore, (const int64_t *)tabdev, ncols, (const double *)XW, X);
      rc = launch_check(ctx, what);
      if (rc) break;
      for (int k = 0; k < nstore; ++k) release((int)tab[2 * k]);
    }
    rc = nstore > 0 && next < ncols ? refill() : multi_upload_mask(f);
  }
  if (!rc) rc = launch_check(ctx, what);
  rc = multi_finish(f, prec, rc, t0); // (drains the stream; the elapsed time of the call lands in the slots' entries)
  for (int64_t j = 0; j < ncols; ++j) res[j].elapsed_s = sres[0].elapsed_s;
  return rc;
}
