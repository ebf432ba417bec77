// Flexible CG, restarted and complete, for one and for m right-hand sides.  Needs krylov_frame.hpp.
#pragma once

// ---- flexible CG, restarted and complete ---------------------------------------------------------------------------------------------
// dune-istl RestartedFCGSolver::apply and CompleteFCGSolver::apply ([solver] type = restartedfcgsolver / completefcgsolver; DUNE 2.10
// solvers.hh, not in the snapshot -- restated in include/ddm_hip.h and in tests/fcg_reference.py): CG for a symmetric positive definite
// operator whose preconditioner is not symmetric or not fixed.  Slots 0 .. mmax hold a direction d_s, its image Ad_s and
// g_s = <d_s, Ad_s>; a fresh direction d_s = M^-1 b is A-orthogonalised against a window J of stored slots by classical Gram-Schmidt
// (all coefficients <Ad_k, d_s> / g_k from the unmodified d_s), then x += alpha d_s, b -= alpha Ad_s with alpha = <d_s, b> / g_s and
// the true defect |b| is tested.  The variants differ in the window and in what the end of a pass over the slots does:
//                  restarted                                       complete
//   window J       {0 .. s - 1}                                    {k < klimit, k != s}; then klimit grows to s + 1
//   end of a pass  slot 0 <-> slot mmax (d, Ad, g), s = 1          s = 0, klimit = mmax + 1: the stale higher slots stay in the window
// One loop per vector count (fcg_loop, fcg_loop_multi) carries the variant as a flag.  Slots are addressed through a table slot ->
// buffer (the swap exchanges two table entries; g is stored per buffer), and a window travels to the kernels as FcgSet chunks of buffer
// indices.  The orthogonalisation is two kernels around ONE all-reduce of the |J| (x m) numerators: k_fcg_project(_multi) reads d_s once
// per FCG_SG1 (FCG_SG) slots, k_fcg_orth(_multi) is one read-modify-write of d_s.  alpha and g stay on the device; the host reads the
// squared defect per iteration (and column), as CG does.  No more than min(mmax, max(maxit, 1)) + 1 slots are ever touched.
static void fcg_window(bool complete, int s, int &klimit, const std::vector<int> &buf, std::vector<int> &J)
{
  J.clear();
  if (!complete) {
    for (int k = 0; k < s; ++k) J.push_back(buf[k]);
    return;
  }
  for (int k = 0; k < klimit; ++k)
    if (k != s) J.push_back(buf[k]);
  if (klimit <= s) ++klimit;
}
static FcgSet fcg_set(const std::vector<int> &J, int j0, int cap)
{
  FcgSet set{};
  set.n = std::min<int>(cap, (int)J.size() - j0);
  for (int j = 0; j < set.n; ++j) set.buf[j] = J[j0 + j];
  return set;
}
// d -= sum_{k in J} (<Ad_k, d> / g_k) d_k for one vector; J: buffer indices into AD / D (vectors at `stride`), g per buffer; num, coef:
// |J| device doubles each (the coefficients stay in coef), part: |J| x nb doubles
static int fcg_orthogonalise(ddm_ctx *ctx, ddm_op *op, const double *AD, const double *D, int64_t stride, const std::vector<int> &J, const double *g,
                             double *num, double *coef, double *part, double *d)
{
  const int nJ = (int)J.size();
  if (nJ == 0) return DDM_OK;
  ScopedTimer t(ctx, "FCG/orthogonalisation");
  const int64_t n = op->n;
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  for (int j0 = 0; j0 < nJ; j0 += FCG_SG1) {
    const FcgSet set = fcg_set(J, j0, FCG_SG1);
    if (op->owner) hipLaunchKernelGGL(k_fcg_project<true>, dim3(nb), dim3(WG), 0, ctx->stream, n, (const uint8_t *)op->owner, AD, stride, set, j0, (const double *)d, part);
    else hipLaunchKernelGGL(k_fcg_project<false>, dim3(nb), dim3(WG), 0, ctx->stream, n, (const uint8_t *)op->owner, AD, stride, set, j0, (const double *)d, part);
  }
  hipLaunchKernelGGL(k_reduce_final_multi, dim3(nJ), dim3(WG), 0, ctx->stream, nb, (const double *)part, num);
  HIPCHECK(ctx, hipGetLastError());
  DDMCHECK(ctx_allreduce(ctx, num, nJ, "Gram-Schmidt coefficients"));
  for (int j0 = 0; j0 < nJ; j0 += FCG_SET_MAX) {
    const FcgSet set = fcg_set(J, j0, FCG_SET_MAX);
    hipLaunchKernelGGL(k_fcg_coef, dim3(1), dim3(64), 0, ctx->stream, set, j0, (const double *)num, g, coef);
    hipLaunchKernelGGL(k_fcg_orth, dim3(grid_for(n)), dim3(WG), 0, ctx->stream, n, D, stride, set, j0, (const double *)coef, d);
  }
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}

// the loop for one right-hand side; what: the exported function's name, for messages
static int fcg_loop(ddm_ctx *ctx, const char *what, bool complete, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit,
                    int mmax, double *hist_host, ddm_solve_result *res)
{
  const int64_t n = op->n, stride = std::max<int64_t>(n, 1);
  const int M = std::min(mmax, std::max(maxit, 1)); // slots 0 .. M: a pass never gets longer than maxit iterations
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  DDMCHECK(gmres_memory_check(ctx, what, 2 * ((int64_t)M + 1), n, 1));
  solve_result_reset(res);
  dbuf<double> Db, ADb, part, sdev; // sdev: g per buffer [0, M + 1), numerators [M], coefficients [M], <d, Ad> and <d, b> [2]
  HIPCHECK(ctx, Db.alloc(stride * (M + 1)));
  HIPCHECK(ctx, ADb.alloc(stride * (M + 1)));
  HIPCHECK(ctx, part.alloc((int64_t)std::max(M, 2) * nb));
  HIPCHECK(ctx, sdev.alloc(3 * (int64_t)M + 3));
  StreamDrain drain{ctx}; // (declared after the buffers: from here on every return waits for the stream before they are released)
  double *D = Db, *AD = ADb, *g = sdev, *num = sdev + (M + 1), *coef = num + M, *dots = coef + M, *scal = ctx->scal;
  HIPCHECK(ctx, hipMemsetAsync(sdev, 0, sizeof(double) * (size_t)(3 * M + 3), ctx->stream));
  double bb = 0.0;
  DDMCHECK(ddm_op_applyscaleadd(ctx, op, -1.0, x, b)); // b -= A x
  DDMCHECK(dot_device(ctx, n, op->owner, b, b, scal + SCAL_DEF2));
  DDMCHECK(ddm_memcpy_d2h(ctx, &bb, scal + SCAL_DEF2, sizeof(double)));
  const double def0 = std::sqrt(bb);
  res->def0 = def0;
  if (hist_host) hist_host[0] = def0;
  if (const Defect0 d0 = classify_initial_defect(def0); d0 != Defect0::Go) {
    if (d0 == Defect0::NaN) return fail(ctx, DDM_ENUMERIC, "%s: initial defect is NaN", what);
    res->converged = 1;
    return DDM_OK;
  }
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<int> buf(M + 1), J;
  for (int k = 0; k <= M; ++k) buf[k] = k;
  int rc = DDM_OK, i = 1, s = 0, klimit = 0;
  bool stop = false;
  double def = def0;
  while (i <= maxit && !stop && !rc) {
    for (; s <= M && i <= maxit && !stop; ++i, ++s) {
      double *ds = D + (int64_t)buf[s] * stride, *ads = AD + (int64_t)buf[s] * stride;
      rc = ddm_combined_apply(ctx, prec, ds, b);                                             // d_s = M^-1 b
      fcg_window(complete, s, klimit, buf, J);
      if (!rc) rc = fcg_orthogonalise(ctx, op, AD, D, stride, J, g, num, coef, part, ds);    // d_s -= sum_J (<Ad_k, d_s> / g_k) d_k
      if (!rc) rc = ddm_op_apply(ctx, op, ds, ads);                                          // Ad_s = A d_s
      if (rc) break;
      if (op->owner) hipLaunchKernelGGL(k_fcg_dots<true>, dim3(nb), dim3(WG), 0, ctx->stream, n, (const uint8_t *)op->owner, (const double *)ds, (const double *)ads, (const double *)b, part);
      else hipLaunchKernelGGL(k_fcg_dots<false>, dim3(nb), dim3(WG), 0, ctx->stream, n, (const uint8_t *)op->owner, (const double *)ds, (const double *)ads, (const double *)b, part);
      hipLaunchKernelGGL(k_reduce_final_multi, dim3(2), dim3(WG), 0, ctx->stream, nb, (const double *)part, dots); // g_s = <d_s, Ad_s>, <d_s, b>
      rc = ctx_allreduce(ctx, dots, 2, "scalar products");
      if (rc) break;
      hipLaunchKernelGGL(k_fcg_alpha, dim3(1), dim3(1), 0, ctx->stream, (const double *)dots, g + buf[s], scal);   // alpha = <d_s, b> / g_s
      if (op->owner) // x += alpha d_s; b -= alpha Ad_s; <b, b>
        hipLaunchKernelGGL(k_cg_update_norm<true>, dim3(nb), dim3(WG), 0, ctx->stream, n, (const double *)scal, (const uint8_t *)op->owner, (const double *)ds, (const double *)ads, x, b, ctx->partial);
      else
        hipLaunchKernelGGL(k_cg_update_norm<false>, dim3(nb), dim3(WG), 0, ctx->stream, n, (const double *)scal, (const uint8_t *)op->owner, (const double *)ds, (const double *)ads, x, b, ctx->partial);
      hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(WG), 0, ctx->stream, nb, ctx->partial, scal + SCAL_DEF2);
      rc = ctx_allreduce(ctx, scal + SCAL_DEF2, 1, "scalar product");
      if (!rc) rc = ddm_memcpy_d2h(ctx, &bb, scal + SCAL_DEF2, sizeof(double)); // the one read-back of the iteration
      if (rc) break;
      def = std::sqrt(bb);
      res->iterations = i;
      if (hist_host) hist_host[i] = def;
      if (!(def == def)) {
        rc = fail(ctx, DDM_ENUMERIC, "%s: defect is NaN in iteration %d (<d, A d> == 0, or a NaN in the recurrence)", what, i);
        break;
      }
      if (def < def0 * reduction || def < 1e-30) stop = true;
    }
    if (rc || s <= M) break; // (an error, the stop or maxit inside the pass)
    if (complete) {
      s = 0;
      klimit = M + 1;
    } else {
      std::swap(buf[0], buf[M]);
      s = 1;
    }
  }
  if (!rc) rc = launch_check(ctx, what);
  rc = krylov_finish(ctx, prec, rc, t0, &res->elapsed_s);
  res->converged = stop ? 1 : 0;
  res->reduction = def / def0;
  return rc;
}

extern "C" int ddm_fcg_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit, int mmax, int complete,
                             double *hist_host, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !x || !b || !res || x == b || maxit < 0 || mmax < 1) return fail(ctx, DDM_EINVAL, "ddm_fcg_solve: bad arguments");
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  return fcg_loop(ctx, "ddm_fcg_solve", complete != 0, op, prec, x, b, reduction, maxit, mmax, hist_host, res);
}

// ---- flexible CG for m right-hand sides ----------------------------------------------------------------------------------------------------
// m independent fcg_loop recurrences: every column shares the slot index s, the window and the slot table (none depends on data); a
// column stops on its own test and is then frozen through ctx->mactive (MultiFrame): no kernel of the loop writes its x, its defect or
// its g afterwards; the operator and the preconditioner still run on its direction entries, which nobody reads.
// The orthogonalisation of the block W against the window J (buffer indices into AD / D, blocks at `stride`; g: m doubles per buffer;
// num, coef: |J| x m device doubles, the coefficients stay in coef; part: |J| x m x nb doubles).  fused: k_fcg_project_multi, ONE
// all-reduce, k_fcg_orth_multi; not fused: the composition they replace, dot_multi_device per slot on the unmodified W, then
// k_axpy_negdev_multi per slot.  Bit-identical.
static int fcg_orthogonalise_multi(ddm_ctx *ctx, ddm_op *op, int m, bool fused, const double *AD, const double *D, int64_t stride, const std::vector<int> &J,
                                   const double *g, double *num, double *coef, double *part, double *W)
{
  const int nJ = (int)J.size();
  if (nJ == 0) return DDM_OK;
  ScopedTimer t(ctx, "FCG/orthogonalisation");
  const int64_t n = op->n;
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  const int32_t *active = ctx->mactive;
  if (fused) {
    for (int j0 = 0; j0 < nJ; j0 += FCG_SG) {
      const FcgSet set = fcg_set(J, j0, FCG_SG);
      for_column_groups(m, [&](int c0, int cb) {
        DDM_MULTI_CB_DISPATCH(k_fcg_project_multi, op->owner != nullptr, cb, dim3(nb), dim3(WG), 0, ctx->stream, n, m, c0, (const uint8_t *)op->owner, AD, stride,
                              set, j0, (const double *)W, part);
      });
    }
    hipLaunchKernelGGL(k_reduce_final_multi, dim3(nJ * m), dim3(WG), 0, ctx->stream, nb, (const double *)part, num);
    HIPCHECK(ctx, hipGetLastError());
    DDMCHECK(ctx_allreduce(ctx, num, (int64_t)nJ * m, "Gram-Schmidt coefficients"));
  } else {
    for (int j = 0; j < nJ; ++j) DDMCHECK(dot_multi_device(ctx, n, op->owner, m, AD + (int64_t)J[j] * stride, W, num + (int64_t)j * m));
  }
  for (int j0 = 0; j0 < nJ; j0 += FCG_SET_MAX) {
    const FcgSet set = fcg_set(J, j0, FCG_SET_MAX);
    hipLaunchKernelGGL(k_fcg_coef_multi, dim3((set.n * m + WG - 1) / WG), dim3(WG), 0, ctx->stream, m, active, set, j0, (const double *)num, g, coef);
    if (fused) {
      hipLaunchKernelGGL(k_fcg_orth_multi, dim3(grid_for(n * m)), dim3(WG), 0, ctx->stream, n, m, active, D, stride, set, j0, (const double *)coef, W);
      continue;
    }
    for (int j = 0; j < set.n; ++j)
      hipLaunchKernelGGL(k_axpy_negdev_multi, dim3(grid_for(n * m)), dim3(WG), 0, ctx->stream, n, m, active, (const double *)(coef + (int64_t)(j0 + j) * m),
                         D + (int64_t)set.buf[j] * stride, W);
  }
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}

// One orthogonalisation on its own, for tests: the block W against the nslots stored blocks DS (directions) and AD (their images),
// consecutive n x nrhs blocks, with g_host[k * nrhs + c] = <d_k, Ad_k>; W -= sum_k (<Ad_k, W> / g_k) d_k in the columns with
// active_host[c] != 0 (the others are not written), coef_host[k * nrhs + c] = the coefficients (0 in the other columns).  fused != 0:
// the kernels the drivers use; fused == 0: the composition they replace.  Synchronous.
extern "C" int ddm_fcg_orth_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, int nslots, const int32_t *active_host, const double *AD, const double *DS,
                                  const double *g_host, double *W, int fused, double *coef_host)
{
  if (!ctx || !op || !active_host || !W || nslots < 0 || (nslots > 0 && (!AD || !DS || !g_host || !coef_host || AD == W || DS == W)))
    return fail(ctx, DDM_EINVAL, "ddm_fcg_orth_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_fcg_orth_multi"));
  DDMCHECK(ctx_multi_scratch(ctx));
  const int m = nrhs;
  const int64_t n = op->n, stride = std::max<int64_t>(n, 1) * m;
  DDMCHECK(ddm_memcpy_h2d(ctx, ctx->mactive, active_host, sizeof(int32_t) * (size_t)m));
  if (nslots == 0) return DDM_OK;
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  const int64_t km = (int64_t)nslots * m;
  dbuf<double> sdev, part; // sdev: g, numerators, coefficients
  HIPCHECK(ctx, sdev.alloc(3 * km));
  HIPCHECK(ctx, part.alloc(km * nb));
  StreamDrain drain{ctx};
  DDMCHECK(ddm_memcpy_h2d(ctx, sdev, g_host, sizeof(double) * (size_t)km));
  std::vector<int> J(nslots);
  for (int k = 0; k < nslots; ++k) J[k] = k;
  DDMCHECK(fcg_orthogonalise_multi(ctx, op, m, fused != 0, AD, DS, stride, J, sdev, sdev + km, sdev + 2 * km, part, W));
  return ddm_memcpy_d2h(ctx, coef_host, sdev + 2 * km, sizeof(double) * (size_t)km);
}

// the loop for m right-hand sides; what: the exported function's name, for messages
static int fcg_loop_multi(ddm_ctx *ctx, const char *what, bool complete, ddm_op *op, ddm_combined *prec, int m, double *X, double *B, double reduction,
                          int maxit, int mmax, double *hist_host, ddm_solve_result *res)
{
  const int64_t n = op->n, stride = std::max<int64_t>(n, 1) * m;
  const int M = std::min(mmax, std::max(maxit, 1)); // slots 0 .. M: a pass never gets longer than maxit iterations
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  DDMCHECK(gmres_memory_check(ctx, what, 2 * ((int64_t)M + 1), n, m));
  for (int c = 0; c < m; ++c) solve_result_reset(&res[c]);
  DDMCHECK(ctx_multi_scratch(ctx));
  dbuf<double> Db, ADb, part, sdev; // sdev: g per buffer [(M + 1) m], numerators [M m], coefficients [M m], <d, Ad> and <d, b> [2 m]
  HIPCHECK(ctx, Db.alloc(stride * (M + 1)));
  HIPCHECK(ctx, ADb.alloc(stride * (M + 1)));
  HIPCHECK(ctx, part.alloc((int64_t)M * m * nb));
  HIPCHECK(ctx, sdev.alloc((3 * (int64_t)M + 3) * m));
  StreamDrain drain{ctx}; // (declared after the buffers: from here on every return waits for the stream before they are released)
  double *D = Db, *AD = ADb, *g = sdev, *num = g + (int64_t)(M + 1) * m, *coef = num + (int64_t)M * m, *dots = coef + (int64_t)M * m, *scal = ctx->mscal;
  const int32_t *active = ctx->mactive;
  HIPCHECK(ctx, hipMemsetAsync(sdev, 0, sizeof(double) * (size_t)((3 * (int64_t)M + 3) * m), ctx->stream));
  double bb[MULTI_MAX];
  MultiFrame f{ctx, what, m, reduction, hist_host, res};
  DDMCHECK(op_applyscaleadd_multi(ctx, op, m, -1.0, X, B)); // b -= A x
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, B, B, scal + SCAL_DEF2 * MULTI_MAX));
  DDMCHECK(ddm_memcpy_d2h(ctx, bb, scal + SCAL_DEF2 * MULTI_MAX, sizeof(double) * (size_t)m));
  DDMCHECK(multi_start(f, bb));
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<int> buf(M + 1), J;
  for (int k = 0; k <= M; ++k) buf[k] = k;
  int rc = DDM_OK, i = 1, s = 0, klimit = 0;
  while (i <= maxit && f.nactive > 0 && !rc) {
    for (; s <= M && i <= maxit && f.nactive > 0; ++i, ++s) {
      double *ds = D + (int64_t)buf[s] * stride, *ads = AD + (int64_t)buf[s] * stride;
      rc = combined_apply_multi_impl(ctx, prec, m, ds, B);                                                   // d_s = M^-1 b
      fcg_window(complete, s, klimit, buf, J);
      if (!rc) rc = fcg_orthogonalise_multi(ctx, op, m, true, AD, D, stride, J, g, num, coef, part, ds);     // d_s -= sum_J (<Ad_k, d_s> / g_k) d_k
      if (!rc) rc = op_apply_multi(ctx, op, m, ds, ads);                                                     // Ad_s = A d_s
      if (rc) break;
      for_column_groups(m, [&](int c0, int cb) { // g_s = <d_s, Ad_s> and <d_s, b> in one pass
        DDM_MULTI_CB_DISPATCH(k_fcg_dots_multi, op->owner != nullptr, cb, dim3(nb), dim3(WG), 0, ctx->stream, n, m, c0, active, (const uint8_t *)op->owner,
                              (const double *)ds, (const double *)ads, (const double *)B, ctx->mpartial);
      });
      hipLaunchKernelGGL(k_reduce_final_multi, dim3(2 * m), dim3(WG), 0, ctx->stream, nb, (const double *)ctx->mpartial, dots);
      rc = ctx_allreduce(ctx, dots, 2 * m, "scalar products");
      if (rc) break;
      hipLaunchKernelGGL(k_fcg_alpha_multi, dim3(1), dim3(64), 0, ctx->stream, m, active, (const double *)dots, g + (int64_t)buf[s] * m, scal); // alpha = <d_s, b> / g_s
      for_column_groups(m, [&](int c0, int cb) { // x += alpha d_s; b -= alpha Ad_s; <b, b> partials
        DDM_MULTI_CB_DISPATCH(k_cg_update_norm_multi, op->owner != nullptr, cb, dim3(nb), dim3(WG), 0, ctx->stream, n, m, c0, active, (const double *)scal, SCAL_STEP,
                              (const uint8_t *)op->owner, (const double *)ds, (const double *)ads, X, B, ctx->mpartial);
      });
      hipLaunchKernelGGL(k_reduce_final_multi, dim3(m), dim3(WG), 0, ctx->stream, nb, (const double *)ctx->mpartial, scal + SCAL_DEF2 * MULTI_MAX);
      rc = ctx_allreduce(ctx, scal + SCAL_DEF2 * MULTI_MAX, m, "defect norms");
      if (!rc) rc = ddm_memcpy_d2h(ctx, bb, scal + SCAL_DEF2 * MULTI_MAX, sizeof(double) * (size_t)m); // the one read-back of the iteration
      for (int c = 0; c < m && !rc; ++c)
        if (f.active[c]) rc = multi_record(f, c, i, std::sqrt(bb[c]));
      if (!rc && f.nactive > 0) rc = multi_upload_mask(f);
      if (rc) break;
    }
    if (rc || s <= M) break; // (an error, every column stopped, or maxit inside the pass)
    if (complete) {
      s = 0;
      klimit = M + 1;
    } else {
      std::swap(buf[0], buf[M]);
      s = 1;
    }
  }
  if (!rc) rc = launch_check(ctx, what);
  return multi_finish(f, prec, rc, t0);
}

extern "C" int ddm_fcg_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit, int mmax,
                                   int complete, double *hist_host, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !X || !B || !res || X == B || maxit < 0 || mmax < 1) return fail(ctx, DDM_EINVAL, "ddm_fcg_solve_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_fcg_solve_multi"));
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  return fcg_loop_multi(ctx, "ddm_fcg_solve_multi", complete != 0, op, prec, nrhs, X, B, reduction, maxit, mmax, hist_host, res);
}
