// Block CG: one shared search space for m right-hand sides, and its three passes on their own.  Needs krylov_frame.hpp.
#pragma once

// ---- block CG: one shared search space for m right-hand sides ---------------------------------------------------------------------------
// O'Leary's block CG with a pseudo-inverse in the m x m coupling (include/ddm_hip.h states the algorithm): unlike every other block
// driver of the library the columns are NOT independent -- each column's error is minimised over the span of all columns' Krylov
// spaces.  No column is frozen, so the driver uses neither ctx->mactive nor the record / mask part of the MultiFrame; what it keeps on
// the device it owns for the call (sdev, part) or borrows from the preconditioner object (P, Q, Z).
// The three passes over the blocks, each usable on its own (ddm_bcg_gram_multi, ddm_bcg_update_multi, ddm_bcg_direction_multi), run one
// workgroup per tile of rows up to RED_MAX_BLOCKS workgroups (what ctx->mpartial and the partial sums of a call are sized for):
static int bcg_grid(int64_t n, int tile_rows) { return grid_for(n, tile_rows, RED_MAX_BLOCKS); }
// G (device, m^2 doubles, with V2 2 m^2) = [U^T V1 | U^T V2] of THIS rank's owned rows; part: G's size x RED_MAX_BLOCKS doubles
static int bcg_gram_device(ddm_ctx *ctx, ddm_op *op, int m, const double *U, const double *V1, const double *V2, double *part, double *G)
{
  ScopedTimer t(ctx, "BCG/gram");
  const int nb = bcg_grid(op->n, BCG_TILE / ((m + 1) & ~1));
  const uint8_t *mask = op->owner;
  if (V2) {
    if (mask) hipLaunchKernelGGL((k_bcg_gram_partial<true, true>), dim3(nb), dim3(WG), 0, ctx->stream, op->n, m, mask, U, V1, V2, part);
    else hipLaunchKernelGGL((k_bcg_gram_partial<true, false>), dim3(nb), dim3(WG), 0, ctx->stream, op->n, m, mask, U, V1, V2, part);
  } else {
    if (mask) hipLaunchKernelGGL((k_bcg_gram_partial<false, true>), dim3(nb), dim3(WG), 0, ctx->stream, op->n, m, mask, U, V1, V2, part);
    else hipLaunchKernelGGL((k_bcg_gram_partial<false, false>), dim3(nb), dim3(WG), 0, ctx->stream, op->n, m, mask, U, V1, V2, part);
  }
  hipLaunchKernelGGL(k_reduce_final_multi, dim3((V2 ? 2 : 1) * m * m), dim3(WG), 0, ctx->stream, nb, (const double *)part, G);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
// X += P alpha; R -= Q alpha; norm2 (m device doubles) = this rank's owner-masked <R_c, R_c> afterwards.  alpha: m x m on the device.
static int bcg_update_device(ddm_ctx *ctx, ddm_op *op, int m, const double *alpha, const double *P, const double *Q, double *X, double *R, double *norm2)
{
  ScopedTimer t(ctx, "BCG/update");
  const int nb = bcg_grid(op->n, 4 * (WG / m));
  if (op->owner) hipLaunchKernelGGL(k_bcg_update_norm<true>, dim3(nb), dim3(WG), 0, ctx->stream, op->n, m, alpha, (const uint8_t *)op->owner, P, Q, X, R, ctx->mpartial);
  else hipLaunchKernelGGL(k_bcg_update_norm<false>, dim3(nb), dim3(WG), 0, ctx->stream, op->n, m, alpha, (const uint8_t *)op->owner, P, Q, X, R, ctx->mpartial);
  hipLaunchKernelGGL(k_reduce_final_multi, dim3(m), dim3(WG), 0, ctx->stream, nb, (const double *)ctx->mpartial, norm2);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
// P = Z + P beta.  beta: m x m on the device.
static int bcg_direction_device(ddm_ctx *ctx, ddm_op *op, int m, const double *beta, const double *Z, double *P)
{
  ScopedTimer t(ctx, "BCG/direction");
  hipLaunchKernelGGL(k_bcg_direction, dim3(bcg_grid(op->n, 4 * (WG / m))), dim3(WG), 0, ctx->stream, op->n, m, beta, Z, P);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
// C = sign A B for m x m row-major host matrices, the inner sum in ascending index (every rank forms the same coefficients)
static void bcg_small_product(int m, double sign, const double *A, const double *B, double *C)
{
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) {
      double s = 0.0;
      for (int k = 0; k < m; ++k) s += A[i * m + k] * B[k * m + j];
      C[i * m + j] = sign * s;
    }
}

extern "C" int ddm_bcg_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit,
                                   double rank_tol, double *hist_host, int32_t *rank_hist_host, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !X || !B || !res || X == B || maxit < 0 || !(rank_tol > 0.0 && rank_tol < 1.0))
    return fail(ctx, DDM_EINVAL, "ddm_bcg_solve_multi: bad arguments (null pointer, X == B, maxit < 0 or rank_tol outside (0, 1))");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_bcg_solve_multi"));
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  const int m = nrhs, mm = m * m;
  const int64_t n = op->n;
  for (int c = 0; c < m; ++c) solve_result_reset(&res[c]);
  DDMCHECK(ctx_multi_scratch(ctx));
  HIPCHECK(ctx, prec->work.reserve(m, n, 3));
  double *P = prec->work.block[0], *Q = prec->work.block[1], *Z = prec->work.block[2]; // P, Q = A P, Z = M^-1 R
  dbuf<double> sdev, part; // sdev: [W | S] (2 m^2), [Q^T Z | norms] (m^2 + m), alpha (m^2), beta (m^2)
  HIPCHECK(ctx, sdev.alloc(5 * mm + m));
  HIPCHECK(ctx, part.alloc((int64_t)2 * mm * RED_MAX_BLOCKS));
  StreamDrain drain{ctx}; // (declared after the buffers: from here on every return waits for the stream before they are released)
  double *ws = sdev, *zn = ws + 2 * mm, *alpha = zn + mm + m, *beta = alpha + mm;
  std::vector<double> h(2 * mm), Wp(mm), coef(mm);
  int first[MULTI_MAX]; // the first iteration at which the column passed its test, -1: not yet
  MultiFrame f{ctx, "ddm_bcg_solve_multi", m, reduction, hist_host, res};
  auto passes = [&](int c) { return f.def[c] < res[c].def0 * reduction || f.def[c] < 1e-30; };
  DDMCHECK(op_applyscaleadd_multi(ctx, op, m, -1.0, X, B)); // R = B - A X, in B
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, B, B, zn + mm));
  DDMCHECK(ddm_memcpy_d2h(ctx, h.data(), zn + mm, sizeof(double) * (size_t)m));
  int failing = 0;
  for (int c = 0; c < m; ++c) {
    const double def0 = f.def[c] = std::sqrt(h[c]);
    res[c].def0 = def0;
    if (hist_host) hist_host[c] = def0;
    const Defect0 d = classify_initial_defect(def0);
    if (d == Defect0::NaN) return fail(ctx, DDM_ENUMERIC, "ddm_bcg_solve_multi: initial defect is NaN in column %d", c);
    first[c] = d == Defect0::Zero ? 0 : -1; // (a column that needs no iteration stays in the block: its defect is exactly zero or negligible)
    failing += d == Defect0::Go;
  }
  if (rank_hist_host) rank_hist_host[0] = 0;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = DDM_OK, k = 0;
  if (failing > 0 && maxit > 0) {
    rc = combined_apply_multi_impl(ctx, prec, m, Z, B); // Z = M^-1 R; P = Z
    if (!rc && hipMemcpyAsync(P, Z, sizeof(double) * (size_t)(n * m), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
      rc = fail(ctx, DDM_EHIP, "ddm_bcg_solve_multi: copy of the first direction block failed");
  }
  while (!rc && failing > 0 && k < maxit) {
    ++k;
    if ((rc = op_apply_multi(ctx, op, m, P, Q))) break;                                   // Q = A P
    if ((rc = bcg_gram_device(ctx, op, m, P, Q, B, part, ws))) break;                     // W = P^T Q, S = P^T R: one pass
    if ((rc = ctx_allreduce(ctx, ws, 2 * mm, "block CG coupling matrix and right-hand side"))) break;
    if ((rc = ddm_memcpy_d2h(ctx, h.data(), ws, sizeof(double) * (size_t)(2 * mm)))) break; // read-back 1 of 2
    int rank = 0;
    if (!dense::sym_pinv(m, h.data(), rank_tol, Wp.data(), &rank)) {
      rc = fail(ctx, DDM_ENUMERIC, "ddm_bcg_solve_multi: P^T A P is not finite (or its eigen-decomposition failed) in iteration %d", k);
      break;
    }
    if (rank_hist_host) rank_hist_host[k] = rank;
    if (rank == 0) {
      rc = fail(ctx, DDM_ENUMERIC, "ddm_bcg_solve_multi: P^T A P has rank 0 in iteration %d while %d columns have not converged", k, failing);
      break;
    }
    bcg_small_product(m, 1.0, Wp.data(), h.data() + mm, coef.data());                      // alpha = W^+ S
    if ((rc = ddm_memcpy_h2d(ctx, alpha, coef.data(), sizeof(double) * (size_t)mm))) break;
    if ((rc = bcg_update_device(ctx, op, m, alpha, P, Q, X, B, zn + mm))) break;          // X += P alpha; R -= Q alpha; <R_c, R_c>
    if ((rc = combined_apply_multi_impl(ctx, prec, m, Z, B))) break;                      // Z = M^-1 R
    if ((rc = bcg_gram_device(ctx, op, m, Q, Z, nullptr, part, zn))) break;               // Q^T Z
    if ((rc = ctx_allreduce(ctx, zn, mm + m, "block CG direction coupling and defect norms"))) break;
    if ((rc = ddm_memcpy_d2h(ctx, h.data(), zn, sizeof(double) * (size_t)(mm + m)))) break; // read-back 2 of 2
    failing = 0;
    for (int c = 0; c < m && !rc; ++c) {
      f.def[c] = std::sqrt(h[mm + c]);
      if (hist_host) hist_host[(int64_t)k * m + c] = f.def[c];
      if (!(f.def[c] == f.def[c])) rc = fail(ctx, DDM_ENUMERIC, "ddm_bcg_solve_multi: defect is NaN in iteration %d (column %d)", k, c);
      else if (!passes(c)) ++failing;
      else if (first[c] < 0) first[c] = k;
    }
    if (rc || failing == 0) break;
    bcg_small_product(m, -1.0, Wp.data(), h.data(), coef.data());                          // beta = -W^+ (Q^T Z)
    if ((rc = ddm_memcpy_h2d(ctx, beta, coef.data(), sizeof(double) * (size_t)mm))) break;
    rc = bcg_direction_device(ctx, op, m, beta, Z, P);                                     // P = Z + P beta
  }
  for (int c = 0; c < m; ++c) {
    res[c].iterations = first[c] >= 0 ? first[c] : k;
    res[c].converged = passes(c) ? 1 : 0;
  }
  return multi_finish(f, prec, rc, t0);
}

// The three passes on their own, for tests.  Blocks are n x nrhs device blocks of op's rows; every call is synchronous.
// G_host ((V2 ? 2 : 1) nrhs^2 doubles) = [U^T V1 | U^T V2], owner-masked and summed over the ranks.
extern "C" int ddm_bcg_gram_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, const double *U, const double *V1, const double *V2, double *G_host)
{
  if (!ctx || !op || !U || !V1 || !G_host) return fail(ctx, DDM_EINVAL, "ddm_bcg_gram_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_bcg_gram_multi"));
  const int cnt = (V2 ? 2 : 1) * nrhs * nrhs;
  dbuf<double> g, part;
  HIPCHECK(ctx, g.alloc(cnt));
  HIPCHECK(ctx, part.alloc((int64_t)cnt * RED_MAX_BLOCKS));
  StreamDrain drain{ctx};
  DDMCHECK(bcg_gram_device(ctx, op, nrhs, U, V1, V2, part, g));
  DDMCHECK(ctx_allreduce(ctx, g, cnt, "block CG Gram products"));
  return ddm_memcpy_d2h(ctx, G_host, g, sizeof(double) * (size_t)cnt);
}
// X += P alpha; R -= Q alpha with alpha_host nrhs x nrhs row-major; norm2_host[c] = <R_c, R_c> afterwards (owner-masked, all ranks)
extern "C" int ddm_bcg_update_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, const double *alpha_host, const double *P, const double *Q, double *X, double *R,
                                    double *norm2_host)
{
  if (!ctx || !op || !alpha_host || !P || !Q || !X || !R || !norm2_host || X == R || P == X || P == R || Q == X || Q == R)
    return fail(ctx, DDM_EINVAL, "ddm_bcg_update_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_bcg_update_multi"));
  DDMCHECK(ctx_multi_scratch(ctx));
  dbuf<double> a;
  HIPCHECK(ctx, a.alloc(nrhs * nrhs + nrhs));
  StreamDrain drain{ctx};
  DDMCHECK(ddm_memcpy_h2d(ctx, a, alpha_host, sizeof(double) * (size_t)(nrhs * nrhs)));
  DDMCHECK(bcg_update_device(ctx, op, nrhs, a, P, Q, X, R, a + nrhs * nrhs));
  DDMCHECK(ctx_allreduce(ctx, a + nrhs * nrhs, nrhs, "block CG defect norms"));
  return ddm_memcpy_d2h(ctx, norm2_host, a + nrhs * nrhs, sizeof(double) * (size_t)nrhs);
}
// P = Z + P beta with beta_host nrhs x nrhs row-major
extern "C" int ddm_bcg_direction_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, const double *beta_host, const double *Z, double *P)
{
  if (!ctx || !op || !beta_host || !Z || !P || Z == P) return fail(ctx, DDM_EINVAL, "ddm_bcg_direction_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_bcg_direction_multi"));
  dbuf<double> b;
  HIPCHECK(ctx, b.alloc(nrhs * nrhs));
  StreamDrain drain{ctx};
  DDMCHECK(ddm_memcpy_h2d(ctx, b, beta_host, sizeof(double) * (size_t)(nrhs * nrhs)));
  return bcg_direction_device(ctx, op, nrhs, b, Z, P);
}
