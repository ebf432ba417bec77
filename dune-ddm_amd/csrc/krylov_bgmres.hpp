// Block GMRES: one shared Krylov space for m right-hand sides, and its three passes on their own.  Needs krylov_frame.hpp.
#pragma once

// ---- block GMRES: one shared Krylov space for m right-hand sides ------------------------------------------------------------------------
// Right-preconditioned block GMRES with a fixed preconditioner (include/ddm_hip.h states the algorithm): the non-symmetric companion
// of block CG.  The block is deflated at every cycle start (width p <= m, fixed for the cycle), the block Arnoldi step orthogonalises
// with block classical Gram-Schmidt applied twice -- four passes over the basis and three all-reduces whatever the step index --, the
// least-squares problem is solved by every rank on the host (dense::BlockHessenberg).  Like block CG it uses neither ctx->mactive nor
// the record / mask part of the MultiFrame.  Its three kernels, each usable on its own (ddm_bgmres_project_multi,
// ddm_bgmres_combine_multi, ddm_bgmres_combine_gram_multi):
//
// workgroups of a projection over K stored blocks of width p: the partial sums are K p^2 doubles per workgroup, so the grid shrinks as
// K p^2 grows (2^23 doubles of partial sums at most, never fewer than 64 workgroups, never more than RED_MAX_BLOCKS).  It depends on
// the step's own K, not on the restart length: a short cycle of a wide block keeps the whole grid.
static int bgmres_project_cap(int K, int p) { return (int)std::max<int64_t>(64, std::min<int64_t>(RED_MAX_BLOCKS, ((int64_t)1 << 23) / ((int64_t)K * p * p))); }
// doubles of partial sums that projections over up to Kmax stored blocks of width p need
static int64_t bgmres_project_partials(int Kmax, int p) { return std::max<int64_t>((int64_t)1 << 23, (int64_t)Kmax * p * p * 64); }
// H (device, K p^2 doubles) = V_k^T W, k < K, of THIS rank's owned rows; part: bgmres_project_partials(K, p) doubles
static int bgmres_project_device(ddm_ctx *ctx, ddm_op *op, int p, int K, const double *V, int64_t vstride, const double *W, double *part, double *H)
{
  ScopedTimer t(ctx, "BGMRES/project");
  const int nb = grid_for(op->n, BCG_TILE / ((p + 1) & ~1), bgmres_project_cap(K, p));
  const uint8_t *mask = op->owner;
  if (mask) hipLaunchKernelGGL(k_bgmres_project<true>, dim3(nb), dim3(WG), 0, ctx->stream, op->n, p, K, mask, V, vstride, W, part);
  else hipLaunchKernelGGL(k_bgmres_project<false>, dim3(nb), dim3(WG), 0, ctx->stream, op->n, p, K, mask, V, vstride, W, part);
  hipLaunchKernelGGL(k_reduce_final_multi, dim3(K * p * p), dim3(WG), 0, ctx->stream, nb, (const double *)part, H);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
static int bgmres_combine_rows(int pin, int q) { return std::min(4 * (WG / q), BCG_TILE / ((pin + 1) & ~1)); }
// Out (n x q) = (mode 0) / += (1) / -= (2) sum_k V_k (n x pin) C_k (pin x q); coef: K pin q device doubles
static int bgmres_combine_device(ddm_ctx *ctx, ddm_op *op, int mode, int pin, int q, int K, const double *V, int64_t vstride, const double *coef, double *Out)
{
  ScopedTimer t(ctx, "BGMRES/combine");
  const dim3 nb(grid_for(op->n, bgmres_combine_rows(pin, q), RED_MAX_BLOCKS));
  const uint8_t *none = nullptr;
  double *nopart = nullptr;
  if (mode == 0) hipLaunchKernelGGL((k_bgmres_combine<0, false, false>), nb, dim3(WG), 0, ctx->stream, op->n, pin, q, K, V, vstride, coef, none, Out, nopart);
  else if (mode == 1) hipLaunchKernelGGL((k_bgmres_combine<1, false, false>), nb, dim3(WG), 0, ctx->stream, op->n, pin, q, K, V, vstride, coef, none, Out, nopart);
  else hipLaunchKernelGGL((k_bgmres_combine<2, false, false>), nb, dim3(WG), 0, ctx->stream, op->n, pin, q, K, V, vstride, coef, none, Out, nopart);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
// W (n x p) -= sum_k V_k C_k and G (device, p^2 doubles) = W^T W of THIS rank's owned rows afterwards; part: p^2 x RED_MAX_BLOCKS doubles
static int bgmres_combine_gram_device(ddm_ctx *ctx, ddm_op *op, int p, int K, const double *V, int64_t vstride, const double *coef, double *W, double *part, double *G)
{
  ScopedTimer t(ctx, "BGMRES/combine");
  const int nb = grid_for(op->n, bgmres_combine_rows(p, p), RED_MAX_BLOCKS);
  const uint8_t *mask = op->owner;
  if (mask) hipLaunchKernelGGL((k_bgmres_combine<2, true, true>), dim3(nb), dim3(WG), 0, ctx->stream, op->n, p, p, K, V, vstride, coef, mask, W, part);
  else hipLaunchKernelGGL((k_bgmres_combine<2, true, false>), dim3(nb), dim3(WG), 0, ctx->stream, op->n, p, p, K, V, vstride, coef, mask, W, part);
  hipLaunchKernelGGL(k_reduce_final_multi, dim3(p * p), dim3(WG), 0, ctx->stream, nb, (const double *)part, G);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}

extern "C" int ddm_bgmres_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit,
                                      int restart, double rank_tol, double *hist_host, int32_t *width_hist_host, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !X || !B || !res || X == B || maxit < 0 || restart < 1 || !(rank_tol > 0.0 && rank_tol < 1.0))
    return fail(ctx, DDM_EINVAL, "ddm_bgmres_solve_multi: bad arguments (null pointer, X == B, maxit < 0, restart < 1 or rank_tol outside (0, 1))");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_bgmres_solve_multi"));
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  const char *what = "ddm_bgmres_solve_multi";
  const int m = nrhs, mm = m * m;
  const int64_t n = op->n, vstride = std::max<int64_t>(n, 1) * m;
  const int R = std::min(restart, std::max(maxit, 1)); // a cycle never gets longer than maxit iterations: no basis block beyond that
  const int64_t npart = std::max<int64_t>(bgmres_project_partials(R + 1, m), (int64_t)mm * RED_MAX_BLOCKS);
  DDMCHECK(gmres_memory_check(ctx, what, (int64_t)R + 4 + (npart + vstride - 1) / vstride, n, m));
  for (int c = 0; c < m; ++c) solve_result_reset(&res[c]);
  DDMCHECK(ctx_multi_scratch(ctx));
  HIPCHECK(ctx, prec->work.reserve(m, n, 3));
  double *U = prec->work.block[0], *W = prec->work.block[1], *Z = prec->work.block[2]; // U (cycle end), W = A Z, Z = M^-1 V_j or M^-1 U
  dbuf<double> Vb, hdev, cdev, part; // hdev: [H1 | H2 | G_W] of a step, norms; cdev: C0 / C / Y, then the unit matrix
  HIPCHECK(ctx, Vb.alloc(vstride * (R + 1)));
  HIPCHECK(ctx, hdev.alloc((int64_t)(2 * (R + 1) + 1) * mm + m));
  HIPCHECK(ctx, cdev.alloc((int64_t)(R + 1) * mm));
  HIPCHECK(ctx, part.alloc(npart));
  StreamDrain drain{ctx}; // (declared after the buffers: from here on every return waits for the stream before they are released)
  double *V = Vb, *unit = cdev + (int64_t)R * mm;
  std::vector<double> h((size_t)(2 * (R + 1) + 1) * mm + m), G(mm), Sf(mm), Cf(mm), scale2(m), block, coef, Y((size_t)R * mm);
  int first[MULTI_MAX]; // the first block iteration at which the column passed its test and stayed passed, -1: not yet
  bool run[MULTI_MAX];
  dense::BlockHessenberg ls;
  MultiFrame f{ctx, what, m, reduction, hist_host, res};
  auto passes = [&](int c) { return f.def[c] < res[c].def0 * reduction || f.def[c] < 1e-30; };
  {
    std::vector<double> eye(mm, 0.0);
    for (int c = 0; c < m; ++c) eye[c * m + c] = 1.0;
    DDMCHECK(ddm_memcpy_h2d(ctx, unit, eye.data(), sizeof(double) * (size_t)mm));
  }
  DDMCHECK(op_applyscaleadd_multi(ctx, op, m, -1.0, X, B)); // R = B - A X, in B
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, B, B, hdev));
  DDMCHECK(ddm_memcpy_d2h(ctx, h.data(), hdev, sizeof(double) * (size_t)m));
  int failing = 0;
  for (int c = 0; c < m; ++c) {
    const double def0 = f.def[c] = std::sqrt(h[c]);
    res[c].def0 = def0;
    if (hist_host) hist_host[c] = def0;
    const Defect0 d = classify_initial_defect(def0);
    if (d == Defect0::NaN) return fail(ctx, DDM_ENUMERIC, "%s: initial defect is NaN in column %d", what, c);
    first[c] = d == Defect0::Zero ? 0 : -1;
    failing += d == Defect0::Go;
  }
  if (width_hist_host) width_hist_host[0] = 0;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = DDM_OK, k = 0;
  while (!rc && failing > 0 && k < maxit) {
    // ---- cycle start: deflation of the running defects ----
    for (int c = 0; c < m; ++c) run[c] = first[c] < 0;
    if ((rc = bgmres_project_device(ctx, op, m, 1, B, vstride, B, part, hdev))) break; // G = R^T R
    if ((rc = ctx_allreduce(ctx, hdev, mm, "block GMRES Gram matrix of the defects"))) break;
    if ((rc = ddm_memcpy_d2h(ctx, G.data(), hdev, sizeof(double) * (size_t)mm))) break;
    for (int a = 0; a < m; ++a)
      for (int b = 0; b < m; ++b)
        if (!run[a] || !run[b]) G[a * m + b] = 0.0;
    int p = 0;
    if (!dense::bgmres_factor(m, G.data(), nullptr, rank_tol, Sf.data(), Cf.data(), &p)) {
      rc = fail(ctx, DDM_ENUMERIC, "%s: the Gram matrix of the defects is not finite (or its eigen-decomposition failed) after %d iterations", what, k);
      break;
    }
    if (p == 0) {
      rc = fail(ctx, DDM_ENUMERIC, "%s: the running defects have rank 0 after %d iterations while %d columns have not converged", what, k, failing);
      break;
    }
    const int pp = p * p;
    const int64_t bstride = std::max<int64_t>(n, 1) * p; // the basis blocks of this cycle
    auto v = [&](int j) { return V + (int64_t)j * bstride; };
    coef.assign((size_t)m * p, 0.0); // C0, m x p; T (p x m) for the least squares: columns / rows of columns that do not run are zero
    block.assign((size_t)p * m, 0.0);
    for (int c = 0; c < m; ++c)
      if (run[c])
        for (int a = 0; a < p; ++a) {
          coef[(size_t)c * p + a] = Cf[(size_t)c * m + a];
          block[(size_t)a * m + c] = Sf[(size_t)a * m + c];
        }
    ls.start(p, m, block.data());
    if ((rc = ddm_memcpy_h2d(ctx, cdev, coef.data(), sizeof(double) * (size_t)(m * p)))) break;
    if ((rc = bgmres_combine_device(ctx, op, 0, m, p, 1, B, vstride, cdev, v(0)))) break; // V_0 = R C0
    int j = 0;
    bool done = false;
    while (!rc && j < R && k < maxit && !done) {
      const int K = j + 1;
      double *H1 = hdev, *H2 = hdev + (int64_t)K * pp, *GW = hdev + (int64_t)2 * K * pp;
      if ((rc = combined_apply_multi_impl(ctx, prec, p, Z, v(j)))) break;                                  // Z = M^-1 V_j
      if ((rc = op_apply_multi(ctx, op, p, Z, W))) break;                                                   // W = A Z
      if ((rc = bgmres_project_device(ctx, op, p, K, V, bstride, W, part, H1))) break;                // H1 = [V_0 .. V_j]^T W
      if ((rc = ctx_allreduce(ctx, H1, (int64_t)K * pp, "block GMRES projection"))) break;
      if ((rc = bgmres_combine_device(ctx, op, 2, p, p, K, V, bstride, H1, W))) break;                      // W -= [V_0 .. V_j] H1
      if ((rc = bgmres_project_device(ctx, op, p, K, V, bstride, W, part, H2))) break;                // H2, the same way
      if ((rc = ctx_allreduce(ctx, H2, (int64_t)K * pp, "block GMRES second projection"))) break;
      if ((rc = bgmres_combine_gram_device(ctx, op, p, K, V, bstride, H2, W, part, GW))) break;             // W -= [..] H2; G_W = W^T W
      if ((rc = ctx_allreduce(ctx, GW, pp, "block GMRES Gram matrix of the new block"))) break;
      if ((rc = ddm_memcpy_d2h(ctx, h.data(), hdev, sizeof(double) * (size_t)((2 * K + 1) * pp)))) break;   // the one read-back of the step
      int rank = 0, still = 0;
      {
        ScopedTimer th(ctx, "BGMRES/host");
        block.assign((size_t)(K + 1) * pp, 0.0); // column block j of the block Hessenberg matrix: [H1 + H2; S]
        for (int e = 0; e < K * pp; ++e) block[e] = h[e] + h[(size_t)K * pp + e];
        for (int c = 0; c < p; ++c) {
          double s2 = 0.0;
          for (int a = 0; a < K * p; ++a) s2 += block[(size_t)a * p + c] * block[(size_t)a * p + c];
          scale2[c] = s2 + h[(size_t)2 * K * pp + (size_t)c * p + c]; // ||W_c||^2 before the orthogonalisation
        }
        if (!dense::bgmres_factor(p, h.data() + (size_t)2 * K * pp, scale2.data(), rank_tol, Sf.data(), Cf.data(), &rank)) {
          rc = fail(ctx, DDM_ENUMERIC, "%s: the block Arnoldi coefficients are not finite (or an eigen-decomposition failed) in iteration %d", what, k + 1);
          break;
        }
        std::copy(Sf.begin(), Sf.begin() + pp, block.begin() + (size_t)K * pp);
        ls.add_block(block.data());
        ++j, ++k;
        if (width_hist_host) width_hist_host[k] = p;
        for (int c = 0; c < m && !rc; ++c) {
          if (run[c]) f.def[c] = ls.residual(c);
          if (hist_host) hist_host[(int64_t)k * m + c] = f.def[c];
          if (!(f.def[c] == f.def[c])) rc = fail(ctx, DDM_ENUMERIC, "%s: defect is NaN in iteration %d (column %d)", what, k, c);
          if (!run[c]) continue;
          if (!passes(c)) first[c] = -1, ++still;
          else if (first[c] < 0) first[c] = k;
        }
      }
      if (rc) break;
      if (rank < p || still == 0) done = true; // exhausted: the step counted, the cycle ends
      else if (j < R && k < maxit) {
        if ((rc = ddm_memcpy_h2d(ctx, cdev, Cf.data(), sizeof(double) * (size_t)pp))) break;
        rc = bgmres_combine_device(ctx, op, 0, p, p, 1, W, bstride, cdev, v(j));                           // V_{j+1} = W C
      }
    }
    if (rc) break;
    // ---- cycle end: U = [V_0 .. V_{j-1}] Y; X += M^-1 U; R -= A M^-1 U; the defect norms recomputed ----
    if (!ls.solve(Y.data())) {
      rc = fail(ctx, DDM_ENUMERIC, "%s: the block Hessenberg matrix is singular after %d iterations", what, k);
      break;
    }
    for (int a = 0; a < j * p; ++a)
      for (int c = 0; c < m; ++c)
        if (!run[c]) Y[(size_t)a * m + c] = 0.0;
    if ((rc = ddm_memcpy_h2d(ctx, cdev, Y.data(), sizeof(double) * (size_t)(j * p * m)))) break;
    if ((rc = bgmres_combine_device(ctx, op, 0, p, m, j, V, bstride, cdev, U))) break;
    if ((rc = combined_apply_multi_impl(ctx, prec, m, Z, U))) break;
    if ((rc = bgmres_combine_device(ctx, op, 1, m, m, 1, Z, vstride, unit, X))) break;                      // X += Z
    if ((rc = op_applyscaleadd_multi(ctx, op, m, -1.0, Z, B))) break;                                      // R -= A Z
    if ((rc = dot_multi_device(ctx, n, op->owner, m, B, B, hdev))) break;
    if ((rc = ddm_memcpy_d2h(ctx, h.data(), hdev, sizeof(double) * (size_t)m))) break;
    failing = 0;
    for (int c = 0; c < m && !rc; ++c) {
      if (run[c]) {
        f.def[c] = std::sqrt(h[c]);
        if (!(f.def[c] == f.def[c])) rc = fail(ctx, DDM_ENUMERIC, "%s: defect is NaN after iteration %d (column %d)", what, k, c);
        if (!passes(c)) first[c] = -1;
        else if (first[c] < 0) first[c] = k;
      }
      if (hist_host) hist_host[(int64_t)k * m + c] = f.def[c];
      failing += first[c] < 0;
    }
  }
  for (int c = 0; c < m; ++c) {
    res[c].iterations = first[c] >= 0 ? first[c] : k;
    res[c].converged = passes(c) ? 1 : 0;
  }
  return multi_finish(f, prec, rc, t0);
}

// The three passes on their own, for tests; every call is synchronous.  V: K blocks of n x p doubles one after the other.
// H_host (K p^2 doubles) = V_k^T W, owner-masked and summed over the ranks
extern "C" int ddm_bgmres_project_multi(ddm_ctx *ctx, ddm_op *op, int p, int K, const double *V, const double *W, double *H_host)
{
  if (!ctx || !op || !V || !W || !H_host || K < 1) return fail(ctx, DDM_EINVAL, "ddm_bgmres_project_multi: bad arguments");
  DDMCHECK(multi_check(ctx, p, "ddm_bgmres_project_multi"));
  const int64_t cnt = (int64_t)K * p * p;
  dbuf<double> hd, part;
  HIPCHECK(ctx, hd.alloc(cnt));
  HIPCHECK(ctx, part.alloc(bgmres_project_partials(K, p)));
  StreamDrain drain{ctx};
  DDMCHECK(bgmres_project_device(ctx, op, p, K, V, std::max<int64_t>(op->n, 1) * p, W, part, hd));
  DDMCHECK(ctx_allreduce(ctx, hd, cnt, "block GMRES projection"));
  return ddm_memcpy_d2h(ctx, H_host, hd, sizeof(double) * (size_t)cnt);
}
// Out (n x q) = (mode 0) / += (1) / -= (2) sum_k V_k (n x pin) C_k (pin x q); coef_host: K pin q doubles
extern "C" int ddm_bgmres_combine_multi(ddm_ctx *ctx, ddm_op *op, int mode, int pin, int q, int K, const double *V, const double *coef_host, double *Out)
{
  if (!ctx || !op || !V || !coef_host || !Out || V == Out || K < 1 || mode < 0 || mode > 2) return fail(ctx, DDM_EINVAL, "ddm_bgmres_combine_multi: bad arguments");
  DDMCHECK(multi_check(ctx, pin, "ddm_bgmres_combine_multi"));
  DDMCHECK(multi_check(ctx, q, "ddm_bgmres_combine_multi"));
  const int64_t cnt = (int64_t)K * pin * q;
  dbuf<double> cd;
  HIPCHECK(ctx, cd.alloc(cnt));
  StreamDrain drain{ctx};
  DDMCHECK(ddm_memcpy_h2d(ctx, cd, coef_host, sizeof(double) * (size_t)cnt));
  return bgmres_combine_device(ctx, op, mode, pin, q, K, V, std::max<int64_t>(op->n, 1) * pin, cd, Out);
}
// W (n x p) -= sum_k V_k C_k; G_host (p^2 doubles) = W^T W afterwards, owner-masked and summed over the ranks
extern "C" int ddm_bgmres_combine_gram_multi(ddm_ctx *ctx, ddm_op *op, int p, int K, const double *V, const double *coef_host, double *W, double *G_host)
{
  if (!ctx || !op || !V || !coef_host || !W || !G_host || V == W || K < 1) return fail(ctx, DDM_EINVAL, "ddm_bgmres_combine_gram_multi: bad arguments");
  DDMCHECK(multi_check(ctx, p, "ddm_bgmres_combine_gram_multi"));
  const int64_t cnt = (int64_t)K * p * p;
  dbuf<double> cd, part;
  HIPCHECK(ctx, cd.alloc(cnt + p * p));
  HIPCHECK(ctx, part.alloc((int64_t)p * p * RED_MAX_BLOCKS));
  StreamDrain drain{ctx};
  DDMCHECK(ddm_memcpy_h2d(ctx, cd, coef_host, sizeof(double) * (size_t)cnt));
  DDMCHECK(bgmres_combine_gram_device(ctx, op, p, K, V, std::max<int64_t>(op->n, 1) * p, cd, W, part, cd + cnt));
  DDMCHECK(ctx_allreduce(ctx, cd + cnt, p * p, "block GMRES Gram matrix of the new block"));
  return ddm_memcpy_d2h(ctx, G_host, cd + cnt, sizeof(double) * (size_t)(p * p));
}
