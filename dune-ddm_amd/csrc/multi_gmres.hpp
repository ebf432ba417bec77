// Restarted GMRES for several right-hand sides at once: ddm_gmres_solve_multi of include/ddm_hip.h (included after multi_rhs.hpp).
// nrhs INDEPENDENT RestartedGMResSolver::apply recurrences in one loop (not a block-Krylov method): every column is what
// ddm_gmres_solve computes on it -- left preconditioning, modified Gram-Schmidt in the order k = 0..i, the Givens code of the
// single-vector driver (gmres_generate_rotation / gmres_apply_rotation, per column on the host) -- while the operator, the
// preconditioner and the orthogonalisation sweep run once per iteration for all columns.  The Krylov basis is min(restart, maxit) + 1
// row-major n x m blocks.  Per basis block the sweep is one AXPY over the block with the coefficients in device memory, the block
// dot (one kernel per column group, k_reduce_final_multi) and one all-reduce of m doubles; with DDM_GMRES_MULTI_FUSED=1 the AXPY and
// the partial sums of the next dot are one kernel (k_mgs_step_multi: bit-identical, 32 instead of 40 bytes per block entry, but
// measured slower on MI355X -- DESIGN.md section 9).  The host reads the (i + 2) x m fresh Hessenberg entries once per iteration and
// nothing else synchronises inside an iteration.
//
// Frozen columns: a column that passed its test is masked out (ctx->mactive) of every kernel of this file; the operator and the
// preconditioner still run on its (stale) basis entries, whose results nobody reads.

// host state of one column: Hessenberg matrix (restart + 1) x restart, right-hand side s of the least-squares problem, rotations
struct GmresColumn {
  int R = 0;
  std::vector<double> H, s, cs, sn;
  double norm = 0.0, def0 = 0.0;
  int cnt = 0; // Hessenberg columns of the current restart cycle
  void init(int restart)
  {
    R = restart;
    H.assign((size_t)(R + 1) * R, 0.0);
    s.assign(R + 1, 0.0);
    cs.assign(R, 0.0);
    sn.assign(R, 0.0);
  }
  double &h(int r, int c) { return H[(size_t)r * R + c]; }
};

// the sweep of iteration i: hdev[k * m + c] = h_{k,i} of column c for k <= i, hdev[(i + 1) * m + c] = <w, w>; w orthogonalised in place
static int gmres_mgs_multi(ddm_ctx *ctx, ddm_op *op, int m, int i, bool fused, const double *V, int64_t vstride, double *W, double *hdev)
{
  ScopedTimer t(ctx, "GMRES/orthogonalisation");
  const int64_t n = op->n;
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  const int32_t *active = ctx->mactive;
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, V, W, hdev)); // h_0 = <v_0, w>
  for (int k = 0; k <= i; ++k) {
    const double *vk = V + (int64_t)k * vstride;
    const double *z = k < i ? V + (int64_t)(k + 1) * vstride : W; // next dot: <v_{k+1}, w>, or <w, w> at the end
    double *out = hdev + (int64_t)(k + 1) * m;
    if (!fused) {
      hipLaunchKernelGGL(k_axpy_negdev_multi, dim3(grid_for(n * m)), dim3(WG), 0, ctx->stream, n, m, active, (const double *)(hdev + (int64_t)k * m), vk, W);
      DDMCHECK(dot_multi_device(ctx, n, op->owner, m, z, W, out));
      continue;
    }
    for_column_groups(m, [&](int c0, int cb) {
      DDM_MULTI_CB_DISPATCH(k_mgs_step_multi, op->owner != nullptr, cb, dim3(nb), dim3(WG), 0, ctx->stream, n, m, c0, active,
                            (const double *)(hdev + (int64_t)k * m), (const uint8_t *)op->owner, vk, z, W, ctx->mpartial);
    });
    hipLaunchKernelGGL(k_reduce_final_multi, dim3(m), dim3(WG), 0, ctx->stream, nb, (const double *)ctx->mpartial, out);
    HIPCHECK(ctx, hipGetLastError());
    DDMCHECK(ctx_allreduce(ctx, out, m, "Gram-Schmidt coefficients"));
  }
  return DDM_OK;
}

extern "C" int ddm_gmres_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit,
                                     int restart, double *hist_host, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !X || !B || !res || X == B || maxit < 0 || restart < 1)
    return fail(ctx, DDM_EINVAL, "ddm_gmres_solve_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_gmres_solve_multi"));
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  const int m = nrhs;
  const int64_t n = op->n;
  const int64_t vstride = std::max<int64_t>(n, 1) * m;
  const int R = std::min(restart, std::max(maxit, 1)); // a cycle never gets longer than maxit iterations: no basis block beyond that
  { // R + 1 basis blocks and the work block must fit into the free device memory: refuse before anything is allocated
    size_t free_b = 0, total_b = 0;
    HIPCHECK(ctx, hipMemGetInfo(&free_b, &total_b));
    const double need = ((double)R + 2.0) * (double)vstride * sizeof(double);
    if (need > (double)free_b)
      return fail(ctx, DDM_ENOTIMPL, "ddm_gmres_solve_multi: the Krylov basis of %d + 1 blocks of %lld x %d doubles and the work block need %.0f bytes, %zu are free",
                  R, (long long)n, m, need, free_b);
  }
  const bool fused = [] { // read once per solve; the unfused composition is the default (it measured faster)
    const char *e = std::getenv("DDM_GMRES_MULTI_FUSED");
    return e && e[0] == '1';
  }();
  for (int c = 0; c < m; ++c) res[c] = ddm_solve_result{0, 0, 0.0, 1.0, 0.0};
  DDMCHECK(ctx_multi_scratch(ctx));
  dbuf<double> Vb, Wb, hdev, ydev;
  dbuf<int32_t> cdev; // [0, m): Hessenberg columns per column in the cycle, [m, 2m): keep W (still running)
  HIPCHECK(ctx, Vb.alloc(vstride * (R + 1)));
  HIPCHECK(ctx, Wb.alloc(vstride));
  HIPCHECK(ctx, hdev.alloc((int64_t)(R + 2) * m));
  HIPCHECK(ctx, ydev.alloc((int64_t)R * m));
  HIPCHECK(ctx, cdev.alloc(2 * m));
  StreamDrain drain{ctx}; // (declared after the buffers: from here on every return waits for the stream before they are released)
  double *V = Vb, *W = Wb;
  auto v = [&](int k) { return V + (int64_t)k * vstride; };
  std::vector<GmresColumn> col(m);
  for (auto &q : col) q.init(R);
  std::vector<double> hcol((size_t)(R + 2) * m), yhost((size_t)R * m), ycol(R);
  int32_t active[MULTI_MAX], cflags[2 * MULTI_MAX];
  MultiCoef coef;
  const int GE = grid_for(n * m);

  // b -= A x; v0 = M^-1 b; def0 = |v0| per column
  DDMCHECK(op_applyscaleadd_multi(ctx, op, m, -1.0, X, B));
  DDMCHECK(combined_apply_multi_impl(ctx, prec, m, v(0), B));
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, v(0), v(0), hdev));
  DDMCHECK(ddm_memcpy_d2h(ctx, hcol.data(), hdev, sizeof(double) * (size_t)m));
  int nactive = 0;
  for (int c = 0; c < m; ++c) {
    col[c].norm = col[c].def0 = std::sqrt(hcol[c]);
    res[c].def0 = col[c].def0;
    if (hist_host) hist_host[c] = col[c].def0;
    if (!(col[c].def0 == col[c].def0)) return fail(ctx, DDM_ENUMERIC, "ddm_gmres_solve_multi: initial defect is NaN in column %d", c);
    active[c] = col[c].def0 < 1e-30 ? 0 : 1;
    if (!active[c]) res[c].converged = 1;
    nactive += active[c];
  }
  DDMCHECK(ddm_memcpy_h2d(ctx, ctx->mactive, active, sizeof(int32_t) * (size_t)m));
  const auto t0 = std::chrono::steady_clock::now();
  int rc = DDM_OK, j = 0;
  while (j < maxit && nactive > 0 && !rc) {
    for (int c = 0; c < m; ++c) {
      GmresColumn &q = col[c];
      q.cnt = 0;
      coef.a[c] = active[c] ? 1.0 / q.norm : 0.0;
      if (!active[c]) continue;
      std::fill(q.s.begin(), q.s.end(), 0.0);
      q.s[0] = q.norm;
    }
    hipLaunchKernelGGL(k_scale_into_multi, dim3(GE), dim3(WG), 0, ctx->stream, n, m, (const int32_t *)ctx->mactive, coef, (const double *)v(0), v(0));
    int i = 0;
    for (; i < R && j < maxit && nactive > 0; ++i, ++j) {
      rc = op_apply_multi(ctx, op, m, v(i), v(i + 1));                      // v[i+1] = A v[i] (temporary)
      if (!rc) rc = combined_apply_multi_impl(ctx, prec, m, W, v(i + 1));   // w = M^-1 A v[i]
      if (!rc) rc = gmres_mgs_multi(ctx, op, m, i, fused, V, vstride, W, hdev);
      if (!rc) rc = ddm_memcpy_d2h(ctx, hcol.data(), hdev, sizeof(double) * (size_t)(i + 2) * m); // the one read-back of the iteration
      if (rc) break;
      for (int c = 0; c < m && !rc; ++c) {
        coef.a[c] = 0.0;
        if (!active[c]) continue;
        GmresColumn &q = col[c];
        for (int k = 0; k <= i; ++k) q.h(k, i) = hcol[(size_t)k * m + c];
        q.h(i + 1, i) = std::sqrt(hcol[(size_t)(i + 1) * m + c]);
        if (std::fabs(q.h(i + 1, i)) < 1e-80)
          rc = fail(ctx, DDM_ENUMERIC, "ddm_gmres_solve_multi: breakdown in GMRes - |w| == 0.0 after %d iterations (column %d)", j, c);
        coef.a[c] = 1.0 / q.h(i + 1, i);
      }
      if (rc) break;
      hipLaunchKernelGGL(k_scale_into_multi, dim3(GE), dim3(WG), 0, ctx->stream, n, m, (const int32_t *)ctx->mactive, coef, (const double *)W, v(i + 1));
      bool changed = false;
      for (int c = 0; c < m; ++c) {
        if (!active[c]) continue;
        GmresColumn &q = col[c];
        for (int k = 0; k < i; ++k) gmres_apply_rotation(q.h(k, i), q.h(k + 1, i), q.cs[k], q.sn[k]);
        gmres_generate_rotation(q.h(i, i), q.h(i + 1, i), q.cs[i], q.sn[i]);
        gmres_apply_rotation(q.h(i, i), q.h(i + 1, i), q.cs[i], q.sn[i]);
        gmres_apply_rotation(q.s[i], q.s[i + 1], q.cs[i], q.sn[i]);
        q.norm = std::fabs(q.s[i + 1]);
        q.cnt = i + 1;
        res[c].iterations = j + 1;
        if (hist_host) hist_host[(int64_t)(j + 1) * m + c] = q.norm;
        if (!(q.norm == q.norm)) {
          rc = fail(ctx, DDM_ENUMERIC, "ddm_gmres_solve_multi: defect is NaN in iteration %d (column %d)", j + 1, c);
          break;
        }
        if (q.norm < q.def0 * reduction || q.norm < 1e-30) {
          res[c].converged = 1;
          active[c] = 0;
          nactive -= 1;
          changed = true;
        }
      }
      if (rc) break;
      if (changed) rc = ddm_memcpy_h2d(ctx, ctx->mactive, active, sizeof(int32_t) * (size_t)m);
      if (rc) break;
    }
    if (rc) break;
    // update(w, i, H, s, v) per column: solve its triangular system of cnt_c unknowns; W_c = sum_k y_k v[k]; X_c += W_c
    std::fill(yhost.begin(), yhost.end(), 0.0);
    for (int c = 0; c < m; ++c) {
      GmresColumn &q = col[c];
      cflags[c] = q.cnt;
      cflags[m + c] = active[c];
      for (int a = q.cnt - 1; a >= 0; --a) {
        double t = q.s[a];
        for (int b = a + 1; b < q.cnt; ++b) t -= q.h(a, b) * ycol[b];
        ycol[a] = t / q.h(a, a);
        yhost[(size_t)a * m + c] = ycol[a];
      }
    }
    rc = ddm_memcpy_h2d(ctx, ydev, yhost.data(), sizeof(double) * (size_t)i * m);
    if (!rc) rc = ddm_memcpy_h2d(ctx, cdev, cflags, sizeof(int32_t) * (size_t)(2 * m));
    if (rc) break;
    {
      ScopedTimer t(ctx, "GMRES/update");
      hipLaunchKernelGGL(k_gmres_update_multi, dim3(GE), dim3(WG), 0, ctx->stream, n, m, (const int32_t *)cdev, (const int32_t *)(cdev + m), (const double *)ydev,
                         (const double *)V, vstride, W, X);
    }
    if (nactive > 0 && j < maxit) { // restart: b -= A w (w = 0 in the columns that are done); v0 = M^-1 b
      rc = op_applyscaleadd_multi(ctx, op, m, -1.0, W, B);
      if (!rc) rc = combined_apply_multi_impl(ctx, prec, m, v(0), B);
      if (!rc) rc = dot_multi_device(ctx, n, op->owner, m, v(0), v(0), hdev);
      if (!rc) rc = ddm_memcpy_d2h(ctx, hcol.data(), hdev, sizeof(double) * (size_t)m);
      for (int c = 0; c < m && !rc; ++c)
        if (active[c]) col[c].norm = std::sqrt(hcol[c]);
    }
  }
  if (!rc && hipGetLastError() != hipSuccess) rc = fail(ctx, DDM_EHIP, "kernel launch failed in ddm_gmres_solve_multi");
  (void)hipStreamSynchronize(ctx->stream);
  const double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  for (int c = 0; c < m; ++c) {
    res[c].elapsed_s = elapsed;
    if (col[c].def0 >= 1e-30) res[c].reduction = col[c].norm / col[c].def0;
  }
  if (!rc && prec->schwarz) {
    int st = 0;
    rc = ddm_ilu0_status(ctx, prec->schwarz->solver, &st);
    if (!rc && st) rc = fail(ctx, DDM_ENUMERIC, "persistent triangular solve timed out waiting for a level (results invalid)");
  }
  return rc;
}
