// Restarted GMRES, left-preconditioned and flexible: one loop per vector count over the same GmresColumn.  Needs krylov_frame.hpp.
#pragma once

// ---- restarted GMRES, left-preconditioned and flexible ------------------------------------------------
// dune-istl RestartedGMResSolver::apply and RestartedFlexibleGMResSolver::apply (DUNE 2.10 solvers.hh; not in the snapshot, restated
// from the published implementation, in oracle/apply_oracle.py and in tests/fgmres_reference.py): modified Gram-Schmidt in the order
// k = 0..i, Givens rotations, restart after `restart` iterations.  Selected by [solver] type = restartedgmressolver
// (examples/poisson.ini:12-17, restart = 100; the default of dune/ddm/twolevel_schwarz.hh:121-130, restart = 30) or
// restartedflexiblegmressolver.  Krylov basis, dots and updates stay on the device; per iteration the i + 2 Hessenberg entries are
// read back for the rotations on the host.  The two variants differ at five points (R = min(restart, max(maxit, 1))):
//                            left                                         flexible
//   initial and restart norm v0 = M^-1 b, ||v0||: the PRECONDITIONED      ||b||: (an estimate of) the TRUE defect b - A x is
//                            defect is monitored                          monitored
//   cycle start              v0 scaled in place                           v0 = b / ||b||
//   step                     v[i+1] = A v[i] (temporary), w = M^-1 v[i+1] z[i] = M^-1 v[i] (kept), w = A z[i]
//   update basis             V (R + 1 vectors): x += sum_k y_k v[k]       Z (R more vectors): x += sum_k y_k z[k]; no further
//                                                                         preconditioner apply, so M^-1 may change between iterations
//   restart                  b -= A w, then M^-1 and the dot              b -= A w, then the dot of b
static void gmres_generate_rotation(double dx, double dy, double &cs, double &sn)
{
  const double ndx = std::fabs(dx), ndy = std::fabs(dy);
  if (ndy < 1e-15) {
    cs = 1.0;
    sn = 0.0;
  } else if (ndx < 1e-15) {
    cs = 0.0;
    sn = 1.0;
  } else if (ndy > ndx) {
    const double t = ndx / ndy;
    cs = 1.0 / std::sqrt(1.0 + t * t);
    sn = cs;
    cs *= t;
    sn *= dx / ndx;
    sn *= dy / ndy;
  } else {
    const double t = ndy / ndx;
    cs = 1.0 / std::sqrt(1.0 + t * t);
    sn = cs;
    sn *= dy / dx;
  }
}
static void gmres_apply_rotation(double &dx, double &dy, double cs, double sn)
{
  const double t = cs * dx + sn * dy;
  dy = -sn * dx + cs * dy;
  dx = t;
}

// host state of one column: Hessenberg matrix (restart + 1) x restart, right-hand side s of the least-squares problem, rotations
struct GmresColumn {
  int R = 0;
  std::vector<double> H, s, cs, sn;
  double norm = 0.0;
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
  void start_cycle() { cnt = 0, std::fill(s.begin(), s.end(), 0.0), s[0] = norm; } // a restart cycle begins from the defect norm in `norm`
  // Iteration i of the cycle, in two halves, because the driver normalises the next basis vector by |w| in between.  First half: the
  // fresh Hessenberg column (hcol[k * stride]: the Gram-Schmidt coefficients k <= i, then <w, w>) goes into H; returns h_{i+1,i} = |w|.
  double take_column(int i, const double *hcol, size_t stride)
  {
    for (int k = 0; k <= i; ++k) h(k, i) = hcol[(size_t)k * stride];
    h(i + 1, i) = std::sqrt(hcol[(size_t)(i + 1) * stride]);
    return h(i + 1, i);
  }
  // Second half: the old rotations applied to column i, the new one generated and applied to it and to s; returns the new defect norm.
  double rotate(int i)
  {
    for (int k = 0; k < i; ++k) gmres_apply_rotation(h(k, i), h(k + 1, i), cs[k], sn[k]);
    gmres_generate_rotation(h(i, i), h(i + 1, i), cs[i], sn[i]);
    gmres_apply_rotation(h(i, i), h(i + 1, i), cs[i], sn[i]);
    gmres_apply_rotation(s[i], s[i + 1], cs[i], sn[i]);
    norm = std::fabs(s[i + 1]);
    cnt = i + 1;
    return norm;
  }
  // y[0, cnt) = solution of the triangular system of the cycle (update(w, i, H, s, v) of dune-istl)
  void back_substitute(double *y)
  {
    for (int a = cnt - 1; a >= 0; --a) {
      double t = s[a];
      for (int b = a + 1; b < cnt; ++b) t -= h(a, b) * y[b];
      y[a] = t / h(a, a);
    }
  }
};

// the loop for one right-hand side; what: the exported function's name, for messages
static int gmres_loop(ddm_ctx *ctx, const char *what, bool flexible, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit,
                      int restart, double *hist_host, ddm_solve_result *res)
{
  const int64_t n = op->n, stride = std::max<int64_t>(n, 1);
  const int R = std::min(restart, std::max(maxit, 1)); // a cycle never gets longer than maxit iterations: no basis vector beyond that
  const int G = grid_for(n);
  DDMCHECK(gmres_memory_check(ctx, what, (flexible ? 2 : 1) * (int64_t)R + 2, n, 1));
  solve_result_reset(res);
  dbuf<double> V, Z, w, hdev;
  HIPCHECK(ctx, V.alloc(stride * (R + 1)));
  if (flexible) HIPCHECK(ctx, Z.alloc(stride * R));
  HIPCHECK(ctx, w.alloc(n));
  HIPCHECK(ctx, hdev.alloc(R + 2));
  StreamDrain drain{ctx}; // (declared after the buffers: from here on every return waits for the stream before they are released)
  auto v = [&](int k) { return V + (size_t)k * (size_t)stride; };
  auto z = [&](int k) { return Z + (size_t)k * (size_t)stride; };
  const size_t bytes = sizeof(double) * (size_t)n;
  std::vector<double> hcol(R + 2), y(R);
  GmresColumn q; // Hessenberg matrix, rotations and least-squares right-hand side (the block loop keeps one of these per column)
  q.init(R);
  // the norm a cycle starts from, b being the defect: left v0 = M^-1 b and ||v0||, flexible ||b||
  auto start_norm = [&]() {
    double nn = 0.0;
    int rc = flexible ? DDM_OK : ddm_combined_apply(ctx, prec, v(0), b);
    if (!rc) rc = dot_device(ctx, n, op->owner, flexible ? b : v(0), flexible ? b : v(0), hdev);
    if (!rc) rc = ddm_memcpy_d2h(ctx, &nn, hdev, sizeof(double));
    q.norm = std::sqrt(nn);
    return rc;
  };
  int rc = ddm_op_applyscaleadd(ctx, op, -1.0, x, b); // b -= A x
  if (!rc) rc = start_norm();
  if (rc) return rc;
  const double def0 = q.norm;
  res->def0 = def0;
  if (hist_host) hist_host[0] = def0;
  if (const Defect0 d = classify_initial_defect(def0); d != Defect0::Go) {
    if (d == Defect0::NaN) return fail(ctx, DDM_ENUMERIC, "%s: initial defect is NaN", what);
    res->converged = 1;
    return DDM_OK;
  }
  const auto t0 = std::chrono::steady_clock::now();
  int j = 0;
  bool conv = false;
  while (j < maxit && !conv && !rc) {
    if (flexible) HIPCHECK(ctx, hipMemcpyAsync(v(0), b, bytes, hipMemcpyDeviceToDevice, ctx->stream)); // v0 = b / beta
    hipLaunchKernelGGL(k_scal, dim3(G), dim3(WG), 0, ctx->stream, n, 1.0 / q.norm, v(0));
    q.start_cycle();
    int i = 0;
    for (; i < R && j < maxit && !conv; ++i, ++j) {
      if (flexible) {
        rc = ddm_combined_apply(ctx, prec, z(i), v(i));             // z_i = M^-1 v_i, kept
        if (!rc) rc = ddm_op_apply(ctx, op, z(i), w);               // w = A z_i
      } else {
        rc = ddm_op_apply(ctx, op, v(i), v(i + 1));                 // v[i+1] = A v[i] (temporary)
        if (!rc) rc = ddm_combined_apply(ctx, prec, w, v(i + 1));   // w = M^-1 A v[i]
      }
      for (int k = 0; k <= i && !rc; ++k) {                         // modified Gram-Schmidt
        rc = dot_device(ctx, n, op->owner, v(k), w, hdev + k);
        hipLaunchKernelGGL(k_axpy_negdev, dim3(G), dim3(WG), 0, ctx->stream, n, hdev + k, v(k), w);
      }
      if (!rc) rc = dot_device(ctx, n, op->owner, w, w, hdev + i + 1);
      if (!rc) rc = ddm_memcpy_d2h(ctx, hcol.data(), hdev, sizeof(double) * (size_t)(i + 2));
      if (rc) break;
      const double wnorm = q.take_column(i, hcol.data(), 1);
      if (std::fabs(wnorm) < 1e-80) {
        rc = fail(ctx, DDM_ENUMERIC, "%s: breakdown in GMRes - |w| == 0.0 after %d iterations", what, j);
        break;
      }
      HIPCHECK(ctx, hipMemcpyAsync(v(i + 1), w, bytes, hipMemcpyDeviceToDevice, ctx->stream));
      hipLaunchKernelGGL(k_scal, dim3(G), dim3(WG), 0, ctx->stream, n, 1.0 / wnorm, v(i + 1));
      const double norm = q.rotate(i);
      res->iterations = j + 1;
      if (hist_host) hist_host[j + 1] = norm;
      if (!(norm == norm)) {
        rc = fail(ctx, DDM_ENUMERIC, "%s: defect is NaN in iteration %d", what, j + 1);
        break;
      }
      if (norm < def0 * reduction || norm < 1e-30) conv = true;
    }
    if (rc) break;
    // update(w, i, H, s, v) of dune-istl: solve the triangular system; w = sum_k y_k u_k with u = v (left) or z (flexible); x += w
    q.back_substitute(y.data());
    HIPCHECK(ctx, hipMemsetAsync(w, 0, bytes, ctx->stream));
    for (int a = 0; a < i; ++a) hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, y[a], (const double *)(flexible ? z(a) : v(a)), w);
    hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, 1.0, (const double *)w, x);
    if (!conv && j < maxit) { // restart: b -= A w, then the norm of the next cycle
      rc = ddm_op_applyscaleadd(ctx, op, -1.0, w, b);
      if (!rc) rc = start_norm();
    }
  }
  if (!rc) rc = launch_check(ctx, what);
  rc = krylov_finish(ctx, prec, rc, t0, &res->elapsed_s);
  res->converged = conv ? 1 : 0;
  res->reduction = q.norm / def0;
  return rc;
}

extern "C" int ddm_gmres_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit,
                               int restart, double *hist_host, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !x || !b || !res || x == b || maxit < 0 || restart < 1) return fail(ctx, DDM_EINVAL, "ddm_gmres_solve: bad arguments");
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  return gmres_loop(ctx, "ddm_gmres_solve", false, op, prec, x, b, reduction, maxit, restart, hist_host, res);
}
extern "C" int ddm_fgmres_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit, int restart,
                                double *hist_host, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !x || !b || !res || x == b || maxit < 0 || restart < 1) return fail(ctx, DDM_EINVAL, "ddm_fgmres_solve: bad arguments");
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  return gmres_loop(ctx, "ddm_fgmres_solve", true, op, prec, x, b, reduction, maxit, restart, hist_host, res);
}

// ---- restarted GMRES for m right-hand sides, left-preconditioned and flexible ------------------------
// Every column is what gmres_loop computes on it (the same variant, modified Gram-Schmidt in the order k = 0..i, its own GmresColumn),
// while the operator, the preconditioner and the orthogonalisation sweep run once for all columns.  Restart cycles are aligned.  A
// basis is min(restart, maxit) blocks (V: one more) of n x m doubles, row-major.  Per basis block the sweep is one AXPY over the
// block with the coefficients in device memory, the block dot (one kernel per column group, k_reduce_final_multi) and one all-reduce
// of m doubles (a kernel that fused the AXPY with the partial sums of the next dot was measured slower on MI355X and removed,
// DESIGN.md section 9).  The host reads the (i + 2) x m fresh Hessenberg entries once per iteration and nothing else synchronises
// inside an iteration.
//
// Frozen columns: a column that passed its test is masked out (ctx->mactive) of every kernel of the loop; the operator and the
// preconditioner still run on its (stale) basis entries, whose results nobody reads.  The flexible variant writes V through the mask
// only (v0 comes straight from B), so it zeroes V once per call; the left variant's v0 = M^-1 B is written in every column.
//
// The cycle end is k_gmres_update_multi over V (left) or Z (flexible): W = sum_k y_k u_k; X += W.  The restart of the left variant is
// B -= A W (W = 0 in the columns that are done), v0 = M^-1 B and the block dot; the flexible one puts T = A W into the basis block
// that the next cycle overwrites anyway and runs k_defect_norm_multi (B -= T and the partial sums of the new defect norms in one
// pass; frozen columns of B untouched).

// the sweep of iteration i: hdev[k * m + c] = h_{k,i} of column c for k <= i, hdev[(i + 1) * m + c] = <w, w>; w orthogonalised in place
static int gmres_mgs_multi(ddm_ctx *ctx, ddm_op *op, int m, int i, const double *V, int64_t vstride, double *W, double *hdev)
{
  ScopedTimer t(ctx, "GMRES/orthogonalisation");
  const int64_t n = op->n;
  const int32_t *active = ctx->mactive;
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, V, W, hdev)); // h_0 = <v_0, w>
  for (int k = 0; k <= i; ++k) {
    const double *vk = V + (int64_t)k * vstride;
    const double *z = k < i ? V + (int64_t)(k + 1) * vstride : W; // next dot: <v_{k+1}, w>, or <w, w> at the end
    double *out = hdev + (int64_t)(k + 1) * m;
    hipLaunchKernelGGL(k_axpy_negdev_multi, dim3(grid_for(n * m)), dim3(WG), 0, ctx->stream, n, m, active, (const double *)(hdev + (int64_t)k * m), vk, W);
    DDMCHECK(dot_multi_device(ctx, n, op->owner, m, z, W, out));
  }
  return DDM_OK;
}

// The restart step on its own, for tests: B -= T in the columns with active_host[c] != 0, norm2_host[c] = <B_c, B_c> of every column
// afterwards.  fused != 0: k_defect_norm_multi; fused == 0: the kernels it replaces (k_axpy_negdev_multi with unit coefficients, then
// the block dot of ddm_dot_multi).  Synchronous.
extern "C" int ddm_fgmres_defect_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, const int32_t *active_host, const double *T, double *B, int fused,
                                       double *norm2_host)
{
  if (!ctx || !op || !active_host || !T || !B || T == B || !norm2_host) return fail(ctx, DDM_EINVAL, "ddm_fgmres_defect_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_fgmres_defect_multi"));
  DDMCHECK(ctx_multi_scratch(ctx));
  const int m = nrhs;
  const int64_t n = op->n;
  DDMCHECK(ddm_memcpy_h2d(ctx, ctx->mactive, active_host, sizeof(int32_t) * (size_t)m));
  double *out = ctx->mscal + SCAL_DOT_MULTI * MULTI_MAX;
  if (fused) {
    DDMCHECK(defect_norm_multi(ctx, op, m, T, B, out));
  } else {
    dbuf<double> one;
    HIPCHECK(ctx, one.alloc(m));
    StreamDrain drain{ctx};
    const std::vector<double> ones(m, 1.0);
    DDMCHECK(ddm_memcpy_h2d(ctx, one, ones.data(), sizeof(double) * (size_t)m));
    hipLaunchKernelGGL(k_axpy_negdev_multi, dim3(grid_for(n * m)), dim3(WG), 0, ctx->stream, n, m, (const int32_t *)ctx->mactive, (const double *)one, T, B);
    DDMCHECK(dot_multi_device(ctx, n, op->owner, m, B, B, out));
  }
  return ddm_memcpy_d2h(ctx, norm2_host, out, sizeof(double) * (size_t)m);
}

// the loop for m right-hand sides; what: the exported function's name, for messages
static int gmres_loop_multi(ddm_ctx *ctx, const char *what, bool flexible, ddm_op *op, ddm_combined *prec, int m, double *X, double *B, double reduction,
                            int maxit, int restart, double *hist_host, ddm_solve_result *res)
{
  const int64_t n = op->n;
  const int64_t vstride = std::max<int64_t>(n, 1) * m;
  const int R = std::min(restart, std::max(maxit, 1)); // a cycle never gets longer than maxit iterations: no basis block beyond that
  DDMCHECK(gmres_memory_check(ctx, what, (flexible ? 2 : 1) * (int64_t)R + 2, n, m));
  for (int c = 0; c < m; ++c) solve_result_reset(&res[c]);
  DDMCHECK(ctx_multi_scratch(ctx));
  dbuf<double> Vb, Zb, Wb, hdev, ydev;
  dbuf<int32_t> cdev; // [0, m): Hessenberg columns per column in the cycle, [m, 2m): keep W (still running)
  HIPCHECK(ctx, Vb.alloc(vstride * (R + 1)));
  if (flexible) HIPCHECK(ctx, Zb.alloc(vstride * R));
  HIPCHECK(ctx, Wb.alloc(vstride));
  HIPCHECK(ctx, hdev.alloc((int64_t)(R + 2) * m));
  HIPCHECK(ctx, ydev.alloc((int64_t)R * m));
  HIPCHECK(ctx, cdev.alloc(2 * m));
  StreamDrain drain{ctx}; // (declared after the buffers: from here on every return waits for the stream before they are released)
  double *V = Vb, *Z = Zb, *W = Wb;
  auto v = [&](int k) { return V + (int64_t)k * vstride; };
  auto z = [&](int k) { return Z + (int64_t)k * vstride; };
  std::vector<GmresColumn> col(m);
  for (auto &q : col) q.init(R);
  std::vector<double> hcol((size_t)(R + 2) * m), yhost((size_t)R * m), ycol(R);
  int32_t cflags[2 * MULTI_MAX];
  MultiCoef coef;
  MultiFrame f{ctx, what, m, reduction, hist_host, res};
  const int GE = grid_for(n * m);
  // flexible: the basis is written through the mask only: a frozen column's entries, which the preconditioner still reads, start as zeros
  if (flexible) HIPCHECK(ctx, hipMemsetAsync(V, 0, sizeof(double) * (size_t)(vstride * (R + 1)), ctx->stream));

  // b -= A x, then the norm the first cycle starts from, per column: left v0 = M^-1 b and |v0|, flexible |b|
  DDMCHECK(op_applyscaleadd_multi(ctx, op, m, -1.0, X, B));
  if (!flexible) DDMCHECK(combined_apply_multi_impl(ctx, prec, m, v(0), B));
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, flexible ? B : v(0), flexible ? B : v(0), hdev));
  DDMCHECK(ddm_memcpy_d2h(ctx, hcol.data(), hdev, sizeof(double) * (size_t)m));
  DDMCHECK(multi_start(f, hcol.data()));
  for (int c = 0; c < m; ++c) col[c].norm = res[c].def0;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = DDM_OK, j = 0;
  while (j < maxit && f.nactive > 0 && !rc) {
    for (int c = 0; c < m; ++c) {
      GmresColumn &q = col[c];
      q.cnt = 0;
      coef.a[c] = f.active[c] ? 1.0 / q.norm : 0.0;
      if (f.active[c]) q.start_cycle();
    }
    // v0 = (left: M^-1 b, in place; flexible: b) / norm
    hipLaunchKernelGGL(k_scale_into_multi, dim3(GE), dim3(WG), 0, ctx->stream, n, m, (const int32_t *)ctx->mactive, coef, (const double *)(flexible ? B : v(0)), v(0));
    int i = 0;
    for (; i < R && j < maxit && f.nactive > 0; ++i, ++j) {
      if (flexible) {
        rc = combined_apply_multi_impl(ctx, prec, m, z(i), v(i));             // z_i = M^-1 v_i, kept
        if (!rc) rc = op_apply_multi(ctx, op, m, z(i), W);                    // w = A z_i
      } else {
        rc = op_apply_multi(ctx, op, m, v(i), v(i + 1));                      // v[i+1] = A v[i] (temporary)
        if (!rc) rc = combined_apply_multi_impl(ctx, prec, m, W, v(i + 1));   // w = M^-1 A v[i]
      }
      if (!rc) rc = gmres_mgs_multi(ctx, op, m, i, V, vstride, W, hdev);
      if (!rc) rc = ddm_memcpy_d2h(ctx, hcol.data(), hdev, sizeof(double) * (size_t)(i + 2) * m); // the one read-back of the iteration
      if (rc) break;
      for (int c = 0; c < m && !rc; ++c) {
        coef.a[c] = 0.0;
        if (!f.active[c]) continue;
        const double wnorm = col[c].take_column(i, hcol.data() + c, (size_t)m);
        if (std::fabs(wnorm) < 1e-80) rc = fail(ctx, DDM_ENUMERIC, "%s: breakdown in GMRes - |w| == 0.0 after %d iterations (column %d)", what, j, c);
        coef.a[c] = 1.0 / wnorm;
      }
      if (rc) break;
      hipLaunchKernelGGL(k_scale_into_multi, dim3(GE), dim3(WG), 0, ctx->stream, n, m, (const int32_t *)ctx->mactive, coef, (const double *)W, v(i + 1));
      for (int c = 0; c < m && !rc; ++c)
        if (f.active[c]) rc = multi_record(f, c, j + 1, col[c].rotate(i));
      if (!rc) rc = multi_upload_mask(f);
      if (rc) break;
    }
    if (rc) break;
    // update(w, i, H, s, v) per column: solve its triangular system of cnt_c unknowns; W_c = sum_k y_k u_k (u = v or z); X_c += W_c
    std::fill(yhost.begin(), yhost.end(), 0.0);
    for (int c = 0; c < m; ++c) {
      GmresColumn &q = col[c];
      cflags[c] = q.cnt;
      cflags[m + c] = f.active[c];
      q.back_substitute(ycol.data());
      for (int a = 0; a < q.cnt; ++a) yhost[(size_t)a * m + c] = ycol[a];
    }
    rc = ddm_memcpy_h2d(ctx, ydev, yhost.data(), sizeof(double) * (size_t)i * m);
    if (!rc) rc = ddm_memcpy_h2d(ctx, cdev, cflags, sizeof(int32_t) * (size_t)(2 * m));
    if (rc) break;
    {
      ScopedTimer t(ctx, "GMRES/update");
      hipLaunchKernelGGL(k_gmres_update_multi, dim3(GE), dim3(WG), 0, ctx->stream, n, m, (const int32_t *)cdev, (const int32_t *)(cdev + m), (const double *)ydev,
                         (const double *)(flexible ? Z : V), vstride, W, X);
    }
    if (f.nactive > 0 && j < maxit) { // restart: the defect and the norm of the next cycle in the running columns
      if (flexible) {
        rc = op_apply_multi(ctx, op, m, W, v(0));                             // t = A w into v0 (overwritten by the next cycle)
        if (!rc) rc = defect_norm_multi(ctx, op, m, v(0), B, hdev);         // b -= t and |b|
      } else {
        rc = op_applyscaleadd_multi(ctx, op, m, -1.0, W, B);                  // b -= A w (w = 0 in the columns that are done)
        if (!rc) rc = combined_apply_multi_impl(ctx, prec, m, v(0), B);       // v0 = M^-1 b
        if (!rc) rc = dot_multi_device(ctx, n, op->owner, m, v(0), v(0), hdev);
      }
      if (!rc) rc = ddm_memcpy_d2h(ctx, hcol.data(), hdev, sizeof(double) * (size_t)m);
      for (int c = 0; c < m && !rc; ++c)
        if (f.active[c]) col[c].norm = std::sqrt(hcol[c]);
    }
  }
  if (!rc) rc = launch_check(ctx, what);
  return multi_finish(f, prec, rc, t0);
}

extern "C" int ddm_gmres_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit,
                                     int restart, double *hist_host, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !X || !B || !res || X == B || maxit < 0 || restart < 1)
    return fail(ctx, DDM_EINVAL, "ddm_gmres_solve_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_gmres_solve_multi"));
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  return gmres_loop_multi(ctx, "ddm_gmres_solve_multi", false, op, prec, nrhs, X, B, reduction, maxit, restart, hist_host, res);
}
extern "C" int ddm_fgmres_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit,
                                      int restart, double *hist_host, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !X || !B || !res || X == B || maxit < 0 || restart < 1)
    return fail(ctx, DDM_EINVAL, "ddm_fgmres_solve_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_fgmres_solve_multi"));
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  return gmres_loop_multi(ctx, "ddm_fgmres_solve_multi", true, op, prec, nrhs, X, B, reduction, maxit, restart, hist_host, res);
}
