// BiCGSTAB: one right-hand side, and any number of them queued through a block of fixed width.  Needs krylov_frame.hpp.
#pragma once

// ---- BiCGSTAB ------------------------------------------------------------------------------------
// dune-istl BiCGSTABSolver::apply ([solver] type = bicgstabsolver; DUNE 2.10 solvers.hh, not in the snapshot -- restated in
// oracle/apply_oracle.py::bicgstab_solve): right-preconditioned, two half steps per iteration, the defect norm is tested after each
// half step (hist_host receives both: up to 2 maxit + 1 entries); result.iterations = ceil of the half-step counter, as dune-istl reports.
extern "C" int ddm_bicgstab_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit, double *hist_host,
                                  int32_t *nhist, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !x || !b || !res) return fail(ctx, DDM_EINVAL, "ddm_bicgstab_solve: bad arguments");
  const int64_t n = op->n;
  const int G = grid_for(n);
  const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(n, 1);
  dbuf<double> buf[5]; // rt, p, v, y, t
  StreamDrain drain{ctx}; // (declared after the buffers: every return waits for the stream before they are released)
  for (auto &q : buf)
    if (q.alloc(n) != hipSuccess) return fail(ctx, DDM_EHIP, "ddm_bicgstab_solve: allocation failed");
  double *rt = buf[0], *p = buf[1], *v = buf[2], *y = buf[3], *t = buf[4], *r = b;
  const double EPS = 1e-80;
  const bool verbose = std::getenv("DDM_KRYLOV_VERBOSE") != nullptr;
  int rc = ddm_op_applyscaleadd(ctx, op, -1.0, x, r); // r = b - A x (b is overwritten by the defect, as in dune-istl)
  if (rc) return rc;
  HIPCHECK(ctx, hipMemcpyAsync(rt, r, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  double norm = 0.0;
  if ((rc = ddm_norm(ctx, op, r, &norm))) return rc;
  const double def0 = norm;
  solve_result_reset(res);
  res->def0 = def0;
  int nh = 0;
  if (hist_host) hist_host[nh] = def0;
  ++nh;
  if (const Defect0 d = classify_initial_defect(def0); d != Defect0::Go) {
    if (d == Defect0::NaN) return fail(ctx, DDM_ENUMERIC, "initial defect is NaN");
    res->converged = 1;
    if (nhist) *nhist = nh;
    return DDM_OK;
  }
  HIPCHECK(ctx, hipMemsetAsync(p, 0, bytes, ctx->stream));
  HIPCHECK(ctx, hipMemsetAsync(v, 0, bytes, ctx->stream));
  double rho = 1.0, alpha = 1.0, omega = 1.0, rho_new = 0.0, h = 0.0;
  const auto t0 = std::chrono::steady_clock::now();
  double it = 0.5;
  bool conv = false;
  auto record = [&](double nrm) {
    if (hist_host) hist_host[nh] = nrm;
    ++nh;
    res->reduction = nrm / def0;
    return nrm <= def0 * reduction;
  };
  for (; it < maxit && !rc; it += 0.5) {
    if ((rc = ddm_dot(ctx, op, rt, r, &rho_new))) break;
    if (verbose) std::fprintf(stderr, "[ddm bicgstab] it %.1f rho_new %.17g rho %.17g alpha %.17g omega %.17g norm %.17g\n", it, rho_new, rho, alpha, omega, norm);
    if (std::fabs(rho) <= EPS) { rc = fail(ctx, DDM_ENUMERIC, "breakdown in BiCGSTAB - rho %g <= EPSILON after %g iterations", rho, it); break; }
    if (std::fabs(omega) <= EPS) { rc = fail(ctx, DDM_ENUMERIC, "breakdown in BiCGSTAB - omega %g <= EPSILON after %g iterations", omega, it); break; }
    if (it < 1) {
      HIPCHECK(ctx, hipMemcpyAsync(p, r, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
      const double beta = (rho_new / rho) * (alpha / omega);
      hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, -omega, (const double *)v, p); // p = r + beta (p - omega v)
      hipLaunchKernelGGL(k_scal, dim3(G), dim3(WG), 0, ctx->stream, n, beta, p);
      hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, 1.0, (const double *)r, p);
    }
    if ((rc = ddm_combined_apply(ctx, prec, y, p))) break;  // y = W^-1 p
    if ((rc = ddm_op_apply(ctx, op, y, v))) break;           // v = A y
    if ((rc = ddm_dot(ctx, op, rt, v, &h))) break;
    if (std::fabs(h) < EPS) { rc = fail(ctx, DDM_ENUMERIC, "abs(h) < EPSILON in BiCGSTAB - abort"); break; }
    alpha = rho_new / h;
    hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, alpha, (const double *)y, x);
    hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, -alpha, (const double *)v, r);
    if ((rc = ddm_norm(ctx, op, r, &norm))) break;
    if (record(norm)) { conv = true; break; }
    it += 0.5;
    if ((rc = ddm_combined_apply(ctx, prec, y, r))) break;  // y = W^-1 r
    if ((rc = ddm_op_apply(ctx, op, y, t))) break;           // t = A y
    double tt = 0.0, tr = 0.0;
    if ((rc = ddm_dot(ctx, op, t, t, &tt))) break;
    if ((rc = ddm_dot(ctx, op, t, r, &tr))) break;
    omega = tr / tt;
    hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, omega, (const double *)y, x);
    hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, -omega, (const double *)t, r);
    rho = rho_new;
    if ((rc = ddm_norm(ctx, op, r, &norm))) break;
    if (record(norm)) { conv = true; break; }
  }
  if (rc) return rc;
  rc = krylov_finish(ctx, prec, rc, t0, &res->elapsed_s);
  res->iterations = (int32_t)std::ceil(std::min(it, (double)maxit));
  res->converged = conv ? 1 : 0;
  if (nhist) *nhist = nh;
  return rc;
}

// ---- BiCGSTAB for any number of right-hand sides through a block of fixed width --------------------------------------------------------
// ncols columns queue for the `width` slots of one block loop, under the protocol of ddm_cg_solve_queue (MultiFrame, the mask
// ctx->mactive, the slot -> column table, store / refill at the boundary).  Every column is what ddm_bicgstab_solve computes on it:
// right-preconditioned, two half steps per iteration, `norm <= def0 * reduction` tested after each, def0 < 1e-30 converged at once,
// iterations = ceil(half steps / 2), maxit full iterations.  A slot's state is seven vectors (x, r, rt, p, v, y, t: n x width work
// blocks of the preconditioner object) and three scalars (rho, alpha, omega, on the device); B is only read.
//   iteration  beta and p = r + beta (p - omega v); y = W^-1 p; v = A y; h = <rt, v>; alpha = rho_new / h; x += alpha y, r -= alpha v
//              and <r, r>: the host reads <r, r>, h and the rho and omega that beta used in ONE copy, runs the single driver's breakdown
//              checks on them (|rho| <= 1e-80, |omega| <= 1e-80, |h| < 1e-80) and tests the defect.  A column that passes is masked
//              out of the second half step: its x, r and scalars do not change.  Then y = W^-1 r; t = A y; <t, t> and <t, r>;
//              omega = <t, r> / <t, t>, rho = rho_new; x += omega y, r -= omega t with <r, r> and the next rho_new = <rt, r>: the
//              host reads the defects.
//   boundary   one per iteration, after the second half step: every slot whose column stopped in either half step or reached maxit is
//              stored and released; the freed slots take the next columns in ascending slot order (x = X[:, j], r = B[:, j],
//              p = v = 0, rho = alpha = omega = 1), then under a mask of the loaded slots only r -= A x with its norm, rt = r and
//              rho_new = <r, r>.  A loaded column with def0 < 1e-30 (or maxit = 0) is finished at once and its slot refilled again
//              at the same boundary.
// A fresh slot needs no special first step: with p = v = 0 the direction update, evaluated as the single driver evaluates it
// (p += (-omega) v; p *= beta; p += r), yields p = r exactly -- the `it < 1` branch of the single driver -- so every step is the
// general step and the slots need not be aligned.  A column's numbers do not depend on whether it entered at the start or through a
// refill: both are this one load path.  A breakdown or a NaN in a running column ends the call with DDM_ENUMERIC: the columns stored
// before keep their results, X[:, j] of the others is as on entry.
// Vector work per iteration, in passes over n x w doubles (every load and store of a block entry a kernel issues counts 1): one
// simple kernel per update and one block dot per sum, 8 + 8 for the first half step and 4 + 6 + 4 for the second: 30, plus the block
// dot for h = <rt, v> (2 more).  A form with fused update-and-sum kernels (19 passes) was measured slower on MI355X and removed
// (DESIGN.md section 9).
extern "C" int ddm_bicgstab_solve_queue(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int64_t ncols, int width, double *X, double *B, double reduction,
                                        int maxit, double *hist_host, int32_t *nhist, ddm_solve_result *res)
{
  const char *what = "ddm_bicgstab_solve_queue";
  if (width < 1 || width > MULTI_MAX) return fail(ctx, DDM_EINVAL, "%s: width = %d outside [1, %d]", what, width, MULTI_MAX);
  if (ncols < 1) return fail(ctx, DDM_EINVAL, "%s: ncols = %lld, at least one column is needed", what, (long long)ncols);
  if (!ctx || !op || !prec || !X || !B || !res || X == B || maxit < 0) return fail(ctx, DDM_EINVAL, "%s: bad arguments", what);
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  const int w = width;
  const int64_t n = op->n;
  const double EPS = 1e-80;
  for (int64_t j = 0; j < ncols; ++j) solve_result_reset(&res[j]);
  if (nhist) std::fill(nhist, nhist + ncols, 0);
  DDMCHECK(ctx_multi_scratch(ctx));
  HIPCHECK(ctx, prec->work.reserve(w, n, 7));
  StreamDrain drain{ctx}; // every return waits for the kernels that read the caller's blocks
  dbuf<double> *blk = prec->work.block;
  double *P = blk[0], *T = blk[1], *XW = blk[2], *R = blk[3], *RT = blk[4], *V = blk[5], *Y = blk[6]; // p, t; the slots' x and defect r; shadow defect, v, y
  int64_t *tabdev = prec->work.tab; // (slot, column) pairs of one load or store launch
  if (n > 0) // a slot that never holds a column stays zero
    for (double *blk : {P, XW, R, RT, V}) HIPCHECK(ctx, hipMemsetAsync(blk, 0, sizeof(double) * (size_t)(n * w), ctx->stream));
  double *scal = ctx->mscal;
  HIPCHECK(ctx, hipMemsetAsync(scal, 0, sizeof(double) * (size_t)(BICG_SCALARS * MULTI_MAX), ctx->stream));
  double *half1 = scal + BICG_HALF1 * MULTI_MAX, *half2 = scal + BICG_HALF2 * MULTI_MAX, *loaddev = scal + BICG_LOAD * MULTI_MAX, *ttdev = scal + BICG_TT * MULTI_MAX;
  const int32_t *active = ctx->mactive;
  const uint8_t *owner = op->owner;
  const int GE = grid_for(n * w);
  double rd[4 * MULTI_MAX];
  ddm_solve_result sres[MULTI_MAX]; // the slots' results; a released column's entry is copied to res
  int64_t column[MULTI_MAX], tab[2 * MULTI_MAX];
  int32_t mask[MULTI_MAX], nhalf[MULTI_MAX];
  for (int s = 0; s < w; ++s) solve_result_reset(&sres[s]), column[s] = -1, nhalf[s] = 0;
  MultiFrame f{ctx, what, w, reduction, nullptr, sres};
  f.column = column;
  std::fill(f.active, f.active + w, 0);
  int64_t next = 0; // head of the queue
  auto upload_table = [&](int npairs) { return ddm_memcpy_h2d(ctx, tabdev, tab, sizeof(int64_t) * 2 * (size_t)npairs); };
  auto launch_ok = [&]() { return launch_check(ctx, what); };
  // slot s is done with its column: the result entry goes to the caller (x has been stored, or never changed)
  auto release = [&](int s) {
    ddm_solve_result &r = res[column[s]] = sres[s];
    r.iterations = (nhalf[s] + 1) / 2;
    if (r.def0 >= 1e-30) r.reduction = f.def[s] / r.def0;
    if (nhist) nhist[column[s]] = nhalf[s] + 1;
    column[s] = -1;
  };
  // a running slot after a half step: history, NaN, the single driver's stop test; a column that passes leaves the mask
  auto record = [&](int s, double norm2) -> int {
    const double def = f.def[s] = std::sqrt(norm2);
    nhalf[s] += 1;
    if (hist_host) hist_host[(int64_t)nhalf[s] * ncols + column[s]] = def;
    if (!(def == def)) return fail(ctx, DDM_ENUMERIC, "%s: defect is NaN after half step %d of column %lld", what, nhalf[s], (long long)column[s]);
    if (def <= sres[s].def0 * reduction) {
      sres[s].converged = 1;
      f.active[s] = 0;
      f.nactive -= 1;
      f.changed = true;
    }
    return DDM_OK;
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
      hipLaunchKernelGGL(k_bicg_column_load_multi, dim3(grid_for(n * nload)), dim3(WG), 0, ctx->stream, n, w, nload, (const int64_t *)tabdev, ncols,
                         (const double *)X, (const double *)B, XW, R, P, V, scal);
      DDMCHECK(launch_ok());
      DDMCHECK(ddm_memcpy_h2d(ctx, ctx->mactive, mask, sizeof(int32_t) * (size_t)w)); // the defect pass writes the loaded slots only
      DDMCHECK(op_apply_multi(ctx, op, w, XW, T));                                     // t = A x (t is free between two iterations)
      DDMCHECK(defect_norm_multi(ctx, op, w, T, R, loaddev));                        // r -= t; <r, r>
      hipLaunchKernelGGL(k_bicg_shadow_multi, dim3(GE), dim3(WG), 0, ctx->stream, n, w, active, (const double *)R, RT, scal); // rt = r; rho_new = <r, r>
      DDMCHECK(launch_ok());
      DDMCHECK(ddm_memcpy_d2h(ctx, rd, loaddev, sizeof(double) * (size_t)w));
      for (int k = 0; k < nload; ++k) {
        const int s = (int)tab[2 * k];
        solve_result_reset(&sres[s]);
        nhalf[s] = 0;
        const double def0 = f.def[s] = std::sqrt(rd[s]);
        sres[s].def0 = def0;
        if (hist_host) hist_host[column[s]] = def0;
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
  auto axpy = [&](const double *coef, double sign, const double *x, double *y) {
    hipLaunchKernelGGL(k_axpy_dev_multi, dim3(GE), dim3(WG), 0, ctx->stream, n, w, active, coef, sign, x, y);
  };
  // first half step; leaves <r, r>, h and the operands of the breakdown checks in half1
  auto half_step_1 = [&]() -> int {
    hipLaunchKernelGGL(k_bicg_beta_multi, dim3(1), dim3(64), 0, ctx->stream, w, active, scal);
    axpy(scal + BICG_OMEGA * MULTI_MAX, -1.0, V, P); // p = r + beta (p - omega v)
    hipLaunchKernelGGL(k_scal_dev_multi, dim3(GE), dim3(WG), 0, ctx->stream, n, w, active, (const double *)(scal + BICG_BETA * MULTI_MAX), P);
    axpy(nullptr, 1.0, R, P);
    DDMCHECK(launch_ok());
    DDMCHECK(combined_apply_multi_impl(ctx, prec, w, Y, P));          // y = W^-1 p
    DDMCHECK(op_apply_multi(ctx, op, w, Y, V));                       // v = A y
    DDMCHECK(dot_multi_device(ctx, n, owner, w, RT, V, half1 + w));   // h = <rt, v>
    hipLaunchKernelGGL(k_bicg_alpha_multi, dim3(1), dim3(64), 0, ctx->stream, w, active, scal); // alpha = rho_new / h
    axpy(scal + BICG_ALPHA * MULTI_MAX, 1.0, Y, XW); // x += alpha y; r -= alpha v; <r, r>
    axpy(scal + BICG_ALPHA * MULTI_MAX, -1.0, V, R);
    DDMCHECK(launch_ok());
    return dot_multi_device(ctx, n, owner, w, R, R, half1);
  };
  // second half step; leaves <r, r> and the next rho_new in half2
  auto half_step_2 = [&]() -> int {
    DDMCHECK(combined_apply_multi_impl(ctx, prec, w, Y, R));          // y = W^-1 r
    DDMCHECK(op_apply_multi(ctx, op, w, Y, T));                       // t = A y
    DDMCHECK(dot_multi_device(ctx, n, owner, w, T, T, ttdev));
    DDMCHECK(dot_multi_device(ctx, n, owner, w, T, R, ttdev + w));
    hipLaunchKernelGGL(k_bicg_omega_multi, dim3(1), dim3(64), 0, ctx->stream, w, active, scal); // omega = <t, r> / <t, t>; rho = rho_new
    axpy(scal + BICG_OMEGA * MULTI_MAX, 1.0, Y, XW); // x += omega y; r -= omega t; <r, r> and <rt, r>
    axpy(scal + BICG_OMEGA * MULTI_MAX, -1.0, T, R);
    DDMCHECK(launch_ok());
    DDMCHECK(dot_multi_device(ctx, n, owner, w, R, R, half2));
    // (the block dot writes every column: the rho_new of a slot that sits out this half step is overwritten, and never read again --
    //  the slot is stored at this boundary)
    return dot_multi_device(ctx, n, owner, w, RT, R, half2 + w);
  };
  int rc = refill();
  (void)hipStreamSynchronize(ctx->stream);
  const auto t0 = std::chrono::steady_clock::now();
  while (f.nactive > 0 && !rc) {
    rc = half_step_1();
    if (!rc) rc = ddm_memcpy_d2h(ctx, rd, half1, sizeof(double) * 4 * (size_t)w); // the one read of the half step
    for (int s = 0; s < w && !rc; ++s) {
      if (!f.active[s]) continue;
      const double h = rd[w + s], rho = rd[2 * w + s], omega = rd[3 * w + s];
      const long long j = (long long)column[s];
      if (std::fabs(rho) <= EPS) rc = fail(ctx, DDM_ENUMERIC, "%s: breakdown in BiCGSTAB - rho %g <= EPSILON after %d half steps of column %lld", what, rho, nhalf[s], j);
      else if (std::fabs(omega) <= EPS) rc = fail(ctx, DDM_ENUMERIC, "%s: breakdown in BiCGSTAB - omega %g <= EPSILON after %d half steps of column %lld", what, omega, nhalf[s], j);
      else if (std::fabs(h) < EPS) rc = fail(ctx, DDM_ENUMERIC, "%s: abs(h) < EPSILON in BiCGSTAB - abort (h %g after %d half steps of column %lld)", what, h, nhalf[s], j);
      else if (!(rho == rho) || !(omega == omega) || !(h == h))
        rc = fail(ctx, DDM_ENUMERIC, "%s: %s is NaN after %d half steps of column %lld", what, !(rho == rho) ? "rho" : !(omega == omega) ? "omega" : "h", nhalf[s], j);
      else rc = record(s, rd[s]);
    }
    if (rc) break;
    if (f.nactive > 0) { // (a column that stopped after the first half step sits out the second)
      rc = multi_upload_mask(f);
      if (!rc) rc = half_step_2();
      if (!rc) rc = ddm_memcpy_d2h(ctx, rd, half2, sizeof(double) * (size_t)w);
      for (int s = 0; s < w && !rc; ++s) {
        if (!f.active[s]) continue;
        rc = record(s, rd[s]);
        if (!rc && f.active[s] && nhalf[s] >= 2 * maxit) { // out of iterations: leaves its slot unconverged
          f.active[s] = 0;
          f.nactive -= 1;
          f.changed = true;
        }
      }
      if (rc) break;
    }
    // the boundary: every slot whose column stopped in this iteration is stored and released, then refilled
    int nstore = 0;
    for (int s = 0; s < w; ++s)
      if (column[s] >= 0 && !f.active[s]) tab[2 * nstore] = s, tab[2 * nstore + 1] = column[s], ++nstore;
    if (nstore > 0) {
      rc = upload_table(nstore);
      if (rc) break;
      hipLaunchKernelGGL(k_column_store_multi, dim3(grid_for(n * nstore)), dim3(WG), 0, ctx->stream, n, w, nstore, (const int64_t *)tabdev, ncols, (const double *)XW, X);
      if ((rc = launch_ok())) break;
      for (int k = 0; k < nstore; ++k) release((int)tab[2 * k]);
    }
    rc = nstore > 0 && next < ncols ? refill() : multi_upload_mask(f);
  }
  if (!rc) rc = launch_ok();
  rc = multi_finish(f, prec, rc, t0); // (drains the stream; the elapsed time of the call lands in the slots' entries)
  for (int64_t j = 0; j < ncols; ++j) res[j].elapsed_s = sres[0].elapsed_s;
  return rc;
}
