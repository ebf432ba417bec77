// The Krylov drivers: CG (begin / steps / defect / solve), restarted GMRES and BiCGSTAB for one right-hand side; CG and restarted GMRES
// for m right-hand sides at once (m independent recurrences in one loop, not block-Krylov methods); CG for any number of right-hand
// sides queued through a block of fixed width (ddm_cg_solve_queue), and BiCGSTAB likewise (ddm_bicgstab_solve_queue).  Restarted GMRES is one algorithm
// with two variants, left-preconditioned and flexible (right-preconditioned, the preconditioned directions kept): one loop per vector
// count (gmres_loop, gmres_loop_multi) behind the four entry points ddm_gmres_solve, ddm_fgmres_solve, ddm_gmres_solve_multi and
// ddm_fgmres_solve_multi.  All drivers share the frame around the loop (solve_result_reset, classify_initial_defect, krylov_finish), the
// block drivers the MultiFrame as well; both GMRES loops run their host arithmetic through the same GmresColumn, which is what keeps
// the host side of a block column bit-identical to the single-vector solve.  Flexible CG, restarted and complete, is likewise one loop per
// vector count (fcg_loop, fcg_loop_multi) behind ddm_fcg_solve and ddm_fcg_solve_multi; ddm_fcg_orth_multi runs its orthogonalisation on
// its own for tests.  Block CG (ddm_bcg_solve_multi, with ddm_bcg_gram_multi / ddm_bcg_update_multi / ddm_bcg_direction_multi for tests) is
// the one symmetric driver whose columns share a search space; block GMRES (ddm_bgmres_solve_multi, with ddm_bgmres_project_multi /
// ddm_bgmres_combine_multi / ddm_bgmres_combine_gram_multi for tests) is its non-symmetric companion.  Device scalars are the slots SCAL_*
// (kernels.hpp) and BICG_* (multi_kernels.hpp); the block drivers' work blocks come from prec->work (krylov_work.hpp).  Needs preconditioners.hpp.
#pragma once

// synchronises the context's stream when it goes out of scope: the Krylov drivers declare it AFTER their work arrays, so that an
// early return waits for the enqueued kernels before the arrays are released
struct StreamDrain {
  ddm_ctx *ctx;
  ~StreamDrain() { (void)hipStreamSynchronize(ctx->stream); }
};

// ---- the frame around every Krylov loop --------------------------------------------------------
static void solve_result_reset(ddm_solve_result *res) { *res = ddm_solve_result{0, 0, 0.0, 1.0, 0.0}; }
// what the initial defect norm says about the loop: do not start (NaN: an error; below 1e-30: already converged) or go
enum class Defect0 { NaN, Zero, Go };
static Defect0 classify_initial_defect(double def0) { return !(def0 == def0) ? Defect0::NaN : def0 < 1e-30 ? Defect0::Zero : Defect0::Go; }
// End of a driver: drains the stream, stops the clock (*elapsed_s: seconds since t0), then asks whether a persistent local solve gave
// up during the loop (its results are invalid then).  An earlier error rc is passed through.
static int krylov_finish(ddm_ctx *ctx, const ddm_combined *prec, int rc, std::chrono::steady_clock::time_point t0, double *elapsed_s)
{
  (void)hipStreamSynchronize(ctx->stream);
  *elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (rc || !prec->schwarz) return rc;
  int st = 0;
  rc = ddm_ilu0_status(ctx, prec->schwarz->solver, &st);
  if (!rc && st) rc = fail(ctx, DDM_ENUMERIC, "persistent triangular solve timed out waiting for a level (results invalid)");
  return rc;
}

// ---- the frame around every block loop (m right-hand sides) ---------------------------------------
// What a block driver keeps per column next to its recurrence: the host copy of the device-side mask ctx->mactive (a column that is
// done is frozen through it) and the latest defect norm.
struct MultiFrame {
  ddm_ctx *ctx;
  const char *what; // the exported function's name, for messages
  int m;
  double reduction;
  double *hist_host; // (maxit + 1) x m, row-major, or null
  ddm_solve_result *res;
  int32_t active[MULTI_MAX];
  double def[MULTI_MAX];
  int nactive = 0;
  bool changed = false; // active[] differs from ctx->mactive
  const int64_t *column = nullptr; // queue driver: column[c] = the caller's column that slot c holds (messages name it); null: c itself
};
// The initial defects (norm2[c]: the squared norm of column c): def0 and the first history row; a column that needs no iteration is
// converged and masked out from the start; the mask goes to the device.
static int multi_start(MultiFrame &f, const double *norm2)
{
  for (int c = 0; c < f.m; ++c) {
    const double def0 = f.def[c] = std::sqrt(norm2[c]);
    f.res[c].def0 = def0;
    if (f.hist_host) f.hist_host[c] = def0;
    const Defect0 d = classify_initial_defect(def0);
    if (d == Defect0::NaN) return fail(f.ctx, DDM_ENUMERIC, "%s: initial defect is NaN in column %d", f.what, c);
    f.active[c] = d == Defect0::Go ? 1 : 0;
    if (!f.active[c]) f.res[c].converged = 1;
    f.nactive += f.active[c];
  }
  return ddm_memcpy_h2d(f.ctx, f.ctx->mactive, f.active, sizeof(int32_t) * (size_t)f.m);
}
// A running column after iteration `it`: its defect norm goes into the result and the history; NaN is an error; a column that passes
// the stop test leaves the mask (multi_upload_mask sends the mask once all columns of the iteration are through).
static int multi_record(MultiFrame &f, int c, int it, double def)
{
  f.def[c] = def;
  f.res[c].iterations = it;
  if (f.hist_host) f.hist_host[(int64_t)it * f.m + c] = def;
  if (!(def == def)) return fail(f.ctx, DDM_ENUMERIC, "%s: defect is NaN in iteration %d (column %lld)", f.what, it, (long long)(f.column ? f.column[c] : c));
  if (def < f.res[c].def0 * f.reduction || def < 1e-30) {
    f.res[c].converged = 1;
    f.active[c] = 0;
    f.nactive -= 1;
    f.changed = true;
  }
  return DDM_OK;
}
static int multi_upload_mask(MultiFrame &f)
{
  if (!f.changed) return DDM_OK;
  f.changed = false;
  return ddm_memcpy_h2d(f.ctx, f.ctx->mactive, f.active, sizeof(int32_t) * (size_t)f.m);
}
// krylov_finish for m columns: the elapsed time and the reduction reached go into every result
static int multi_finish(MultiFrame &f, const ddm_combined *prec, int rc, std::chrono::steady_clock::time_point t0)
{
  double elapsed = 0.0;
  rc = krylov_finish(f.ctx, prec, rc, t0, &elapsed);
  for (int c = 0; c < f.m; ++c) {
    f.res[c].elapsed_s = elapsed;
    if (f.res[c].def0 >= 1e-30) f.res[c].reduction = f.def[c] / f.res[c].def0;
  }
  return rc;
}

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

// what the basis (bases) and the work block need against the free device memory: DDM_ENOTIMPL before anything is allocated.
// blocks: R + 2 (left), 2 R + 2 (flexible) of n x m doubles
static int gmres_memory_check(ddm_ctx *ctx, const char *what, int64_t blocks, int64_t n, int m)
{
  size_t free_b = 0, total_b = 0;
  HIPCHECK(ctx, hipMemGetInfo(&free_b, &total_b));
  const double need = (double)blocks * (double)(std::max<int64_t>(n, 1) * m) * sizeof(double);
  if (need > (double)free_b)
    return fail(ctx, DDM_ENOTIMPL, "%s: the Krylov basis and the work block, %lld blocks of %lld x %d doubles, need %.0f bytes, %zu are free", what,
                (long long)blocks, (long long)n, m, need, free_b);
  return DDM_OK;
}

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
  if (!rc && hipGetLastError() != hipSuccess) rc = fail(ctx, DDM_EHIP, "kernel launch failed in %s", what);
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

// B -= T in the columns of ctx->mactive; out (m device doubles) = owner-masked <B_c, B_c>, summed over the ranks (the restart of the
// flexible GMRES block loop and the initial defect of the slots that ddm_cg_solve_queue refills)
static int defect_norm_multi(ddm_ctx *ctx, ddm_op *op, int m, const double *T, double *B, double *out)
{
  const int64_t n = op->n;
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  for_column_groups(m, [&](int c0, int cb) {
    DDM_MULTI_CB_DISPATCH(k_defect_norm_multi, op->owner != nullptr, cb, dim3(nb), dim3(WG), 0, ctx->stream, n, m, c0, (const int32_t *)ctx->mactive,
                          (const uint8_t *)op->owner, T, B, ctx->mpartial);
  });
  hipLaunchKernelGGL(k_reduce_final_multi, dim3(m), dim3(WG), 0, ctx->stream, nb, (const double *)ctx->mpartial, out);
  HIPCHECK(ctx, hipGetLastError());
  return ctx_allreduce(ctx, out, m, "defect norms");
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

// ---- block CG: one shared search space for m right-hand sides ---------------------------------------------------------------------------
// O'Leary's block CG with a pseudo-inverse in the m x m coupling (include/ddm_hip.h states the algorithm): unlike every other block
// driver of this file the columns are NOT independent -- each column's error is minimised over the span of all columns' Krylov
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
      if (hipGetLastError() != hipSuccess) rc = fail(ctx, DDM_EHIP, "kernel launch failed in %s", what);
      if (rc) break;
      for (int k = 0; k < nstore; ++k) release((int)tab[2 * k]);
    }
    rc = nstore > 0 && next < ncols ? refill() : multi_upload_mask(f);
  }
  if (!rc && hipGetLastError() != hipSuccess) rc = fail(ctx, DDM_EHIP, "kernel launch failed in %s", what);
  rc = multi_finish(f, prec, rc, t0); // (drains the stream; the elapsed time of the call lands in the slots' entries)
  for (int64_t j = 0; j < ncols; ++j) res[j].elapsed_s = sres[0].elapsed_s;
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
  auto launch_ok = [&]() { return hipGetLastError() == hipSuccess ? DDM_OK : fail(ctx, DDM_EHIP, "kernel launch failed in %s", what); };
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
  if (!rc && hipGetLastError() != hipSuccess) rc = fail(ctx, DDM_EHIP, "kernel launch failed in %s", what);
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
  if (!rc && hipGetLastError() != hipSuccess) rc = fail(ctx, DDM_EHIP, "kernel launch failed in %s", what);
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
  if (!rc && hipGetLastError() != hipSuccess) rc = fail(ctx, DDM_EHIP, "kernel launch failed in %s", what);
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
