// What the Krylov drivers (krylov_*.hpp) share: the stream drain, the frame around every loop (solve_result_reset,
// classify_initial_defect, krylov_finish) and around every block loop (MultiFrame), the launch check, the block defect pass and the
// memory check of the GMRES bases.  The drivers' device scalars are the slots SCAL_* and BICG_* of the context, the block drivers' work
// blocks come from prec->work (krylov_work.hpp).  Needs preconditioners.hpp.
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

// the launches enqueued since the last query: DDM_OK, or the error with the driver's name (what)
static int launch_check(ddm_ctx *ctx, const char *what)
{
  return hipGetLastError() == hipSuccess ? DDM_OK : fail(ctx, DDM_EHIP, "kernel launch failed in %s", what);
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
