// Value refresh of a device supernodal factor (SnDirect: local_factor.hpp; C ABI: ddm_ilu0_refresh, which hands F->sn factors to
// sn_refresh): the numeric factorisation again, on the structure the factor was created with.  Same pattern, same plans, new values;
// the result is bit for bit what ddm_direct_create makes of the new values.  Needs local_solver.hpp (sn_probe_refinement).
//
// Nothing sn::build made depends on the values, and sn::factorize takes the matrix as device CSR, zeroes the panels and leaves a
// result that does not depend on what the panels held (its updates run colour by colour: one order of summation).  So:
//   * KEPT: the sn::Factor with its supernodes, row lists, colours, top plan, chain plan, d_iperm / d_perm, all solve scratch
//     (d_contrib, d_partial, the top kernel's words), the factor's work vectors pd / px / pD and the status word.
//   * RECOMPUTED by sn::factorize: the panels (L; L U: also U^T), d_piv, the inverse triangles and external blocks of the chains
//     (chain_setup), from A->rp / A->ci / A->va of the matrix the factor was created on (F->A, not owned).  L U: tiny = sqrt(eps)
//     max |a_ij| from the new h_va.  No second panel array: the only extra memory is chain_setup's temporaries (one dense copy of
//     the chains' triangles, two for L U; ChainHost::wtot doubles each), freed before the call returns.
//   * DECIDED AGAIN: the refinement steps, by the probe of the creation (sn_probe_refinement, DDM_DIRECT_REFINE honoured), after
//     the refinement's copy of the matrix values (ref_va) has been brought up to date.  The step count may go either way; the
//     matrix copies and the residual block are allocated or released with it.
//   * DROPPED: both captured graphs (they hold kernel nodes for a fixed number of refinement steps and the residual block's address).
// The panels are overwritten in place, so a failure cannot leave the previous factor: the factor is marked invalid instead
// (SnDirect::invalid), and every solve entry returns DDM_ENUMERIC until a later refresh succeeds (sn_check_valid, local_solve.hpp).
// The return codes are those of a creation on the same values (sn_direct_create): DDM_ENUMERIC where it fails (Cholesky: not positive
// definite; the engine forced by DDM_DIRECT_ENGINE=device: a vanishing pivot column, a probe above 1e-9), DDM_ENOTIMPL where an
// unforced creation hands the matrix to the host engine (L U: a vanishing pivot column, a probe above 1e-9) -- the caller creates a
// new factor and arrives where a creation arrives.
// Synchronous, on the caller's thread and the context's stream, outside any stream capture.

static int sn_refresh(ddm_ctx *ctx, ddm_ilu0 *F)
{
  if (F->n == 0) return DDM_OK;
  SnDirect &R = *F->sn;
  sn::Factor &S = *R.f;
  const ddm_csr *A = F->A;
  if (!A || A->nrows != F->n) return fail(ctx, DDM_EINVAL, "ddm_ilu0_refresh: the factor does not know its matrix");
  DDMCHECK(csr_wait_upload(ctx, A));
  if (A->host_only) return fail(ctx, DDM_EINVAL, "the matrix was created without device arrays (ddm_csr_create_host)");
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream)); // (solves enqueued before the refresh read the panels and run the graphs dropped here)
  const char *eng = std::getenv("DDM_DIRECT_ENGINE");
  const bool force = eng && !std::strcmp(eng, "device"), lu = S.lu;
  // from here on the panels hold no factor until the end is reached
  R.invalid = true;
  F->graph.reset();
  F->mgraph.reset();
  const auto t0 = std::chrono::steady_clock::now();
  auto seconds_since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
  unsigned badsn = 0, perturbed = 0;
  double amax = 0.0;
  if (lu)
    for (double v : A->h_va) amax = std::max(amax, std::fabs(v));
  hipError_t he;
  {
    ScopedTimer t(ctx, "Refresh/sn factor");
    he = sn::factorize(S, ctx->stream, A->rp, A->ci, A->va, &badsn, 1.4901161193847656e-08 * amax, &perturbed);
  }
  if (he != hipSuccess) return fail(ctx, DDM_EHIP, "sparse direct solver (device): %s", hipGetErrorString(he));
  if (badsn) {
    if (lu && !force)
      return fail(ctx, DDM_ENOTIMPL, "ddm_ilu0_refresh: vanishing pivot column inside the diagonal block of supernode %u (the host engine takes such a matrix): create a new factor on the new values",
                  badsn - 1);
    return fail(ctx, DDM_ENUMERIC, lu ? "sparse direct solver: vanishing pivot column inside the diagonal block of supernode %u (matrix singular?)"
                                     : "sparse direct solver: matrix is not positive definite (supernode %u)", badsn - 1);
  }
  const double t_factor = seconds_since(t0);
  // the refinement: the matrix copy of the residuals first (the probe fills it only when it allocates it), then the probe of the
  // creation from a clean slate, so that a refreshed and a fresh factor decide alike
  if (R.ref_va) HIPCHECK(ctx, hipMemcpyAsync(R.ref_va, A->va, sizeof(double) * (size_t)A->nnz, hipMemcpyDeviceToDevice, ctx->stream));
  R.refine_steps = 0;
  std::fill(R.refine_omega, R.refine_omega + 5, 0.0);
  const auto t1 = std::chrono::steady_clock::now();
  double omega = 0.0;
  R.invalid = false; // (the probe solves through ilu0_solve_epilogue)
  int rc;
  {
    ScopedTimer t(ctx, "Refresh/sn probe");
    rc = sn_probe_refinement(ctx, F, A, &omega);
  }
  if (rc) {
    R.invalid = true;
    F->graph.reset();
    return rc;
  }
  if (R.refine_steps == 0) { // (also where DDM_DIRECT_REFINE=off kept the probe from running)
    (void)R.ref_rp.reset(), (void)R.ref_ci.reset(), (void)R.ref_va.reset(), (void)R.pr.reset();
    R.pr_cols = 0;
  }
  if (std::getenv("DDM_PIPE_VERBOSE"))
    std::fprintf(stderr, "[ddm] device supernodal %s refresh: numeric factorisation %.4f s (chain inverses %.4f s of it), probe %.4f s: %d refinement step(s) per solve, backward error of the probe %.2e -> %.2e%s\n",
                 lu ? "L U" : "Cholesky", t_factor, S.chain_setup_s, seconds_since(t1), R.refine_steps, R.refine_omega[0], omega, perturbed ? " (vanishing pivot columns replaced)" : "");
  if (!(omega <= 1e-9)) { // (as at creation: element growth beyond what pivoting inside the supernodes and three steps repair)
    R.invalid = true;
    F->graph.reset();
    if (!force)
      return fail(ctx, DDM_ENOTIMPL, "ddm_ilu0_refresh: backward error %.2e after iterative refinement (the host engine takes such a matrix): create a new factor on the new values", omega);
    return fail(ctx, DDM_ENUMERIC, "sparse direct solver (device): backward error %.2e after iterative refinement (the matrix needs pivoting across supernodes)", omega);
  }
  return DDM_OK;
}
