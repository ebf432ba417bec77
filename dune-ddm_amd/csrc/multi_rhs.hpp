// Several right-hand sides at once: the ddm_*_multi entry points of include/ddm_hip.h (included at the end of ddm_hip.hip, after the
// objects they work on).  Block vectors are row-major n x m (entry (i, c) at i * m + c), 1 <= m <= MULTI_MAX.  Every object keeps its
// own block scratch, allocated on first use for the widest m seen so far and reused afterwards; the single-vector buffers and paths are
// not touched.  ddm_cg_solve_multi runs m INDEPENDENT dune-istl CG recurrences (not a block-Krylov method): the matrix, the factor, the
// halo index lists and the coarse basis are read once per block iteration for all columns; the level engine of the local solve pays
// its per-level latency once for all of them.
#include "multi_kernels.hpp"

static int multi_check(ddm_ctx *ctx, int m, const char *what)
{
  if (m < 1 || m > MULTI_MAX) return fail(ctx, DDM_EINVAL, "%s: nrhs = %d outside [1, %d]", what, m, MULTI_MAX);
  return DDM_OK;
}
static int ctx_multi_scratch(ddm_ctx *ctx)
{
  if (ctx->mscal) return DDM_OK;
  HIPCHECK(ctx, ctx->mpartial.alloc((int64_t)RED_MAX_BLOCKS * MULTI_MAX));
  HIPCHECK(ctx, ctx->mactive.alloc(MULTI_MAX));
  HIPCHECK(ctx, ctx->mscal.alloc(8 * MULTI_MAX));
  return DDM_OK;
}

// ---- halo: m columns ---------------------------------------------------------------------------------------------------------------
// In-library exchange (RCCL) and a single rank: one message of m x count doubles per peer.  Callback exchange: the callback's buffers
// and counts are fixed at ddm_halo_create, so the block is exchanged column by column through the unchanged callback.
static int halo_exchange_multi(ddm_ctx *ctx, ddm_halo *H, int m, double *v)
{
  if (!H) return DDM_OK;
  if (H->nsend == 0 && H->ndst == 0 && !H->remote) return DDM_OK;
  HIPCHECK(ctx, reserve_cols<double>(H->mcols, m, {{H->msend, H->nsend}, {H->mrecv, H->nrecv}}));
  if (H->nsend > 0) hipLaunchKernelGGL(k_pack_multi, dim3(grid_for(H->nsend * m)), dim3(WG), 0, ctx->stream, H->nsend, m, H->send_idx, (const double *)v, H->msend);
  const double *rbuf = H->mrecv;
  if (ctx->rccl && (ctx->nranks > 1 || ctx->rccl_self)) {
    ctx->n_halo_groups += 1;
    if (H->self_count > 0 && !ctx->rccl_self)
      HIPCHECK(ctx, hipMemcpyAsync(H->mrecv + H->self_off_recv * m, H->msend + H->self_off_send * m, sizeof(double) * (size_t)(H->self_count * m),
                                   hipMemcpyDeviceToDevice, ctx->stream));
    NCCLCHECK(ctx, ctx->nccl.GroupStart());
    int64_t so = 0, ro = 0;
    for (int r = 0; r < ctx->nranks; ++r) {
      const bool self = r == ctx->rank;
      if ((!self || ctx->rccl_self) && H->recv_counts[r] > 0)
        NCCLCHECK(ctx, ctx->nccl.Recv(H->mrecv + ro * m, (size_t)(H->recv_counts[r] * m), ncclDouble, r, ctx->rccl_comm, ctx->stream));
      if ((!self || ctx->rccl_self) && H->send_counts[r] > 0)
        NCCLCHECK(ctx, ctx->nccl.Send(H->msend + so * m, (size_t)(H->send_counts[r] * m), ncclDouble, r, ctx->rccl_comm, ctx->stream));
      so += H->send_counts[r];
      ro += H->recv_counts[r];
    }
    NCCLCHECK(ctx, ctx->nccl.GroupEnd());
  } else if (ctx->nranks > 1) {
    if (!ctx->a2a) return fail(ctx, DDM_ECOMM, "multi-rank context without an exchange (ddm_ctx_set_rccl / ddm_ctx_set_comm)");
    for (int c = 0; c < m; ++c) {
      ctx->n_halo_groups += 1;
      if (H->nsend > 0)
        hipLaunchKernelGGL(k_column_copy<false>, dim3(grid_for(H->nsend)), dim3(WG), 0, ctx->stream, H->nsend, m, c, (const double *)H->msend, H->sendbuf);
      if (ctx->a2a(ctx->user, H->tag, H->sendbuf, H->recvbuf) != 0) return fail(ctx, DDM_ECOMM, "alltoall callback failed (tag %d, column %d)", H->tag, c);
      if (H->nrecv > 0)
        hipLaunchKernelGGL(k_column_copy<true>, dim3(grid_for(H->nrecv)), dim3(WG), 0, ctx->stream, H->nrecv, m, c, (const double *)H->recvbuf, H->mrecv);
    }
  } else {
    ctx->n_halo_groups += 1;
    rbuf = H->msend; // single rank: the self segment is the whole buffer
  }
  if (H->ndst > 0) {
    if (H->mode == 1)
      hipLaunchKernelGGL(k_unpack_multi<true>, dim3(grid_for(H->ndst * m)), dim3(WG), 0, ctx->stream, H->ndst, m, H->dst_idx, H->dst_ptr, H->src_pos, rbuf, v);
    else
      hipLaunchKernelGGL(k_unpack_multi<false>, dim3(grid_for(H->ndst * m)), dim3(WG), 0, ctx->stream, H->ndst, m, H->dst_idx, H->dst_ptr, H->src_pos, rbuf, v);
  }
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}

// ---- reductions: m owner-masked dots, one kernel per group of up to 8 columns, one all-reduce of m doubles ----------------------
template <class Launch>
static void for_column_groups(int m, Launch &&launch)
{
  for (int c0 = 0; c0 < m;) {
    const int cb = m - c0 >= 8 ? 8 : m - c0 >= 4 ? 4 : m - c0 >= 2 ? 2 : 1;
    launch(c0, cb);
    c0 += cb;
  }
}
#define DDM_MULTI_CB_DISPATCH(KERNEL, MASKED, cb, ...)                                                                 \
  do {                                                                                                                 \
    if (MASKED) {                                                                                                      \
      if (cb == 8) hipLaunchKernelGGL((KERNEL<8, true>), __VA_ARGS__);                                                 \
      else if (cb == 4) hipLaunchKernelGGL((KERNEL<4, true>), __VA_ARGS__);                                            \
      else if (cb == 2) hipLaunchKernelGGL((KERNEL<2, true>), __VA_ARGS__);                                            \
      else hipLaunchKernelGGL((KERNEL<1, true>), __VA_ARGS__);                                                         \
    } else {                                                                                                           \
      if (cb == 8) hipLaunchKernelGGL((KERNEL<8, false>), __VA_ARGS__);                                                \
      else if (cb == 4) hipLaunchKernelGGL((KERNEL<4, false>), __VA_ARGS__);                                           \
      else if (cb == 2) hipLaunchKernelGGL((KERNEL<2, false>), __VA_ARGS__);                                           \
      else hipLaunchKernelGGL((KERNEL<1, false>), __VA_ARGS__);                                                        \
    }                                                                                                                  \
  } while (0)

// out (m device doubles) = sum over ranks of sum_i [mask_i] x_ic y_ic; per column bit-identical to dot_device
static int dot_multi_device(ddm_ctx *ctx, int64_t n, const uint8_t *mask, int m, const double *X, const double *Y, double *out)
{
  DDMCHECK(ctx_multi_scratch(ctx));
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  double *partial = ctx->mpartial;
  for_column_groups(m, [&](int c0, int cb) {
    DDM_MULTI_CB_DISPATCH(k_dot_partial_multi, mask != nullptr, cb, dim3(nb), dim3(WG), 0, ctx->stream, n, m, c0, mask, X, Y, partial);
  });
  hipLaunchKernelGGL(k_reduce_final_multi, dim3(m), dim3(WG), 0, ctx->stream, nb, (const double *)partial, out);
  HIPCHECK(ctx, hipGetLastError());
  return ctx_allreduce(ctx, out, m, "scalar products");
}

// ---- NonOverlappingOperator ------------------------------------------------------------------------------------------------------
static int op_apply_multi(ddm_ctx *ctx, ddm_op *op, int m, const double *X, double *Y)
{
  ScopedTimer t(ctx, "Operator/apply");
  DDMCHECK(csr_mm_ld(ctx, op->A, m, X, m, Y, m)); // A->mv(x, y) for every column
  return halo_exchange_multi(ctx, op->halo, m, Y); // comm->addOwnerCopyToOwnerCopy(y, y)
}
static int op_applyscaleadd_multi(ddm_ctx *ctx, ddm_op *op, int m, double alpha, const double *X, double *Y)
{
  ScopedTimer t(ctx, "Operator/applyscaleadd");
  HIPCHECK(ctx, reserve_cols(op->mcols, m, op->mtmp, op->n));
  DDMCHECK(csr_mm_ld(ctx, op->A, m, X, m, op->mtmp, m));
  DDMCHECK(halo_exchange_multi(ctx, op->halo, m, op->mtmp));
  hipLaunchKernelGGL(k_axpy, dim3(grid_for(op->n * m)), dim3(WG), 0, ctx->stream, op->n * m, alpha, (const double *)op->mtmp, Y); // element-wise: y += alpha t
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_op_apply_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, const double *X, double *Y)
{
  if (!ctx || !op || !X || !Y || X == Y) return fail(ctx, DDM_EINVAL, "ddm_op_apply_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_op_apply_multi"));
  return op_apply_multi(ctx, op, nrhs, X, Y);
}
extern "C" int ddm_op_applyscaleadd_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, double alpha, const double *X, double *Y)
{
  if (!ctx || !op || !X || !Y || X == Y) return fail(ctx, DDM_EINVAL, "ddm_op_applyscaleadd_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_op_applyscaleadd_multi"));
  return op_applyscaleadd_multi(ctx, op, nrhs, alpha, X, Y);
}
extern "C" int ddm_dot_multi(ddm_ctx *ctx, ddm_op *op, int nrhs, const double *X, const double *Y, double *result_host)
{
  if (!ctx || !op || !X || !Y || !result_host) return fail(ctx, DDM_EINVAL, "ddm_dot_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_dot_multi"));
  DDMCHECK(ctx_multi_scratch(ctx));
  double *out = ctx->mscal + 6 * MULTI_MAX;
  DDMCHECK(dot_multi_device(ctx, op->n, op->owner, nrhs, X, Y, out));
  return ddm_memcpy_d2h(ctx, result_host, out, sizeof(double) * (size_t)nrhs);
}

// ---- SchwarzPreconditioner -----------------------------------------------------------------------------------------------------------
static int schwarz_multi_scratch(ddm_ctx *ctx, ddm_schwarz *S, int m)
{
  HIPCHECK(ctx, reserve_cols<double>(S->mcols, m, {{S->md_ovlp, S->n}, {S->mx_ovlp, S->n}}));
  return DDM_OK;
}
static int local_status_check(ddm_ctx *ctx, const ddm_schwarz *S)
{
  if (const unsigned e = S ? ilu0_peek_status(S->solver) : 0u) // fail fast: an earlier local solve gave up (no stream synchronisation here)
    return fail(ctx, DDM_ENUMERIC, "an earlier local triangular solve timed out waiting for a dependency (code %u): results since then are invalid", e);
  return DDM_OK;
}
// X (= or +=) R~^T [D] A_dir^-1 R~ D for m columns (schwarz.hh:115-149)
static int schwarz_apply_multi_impl(ddm_ctx *ctx, ddm_schwarz *S, int m, double *X, const double *D, bool acc)
{
  DDMCHECK(local_status_check(ctx, S));
  DDMCHECK(schwarz_multi_scratch(ctx, S, m));
  {
    ScopedTimer t(ctx, "Schwarz/get defect");
    hipLaunchKernelGGL(k_extend_multi, dim3(grid_for(S->n * m)), dim3(WG), 0, ctx->stream, S->n, m, S->ext_map, D, S->md_ovlp); // :121-122
    DDMCHECK(halo_exchange_multi(ctx, S->copy, m, S->md_ovlp));                                                                // :125
  }
  {
    ScopedTimer t(ctx, "Schwarz/local solve");
    DDMCHECK(ilu0_solve_multi_ld(ctx, S->solver, m, S->md_ovlp, m, S->mx_ovlp, m)); // :131-133 (level engine / direct multi-RHS solve)
  }
  {
    ScopedTimer t(ctx, "Schwarz/add solution");
    if (S->type == 1 && S->pou)
      hipLaunchKernelGGL(k_scale_add_multi, dim3(grid_for(S->n * m)), dim3(WG), 0, ctx->stream, S->n, m, (const double *)S->pou, (const double *)nullptr, S->mx_ovlp); // :139-141
    DDMCHECK(halo_exchange_multi(ctx, S->add, m, S->mx_ovlp)); // :138/:142
    if (acc) hipLaunchKernelGGL(k_restrict_multi<true>, dim3(grid_for(S->n * m)), dim3(WG), 0, ctx->stream, S->n, m, S->ext_map, (const double *)S->mx_ovlp, X);
    else hipLaunchKernelGGL(k_restrict_multi<false>, dim3(grid_for(S->n * m)), dim3(WG), 0, ctx->stream, S->n, m, S->ext_map, (const double *)S->mx_ovlp, X); // :146
    HIPCHECK(ctx, hipGetLastError());
  }
  return DDM_OK;
}
extern "C" int ddm_schwarz_apply_multi(ddm_ctx *ctx, ddm_schwarz *S, int nrhs, double *X, const double *D)
{
  if (!ctx || !S || !X || !D || X == D) return fail(ctx, DDM_EINVAL, "ddm_schwarz_apply_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_schwarz_apply_multi"));
  ScopedTimer t(ctx, "Schwarz/apply");
  return schwarz_apply_multi_impl(ctx, S, nrhs, X, D, false);
}

// ---- GalerkinPreconditioner ----------------------------------------------------------------------------------------------------------
static int galerkin_multi_scratch(ddm_ctx *ctx, ddm_galerkin *G, int m)
{
  HIPCHECK(ctx, reserve_cols<double>(G->mcols, m, {{G->mpartial, (int64_t)G->nchunk * G->kmax}, {G->md0, G->K}, {G->mx0, G->K}, {G->md_ovlp, G->n}, {G->mx_ovlp, G->n}}));
  return DDM_OK;
}
// restrict (one pass over the basis for all columns) -> one all-reduce of K x m doubles -> A0^-1 D0 -> prolong into G->mx_ovlp
static int coarse_chain_multi(ddm_ctx *ctx, ddm_galerkin *G, int m, const double *dov)
{
  ScopedTimer t(ctx, "GalerkinPrec/apply");
  hipLaunchKernelGGL(k_coarse_restrict_partial_multi, dim3(G->nchunk), dim3(WG), 0, ctx->stream, (int)G->kmax, G->ld, (const double *)G->basis, m, dov,
                     (const RowChunk *)G->chunks, G->mpartial, G->nchunk); // :165-167
  hipLaunchKernelGGL(k_coarse_restrict_final_multi, dim3(1), dim3(WG), 0, ctx->stream, (int)G->nsub, (int)G->kmax, m, (const int32_t *)G->sub_chunk_ptr,
                     (const double *)G->mpartial, (const int64_t *)G->coarse_index, G->K, G->md0);
  HIPCHECK(ctx, hipGetLastError());
  DDMCHECK(ctx_allreduce(ctx, G->md0, G->K * m, "coarse defect block")); // :170-171 (replicated coarse problem)
  if (G->K > 0)
    hipLaunchKernelGGL(k_dense_mm, dim3((unsigned)((G->K * m + WG - 1) / WG)), dim3(WG), 0, ctx->stream, G->K, m, (const double *)G->a0inv, (const double *)G->md0, G->mx0); // :174-179
  hipLaunchKernelGGL(k_coarse_prolong_multi, dim3(G->nchunk), dim3(WG), 0, ctx->stream, (int)G->kmax, G->ld, (const double *)G->basis, m, (const double *)G->mx0,
                     (const int64_t *)G->coarse_index, (const RowChunk *)G->chunks, G->mx_ovlp, G->nchunk); // :186-188
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
static int galerkin_apply_multi_impl(ddm_ctx *ctx, ddm_galerkin *G, int m, double *X, const double *D, bool acc, const double *dov_ready = nullptr)
{
  DDMCHECK(galerkin_multi_scratch(ctx, G, m));
  const double *dov = dov_ready;
  if (!dov) {
    hipLaunchKernelGGL(k_extend_multi, dim3(grid_for(G->n * m)), dim3(WG), 0, ctx->stream, G->n, m, G->ext_map, D, G->md_ovlp); // :159
    DDMCHECK(halo_exchange_multi(ctx, G->copy, m, G->md_ovlp));                                                                // :162
    dov = G->md_ovlp;
  }
  DDMCHECK(coarse_chain_multi(ctx, G, m, dov));
  DDMCHECK(halo_exchange_multi(ctx, G->add, m, G->mx_ovlp)); // :190
  if (acc) hipLaunchKernelGGL(k_restrict_multi<true>, dim3(grid_for(G->n * m)), dim3(WG), 0, ctx->stream, G->n, m, G->ext_map, (const double *)G->mx_ovlp, X);
  else hipLaunchKernelGGL(k_restrict_multi<false>, dim3(grid_for(G->n * m)), dim3(WG), 0, ctx->stream, G->n, m, G->ext_map, (const double *)G->mx_ovlp, X); // :193
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_galerkin_apply_multi(ddm_ctx *ctx, ddm_galerkin *G, int nrhs, double *X, const double *D)
{
  if (!ctx || !G || !X || !D || X == D) return fail(ctx, DDM_EINVAL, "ddm_galerkin_apply_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_galerkin_apply_multi"));
  return galerkin_apply_multi_impl(ctx, G, nrhs, X, D, false);
}

// ---- CombinedPreconditioner (combined_preconditioner.hh:127-163) --------------------------------------------------------------------
static int combined_apply_multi_impl(ddm_ctx *ctx, ddm_combined *C, int m, double *X, const double *D)
{
  ScopedTimer t(ctx, "CombinedPreconditioner/apply");
  ddm_schwarz *S = C->schwarz;
  ddm_galerkin *G = C->galerkin;
  DDMCHECK(local_status_check(ctx, S));
  if (C->mode == 0 && G && C->fused) {
    // the fused order of combined_apply_fused (one stream): extend + copy-halo -> coarse chain -> local solve -> (POU) + coarse ->
    // one halo add -> restrict
    DDMCHECK(schwarz_multi_scratch(ctx, S, m));
    DDMCHECK(galerkin_multi_scratch(ctx, G, m));
    {
      ScopedTimer t2(ctx, "Schwarz/get defect");
      hipLaunchKernelGGL(k_extend_multi, dim3(grid_for(S->n * m)), dim3(WG), 0, ctx->stream, S->n, m, S->ext_map, D, S->md_ovlp);
      DDMCHECK(halo_exchange_multi(ctx, S->copy, m, S->md_ovlp));
    }
    DDMCHECK(coarse_chain_multi(ctx, G, m, S->md_ovlp));
    {
      ScopedTimer t2(ctx, "Schwarz/local solve");
      DDMCHECK(ilu0_solve_multi_ld(ctx, S->solver, m, S->md_ovlp, m, S->mx_ovlp, m));
    }
    {
      ScopedTimer t2(ctx, "Schwarz/add solution");
      const double *pou = S->type == 1 ? S->pou : nullptr;
      hipLaunchKernelGGL(k_scale_add_multi, dim3(grid_for(S->n * m)), dim3(WG), 0, ctx->stream, S->n, m, pou, (const double *)G->mx_ovlp, S->mx_ovlp);
      DDMCHECK(halo_exchange_multi(ctx, S->add, m, S->mx_ovlp));
      hipLaunchKernelGGL(k_restrict_multi<false>, dim3(grid_for(S->n * m)), dim3(WG), 0, ctx->stream, S->n, m, S->ext_map, (const double *)S->mx_ovlp, X);
      HIPCHECK(ctx, hipGetLastError());
    }
    return DDM_OK;
  }
  DDMCHECK(schwarz_apply_multi_impl(ctx, S, m, X, D, false)); // x = 0; precs[0]->apply(x, d)  (:133-134)
  if (!G) return DDM_OK;
  if (C->mode == 0) { // additive (:136-142); the Schwarz level's extended defect is shared when both levels use the same interface
    const bool share = G->copy == S->copy && G->n == S->n && G->n_novlp == S->n_novlp;
    return galerkin_apply_multi_impl(ctx, G, m, X, D, true, share ? S->md_ovlp : nullptr);
  }
  // multiplicative: dnext = d - A x; x += P1 dnext (:149-158)
  HIPCHECK(ctx, reserve_cols(C->mcols, m, C->mdnext, C->n));
  HIPCHECK(ctx, hipMemcpyAsync(C->mdnext, D, sizeof(double) * (size_t)(C->n * m), hipMemcpyDeviceToDevice, ctx->stream));
  DDMCHECK(op_applyscaleadd_multi(ctx, C->op, m, -1.0, X, C->mdnext));
  return galerkin_apply_multi_impl(ctx, G, m, X, C->mdnext, true);
}
extern "C" int ddm_combined_apply_multi(ddm_ctx *ctx, ddm_combined *C, int nrhs, double *X, const double *D)
{
  if (!ctx || !C || !X || !D || X == D) return fail(ctx, DDM_EINVAL, "ddm_combined_apply_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_combined_apply_multi"));
  return combined_apply_multi_impl(ctx, C, nrhs, X, D);
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
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, first ? P : Q, B, scal + (first ? 0 : 3 * MULTI_MAX))); // rho = <q, b>
  if (!first) {
    hipLaunchKernelGGL(k_cg_beta_multi, dim3(1), dim3(64), 0, ctx->stream, m, (const int32_t *)ctx->mactive, scal); // beta = rho / rholast
    hipLaunchKernelGGL(k_cg_direction_multi, dim3(grid_for(n * m)), dim3(WG), 0, ctx->stream, n, m, (const int32_t *)ctx->mactive, (const double *)scal,
                       (const double *)Q, P); // p = beta p + q
  }
  DDMCHECK(op_apply_multi(ctx, op, m, P, Q));                                           // q = A p
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, P, Q, scal + MULTI_MAX));           // alpha = <p, q>
  hipLaunchKernelGGL(k_cg_lambda_multi, dim3(1), dim3(64), 0, ctx->stream, m, (const int32_t *)ctx->mactive, scal); // lambda = rholast / alpha
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  for_column_groups(m, [&](int c0, int cb) { // x += lambda p; b -= lambda q; <b, b> partials
    DDM_MULTI_CB_DISPATCH(k_cg_update_norm_multi, op->owner != nullptr, cb, dim3(nb), dim3(WG), 0, ctx->stream, n, m, c0, (const int32_t *)ctx->mactive,
                          (const double *)scal, (const uint8_t *)op->owner, (const double *)P, (const double *)Q, X, B, ctx->mpartial);
  });
  hipLaunchKernelGGL(k_reduce_final_multi, dim3(m), dim3(WG), 0, ctx->stream, nb, (const double *)ctx->mpartial, scal + 5 * MULTI_MAX);
  HIPCHECK(ctx, hipGetLastError());
  return ctx_allreduce(ctx, scal + 5 * MULTI_MAX, m, "defect norms");
}
extern "C" int ddm_cg_solve_multi(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int nrhs, double *X, double *B, double reduction, int maxit,
                                  double *hist_host, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !X || !B || !res || X == B || maxit < 0) return fail(ctx, DDM_EINVAL, "ddm_cg_solve_multi: bad arguments");
  DDMCHECK(multi_check(ctx, nrhs, "ddm_cg_solve_multi"));
  DDMCHECK(local_status_check(ctx, prec->schwarz));
  const int m = nrhs;
  const int64_t n = op->n;
  for (int c = 0; c < m; ++c) res[c] = ddm_solve_result{0, 0, 0.0, 1.0, 0.0};
  DDMCHECK(ctx_multi_scratch(ctx));
  HIPCHECK(ctx, reserve_cols<double>(prec->mcg_cols, m, {{prec->mp, n}, {prec->mq, n}})); // search directions p, q: block scratch of the preconditioner object
  double *P = prec->mp, *Q = prec->mq;
  double bb[MULTI_MAX], def0[MULTI_MAX], def[MULTI_MAX];
  int32_t active[MULTI_MAX];
  DDMCHECK(op_applyscaleadd_multi(ctx, op, m, -1.0, X, B)); // prec.pre(x, b); b -= A x
  DDMCHECK(dot_multi_device(ctx, n, op->owner, m, B, B, ctx->mscal + 5 * MULTI_MAX));
  DDMCHECK(ddm_memcpy_d2h(ctx, bb, ctx->mscal + 5 * MULTI_MAX, sizeof(double) * (size_t)m));
  int nactive = 0;
  for (int c = 0; c < m; ++c) {
    def0[c] = def[c] = std::sqrt(bb[c]);
    res[c].def0 = def0[c];
    if (hist_host) hist_host[c] = def0[c];
    if (!(def0[c] == def0[c])) return fail(ctx, DDM_ENUMERIC, "initial defect is NaN in column %d", c);
    active[c] = def0[c] < 1e-30 ? 0 : 1;
    if (!active[c]) res[c].converged = 1;
    nactive += active[c];
  }
  DDMCHECK(ddm_memcpy_h2d(ctx, ctx->mactive, active, sizeof(int32_t) * (size_t)m));
  (void)hipStreamSynchronize(ctx->stream);
  const auto t0 = std::chrono::steady_clock::now();
  int rc = DDM_OK;
  for (int i = 1; i <= maxit && nactive > 0 && !rc; ++i) {
    rc = cg_multi_step(ctx, op, prec, m, i == 1, X, B, P, Q);
    if (!rc) rc = ddm_memcpy_d2h(ctx, bb, ctx->mscal + 5 * MULTI_MAX, sizeof(double) * (size_t)m); // the defects are tested every iteration
    if (rc) break;
    bool changed = false;
    for (int c = 0; c < m; ++c) {
      if (!active[c]) continue;
      def[c] = std::sqrt(bb[c]);
      res[c].iterations = i;
      if (hist_host) hist_host[(int64_t)i * m + c] = def[c];
      if (!(def[c] == def[c])) {
        rc = fail(ctx, DDM_ENUMERIC, "defect is NaN in iteration %d (column %d)", i, c);
        break;
      }
      if (def[c] < def0[c] * reduction || def[c] < 1e-30) {
        res[c].converged = 1;
        active[c] = 0;
        nactive -= 1;
        changed = true;
      }
    }
    if (!rc && changed && nactive > 0) rc = ddm_memcpy_h2d(ctx, ctx->mactive, active, sizeof(int32_t) * (size_t)m);
  }
  (void)hipStreamSynchronize(ctx->stream);
  const double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  for (int c = 0; c < m; ++c) {
    res[c].elapsed_s = elapsed;
    if (def0[c] >= 1e-30) res[c].reduction = def[c] / def0[c];
  }
  if (!rc && prec->schwarz) {
    int st = 0;
    rc = ddm_ilu0_status(ctx, prec->schwarz->solver, &st);
    if (!rc && st) rc = fail(ctx, DDM_ENUMERIC, "persistent triangular solve timed out waiting for a level (results invalid)");
  }
  return rc;
}
// diagnostic: overwrite the status word of a local solver (0 clears it) -- lets a caller exercise the fail-fast path of the applies
extern "C" int ddm_ilu0_set_status(ddm_ilu0 *F, int status)
{
  if (!F || !F->err) return DDM_EINVAL;
  *(volatile unsigned *)F->err = (unsigned)status;
  return DDM_OK;
}
