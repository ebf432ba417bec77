// The objects a Krylov driver applies: the owner-masked dot products, NonOverlappingOperator (ddm_op), SchwarzPreconditioner
// (ddm_schwarz), GalerkinPreconditioner (ddm_galerkin, with ddm_galerkin_products) and CombinedPreconditioner (ddm_combined).  Each
// object's single-vector apply is followed by its apply to m columns (the ddm_*_multi entry points).  Block vectors are row-major
// n x m (entry (i, c) at i * m + c), 1 <= m <= MULTI_MAX; every object keeps its own block scratch, allocated on first use for the
// widest m seen so far.  The single-vector applies are NOT the block applies at m = 1: they use the fused epilogue of the pipe engine
// and the all-reduce a scalar can ride on (the rider argument of combined_apply_impl, down to coarse_allreduce); the headline number depends
// on them.  ddm_combined also holds the block drivers' work blocks (KrylovWork).  Needs halo.hpp, krylov_work.hpp and the local solver (local_factor.hpp .. local_solver.hpp).
#pragma once

// ---- reductions --------------------------------------------------------------------------------
// result (device scalar) = sum over ranks of sum_i [mask_i] x_i y_i
static int dot_device(ddm_ctx *ctx, int64_t n, const uint8_t *mask, const double *x, const double *y, double *result_dev)
{
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  if (mask)
    hipLaunchKernelGGL(k_dot_partial<true>, dim3(nb), dim3(WG), 0, ctx->stream, n, mask, x, y, ctx->partial);
  else
    hipLaunchKernelGGL(k_dot_partial<false>, dim3(nb), dim3(WG), 0, ctx->stream, n, mask, x, y, ctx->partial);
  hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(WG), 0, ctx->stream, nb, ctx->partial, result_dev);
  HIPCHECK(ctx, hipGetLastError());
  DDMCHECK(ctx_allreduce(ctx, result_dev, 1, "scalar product"));
  return DDM_OK;
}

// the same sum from ONE launch: the reduction finishes itself (k_dot_fin), bit-identical to dot_device
static int dot_device_fin(ddm_ctx *ctx, int64_t n, const uint8_t *mask, const double *x, const double *y, double *result_dev)
{
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  if (mask)
    hipLaunchKernelGGL(k_dot_fin<true>, dim3(nb), dim3(WG), 0, ctx->stream, n, mask, x, y, ctx->partial, ctx->ticket, result_dev);
  else
    hipLaunchKernelGGL(k_dot_fin<false>, dim3(nb), dim3(WG), 0, ctx->stream, n, mask, x, y, ctx->partial, ctx->ticket, result_dev);
  HIPCHECK(ctx, hipGetLastError());
  DDMCHECK(ctx_allreduce(ctx, result_dev, 1, "scalar product"));
  return DDM_OK;
}

// ... and for m columns: m owner-masked dots, one kernel per group of up to 8 columns, one all-reduce of m doubles
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

// ---- NonOverlappingOperator --------------------------------------------------------------------
struct ddm_op {
  const ddm_csr *A = nullptr;
  ddm_halo *halo = nullptr;
  dbuf<uint8_t> owner;
  int64_t n = 0;
  dbuf<double> tmp;
  dbuf<double> mtmp; // multi-RHS block (mcols columns)
  int mcols = 0;
  // A on diagonal row blocks (dia_build; k_spmv_dia), or nothing (dia_nblk == 0): then the products are ddm_csr_mv
  dbuf<DiaBlock> dia_blk;
  dbuf<int32_t> dia_tab;
  dbuf<uint32_t> dia_mask;
  dbuf<double> dia_val;    // the slabs of the segments that have an uncoded block
  dbuf<uint32_t> dia_code; // DIA_CODE_WORDS per row and the dictionaries of the coded blocks, or nothing
  dbuf<double> dia_dict;
  int dia_nblk = 0;
};
// y = A x: bit-identical to ddm_csr_mv in either layout
static int op_mv(ddm_ctx *ctx, const ddm_op *op, const double *x, double *y)
{
  if (!op->dia_nblk) return ddm_csr_mv(ctx, op->A, x, y);
  if (x == y) return fail(ctx, DDM_EINVAL, "operator product: x and y alias");
  const ddm_csr *A = op->A;
  hipLaunchKernelGGL(k_spmv_dia, dim3(op->dia_nblk), dim3(WG), 0, ctx->stream, (const DiaBlock *)op->dia_blk, op->dia_nblk, (const int32_t *)op->dia_tab,
                     (const uint32_t *)op->dia_mask, (const double *)op->dia_val, reinterpret_cast<const uint4 *>(op->dia_code.get()), (const double *)op->dia_dict, A->rp, A->ci, A->va, (int)op->n, x, y);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
// the diagonal-block storage of op->A's current values (replaces what the operator held); the CSR-stream product where none applies
static int op_build_dia(ddm_ctx *ctx, ddm_op *op)
{
  const ddm_csr *A = op->A;
  int rc = DDM_OK;
  op->dia_nblk = 0;
  (void)op->dia_blk.reset(), (void)op->dia_tab.reset(), (void)op->dia_mask.reset(), (void)op->dia_val.reset(), (void)op->dia_code.reset(), (void)op->dia_dict.reset();
  const char *fmt = std::getenv("DDM_SPMV_FORMAT"); // "csr": keep the CSR-stream product (A/B runs, tests)
  if (A->host_only || (fmt && !std::strcmp(fmt, "csr"))) return DDM_OK;
  DiaLayout L;
  dia_build(A->nrows, A->h_rp.data(), A->h_ci.data(), A->h_va.data(), L, dia_stage_x_from_env(), dia_code_from_env()); // DDM_SPMV_STAGE_X=0: no x windows in LDS, DDM_SPMV_CODE=0: no dictionaries
  if (!L.ndia) return DDM_OK;
  rc = upload(ctx, L.blk.data(), (int64_t)L.blk.size(), op->dia_blk);
  if (!rc) rc = upload(ctx, L.tab.data(), (int64_t)L.tab.size(), op->dia_tab);
  if (!rc) rc = upload(ctx, L.mask.data(), (int64_t)L.mask.size(), op->dia_mask);
  if (!rc) rc = upload(ctx, L.val.data(), (int64_t)L.val.size(), op->dia_val);
  if (!rc && L.ncoded) rc = upload(ctx, L.code.data(), (int64_t)L.code.size(), op->dia_code);
  if (!rc && L.ncoded) rc = upload(ctx, L.dict.data(), (int64_t)L.dict.size(), op->dia_dict);
  if (!rc) op->dia_nblk = (int)L.blk.size();
  return rc;
}
extern "C" int ddm_op_create(ddm_ctx *ctx, const ddm_csr *A, ddm_halo *novlp_add, const uint8_t *owner_mask_host, ddm_op **out)
{
  if (!ctx || !A || !out || !owner_mask_host) return fail(ctx, DDM_EINVAL, "ddm_op_create: bad arguments");
  if (A->nrows != A->ncols) return fail(ctx, DDM_EINVAL, "operator matrix must be square");
  if (novlp_add && novlp_add->mode != 1) return fail(ctx, DDM_EINVAL, "operator halo must be an 'add' halo");
  auto op = std::make_unique<ddm_op>();
  op->A = A;
  op->halo = novlp_add;
  op->n = A->nrows;
  int rc = upload(ctx, owner_mask_host, op->n, op->owner);
  if (!rc && op->tmp.alloc(op->n) != hipSuccess) rc = DDM_EHIP;
  if (!rc) rc = op_build_dia(ctx, op.get());
  if (rc) return fail(ctx, rc, "ddm_op_create: allocation failed");
  *out = op.release();
  return DDM_OK;
}
// The diagonal-block storage again, from the values A has now (ddm_csr_set_values).  Whether a block can be coded by a dictionary
// depends on its values, so the layout is built anew and the six arrays are replaced: what ddm_op_create builds on these values.
// The products are not captured in graphs, so nothing holds the old addresses.
extern "C" int ddm_op_refresh(ddm_ctx *ctx, ddm_op *op)
{
  if (!ctx || !op) return fail(ctx, DDM_EINVAL, "ddm_op_refresh: bad arguments");
  DDMCHECK(csr_wait_upload(ctx, op->A));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream)); // (products in flight read the arrays that go)
  if (const int rc = op_build_dia(ctx, op)) return fail(ctx, rc, "ddm_op_refresh: allocation failed");
  return DDM_OK;
}
extern "C" void ddm_op_destroy(ddm_op *op) { delete op; }
extern "C" int ddm_op_apply(ddm_ctx *ctx, ddm_op *op, const double *x, double *y)
{
  ScopedTimer t(ctx, "Operator/apply");
  DDMCHECK(op_mv(ctx, op, x, y));                   // A->mv(x, y)
  return ddm_halo_exchange(ctx, op->halo, y);       // comm->addOwnerCopyToOwnerCopy(y, y)
}
extern "C" int ddm_op_applyscaleadd(ddm_ctx *ctx, ddm_op *op, double alpha, const double *x, double *y)
{
  ScopedTimer t(ctx, "Operator/applyscaleadd");
  // y1 = y; y = 0; usmv; halo; y += y1   (only alpha*A*x is communicated, y is already consistent)
  DDMCHECK(op_mv(ctx, op, x, op->tmp));
  DDMCHECK(ddm_halo_exchange(ctx, op->halo, op->tmp));
  hipLaunchKernelGGL(k_axpy, dim3(grid_for(op->n)), dim3(WG), 0, ctx->stream, op->n, alpha, op->tmp, y);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_dot(ddm_ctx *ctx, ddm_op *op, const double *x, const double *y, double *result_host)
{
  DDMCHECK(dot_device(ctx, op->n, op->owner, x, y, ctx->scal + SCAL_DOT));
  return ddm_memcpy_d2h(ctx, result_host, ctx->scal + SCAL_DOT, sizeof(double));
}
extern "C" int ddm_norm(ddm_ctx *ctx, ddm_op *op, const double *x, double *result_host)
{
  DDMCHECK(ddm_dot(ctx, op, x, x, result_host));
  *result_host = std::sqrt(*result_host);
  return DDM_OK;
}
// ... and for m columns
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
  double *out = ctx->mscal + SCAL_DOT_MULTI * MULTI_MAX;
  DDMCHECK(dot_multi_device(ctx, op->n, op->owner, nrhs, X, Y, out));
  return ddm_memcpy_d2h(ctx, result_host, out, sizeof(double) * (size_t)nrhs);
}

// ---- SchwarzPreconditioner ---------------------------------------------------------------------
struct ddm_schwarz {
  int64_t n = 0, n_novlp = 0;
  int type = 1;
  ddm_ilu0 *solver = nullptr; // owned
  dbuf<int32_t> ext_map;
  dbuf<double> pou;
  dbuf<double> d_ovlp, x_ovlp;
  ddm_halo *copy = nullptr, *add = nullptr;
  dbuf<double> md_ovlp, mx_ovlp; // multi-RHS blocks (mcols columns)
  int mcols = 0;
  bool multi_f32 = false; // ddm_schwarz_set_multi_precision: single-precision sweeps in the block local solve
  // The single-vector apply's two exchanges as index tables (local_maps_build, halo.hpp), where both plans are rank-local and
  // DDM_FUSE_LOCAL is not "0"; otherwise (local == false) the apply runs k_extend, the exchanges and k_restrict.
  dbuf<int32_t> src_of, own_of, cp_ptr, cp_idx;
  bool local = false;
  ~ddm_schwarz() { ddm_ilu0_destroy(solver); }
};
extern "C" int ddm_schwarz_create(ddm_ctx *ctx, const ddm_csr *A_dir, int64_t nblocks, const int64_t *block_ptr, int64_t n_novlp,
                                  const int32_t *ext_map_host, const double *pou_host, int type, ddm_halo *ovlp_copy,
                                  ddm_halo *ovlp_add, ddm_schwarz **out)
{
  return ddm_schwarz_create_ex(ctx, A_dir, nblocks, block_ptr, n_novlp, ext_map_host, pou_host, type, "ilu0", ovlp_copy, ovlp_add, out);
}
// subdomain_solver: the `type` key of the [schwarz.subdomain_solver] sub-tree (schwarz.hh:85-92): "ilu0" (dune-istl's SeqILU,
// n = 0) or one of "cholmod" / "ldl" / "spqr"-less synonyms "direct", "cholesky" for the sparse direct solver of this library
// (SPD matrices; "umfpack" is accepted for symmetric positive definite input only).
extern "C" int ddm_schwarz_create_ex(ddm_ctx *ctx, const ddm_csr *A_dir, int64_t nblocks, const int64_t *block_ptr, int64_t n_novlp,
                                     const int32_t *ext_map_host, const double *pou_host, int type, const char *subdomain_solver,
                                     ddm_halo *ovlp_copy, ddm_halo *ovlp_add, ddm_schwarz **out)
{
  if (!ctx || !A_dir || !out || !ext_map_host) return fail(ctx, DDM_EINVAL, "ddm_schwarz_create: bad arguments");
  const std::string st = subdomain_solver ? subdomain_solver : "ilu0";
  const bool direct = st == "cholmod" || st == "direct" || st == "cholesky" || st == "umfpack" || st == "ldl";
  if (!direct && st != "ilu0" && st != "ilu") return fail(ctx, DDM_ENOTIMPL, "Unknown subdomain solver type '%s'", st.c_str()); // solver factory lookup (:85-92)
  bool general = st == "umfpack";
  if (st == "direct") { // pick the factorisation by looking at the values: symmetric -> Cholesky
    general = false;
    const int64_t nn = A_dir->nrows;
    for (int64_t i = 0; i < nn && !general; ++i)
      for (int64_t k = A_dir->h_rp[i]; k < A_dir->h_rp[i + 1] && !general; ++k) {
        const int64_t j = A_dir->h_ci[k];
        if (j <= i) continue;
        const auto b = A_dir->h_ci.begin() + A_dir->h_rp[j], e = A_dir->h_ci.begin() + A_dir->h_rp[j + 1];
        const auto it = std::lower_bound(b, e, (int32_t)i);
        const double vt = (it != e && *it == i) ? A_dir->h_va[(size_t)(it - A_dir->h_ci.begin())] : 0.0;
        if (std::fabs(vt - A_dir->h_va[k]) > 1e-12 * (std::fabs(vt) + std::fabs(A_dir->h_va[k]))) general = true;
      }
  }
  if (type != 0 && type != 1) return fail(ctx, DDM_ENOTIMPL, "Unknown Schwarz type %d", type); // schwarz.hh:83
  if (ovlp_copy && ovlp_copy->mode != 0) return fail(ctx, DDM_EINVAL, "ovlp_copy must be a 'copy' halo");
  if (ovlp_add && ovlp_add->mode != 1) return fail(ctx, DDM_EINVAL, "ovlp_add must be an 'add' halo");
  const int64_t n = A_dir->nrows;
  for (int64_t i = 0; i < n; ++i)
    if (ext_map_host[i] >= n_novlp) return fail(ctx, DDM_EINVAL, "ext_map entry out of range"); // size checks, schwarz.hh:186-193
  auto S = std::make_unique<ddm_schwarz>();
  S->n = n;
  S->n_novlp = n_novlp;
  S->type = type;
  S->copy = ovlp_copy;
  S->add = ovlp_add;
  DDMCHECK(direct ? ddm_direct_create(ctx, A_dir, nblocks, block_ptr, general ? 1 : 0, 0.0, &S->solver)
                  : ddm_ilu0_create(ctx, A_dir, nblocks, block_ptr, &S->solver)); // factorisation happens in the ctor (:92)
  DDMCHECK(upload(ctx, ext_map_host, n, S->ext_map));
  if (pou_host) DDMCHECK(upload(ctx, pou_host, n, S->pou));
  if (S->d_ovlp.alloc(n) != hipSuccess || S->x_ovlp.alloc(n) != hipSuccess) return fail(ctx, DDM_EHIP, "alloc");
  const char *fl = std::getenv("DDM_FUSE_LOCAL"); // "0": the general path also where the plans are rank-local (A/B runs, tests)
  if (!(fl && fl[0] == '0') && halo_is_local(ctx, ovlp_copy) && halo_is_local(ctx, ovlp_add)) {
    LocalMapsHost M;
    if (local_maps_build(n, n_novlp, ext_map_host, halo_plan_host(ovlp_copy), halo_plan_host(ovlp_add), M)) {
      DDMCHECK(upload(ctx, M.src_of.data(), (int64_t)M.src_of.size(), S->src_of));
      DDMCHECK(upload(ctx, M.own_of.data(), (int64_t)M.own_of.size(), S->own_of));
      DDMCHECK(upload(ctx, M.cp_ptr.data(), (int64_t)M.cp_ptr.size(), S->cp_ptr));
      DDMCHECK(upload(ctx, M.cp_idx.data(), (int64_t)M.cp_idx.size(), S->cp_idx));
      S->local = true;
    }
  }
  *out = S.release();
  return DDM_OK;
}
// the local solver again from A_dir's current values (ddm_ilu0_refresh: DDM_ENOTIMPL for direct local solvers and the box engine)
extern "C" int ddm_schwarz_refresh(ddm_ctx *ctx, ddm_schwarz *S)
{
  if (!ctx || !S) return fail(ctx, DDM_EINVAL, "ddm_schwarz_refresh: bad arguments");
  return ddm_ilu0_refresh(ctx, S->solver);
}
extern "C" void ddm_schwarz_destroy(ddm_schwarz *S) { delete S; }
extern "C" int64_t ddm_schwarz_num_levels(const ddm_schwarz *S, int upper) { return ddm_ilu0_num_levels(S->solver, upper); }
extern "C" int64_t ddm_schwarz_factor_nnz(const ddm_schwarz *S) { return (S && S->solver) ? S->solver->nnz : 0; } // stored entries of L + U (+ diagonal)
extern "C" int ddm_schwarz_engine(const ddm_schwarz *S) { return S ? ddm_ilu0_engine(S->solver) : -1; }
// Synchronous.  DDM_OK, or DDM_ENUMERIC when a single-launch local solve gave up waiting (its results are invalid: the
// GPU is shared with another process, or the grid was not co-resident) -- the reference's apply has no error return
// (schwarz.hh:131 discards the InverseOperatorResult), so the adaptors poll this in post() and the Krylov drivers at the end.
extern "C" ddm_ilu0 *ddm_schwarz_local_solver(ddm_schwarz *S) { return S ? S->solver : nullptr; } // borrowed (owned by S)
extern "C" int ddm_schwarz_status(ddm_ctx *ctx, const ddm_schwarz *S)
{
  if (!S) return fail(ctx, DDM_EINVAL, "ddm_schwarz_status: bad arguments");
  int st = 0;
  DDMCHECK(ddm_ilu0_status(ctx, S->solver, &st));
  if (st) return fail(ctx, DDM_ENUMERIC, "local triangular solve timed out waiting for a dependency (code %d): results are invalid", st);
  return DDM_OK;
}
// Every apply and every block driver starts with this (S may be null: nothing to check).
static int local_status_check(ddm_ctx *ctx, const ddm_schwarz *S)
{
  if (const unsigned e = S ? ilu0_peek_status(S->solver) : 0u) // fail fast: an earlier local solve gave up (no stream synchronisation here)
    return fail(ctx, DDM_ENUMERIC, "an earlier local triangular solve timed out waiting for a dependency (code %u): results since then are invalid", e);
  return DDM_OK;
}
// A caller's wish for sum_m [mask_m] z_m r_m of the vector z an apply is about to produce (CG's rho = <z, r>).  An apply whose last
// pass over z can form it on the way does so -- into out, summed over the ranks, the bits of dot_device(z, r) -- and sets done;
// otherwise it leaves the request alone and the caller takes the dot product itself.
struct ApplyDot {
  const uint8_t *mask;
  const double *r;
  double *out;
  bool done;
};
static bool schwarz_is_local(const ddm_ctx *ctx, const ddm_schwarz *S) { return S->local && halo_is_local(ctx, S->copy) && halo_is_local(ctx, S->add); }
// k_extend + the copy exchange (schwarz.hh:121-125), in one gather where the plans are rank-local
static int schwarz_get_defect(ddm_ctx *ctx, ddm_schwarz *S, const double *d)
{
  if (schwarz_is_local(ctx, S)) {
    hipLaunchKernelGGL(k_defect_gather, dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, (const int32_t *)S->src_of, d, S->d_ovlp);
    halo_count_local(ctx, S->copy);
    HIPCHECK(ctx, hipGetLastError());
    return DDM_OK;
  }
  hipLaunchKernelGGL(k_extend, dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, S->ext_map, d, S->d_ovlp); // :121-122
  return ddm_halo_exchange(ctx, S->copy, S->d_ovlp);                                                            // :125
}
// the add exchange + k_restrict<false, false> (schwarz.hh:138/:142, :146): x = the restriction of the summed S->x_ovlp.  Where the
// plans are rank-local one pass does both (the non-owner rows of S->x_ovlp are then NOT updated: nothing reads them before the next
// local solve overwrites them) and takes the dot product of a request on the way.
static int schwarz_sum_restrict(ddm_ctx *ctx, ddm_schwarz *S, double *x, ApplyDot *dot)
{
  if (!schwarz_is_local(ctx, S)) {
    DDMCHECK(ddm_halo_exchange(ctx, S->add, S->x_ovlp));
    hipLaunchKernelGGL((k_restrict<false, false>), dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, S->ext_map, S->x_ovlp, (const double *)nullptr, x);
    HIPCHECK(ctx, hipGetLastError());
    return DDM_OK;
  }
  const int64_t n = S->n_novlp;
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS); // (the grid of dot_device: the dot's partial sums are those of k_dot_partial)
  const int32_t *own = S->own_of, *cp = S->cp_ptr, *ci = S->cp_idx;
  const double *xov = S->x_ovlp;
  halo_count_local(ctx, S->add);
  if (!dot)
    hipLaunchKernelGGL((k_halo_sum_restrict<false, false>), dim3(nb), dim3(WG), 0, ctx->stream, n, own, cp, ci, xov, x, (const uint8_t *)nullptr, (const double *)nullptr,
                       (double *)nullptr, (unsigned *)nullptr, (double *)nullptr);
  else if (dot->mask)
    hipLaunchKernelGGL((k_halo_sum_restrict<true, true>), dim3(nb), dim3(WG), 0, ctx->stream, n, own, cp, ci, xov, x, dot->mask, dot->r, ctx->partial, ctx->ticket, dot->out);
  else
    hipLaunchKernelGGL((k_halo_sum_restrict<false, true>), dim3(nb), dim3(WG), 0, ctx->stream, n, own, cp, ci, xov, x, dot->mask, dot->r, ctx->partial, ctx->ticket, dot->out);
  HIPCHECK(ctx, hipGetLastError());
  if (dot) {
    DDMCHECK(ctx_allreduce(ctx, dot->out, 1, "scalar product"));
    dot->done = true;
  }
  return DDM_OK;
}
// x (= or +=) R~^T [D] A_dir^-1 R~ d; dot: a request the apply may serve (acc == false only), or null
static int schwarz_apply_impl(ddm_ctx *ctx, ddm_schwarz *S, double *x, const double *d, bool acc, ApplyDot *dot = nullptr)
{
  DDMCHECK(local_status_check(ctx, S));
  {
    ScopedTimer t(ctx, "Schwarz/get defect");
    DDMCHECK(schwarz_get_defect(ctx, S, d));
  }
  {
    ScopedTimer t(ctx, "Schwarz/local solve");
    DDMCHECK(ddm_ilu0_solve(ctx, S->solver, S->d_ovlp, S->x_ovlp)); // :131-133
  }
  {
    ScopedTimer t(ctx, "Schwarz/add solution");
    if (S->type == 1 && S->pou)
      hipLaunchKernelGGL(k_scale, dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, S->pou, S->x_ovlp); // :139-141
    if (!acc) return schwarz_sum_restrict(ctx, S, x, dot);                                                   // :138/:142, :146
    DDMCHECK(ddm_halo_exchange(ctx, S->add, S->x_ovlp));
    hipLaunchKernelGGL((k_restrict<true, false>), dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, S->ext_map, S->x_ovlp, (const double *)nullptr, x);
    HIPCHECK(ctx, hipGetLastError());
  }
  return DDM_OK;
}
extern "C" int ddm_schwarz_apply(ddm_ctx *ctx, ddm_schwarz *S, double *x, const double *d)
{
  ScopedTimer t(ctx, "Schwarz/apply");
  return schwarz_apply_impl(ctx, S, x, d, false);
}
// ... and for m columns
static int schwarz_multi_scratch(ddm_ctx *ctx, ddm_schwarz *S, int m)
{
  HIPCHECK(ctx, reserve_cols<double>(S->mcols, m, {{S->md_ovlp, S->n}, {S->mx_ovlp, S->n}}));
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
    DDMCHECK(ilu0_solve_multi_ld(ctx, S->solver, m, S->md_ovlp, m, S->mx_ovlp, m, S->multi_f32)); // :131-133 (level engine / direct multi-RHS solve)
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
// f32 != 0: the block applies (ddm_schwarz_apply_multi, and ddm_combined_apply_multi with it) run their local solve on the path of
// ddm_ilu0_solve_multi_f32, which falls back to the double sweeps under its own conditions; the single-vector apply is not affected
extern "C" int ddm_schwarz_set_multi_precision(ddm_schwarz *S, int f32)
{
  if (!S) return DDM_EINVAL;
  S->multi_f32 = f32 != 0;
  return DDM_OK;
}
// the engine of the local solver's block solves (ddm_ilu0_set_multi_engine); the single-vector apply is not affected
extern "C" int ddm_schwarz_set_multi_engine(ddm_schwarz *S, int mode)
{
  if (!S) return DDM_EINVAL;
  return ilu0_set_multi_mode(S->solver, mode);
}
// diagnostic: overwrite the status word of a local solver (0 clears it) -- lets a caller exercise the fail-fast path of the applies
extern "C" int ddm_ilu0_set_status(ddm_ilu0 *F, int status)
{
  if (!F || !F->err) return DDM_EINVAL;
  *(volatile unsigned *)F->err = (unsigned)status;
  return DDM_OK;
}

// ---- GalerkinPreconditioner --------------------------------------------------------------------
struct ddm_galerkin {
  int64_t n = 0, n_novlp = 0, nsub = 0, kmax = 0, K = 0, ld = 0;
  dbuf<int32_t> ext_map;
  dbuf<double> basis;       // kmax x ld
  dbuf<int64_t> coarse_index;
  dbuf<double> a0inv;
  dbuf<RowChunk> chunks;
  dbuf<int32_t> sub_chunk_ptr;
  int nchunk = 0;
  dbuf<double> partial, d0, x0;
  dbuf<double> d_ovlp, x_ovlp;
  ddm_halo *copy = nullptr, *add = nullptr;
  dbuf<double> mpartial, md0, mx0, md_ovlp, mx_ovlp; // multi-RHS blocks (mcols columns)
  int mcols = 0;
};
static constexpr int64_t COARSE_CHUNK_ROWS = 8192;

extern "C" int ddm_galerkin_create(ddm_ctx *ctx, int64_t n, int64_t n_novlp, const int32_t *ext_map_host, int64_t nsub,
                                   const int64_t *sub_ptr, int64_t kmax, const double *basis_host, const int64_t *coarse_index,
                                   int64_t K, const double *a0inv_host, ddm_halo *ovlp_copy, ddm_halo *ovlp_add,
                                   ddm_galerkin **out)
{
  if (!ctx || !out || !ext_map_host || !sub_ptr || !basis_host || !coarse_index || !a0inv_host)
    return fail(ctx, DDM_EINVAL, "ddm_galerkin_create: bad arguments");
  if (kmax < 1) return fail(ctx, DDM_EINVAL, "Must at least pass one template vector"); // galerkin_preconditioner.hh:129
  if (kmax > COARSE_KMAX) return fail(ctx, DDM_ENOTIMPL, "more than %d basis vectors per subdomain are not supported", COARSE_KMAX);
  if (sub_ptr[0] != 0 || sub_ptr[nsub] != n) return fail(ctx, DDM_EINVAL, "Template vectors must match size of matrix"); // :131
  for (int64_t t = 0; t < nsub * kmax; ++t)
    if (coarse_index[t] >= K) return fail(ctx, DDM_EINVAL, "coarse_index out of range");
  auto G = std::make_unique<ddm_galerkin>();
  G->n = n;
  G->n_novlp = n_novlp;
  G->nsub = nsub;
  G->kmax = kmax;
  G->K = K;
  G->ld = (n + 63) / 64 * 64;
  G->copy = ovlp_copy;
  G->add = ovlp_add;
  std::vector<RowChunk> chunks;
  std::vector<int32_t> scp(nsub + 1, 0);
  for (int64_t s = 0; s < nsub; ++s) {
    for (int64_t r = sub_ptr[s]; r < sub_ptr[s + 1]; r += COARSE_CHUNK_ROWS)
      chunks.push_back(RowChunk{r, std::min(r + COARSE_CHUNK_ROWS, sub_ptr[s + 1]), (int32_t)s, 0});
    scp[s + 1] = (int32_t)chunks.size();
  }
  G->nchunk = (int)chunks.size();
  DDMCHECK(upload(ctx, ext_map_host, n, G->ext_map));
  DDMCHECK(upload(ctx, coarse_index, nsub * kmax, G->coarse_index));
  DDMCHECK(upload(ctx, a0inv_host, K * K, G->a0inv));
  DDMCHECK(upload(ctx, chunks.data(), (int64_t)chunks.size(), G->chunks));
  DDMCHECK(upload(ctx, scp.data(), nsub + 1, G->sub_chunk_ptr));
  if (G->basis.alloc(kmax * G->ld) != hipSuccess || G->partial.alloc((int64_t)G->nchunk * kmax) != hipSuccess ||
      G->d0.alloc(K + 1) != hipSuccess || // (+ 1: a scalar may ride on the all-reduce, coarse_allreduce)
      G->x0.alloc(K) != hipSuccess || G->d_ovlp.alloc(n) != hipSuccess || G->x_ovlp.alloc(n) != hipSuccess)
    return fail(ctx, DDM_EHIP, "galerkin: allocation failed");
  if (hipMemset(G->basis, 0, sizeof(double) * (size_t)(kmax * G->ld)) != hipSuccess) return DDM_EHIP;
  if (hipMemcpy2D(G->basis, sizeof(double) * (size_t)G->ld, basis_host, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n,
                  (size_t)kmax, hipMemcpyHostToDevice) != hipSuccess)
    return fail(ctx, DDM_EHIP, "galerkin: basis upload failed");
  *out = G.release();
  return DDM_OK;
}
// a new inverse of the coarse matrix (K x K, row-major) into the buffer the applies read, on the context's stream; synchronous
extern "C" int ddm_galerkin_set_inverse(ddm_ctx *ctx, ddm_galerkin *G, const double *a0inv_host)
{
  if (!ctx || !G || !a0inv_host) return fail(ctx, DDM_EINVAL, "ddm_galerkin_set_inverse: bad arguments");
  return ddm_memcpy_h2d(ctx, G->a0inv, a0inv_host, (int64_t)sizeof(double) * G->K * G->K);
}
extern "C" void ddm_galerkin_destroy(ddm_galerkin *G) { delete G; }
// restrict -> all-reduce (rider rides along: coarse_allreduce) -> A0^-1 d0 -> prolong into G->x_ovlp, all enqueued on `stream`.
// spread_grid == 0: the full-grid passes over the basis, one workgroup per chunk; spread_grid > 0: the spread ones on that
// many one-wave workgroups (the chain runs beside the local solve).  Same result bit for bit either way.
// Not timed here: the callers' "GalerkinPrec/apply" scopes differ.
static int coarse_chain(ddm_ctx *ctx, ddm_galerkin *G, const double *dov, hipStream_t stream, double *rider, int spread_grid = 0)
{
  const unsigned sgrid = (unsigned)spread_grid;
  if (spread_grid > 0)
    hipLaunchKernelGGL(k_coarse_restrict_spread, dim3(sgrid), dim3(SPREAD_WG), 0, stream, (int)G->kmax, G->ld, G->basis, dov, G->chunks, G->partial, G->nchunk);
  else
    hipLaunchKernelGGL(k_coarse_restrict_partial, dim3(G->nchunk), dim3(WG), 0, stream, (int)G->kmax, G->ld, G->basis, dov, G->chunks, G->partial, G->nchunk); // :165-167
  hipLaunchKernelGGL(k_coarse_restrict_final, dim3(1), dim3(WG), 0, stream, (int)G->nsub, (int)G->kmax, G->sub_chunk_ptr, G->partial, G->coarse_index, G->K, G->d0);
  HIPCHECK(ctx, hipGetLastError());
  DDMCHECK(coarse_allreduce(ctx, G->d0, G->K, rider, stream)); // replaces MPI_Gatherv (:170-171): every rank obtains the full coarse defect
  hipLaunchKernelGGL(k_dense_mv, dim3((unsigned)((G->K + 3) / 4)), dim3(WG), 0, stream, G->K, G->a0inv, G->d0, G->x0); // :174-179 (replicated)
  if (spread_grid > 0)
    hipLaunchKernelGGL(k_coarse_prolong_spread, dim3(sgrid), dim3(SPREAD_WG), 0, stream, (int)G->kmax, G->ld, G->basis, G->x0, G->coarse_index, G->chunks, G->x_ovlp, G->nchunk);
  else
    hipLaunchKernelGGL(k_coarse_prolong, dim3(G->nchunk), dim3(WG), 0, stream, (int)G->kmax, G->ld, G->basis, G->x0, G->coarse_index, G->chunks, G->x_ovlp, G->nchunk); // :186-188
  return DDM_OK;
}
// d_ovlp_ready: the overlapping defect (extended + owner values copied to all holders) if the caller already has it -- in the
// additive combination both levels start from the same defect (schwarz.hh:121-125 and galerkin_preconditioner.hh:159-162)
static int galerkin_apply_impl(ddm_ctx *ctx, ddm_galerkin *G, double *x, const double *d, bool acc, double *rider, const double *d_ovlp_ready = nullptr)
{
  ScopedTimer t(ctx, "GalerkinPrec/apply");
  const double *dov = d_ovlp_ready;
  if (!dov) {
    hipLaunchKernelGGL(k_extend, dim3(grid_for(G->n)), dim3(WG), 0, ctx->stream, G->n, G->ext_map, d, G->d_ovlp); // :159
    DDMCHECK(ddm_halo_exchange(ctx, G->copy, G->d_ovlp));                                                         // :162
    dov = G->d_ovlp;
  }
  DDMCHECK(coarse_chain(ctx, G, dov, ctx->stream, rider));
  DDMCHECK(ddm_halo_exchange(ctx, G->add, G->x_ovlp)); // :190
  if (acc)
    hipLaunchKernelGGL((k_restrict<true, false>), dim3(grid_for(G->n)), dim3(WG), 0, ctx->stream, G->n, G->ext_map, G->x_ovlp, (const double *)nullptr, x);
  else
    hipLaunchKernelGGL((k_restrict<false, false>), dim3(grid_for(G->n)), dim3(WG), 0, ctx->stream, G->n, G->ext_map, G->x_ovlp, (const double *)nullptr, x); // :193
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_galerkin_apply(ddm_ctx *ctx, ddm_galerkin *G, double *x, const double *d)
{
  return galerkin_apply_impl(ctx, G, x, d, false, nullptr);
}
// Diagnostic (not part of the product path): the coarse chain alone on an overlapping defect the caller supplies (n doubles on the
// device), with the full-grid basis passes (spread_grid == 0) or the spread ones on spread_grid one-wave workgroups; copies the chunk
// partials (*npartial = chunks x kmax doubles), the coarse defect (K) and the prolonged correction (n) to the caller's device arrays.
// All three may be null to query *npartial.
extern "C" int ddm_galerkin_debug_chain(ddm_ctx *ctx, ddm_galerkin *G, const double *d_ovlp, int spread_grid, double *partial_out, double *d0_out,
                                        double *x_ovlp_out, int64_t *npartial)
{
  if (!ctx || !G || !npartial || spread_grid < 0) return fail(ctx, DDM_EINVAL, "ddm_galerkin_debug_chain: bad arguments");
  *npartial = (int64_t)G->nchunk * G->kmax;
  if (!partial_out && !d0_out && !x_ovlp_out) return DDM_OK;
  if (!d_ovlp || !partial_out || !d0_out || !x_ovlp_out) return fail(ctx, DDM_EINVAL, "ddm_galerkin_debug_chain: bad arguments");
  DDMCHECK(coarse_chain(ctx, G, d_ovlp, ctx->stream, nullptr, spread_grid));
  HIPCHECK(ctx, hipMemcpyAsync(partial_out, G->partial, sizeof(double) * (size_t)*npartial, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHECK(ctx, hipMemcpyAsync(d0_out, G->d0, sizeof(double) * (size_t)G->K, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHECK(ctx, hipMemcpyAsync(x_ovlp_out, G->x_ovlp, sizeof(double) * (size_t)G->n, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DDM_OK;
}
// ... and for m columns
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

extern "C" int ddm_galerkin_products(ddm_ctx *ctx, const ddm_csr *A_dir, int64_t nleft, const double *left, int64_t nright,
                                     const double *right, int64_t row0, int64_t row1, double *out_host)
{
  // out[j*nleft + i] = <left_i, A_dir right_j> over rows [row0,row1)   (column-major nleft x nright,
  // the slab layout of galerkin_preconditioner.hh:294 / helpers.hh:252)
  if (!A_dir || !left || !right || !out_host || nleft < 1 || nleft > COARSE_KMAX || nright < 1 || row0 < 0 || row1 > A_dir->nrows || row0 > row1)
    return fail(ctx, DDM_EINVAL, "ddm_galerkin_products: bad arguments");
  if (A_dir->host_only) return fail(ctx, DDM_EINVAL, "the matrix was created without device arrays (ddm_csr_create_host)");
  const int64_t n = A_dir->nrows;
  dbuf<double> y, partial, outd;
  dbuf<RowChunk> chunks;
  std::vector<RowChunk> hc;
  for (int64_t r = row0; r < row1; r += COARSE_CHUNK_ROWS) hc.push_back(RowChunk{r, std::min(r + COARSE_CHUNK_ROWS, row1), 0, 0});
  const int nchunk = (int)hc.size();
  HIPCHECK(ctx, y.alloc(n));
  HIPCHECK(ctx, partial.alloc((int64_t)nchunk * nleft));
  HIPCHECK(ctx, outd.alloc(nleft * nright));
  int rc = upload(ctx, hc.data(), (int64_t)hc.size(), chunks);
  std::vector<int32_t> scp = {0, nchunk};
  std::vector<int64_t> cidx(nleft);
  dbuf<int32_t> d_scp;
  dbuf<int64_t> d_cidx;
  if (!rc) rc = upload(ctx, scp.data(), 2, d_scp);
  for (int64_t j = 0; j < nright && !rc; ++j) {
    // y[row0:row1) = (A_dir right_j)[row0:row1): only the rows the products below read (a whole-matrix product per vector and call
    // was 1 s of the headline setup: 1 280 passes over 3.5 GB); same row sums in the same order as ddm_csr_mv
    if (row1 > row0)
      hipLaunchKernelGGL(k_spmm_rowmajor, dim3((unsigned)((row1 - row0 + WG - 1) / WG)), dim3(WG), 0, ctx->stream, row1 - row0, 1, A_dir->rp + row0, A_dir->ci, A_dir->va,
                         right + j * n, (int64_t)1, y + row0, (int64_t)1);
    if (hipGetLastError() != hipSuccess) rc = fail(ctx, DDM_EHIP, "ddm_galerkin_products: kernel launch failed");
    for (int64_t i = 0; i < nleft; ++i) cidx[i] = i;
    if (!d_cidx) rc = upload(ctx, cidx.data(), nleft, d_cidx);
    if (rc) break;
    if (nchunk > 0)
      hipLaunchKernelGGL(k_coarse_restrict_partial, dim3(nchunk), dim3(WG), 0, ctx->stream, (int)nleft, n, left, y, chunks, partial, nchunk);
    hipLaunchKernelGGL(k_coarse_restrict_final, dim3(1), dim3(WG), 0, ctx->stream, 1, (int)nleft, d_scp, partial, d_cidx, nleft, outd + j * nleft);
  }
  if (!rc) rc = ddm_memcpy_d2h(ctx, out_host, outd, sizeof(double) * (size_t)(nleft * nright));
  return rc;
}

// ---- CombinedPreconditioner --------------------------------------------------------------------
// the coarse chain beside the local solve (combined_apply_fused): whether it is on where DDM_OVERLAP_COARSE is unset, and its width
constexpr bool OVERLAP_DEFAULT = true;
// One-wave workgroups of the side stream's basis passes: OVERLAP_WAVES_PER_16_CU per 16 CUs at up to OVERLAP_KMAX_MEASURED basis
// vectors per subdomain, in proportion to the vector count beyond that, never more than one per CU (overlap_default_grid).
// The width is tuned at ONE shape (216^3, 27-point rows, 20 vectors: DESIGN.md section 4, measured at 5, 6, 7, 8, 16 and 32 per 16
// CUs) and the optimum has a steep side: the narrower the chain, the less it slows the solve beside it, but a chain that outlasts
// the solve is paid in full (5 per 16 CUs: 4.84 instead of 4.28 ms per iteration).  7 per 16 CUs leaves the chain 0.4 ms of a
// 3.5 ms solve.  The chain's time grows with vectors x rows, hence the scaling; a local solve that is much cheaper per row than
// ILU(0) of a 27-point matrix is not covered by it and wants DDM_OVERLAP_GRID.
constexpr int OVERLAP_WAVES_PER_16_CU = 7, OVERLAP_KMAX_MEASURED = 20;
static int overlap_default_grid(int num_cu, int64_t kmax)
{
  const int64_t k = std::max<int64_t>(kmax, OVERLAP_KMAX_MEASURED);
  const int64_t g = (OVERLAP_WAVES_PER_16_CU * num_cu * k + 16 * OVERLAP_KMAX_MEASURED - 1) / (16 * OVERLAP_KMAX_MEASURED);
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, num_cu));
}
struct ddm_combined {
  int mode = 0;
  ddm_op *op = nullptr;
  ddm_schwarz *schwarz = nullptr;
  ddm_galerkin *galerkin = nullptr;
  dbuf<double> dnext;
  int64_t n = 0;
  bool fused = false;   // additive mode: the levels' overlapping results are summed before ONE halo add (combined_apply_fused)
  int overlap = 0;      // ... and the coarse chain runs on a side stream beside the local solve: 0 never, 1 always, 2 where the local engine is pipe
  int side_grid = 0;    // one-wave workgroups of the chain's two basis passes on the side stream
  dbuf<double> mdnext; // multi-RHS block: multiplicative defect (mcols columns)
  int mcols = 0;
  KrylovWork work;     // the block drivers' work blocks, kept between calls (krylov_work.hpp): not preconditioner state
};
extern "C" int ddm_combined_create(ddm_ctx *ctx, int mode, ddm_op *op, ddm_schwarz *schwarz, ddm_galerkin *galerkin, ddm_combined **out)
{
  if (!ctx || !out || !schwarz) return fail(ctx, DDM_EINVAL, "ERROR: No preconditioners added yet"); // combined_preconditioner.hh:77
  if (mode != 0 && mode != 1) return fail(ctx, DDM_ENOTIMPL, "Unknown apply mode in CombinedPreconditioner, use either additive or multiplicative"); // :68
  if (mode == 1 && galerkin && !op) return fail(ctx, DDM_EINVAL, "ERROR: ApplyMode is multiplicative but operator A is not provided. Set with `set_op`"); // :146
  auto C = std::make_unique<ddm_combined>();
  C->mode = mode;
  C->op = op;
  C->schwarz = schwarz;
  C->galerkin = galerkin;
  C->n = schwarz->n_novlp;
  if (mode == 0 && galerkin) {
    const char *f = std::getenv("DDM_FUSE_LEVELS");    // "0": the two levels one after the other (two halo adds: the reference's order of sums)
    const char *e = std::getenv("DDM_OVERLAP_COARSE"); // "1" / "0": coarse chain on a side stream / not; unset: OVERLAP_DEFAULT, pipe engine only
    const char *g = std::getenv("DDM_OVERLAP_GRID");   // workgroups of the side stream's basis passes (default: overlap_default_grid)
    C->fused = !(f && f[0] == '0') && galerkin->copy == schwarz->copy && galerkin->add == schwarz->add && galerkin->n == schwarz->n && galerkin->n_novlp == schwarz->n_novlp;
    if (C->fused && (ctx->nranks == 1 || ctx->rccl)) C->overlap = e ? (e[0] == '1' ? 1 : 0) : (OVERLAP_DEFAULT ? 2 : 0);
    C->side_grid = g ? std::max(1, std::atoi(g)) : overlap_default_grid(ctx->num_cu, galerkin->kmax);
  }
  if (C->dnext.alloc(C->n) != hipSuccess) return fail(ctx, DDM_EHIP, "combined: allocation failed");
  *out = C.release();
  return DDM_OK;
}
extern "C" int ddm_combined_status(ddm_ctx *ctx, const ddm_combined *C)
{
  if (!C) return fail(ctx, DDM_EINVAL, "ddm_combined_status: bad arguments");
  return C->schwarz ? ddm_schwarz_status(ctx, C->schwarz) : DDM_OK;
}
extern "C" void ddm_combined_destroy(ddm_combined *C) { delete C; }
// Additive combination, fused: both levels start from the same extended defect and add over the same interface, so their
// overlapping results are summed BEFORE the exchange (linearity of addOwnerCopyToAll; schwarz.hh:138-146 +
// galerkin_preconditioner.hh:190-193 + combined_preconditioner.hh:136-142) -- one extend, one copy-halo, one halo add and one restrict
// instead of two each; the result differs from the two-pass order by rounding only (measured: 5.54 -> 5.31 ms per iteration at 216^3).
//   extend + copy-halo -> local solve -> (POU scale) -> R d -> all-reduce -> A0^-1 -> R^T x0 -> x_s += x_c -> halo add -> restrict
// two_streams (C->overlap; needs the in-library exchange or a single rank): the coarse chain runs on a low-priority side stream BESIDE
// the local solve, which is latency-bound and leaves most of the HBM bandwidth idle.  The chain's two passes over the basis are the
// spread kernels (one-wave workgroups, C->side_grid of them, fewer than CUs by default: a wave is small enough for the solve's
// workgroups to stay resident next to it, and the chain is kept as narrow as still ends inside the solve).  With the pipe engine the chain joins between the solve kernel and its output permutation,
// which applies "x *= pou; x += x_coarse" as on one stream: the same kernels' sums in the same order, the result is bit-identical.
// The other engines join behind the solve with k_scale + k_axpy (the same operations as separate passes).
// Measurements, the losing configurations included: DESIGN.md section 4.
static int combined_apply_fused(ddm_ctx *ctx, ddm_combined *C, double *x, const double *d, double *rider, ApplyDot *dot)
{
  ddm_schwarz *S = C->schwarz;
  ddm_galerkin *G = C->galerkin;
  bool pipe_engine = false;
  if (C->overlap != 0) DDMCHECK(ilu0_is_pipe(ctx, S->solver, &pipe_engine));
  const bool two_streams = C->overlap == 1 || (C->overlap == 2 && pipe_engine);
  if (two_streams) DDMCHECK(ctx_side_stream(ctx));
  {
    ScopedTimer t(ctx, "Schwarz/get defect");
    DDMCHECK(schwarz_get_defect(ctx, S, d));
  }
  // The coarse chain (kernels, RCCL all-reduce, timer) goes to the side stream, or runs first on the one stream, so that the local
  // solve's last kernel can also apply "x *= pou; x += x_coarse".
  // inter-rank operations stay totally ordered: copy-halo (main) -> all-reduce (side) -> [join] -> halo add (main)
  const hipStream_t chain = two_streams ? ctx->side : ctx->stream;
  if (two_streams) {
    HIPCHECK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    HIPCHECK(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
  }
  {
    ScopedTimer t(ctx, "GalerkinPrec/apply", chain);
    DDMCHECK(coarse_chain(ctx, G, S->d_ovlp, chain, rider, two_streams ? C->side_grid : 0));
  }
  if (two_streams) HIPCHECK(ctx, hipEventRecord(ctx->ev_join, ctx->side));
  const double *pou = S->type == 1 ? S->pou : nullptr;
  const bool fold = !two_streams || pipe_engine; // the solve's output pass applies the POU scale and adds the coarse correction
  {
    ScopedTimer t(ctx, "Schwarz/local solve");
    DDMCHECK(ilu0_solve_epilogue(ctx, S->solver, S->d_ovlp, S->x_ovlp, fold ? pou : nullptr, fold ? (const double *)G->x_ovlp : nullptr,
                                 two_streams && fold ? ctx->ev_join : nullptr));
  }
  {
    ScopedTimer t(ctx, "Schwarz/add solution");
    if (!fold) {
      if (pou) hipLaunchKernelGGL(k_scale, dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, pou, S->x_ovlp);
      HIPCHECK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
      hipLaunchKernelGGL(k_axpy, dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, 1.0, (const double *)G->x_ovlp, S->x_ovlp);
    }
    DDMCHECK(schwarz_sum_restrict(ctx, S, x, dot));
  }
  return DDM_OK;
}

// rider: a device scalar to be summed over the ranks, or null.  Wherever C has a Galerkin level, exactly ONE coarse_allreduce of the
// apply receives it -- fused, additive unfused and multiplicative alike -- so a caller that passes one need not reduce it itself
// (ddm_cg_steps: the squared defect norm of the previous iteration); without a Galerkin level it is ignored.
// dot: a request for <x, r> (ApplyDot) or null; served where the Schwarz level's restriction is the apply's last pass over x (the
// fused additive combination, no Galerkin level) and its plans are rank-local.
static int combined_apply_impl(ddm_ctx *ctx, ddm_combined *C, double *x, const double *d, double *rider, ApplyDot *dot = nullptr)
{
  ScopedTimer t(ctx, "CombinedPreconditioner/apply");
  DDMCHECK(local_status_check(ctx, C->schwarz));
  if (C->mode == 0 && C->galerkin && C->fused) return combined_apply_fused(ctx, C, x, d, rider, dot);
  // x = 0; precs[0]->apply(x, d)  (:133-134)  -- the restrict kernel overwrites every entry of x
  DDMCHECK(schwarz_apply_impl(ctx, C->schwarz, x, d, false, C->galerkin ? nullptr : dot));
  if (!C->galerkin) return DDM_OK;
  if (C->mode == 0) { // additive: xnext = P1 d; x += xnext (:136-142) -- fused into the restrict of the coarse level
    // both levels extend the same defect over the same interface: the Schwarz level's copy is reused (the local solves read it only)
    static const bool no_share = std::getenv("DDM_NO_SHARED_DEFECT") != nullptr; // diagnostic switch
    const bool share = !no_share && C->galerkin->copy == C->schwarz->copy && C->galerkin->n == C->schwarz->n && C->galerkin->n_novlp == C->schwarz->n_novlp;
    return galerkin_apply_impl(ctx, C->galerkin, x, d, true, rider, share ? C->schwarz->d_ovlp : nullptr);
  }
  // multiplicative: dnext = d - A x; x += P1 dnext (:149-158)
  HIPCHECK(ctx, hipMemcpyAsync(C->dnext, d, sizeof(double) * (size_t)C->n, hipMemcpyDeviceToDevice, ctx->stream));
  DDMCHECK(ddm_op_applyscaleadd(ctx, C->op, -1.0, x, C->dnext));
  return galerkin_apply_impl(ctx, C->galerkin, x, C->dnext, true, rider);
}
extern "C" int ddm_combined_apply(ddm_ctx *ctx, ddm_combined *C, double *x, const double *d) { return combined_apply_impl(ctx, C, x, d, nullptr); }
// ... and for m columns (combined_preconditioner.hh:127-163)
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
      DDMCHECK(ilu0_solve_multi_ld(ctx, S->solver, m, S->md_ovlp, m, S->mx_ovlp, m, S->multi_f32));
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

// ---- diagnostics of the rank-local passes and the self-finishing reductions (not part of the product path) ------------------------
// Whether S applies through the rank-local tables, and its two overlapping work vectors (n doubles each; either may be null).
extern "C" int ddm_schwarz_debug_local(ddm_ctx *ctx, ddm_schwarz *S, int *local, double **d_ovlp, double **x_ovlp)
{
  if (!ctx || !S || !local) return fail(ctx, DDM_EINVAL, "ddm_schwarz_debug_local: bad arguments");
  *local = schwarz_is_local(ctx, S) ? 1 : 0;
  if (d_ovlp) *d_ovlp = S->d_ovlp;
  if (x_ovlp) *x_ovlp = S->x_ovlp;
  return DDM_OK;
}
extern "C" double *ddm_ctx_scalars(ddm_ctx *ctx) { return ctx ? ctx->scal.get() : nullptr; } // the SCAL_SLOTS device scalars
// The second half of a Schwarz apply on an overlapping vector the caller supplies (n device doubles, copied into S's work vector):
// z = restriction of its sum over the copies, out[0] = <z, r> with the owner mask (null: none).  general != 0: the add exchange,
// k_restrict and dot_device, whatever S would take; general == 0: what S takes (the one pass where its plans are rank-local).
extern "C" int ddm_schwarz_debug_sum_restrict(ddm_ctx *ctx, ddm_schwarz *S, const double *x_ovlp, int general, const uint8_t *mask, const double *r, double *z, double *out)
{
  if (!ctx || !S || !x_ovlp || !r || !z || !out) return fail(ctx, DDM_EINVAL, "ddm_schwarz_debug_sum_restrict: bad arguments");
  HIPCHECK(ctx, hipMemcpyAsync(S->x_ovlp, x_ovlp, sizeof(double) * (size_t)S->n, hipMemcpyDeviceToDevice, ctx->stream));
  ApplyDot dot{mask, r, out, false};
  if (general) {
    const bool keep = S->local;
    S->local = false;
    const int rc = schwarz_sum_restrict(ctx, S, z, &dot);
    S->local = keep;
    DDMCHECK(rc);
  } else
    DDMCHECK(schwarz_sum_restrict(ctx, S, z, &dot));
  if (!dot.done) DDMCHECK(dot_device(ctx, S->n_novlp, mask, z, r, out));
  return DDM_OK;
}
// One reduction of the CG loop on n rows, enqueued without synchronising; fin != 0: the self-finishing kernel, fin == 0: the kernels
// it stands in for.  mask: n bytes or null.  out: device doubles.
//   kind 0  out[0] = <a, b>                                    k_dot_fin                | k_dot_partial + k_reduce_final
//   kind 1  a += lambda c, b -= lambda d, lambda = rho / pq;    k_cg_update_norm_fin     | [k_cg_beta +] k_cg_lambda + k_cg_update_norm + k_reduce_final
//           out[0 .. 2] = <b, b>, lambda, rholast.  The caller has put pq into SCAL_PQ and rho into SCAL_RHOLAST (first != 0: the
//           first iteration) or into SCAL_RHO with the last rho in SCAL_RHOLAST (first == 0) of ddm_ctx_scalars.
//   kind 2  a = rows of c summed by the tables (own_of, cp_ptr, cp_idx over n rows), out[0] = <a, b>
//                                                               k_halo_sum_restrict<., true> | the same kernel without the dot + the kind 0 pair
extern "C" int ddm_debug_reduction(ddm_ctx *ctx, int kind, int fin, int64_t n, const uint8_t *mask, double *a, double *b, const double *c, const double *d,
                                   int first, const int32_t *own_of, const int32_t *cp_ptr, const int32_t *cp_idx, double *out)
{
  if (!ctx || n < 1 || !a || !b || !out || kind < 0 || kind > 2) return fail(ctx, DDM_EINVAL, "ddm_debug_reduction: bad arguments");
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  double *scal = ctx->scal;
  if (kind == 0) return fin ? dot_device_fin(ctx, n, mask, a, b, out) : dot_device(ctx, n, mask, a, b, out);
  if (kind == 1) {
    if (!c || !d) return fail(ctx, DDM_EINVAL, "ddm_debug_reduction: bad arguments");
    if (fin) {
      const int num = first ? SCAL_RHOLAST : SCAL_RHO;
      if (mask) hipLaunchKernelGGL(k_cg_update_norm_fin<true>, dim3(nb), dim3(WG), 0, ctx->stream, n, scal, num, mask, c, d, a, b, ctx->partial, ctx->ticket, scal + SCAL_DEF2);
      else hipLaunchKernelGGL(k_cg_update_norm_fin<false>, dim3(nb), dim3(WG), 0, ctx->stream, n, scal, num, mask, c, d, a, b, ctx->partial, ctx->ticket, scal + SCAL_DEF2);
    } else {
      if (!first) hipLaunchKernelGGL(k_cg_beta, dim3(1), dim3(1), 0, ctx->stream, scal);
      hipLaunchKernelGGL(k_cg_lambda, dim3(1), dim3(1), 0, ctx->stream, scal);
      if (mask) hipLaunchKernelGGL(k_cg_update_norm<true>, dim3(nb), dim3(WG), 0, ctx->stream, n, (const double *)scal, mask, c, d, a, b, ctx->partial);
      else hipLaunchKernelGGL(k_cg_update_norm<false>, dim3(nb), dim3(WG), 0, ctx->stream, n, (const double *)scal, mask, c, d, a, b, ctx->partial);
      hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(WG), 0, ctx->stream, nb, ctx->partial, scal + SCAL_DEF2);
    }
    hipLaunchKernelGGL(k_copy_scalar, dim3(1), dim3(1), 0, ctx->stream, (const double *)(scal + SCAL_DEF2), out);
    hipLaunchKernelGGL(k_copy_scalar, dim3(1), dim3(1), 0, ctx->stream, (const double *)(scal + SCAL_STEP), out + 1);
    hipLaunchKernelGGL(k_copy_scalar, dim3(1), dim3(1), 0, ctx->stream, (const double *)(scal + SCAL_RHOLAST), out + 2);
    HIPCHECK(ctx, hipGetLastError());
    return DDM_OK;
  }
  if (!c || !own_of || !cp_ptr || !cp_idx) return fail(ctx, DDM_EINVAL, "ddm_debug_reduction: bad arguments");
  if (fin) {
    if (mask) hipLaunchKernelGGL((k_halo_sum_restrict<true, true>), dim3(nb), dim3(WG), 0, ctx->stream, n, own_of, cp_ptr, cp_idx, c, a, mask, (const double *)b, ctx->partial, ctx->ticket, out);
    else hipLaunchKernelGGL((k_halo_sum_restrict<false, true>), dim3(nb), dim3(WG), 0, ctx->stream, n, own_of, cp_ptr, cp_idx, c, a, mask, (const double *)b, ctx->partial, ctx->ticket, out);
    HIPCHECK(ctx, hipGetLastError());
    return DDM_OK;
  }
  hipLaunchKernelGGL((k_halo_sum_restrict<false, false>), dim3(nb), dim3(WG), 0, ctx->stream, n, own_of, cp_ptr, cp_idx, c, a, (const uint8_t *)nullptr, (const double *)nullptr,
                     (double *)nullptr, (unsigned *)nullptr, (double *)nullptr);
  return dot_device(ctx, n, mask, a, b, out);
}
