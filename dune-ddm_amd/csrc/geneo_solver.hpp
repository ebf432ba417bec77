// The GenEO eigensolver as an object that outlives one call (included by geneo.hpp after GeneoSetup / GeneoRun; C ABI: ddm_geneo_create,
// ddm_geneo_compute, ddm_geneo_refresh, ddm_geneo_state, ddm_geneo_destroy in include/ddm_hip.h).
//
// A ddm_geneo holds, between calls,
//   * the pencil A~ / C~ (GeneoSetup::At, C: one pattern, two value arrays, host copy of A~), the chosen preconditioner T, the Dirichlet
//     mask and the POU on the device;
//   * the origin map of the pencil: per entry one 32-bit word that says where the entry comes from in A_neu and in B_neu (build_pencil_host),
//     with the row pointers of the two matrices on the device -- what k_geneo_pencil_refresh needs to recompute both value arrays in place;
//   * the raw block X of the last run (n x m doubles, before v <- D v), the start block of a warm run.
// The six n x 3m blocks of a run are allocated by compute and freed before it returns.  A_neu, B_neu and the parameters are borrowed (the
// parameters are read again by every compute, so nev, extra, the threshold and the tolerance may change between two of them; the shift and
// the preconditioner choice are those of the creation); sub_ptr, the POU and the Dirichlet mask are copied.
//
// refresh: pencil values on the device from the matrices' current values (their device arrays, or a staged upload of their host
// arrays for host-only matrices), then the preconditioner -- ILU(0) by ilu0_refresh_impl, the device supernodal factor by sn_refresh,
// both in place with schedules and plans kept; a factor that answers DDM_ENOTIMPL (host-engine direct factor, a device factor whose new
// values belong to the host engine) is dropped and chosen again by GeneoSetup::choose_preconditioner after the host values of A~ have
// been brought up to date.  Any failure leaves the object refusing compute with that code until a refresh succeeds.
//
// ddm_geneo_basis / ddm_msgfem_basis / ddm_svd_basis are create + compute(cold) + destroy on an object without origin map.
#pragma once

// The LOBPCG loop of the head of geneo.hpp at block width nev + extra on a setup: basis_dev is nev x n, eig_host nsub x nev.  kept / mk /
// ldk: the start block of a warm run (GeneoRun::start_block).  keep_out (optional): receives the raw block X (n x m, ld m) at the end;
// *keep_cols is the width it is allocated for.
static int geneo_run(GeneoSetup &K, int nev, const double *kept, int mk, int64_t ldk, double *basis_dev, double *eig_host, ddm_geneo_info *info, dbuf<double> *keep_out, int *keep_cols)
{
  ddm_ctx *ctx = K.ctx;
  const ddm_geneo_params &P = *K.P;
  const int m = nev + std::max(P.extra, 1);
  if (m > GENEO_MAX_BLOCK) return fail(ctx, DDM_ENOTIMPL, "GenEO: nev + extra = %d exceeds %d vectors per subdomain", m, GENEO_MAX_BLOCK);
  for (int64_t s = 0; s < K.nsub; ++s)
    if (K.Q.sub_ptr[s + 1] - K.Q.sub_ptr[s] < 3 * (int64_t)m) return fail(ctx, DDM_EINVAL, "GenEO: subdomain %lld has fewer than 3 (nev + extra) = %d rows", (long long)s, 3 * m);
  GeneoRun G(K, nev);
  DDMCHECK(G.allocate());
  DDMCHECK(G.start_block(kept, mk, ldk));
  int it = 0, converged = 0;
  const auto t_iter = std::chrono::steady_clock::now();
  for (it = 0; it <= P.maxit; ++it) {
    if (it > 0) DDMCHECK(G.search_directions());
    DDMCHECK(G.projected_problem());
    if (it > 0) {
      if (G.residual_test(it)) {
        converged = 1;
        break;
      }
      if (it == P.maxit) break;
    }
    DDMCHECK(G.rayleigh_ritz(/*with_wp=*/it > 0));
    DDMCHECK(G.rotate_blocks());
    if (it > 0 && it % G.refresh_period == 0) DDMCHECK(G.refresh());
  }
  const double t_loop = seconds_since(t_iter);
  if (keep_out) { // (kept may be keep_out's own array: it was read by start_block only, which the loop's first synchronisation is behind)
    if (*keep_cols != m) {
      *keep_cols = 0;
      DDMCHECK(G.W.alloc(*keep_out, (size_t)G.n * m));
      *keep_cols = m;
    }
    launch_geneo_copy_cols(ctx, G.n, m, G.S[G.cur], G.ld, *keep_out, m);
  }
  DDMCHECK(G.output(basis_dev, eig_host));
  if (info) {
    info->iterations = it;
    info->converged = converged;
    info->used_direct = K.direct;
    info->worst_residual = G.worst;
    info->setup_s = 0.0; // (the caller knows what setup preceded this run: geneo_compute_impl)
    info->iterate_s = t_loop;
    info->nev = nev;
    info->direct_flops = K.direct ? ilu0_direct_flops(K.T.get()) : 0.0;
  }
  return DDM_OK;
}

struct ddm_geneo {
  std::vector<int64_t> sub_ptr;
  std::vector<double> pou, pou_pencil;
  std::vector<uint8_t> dirichlet;
  std::unique_ptr<GeneoSetup> K;
  // value refresh: origin map and the row pointers of A_neu / B_neu on the device, staged values of host-only matrices
  bool has_origin = false;
  dbuf<uint32_t> origin;
  dbuf<int64_t> a_rp, b_rp;
  dbuf<double> stage_a, stage_b;
  // warm start
  dbuf<double> X; // n x kept_m, raw
  int kept_m = 0, kept_nev = 0; // kept_m: the width X is allocated for and holds (0: none)
  int32_t pencil_refreshes = 0, prec_in_place = 0, prec_anew = 0;
  int broken = DDM_OK; // a refresh failed: compute answers this until one succeeds
  double setup_s = 0.0; // setup done since the last compute (the creation, a refresh): what that compute reports as info->setup_s
};

static int geneo_create_impl(ddm_ctx *ctx, const GeneoProblem &Q0, const ddm_geneo_params *params, bool want_origin, ddm_geneo **out)
{
  const int64_t nsub = Q0.nsub;
  if (!ctx || !out || !Q0.A || !Q0.B || !Q0.sub_ptr || !Q0.pou || !params || nsub < 1) return fail(ctx, DDM_EINVAL, "%s: bad arguments", Q0.who);
  if (Q0.A->nrows != Q0.A->ncols || Q0.B->nrows != Q0.A->nrows || Q0.B->ncols != Q0.A->ncols)
    return fail(ctx, DDM_EINVAL, "The matrix and the partition of unity must have the same size"); // coarse_spaces.hh:323
  if (Q0.sub_ptr[0] != 0 || Q0.sub_ptr[nsub] != Q0.A->nrows) return fail(ctx, DDM_EINVAL, "sub_ptr does not cover the matrix");
  if (params->nev < 1 || params->extra < 1 || !(params->tolerance > 0.0)) return fail(ctx, DDM_EINVAL, "%s: bad eigensolver parameters", Q0.who);
  const int64_t n = Q0.A->nrows;
  auto G = std::make_unique<ddm_geneo>();
  GeneoProblem Q = Q0;
  if (want_origin) { // a kept object outlives the caller's arrays
    G->sub_ptr.assign(Q0.sub_ptr, Q0.sub_ptr + nsub + 1);
    G->pou.assign(Q0.pou, Q0.pou + n);
    if (Q0.dirichlet) G->dirichlet.assign(Q0.dirichlet, Q0.dirichlet + n);
    if (Q0.pou_pencil) G->pou_pencil.assign(Q0.pou_pencil, Q0.pou_pencil + n);
    Q.sub_ptr = G->sub_ptr.data();
    Q.pou = G->pou.data();
    Q.dirichlet = Q0.dirichlet ? G->dirichlet.data() : nullptr;
    Q.pou_pencil = Q0.pou_pencil ? G->pou_pencil.data() : nullptr;
  }
  G->K = std::make_unique<GeneoSetup>(ctx, Q, params);
  GeneoSetup &K = *G->K;
  hvec<uint32_t> origin;
  bool fits = false;
  K.assemble_pencil(want_origin ? &origin : nullptr, &fits);
  G->has_origin = want_origin && fits;
  DDMCHECK(K.choose_preconditioner());
  DDMCHECK(K.upload_masks());
  G->setup_s = K.t_setup;
  if (G->has_origin) {
    DDMCHECK(upload(ctx, origin.data(), (int64_t)origin.size(), G->origin));
    DDMCHECK(upload(ctx, Q.A->h_rp.data(), n + 1, G->a_rp));
    if (Q.B != Q.A) DDMCHECK(upload(ctx, Q.B->h_rp.data(), n + 1, G->b_rp));
  }
  *out = G.release();
  return DDM_OK;
}

// The threshold mode of spectra_gevp_op (eigensolvers/spectra.hh:157-163, 186-189) around geneo_run: keep the eigenvalues below the
// threshold (at least one), double nev until the largest computed one exceeds it or nev >= nev_max.  Every width iterates on the one
// pencil and preconditioner of the object; the work space and the start block are per width.  start 0: every width starts from the
// random block; 1: the first width from the kept block, a doubled one from the block just converged.
static int geneo_compute_impl(ddm_ctx *ctx, ddm_geneo *G, int start, bool keep, int64_t kmax, double *basis_host, int32_t *nconv, double *eigenvalues_host,
                              ddm_geneo_info *info)
{
  GeneoSetup &K = *G->K;
  const GeneoProblem &Q = K.Q;
  if (!basis_host || !nconv || !eigenvalues_host) return fail(ctx, DDM_EINVAL, "%s: bad arguments", Q.who);
  if (G->broken) return fail(ctx, G->broken, "%s: the last value refresh failed; the eigensolver computes again after one that succeeds", Q.who);
  const ddm_geneo_params &P = *K.P;
  if (P.nev < 1 || P.extra < 1 || !(P.tolerance > 0.0)) return fail(ctx, DDM_EINVAL, "%s: bad eigensolver parameters", Q.who);
  const int64_t n = K.n, nsub = K.nsub;
  const bool warm = start != 0 && G->kept_m > 0; // (start = 1 without a kept block is start = 0, every width of it)
  int nev = warm ? std::max(P.nev, G->kept_nev) : P.nev;
  for (;;) {
    if (nev > kmax) return fail(ctx, DDM_EINVAL, "%s: kmax = %lld is smaller than nev = %d", Q.who, (long long)kmax, nev);
    dbuf<double> basis_dev;
    HIPCHECK(ctx, basis_dev.alloc(nev * std::max<int64_t>(n, 1)));
    std::vector<double> eig((size_t)nsub * nev);
    int rc = geneo_run(K, nev, warm ? (const double *)G->X : nullptr, G->kept_m, G->kept_m, basis_dev, eig.data(), info, keep ? &G->X : nullptr, &G->kept_m);
    if (!rc && keep) G->kept_nev = nev;
    if (!rc && hipMemcpy(basis_host, basis_dev, sizeof(double) * (size_t)nev * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(ctx, DDM_EHIP, "%s: basis download failed", Q.who);
    if (rc) return rc;
    bool done = true;
    if (P.threshold > 0.0) {
      for (int64_t s = 0; s < nsub; ++s) done = done && eig[(size_t)s * nev + nev - 1] >= P.threshold;
      // the block eigensolver takes nev + extra <= GENEO_MAX_BLOCK vectors per subdomain: the doubling stops there and the last
      // converged block is returned (info->nev tells the caller how far it got) instead of failing the whole basis build
      done = done || nev >= P.nev_max || 2 * nev > kmax || 2 * nev + P.extra > GENEO_MAX_BLOCK;
    }
    if (done) {
      for (int64_t s = 0; s < nsub; ++s) {
        int cnt = nev;
        if (P.threshold > 0.0) {
          cnt = 0;
          while (cnt < nev - 1 && eig[(size_t)s * nev + cnt] < P.threshold) ++cnt;
          cnt = std::max(cnt, 1);
        }
        nconv[s] = cnt;
        for (int j = 0; j < nev; ++j) eigenvalues_host[(size_t)s * kmax + j] = eig[(size_t)s * nev + j];
      }
      if (info) info->nev = nev, info->setup_s = G->setup_s;
      G->setup_s = 0.0; // (a compute that follows without a refresh did no setup)
      return DDM_OK;
    }
    nev *= 2;
  }
}

extern "C" int ddm_geneo_create(ddm_ctx *ctx, const ddm_csr *A_neu, const ddm_csr *B_neu, int64_t nsub, const int64_t *sub_ptr, const double *pou_host,
                                const uint8_t *dirichlet_host, const ddm_geneo_params *params, ddm_geneo **out)
{
  const GeneoProblem Q{"ddm_geneo_create", A_neu, B_neu, nsub, sub_ptr, pou_host, dirichlet_host};
  return geneo_create_impl(ctx, Q, params, /*want_origin=*/true, out);
}
extern "C" void ddm_geneo_destroy(ddm_geneo *G) { delete G; }
using geneo_ptr = std::unique_ptr<ddm_geneo, Destroyer<ddm_geneo_destroy>>;

extern "C" int ddm_geneo_compute(ddm_ctx *ctx, ddm_geneo *G, int start, int64_t kmax, double *basis_host, int32_t *nconv, double *eigenvalues_host, ddm_geneo_info *info)
{
  if (!ctx || !G || (start != 0 && start != 1)) return fail(ctx, DDM_EINVAL, "ddm_geneo_compute: bad arguments");
  return geneo_compute_impl(ctx, G, start, /*keep=*/true, kmax, basis_host, nconv, eigenvalues_host, info);
}

extern "C" int ddm_geneo_state(const ddm_geneo *G, int32_t out[4])
{
  if (!G || !out) return DDM_EINVAL;
  out[0] = G->kept_m, out[1] = G->pencil_refreshes, out[2] = G->prec_in_place, out[3] = G->prec_anew;
  return DDM_OK;
}

// *touched: the pencil kernel has been launched -- from there on a failure leaves pencil and preconditioner out of step
static int geneo_refresh_impl(ddm_ctx *ctx, ddm_geneo *G, bool *touched)
{
  GeneoSetup &K = *G->K;
  const auto t0 = std::chrono::steady_clock::now();
  const ddm_csr *A = K.Q.A, *B = K.Q.B;
  if (!G->has_origin)
    return fail(ctx, DDM_ENOTIMPL, "ddm_geneo_refresh: the object keeps no origin map (a row of A_neu or B_neu has more than %lld entries)", (long long)GENEO_ORIGIN_MAX_ROW);
  if (K.Q.pou_pencil || K.Q.op_C || K.Q.con) return fail(ctx, DDM_ENOTIMPL, "ddm_geneo_refresh: plain GenEO pencils only");
  if (A->nrows != K.n || B->nrows != K.n || A->nnz != (int64_t)A->h_va.size() || B->nnz != (int64_t)B->h_va.size())
    return fail(ctx, DDM_EINVAL, "ddm_geneo_refresh: the matrices are not the ones the object was created on");
  DDMCHECK(csr_wait_upload(ctx, A));
  DDMCHECK(csr_wait_upload(ctx, B));
  DDMCHECK(csr_wait_upload(ctx, K.At.get()));
  // (a) the pencil, on the device
  auto values_of = [&](const ddm_csr *M, dbuf<double> &stage, const double **va) -> int {
    if (!M->host_only) {
      *va = M->va;
      return DDM_OK;
    }
    HIPCHECK(ctx, stage.alloc(M->nnz));
    if (M->nnz) HIPCHECK(ctx, hipMemcpyAsync(stage, M->h_va.data(), sizeof(double) * (size_t)M->nnz, hipMemcpyHostToDevice, ctx->stream));
    *va = stage;
    return DDM_OK;
  };
  const double *a_va = nullptr, *b_va = nullptr;
  DDMCHECK(values_of(A, G->stage_a, &a_va));
  if (B == A) b_va = a_va;
  else DDMCHECK(values_of(B, G->stage_b, &b_va));
  *touched = true;
  if (K.n > 0) {
    ScopedTimer t(ctx, "Refresh/geneo pencil");
    hipLaunchKernelGGL(k_geneo_pencil_refresh, dim3((unsigned)((K.n + PENCIL_WAVES - 1) / PENCIL_WAVES)), dim3(64 * PENCIL_WAVES), 0, ctx->stream, K.n, (const int64_t *)K.At->rp,
                       (const int32_t *)K.At->ci, (const uint32_t *)G->origin, (const int64_t *)G->a_rp, a_va, (const int64_t *)(B == A ? G->a_rp : G->b_rp), b_va,
                       (const double *)K.poud, (const double *)K.maskd, K.sigma, K.At->va.get(), K.C->va.get());
    HIPCHECK(ctx, hipGetLastError());
  }
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream)); // (the staged values may be freed, the factor refresh reads A~)
  (void)G->stage_a.reset(), (void)G->stage_b.reset();
  ++G->pencil_refreshes;
  // (b) the preconditioner.  The host values of A~ are brought up to date only where somebody reads them: the refinement probe of the
  // device supernodal factor measures its backward error against them (sn_probe_refinement), the host factorisation and the
  // symmetry check of a factor built anew start from them.  The ILU(0) refresh reads the device values alone.
  bool host_current = false;
  auto sync_host_values = [&]() -> int {
    if (!host_current && K.At->nnz) HIPCHECK(ctx, hipMemcpy(K.At->h_va.data(), K.At->va, sizeof(double) * (size_t)K.At->nnz, hipMemcpyDeviceToHost));
    host_current = true;
    return DDM_OK;
  };
  if (K.T) { // (empty after a rebuild that failed: the object is `broken`, and this refresh is the way out -- straight to the rebuild)
    if (K.T->sn) DDMCHECK(sync_host_values());
    const int rc = ilu0_refresh_impl(ctx, K.T.get());
    if (rc == DDM_OK) {
      ++K.T->refresh_count;
      ++G->prec_in_place;
      G->setup_s = seconds_since(t0);
      return DDM_OK;
    }
    if (rc != DDM_ENOTIMPL) return rc;
  }
  // not refreshed in place: chosen and built anew, by the rules of the creation, on the host values of A~ brought up to date
  K.T.reset();
  K.T_ilu.reset();
  DDMCHECK(sync_host_values());
  K.restart_clock();
  DDMCHECK(K.choose_preconditioner());
  ++G->prec_anew;
  G->setup_s = seconds_since(t0);
  return DDM_OK;
}
extern "C" int ddm_geneo_refresh(ddm_ctx *ctx, ddm_geneo *G)
{
  if (!ctx || !G) return fail(ctx, DDM_EINVAL, "ddm_geneo_refresh: bad arguments");
  bool touched = false;
  const int rc = geneo_refresh_impl(ctx, G, &touched);
  if (touched) G->broken = rc; // (a refusal that touched nothing leaves the object as it was, usable or not)
  return rc;
}

// ---- for tests -------------------------------------------------------------------------------------------------------------------
// The pencil of the object as it is on the device: *nnz always; rowptr (n + 1), col, val_At, val_C (nnz each) where not NULL.  Synchronous.
extern "C" int ddm_geneo_debug_pencil(ddm_ctx *ctx, const ddm_geneo *G, int64_t *nnz, int64_t *rowptr, int32_t *col, double *val_At, double *val_C)
{
  if (!ctx || !G || !nnz) return fail(ctx, DDM_EINVAL, "ddm_geneo_debug_pencil: bad arguments");
  const ddm_csr *At = G->K->At.get(), *C = G->K->C.get();
  DDMCHECK(csr_wait_upload(ctx, At));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  *nnz = At->nnz;
  if (rowptr) HIPCHECK(ctx, hipMemcpy(rowptr, At->rp, sizeof(int64_t) * (size_t)(At->nrows + 1), hipMemcpyDeviceToHost));
  if (col && At->nnz) HIPCHECK(ctx, hipMemcpy(col, At->ci, sizeof(int32_t) * (size_t)At->nnz, hipMemcpyDeviceToHost));
  if (val_At && At->nnz) HIPCHECK(ctx, hipMemcpy(val_At, At->va, sizeof(double) * (size_t)At->nnz, hipMemcpyDeviceToHost));
  if (val_C && At->nnz) HIPCHECK(ctx, hipMemcpy(val_C, C->va, sizeof(double) * (size_t)At->nnz, hipMemcpyDeviceToHost));
  return DDM_OK;
}
// k_geneo_start_block through its launch function: S (n x 3m, device) from kept (n x m_kept, device; its first min(m_kept, m) columns)
// and mask (n, device).  Synchronous.
extern "C" int ddm_geneo_debug_start_block(ddm_ctx *ctx, int64_t n, int m, int m_kept, uint64_t seed, const double *mask, const double *kept, double *S)
{
  if (!ctx || n < 1 || m < 1 || m_kept < 1 || !mask || !kept || !S) return fail(ctx, DDM_EINVAL, "ddm_geneo_debug_start_block: bad arguments");
  launch_geneo_start_block(ctx, n, m, std::min(m_kept, m), m_kept, (unsigned long long)seed, mask, kept, S);
  HIPCHECK(ctx, hipGetLastError());
  return ddm_ctx_sync(ctx);
}
// Host twins (no device, no context): the pencil of (A, B) on the union pattern with its origin map, and the value refresh through
// the map.  rowptr_out: n + 1; col_out, val_At_out, val_C_out, origin_out: room for nnz(A) + nnz(B) entries, *nnz_out are used.
// dirichlet may be NULL.  DDM_ENOTIMPL when a row has more entries than the map addresses.
extern "C" int ddm_geneo_pencil_host(int64_t n, const int64_t *a_rowptr, const int32_t *a_col, const double *a_val, const int64_t *b_rowptr, const int32_t *b_col,
                                     const double *b_val, const double *pou, const uint8_t *dirichlet, double sigma, int64_t *rowptr_out, int32_t *col_out,
                                     double *val_At_out, double *val_C_out, uint32_t *origin_out, int64_t *nnz_out)
{
  if (n < 0 || !a_rowptr || !b_rowptr || !pou || !rowptr_out || !col_out || !val_At_out || !val_C_out || !origin_out || !nnz_out) return DDM_EINVAL;
  if ((a_rowptr[n] > 0 && (!a_col || !a_val)) || (b_rowptr[n] > 0 && (!b_col || !b_val))) return DDM_EINVAL;
  hvec<int64_t> rp;
  hvec<int32_t> ci;
  hvec<double> vT, vC;
  hvec<uint32_t> org;
  if (!build_pencil_host(PencilInput{n, a_rowptr, a_col, a_val, b_rowptr, b_col, b_val}, pou, dirichlet, sigma, rp, ci, vT, vC, &org)) return DDM_ENOTIMPL;
  const size_t nnz = (size_t)rp[(size_t)n];
  std::memcpy(rowptr_out, rp.data(), sizeof(int64_t) * ((size_t)n + 1));
  if (nnz) {
    std::memcpy(col_out, ci.data(), sizeof(int32_t) * nnz);
    std::memcpy(val_At_out, vT.data(), sizeof(double) * nnz);
    std::memcpy(val_C_out, vC.data(), sizeof(double) * nnz);
    std::memcpy(origin_out, org.data(), sizeof(uint32_t) * nnz);
  }
  *nnz_out = (int64_t)nnz;
  return DDM_OK;
}
extern "C" int ddm_geneo_pencil_refresh_host(int64_t n, const int64_t *rowptr, const int32_t *col, const uint32_t *origin, const int64_t *a_rowptr, const double *a_val,
                                             const int64_t *b_rowptr, const double *b_val, const double *pou, const uint8_t *dirichlet, double sigma, double *val_At,
                                             double *val_C)
{
  if (n < 0 || !rowptr || !a_rowptr || !b_rowptr || !pou || (rowptr[n] > 0 && (!col || !origin || !val_At || !val_C))) return DDM_EINVAL;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t q = rowptr[i]; q < rowptr[i + 1]; ++q) {
      const int64_t oa = origin[q] & 0xffffu, ob = origin[q] >> 16;
      if (oa > a_rowptr[i + 1] - a_rowptr[i] || ob > b_rowptr[i + 1] - b_rowptr[i] || (oa && !a_val) || (ob && !b_val) || col[q] < 0 || col[q] >= n) return DDM_EINVAL;
    }
  geneo_pencil_refresh_host(n, rowptr, col, origin, a_rowptr, a_val, b_rowptr, b_val, pou, dirichlet, sigma, val_At, val_C);
  return DDM_OK;
}
