// xcd2 engine of the ILU(0) solve (XcdEngine: local_factor.hpp; kernels: kernels.hpp): builder and enqueue.  Takes any matrix; built
// on first use (ilu0_prepare_engine).  Needs local_factor.hpp.

// Per-block level schedules of the XCD-local engine: for every diagonal block its L levels then its U
// levels, rows level-sorted, entries in sliced ELL; everything concatenated into one set of arrays (F->xcd).
static int build_xcd_schedule(ddm_ctx *ctx, ddm_ilu0 *F)
{
  const ddm_csr *A = F->A;
  DDMCHECK(ilu0_sync_host_factor(ctx, F)); // (a value refresh drops this part: it is rebuilt here from the refreshed factor)
  const int64_t *rp = A->h_rp.data();
  const int32_t *ci = A->h_ci.data();
  const hvec<double> &lu = F->h_lu;
  const std::vector<int64_t> &diag = F->h_diag;
  const int nb = (int)F->h_block_ptr.size() - 1;
  std::vector<GroupDesc> groups(nb);
  std::vector<LevelDesc> desc;
  std::vector<int64_t> flag_off(nb);
  std::vector<int32_t> rows, cols;
  std::vector<double> vals, dinv;
  rows.reserve(2 * (size_t)A->nrows);
  dinv.reserve(2 * (size_t)A->nrows);
  cols.reserve((size_t)A->nnz);
  vals.reserve((size_t)A->nnz);
  std::vector<int32_t> level(A->nrows);
  int64_t nflag = 0;
  for (int b = 0; b < nb; ++b) {
    const int64_t r0 = F->h_block_ptr[b], r1 = F->h_block_ptr[b + 1];
    groups[b].lev_off = (int64_t)desc.size();
    flag_off[b] = nflag;
    for (int pass = 0; pass < 2; ++pass) {
      const bool upper = pass == 1;
      int32_t maxlev = -1;
      if (!upper)
        for (int64_t i = r0; i < r1; ++i) {
          int32_t l = 0;
          for (int64_t k = rp[i]; k < diag[i]; ++k) l = std::max(l, level[ci[k]] + 1);
          level[i] = l;
          maxlev = std::max(maxlev, l);
        }
      else
        for (int64_t i = r1 - 1; i >= r0; --i) {
          int32_t l = 0;
          for (int64_t k = diag[i] + 1; k < rp[i + 1]; ++k) l = std::max(l, level[ci[k]] + 1);
          level[i] = l;
          maxlev = std::max(maxlev, l);
        }
      const int64_t nlev = (int64_t)maxlev + 1;
      (upper ? groups[b].nlevU : groups[b].nlevL) = (int32_t)nlev;
      std::vector<int64_t> lptr(nlev + 1, 0);
      for (int64_t i = r0; i < r1; ++i) lptr[level[i] + 1]++;
      for (int64_t l = 0; l < nlev; ++l) lptr[l + 1] += lptr[l];
      const int64_t base = (int64_t)rows.size();
      rows.resize(base + (r1 - r0));
      dinv.resize(base + (r1 - r0), 0.0);
      {
        std::vector<int64_t> pos(lptr.begin(), lptr.end() - 1);
        for (int64_t i = r0; i < r1; ++i) rows[base + pos[level[i]]++] = (int32_t)i;
      }
      for (int64_t l = 0; l < nlev; ++l) {
        const int64_t m = lptr[l + 1] - lptr[l];
        int w = 0;
        for (int64_t r = 0; r < m; ++r) {
          const int64_t i = rows[base + lptr[l] + r];
          w = std::max(w, upper ? (int)(rp[i + 1] - diag[i] - 1) : (int)(diag[i] - rp[i]));
        }
        const int64_t ent = (int64_t)cols.size();
        desc.push_back(LevelDesc{(int32_t)m, (int32_t)w, base + lptr[l], ent});
        cols.resize(ent + m * (int64_t)w);
        vals.resize(ent + m * (int64_t)w);
        for (int64_t r = 0; r < m; ++r) {
          const int64_t i = rows[base + lptr[l] + r];
          const int64_t k0 = upper ? diag[i] + 1 : rp[i], k1 = upper ? rp[i + 1] : diag[i];
          int k = 0;
          for (int64_t p = k0; p < k1; ++p, ++k) {
            cols[ent + (int64_t)k * m + r] = ci[p];
            vals[ent + (int64_t)k * m + r] = lu[p];
          }
          for (; k < w; ++k) {
            cols[ent + (int64_t)k * m + r] = ci[k0];
            vals[ent + (int64_t)k * m + r] = 0.0;
          }
          if (upper) dinv[base + lptr[l] + r] = lu[diag[i]];
        }
      }
    }
    nflag += (int64_t)(groups[b].nlevL + groups[b].nlevU) * TRSV_X_MAXW;
  }
  auto X = std::make_unique<XcdEngine>();
  X->ngroups = nb;
  DDMCHECK(upload(ctx, groups.data(), (int64_t)groups.size(), X->groups));
  DDMCHECK(upload(ctx, desc.data(), (int64_t)desc.size(), X->desc));
  DDMCHECK(upload(ctx, flag_off.data(), (int64_t)flag_off.size(), X->flag_off));
  DDMCHECK(upload(ctx, rows.data(), (int64_t)rows.size(), X->rows));
  DDMCHECK(upload(ctx, cols.data(), (int64_t)cols.size(), X->cols));
  DDMCHECK(upload(ctx, vals.data(), (int64_t)vals.size(), X->vals));
  DDMCHECK(upload(ctx, dinv.data(), (int64_t)dinv.size(), X->dinv));
  HIPCHECK(ctx, X->flags.alloc(nflag));
  HIPCHECK(ctx, dev_memset(X->flags, 0, sizeof(unsigned) * (size_t)std::max<int64_t>(nflag, 1)));
  DDMCHECK(ilu0_alloc_xstate(ctx, F));
  {
    std::vector<int64_t> lpos;
    lpos.reserve((size_t)A->nrows);
    int64_t base = 0;
    for (int b = 0; b < nb; ++b) {
      const int64_t nbk = F->h_block_ptr[b + 1] - F->h_block_ptr[b];
      for (int64_t p = 0; p < nbk; ++p) lpos.push_back(base + p);
      base += 2 * nbk;
    }
    DDMCHECK(upload(ctx, lpos.data(), (int64_t)lpos.size(), X->lpos));
  }
  HIPCHECK(ctx, X->dperm.alloc((int64_t)rows.size()));
  HIPCHECK(ctx, hipFuncSetAttribute((const void *)k_trsv_xcd2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(TrsvLds)));
  F->xcd = std::move(X);
  return DDM_OK;
}

static void enqueue_xcd2(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, unsigned *err, unsigned long long *stamps)
{
  const XcdEngine &X = *F->xcd;
  hipLaunchKernelGGL(k_trsv_xcd_prologue, dim3(1), dim3(64), 0, ctx->stream, F->xstate);
  hipLaunchKernelGGL(k_w_permute_in, dim3(grid_for(F->n)), dim3(WG), 0, ctx->stream, F->n, X.lpos, X.rows, d, X.dperm);
  hipLaunchKernelGGL(k_trsv_xcd2, dim3(persistent_grid(ctx)), dim3(64 * (1 + TRSV_L_LOADERS)), sizeof(TrsvLds), ctx->stream, X.ngroups, X.groups, X.desc, X.flag_off,
                     X.rows, X.cols, X.vals, X.dinv, X.dperm, x, X.flags, F->xstate, err, stamps);
}
