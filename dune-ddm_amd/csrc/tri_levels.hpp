// Level schedules of an ILU(0) factor in sliced ELL (TriSchedule, LevelEngine: local_factor.hpp): the builder, the single-vector
// launches (engine `levels`) and the block launches every ILU(0) factor runs its multi-RHS solves on.  Needs local_factor.hpp.

static constexpr int SMALL_LEVEL_ROWS = 2048;
static constexpr int SMALL_LEVELS_PER_LAUNCH = 256;

// Builds the level schedule of the lower (upper=false) or upper factor.
static int build_schedule(ddm_ctx *ctx, const ddm_csr *A, const hvec<double> &lu, const std::vector<int64_t> &diag,
                          bool upper, const std::vector<int64_t> &block_ptr, TriSchedule &S)
{
  const int64_t n = A->nrows;
  const int64_t *rp = A->h_rp.data();
  const int32_t *ci = A->h_ci.data();
  std::vector<int32_t> level(n, 0);
  const int32_t maxlev = multi_xcd::tri_levels(n, rp, ci, diag.data(), upper, level.data());
  const int64_t nlev = (int64_t)maxlev + 1;
  S.nlev = nlev;
  std::vector<int64_t> lptr(nlev + 1, 0);
  for (int64_t i = 0; i < n; ++i) lptr[level[i] + 1]++;
  for (int64_t l = 0; l < nlev; ++l) lptr[l + 1] += lptr[l];
  std::vector<int32_t> rows(n);
  {
    std::vector<int64_t> pos(lptr.begin(), lptr.end() - 1);
    for (int64_t i = 0; i < n; ++i) rows[pos[level[i]]++] = (int32_t)i; // ascending row inside a level
  }
  S.desc.resize(nlev);
  int64_t ent = 0;
  for (int64_t l = 0; l < nlev; ++l) {
    const int64_t m = lptr[l + 1] - lptr[l];
    int w = 0;
    for (int64_t r = lptr[l]; r < lptr[l + 1]; ++r) {
      const int64_t i = rows[r];
      const int cnt = upper ? (int)(rp[i + 1] - diag[i] - 1) : (int)(diag[i] - rp[i]);
      w = std::max(w, cnt);
    }
    S.desc[l] = LevelDesc{(int32_t)m, (int32_t)w, lptr[l], ent};
    ent += m * (int64_t)w;
  }
  S.ell_entries = ent;
  hvec<int32_t> cols((size_t)std::max<int64_t>(ent, 1));
  hvec<double> vals((size_t)std::max<int64_t>(ent, 1));
  hvec<double> dinv;
  if (upper) dinv.resize(n);
  // the sliced-ELL fill (strided writes, 1.8 GB per triangle at 216^3) on several threads: levels are independent, each thread takes a
  // run of consecutive levels with about the same number of entries (the two triangles are built at the same time: half the cores each)
  const int nfill = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)std::max(1u, host_threads() / 2), nlev, ent / (1 << 20) + 1}));
  std::vector<int64_t> cut((size_t)nfill + 1, nlev);
  cut[0] = 0;
  for (int t = 1, l = 0; t < nfill; ++t) {
    while (l < nlev && S.desc[l].ent_off < ent * t / nfill) ++l;
    cut[(size_t)t] = l;
  }
  auto fill = [&](int64_t l0, int64_t l1) {
  for (int64_t l = l0; l < l1; ++l) {
    const LevelDesc &D = S.desc[l];
    for (int64_t r = 0; r < D.m; ++r) {
      const int64_t i = rows[D.row_off + r];
      const int64_t k0 = upper ? diag[i] + 1 : rp[i];
      const int64_t k1 = upper ? rp[i + 1] : diag[i];
      int k = 0;
      for (int64_t p = k0; p < k1; ++p, ++k) {
        cols[D.ent_off + (int64_t)k * D.m + r] = ci[p];
        vals[D.ent_off + (int64_t)k * D.m + r] = lu[p];
      }
      for (; k < D.w; ++k) { // padding: a dependency that is already resolved, value 0
        cols[D.ent_off + (int64_t)k * D.m + r] = ci[k0];
        vals[D.ent_off + (int64_t)k * D.m + r] = 0.0;
      }
      if (upper) dinv[D.row_off + r] = lu[diag[i]];
    }
  }
  };
  if (nfill <= 1) fill(0, nlev);
  else {
    std::vector<std::thread> th;
    for (int t = 0; t < nfill; ++t) th.emplace_back(fill, cut[(size_t)t], cut[(size_t)t + 1]);
    for (auto &t : th) t.join();
  }
  // launch plan: runs of small levels share one single-workgroup launch
  int l = 0;
  while (l < nlev) {
    if (S.desc[l].m <= SMALL_LEVEL_ROWS) {
      int c = 0;
      while (l + c < nlev && c < SMALL_LEVELS_PER_LAUNCH && S.desc[l + c].m <= SMALL_LEVEL_ROWS) ++c;
      S.plan.push_back({l, c, true});
      l += c;
    } else {
      S.plan.push_back({l, 1, false});
      l += 1;
    }
  }
  DDMCHECK(upload(ctx, rows.data(), n, S.rows));
  DDMCHECK(upload(ctx, cols.data(), ent, S.cols));
  DDMCHECK(upload(ctx, vals.data(), ent, S.vals));
  if (upper) DDMCHECK(upload(ctx, dinv.data(), n, S.dinv));
  DDMCHECK(upload(ctx, S.desc.data(), nlev, S.d_desc));
  // per-block sub-ranges of the levels (trsv_multi_plan.hpp): what the single-launch block solve walks; depends on the pattern only
  {
    std::vector<int32_t> off;
    multi_xcd::plan_tables(nlev, (int64_t)block_ptr.size() - 1, block_ptr.data(), level.data(), off, S.h_blk_nlev);
    DDMCHECK(upload(ctx, off.data(), (int64_t)off.size(), S.blk_off));
    DDMCHECK(upload(ctx, S.h_blk_nlev.data(), (int64_t)S.h_blk_nlev.size(), S.blk_nlev));
  }
  return DDM_OK;
}

static int enqueue_tri(ddm_ctx *ctx, const TriSchedule &S, bool upper, const double *d, double *x)
{
  for (const auto &p : S.plan) {
    if (p.small) {
      hipLaunchKernelGGL(upper ? k_trsv_small_levels<true> : k_trsv_small_levels<false>, dim3(1), dim3(TRSV_SMALL_WG), 0, ctx->stream, p.count, S.d_desc + p.first,
                         S.rows, S.cols, S.vals, S.dinv, d, x);
    } else {
      const LevelDesc &D = S.desc[p.first];
      const int grid = (D.m + WG - 1) / WG;
      if (upper)
        hipLaunchKernelGGL(k_trsv_upper_level, dim3(grid), dim3(WG), 0, ctx->stream, D.m, D.w, S.rows + D.row_off, S.cols + D.ent_off,
                           S.vals + D.ent_off, S.dinv + D.row_off, x);
      else
        hipLaunchKernelGGL(k_trsv_lower_level, dim3(grid), dim3(WG), 0, ctx->stream, D.m, D.w, S.rows + D.row_off, S.cols + D.ent_off,
                           S.vals + D.ent_off, d, x);
    }
  }
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}

// block solves: one launch per level (wide levels: one workgroup per row)
static void enqueue_multi_levels(ddm_ctx *ctx, const LevelEngine &E, int nrhs, const double *D, int64_t ldd, double *X, int64_t ldx)
{
  for (int pass = 0; pass < 2; ++pass) {
    const TriSchedule &S = pass ? E.U : E.L;
    for (int64_t l = 0; l < S.nlev; ++l) {
      const LevelDesc &L = S.desc[l];
      if (L.m == 0) continue;
      const bool wide = L.w >= 96 && nrhs <= WG;
      const bool quad = !wide && nrhs % 4 == 0 && ldd % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)D & 31) == 0 && ((uintptr_t)X & 31) == 0;
      const int64_t threads = (int64_t)L.m * (quad ? nrhs / 4 : nrhs);
      const unsigned grid = wide ? (unsigned)L.m : (unsigned)((threads + WG - 1) / WG);
      const double *dinv = pass ? S.dinv + L.row_off : nullptr;
      if (quad)
        hipLaunchKernelGGL(pass ? k_trsv_level_multi4<true> : k_trsv_level_multi4<false>, dim3(grid), dim3(WG), 0, ctx->stream, L.m, L.w, nrhs / 4, S.rows + L.row_off,
                           S.cols + L.ent_off, S.vals + L.ent_off, dinv, D, ldd, X, ldx);
      else
        hipLaunchKernelGGL(wide ? (pass ? k_trsv_level_multi_wide<true> : k_trsv_level_multi_wide<false>) : (pass ? k_trsv_level_multi<true> : k_trsv_level_multi<false>), dim3(grid),
                           dim3(WG), 0, ctx->stream, L.m, L.w, nrhs, S.rows + L.row_off, S.cols + L.ent_off, S.vals + L.ent_off, dinv, D, ldd, X, ldx);
    }
  }
}
// single-precision preconditioner sweeps of an ILU(0) factor (kernels.hpp: k_trsv_level_multi4_f32); D, X double
// columns [c0, c0 + nc) of the block on `stream` (nc % 4 == 0): the columns are independent, so two halves can run as two chains
static void enqueue_multi_levels_f32(const LevelEngine &E, hipStream_t stream, int nrhs, int c0, int nc, const double *D, int64_t ldd, double *X, int64_t ldx)
{
  for (int pass = 0; pass < 2; ++pass) {
    const TriSchedule &S = pass ? E.U : E.L;
    for (int64_t l = 0; l < S.nlev; ++l) {
      const LevelDesc &L = S.desc[l];
      if (L.m == 0) continue;
      const unsigned grid = (unsigned)(((int64_t)L.m * (nc / 4) + WG - 1) / WG);
      hipLaunchKernelGGL(pass ? k_trsv_level_multi4_f32<true> : k_trsv_level_multi4_f32<false>, dim3(grid), dim3(WG), 0, stream, L.m, L.w, nc / 4, S.rows + L.row_off, S.cols + L.ent_off,
                         S.vals_f32 + L.ent_off, pass ? S.dinv_f32 + L.row_off : nullptr, D + c0, ldd, E.xf + c0, (int64_t)nrhs, X + c0, ldx);
    }
  }
}
