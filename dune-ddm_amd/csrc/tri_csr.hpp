// Level schedules of the host sparse direct factor in CSR (TriCsr, CsrDirect: local_factor.hpp): supernode detection and inversion,
// the builder, the single-vector and the block launches.  Needs local_factor.hpp.

// Supernodes of a direct factor: maximal runs J = [j0, j1) of consecutive eliminated indices whose diagonal block L[J, J] is a
// dense triangle (row i of J holds all columns j0 .. i-1; by the symmetric pattern of the factor U[J, J] is dense as well) -- the
// separators of the nested dissection.  Solving through such a block row by row costs |J| dependency levels; with the diagonal
// blocks INVERTED once on the host (dense triangular inverses, |J|^3 / 3 flops) it costs two:
//   t_J = rhs_J - F[J, outside J] x      (|J| independent rows; results in virtual unknowns n + q)
//   x_J = T_J^-1 t_J                     (|J| independent rows of the inverted block)
// which is how sparse triangular solves are usually made parallel on GPUs.  The inverse has as many entries as the triangle it
// replaces.  min_size: smaller runs stay row by row.
struct Supernodes {
  std::vector<int64_t> j0, j1;
  std::vector<int32_t> sn_of;   // supernode of a row or -1
  std::vector<int32_t> virt_of; // virtual unknown (>= n) of a supernode row
  int64_t nvirt = 0;
  std::vector<std::vector<double>> Linv, Uinv; // inverted diagonal blocks (dense s x s, row-major), filled by invert_supernodes
};
// T^-1 of the unit lower / M^-1 of the upper (pivots on the diagonal) diagonal block of every supernode; row-oriented substitution
// (row i of the inverse is a combination of the finished rows: contiguous updates), supernodes in parallel on the host threads
static void invert_supernodes(const hvec<double> &lu, const std::vector<int64_t> &diag, Supernodes &SN)
{
  const size_t ns = SN.j0.size();
  SN.Linv.assign(ns, {});
  SN.Uinv.assign(ns, {});
  std::vector<size_t> order(ns);
  for (size_t q = 0; q < ns; ++q) order[q] = q;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return SN.j1[a] - SN.j0[a] > SN.j1[b] - SN.j0[b]; }); // largest first
  const unsigned hw = host_threads();
  const int nth = (int)std::min<size_t>(hw, std::max<size_t>(ns, 1));
  std::atomic<size_t> next{0};
  std::vector<std::thread> th;
  for (int t = 0; t < nth; ++t)
    th.emplace_back([&]() {
      for (;;) {
        const size_t w = next.fetch_add(1);
        if (w >= ns) break;
        const size_t id = order[w];
        const int64_t j0 = SN.j0[id], j1 = SN.j1[id], sz = j1 - j0;
        std::vector<double> &Li = SN.Linv[id], &Ui = SN.Uinv[id];
        Li.assign((size_t)(sz * sz), 0.0);
        Ui.assign((size_t)(sz * sz), 0.0);
        for (int64_t i = 0; i < sz; ++i) { // Linv[i, :] = e_i - sum_{k < i} L[i, k] Linv[k, :]
          double *ri = Li.data() + i * sz;
          ri[i] = 1.0;
          const int64_t gi = j0 + i;
          for (int64_t k = 0; k < i; ++k) {
            const double l = lu[diag[gi] - (i - k)];
            if (l == 0.0) continue;
            const double *rk = Li.data() + k * sz;
            for (int64_t c = 0; c <= k; ++c) ri[c] -= l * rk[c];
          }
        }
        for (int64_t i = sz - 1; i >= 0; --i) { // Uinv[i, :] = dinv_i (e_i - sum_{k > i} U[i, k] Uinv[k, :])
          double *ri = Ui.data() + i * sz;
          ri[i] = 1.0;
          const int64_t gi = j0 + i;
          for (int64_t k = i + 1; k < sz; ++k) {
            const double u = lu[diag[gi] + (k - i)];
            if (u == 0.0) continue;
            const double *rk = Ui.data() + k * sz;
            for (int64_t c = k; c < sz; ++c) ri[c] -= u * rk[c];
          }
          const double dv = lu[diag[gi]]; // stored inverse pivot
          for (int64_t c = i; c < sz; ++c) ri[c] *= dv;
        }
      }
    });
  for (auto &t : th) t.join();
}
static Supernodes detect_supernodes(const ddm_csr *A, const std::vector<int64_t> &diag, int min_size)
{
  const int64_t n = A->nrows;
  const int64_t *rp = A->h_rp.data();
  const int32_t *ci = A->h_ci.data();
  Supernodes SN;
  SN.sn_of.assign((size_t)n, -1);
  SN.virt_of.assign((size_t)n, -1);
  int64_t j0 = 0;
  while (j0 < n) {
    int64_t j1 = j0 + 1;
    while (j1 < n) {
      const int64_t w = j1 - j0;
      if (diag[j1] - rp[j1] < w || ci[diag[j1] - w] != j0) break;                 // row j1 holds columns j0 .. j1-1
      if (rp[j0 + 1] - diag[j0] - 1 < w || ci[diag[j0] + w] != j1) break;         // row j0 holds column j1 (upper part)
      ++j1;
    }
    bool ok = j1 - j0 >= min_size;
    for (int64_t i = j0; ok && i < j1; ++i) // every row of the run holds i+1 .. j1-1 right behind its diagonal
      ok = (rp[i + 1] - diag[i] - 1 >= j1 - 1 - i) && (i == j1 - 1 || ci[diag[i] + (j1 - 1 - i)] == j1 - 1);
    if (ok) {
      const int32_t id = (int32_t)SN.j0.size();
      SN.j0.push_back(j0);
      SN.j1.push_back(j1);
      for (int64_t i = j0; i < j1; ++i) {
        SN.sn_of[(size_t)i] = id;
        SN.virt_of[(size_t)i] = (int32_t)(n + SN.nvirt++);
      }
    }
    j0 = ok ? j1 : j0 + 1;
  }
  return SN;
}

// block_ptr != nullptr: rows ordered by (block, level), levels numbered per block (blk_lev_ptr), for k_trsv_csr_blocks
static int build_csr_schedule(ddm_ctx *ctx, const ddm_csr *A, const hvec<double> &lu, const std::vector<int64_t> &diag, bool upper, TriCsr &S,
                              const Supernodes &SN, int64_t nblocks = 0, const int64_t *block_ptr = nullptr)
{
  const int64_t n = A->nrows;
  const int64_t *rp = A->h_rp.data();
  const int32_t *ci = A->h_ci.data();
  const int64_t nunk = n + SN.nvirt;
  // ---- transformed rows: dst <- (rhs >= 0 ? rhsvec[rhs] : 0) - sum val * x[col], times dinv ----
  std::vector<int64_t> rptr(1, 0);
  std::vector<int32_t> rcol, rdst, rrhs, rown; // rown: original row the transformed row belongs to (for the block id)
  std::vector<double> rval, rdinv;
  rdst.reserve((size_t)nunk);
  std::vector<int32_t> level((size_t)nunk, 0);
  auto finish_row = [&](int32_t dst, int32_t rhs, double dv, int32_t owner) {
    int32_t l = 0;
    for (int64_t k = rptr.back(); k < (int64_t)rcol.size(); ++k) l = std::max(l, level[(size_t)rcol[(size_t)k]] + 1);
    level[(size_t)dst] = l;
    rptr.push_back((int64_t)rcol.size());
    rdst.push_back(dst);
    rrhs.push_back(rhs);
    rdinv.push_back(dv);
    rown.push_back(owner);
  };
  auto do_supernode = [&](int32_t id) {
    const int64_t j0 = SN.j0[(size_t)id], j1 = SN.j1[(size_t)id], s = j1 - j0;
    const std::vector<double> &Ti = upper ? SN.Uinv[(size_t)id] : SN.Linv[(size_t)id];
    if (!upper) {
      for (int64_t i = j0; i < j1; ++i) { // phase 1: t_i = d_i - F[i, < j0] x
        rcol.insert(rcol.end(), ci + rp[i], ci + (diag[i] - (i - j0)));
        rval.insert(rval.end(), lu.begin() + rp[i], lu.begin() + (diag[i] - (i - j0)));
        finish_row(SN.virt_of[(size_t)i], (int32_t)i, 1.0, (int32_t)i);
      }
      for (int64_t i = j0; i < j1; ++i) { // phase 2: x_i = sum_{c <= i} Tinv[i, c] t_c
        for (int64_t c = j0; c <= i; ++c) {
          rcol.push_back(SN.virt_of[(size_t)c]);
          rval.push_back(-Ti[(size_t)((i - j0) * s + (c - j0))]);
        }
        finish_row((int32_t)i, -1, 1.0, (int32_t)i);
      }
    } else {
      for (int64_t i = j1 - 1; i >= j0; --i) { // phase 1: t_i = y_i - F[i, >= j1] x   (y_i is read from x[i])
        rcol.insert(rcol.end(), ci + (diag[i] + (j1 - i)), ci + rp[i + 1]);
        rval.insert(rval.end(), lu.begin() + (diag[i] + (j1 - i)), lu.begin() + rp[i + 1]);
        finish_row(SN.virt_of[(size_t)i], (int32_t)i, 1.0, (int32_t)i);
      }
      for (int64_t i = j1 - 1; i >= j0; --i) { // phase 2: x_i = sum_{c >= i} Minv[i, c] t_c
        for (int64_t c = i; c < j1; ++c) {
          rcol.push_back(SN.virt_of[(size_t)c]);
          rval.push_back(-Ti[(size_t)((i - j0) * s + (c - j0))]);
        }
        finish_row((int32_t)i, -1, 1.0, (int32_t)i);
      }
    }
  };
  if (!upper) {
    for (int64_t i = 0; i < n; ++i) {
      const int32_t id = SN.sn_of[(size_t)i];
      if (id >= 0) {
        if (i == SN.j0[(size_t)id]) do_supernode(id);
        continue;
      }
      rcol.insert(rcol.end(), ci + rp[i], ci + diag[i]);
      rval.insert(rval.end(), lu.begin() + rp[i], lu.begin() + diag[i]);
      finish_row((int32_t)i, (int32_t)i, 1.0, (int32_t)i);
    }
  } else {
    for (int64_t i = n - 1; i >= 0; --i) {
      const int32_t id = SN.sn_of[(size_t)i];
      if (id >= 0) {
        if (i == SN.j1[(size_t)id] - 1) do_supernode(id);
        continue;
      }
      rcol.insert(rcol.end(), ci + diag[i] + 1, ci + rp[i + 1]);
      rval.insert(rval.end(), lu.begin() + diag[i] + 1, lu.begin() + rp[i + 1]);
      finish_row((int32_t)i, (int32_t)i, lu[diag[i]], (int32_t)i);
    }
  }
  const int64_t nr = (int64_t)rdst.size();
  // ---- levels (per block when block_ptr is given) ----
  std::vector<int32_t> rlev((size_t)nr);
  int32_t maxlev = -1;
  for (int64_t q = 0; q < nr; ++q) {
    rlev[(size_t)q] = level[(size_t)rdst[(size_t)q]];
    maxlev = std::max(maxlev, rlev[(size_t)q]);
  }
  int64_t nlev = (int64_t)maxlev + 1;
  std::vector<int32_t> blp;
  if (block_ptr) {
    std::vector<int32_t> blk_of((size_t)n);
    for (int64_t b = 0; b < nblocks; ++b)
      for (int64_t i = block_ptr[b]; i < block_ptr[b + 1]; ++i) blk_of[(size_t)i] = (int32_t)b;
    std::vector<int32_t> mx((size_t)nblocks, -1);
    for (int64_t q = 0; q < nr; ++q) mx[(size_t)blk_of[(size_t)rown[(size_t)q]]] = std::max(mx[(size_t)blk_of[(size_t)rown[(size_t)q]]], rlev[(size_t)q]);
    blp.assign(1, 0);
    for (int64_t b = 0; b < nblocks; ++b) blp.push_back(blp.back() + mx[(size_t)b] + 1);
    for (int64_t q = 0; q < nr; ++q) rlev[(size_t)q] += blp[(size_t)blk_of[(size_t)rown[(size_t)q]]];
    nlev = blp.back();
    S.nblocks = (int)nblocks;
  }
  S.nlev = nlev;
  std::vector<int64_t> lptr((size_t)nlev + 1, 0);
  for (int64_t q = 0; q < nr; ++q) lptr[(size_t)rlev[(size_t)q] + 1]++;
  for (int64_t l = 0; l < nlev; ++l) lptr[(size_t)l + 1] += lptr[(size_t)l];
  std::vector<int64_t> order((size_t)nr);
  {
    std::vector<int64_t> pos(lptr.begin(), lptr.end() - 1);
    for (int64_t q = 0; q < nr; ++q) order[(size_t)pos[(size_t)rlev[(size_t)q]]++] = q; // stable inside a level
  }
  std::vector<int32_t> rows((size_t)nr), rhs((size_t)nr), cols((size_t)std::max<int64_t>((int64_t)rcol.size(), 1));
  std::vector<int64_t> lrp((size_t)nr + 1, 0);
  std::vector<double> vals((size_t)std::max<int64_t>((int64_t)rval.size(), 1)), dinv((size_t)nr);
  for (int64_t t = 0; t < nr; ++t) {
    const int64_t q = order[(size_t)t];
    rows[(size_t)t] = rdst[(size_t)q];
    rhs[(size_t)t] = rrhs[(size_t)q];
    dinv[(size_t)t] = rdinv[(size_t)q];
    const int64_t len = rptr[(size_t)q + 1] - rptr[(size_t)q];
    lrp[(size_t)t + 1] = lrp[(size_t)t] + len;
    std::copy(rcol.begin() + rptr[(size_t)q], rcol.begin() + rptr[(size_t)q + 1], cols.begin() + lrp[(size_t)t]);
    std::copy(rval.begin() + rptr[(size_t)q], rval.begin() + rptr[(size_t)q + 1], vals.begin() + lrp[(size_t)t]);
  }
  S.desc.resize((size_t)nlev);
  for (int64_t l = 0; l < nlev; ++l) {
    const int64_t m = lptr[(size_t)l + 1] - lptr[(size_t)l];
    const int64_t ent = lrp[(size_t)lptr[(size_t)l + 1]] - lrp[(size_t)lptr[(size_t)l]];
    int Sl = 1; // lanes per row: about a quarter of the average row length
    while (Sl < 64 && 4 * Sl * m < ent) Sl <<= 1;
    S.desc[(size_t)l] = CsrLevel{(int32_t)m, Sl, lptr[(size_t)l]};
  }
  int l = 0;
  while (l < nlev) { // runs of levels whose rows x lanes fit a few rounds of one workgroup are fused
    auto small = [&](int q) { return (int64_t)S.desc[(size_t)q].m * S.desc[(size_t)q].S <= 4 * TRSV_SMALL_WG; };
    if (small(l)) {
      int c = 0;
      while (l + c < nlev && c < 4096 && small(l + c)) ++c;
      S.plan.push_back({l, c, true});
      l += c;
    } else {
      S.plan.push_back({l, 1, false});
      l += 1;
    }
  }
  S.nrows = nr;
  S.entries = (int64_t)rcol.size();
  DDMCHECK(upload(ctx, rows.data(), nr, S.rows));
  DDMCHECK(upload(ctx, rhs.data(), nr, S.rhs));
  DDMCHECK(upload(ctx, lrp.data(), nr + 1, S.lrp));
  DDMCHECK(upload(ctx, cols.data(), (int64_t)rcol.size(), S.cols));
  DDMCHECK(upload(ctx, vals.data(), (int64_t)rval.size(), S.vals));
  if (upper) DDMCHECK(upload(ctx, dinv.data(), nr, S.dinv));
  DDMCHECK(upload(ctx, S.desc.data(), nlev, S.d_desc));
  if (block_ptr) DDMCHECK(upload(ctx, blp.data(), (int64_t)blp.size(), S.blk_lev_ptr));
  return DDM_OK;
}
static int enqueue_tri_csr(ddm_ctx *ctx, const TriCsr &S, bool upper, const double *d, double *x)
{
  if (S.nblocks > 0) { // one workgroup per independent block
    hipLaunchKernelGGL(upper ? k_trsv_csr_blocks<true> : k_trsv_csr_blocks<false>, dim3(S.nblocks), dim3(TRSV_SMALL_WG), 0, ctx->stream, S.blk_lev_ptr, S.d_desc, S.rows, S.rhs, S.lrp,
                       S.cols, S.vals, S.dinv, d, x);
    HIPCHECK(ctx, hipGetLastError());
    return DDM_OK;
  }
  for (const auto &p : S.plan) {
    if (p.fused) {
      hipLaunchKernelGGL(upper ? k_trsv_csr_fused<true> : k_trsv_csr_fused<false>, dim3(1), dim3(TRSV_SMALL_WG), 0, ctx->stream, p.count, S.d_desc + p.first, S.rows, S.rhs, S.lrp,
                         S.cols, S.vals, S.dinv, d, x);
    } else {
      const CsrLevel &L = S.desc[p.first];
      const int gpb = WG / L.S;
      const int grid = (int)std::min<int64_t>(((int64_t)L.m + gpb - 1) / gpb, 8192);
      hipLaunchKernelGGL(upper ? k_trsv_csr_level<true> : k_trsv_csr_level<false>, dim3(grid), dim3(WG), 0, ctx->stream, L, S.rows, S.rhs, S.lrp, S.cols, S.vals, S.dinv, d, x);
    }
  }
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
static void enqueue_multi_levels_csr(ddm_ctx *ctx, const TriCsr &S, bool upper, int nrhs, const double *D, int64_t ldd, double *X, int64_t ldx)
{
  int smax = 1;
  while (2 * smax * nrhs <= WG && smax < 64) smax <<= 1;
  for (int64_t l = 0; l < S.nlev; ++l) {
    const CsrLevel &L = S.desc[l];
    if (L.m == 0) continue;
    const int Sm = std::min(L.S, smax);
    const int rpb = WG / (Sm * nrhs);
    const unsigned grid = (unsigned)((L.m + rpb - 1) / rpb);
    hipLaunchKernelGGL(upper ? k_trsv_csr_level_multi<true> : k_trsv_csr_level_multi<false>, dim3(grid), dim3(WG), 0, ctx->stream, L, Sm, nrhs, S.rows, S.rhs, S.lrp, S.cols, S.vals,
                       S.dinv, D, ldd, X, ldx);
  }
}
