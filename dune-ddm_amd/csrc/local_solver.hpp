// The local solver of the Schwarz level (included by ddm_hip.hip after context.hpp and csr.hpp; C ABI: the ddm_ilu0_* / ddm_chol_* / ddm_direct_* / ddm_sn_host_*
// functions of include/ddm_hip.h): ILU(0) and sparse direct factors and their triangular-solve engines.
//
// A factor (struct ddm_ilu0) holds what all engines share and one part per engine it has: LevelEngine (one launch per level; every
// ILU(0) factor has it, the multi-RHS solves run on it), XcdEngine (xcd2), PipeEngine (pipe), BoxEngine (box), CsrDirect (host sparse
// direct factor, CSR level solves) and SnDirect (supernodal factor on the device).  F->engine is the one record of which engine the
// single-vector solve uses (requested_engine at creation, settle_engine after the background build).  The rest of the library
// reaches factors only through the ddm_ilu0_* entry points and ilu0_create_impl, direct_create_impl, ilu0_solve_epilogue,
// ilu0_solve_multi_ld, ilu0_peek_status and ilu0_direct_flops.

// ---- ILU(0) -----------------------------------------------------------------------------------
// Host factorisation: dune-istl blockILU0Decomposition semantics (IKJ in the pattern, multipliers
// in L, inverse pivots on the diagonal), natural row order; independent diagonal blocks
// (subdomains) are factorised by separate threads.
static int ilu0_factor_block(const int64_t *rp, const int32_t *ci, double *lu, int64_t *diag, int64_t r0, int64_t r1)
{
  for (int64_t i = r0; i < r1; ++i) {
    diag[i] = -1;
    for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
      if (ci[k] < r0 || ci[k] >= r1) return -2; // entry outside the diagonal block
      if (k > rp[i] && ci[k] <= ci[k - 1]) return -3; // unsorted row
      if (ci[k] == i) diag[i] = k;
    }
    if (diag[i] < 0) return -1;
  }
  for (int64_t i = r0; i < r1; ++i) {
    for (int64_t kk = rp[i]; kk < diag[i]; ++kk) {
      const int64_t k = ci[kk];
      lu[kk] *= lu[diag[k]];
      const double lik = lu[kk];
      int64_t pi = kk + 1;
      for (int64_t pk = diag[k] + 1; pk < rp[k + 1]; ++pk) {
        const int32_t j = ci[pk];
        while (pi < rp[i + 1] && ci[pi] < j) ++pi;
        if (pi == rp[i + 1]) break;
        if (ci[pi] == j) lu[pi] -= lik * lu[pk];
      }
    }
    if (lu[diag[i]] == 0.0) return -1;
    lu[diag[i]] = 1.0 / lu[diag[i]];
  }
  return 0;
}

struct TriSchedule { // one triangular factor, level by level in sliced ELL
  int64_t nlev = 0;
  std::vector<LevelDesc> desc;        // per level
  dbuf<int32_t> rows;                 // [n] rows sorted by level
  dbuf<int32_t> cols;                 // sliced ELL columns
  dbuf<double> vals;                  // sliced ELL values
  dbuf<double> dinv;                  // upper only: inverse pivots in level order
  dbuf<float> vals_f32, dinv_f32;     // single-precision copies for the preconditioner sweeps (made on first use)
  dbuf<LevelDesc> d_desc;             // device copy (for the small-level kernel)
  struct Launch {                     // execution plan
    int first, count;                 // levels [first, first+count)
    bool small;                       // one workgroup loops over the levels
  };
  std::vector<Launch> plan;
  int64_t ell_entries = 0;
};

struct TriCsr { // one triangular factor of the sparse direct solver: rows in level order, CSR entries (kernels.hpp: CsrLevel)
  int64_t nlev = 0;
  std::vector<CsrLevel> desc;
  int64_t nrows = 0, entries = 0; // transformed rows (real + virtual unknowns of the supernodes), stored entries
  dbuf<int32_t> rows;             // destination unknown of a row
  dbuf<int32_t> rhs;              // index of its right-hand side (lower: in d, upper: in x) or -1 (none)
  dbuf<int64_t> lrp;
  dbuf<int32_t> cols;
  dbuf<double> vals;
  dbuf<double> dinv; // upper only
  dbuf<CsrLevel> d_desc;
  struct Launch {
    int first, count;
    bool fused;
  };
  std::vector<Launch> plan;
  // block-wise variant (rows ordered by (block, level)): one workgroup per block runs the block's whole solve
  int nblocks = 0;
  dbuf<int32_t> blk_lev_ptr;
};

static constexpr int SMALL_LEVEL_ROWS = 2048;
static constexpr int SMALL_LEVELS_PER_LAUNCH = 256;

// Builds the level schedule of the lower (upper=false) or upper factor.
static int build_schedule(ddm_ctx *ctx, const ddm_csr *A, const hvec<double> &lu, const std::vector<int64_t> &diag,
                          bool upper, TriSchedule &S)
{
  const int64_t n = A->nrows;
  const int64_t *rp = A->h_rp.data();
  const int32_t *ci = A->h_ci.data();
  std::vector<int32_t> level(n, 0);
  int32_t maxlev = -1;
  if (!upper) {
    for (int64_t i = 0; i < n; ++i) {
      int32_t l = 0;
      for (int64_t k = rp[i]; k < diag[i]; ++k) l = std::max(l, level[ci[k]] + 1);
      level[i] = l;
      maxlev = std::max(maxlev, l);
    }
  } else {
    for (int64_t i = n - 1; i >= 0; --i) {
      int32_t l = 0;
      for (int64_t k = diag[i] + 1; k < rp[i + 1]; ++k) l = std::max(l, level[ci[k]] + 1);
      level[i] = l;
      maxlev = std::max(maxlev, l);
    }
  }
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
  return DDM_OK;
}

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

// ---- the parts of a factor ----------------------------------------------------------------------
// Device arrays are dbuf members (device_buffer.hpp), so a part's destructor only says what is NOT memory, or an order that matters.

// Engine of the single-vector solve; the values are the codes ddm_ilu0_engine reports.
enum class Engine : int { Levels = 0, Xcd2 = 4, Pipe = 8, Supernodal = 16, Box = 32 };

struct LevelEngine { // one launch per level (runs of small levels in one workgroup); also the multi-RHS solves of every ILU(0) factor
  TriSchedule L, U;
  dbuf<float> xf; // n x xf_nrhs work block of the single-precision multi-RHS sweeps
  int xf_nrhs = 0;
};

struct XcdEngine { // xcd2 (XCD-local + loader waves): per-block (subdomain) level schedules, built on first use (build_xcd_schedule)
  int ngroups = 0;
  dbuf<GroupDesc> groups;
  dbuf<LevelDesc> desc;
  dbuf<int64_t> flag_off;
  dbuf<int32_t> rows, cols;
  dbuf<double> vals, dinv;
  dbuf<unsigned> flags;
  dbuf<double> dperm; // right-hand side permuted into level order (loader engine)
  dbuf<int64_t> lpos; // positions of the L parts (only those need the permuted right-hand side)
};

struct PipeEngine { // pipe: chains x tasks, see trsv_pipe_host.hpp
  int ngroups = 0;
  dbuf<pipe::Group> groups;
  dbuf<pipe::Task> tasks;
  dbuf<unsigned char> stream;
  dbuf<int32_t> koff, posU, rowU; // rowU: natural row of every U position (-1: padding)
  dbuf<double> ypos, xpos;
  dbuf<unsigned long long> progress;
  dbuf<unsigned> queue;
  int64_t nposU = 0;
  int spread = 0; // placement-independent mode (set when a subdomain has more work per level than one XCD's workgroups take)
  int grid = 0;
  pipe::Stats stats;
};

struct BoxEngine { // box (trsv_box_host.hpp): structured leading box of every block + a nested factor for the rows behind it
  int nblocks = 0;
  int64_t nshell = 0, nprod = 0;
  dbuf<box::Block> blocks;
  dbuf<box::StepTab> steps;
  dbuf<double> stream;
  dbuf<unsigned long long> einfo;
  dbuf<double> E, ext_val;
  dbuf<int32_t> ext_col;
  dbuf<double> xs;
  dbuf<unsigned long long> prog;
  dbuf<unsigned> queue;
  unsigned long long *dbg = nullptr;    // DDM_BOX_CHECK: pinned host words of the kernels' address check (hipHostMalloc)
  int64_t n = 0, stream_len = 0, xs_len = 0, prog_len = 0, einfo_len = 0;
  // shell system
  dbuf<int64_t> srp;
  dbuf<int32_t> sci, srow;
  dbuf<double> sva, ds, xsol;
  ddm_csr *shell_csr = nullptr;
  ddm_ilu0 *shell = nullptr;
  int grid = 0;
  box::Stats stats;
  ~BoxEngine() // the body runs before the members go: the nested factor (it reads shell_csr), then its matrix, then the arrays above
  {
    ddm_ilu0_destroy(shell);
    ddm_csr_destroy(shell_csr);
    if (dbg) (void)hipHostFree(dbg);
  }
};

struct CsrDirect { // host sparse direct factor (ddm_chol_create): lives in a fill-reducing order, d / x are permuted around the solve
  ddm_csr *pattern = nullptr; // host-only CSR pattern of L + D + L^T in the permuted order (owned)
  dbuf<int32_t> perm;         // device: perm[new] = old
  int64_t nvirt = 0;          // virtual unknowns of the supernodal transformation: the permuted solution holds n + nvirt entries
  TriCsr Lc, Uc;              // global levels: multi-RHS solves, one launch per level
  TriCsr Lb, Ub;              // the same factors ordered by (block, level): single right-hand side, one workgroup per block
  ~CsrDirect() { delete pattern; }
};

struct SnDirect { // supernodal factor computed ON THE DEVICE (sn_chol.hpp); solves run on its panels, in place in pd / pD
  std::unique_ptr<sn::Factor> f;
  // iterative refinement (dune/ddm/eigensolvers/umfpack.hh:42-129; UMFPACK refines inside its own solve too): the number of steps
  // is fixed when the factor is created, from the backward error of a probe solve (sn_direct_create), so that the solves stay
  // captured HIP graphs; the matrix is kept as device copies of its three arrays
  int refine_steps = 0;
  double refine_omega[5] = {0, 0, 0, 0, 0}; // backward error of the probe after 0, 1, .. steps
  dbuf<int64_t> ref_rp;
  dbuf<int32_t> ref_ci;
  dbuf<double> ref_va, pr; // pr: residual block (n x pr_cols)
  int pr_cols = 0;
};

struct GraphCache { // one captured, instantiated solve (capture_and_launch)
  hipGraphExec_t exec = nullptr;
  void reset() { if (exec) (void)hipGraphExecDestroy(exec); exec = nullptr; }
  ~GraphCache() { reset(); }
};

struct ddm_ilu0 {
  int64_t n = 0, nnz = 0;
  Engine engine = Engine::Levels;
  hvec<double> h_lu; // factor values in the pattern of A
  std::vector<int64_t> h_diag, h_block_ptr;
  const ddm_csr *A = nullptr;
  // status word of the single-launch engines in pinned, device-mapped HOST memory: a wave that gives up waiting writes its code
  // straight into it, so the host can look at it without synchronising the stream (ilu0_peek_status: every apply checks the
  // applies before it -- fail fast instead of returning stale results until somebody calls ddm_ilu0_status)
  unsigned *err = nullptr;
  dbuf<XcdState> xstate; // tickets and epoch of the persistent kernels (pipe, xcd2, box)
  // direct factors: right-hand side / solution permuted into the factor's order (n, n + nvirt doubles), the same for row-major blocks
  dbuf<double> pd, px;
  dbuf<double> pD, pX;
  int pm_nrhs = 0;
  double direct_flops = 0.0;
  // the pipe / box part is built in the background (its own host threads + uploads; 2.6 s at 216^3, nothing of it is needed before
  // the first single-vector solve): every reader of those parts or of `engine` joins first (ilu0_join)
  std::thread builder;
  int builder_rc = DDM_OK;
  std::string builder_err;
  std::unique_ptr<LevelEngine> lev;
  std::unique_ptr<XcdEngine> xcd;
  std::unique_ptr<PipeEngine> pipe;
  std::unique_ptr<BoxEngine> box;
  std::unique_ptr<CsrDirect> csr;
  std::unique_ptr<SnDirect> sn;
  // HIP graph caches: the single-vector solve for one (d, x, scale, add), the multi-RHS solve for one (D, X, nrhs, ld, f32)
  GraphCache graph, mgraph;
  const double *g_d = nullptr, *g_scale = nullptr, *g_add = nullptr;
  double *g_x = nullptr;
  const double *mg_D = nullptr;
  double *mg_X = nullptr;
  int mg_nrhs = 0;
  int64_t mg_ldd = 0, mg_ldx = 0;
  bool mg_f32 = false; // the cached graph runs the single-precision sweeps
  ~ddm_ilu0() // the body runs before any member goes: the builder thread writes the parts, the graph execs point into the arrays
  {
    if (builder.joinable()) builder.join();
    graph.reset();
    mgraph.reset();
    if (err) (void)hipHostFree(err);
  }
};
static inline double ilu0_direct_flops(const ddm_ilu0 *F) { return F->direct_flops; }

static int ilu0_alloc_status(ddm_ctx *ctx, ddm_ilu0 *F)
{
  if (hipHostMalloc((void **)&F->err, 128, hipHostMallocMapped) != hipSuccess) return fail(ctx, DDM_EHIP, "local solver: allocation failed");
  std::memset(F->err, 0, 128);
  return DDM_OK;
}
// the XcdState of a factor: allocated by the first builder of a persistent engine, shared by the others
static int ilu0_alloc_xstate(ddm_ctx *ctx, ddm_ilu0 *F)
{
  if (F->xstate) return DDM_OK;
  HIPCHECK(ctx, F->xstate.alloc(1));
  HIPCHECK(ctx, dev_memset(F->xstate, 0, sizeof(XcdState)));
  return DDM_OK;
}

// ---- engine choice ------------------------------------------------------------------------------
// At creation: DDM_TRSV_MODE = levels | xcd2 | box | pipe (the default; also any other value), the box engine only where allowed
// (not for its own nested factor); the level kernels for a factor that only sees multi-RHS solves.  Direct factors are created
// with theirs (levels for the host factor, supernodal for the device factor).  The box engine is opt-in: bit-exact, but at the
// benchmark's size still slower than pipe (4.4 against 3.25 ms per solve: DESIGN.md section 3d says what bounds it).
static Engine requested_engine(bool multi_rhs_only, bool box_allowed)
{
  if (multi_rhs_only) return Engine::Levels;
  const char *m = std::getenv("DDM_TRSV_MODE");
  if (!m) return Engine::Pipe;
  if (!std::strcmp(m, "levels")) return Engine::Levels;
  if (!std::strcmp(m, "xcd2")) return Engine::Xcd2;
  return box_allowed && !std::strcmp(m, "box") ? Engine::Box : Engine::Pipe;
}
// After the background build: an engine whose builder declined the matrix hands it on -- box to pipe, pipe to xcd2 (which takes
// any matrix; its schedules are built on first use).  A failed build leaves the choice alone: every call that needs it reports the
// failure.  Idempotent.
static void settle_engine(ddm_ilu0 *F)
{
  if (F->builder_rc) return;
  if (F->engine == Engine::Box && !F->box) F->engine = Engine::Pipe;
  if (F->engine == Engine::Pipe && !F->pipe && F->n > 0) F->engine = Engine::Xcd2;
}
static void ilu0_join_builder(ddm_ilu0 *F)
{
  if (F->builder.joinable()) F->builder.join();
  settle_engine(F);
}
// waits for the background part of the setup; its failure is reported by every call that needs the result
static int ilu0_join(ddm_ctx *ctx, ddm_ilu0 *F)
{
  ilu0_join_builder(F);
  if (F->builder_rc) return fail(ctx, F->builder_rc, "%s", F->builder_err.c_str());
  return DDM_OK;
}
// diagnostic: the stamps of the box engine's last solve (DDM_BOX_CHECK=1 at creation): out[2][128][4] = per sweep and plane of block 0
// {start, end (100 MHz clock), polls of the previous plane's progress word, XCC}; zeros without the switch
extern "C" int ddm_ilu0_box_check(const ddm_ilu0 *F, unsigned long long *out1024)
{
  if (!F || !out1024) return DDM_EINVAL;
  for (int k = 0; k < 1024; ++k) out1024[k] = (F->box && F->box->dbg) ? F->box->dbg[k] : 0ull;
  return DDM_OK;
}
extern "C" int ddm_ilu0_wait(ddm_ctx *ctx, ddm_ilu0 *F) { return F ? ilu0_join(ctx, F) : fail(ctx, DDM_EINVAL, "ddm_ilu0_wait: bad arguments"); }

static int build_pipe_schedule(ddm_ctx *ctx, ddm_ilu0 *F);
static int build_box_engine(ddm_ctx *ctx, ddm_ilu0 *F);
// Level schedules of an ILU(0) factor (values F->h_lu in the pattern of A), its status words, and the pipe or box part it asks for
// (in the background).
static int ilu0_build_engines(ddm_ctx *ctx, ddm_ilu0 *F, const ddm_csr *A, const std::vector<int64_t> &diag, int64_t nblocks, const int64_t *block_ptr,
                              bool multi_rhs_only, bool box_allowed)
{
  F->engine = requested_engine(multi_rhs_only, box_allowed);
  F->A = A;
  F->h_diag = diag;
  F->h_block_ptr.assign(block_ptr, block_ptr + nblocks + 1);
  F->lev = std::make_unique<LevelEngine>();
  DDMCHECK(ilu0_alloc_status(ctx, F));
  // the two triangles of the level schedules on two host threads (each is a single pass over the factor with scattered writes:
  // 1.3 s at 216^3), the pipe / box part (its own thread pool) beside them
  int rcU = DDM_OK;
  std::thread tu([&]() {
    (void)hipSetDevice(ctx->device);
    BackgroundTransfers own_stream;   // (this create may itself run on a background thread: the box engine's nested factor)
    rcU = build_schedule(ctx, A, F->h_lu, diag, true, F->lev->U);
  });
  if ((F->engine == Engine::Pipe || F->engine == Engine::Box) && F->n > 0) {
    F->builder = std::thread([ctx, F]() {
      (void)hipSetDevice(ctx->device);
      BackgroundTransfers own_stream;
      int rc = F->engine == Engine::Box ? build_box_engine(ctx, F) : DDM_OK; // (declined: F->box stays null, pipe takes the matrix)
      if (!rc && !F->box) rc = build_pipe_schedule(ctx, F);                 // (declined: F->pipe stays null, see settle_engine)
      F->builder_rc = rc;
      if (rc) F->builder_err = last_error_of_this_thread();
    });
  }
  int rc = build_schedule(ctx, A, F->h_lu, diag, false, F->lev->L);
  tu.join();
  if (!rc) rc = rcU;
  static const bool background = !std::getenv("DDM_PIPE_ASYNC") || std::atoi(std::getenv("DDM_PIPE_ASYNC")) != 0;
  if (!background || rc) {     // DDM_PIPE_ASYNC=0: the whole setup inside the create call, as before round 4
    const int rcj = ilu0_join(ctx, F);
    if (!rc) rc = rcj;
  }
  return rc;
}
static int ilu0_create_impl(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, bool multi_rhs_only, ddm_ilu0 **out)
{
  if (!ctx || !A || !out || nblocks < 1 || !block_ptr) return fail(ctx, DDM_EINVAL, "ddm_ilu0_create: bad arguments");
  if (A->nrows != A->ncols) return fail(ctx, DDM_EINVAL, "ILU(0) needs a square matrix");
  if (block_ptr[0] != 0 || block_ptr[nblocks] != A->nrows) return fail(ctx, DDM_EINVAL, "block_ptr does not cover the matrix");
  const auto t_begin = std::chrono::steady_clock::now();
  auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); };
  ddm_ilu0 *F = new ddm_ilu0;
  F->n = A->nrows;
  F->nnz = A->nnz;
  hvec_copy(F->h_lu, A->h_va.data(), A->h_va.size());
  std::vector<int64_t> diag(A->nrows);
  std::vector<int> rcs(nblocks, 0);
  {
    const unsigned hw = host_threads();
    const int nthreads = (int)std::min<int64_t>(nblocks, hw);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
      th.emplace_back([&, t]() {
        for (int64_t b = t; b < nblocks; b += nthreads)
          rcs[b] = ilu0_factor_block(A->h_rp.data(), A->h_ci.data(), F->h_lu.data(), diag.data(), block_ptr[b], block_ptr[b + 1]);
      });
    for (auto &t : th) t.join();
  }
  for (int64_t b = 0; b < nblocks; ++b)
    if (rcs[b]) {
      const int rc = rcs[b];
      delete F;
      if (rc == -2) return fail(ctx, DDM_EINVAL, "ILU(0): block %lld has entries outside its diagonal block", (long long)b);
      if (rc == -3) return fail(ctx, DDM_EINVAL, "ILU(0): rows must have sorted column indices");
      return fail(ctx, DDM_ENUMERIC, "ILU(0): missing or zero pivot in block %lld", (long long)b);
    }
  const double t_factor = since();
  const int rc = ilu0_build_engines(ctx, F, A, diag, nblocks, block_ptr, multi_rhs_only, /*box_allowed=*/true);
  if (rc) {
    ddm_ilu0_destroy(F);
    return rc;
  }
  if (std::getenv("DDM_PIPE_VERBOSE"))
    std::fprintf(stderr, "[ddm] ILU(0) setup: %lld rows, factorisation (host, one thread per block) %.2f s, level schedules%s %.2f s\n", (long long)F->n, t_factor,
                 multi_rhs_only ? "" : (F->builder.joinable() ? " (single-launch engine: being built in the background)" : " + single-launch engine"), since() - t_factor);
  *out = F;
  return DDM_OK;
}
extern "C" int ddm_ilu0_create(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, ddm_ilu0 **out)
{
  return ilu0_create_impl(ctx, A, nblocks, block_ptr, false, out);
}

// ---- sparse direct local solver (host Cholesky, device triangular solves) ----------------------------------------
struct CholResult {
  std::vector<int32_t> perm; // perm[new] = old (rank-local indices; blocks stay contiguous)
  hvec<int64_t> rp;
  std::vector<int64_t> diag;
  hvec<int32_t> ci;
  hvec<double> lu;
  double flops = 0.0;
  int64_t nnzL = 0;
  std::string error;
};
// rc: DDM_OK, DDM_ENOTIMPL (more than max_flops: nothing was factorised), DDM_ENUMERIC (not positive definite), DDM_EINVAL
// general = true: L U without pivoting on the pattern of A + A^T (matrices with a positive definite symmetric part)
static int chol_build(int64_t n, const int64_t *rp, const int32_t *ci, const double *va, int64_t nblocks, const int64_t *block_ptr, double max_flops,
                      bool numeric, CholResult &R, bool general = false)
{
  if (n < 0 || !rp || !ci || nblocks < 1 || !block_ptr || block_ptr[0] != 0 || block_ptr[nblocks] != n) {
    R.error = "bad arguments";
    return DDM_EINVAL;
  }
  std::vector<chol::BlockFactor> BF((size_t)nblocks);
  std::vector<chol::PermutedLower> PL((size_t)nblocks);
  std::vector<chol::PermutedLowerLU> PU((size_t)(general ? nblocks : 0));
  std::vector<std::vector<double>> UX((size_t)(general ? nblocks : 0));
  const unsigned hw = host_threads();
  const int nthreads = (int)std::min<int64_t>(nblocks, hw);
  auto parallel = [&](auto fn) {
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
      th.emplace_back([&, t]() {
        for (int64_t b = t; b < nblocks; b += nthreads) fn(b);
      });
    for (auto &t : th) t.join();
  };
  std::vector<int> bad((size_t)nblocks, 0);
  parallel([&](int64_t b) {
    const int64_t r0 = block_ptr[b], r1 = block_ptr[b + 1];
    for (int64_t i = r0; i < r1 && !bad[(size_t)b]; ++i)
      for (int64_t k = rp[i]; k < rp[i + 1]; ++k)
        if (ci[k] < r0 || ci[k] >= r1) bad[(size_t)b] = 1;
    if (bad[(size_t)b]) return;
    chol::Graph G = chol::block_graph(rp, ci, r0, r1);
    BF[(size_t)b].perm = chol::nested_dissection(G);
    if (general) {
      PU[(size_t)b] = chol::permute_lower_lu(rp, ci, va, r0, r1, BF[(size_t)b].perm);
      chol::analyze(PU[(size_t)b].lo, (int32_t)(r1 - r0), BF[(size_t)b]);
    } else {
      PL[(size_t)b] = chol::permute_lower(rp, ci, va, r0, r1, BF[(size_t)b].perm);
      chol::analyze(PL[(size_t)b], (int32_t)(r1 - r0), BF[(size_t)b]);
    }
  });
  for (int64_t b = 0; b < nblocks; ++b)
    if (bad[(size_t)b]) {
      R.error = "block " + std::to_string(b) + " has entries outside its diagonal block";
      return DDM_EINVAL;
    }
  R.flops = 0.0;
  R.nnzL = 0;
  for (auto &f : BF) {
    R.flops += (general ? 2.0 : 1.0) * f.flops;
    R.nnzL += f.nnzL;
  }
  R.perm.resize((size_t)n);
  for (int64_t b = 0; b < nblocks; ++b)
    for (int32_t k = 0; k < BF[(size_t)b].n; ++k) R.perm[(size_t)(block_ptr[b] + k)] = (int32_t)(block_ptr[b] + BF[(size_t)b].perm[(size_t)k]);
  if (max_flops > 0.0 && R.flops > max_flops) {
    R.error = "sparse direct factorisation needs " + std::to_string(R.flops) + " flops (limit " + std::to_string(max_flops) + ")";
    return DDM_ENOTIMPL;
  }
  if (!numeric) return DDM_OK;
  if (!va) {
    R.error = "bad arguments";
    return DDM_EINVAL;
  }
  parallel([&](int64_t b) {
    if (general) {
      if (!chol::factorize_lu(PU[(size_t)b], BF[(size_t)b], UX[(size_t)b])) bad[(size_t)b] = 1;
      PU[(size_t)b] = chol::PermutedLowerLU();
    } else {
      if (!chol::factorize(PL[(size_t)b], BF[(size_t)b])) bad[(size_t)b] = 1;
      PL[(size_t)b] = chol::PermutedLower(); // release
    }
  });
  for (int64_t b = 0; b < nblocks; ++b)
    if (bad[(size_t)b]) {
      R.error = "block " + std::to_string(b) + ": " + BF[(size_t)b].error;
      return DDM_ENUMERIC;
    }
  R.rp.assign(1, 0);
  R.rp.reserve((size_t)n + 1);
  R.diag.reserve((size_t)n);
  for (int64_t b = 0; b < nblocks; ++b) {
    if (general) {
      chol::append_rows_lu(BF[(size_t)b], UX[(size_t)b], block_ptr[b], R.rp, R.ci, R.lu, R.diag);
      std::vector<double>().swap(UX[(size_t)b]);
    } else
      chol::append_rows(BF[(size_t)b], block_ptr[b], R.rp, R.ci, R.lu, R.diag);
    BF[(size_t)b] = chol::BlockFactor();
  }
  return DDM_OK;
}

struct ddm_chol_host {
  CholResult R;
};
extern "C" int ddm_chol_host_create(int64_t n, const int64_t *rp, const int32_t *ci, const double *va, int64_t nblocks, const int64_t *block_ptr,
                                    ddm_chol_host **out)
{
  return ddm_direct_host_create(n, rp, ci, va, nblocks, block_ptr, 0, out);
}
extern "C" int ddm_direct_host_create(int64_t n, const int64_t *rp, const int32_t *ci, const double *va, int64_t nblocks, const int64_t *block_ptr,
                                      int general, ddm_chol_host **out)
{
  if (!out) return DDM_EINVAL;
  ddm_chol_host *H = new ddm_chol_host;
  const int rc = chol_build(n, rp, ci, va, nblocks, block_ptr, 0.0, va != nullptr, H->R, general != 0);
  if (rc) {
    delete H;
    return rc;
  }
  *out = H;
  return DDM_OK;
}
extern "C" void ddm_chol_host_destroy(ddm_chol_host *H) { delete H; }
extern "C" int64_t ddm_chol_host_nnz(const ddm_chol_host *H) { return H ? (int64_t)H->R.ci.size() : 0; }
extern "C" int64_t ddm_chol_host_nnz_factor(const ddm_chol_host *H) { return H ? H->R.nnzL : 0; }
extern "C" double ddm_chol_host_flops(const ddm_chol_host *H) { return H ? H->R.flops : 0.0; }
extern "C" int ddm_chol_host_get(const ddm_chol_host *H, int32_t *perm, int64_t *rp, int32_t *ci, double *lu)
{
  if (!H) return DDM_EINVAL;
  if (perm) std::copy(H->R.perm.begin(), H->R.perm.end(), perm);
  if (rp) std::copy(H->R.rp.begin(), H->R.rp.end(), rp);
  if (ci) std::copy(H->R.ci.begin(), H->R.ci.end(), ci);
  if (lu) std::copy(H->R.lu.begin(), H->R.lu.end(), lu);
  return DDM_OK;
}

// Supernodal Cholesky on the device.  Returns DDM_OK / an error code, or 1 when the factorisation is too small to be worth it and
// force == false (the caller then takes the host path).
// multiply-adds of a supernodal factorisation of all blocks, estimated from the first separator of the LARGEST block alone (host only,
// one thread, ~1 s per 10^6 rows); 0 when that block has entries outside its diagonal block
static double sn_probe_largest_block(const int64_t *rp, const int32_t *ci, int64_t nblocks, const int64_t *block_ptr, bool lu)
{
  int64_t bl = 0;
  for (int64_t b = 1; b < nblocks; ++b)
    if (block_ptr[b + 1] - block_ptr[b] > block_ptr[bl + 1] - block_ptr[bl]) bl = b;
  const int64_t r0 = block_ptr[bl], r1 = block_ptr[bl + 1];
  for (int64_t i = r0; i < r1; ++i)
    for (int64_t k = rp[i]; k < rp[i + 1]; ++k)
      if (ci[k] < r0 || ci[k] >= r1) return 0.0;
  return (lu ? 2.0 : 1.0) * sn::estimate_flops(chol::block_graph(rp, ci, r0, r1)) * (double)nblocks;
}
static int ilu0_solve_epilogue(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, const double *scale, const double *add);
// Fixes the number of iterative-refinement steps of a device factor (SnDirect::refine_steps) from a probe solve with a pseudo-random
// right-hand side: the loop of dune/ddm/eigensolvers/umfpack.hh:42-129 -- backward error omega = ||b - A x|| / (||A||_inf ||x|| + ||b||)
// (here: the larger of that and 1e-2 x the componentwise backward error UMFPACK's own solve refines by), stop below 1e-14, stop when a step does not halve it, at most 3 steps -- run ONCE here instead of in every solve, so that the
// solves stay captured graphs.  DDM_DIRECT_REFINE = off | <steps> overrides.  Returns the last backward error in *omega_out.
static int sn_probe_refinement(ddm_ctx *ctx, ddm_ilu0 *F, const ddm_csr *A, double *omega_out)
{
  const int64_t n = F->n;
  SnDirect &R = *F->sn;
  *omega_out = 0.0;
  int forced = -1, max_steps = 3;
  if (const char *e = std::getenv("DDM_DIRECT_REFINE")) {
    if (!std::strcmp(e, "off")) return DDM_OK;
    forced = std::max(0, std::min(4, std::atoi(e)));
  }
  if (n == 0) return DDM_OK;
  const int64_t *rp = A->h_rp.data();
  const int32_t *ci = A->h_ci.data();
  const double *va = A->h_va.data();
  const unsigned nth = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  auto par_rows = [&](const std::function<void(int64_t, int64_t, unsigned)> &f) {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nth; ++t) th.emplace_back([&, t]() { f(n * t / nth, n * (t + 1) / nth, t); });
    for (auto &t : th) t.join();
  };
  std::vector<double> part(nth, 0.0);
  par_rows([&](int64_t r0, int64_t r1, unsigned t) {
    double m = 0.0;
    for (int64_t i = r0; i < r1; ++i) {
      double a = 0.0;
      for (int64_t k = rp[i]; k < rp[i + 1]; ++k) a += std::fabs(va[k]);
      m = std::max(m, a);
    }
    part[t] = m;
  });
  double anorm = 0.0;
  for (double v : part) anorm = std::max(anorm, v);
  std::vector<double> b((size_t)n), x((size_t)n);
  uint64_t lcg = 0x9E3779B97F4A7C15ull;
  double bn2 = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    b[(size_t)i] = (double)(int64_t)(lcg >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
    bn2 += b[(size_t)i] * b[(size_t)i];
  }
  dbuf<double> db, dx;
  HIPCHECK(ctx, db.alloc(n));
  if (dx.alloc(n) != hipSuccess) return fail(ctx, DDM_EHIP, "sparse direct solver: allocation failed");
  int rc = ddm_memcpy_h2d(ctx, db, b.data(), sizeof(double) * (size_t)n);
  auto omega_now = [&](double &om) -> int {
    int r = ddm_memcpy_d2h(ctx, x.data(), dx, sizeof(double) * (size_t)n); // (synchronises the stream)
    if (r) return r;
    std::vector<double> pr(nth, 0.0), px(nth, 0.0), pc(nth, 0.0);
    par_rows([&](int64_t r0, int64_t r1, unsigned t) {
      double sr = 0.0, sx = 0.0, wc = 0.0;
      for (int64_t i = r0; i < r1; ++i) {
        double res = b[(size_t)i], den = std::fabs(b[(size_t)i]);
        for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
          res -= va[k] * x[(size_t)ci[k]];
          den += std::fabs(va[k] * x[(size_t)ci[k]]);
        }
        sr += res * res;
        sx += x[(size_t)i] * x[(size_t)i];
        if (den > 0.0) wc = std::max(wc, std::fabs(res) / den);
      }
      pr[t] = sr;
      px[t] = sx;
      pc[t] = wc;
    });
    double sr = 0.0, sx = 0.0, wc = 0.0;
    for (unsigned t = 0; t < nth; ++t) sr += pr[t], sx += px[t], wc = std::max(wc, pc[t]);
    // normwise backward error of umfpack.hh:66-74, and the componentwise one UMFPACK's own solve refines by (max_i |r_i| / (|A||x| + |b|)_i),
    // weighted so that ONE threshold (1e-14) means: normwise below 1e-14 and componentwise below 1e-12
    om = std::max(std::sqrt(sr) / (anorm * std::sqrt(sx) + std::sqrt(bn2)), 1e-2 * wc);
    return DDM_OK;
  };
  auto solve_with = [&](int steps) -> int {
    if (steps > 0 && !R.ref_rp) { // device copies of the matrix for the residuals
      HIPCHECK(ctx, R.ref_rp.alloc(n + 1));
      HIPCHECK(ctx, R.ref_ci.alloc(A->nnz));
      HIPCHECK(ctx, R.ref_va.alloc(A->nnz));
      HIPCHECK(ctx, R.pr.alloc(n));
      R.pr_cols = 1;
      HIPCHECK(ctx, hipMemcpyAsync(R.ref_rp, A->rp, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHECK(ctx, hipMemcpyAsync(R.ref_ci, A->ci, sizeof(int32_t) * (size_t)A->nnz, hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHECK(ctx, hipMemcpyAsync(R.ref_va, A->va, sizeof(double) * (size_t)A->nnz, hipMemcpyDeviceToDevice, ctx->stream));
    }
    R.refine_steps = steps;
    F->graph.reset();
    return ilu0_solve_epilogue(ctx, F, db, dx, nullptr, nullptr);
  };
  double om = 0.0, om_prev = 0.0;
  int steps = 0;
  if (!rc) rc = solve_with(0);
  if (!rc) rc = omega_now(om);
  R.refine_omega[0] = om;
  while (!rc && steps < (forced >= 0 ? forced : max_steps)) {
    if (forced < 0) {
      if (om < 1e-14 || !(om == om)) break;            // converged (or NaN: refinement cannot help)
      if (steps > 0 && om > om_prev / 2.0) break;      // the last step did not halve the backward error
    }
    om_prev = om;
    rc = solve_with(steps + 1);
    if (!rc) rc = omega_now(om);
    ++steps;
    R.refine_omega[std::min(steps, 4)] = om;
  }
  R.refine_steps = steps;
  F->graph.reset(); // (bound to the probe vectors)
  if (steps == 0) { // (no residuals needed)
    (void)R.ref_rp.reset(), (void)R.ref_ci.reset(), (void)R.ref_va.reset(), (void)R.pr.reset();
    R.pr_cols = 0;
  }
  *omega_out = om;
  return rc;
}
static int sn_direct_create(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, double max_flops, bool force, bool lu, bool setup_use, ddm_ilu0 **out)
{
  const int64_t n = A->nrows;
  if (block_ptr[0] != 0 || block_ptr[nblocks] != n) return fail(ctx, DDM_EINVAL, "block_ptr does not cover the matrix");
  const int64_t *rp = A->h_rp.data();
  const int32_t *ci = A->h_ci.data();
  std::vector<sn::BlockSym> BS((size_t)nblocks);
  std::vector<int> bad((size_t)nblocks, 0);
  std::vector<double> quick((size_t)nblocks, 0.0);
  if (max_flops > 0.0 && nblocks > 1) {
    // the largest block first, alone: when its first separator already says "a factor of four beyond the limit" the other blocks are
    // not looked at (the callers run other host work beside this analysis: one busy thread instead of one per block)
    const double q = sn_probe_largest_block(rp, ci, nblocks, block_ptr, lu);
    if (q > 4.0 * max_flops)
      return fail(ctx, DDM_ENOTIMPL, "sparse direct solver: the factorisation needs about %.1g flops (estimate from the first separator of the largest block; limit %.3g)", q,
                  max_flops);
  }
  {
    const unsigned hw = host_threads();
    const int nthreads = (int)std::min<int64_t>(nblocks, hw);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
      th.emplace_back([&, t]() {
        for (int64_t b = t; b < nblocks; b += nthreads) {
          const int64_t r0 = block_ptr[b], r1 = block_ptr[b + 1];
          for (int64_t i = r0; i < r1 && !bad[(size_t)b]; ++i)
            for (int64_t k = rp[i]; k < rp[i + 1]; ++k)
              if (ci[k] < r0 || ci[k] >= r1) bad[(size_t)b] = 1;
          if (bad[(size_t)b]) continue;
          const chol::Graph G = chol::block_graph(rp, ci, r0, r1);
          if (max_flops > 0.0) { // early decline from the first separator alone: a factor of four beyond the limit is not worth the full ordering
            quick[(size_t)b] = (lu ? 2.0 : 1.0) * sn::estimate_flops(G);
            if (quick[(size_t)b] * (double)nblocks > 4.0 * max_flops) continue;
          }
          BS[(size_t)b] = sn::analyse(G);
        }
      });
    for (auto &t : th) t.join();
  }
  for (int64_t b = 0; b < nblocks; ++b)
    if (bad[(size_t)b]) return fail(ctx, DDM_EINVAL, "sparse direct solver: block %lld has entries outside its diagonal block", (long long)b);
  if (max_flops > 0.0) {
    double q = 0.0;
    for (double v : quick) q = std::max(q, v);
    if (q * (double)nblocks > 4.0 * max_flops)
      return fail(ctx, DDM_ENOTIMPL, "sparse direct solver: the factorisation needs about %.1g flops (estimate from the first separator; limit %.3g)", q * (double)nblocks, max_flops);
  }
  double flops = 0.0;
  int64_t entries = 0;
  for (auto &S : BS) {
    flops += (lu ? 2.0 : 1.0) * S.flops;
    entries += (lu ? 2 : 1) * S.entries; // (L U: the U^T blocks; slightly over-counted by the diagonal blocks)
  }
  double min_flops = setup_use ? 1e10 : 2e10; // (see direct_create_impl)
  if (const char *e = std::getenv("DDM_DIRECT_DEVICE_MIN_FLOPS")) min_flops = std::atof(e);
  if (!force && flops < min_flops) return 1;
  if (max_flops > 0.0 && flops > max_flops)
    return fail(ctx, DDM_ENOTIMPL, "sparse direct solver: the factorisation needs %.3g flops (limit %.3g)", flops, max_flops);
  DDMCHECK(csr_wait_upload(ctx, A)); // (matrices the library assembled itself are uploaded by a helper thread: csr_adopt)
  if (A->host_only) return fail(ctx, DDM_EINVAL, "the matrix was created without device arrays (ddm_csr_create_host)");
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)entries * 8.0 > 0.85 * (double)free_b)
    return fail(ctx, DDM_ENOTIMPL, "sparse direct solver: the factor needs %.1f GB, %.1f GB of device memory are free", entries * 8e-9, free_b * 1e-9);
  const auto t0 = std::chrono::steady_clock::now();
  sn::Factor *S = new sn::Factor;
  if (!sn::build(*S, n, nblocks, block_ptr, BS, lu)) {
    delete S;
    return fail(ctx, DDM_EHIP, "sparse direct solver (device): allocation of %.1f GB failed", entries * 8e-9);
  }
  unsigned badsn = 0, perturbed = 0;
  double amax = 0.0;
  if (lu)
    for (double v : A->h_va) amax = std::max(amax, std::fabs(v));
  const hipError_t he = sn::factorize(*S, ctx->stream, A->rp, A->ci, A->va, &badsn, 1.4901161193847656e-08 * amax, &perturbed);
  if (he != hipSuccess) {
    delete S;
    return fail(ctx, DDM_EHIP, "sparse direct solver (device): %s", hipGetErrorString(he));
  }
  if (badsn) {
    delete S;
    if (lu && !force) return 1; // (not forced: the host engine takes the matrix)
    return fail(ctx, DDM_ENUMERIC, lu ? "sparse direct solver: vanishing pivot column inside the diagonal block of supernode %u (matrix singular?)"
                                     : "sparse direct solver: matrix is not positive definite (supernode %u)", badsn - 1);
  }
  if (std::getenv("DDM_PIPE_VERBOSE"))
    std::fprintf(stderr, "[ddm] device supernodal %s: %lld rows, %d supernodes, %d levels, %.2f GB of panels, %.3g flops, numeric factorisation %.3f s (%.2f TFLOP/s)\n",
                 lu ? "L U" : "Cholesky", (long long)n, S->nsn, S->nlev, (S->entries + S->uentries) * 8e-9, (lu ? 2.0 : 1.0) * S->flops, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(),
                 (lu ? 4e-12 : 2e-12) * S->flops / std::max(1e-9, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()));
  ddm_ilu0 *F = new ddm_ilu0;
  F->n = n;
  F->nnz = S->entries + S->uentries;
  F->direct_flops = (lu ? 2.0 : 1.0) * S->flops;
  F->engine = Engine::Supernodal;
  F->sn = std::make_unique<SnDirect>();
  F->sn->f.reset(S);
  int rc = ilu0_alloc_status(ctx, F);
  if (!rc && (F->pd.alloc(n) != hipSuccess || F->px.alloc(n) != hipSuccess))
    rc = fail(ctx, DDM_EHIP, "sparse direct solver: allocation failed");
  double omega = 0.0;
  if (!rc) rc = sn_probe_refinement(ctx, F, A, &omega);
  if (rc) {
    ddm_ilu0_destroy(F);
    return rc;
  }
  if (std::getenv("DDM_PIPE_VERBOSE"))
    std::fprintf(stderr, "[ddm] device supernodal %s: single-vector solve: levels 0..%d by launches, %d top levels by the persistent kernel (%d forward phases, grid %d, %s)\n",
                 lu ? "L U" : "Cholesky", S->ltop - 1, S->ntop, S->top.nph, S->top_grid, S->top_spread ? "one group over all XCDs" : "block b on XCD b % 8");
  if (std::getenv("DDM_PIPE_VERBOSE") && S->chains_ready)
    std::fprintf(stderr, "[ddm] device supernodal %s: the top levels as %d dense chains on %d chain levels (longest %d links; inverse triangles %.1f MB, external blocks %.1f MB%s), grid %d\n",
                 lu ? "L U" : "Cholesky", S->ch.nchain(), S->ch.nclev, S->ch.max_links, S->ch.wtot * 8e-6, S->ch.etot * 8e-6, lu ? ", twice for L U" : "", S->chain_grid);
  if (std::getenv("DDM_PIPE_VERBOSE"))
    std::fprintf(stderr, "[ddm] device supernodal %s: %d refinement step(s) per solve, backward error of the probe %.2e -> %.2e%s\n", lu ? "L U" : "Cholesky", F->sn->refine_steps,
                 F->sn->refine_omega[0], omega, perturbed ? " (vanishing pivot columns replaced)" : "");
  if (!(omega <= 1e-9)) { // element growth beyond what pivoting inside the supernodes and three refinement steps repair
    ddm_ilu0_destroy(F);
    if (!force) return 1;
    return fail(ctx, DDM_ENUMERIC, "sparse direct solver (device): backward error %.2e after iterative refinement (the matrix needs pivoting across supernodes)", omega);
  }
  *out = F;
  return DDM_OK;
}
// host part of the device engine alone (ordering + supernodal symbolic analysis; no device needed): used by the CPU tests
struct ddm_sn_host {
  std::vector<sn::BlockSym> BS;
  std::vector<int64_t> block_ptr;
};
extern "C" int ddm_sn_host_create(int64_t n, const int64_t *rp, const int32_t *ci, int64_t nblocks, const int64_t *block_ptr, ddm_sn_host **out)
{
  if (!out || !rp || !ci || nblocks < 1 || !block_ptr || block_ptr[0] != 0 || block_ptr[nblocks] != n) return DDM_EINVAL;
  ddm_sn_host *H = new ddm_sn_host;
  H->block_ptr.assign(block_ptr, block_ptr + nblocks + 1);
  for (int64_t b = 0; b < nblocks; ++b) H->BS.push_back(sn::analyse(chol::block_graph(rp, ci, block_ptr[b], block_ptr[b + 1])));
  *out = H;
  return DDM_OK;
}
extern "C" void ddm_sn_host_destroy(ddm_sn_host *H) { delete H; }
// sizes[4] = {supernodes, entries of `rows`, panel entries, levels}; flops = multiply-adds of the factorisation
extern "C" int ddm_sn_host_sizes(const ddm_sn_host *H, int64_t block, int64_t *sizes, double *flops)
{
  if (!H || block < 0 || block >= (int64_t)H->BS.size() || !sizes) return DDM_EINVAL;
  const sn::BlockSym &S = H->BS[(size_t)block];
  int32_t nlev = 0;
  for (int32_t l : S.level) nlev = std::max(nlev, l + 1);
  sizes[0] = (int64_t)S.first.size() - 1;
  sizes[1] = (int64_t)S.rows.size();
  sizes[2] = S.entries;
  sizes[3] = nlev;
  if (flops) *flops = S.flops;
  return DDM_OK;
}
// perm[n_b] (perm[new] = old, block-local), first[nsn + 1], rptr[nsn + 1], rows[...], parent[nsn], level[nsn] of one block
extern "C" int ddm_sn_host_get(const ddm_sn_host *H, int64_t block, int32_t *perm, int32_t *first, int64_t *rptr, int32_t *rows, int32_t *parent, int32_t *level)
{
  if (!H || block < 0 || block >= (int64_t)H->BS.size()) return DDM_EINVAL;
  const sn::BlockSym &S = H->BS[(size_t)block];
  if (perm) std::copy(S.perm.begin(), S.perm.end(), perm);
  if (first) std::copy(S.first.begin(), S.first.end(), first);
  if (rptr) std::copy(S.rptr.begin(), S.rptr.end(), rptr);
  if (rows) std::copy(S.rows.begin(), S.rows.end(), rows);
  if (parent) std::copy(S.parent.begin(), S.parent.end(), parent);
  if (level) std::copy(S.level.begin(), S.level.end(), level);
  return DDM_OK;
}
extern "C" int ddm_chol_create(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, double max_flops, ddm_ilu0 **out)
{
  return ddm_direct_create(ctx, A, nblocks, block_ptr, 0, max_flops, out);
}
static int direct_create_impl(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, int general, double max_flops, bool setup_use, ddm_ilu0 **out);
extern "C" int ddm_direct_create(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, int general, double max_flops, ddm_ilu0 **out)
{
  return direct_create_impl(ctx, A, nblocks, block_ptr, general, max_flops, false, out);
}
// setup_use: the factor serves a handful of block solves during a setup phase (GenEO preconditioner, harmonic extensions) -- the
// device engine pays from ~1e10 multiply-adds.  As the local solver of a Krylov loop the host engine's CSR level solves are the
// faster single-vector solves (measured on configs[4]: 1.31 against 1.75 ms), but its factorisation costs ~1 s per 1e10
// multiply-adds against ~0.05 s on the device: from 2e10 the device engine wins the time to solution of any solve shorter than
// several thousand iterations, so that is the default there (DDM_DIRECT_DEVICE_MIN_FLOPS / DDM_DIRECT_ENGINE override).
static int direct_create_impl(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, int general, double max_flops, bool setup_use, ddm_ilu0 **out)
{
  if (!ctx || !A || !out || nblocks < 1 || !block_ptr) return fail(ctx, DDM_EINVAL, "ddm_direct_create: bad arguments");
  if (A->nrows != A->ncols) return fail(ctx, DDM_EINVAL, "the sparse direct solver needs a square matrix");
  // Engine: "device" = supernodal factorisation and solves on the GPU (sn_chol.hpp; symmetric positive definite input), "host" = the
  // up-looking host factorisation with CSR level solves on the device.  Default: the device engine when the matrix is symmetric
  // and the factorisation is worth it (DDM_DIRECT_DEVICE_MIN_FLOPS; defaults in direct_create_impl); DDM_DIRECT_ENGINE overrides.
  {
    const char *eng = std::getenv("DDM_DIRECT_ENGINE");
    if (!eng || std::strcmp(eng, "host") != 0) {
      const int rcs = sn_direct_create(ctx, A, nblocks, block_ptr, max_flops, eng && !std::strcmp(eng, "device"), general != 0, setup_use, out);
      if (rcs != 1) return rcs; // 1 = not taken (too small for the device engine): fall through to the host path
    }
  }
  CholResult R;
  const int rc0 = chol_build(A->nrows, A->h_rp.data(), A->h_ci.data(), A->h_va.data(), nblocks, block_ptr, max_flops, true, R, general != 0);
  if (rc0) return fail(ctx, rc0, "sparse direct solver: %s", R.error.c_str());
  ddm_ilu0 *F = new ddm_ilu0;
  F->n = A->nrows;
  F->nnz = (int64_t)R.ci.size();
  F->direct_flops = R.flops;
  F->h_lu = std::move(R.lu);
  // a direct factor has few, wide rows per level and thousands of levels: the level kernels (runs of small levels fused into one
  // workgroup that splits wide rows over lanes) take it; the pipe / xcd2 engines are built for the narrow rows of ILU(0)
  F->engine = Engine::Levels;
  F->csr = std::make_unique<CsrDirect>();
  CsrDirect &C = *F->csr;
  ddm_csr *P = new ddm_csr; // host-only pattern of the factor (the schedule builders read h_rp / h_ci)
  P->nrows = P->ncols = A->nrows;
  P->nnz = F->nnz;
  P->h_rp = std::move(R.rp);
  P->h_ci = std::move(R.ci);
  C.pattern = P;
  F->A = P;
  F->h_diag = R.diag;
  F->h_block_ptr.assign(block_ptr, block_ptr + nblocks + 1);
  int min_sn = 8;
  if (const char *e = std::getenv("DDM_DIRECT_SUPERNODE_MIN")) min_sn = std::max(2, std::atoi(e)); // a huge value switches the transformation off
  Supernodes SN = detect_supernodes(P, R.diag, min_sn);
  invert_supernodes(F->h_lu, R.diag, SN);
  C.nvirt = SN.nvirt;
  int rc = build_csr_schedule(ctx, P, F->h_lu, R.diag, false, C.Lc, SN);
  if (!rc) rc = build_csr_schedule(ctx, P, F->h_lu, R.diag, true, C.Uc, SN);
  // Few, large levels (the supernodal transformation worked): one grid-wide launch per level.  Thousands of small levels and
  // enough independent blocks: one workgroup per block walks its levels with workgroup barriers instead.
  if (!rc && nblocks >= 4 && C.Lc.nlev + C.Uc.nlev > 600) {
    rc = build_csr_schedule(ctx, P, F->h_lu, R.diag, false, C.Lb, SN, nblocks, block_ptr);
    if (!rc) rc = build_csr_schedule(ctx, P, F->h_lu, R.diag, true, C.Ub, SN, nblocks, block_ptr);
  }
  if (std::getenv("DDM_PIPE_VERBOSE"))
    std::fprintf(stderr, "[ddm] direct factor: %lld rows, %lld stored entries; %zu supernodes (>= %d rows) with %lld rows; levels L/U %lld/%lld (transformed rows %lld)\n",
                 (long long)F->n, (long long)F->nnz, SN.j0.size(), min_sn, (long long)SN.nvirt, (long long)C.Lc.nlev, (long long)C.Uc.nlev, (long long)C.Lc.nrows);
  if (!rc) rc = ilu0_alloc_status(ctx, F);
  if (!rc) rc = upload(ctx, R.perm.data(), A->nrows, C.perm);
  if (!rc && (F->pd.alloc(F->n) != hipSuccess || F->px.alloc(F->n + C.nvirt) != hipSuccess))
    rc = fail(ctx, DDM_EHIP, "ddm_chol_create: allocation failed");
  if (rc) {
    ddm_ilu0_destroy(F);
    return rc;
  }
  *out = F;
  return DDM_OK;
}
extern "C" int ddm_ilu0_is_direct(const ddm_ilu0 *F) { return F && (F->csr || F->sn) ? 1 : 0; }
extern "C" int ddm_ilu0_refinement(const ddm_ilu0 *F, double *omega)
{
  if (!F) return 0;
  if (omega)
    for (int k = 0; k < 5; ++k) omega[k] = F->sn ? F->sn->refine_omega[k] : 0.0;
  return F->sn ? F->sn->refine_steps : 0;
}
extern "C" int64_t ddm_ilu0_nnz(const ddm_ilu0 *F) { return F ? F->nnz : 0; }
extern "C" void ddm_ilu0_destroy(ddm_ilu0 *F) { delete F; }
// 0 = ok, 1 = a wave of the persistent kernel gave up waiting (results invalid); synchronous
extern "C" int ddm_ilu0_status(ddm_ctx *ctx, const ddm_ilu0 *F, int *status)
{
  if (!F || !status) return fail(ctx, DDM_EINVAL, "ddm_ilu0_status: bad arguments");
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  *status = (int)*(volatile unsigned *)F->err;
  return DDM_OK;
}
// the same word WITHOUT synchronising: what the solves that have finished so far reported (0 = nothing wrong yet)
static inline unsigned ilu0_peek_status(const ddm_ilu0 *F) { return (F && F->err) ? *(volatile unsigned *)F->err : 0u; }
extern "C" int ddm_ilu0_peek_status(const ddm_ilu0 *F) { return (int)ilu0_peek_status(F); }
extern "C" int64_t ddm_ilu0_num_levels(const ddm_ilu0 *F, int upper)
{
  if (F->sn) return F->sn->f->nlev;
  if (F->csr) return upper ? F->csr->Uc.nlev : F->csr->Lc.nlev;
  return upper ? F->lev->U.nlev : F->lev->L.nlev;
}
// engine the next ddm_ilu0_solve uses (enum Engine)
extern "C" int ddm_ilu0_engine(const ddm_ilu0 *F)
{
  if (!F) return -1;
  ilu0_join_builder(const_cast<ddm_ilu0 *>(F)); // (the answer depends on what the builder found)
  return (int)F->engine;
}
extern "C" int ddm_ilu0_get_factors_host(ddm_ctx *ctx, const ddm_ilu0 *F, double *lu_host)
{
  if (!F || !lu_host) return fail(ctx, DDM_EINVAL, "bad arguments");
  if (F->sn) return fail(ctx, DDM_ENOTIMPL, "ddm_ilu0_get_factors_host: the device supernodal factor has no CSR form");
  std::memcpy(lu_host, F->h_lu.data(), sizeof(double) * (size_t)F->nnz);
  return DDM_OK;
}

// Per-block level schedules of the XCD-local engine: for every diagonal block its L levels then its U
// levels, rows level-sorted, entries in sliced ELL; everything concatenated into one set of arrays (F->xcd).
static int build_xcd_schedule(ddm_ctx *ctx, ddm_ilu0 *F)
{
  const ddm_csr *A = F->A;
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

// Chain/task schedule of the pipe engine (F->pipe); left null when the builder reports that the matrix does not fit the tile
// format (settle_engine then hands the matrix to xcd2).
static int build_pipe_schedule(ddm_ctx *ctx, ddm_ilu0 *F)
{
  const ddm_csr *A = F->A;
  pipe::Options opt;
  if (const char *e = std::getenv("DDM_PIPE_DELTA")) opt.delta = std::atoi(e);
  if (const char *e = std::getenv("DDM_PIPE_SPAN")) opt.max_span = std::atoi(e);
  if (const char *e = std::getenv("DDM_PIPE_REUSE")) opt.vote = std::atoi(e);
  int spread_env = -1;
  if (const char *e = std::getenv("DDM_PIPE_SPREAD")) spread_env = std::atoi(e);
  pipe::Schedule S;
  const int nb = (int)F->h_block_ptr.size() - 1;
  if (!pipe::build(A->nrows, A->h_rp.data(), A->h_ci.data(), F->h_lu.data(), F->h_diag.data(), nb, F->h_block_ptr.data(), opt, S)) {
    if (std::getenv("DDM_PIPE_VERBOSE")) std::fprintf(stderr, "[ddm] pipe engine not applicable: %s\n", S.error.c_str());
    return DDM_OK;
  }
  auto E = std::make_unique<PipeEngine>();
  E->ngroups = nb;
  E->stats = S.stats;
  // one XCD hosts 64 workgroups (2 per CU): a subdomain whose sweeps are wider than ~48 wavefronts per level is spread over
  // all XCDs (write-through hand-overs); measured at 216^3: 1 subdomain 6.9 vs 9.2 ms, 2 subdomains 7.6 vs 8.3 ms
  E->spread = spread_env >= 0 ? spread_env : (nb < 8 && S.stats.max_rows_per_level > 48.0 * 64.0 ? 1 : 0);
  E->nposU = S.nposU;
  DDMCHECK(upload(ctx, S.groups.data(), (int64_t)S.groups.size(), E->groups));
  DDMCHECK(upload(ctx, S.tasks.data(), (int64_t)S.tasks.size(), E->tasks));
  DDMCHECK(upload(ctx, S.stream.data(), (int64_t)S.stream.size(), E->stream));
  DDMCHECK(upload(ctx, S.koff.data(), (int64_t)S.koff.size(), E->koff));
  DDMCHECK(upload(ctx, S.posU.data(), (int64_t)S.posU.size(), E->posU));
  {
    std::vector<int32_t> rowU((size_t)std::max<int64_t>(S.nposU, 1), -1);
    for (size_t i = 0; i < S.posU.size(); ++i) rowU[(size_t)S.posU[i]] = (int32_t)i;
    DDMCHECK(upload(ctx, rowU.data(), (int64_t)rowU.size(), E->rowU));
  }
  HIPCHECK(ctx, E->ypos.alloc(S.nposL));
  HIPCHECK(ctx, E->xpos.alloc(S.nposU));
  HIPCHECK(ctx, dev_memset(E->ypos, 0, sizeof(double) * (size_t)std::max<int64_t>(S.nposL, 1)));
  HIPCHECK(ctx, dev_memset(E->xpos, 0, sizeof(double) * (size_t)std::max<int64_t>(S.nposU, 1)));
  const size_t pbytes = sizeof(unsigned long long) * 16 * std::max<size_t>(S.tasks.size(), 1);
  HIPCHECK(ctx, E->progress.alloc((int64_t)(pbytes / sizeof(unsigned long long))));
  HIPCHECK(ctx, dev_memset(E->progress, 0, pbytes));
  HIPCHECK(ctx, E->queue.alloc(32 * 4 * (int64_t)nb));
  HIPCHECK(ctx, dev_memset(E->queue, 0, sizeof(unsigned) * 32 * 4 * (size_t)nb));
  DDMCHECK(ilu0_alloc_xstate(ctx, F));
  HIPCHECK(ctx, hipFuncSetAttribute((const void *)k_trsv_pipe<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PIPE_LDS_BYTES));
  HIPCHECK(ctx, hipFuncSetAttribute((const void *)k_trsv_pipe<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PIPE_LDS_BYTES));
  int per_cu = 0;
  HIPCHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_trsv_pipe<false>, 64 * (PIPE_NC + PIPE_NL), PIPE_LDS_BYTES));
  per_cu = std::max(1, std::min(per_cu, 2));
  if (const char *e = std::getenv("DDM_PIPE_WG_PER_CU")) per_cu = std::max(1, std::min(per_cu, std::atoi(e)));
  E->grid = per_cu * (ctx->num_cu / 8 * 8);
  if (std::getenv("DDM_PIPE_VERBOSE")) {
    const pipe::Stats &st = S.stats;
    std::fprintf(stderr,
                 "[ddm] pipe schedule: %lld rows, tasks %lld+%lld, steps %lld+%lld (lane occupancy %.3f / %.3f), entries %lld: local %.3f self-global %.3f remote %.3f, "
                 "stream %.1f MB (%.2fx of 12 B/entry), max producers %lld, max steps %lld, regrouped %lld, levels <= %lld, rows/level <= %.0f, spread %d, grid %d\n",
                 (long long)st.rows, (long long)st.ntasks[0], (long long)st.ntasks[1], (long long)st.nsteps[0], (long long)st.nsteps[1],
                 (double)st.rows / (64.0 * std::max<int64_t>(st.nsteps[0], 1)), (double)st.rows / (64.0 * std::max<int64_t>(st.nsteps[1], 1)), (long long)st.entries,
                 (double)st.entries_local / std::max<int64_t>(st.entries, 1), (double)st.entries_self_global / std::max<int64_t>(st.entries, 1),
                 (double)st.entries_remote / std::max<int64_t>(st.entries, 1), S.stream.size() / 1e6, S.stream.size() / (12.0 * std::max<int64_t>(st.entries, 1)),
                 (long long)st.max_prod, (long long)st.max_steps, (long long)st.regrouped, (long long)st.max_levels, st.max_rows_per_level, E->spread, E->grid);
  }
  F->pipe = std::move(E);
  return DDM_OK;
}

static unsigned perm_grid(ddm_ctx *ctx, int64_t npos) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((npos + PERM_TILE - 1) / PERM_TILE, (int64_t)ctx->num_cu * 16)); }
static void enqueue_pipe(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, unsigned *err, unsigned long long *stamps, const double *scale = nullptr,
                         const double *add = nullptr)
{
  const PipeEngine &E = *F->pipe;
  PipeParams P;
  P.ngroups = E.ngroups;
  P.groups = E.groups;
  P.tasks = E.tasks;
  P.stream = E.stream;
  P.koff = E.koff;
  P.d = d;
  P.ypos = E.ypos;
  P.xpos = E.xpos;
  P.progress = E.progress;
  P.queue = E.queue;
  P.st = F->xstate;
  P.err = err;
  P.stamps = stamps;
  P.spread = E.spread;
  hipLaunchKernelGGL(k_pipe_prologue, dim3(1), dim3(64), 0, ctx->stream, F->xstate, E.queue, E.ngroups * 4);
  if (stamps) hipLaunchKernelGGL((k_trsv_pipe<true>), dim3(E.grid), dim3(64 * (PIPE_NC + PIPE_NL)), PIPE_LDS_BYTES, ctx->stream, P);
  else hipLaunchKernelGGL((k_trsv_pipe<false>), dim3(E.grid), dim3(64 * (PIPE_NC + PIPE_NL)), PIPE_LDS_BYTES, ctx->stream, P);
  hipLaunchKernelGGL(k_pipe_permute_out, dim3(perm_grid(ctx, E.nposU)), dim3(PERM_WG), 0, ctx->stream, E.nposU, E.rowU, (const double *)E.xpos, x, scale, add);
}

// ---- box engine (trsv_box_host.hpp / trsv_box.hpp) ----
// Box engine part (F->box); left null when the builder declines the matrix (settle_engine then hands it to pipe).
static int build_box_engine(ddm_ctx *ctx, ddm_ilu0 *F)
{
  const ddm_csr *A = F->A;
  const int nb = (int)F->h_block_ptr.size() - 1;
  const auto t0 = std::chrono::steady_clock::now();
  box::Schedule S;
  if (!box::build(A->nrows, A->h_rp.data(), A->h_ci.data(), F->h_lu.data(), F->h_diag.data(), nb, F->h_block_ptr.data(), S)) {
    if (std::getenv("DDM_PIPE_VERBOSE")) std::fprintf(stderr, "[ddm] box engine not applicable: %s\n", S.error.c_str());
    return DDM_OK;
  }
  auto X = std::make_unique<BoxEngine>();
  X->nblocks = nb;
  X->nshell = (int64_t)S.srow.size();
  X->nprod = (int64_t)S.ext_val.size();
  X->stats = S.stats;
  int rc = upload(ctx, S.blocks.data(), (int64_t)S.blocks.size(), X->blocks);
  if (!rc) rc = upload(ctx, S.steps.data(), (int64_t)S.steps.size(), X->steps);
  if (!rc) rc = upload(ctx, S.stream.data(), (int64_t)S.stream.size(), X->stream);
  if (!rc) rc = upload(ctx, (const unsigned long long *)S.einfo.data(), (int64_t)S.einfo.size(), X->einfo);
  if (!rc) rc = upload(ctx, S.ext_val.data(), X->nprod, X->ext_val);
  if (!rc) rc = upload(ctx, S.ext_col.data(), X->nprod, X->ext_col);
  if (!rc) rc = upload(ctx, S.srp.data(), (int64_t)S.srp.size(), X->srp);
  if (!rc) rc = upload(ctx, S.sci.data(), (int64_t)S.sci.size(), X->sci);
  if (!rc) rc = upload(ctx, S.sva.data(), (int64_t)S.sva.size(), X->sva);
  if (!rc) rc = upload(ctx, S.srow.data(), X->nshell, X->srow);
  if (rc) return rc;
  auto zalloc = [&](auto &buf, int64_t count) {
    count = std::max<int64_t>(count, 1);
    if (buf.alloc(count) != hipSuccess) return fail(ctx, DDM_EHIP, "box engine: allocation failed");
    if (dev_memset(buf, 0, sizeof(*buf.get()) * (size_t)count) != hipSuccess) return fail(ctx, DDM_EHIP, "box engine: memset failed");
    return DDM_OK;
  };
  rc = zalloc(X->E, X->nprod);
  if (!rc) rc = zalloc(X->xs, S.xs_len);
  if (!rc) rc = zalloc(X->prog, S.prog_len);
  if (!rc) rc = zalloc(X->queue, 32 * 2 * (int64_t)nb);
  if (!rc) rc = zalloc(X->ds, X->nshell);
  if (!rc) rc = zalloc(X->xsol, X->nshell);
  if (!rc) rc = ilu0_alloc_xstate(ctx, F);
  if (rc) return rc;
  if (X->nshell > 0) { // the rows behind the boxes: a factor object of their own with the general engines
    rc = csr_create_impl(ctx, X->nshell, X->nshell, S.frp.data(), S.fci.data(), S.fva.data(), /*host_only=*/true, &X->shell_csr);
    if (rc) return rc;
    ddm_ilu0 *G = new ddm_ilu0;
    X->shell = G;
    G->n = X->nshell;
    G->nnz = (int64_t)S.fci.size();
    hvec_copy(G->h_lu, S.fva.data(), S.fva.size());
    rc = ilu0_build_engines(ctx, G, X->shell_csr, S.fdiag, nb, S.fblock_ptr.data(), /*level kernels only=*/std::getenv("DDM_BOX_SHELL_LEVELS") != nullptr,
                            /*box_allowed=*/false);
    if (rc) return rc;
  }
  X->n = A->nrows;
  X->stream_len = (int64_t)S.stream.size();
  X->xs_len = S.xs_len;
  X->prog_len = S.prog_len;
  X->einfo_len = (int64_t)S.einfo.size();
  if (std::getenv("DDM_BOX_CHECK")) {
    if (hipHostMalloc((void **)&X->dbg, 8192, hipHostMallocMapped) != hipSuccess) return fail(ctx, DDM_EHIP, "box engine: allocation failed");
    std::memset(X->dbg, 0, 8192);
  }
  X->grid = 2 * (ctx->num_cu / 8 * 8);
  if (const char *e = std::getenv("DDM_BOX_GRID")) X->grid = std::max(8, std::atoi(e) / 8 * 8);
  if (std::getenv("DDM_PIPE_VERBOSE")) {
    const box::Block &B0 = S.blocks[0];
    std::fprintf(stderr, "[ddm] box engine: %d blocks, box rows %lld (block 0: %d x %d x %d, %d steps per plane), rows behind the boxes %lld (nested factor: %lld entries), "
                 "streams %.1f MB (%.2f B per factor entry of the boxes), shell products %lld, grid %d, built in %.2f s\n",
                 nb, (long long)S.stats.box_rows, B0.nx, B0.ny, B0.nz, B0.nsteps, (long long)X->nshell, (long long)S.fci.size(), S.stats.stream_bytes / 1e6,
                 (double)S.stats.stream_bytes / (27.0 * std::max<int64_t>(S.stats.box_rows, 1)), (long long)X->nprod, X->grid,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  F->box = std::move(X);
  return DDM_OK;
}
// ---- single right-hand side ---------------------------------------------------------------------
// joins the background build and builds what the settled engine still lacks (the single-vector solve and the box engine's nested
// factor): xcd2 schedules are built on first use
static int ilu0_prepare_engine(ddm_ctx *ctx, ddm_ilu0 *F)
{
  DDMCHECK(ilu0_join(ctx, F));
  if (F->engine == Engine::Box && F->box->shell) return ilu0_prepare_engine(ctx, F->box->shell);
  if (F->engine == Engine::Xcd2 && !F->xcd) return build_xcd_schedule(ctx, F);
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

static int ilu0_enqueue(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, const double *scale, const double *add, unsigned *err, bool *folded);
static int enqueue_box(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, const double *scale, const double *add, unsigned *err)
{
  BoxEngine *X = F->box.get();
  BoxParams P;
  P.nblocks = X->nblocks;
  P.blocks = X->blocks;
  P.steps = X->steps;
  P.stream = X->stream;
  P.einfo = X->einfo;
  P.E = X->E;
  P.xs = X->xs;
  P.prog = X->prog;
  P.queue = X->queue;
  P.st = F->xstate;
  P.err = err;
  P.spread = 0;
  if (const char *e = std::getenv("DDM_BOX_SPREAD")) P.spread = std::atoi(e);
  P.dbg = X->dbg;
  P.n = X->n;
  P.stream_len = X->stream_len;
  P.xs_len = X->xs_len;
  P.prog_len = X->prog_len;
  P.einfo_len = X->einfo_len;
  P.e_len = X->nprod;
  // forward sweep of the boxes: y into x
  P.rhs = d;
  P.out = x;
  P.scale = P.add = nullptr;
  int dbg = 0;   // diagnostic: DDM_BOX_DEBUG bit mask switches phases off (1 forward boxes, 2 nested solve, 4 products, 8 backward boxes, 16 shell rhs / out)
  if (const char *e = std::getenv("DDM_BOX_DEBUG")) dbg = std::atoi(e);
  hipLaunchKernelGGL(k_pipe_prologue, dim3(1), dim3(64), 0, ctx->stream, F->xstate, X->queue, X->nblocks * 2);
  hipLaunchKernelGGL(k_box_fill, dim3(grid_for(X->xs_len, WG, 4096)), dim3(WG), 0, ctx->stream, X->xs_len, (unsigned long long *)X->xs.get());   // "not written yet"
  if (!(dbg & 1)) hipLaunchKernelGGL((k_box_sweep<false>), dim3(X->grid), dim3(BOX_WG), 0, ctx->stream, P);
  if (X->nshell > 0 && !(dbg & 2)) {
    if (!(dbg & 16))
      hipLaunchKernelGGL(k_box_shell_rhs, dim3(grid_for(X->nshell)), dim3(WG), 0, ctx->stream, X->nshell, (const int64_t *)X->srp, (const int32_t *)X->sci, (const double *)X->sva,
                         (const int32_t *)X->srow, d, (const double *)x, X->ds);
    bool folded = false; // (nothing to fold: no scale / add)
    DDMCHECK(ilu0_enqueue(ctx, X->shell, X->ds, X->xsol, nullptr, nullptr, err, &folded)); // the nested solve reports into this factor's status word
  }
  // products of the box rows' shell entries, then the backward sweep of the boxes (with the level's tail) and the shell rows of x
  if (!(dbg & 4))
    hipLaunchKernelGGL(k_box_products, dim3(grid_for(X->nprod)), dim3(WG), 0, ctx->stream, X->nprod, (const double *)X->ext_val, (const int32_t *)X->ext_col, (const double *)X->xsol, X->E);
  P.rhs = x;
  P.scale = scale;
  P.add = add;
  hipLaunchKernelGGL(k_pipe_prologue, dim3(1), dim3(64), 0, ctx->stream, F->xstate, X->queue, X->nblocks * 2);
  hipLaunchKernelGGL(k_box_fill, dim3(grid_for(X->xs_len, WG, 4096)), dim3(WG), 0, ctx->stream, X->xs_len, (unsigned long long *)X->xs.get());
  if (!(dbg & 8)) hipLaunchKernelGGL((k_box_sweep<true>), dim3(X->grid), dim3(BOX_WG), 0, ctx->stream, P);
  if (X->nshell > 0 && !(dbg & 16))
    hipLaunchKernelGGL(k_box_shell_out, dim3(grid_for(X->nshell)), dim3(WG), 0, ctx->stream, X->nshell, (const int32_t *)X->srow, (const double *)X->xsol, x, scale, add);
  HIPCHECK(ctx, hipGetLastError());
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


// supernodal device factor: gather into the permuted work vector, solve in place on the panels, scatter; then the refinement steps
static void enqueue_sn(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, unsigned *err)
{
  const SnDirect &S = *F->sn;
  hipLaunchKernelGGL(k_perm_gather, dim3(grid_for(F->n)), dim3(WG), 0, ctx->stream, F->n, 1, S.f->d_perm, d, (int64_t)1, F->pd);
  sn::solve(*S.f, ctx->stream, 1, F->pd, 1, F->px, err); // (a time-out of the persistent top kernel lands in the status word)
  hipLaunchKernelGGL(k_perm_scatter, dim3(grid_for(F->n)), dim3(WG), 0, ctx->stream, F->n, 1, S.f->d_perm, (const double *)F->pd, x, (int64_t)1);
  for (int it = 0; it < S.refine_steps; ++it) { // x += A^-1 (d - A x)
    hipLaunchKernelGGL(k_residual_rowmajor, dim3((unsigned)((F->n + WG - 1) / WG)), dim3(WG), 0, ctx->stream, F->n, 1, (const int64_t *)S.ref_rp, (const int32_t *)S.ref_ci, (const double *)S.ref_va,
                       (const double *)x, (int64_t)1, d, (int64_t)1, S.pr, (int64_t)1);
    hipLaunchKernelGGL(k_perm_gather, dim3(grid_for(F->n)), dim3(WG), 0, ctx->stream, F->n, 1, S.f->d_perm, (const double *)S.pr, (int64_t)1, F->pd);
    sn::solve(*S.f, ctx->stream, 1, F->pd, 1, F->px, err);
    hipLaunchKernelGGL(k_perm_scatter_add, dim3(grid_for(F->n)), dim3(WG), 0, ctx->stream, F->n, 1, S.f->d_perm, (const double *)F->pd, x, (int64_t)1);
  }
}
// host sparse direct factor: the level solves in the fill-reducing order
static int enqueue_csr_direct(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x)
{
  const CsrDirect &C = *F->csr;
  hipLaunchKernelGGL(k_perm_gather, dim3(grid_for(F->n)), dim3(WG), 0, ctx->stream, F->n, 1, C.perm, d, (int64_t)1, F->pd);
  DDMCHECK(enqueue_tri_csr(ctx, C.Lb.nblocks ? C.Lb : C.Lc, false, F->pd, F->px));
  DDMCHECK(enqueue_tri_csr(ctx, C.Ub.nblocks ? C.Ub : C.Uc, true, F->pd, F->px));
  hipLaunchKernelGGL(k_perm_scatter, dim3(grid_for(F->n)), dim3(WG), 0, ctx->stream, F->n, 1, C.perm, (const double *)F->px, x, (int64_t)1);
  return DDM_OK;
}

// x = (LU)^-1 d on the settled engine (ilu0_prepare_engine); the single-launch kernels report time-outs into *err.  *folded: the
// engine applied x *= scale and x += add (either may be null) in its output pass (pipe, box); otherwise that is left to the caller.
static int ilu0_enqueue(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, const double *scale, const double *add, unsigned *err, bool *folded)
{
  *folded = F->engine == Engine::Box || F->engine == Engine::Pipe;
  switch (F->engine) {
  case Engine::Box: return enqueue_box(ctx, F, d, x, scale, add, err);
  case Engine::Pipe: enqueue_pipe(ctx, F, d, x, err, nullptr, scale, add); return DDM_OK;
  case Engine::Xcd2: enqueue_xcd2(ctx, F, d, x, err, nullptr); return DDM_OK;
  case Engine::Supernodal: enqueue_sn(ctx, F, d, x, err); return DDM_OK;
  case Engine::Levels: break;
  }
  if (F->csr) return enqueue_csr_direct(ctx, F, d, x);
  DDMCHECK(enqueue_tri(ctx, F->lev->L, false, d, x));
  return enqueue_tri(ctx, F->lev->U, true, d, x);
}

// Captures what enqueue() puts on the context's stream into `cache` (replacing the graph it held), then launches it.
template <class Enqueue>
static int capture_and_launch(ddm_ctx *ctx, GraphCache &cache, Enqueue &&enqueue)
{
  cache.reset();
  hipGraph_t g = nullptr;
  HIPCHECK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue();
  hipError_t e = hipStreamEndCapture(ctx->stream, &g);
  if (rc || e != hipSuccess) {
    if (g) (void)hipGraphDestroy(g);
    return rc ? rc : fail(ctx, DDM_EHIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
  }
  e = hipGraphInstantiate(&cache.exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) {
    cache.exec = nullptr;
    return fail(ctx, DDM_EHIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
  }
  HIPCHECK(ctx, hipGraphLaunch(cache.exec, ctx->stream));
  return DDM_OK;
}

// Diagnostic (not part of the product path): one solve with the loader engine and in-kernel cycle stamps of one
// compute wave.  out[0..5] = cycles waiting for the LDS tile, for the level flags, for the x gathers, for the
// store drain + flag; work items; total cycles (s_memtime ticks, 100 MHz constant clock on gfx9).
extern "C" int ddm_ilu0_debug_stamps(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, unsigned long long *out_host)
{
  dbuf<unsigned long long> st;
  HIPCHECK(ctx, st.alloc(8));
  HIPCHECK(ctx, hipMemset(st, 0, 64));
  DDMCHECK(ilu0_join(ctx, F));
  if (!F->xcd) DDMCHECK(build_xcd_schedule(ctx, F));
  enqueue_xcd2(ctx, F, d, x, F->err, st);
  return ddm_memcpy_d2h(ctx, out_host, st, 48);
}

// Diagnostic (not part of the product path): one solve with the stamped build of the pipe kernel.  Per task 8 words
// (layout: trsv_pipe.hpp, STAMP) followed by nothing; returns the number of tasks in *ntasks.  out_host may be null
// to query the size.  Also reports group / sweep of every task in meta_host[2 * ntasks] when given.
extern "C" int ddm_ilu0_pipe_trace(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, unsigned long long *out_host, int32_t *meta_host,
                                   int64_t capacity_tasks, int64_t *ntasks)
{
  if (!F || !ntasks) return fail(ctx, DDM_EINVAL, "ddm_ilu0_pipe_trace: bad arguments");
  DDMCHECK(ilu0_join(ctx, F));
  if (!F->pipe) DDMCHECK(build_pipe_schedule(ctx, F));
  if (!F->pipe) return fail(ctx, DDM_EINVAL, "pipe engine not applicable to this matrix");
  const int64_t nt = F->pipe->stats.ntasks[0] + F->pipe->stats.ntasks[1];
  *ntasks = nt;
  if (!out_host) return DDM_OK;
  if (capacity_tasks < nt || !d || !x || d == x) return fail(ctx, DDM_EINVAL, "ddm_ilu0_pipe_trace: bad arguments");
  dbuf<unsigned long long> st;
  HIPCHECK(ctx, st.alloc(PIPE_STAMP_WORDS * (nt + 1)));
  HIPCHECK(ctx, hipMemsetAsync(st, 0, sizeof(unsigned long long) * PIPE_STAMP_WORDS * (size_t)(nt + 1), ctx->stream));
  enqueue_pipe(ctx, F, d, x, F->err, st);
  int rc = ddm_memcpy_d2h(ctx, out_host, st, (int64_t)sizeof(unsigned long long) * PIPE_STAMP_WORDS * nt);
  if (!rc && meta_host) {
    std::vector<pipe::Task> tasks((size_t)nt);
    rc = ddm_memcpy_d2h(ctx, tasks.data(), F->pipe->tasks, (int64_t)sizeof(pipe::Task) * nt);
    for (int64_t t = 0; t < nt && !rc; ++t) {
      meta_host[2 * t] = tasks[(size_t)t].group;
      meta_host[2 * t + 1] = tasks[(size_t)t].sweep;
    }
  }
  return rc;
}

// x = (LU)^-1 d, then optionally x *= scale and x += add (the tail of the Schwarz level: partition of unity of the restricted
// variant and the coarse correction); the pipe and box engines fold both into their output pass, the others append the two kernels.
static int ilu0_solve_epilogue(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x, const double *scale, const double *add)
{
  if (F && F->n == 0) return DDM_OK;
  if (!F || !d || !x || d == x) return fail(ctx, DDM_EINVAL, "ddm_ilu0_solve: bad arguments (d and x must not alias)");
  if (F->graph.exec && F->g_d == d && F->g_x == x && F->g_scale == scale && F->g_add == add) {
    HIPCHECK(ctx, hipGraphLaunch(F->graph.exec, ctx->stream));
    return DDM_OK;
  }
  // (re)capture the ~2*nlev launches into a graph bound to this (d, x) pair
  F->graph.reset();
  if (F->sn && !sn::reserve(*F->sn->f, 1)) return fail(ctx, DDM_EHIP, "sparse direct solver: allocation failed");
  DDMCHECK(ilu0_prepare_engine(ctx, F));
  F->g_d = d;
  F->g_x = x;
  F->g_scale = scale;
  F->g_add = add;
  return capture_and_launch(ctx, F->graph, [&]() {
    bool folded = false;
    const int rc = ilu0_enqueue(ctx, F, d, x, scale, add, F->err, &folded);
    if (!folded) {
      if (scale) hipLaunchKernelGGL(k_scale, dim3(grid_for(F->n)), dim3(WG), 0, ctx->stream, F->n, scale, x);
      if (add) hipLaunchKernelGGL(k_axpy, dim3(grid_for(F->n)), dim3(WG), 0, ctx->stream, F->n, 1.0, add, x);
    }
    return rc;
  });
}

extern "C" int ddm_ilu0_solve(ddm_ctx *ctx, ddm_ilu0 *F, const double *d, double *x) { return ilu0_solve_epilogue(ctx, F, d, x, nullptr, nullptr); }

// Multi-RHS solve X = (LU)^-1 D for row-major n x nrhs block vectors with leading dimensions ldd / ldx (GenEO setup path).
// One launch per level (wide levels of direct factors: one workgroup per row); the launches of one (D, X, nrhs) combination are
// captured into a HIP graph on first use and replayed afterwards (the block eigensolver calls with the same buffers every iteration).
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
static int ilu0_solve_multi_ld(ddm_ctx *ctx, ddm_ilu0 *F, int nrhs, const double *D, int64_t ldd, double *X, int64_t ldx, bool f32 = false)
{
  if (!F || !D || !X || D == X || nrhs < 1 || ldd < nrhs || ldx < nrhs) return fail(ctx, DDM_EINVAL, "ddm_ilu0_solve_multi: bad arguments");
  if (F->n == 0) return DDM_OK;
  // single precision only for plain ILU(0) factors on aligned blocks of a multiple of 4 columns without wide levels
  f32 = f32 && F->lev && nrhs % 4 == 0 && ldd % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)D & 31) == 0 && ((uintptr_t)X & 31) == 0;
  if (f32)
    for (const TriSchedule *S : {&F->lev->L, &F->lev->U})
      for (const LevelDesc &L : S->desc) f32 = f32 && L.w < 96;
  if (F->mgraph.exec && F->mg_D == D && F->mg_X == X && F->mg_nrhs == nrhs && F->mg_ldd == ldd && F->mg_ldx == ldx && F->mg_f32 == f32) {
    HIPCHECK(ctx, hipGraphLaunch(F->mgraph.exec, ctx->stream));
    return DDM_OK;
  }
  if (f32) {
    LevelEngine &E = *F->lev;
    for (TriSchedule *S : {&E.L, &E.U}) {
      if (!S->vals_f32 && S->ell_entries > 0) {
        HIPCHECK(ctx, S->vals_f32.alloc(S->ell_entries));
        hipLaunchKernelGGL(k_to_float, dim3((unsigned)((S->ell_entries + 255) / 256)), dim3(256), 0, ctx->stream, S->ell_entries, (const double *)S->vals, S->vals_f32);
      }
      if (S == &E.U && !S->dinv_f32) {
        HIPCHECK(ctx, S->dinv_f32.alloc(F->n));
        hipLaunchKernelGGL(k_to_float, dim3((unsigned)((F->n + 255) / 256)), dim3(256), 0, ctx->stream, F->n, (const double *)S->dinv, S->dinv_f32);
      }
    }
    HIPCHECK(ctx, reserve_cols(E.xf_nrhs, nrhs, E.xf, F->n));
    HIPCHECK(ctx, hipGetLastError());
  }
  F->mgraph.reset();
  if (F->sn) {
    SnDirect &S = *F->sn;
    const int w = std::min(nrhs, 48); // the panel kernels take up to 48 columns: wider blocks are solved in column panels
    const double *partial_before = S.f->d_partial, *contrib_before = S.f->d_contrib;
    if (!sn::reserve(*S.f, w)) return fail(ctx, DDM_EHIP, "sparse direct solver: allocation failed");
    if (S.f->d_partial != partial_before || S.f->d_contrib != contrib_before) F->graph.reset(); // the single-vector graph's nodes hold the old scratch pointers
    HIPCHECK(ctx, reserve_cols(F->pm_nrhs, w, F->pD, F->n));
    if (S.refine_steps > 0 && S.pr_cols < w) {
      HIPCHECK(ctx, reserve_cols(S.pr_cols, w, S.pr, F->n));
      F->graph.reset(); // (the single-vector graph holds the old residual buffer)
    }
  }
  if (F->csr) HIPCHECK(ctx, reserve_cols<double>(F->pm_nrhs, nrhs, {{F->pX, F->n + F->csr->nvirt}, {F->pD, F->n}}));
  F->mg_D = D;
  F->mg_X = X;
  F->mg_nrhs = nrhs;
  F->mg_ldd = ldd;
  F->mg_ldx = ldx;
  F->mg_f32 = f32;
  return capture_and_launch(ctx, F->mgraph, [&]() {
    if (F->sn) {
      const SnDirect &S = *F->sn;
      for (int c0 = 0; c0 < nrhs; c0 += 48) {
        const int w = std::min(48, nrhs - c0);
        hipLaunchKernelGGL(k_perm_gather, dim3(grid_for(F->n * w)), dim3(WG), 0, ctx->stream, F->n, w, S.f->d_perm, D + c0, ldd, F->pD);
        sn::solve(*S.f, ctx->stream, w, F->pD, w);
        hipLaunchKernelGGL(k_perm_scatter, dim3(grid_for(F->n * w)), dim3(WG), 0, ctx->stream, F->n, w, S.f->d_perm, (const double *)F->pD, X + c0, ldx);
        for (int it = 0; it < S.refine_steps; ++it) { // X += A^-1 (D - A X), panel by panel
          hipLaunchKernelGGL(k_residual_rowmajor, dim3((unsigned)((F->n * (int64_t)w + WG - 1) / WG)), dim3(WG), 0, ctx->stream, F->n, w, (const int64_t *)S.ref_rp, (const int32_t *)S.ref_ci,
                             (const double *)S.ref_va, (const double *)(X + c0), ldx, D + c0, ldd, S.pr, (int64_t)w);
          hipLaunchKernelGGL(k_perm_gather, dim3(grid_for(F->n * w)), dim3(WG), 0, ctx->stream, F->n, w, S.f->d_perm, (const double *)S.pr, (int64_t)w, F->pD);
          sn::solve(*S.f, ctx->stream, w, F->pD, w);
          hipLaunchKernelGGL(k_perm_scatter_add, dim3(grid_for(F->n * w)), dim3(WG), 0, ctx->stream, F->n, w, S.f->d_perm, (const double *)F->pD, X + c0, ldx);
        }
      }
    } else if (F->csr) { // sparse direct factor: solve in the fill-reducing order on packed work blocks
      const CsrDirect &C = *F->csr;
      hipLaunchKernelGGL(k_perm_gather, dim3(grid_for(F->n * nrhs)), dim3(WG), 0, ctx->stream, F->n, nrhs, C.perm, D, ldd, F->pD);
      enqueue_multi_levels_csr(ctx, C.Lc, false, nrhs, F->pD, nrhs, F->pX, nrhs);
      enqueue_multi_levels_csr(ctx, C.Uc, true, nrhs, F->pD, nrhs, F->pX, nrhs);
      hipLaunchKernelGGL(k_perm_scatter, dim3(grid_for(F->n * nrhs)), dim3(WG), 0, ctx->stream, F->n, nrhs, C.perm, (const double *)F->pX, X, ldx);
    } else if (f32) {
      // (Splitting the columns into two halves that run as two parallel chains of the captured graph -- a second stream joining the
      //  capture -- was measured and is slower: 6.8 against 5.6 s for the 109 block iterations of the headline GenEO run; every level
      //  kernel is latency-bound, so two half-width kernels cost two full ones and the chains do not overlap enough to pay for that.)
      enqueue_multi_levels_f32(*F->lev, ctx->stream, nrhs, 0, nrhs, D, ldd, X, ldx);
    } else {
      enqueue_multi_levels(ctx, *F->lev, nrhs, D, ldd, X, ldx);
    }
    return DDM_OK;
  });
}
extern "C" int ddm_ilu0_solve_multi(ddm_ctx *ctx, ddm_ilu0 *F, int nrhs, const double *D, double *X) { return ilu0_solve_multi_ld(ctx, F, nrhs, D, nrhs, X, nrhs); }
// the same solve with SINGLE-PRECISION sweeps (factor entries and work block in float, D read and X written in double): preconditioner
// grade -- what the GenEO block iteration applies.  Falls back to the double sweeps when nrhs is not a multiple of 4 or F is a sparse
// direct factor.
extern "C" int ddm_ilu0_solve_multi_f32(ddm_ctx *ctx, ddm_ilu0 *F, int nrhs, const double *D, double *X) { return ilu0_solve_multi_ld(ctx, F, nrhs, D, nrhs, X, nrhs, true); }
