// Creation of the local solver's factors (the last of the local-solver files; local_factor.hpp names them all and the entry points the
// rest of the library may use): ILU(0) on the host, the host sparse Cholesky / L U, the supernodal factor on the device with its
// refinement probe, and the small query exports.  Needs local_solve.hpp (the probe solves) and the engine builders.

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

// Level schedules of an ILU(0) factor (values F->h_lu in the pattern of A), its status words, and the pipe or box part it asks for
// (in the background).
static int ilu0_build_engines(ddm_ctx *ctx, ddm_ilu0 *F, const ddm_csr *A, const std::vector<int64_t> &diag, int64_t nblocks, const int64_t *block_ptr,
                              bool multi_rhs_only, bool box_allowed)
{
  F->engine = requested_engine(multi_rhs_only, box_allowed);
  F->multi_mode = requested_multi_mode();
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
    rcU = build_schedule(ctx, A, F->h_lu, diag, true, F->h_block_ptr, F->lev->U);
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
  int rc = build_schedule(ctx, A, F->h_lu, diag, false, F->h_block_ptr, F->lev->L);
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
// Supernodal Cholesky on the device.  Returns DDM_OK / an error code, or 1 when the factorisation is too small to be worth it and
// force == false (the caller then takes the host path).
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
  F->A = A; // (not owned, as for ILU(0) factors: read again by a value refresh only, sn_refresh.hpp)
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
extern "C" int ddm_chol_create(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, double max_flops, ddm_ilu0 **out)
{
  return ddm_direct_create(ctx, A, nblocks, block_ptr, 0, max_flops, out);
}
extern "C" int ddm_direct_create(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, int general, double max_flops, ddm_ilu0 **out)
{
  return direct_create_impl(ctx, A, nblocks, block_ptr, general, max_flops, false, out);
}
extern "C" int ddm_ilu0_wait(ddm_ctx *ctx, ddm_ilu0 *F) { return F ? ilu0_join(ctx, F) : fail(ctx, DDM_EINVAL, "ddm_ilu0_wait: bad arguments"); }
extern "C" int ddm_ilu0_is_direct(const ddm_ilu0 *F) { return F && (F->csr || F->sn) ? 1 : 0; }
extern "C" int ddm_ilu0_refinement(const ddm_ilu0 *F, double *omega)
{
  if (!F) return 0;
  if (omega)
    for (int k = 0; k < 5; ++k) omega[k] = F->sn ? F->sn->refine_omega[k] : 0.0;
  return F->sn ? F->sn->refine_steps : 0;
}
// the row order k_sn_lu_diag chose, read-only (tests): out_n[first[s] + k] = block-local row of supernode s that ended in position k
extern "C" int ddm_ilu0_sn_pivots(ddm_ctx *ctx, const ddm_ilu0 *F, int32_t *out_n)
{
  if (!ctx || !F || !out_n || !F->sn || !F->sn->f || !F->sn->f->lu) return fail(ctx, DDM_EINVAL, "ddm_ilu0_sn_pivots: not a device L U factor");
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (F->n > 0) HIPCHECK(ctx, hipMemcpy(out_n, F->sn->f->d_piv, sizeof(int32_t) * (size_t)F->n, hipMemcpyDeviceToHost));
  return DDM_OK;
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
  DDMCHECK(ilu0_sync_host_factor(ctx, const_cast<ddm_ilu0 *>(F))); // (after ddm_ilu0_refresh the factor is on the device)
  std::memcpy(lu_host, F->h_lu.data(), sizeof(double) * (size_t)F->nnz);
  return DDM_OK;
}
