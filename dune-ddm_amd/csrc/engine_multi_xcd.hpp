// Engine `xcd` of the block solve of a plain ILU(0) factor (kernel: k_trsv_multi_xcd in kernels.hpp; plan: trsv_multi_plan.hpp, built
// with the level schedules in tri_levels.hpp): both sweeps of all diagonal blocks in ONE persistent launch on the level engine's own
// arrays, bit for bit the level launches.  Opt-in (ddm_ilu0_set_multi_engine, DDM_TRSV_MULTI_MODE); what it needs besides the level
// engine -- flags and a report, no factor memory -- is built by the first solve that takes it.  Needs local_factor.hpp.

// the requested engine at creation: DDM_TRSV_MULTI_MODE = levels (the default; also any other value) | xcd
static int requested_multi_mode()
{
  const char *m = std::getenv("DDM_TRSV_MULTI_MODE");
  return m && !std::strcmp(m, "xcd") ? MULTI_XCD : MULTI_LEVELS;
}

// whether ilu0_solve_multi_ld runs this block solve on engine `xcd`; *why: MULTI_RAN_REQUESTED or the reason it runs what it ran before
static bool multi_xcd_applies(const ddm_ilu0 *F, int *why)
{
  *why = MULTI_RAN_REQUESTED;
  if (F->csr || F->sn || !F->lev) *why = MULTI_DIRECT_FACTOR;
  else if (F->multi_mode == MULTI_LEVELS) *why = MULTI_NOT_REQUESTED;
  else
    for (const TriSchedule *S : {&F->lev->L, &F->lev->U})
      for (const LevelDesc &L : S->desc)
        if (L.w >= 96) *why = MULTI_WIDE_LEVEL; // that level takes k_trsv_level_multi_wide, which sums in another order
  return *why == MULTI_RAN_REQUESTED;
}

// flags, report words and the ticket state (allocations: before the capture of the solve)
static int build_multi_xcd(ddm_ctx *ctx, ddm_ilu0 *F)
{
  LevelEngine &E = *F->lev;
  if (E.mx) return DDM_OK;
  auto M = std::make_unique<MultiXcdSync>();
  M->grid = persistent_grid(ctx);
  const int64_t words = (int64_t)MULTI_XCD_TEAMS * M->grid * MULTI_XCD_FLAG_STRIDE;
  HIPCHECK(ctx, M->flags.alloc(words));
  HIPCHECK(ctx, dev_memset(M->flags, 0, sizeof(unsigned long long) * (size_t)words));
  if (hipHostMalloc((void **)&M->report, 64, hipHostMallocMapped) != hipSuccess) return fail(ctx, DDM_EHIP, "local solver: allocation failed");
  std::memset(M->report, 0, 64);
  DDMCHECK(ilu0_alloc_xstate(ctx, F));
  E.mx = std::move(M);
  return DDM_OK;
}

template <class T>
static MultiXcdTri<T> multi_xcd_view(const TriSchedule &S)
{
  MultiXcdTri<T> V;
  V.desc = S.d_desc, V.rows = S.rows, V.cols = S.cols, V.blk_off = S.blk_off, V.blk_nlev = S.blk_nlev;
  if constexpr (sizeof(T) == 8) V.vals = S.vals, V.dinv = S.dinv;
  else V.vals = S.vals_f32, V.dinv = S.dinv_f32;
  return V;
}

// quad: the predicate of enqueue_multi_levels (always true for f32: ilu0_solve_multi_ld checked it)
static void enqueue_multi_xcd(ddm_ctx *ctx, const ddm_ilu0 *F, int mode, bool f32, int nrhs, const double *D, int64_t ldd, double *X, int64_t ldx)
{
  const LevelEngine &E = *F->lev;
  const MultiXcdSync &M = *E.mx;
  hipLaunchKernelGGL(k_trsv_xcd_prologue, dim3(1), dim3(64), 0, ctx->stream, F->xstate);
  auto args = [&](auto *x, int64_t ld) {
    typedef std::remove_pointer_t<decltype(x)> T;
    MultiXcdArgs<T> A;
    A.nb = (int)F->h_block_ptr.size() - 1, A.nrhs = nrhs, A.force_one = mode == MULTI_XCD_ONE_TEAM, A.slots = M.grid;
    A.tri[0] = multi_xcd_view<T>(E.L), A.tri[1] = multi_xcd_view<T>(E.U);
    A.D = D, A.ldd = ldd, A.X = x, A.ldx = ld, A.xout = X, A.ldo = ldx;
    A.st = F->xstate, A.flags = M.flags, A.err = F->err, A.report = M.report;
    return A;
  };
  const dim3 grid((unsigned)M.grid), block(WG);
  if (f32) {
    hipLaunchKernelGGL((k_trsv_multi_xcd<float, true>), grid, block, 0, ctx->stream, args((float *)E.xf, (int64_t)nrhs));
    return;
  }
  const bool quad = nrhs % 4 == 0 && ldd % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)D & 31) == 0 && ((uintptr_t)X & 31) == 0;
  if (quad) hipLaunchKernelGGL((k_trsv_multi_xcd<double, true>), grid, block, 0, ctx->stream, args(X, ldx));
  else hipLaunchKernelGGL((k_trsv_multi_xcd<double, false>), grid, block, 0, ctx->stream, args(X, ldx));
}

// ---- C ABI ----
static int ilu0_set_multi_mode(ddm_ilu0 *F, int mode)
{
  if (!F || mode < MULTI_LEVELS || mode > MULTI_XCD_ONE_TEAM) return DDM_EINVAL;
  if (F->csr || F->sn || !F->lev) return DDM_OK; // direct factors have one block solve
  if (mode != F->multi_mode) F->mgraph.reset();
  F->multi_mode = mode;
  return DDM_OK;
}
extern "C" int ddm_ilu0_set_multi_engine(ddm_ctx *ctx, ddm_ilu0 *F, int mode)
{
  const int rc = ilu0_set_multi_mode(F, mode);
  return rc ? fail(ctx, rc, "ddm_ilu0_set_multi_engine: bad arguments (mode: 0 = levels, 1 = xcd, 2 = xcd with one team)") : DDM_OK;
}
// out[0] requested mode, [1] engine of the last block solve (-1: none yet; 0 levels, 1 xcd), [2] why xcd was not taken (0: it was; 1 not
// requested, 2 direct factor, 3 a level of w >= 96), then for the last xcd launch [3] grid, [4] teams, [5] one-team flag, [6..13]
// workgroups per XCD.  The kernel writes [4..13]: synchronise the stream first.
extern "C" int ddm_ilu0_multi_info(const ddm_ilu0 *F, int64_t *out, int64_t cap, int64_t *count)
{
  if (!F || !count) return DDM_EINVAL;
  *count = 14;
  if (!out) return DDM_OK;
  if (cap < 14) return DDM_EINVAL;
  for (int k = 0; k < 14; ++k) out[k] = 0;
  int why;
  (void)multi_xcd_applies(F, &why);
  out[0] = F->multi_mode, out[1] = F->multi_last, out[2] = F->multi_last < 0 ? why : F->multi_decline;
  if (F->lev && F->lev->mx) {
    const MultiXcdSync &M = *F->lev->mx;
    out[3] = M.grid, out[4] = ((volatile unsigned *)M.report)[8], out[5] = ((volatile unsigned *)M.report)[9];
    for (int x = 0; x < 8; ++x) out[6 + x] = ((volatile unsigned *)M.report)[x];
  }
  return DDM_OK;
}
// levels, per-block sub-ranges and per-block level counts of one triangle of a CSR pattern with sorted rows and a full diagonal, as
// build_schedule computes them (trsv_multi_plan.hpp).  *nlev is always set; off[(nlev) (nblocks + 1)] and blk_nlev[nblocks] are
// filled when off is given and cap holds them.  Host only, no device needed.
extern "C" int ddm_trsv_multi_plan_host(int64_t n, const int64_t *rp, const int32_t *ci, int64_t nblocks, const int64_t *block_ptr, int upper, int32_t *off, int64_t cap,
                                        int32_t *blk_nlev, int64_t *nlev)
{
  if (n < 0 || !rp || (n > 0 && !ci) || nblocks < 1 || !block_ptr || !nlev || block_ptr[0] != 0 || block_ptr[nblocks] != n || (off && !blk_nlev)) return DDM_EINVAL;
  for (int64_t b = 0; b < nblocks; ++b)
    if (block_ptr[b] > block_ptr[b + 1]) return DDM_EINVAL;
  std::vector<int64_t> diag((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    if (rp[i] > rp[i + 1] || (i == 0 && rp[0] != 0)) return DDM_EINVAL;
    int64_t dg = -1;
    for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
      if (ci[k] < 0 || ci[k] >= n || (k > rp[i] && ci[k] <= ci[k - 1])) return DDM_EINVAL;
      if (ci[k] == i) dg = k;
    }
    if (dg < 0) return DDM_EINVAL;
    diag[(size_t)i] = dg;
  }
  std::vector<int32_t> level((size_t)n, 0), o, bn;
  *nlev = (int64_t)multi_xcd::tri_levels(n, rp, ci, diag.data(), upper != 0, level.data()) + 1;
  if (!off) return DDM_OK;
  if (cap < *nlev * (nblocks + 1)) return DDM_EINVAL;
  multi_xcd::plan_tables(*nlev, nblocks, block_ptr, level.data(), o, bn);
  std::copy(o.begin(), o.end(), off);
  std::copy(bn.begin(), bn.end(), blk_nlev);
  return DDM_OK;
}
// the team arithmetic of k_trsv_multi_xcd for one workgroup (tests): out = {teams, team, rank, size, one-team flag}
extern "C" int ddm_trsv_multi_team_host(const uint32_t *tickets8, int nblocks, int force_one, int xcc, uint32_t xcd_ticket, uint32_t global_ticket, uint32_t grid, int32_t *out5)
{
  if (!tickets8 || !out5 || nblocks < 1 || xcc < 0 || xcc > 7) return DDM_EINVAL;
  const multi_xcd::Team t = multi_xcd::team_of(tickets8, nblocks, force_one, (unsigned)xcc, xcd_ticket, global_ticket, grid);
  out5[0] = t.nteams, out5[1] = t.team, out5[2] = t.rank, out5[3] = t.size, out5[4] = t.one;
  return DDM_OK;
}
