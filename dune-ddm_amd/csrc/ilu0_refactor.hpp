// Value refresh of an ILU(0) factor (Refactor: local_factor.hpp; C ABI: ddm_ilu0_refresh): the numeric factorisation on the device
// and the scatter of the new factor into the engines' layouts.  Same pattern, same schedules, new values; the result is bit for bit
// what ddm_ilu0_create makes of the new values.  Needs local_factor.hpp, tri_levels.hpp, engine_xcd2.hpp, engine_pipe.hpp.
//
// What a refresh does to each part of the factor:
//   * LevelEngine (every factor has it): `vals` / `dinv` of both triangles are rewritten IN PLACE, the single-precision copies are
//     reconverted in place where they exist.  Every buffer keeps its address, so the captured graphs (F->graph of the `levels`
//     engine, F->mgraph) stay valid and are kept.
//   * PipeEngine: the value slots and the s0 slots of the tile stream are rewritten in place; F->graph stays valid.
//   * XcdEngine: a built part is DROPPED (and F->graph with it when xcd2 is the settled engine); the next solve rebuilds it from
//     the refreshed h_lu, as the first solve after creation builds it.
//   * the host-engine direct factor (F->csr) and the box engine are refused (DDM_ENOTIMPL, nothing touched): the caller creates a
//     new factor.  The device supernodal factor (F->sn) is refreshed by sn_refresh.hpp.
//   * h_lu is brought up to date when it is next read (ilu0_sync_host_factor).
// The factorisation writes a scratch array; the engines are touched only after the status word has come back clean, so a vanishing
// pivot (DDM_ENUMERIC) leaves the previous factor in place everywhere.
// Everything here runs on the CALLER's thread and on the context's stream, after the background builder has been joined: no helper
// thread uploads, so there is nothing that needs a BackgroundTransfers (context.hpp); a refresh is not meant to be captured.

// ---- numeric factorisation ------------------------------------------------------------------------
// ilu0_factor_block (local_solver.hpp) on the device: IKJ inside the pattern, multipliers in L, the inverse pivot on the diagonal.
// Row i needs exactly the rows of its L pattern, so the L level schedule is the schedule: one launch per level, one workgroup
// looping over a run of levels of a few rows (Refactor::plan); no workgroup waits for another.  One wave per row: the eliminations
// run over k in ascending column order, the lanes take the U entries of row k and look their column up in row i (binary search);
// every entry is updated by one multiplication followed by one subtraction (-ffp-contract=off), as on the host.  Row i sits in LDS
// while it is eliminated when it has at most REFAC_LDS_ROW entries, in the scratch array in global memory otherwise.
constexpr int REFAC_LDS_ROW = 512;
constexpr int REFAC_WAVES = 4;        // waves (rows) per workgroup of the one-level kernel
constexpr int REFAC_SMALL_WAVES = 8;  // ... of the kernel that loops over small levels
constexpr int REFAC_SMALL_ROWS = 16;  // a level of at most this many rows is "small": two rows per wave cost about what a launch costs
constexpr unsigned REFAC_OK = 0xffffffffu;

// orders the wave's own accesses to row i between two elimination steps (other lanes wrote entries this lane reads next)
template <bool LDS>
__device__ __forceinline__ void refac_wave_sync()
{
  if (LDS) { // LDS operations of one wave execute in order: only the compiler has to keep them in place
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
}
// position of column j in cols[lo, hi) (ascending), or hi
template <class Cols>
__device__ __forceinline__ int refac_find(const Cols &cols, int lo, int hi, int32_t j)
{
  const int end = hi;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cols(mid) < j) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && cols(lo) == j ? lo : end;
}
template <bool LDS>
__device__ void refac_eliminate(int lane, int64_t p0, int len, int nl, const int32_t *__restrict__ ci, const int64_t *__restrict__ rp, const int64_t *__restrict__ diag,
                                double *lu, double *srow, const int32_t *scol)
{
  double *row = LDS ? srow : lu + p0;
  auto cols = [&](int e) { return LDS ? scol[e] : ci[p0 + e]; };
  for (int e = 0; e < nl; ++e) { // the L entries of row i, ascending columns
    const int32_t k = cols(e);
    const int64_t dk = diag[k];
    const double lik = row[e] * lu[dk]; // (row k is final: an earlier level)
    refac_wave_sync<LDS>();             // every lane has read row[e]
    if (lane == 0) row[e] = lik;
    const int64_t u1 = rp[k + 1];
    for (int64_t pk = dk + 1 + lane; pk < u1; pk += 64) {
      const int pos = refac_find(cols, e + 1, len, ci[pk]);
      if (pos < len) {
        const double prod = lik * lu[pk];
        row[pos] = row[pos] - prod;
      }
    }
    refac_wave_sync<LDS>();
  }
}
// one row by one wave; srow / scol: the wave's REFAC_LDS_ROW entries of LDS
__device__ void refac_row(int64_t i, int lane, const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const double *__restrict__ va,
                          const int64_t *__restrict__ diag, double *lu, unsigned *status, double *srow, int32_t *scol)
{
  // a pivot has failed: stop eliminating (one answer for the whole wave)
  if ((unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != REFAC_OK) return;
  const int64_t p0 = rp[i];
  const int len = (int)(rp[i + 1] - p0), nl = (int)(diag[i] - p0);
  const bool in_lds = len <= REFAC_LDS_ROW;
  if (in_lds) {
    for (int e = lane; e < len; e += 64) {
      srow[e] = va[p0 + e];
      scol[e] = ci[p0 + e];
    }
    refac_wave_sync<true>();
    refac_eliminate<true>(lane, p0, len, nl, ci, rp, diag, lu, srow, scol);
  } else {
    for (int e = lane; e < len; e += 64) lu[p0 + e] = va[p0 + e];
    refac_wave_sync<false>();
    refac_eliminate<false>(lane, p0, len, nl, ci, rp, diag, lu, srow, scol);
  }
  const double piv = in_lds ? srow[nl] : lu[p0 + nl];
  const bool bad = !(piv != 0.0) || !(fabs(piv) <= 1.7976931348623157e308); // zero, NaN or infinite
  if (bad) {
    if (lane == 0) atomicMin(status, (unsigned)i); // the first such row: the host names its block
    return;                                        // (nothing is divided, the row stays unfinished in the scratch array)
  }
  const double inv = 1.0 / piv;
  if (in_lds) {
    refac_wave_sync<true>();
    for (int e = lane; e < len; e += 64) lu[p0 + e] = e == nl ? inv : srow[e];
  } else if (lane == 0)
    lu[p0 + nl] = inv;
}
__global__ __launch_bounds__(64 * REFAC_WAVES) void k_ilu0_refactor_level(int m, const int32_t *__restrict__ rows, const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                                         const double *__restrict__ va, const int64_t *__restrict__ diag, double *lu, unsigned *status)
{
  __shared__ double srow[REFAC_WAVES][REFAC_LDS_ROW];
  __shared__ int32_t scol[REFAC_WAVES][REFAC_LDS_ROW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * REFAC_WAVES + wave;
  if (r < m) refac_row(rows[r], lane, rp, ci, va, diag, lu, status, srow[wave], scol[wave]);
}
// one workgroup, levels [0, nlev) of desc one after the other (each level reads what the levels before it wrote: workgroup barrier)
__global__ __launch_bounds__(64 * REFAC_SMALL_WAVES) void k_ilu0_refactor_small_levels(int nlev, const LevelDesc *__restrict__ desc, const int32_t *__restrict__ rows,
                                                                                      const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const double *__restrict__ va,
                                                                                      const int64_t *__restrict__ diag, double *lu, unsigned *status)
{
  __shared__ double srow[REFAC_SMALL_WAVES][REFAC_LDS_ROW];
  __shared__ int32_t scol[REFAC_SMALL_WAVES][REFAC_LDS_ROW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int l = 0; l < nlev; ++l) {
    const LevelDesc L = desc[l];
    for (int r = wave; r < L.m; r += REFAC_SMALL_WAVES) refac_row(rows[L.row_off + r], lane, rp, ci, va, diag, lu, status, srow[wave], scol[wave]);
    __syncthreads(); // workgroup-scope release / acquire of the rows just written (k_trsv_small_levels relies on the same)
  }
}

// ---- scatter into the engines' layouts ------------------------------------------------------------
// Sliced ELL of one triangle (build_schedule): one thread per stored entry t; its level by bisection over the levels' ent_off, then
// k = (t - ent_off) / m, r = (t - ent_off) % m, row = rows[row_off + r]: vals[t] = entry k of the row's triangle, 0.0 in the padding.
template <bool UPPER>
__global__ __launch_bounds__(WG) void k_ell_scatter(int64_t ell_entries, int nlev, const LevelDesc *__restrict__ desc, const int32_t *__restrict__ rows,
                                                    const int64_t *__restrict__ rp, const int64_t *__restrict__ diag, const double *__restrict__ lu, double *__restrict__ vals)
{
  const int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x;
  if (t >= ell_entries) return;
  int lo = 0, hi = nlev; // last level with ent_off <= t (empty levels share their offset with the next one: never the last)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (desc[mid].ent_off <= t) lo = mid;
    else hi = mid;
  }
  const LevelDesc L = desc[lo];
  const int64_t q = t - L.ent_off;
  const int64_t k = q / L.m, r = q - k * L.m;
  const int64_t i = rows[L.row_off + r];
  const int64_t k0 = UPPER ? diag[i] + 1 : rp[i], k1 = UPPER ? rp[i + 1] : diag[i];
  vals[t] = k0 + k < k1 ? lu[k0 + k] : 0.0;
}
// inverse pivots in level order (upper triangle)
__global__ __launch_bounds__(WG) void k_dinv_scatter(int64_t n, const int32_t *__restrict__ rows, const int64_t *__restrict__ diag, const double *__restrict__ lu,
                                                     double *__restrict__ dinv)
{
  const int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x;
  if (t < n) dinv[t] = lu[diag[rows[t]]];
}
// Tile stream of the pipe engine: 32 threads per (row, sweep), thread u < 26 writes entry u of the row's triangle to
// Geometry::val_off(u, lane) of the row's tile (pipe::row_slot), thread 31 of a U row the inverse pivot to the s0 slot at byte 512.
// The device twin of pipe::refresh_values.
__global__ __launch_bounds__(WG) void k_pipe_scatter(int64_t n, const int64_t *__restrict__ slot, const int64_t *__restrict__ rp, const int64_t *__restrict__ diag,
                                                     const double *__restrict__ lu, unsigned char *__restrict__ stream)
{
  static_assert(pipe::MAX_W < 31, "one thread per entry and one for the pivot");
  const int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x;
  const int64_t rs = t >> 5; // sweep * n + row
  const int u = (int)(t & 31);
  if (rs >= 2 * n) return;
  const bool upper = rs >= n;
  const int64_t g = upper ? rs - n : rs;
  const int64_t word = slot[rs];
  unsigned char *tile = stream + (word >> 16) * 1024;
  const int lane = (int)(word & 0xff);
  const int64_t k0 = upper ? diag[g] + 1 : rp[g], k1 = upper ? rp[g + 1] : diag[g];
  if (k0 + u < k1) {
    const pipe::Geometry G((int)(word >> 8 & 0xff));
    *reinterpret_cast<double *>(tile + G.val_off(u, lane)) = lu[k0 + u];
  } else if (u == 31 && upper)
    *reinterpret_cast<double *>(tile + 512 + lane * 8) = lu[diag[g]];
}

// ---- the refresh ----------------------------------------------------------------------------------
static int ilu0_refactor_enqueue(ddm_ctx *ctx, ddm_ilu0 *F, double *lu)
{
  const ddm_csr *A = F->A;
  const TriSchedule &S = F->lev->L;
  Refactor &R = *F->refac;
  HIPCHECK(ctx, hipMemsetAsync(R.status, 0xff, sizeof(unsigned), ctx->stream));
  for (const auto &p : R.plan) {
    if (p.small)
      hipLaunchKernelGGL(k_ilu0_refactor_small_levels, dim3(1), dim3(64 * REFAC_SMALL_WAVES), 0, ctx->stream, p.count, S.d_desc + p.first, (const int32_t *)S.rows, A->rp, A->ci,
                         (const double *)A->va, (const int64_t *)R.diag, lu, R.status.get());
    else {
      const LevelDesc &D = S.desc[p.first];
      hipLaunchKernelGGL(k_ilu0_refactor_level, dim3((unsigned)((D.m + REFAC_WAVES - 1) / REFAC_WAVES)), dim3(64 * REFAC_WAVES), 0, ctx->stream, D.m, S.rows + D.row_off, A->rp,
                         A->ci, (const double *)A->va, (const int64_t *)R.diag, lu, R.status.get());
    }
  }
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
static int ilu0_scatter_enqueue(ddm_ctx *ctx, ddm_ilu0 *F, const double *lu)
{
  const ddm_csr *A = F->A;
  const int64_t *diag = F->refac->diag;
  for (int pass = 0; pass < 2; ++pass) {
    TriSchedule &S = pass ? F->lev->U : F->lev->L;
    if (S.ell_entries > 0) {
      const dim3 grid((unsigned)((S.ell_entries + WG - 1) / WG));
      hipLaunchKernelGGL(pass ? k_ell_scatter<true> : k_ell_scatter<false>, grid, dim3(WG), 0, ctx->stream, S.ell_entries, (int)S.nlev, (const LevelDesc *)S.d_desc,
                         (const int32_t *)S.rows, A->rp, diag, lu, S.vals.get());
      if (S.vals_f32) hipLaunchKernelGGL(k_to_float, dim3((unsigned)((S.ell_entries + 255) / 256)), dim3(256), 0, ctx->stream, S.ell_entries, (const double *)S.vals, S.vals_f32.get());
    }
    if (pass) {
      hipLaunchKernelGGL(k_dinv_scatter, dim3((unsigned)((F->n + WG - 1) / WG)), dim3(WG), 0, ctx->stream, F->n, (const int32_t *)S.rows, diag, lu, S.dinv.get());
      if (S.dinv_f32) hipLaunchKernelGGL(k_to_float, dim3((unsigned)((F->n + 255) / 256)), dim3(256), 0, ctx->stream, F->n, (const double *)S.dinv, S.dinv_f32.get());
    }
  }
  if (F->pipe)
    hipLaunchKernelGGL(k_pipe_scatter, dim3((unsigned)((2 * F->n * 32 + WG - 1) / WG)), dim3(WG), 0, ctx->stream, F->n, (const int64_t *)F->pipe->slot, A->rp, diag, lu,
                       F->pipe->stream.get());
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}

static int sn_refresh(ddm_ctx *ctx, ddm_ilu0 *F); // sn_refresh.hpp
static int ilu0_refresh_impl(ddm_ctx *ctx, ddm_ilu0 *F)
{
  if (F->csr) return fail(ctx, DDM_ENOTIMPL, "ddm_ilu0_refresh: a sparse direct factor is not refreshed in place: create a new factor on the new values");
  if (F->sn) return sn_refresh(ctx, F);
  DDMCHECK(ilu0_join(ctx, F)); // (the background builder writes the parts the scatter fills; the engine is settled afterwards)
  if (F->engine == Engine::Box) return fail(ctx, DDM_ENOTIMPL, "ddm_ilu0_refresh: the box engine is not refreshed in place: create a new factor on the new values");
  if (F->n == 0) return DDM_OK;
  const ddm_csr *A = F->A;
  DDMCHECK(csr_wait_upload(ctx, A));
  if (A->host_only) return fail(ctx, DDM_EINVAL, "the matrix was created without device arrays (ddm_csr_create_host)");
  if (2 * F->n * 32 + WG >= ((int64_t)1 << 31) * WG) return fail(ctx, DDM_ENOTIMPL, "ddm_ilu0_refresh: too many rows for the scatter grid");
  if (!F->refac) {
    auto R = std::make_unique<Refactor>();
    DDMCHECK(upload(ctx, F->h_diag.data(), F->n, R->diag));
    HIPCHECK(ctx, R->lu.alloc(F->nnz));
    HIPCHECK(ctx, R->scratch.alloc(F->nnz));
    HIPCHECK(ctx, R->status.alloc(1));
    // launch plan over the L levels: a level of more than REFAC_SMALL_ROWS rows gets a launch of its own, runs of smaller ones share
    // one workgroup.  (Not the plan of the level SOLVE: a row costs a wave tens of microseconds here, so one workgroup pays only for
    // levels of a few rows -- with the solve's 2048-row threshold the single workgroup took 0.33 of the 0.35 s at 216^3.)
    const std::vector<LevelDesc> &desc = F->lev->L.desc;
    for (int l = 0, nlev = (int)desc.size(); l < nlev;) {
      int c = 0;
      while (l + c < nlev && c < SMALL_LEVELS_PER_LAUNCH && desc[l + c].m <= REFAC_SMALL_ROWS) ++c;
      R->plan.push_back({l, std::max(c, 1), c > 0});
      l += std::max(c, 1);
    }
    F->refac = std::move(R);
  }
  Refactor &R = *F->refac;
  {
    ScopedTimer t(ctx, "Refresh/factor");
    DDMCHECK(ilu0_refactor_enqueue(ctx, F, R.scratch));
  }
  unsigned status = 0;
  HIPCHECK(ctx, hipMemcpyAsync(&status, R.status, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (status != REFAC_OK) { // the engines, `lu` and h_lu still hold the previous factor
    const int64_t b = std::upper_bound(F->h_block_ptr.begin(), F->h_block_ptr.end(), (int64_t)status) - F->h_block_ptr.begin() - 1;
    return fail(ctx, DDM_ENUMERIC, "ILU(0): missing or zero pivot in block %lld", (long long)b);
  }
  {
    ScopedTimer t(ctx, "Refresh/scatter");
    DDMCHECK(ilu0_scatter_enqueue(ctx, F, R.scratch));
  }
  if (F->xcd) { // rebuilt from the refreshed h_lu by the next solve that needs it; the graph of an xcd2 solve points into the dropped arrays
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    F->xcd.reset();
    if (F->engine == Engine::Xcd2) F->graph.reset();
  }
  std::swap(R.lu, R.scratch);
  R.host_stale = true;
  return DDM_OK;
}
extern "C" int ddm_ilu0_refresh(ddm_ctx *ctx, ddm_ilu0 *F)
{
  if (!ctx || !F) return fail(ctx, DDM_EINVAL, "ddm_ilu0_refresh: bad arguments");
  DDMCHECK(ilu0_refresh_impl(ctx, F));
  ++F->refresh_count;
  return DDM_OK;
}
// successful in-place refreshes since creation (0 after creation; a failed or refused refresh does not count)
extern "C" int ddm_ilu0_refresh_count(const ddm_ilu0 *F) { return F ? F->refresh_count : 0; }
