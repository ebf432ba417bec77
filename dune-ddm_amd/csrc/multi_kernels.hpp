// Device kernels of the multi-right-hand-side path (ddm_*_multi: the block applies of csrc/halo.hpp and csrc/preconditioners.hpp, the block drivers of csrc/krylov_*.hpp): m independent columns stored as a row-major
// n x m block (entry (i, c) at i * m + c, the layout of ddm_csr_mm and ddm_ilu0_solve_multi), 1 <= m <= MULTI_MAX.
// Element-wise kernels run one thread per block entry (consecutive threads = consecutive addresses).  Reductions keep the tree of
// the single-vector kernels where that costs nothing: the owner-masked dots and the fused CG update use the grid, the thread-to-row
// mapping and block_sum of k_dot_partial / k_cg_update_norm, so every column's sum is bit-identical to the single-vector one.
#pragma once
#include "kernels.hpp"

namespace ddm {

constexpr int MULTI_MAX = 32; // columns of one block (ddm_cg_solve_multi)

// ---- halo: pack / deterministic unpack of m columns (one message of m x count doubles per peer) ----------------------------------
__global__ void k_pack_multi(int64_t nsend, int m, const int64_t *__restrict__ idx, const double *__restrict__ v, double *__restrict__ buf)
{
  const int64_t total = nsend * m;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    const int64_t k = t / m;
    buf[t] = v[idx[k] * m + (t - k * m)];
  }
}
// contributions in list order, as k_unpack: bit-identical per column
template <bool ADD>
__global__ void k_unpack_multi(int64_t ndst, int m, const int64_t *__restrict__ dst_idx, const int64_t *__restrict__ dst_ptr,
                               const int64_t *__restrict__ src_pos, const double *__restrict__ buf, double *__restrict__ v)
{
  const int64_t total = ndst * m;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    const int64_t k = t / m;
    const int c = (int)(t - k * m);
    const int64_t i = dst_idx[k] * m + c;
    double s = ADD ? v[i] : 0.0;
    for (int64_t q = dst_ptr[k]; q < dst_ptr[k + 1]; ++q) s = ADD ? s + buf[src_pos[q] * m + c] : buf[src_pos[q] * m + c];
    v[i] = s;
  }
}
// column c of an n x m block <-> a contiguous vector (the column-by-column exchange through the fixed-layout alltoall callback)
template <bool TO_BLOCK>
__global__ void k_column_copy(int64_t n, int m, int c, const double *__restrict__ src, double *__restrict__ dst)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) {
    if (TO_BLOCK) dst[i * m + c] = src[i];
    else dst[i] = src[i * m + c];
  }
}

// ---- Schwarz level: extend / restrict / partition of unity --------------------------------------------------------------------------
__global__ void k_extend_multi(int64_t n, int m, const int32_t *__restrict__ ext_map, const double *__restrict__ d, double *__restrict__ dov)
{
  const int64_t total = n * m;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    const int64_t i = t / m;
    const int32_t e = ext_map[i];
    dov[t] = e >= 0 ? d[(int64_t)e * m + (t - i * m)] : 0.0;
  }
}
template <bool ACC>
__global__ void k_restrict_multi(int64_t n, int m, const int32_t *__restrict__ ext_map, const double *__restrict__ xov, double *__restrict__ x)
{
  const int64_t total = n * m;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    const int64_t i = t / m;
    const int32_t e = ext_map[i];
    if (e >= 0) {
      const int64_t o = (int64_t)e * m + (t - i * m);
      x[o] = ACC ? x[o] + xov[t] : xov[t];
    }
  }
}
// x = x * w (w may be NULL), then x += add (may be NULL): the tail of the Schwarz level in the fused additive combination, in the
// order of the single-vector epilogue (k_scale, then k_axpy with 1.0)
__global__ void k_scale_add_multi(int64_t n, int m, const double *__restrict__ w, const double *__restrict__ add, double *__restrict__ x)
{
  const int64_t total = n * m;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    double v = x[t];
    if (w) v *= w[t / m];
    if (add) v += add[t];
    x[t] = v;
  }
}

// ---- coarse level ------------------------------------------------------------------------------------------------------------------
// partial[(ch * kmax + j) * m + c] = <r_j, d_c> over the rows of chunk ch.  One wave per (chunk, basis vector): its lanes cover
// R = 64 / m consecutive rows x m columns of the block (lane = row offset * m + column), so each basis entry is read once for all
// m columns and the block rows are read contiguously; the R lanes of one column are summed at the end.
__global__ __launch_bounds__(WG) void k_coarse_restrict_partial_multi(int kmax, int64_t ld, const double *__restrict__ basis, int m,
                                                                       const double *__restrict__ d, const RowChunk *__restrict__ chunks,
                                                                       double *__restrict__ partial, int nchunk)
{
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int R = 64 / m, rr = lane / m, c = lane - rr * m;
  const bool on = rr < R;
  for (int ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const RowChunk cu = chunks[ch];
    for (int j = w; j < kmax; j += 4) {
      const double *bj = basis + (int64_t)j * ld;
      double s = 0.0;
      if (on) {
        int64_t r = cu.r0 + rr;
        for (; r + 3 * R < cu.r1; r += 4 * R) { // four rows of each stream in flight per lane
          double bv[4], dv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) bv[u] = __builtin_nontemporal_load(bj + r + u * R);
#pragma unroll
          for (int u = 0; u < 4; ++u) dv[u] = d[(r + u * R) * m + c];
#pragma unroll
          for (int u = 0; u < 4; ++u) s += bv[u] * dv[u];
        }
        for (; r < cu.r1; r += R) s += bj[r] * d[r * m + c];
      }
      double acc = s;
      for (int q = 1; q < R; ++q) { // lanes c, c + m, c + 2m, ... hold the partial sums of column c
        const double o = __shfl(s, lane + q * m, 64);
        acc += o;
      }
      if (lane < m) partial[((int64_t)ch * kmax + j) * m + lane] = acc;
    }
  }
}
// one workgroup: chunk partials of every (subdomain, vector, column) summed in chunk order, scattered to the K x m coarse defect
__global__ __launch_bounds__(WG) void k_coarse_restrict_final_multi(int nsub, int kmax, int m, const int32_t *__restrict__ sub_chunk_ptr,
                                                                     const double *__restrict__ partial, const int64_t *__restrict__ coarse_index,
                                                                     int64_t K, double *__restrict__ d0)
{
  for (int64_t i = threadIdx.x; i < K * m; i += WG) d0[i] = 0.0;
  __syncthreads();
  const int total = nsub * kmax * m;
  for (int t = threadIdx.x; t < total; t += WG) {
    const int sj = t / m, c = t - sj * m;
    const int s = sj / kmax, j = sj - s * kmax;
    const int64_t gi = coarse_index[sj];
    if (gi < 0) continue;
    double acc = 0.0;
    for (int q = sub_chunk_ptr[s]; q < sub_chunk_ptr[s + 1]; ++q) acc += partial[((int64_t)q * kmax + j) * m + c];
    d0[gi * m + c] = acc;
  }
}
// X0 = A0^-1 D0 with the replicated K x K inverse and K x m blocks: one thread per entry of X0 (the row of A0^-1 is shared by the
// m threads of one row; D0 is read along its rows)
__global__ __launch_bounds__(WG) void k_dense_mm(int64_t K, int m, const double *__restrict__ M, const double *__restrict__ D0, double *__restrict__ X0)
{
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (t >= K * m) return;
  const int64_t row = t / m;
  const int c = (int)(t - row * m);
  const double *mr = M + row * K;
  double s = 0.0;
  for (int64_t k = 0; k < K; ++k) s += mr[k] * D0[k * m + c];
  X0[t] = s;
}
// x_ovlp[r, c] = sum_j x0[(s, j), c] r_j[r]: one thread per block entry, the basis vectors added in the order of k_coarse_prolong
// (the same products and sums per entry)
__global__ __launch_bounds__(WG) void k_coarse_prolong_multi(int kmax, int64_t ld, const double *__restrict__ basis, int m, const double *__restrict__ x0,
                                                              const int64_t *__restrict__ coarse_index, const RowChunk *__restrict__ chunks,
                                                              double *__restrict__ xov, int nchunk)
{
  __shared__ int64_t gidx[COARSE_KMAX];
  for (int ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const RowChunk cu = chunks[ch];
    __syncthreads(); // gidx of the previous chunk is no longer read
    if (threadIdx.x < kmax) gidx[threadIdx.x] = coarse_index[(int64_t)cu.sub * kmax + threadIdx.x];
    __syncthreads();
    const int64_t e1 = cu.r1 * m;
    for (int64_t e = cu.r0 * m + threadIdx.x; e < e1; e += WG) {
      const int64_t r = e / m;
      const int c = (int)(e - r * m);
      double s = 0.0;
      for (int j = 0; j < kmax; ++j) {
        const int64_t gi = gidx[j];
        const double cj = gi >= 0 ? x0[gi * m + c] : 0.0;
        s += cj * __builtin_nontemporal_load(basis + (int64_t)j * ld + r);
      }
      xov[e] = s;
    }
  }
}

// ---- CG vector work ----------------------------------------------------------------------------------------------------------------
// owner-masked dots of columns [c0, c0 + CB): the grid, rows per thread and block_sum of k_dot_partial; partial[c * gridDim.x + b]
template <int CB, bool MASKED>
__global__ __launch_bounds__(WG) void k_dot_partial_multi(int64_t n, int m, int c0, const uint8_t *__restrict__ mask, const double *__restrict__ x,
                                                          const double *__restrict__ y, double *__restrict__ partial)
{
  __shared__ double red[4];
  double s[CB];
#pragma unroll
  for (int u = 0; u < CB; ++u) s[u] = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG)
    if (!MASKED || mask[i]) {
      const double *xi = x + i * m + c0, *yi = y + i * m + c0;
#pragma unroll
      for (int u = 0; u < CB; ++u) s[u] += xi[u] * yi[u];
    }
#pragma unroll
  for (int u = 0; u < CB; ++u) {
    const double t = block_sum(s[u], red);
    if (threadIdx.x == 0) partial[(int64_t)(c0 + u) * gridDim.x + blockIdx.x] = t;
  }
}
// one workgroup per column: the partials summed as k_reduce_final does
__global__ __launch_bounds__(WG) void k_reduce_final_multi(int nb, const double *__restrict__ partial, double *__restrict__ out)
{
  __shared__ double red[4];
  const double *p = partial + (int64_t)blockIdx.x * nb;
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += WG) s += p[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}
// per-column CG scalars of the ACTIVE columns (a converged column keeps its values; nothing is multiplied by a zero step).
// scal: the rows SCAL_* (kernels.hpp) of ctx->mscal
__global__ void k_cg_beta_multi(int m, const int32_t *__restrict__ active, double *__restrict__ scal)
{
  const int c = threadIdx.x;
  if (c < m && active[c]) {
    scal[SCAL_BETA * MULTI_MAX + c] = scal[SCAL_RHO * MULTI_MAX + c] / scal[SCAL_RHOLAST * MULTI_MAX + c];
    scal[SCAL_RHOLAST * MULTI_MAX + c] = scal[SCAL_RHO * MULTI_MAX + c];
  }
}
__global__ void k_cg_lambda_multi(int m, const int32_t *__restrict__ active, double *__restrict__ scal)
{
  const int c = threadIdx.x;
  if (c < m && active[c]) scal[SCAL_STEP * MULTI_MAX + c] = scal[SCAL_RHOLAST * MULTI_MAX + c] / scal[SCAL_PQ * MULTI_MAX + c];
}
// p = beta p + q in the active columns
__global__ void k_cg_direction_multi(int64_t n, int m, const int32_t *__restrict__ active, const double *__restrict__ scal, const double *__restrict__ q,
                                     double *__restrict__ p)
{
  const int64_t total = n * m;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    const int c = (int)(t % m);
    if (active[c]) p[t] = scal[SCAL_BETA * MULTI_MAX + c] * p[t] + q[t];
  }
}
// x += lambda p; b -= lambda q; partial sums of <b, b> for columns [c0, c0 + CB) -- k_cg_update_norm per column (same grid, rows per
// thread and block_sum).  Columns that are not active are neither read nor written (their partials are 0).  lambda_c is
// scal[slot * MULTI_MAX + c]: slot SCAL_STEP in the CG drivers.
template <int CB, bool MASKED>
__global__ __launch_bounds__(WG) void k_cg_update_norm_multi(int64_t n, int m, int c0, const int32_t *__restrict__ active, const double *__restrict__ scal,
                                                             int slot, const uint8_t *__restrict__ mask, const double *__restrict__ p, const double *__restrict__ q,
                                                             double *__restrict__ x, double *__restrict__ b, double *__restrict__ partial)
{
  __shared__ double red[4];
  double lam[CB], s[CB];
  bool on[CB];
#pragma unroll
  for (int u = 0; u < CB; ++u) {
    on[u] = active[c0 + u] != 0;
    lam[u] = scal[slot * MULTI_MAX + c0 + u];
    s[u] = 0.0;
  }
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) {
    const int64_t o = i * m + c0;
    const bool own = !MASKED || mask[i];
#pragma unroll
    for (int u = 0; u < CB; ++u)
      if (on[u]) {
        x[o + u] += lam[u] * p[o + u];
        const double bi = b[o + u] - lam[u] * q[o + u];
        b[o + u] = bi;
        if (own) s[u] += bi * bi;
      }
  }
#pragma unroll
  for (int u = 0; u < CB; ++u) {
    const double t = block_sum(s[u], red);
    if (threadIdx.x == 0) partial[(int64_t)(c0 + u) * gridDim.x + blockIdx.x] = t;
  }
}

// ---- queued CG (ddm_cg_solve_queue, csrc/krylov_cg.hpp): columns of the caller's n x ncols blocks enter and leave the slots of the n x m work blocks ----
// tab: nload (slot, column) pairs, tab[2k] = slot < m and tab[2k + 1] = column < ncols.  One thread per (row, pair) entry, the pair
// index running fastest (consecutive lanes = consecutive table entries of one row).
// Load: x_slot = X[:, column], b_slot = B[:, column], p_slot = 0 and rholast_slot = 1 (scal as in k_cg_beta_multi): the slot's next
// beta = rho / 1 is finite and its next direction p = beta * 0 + q is q, the first CG direction of the new column.
__global__ void k_column_load_multi(int64_t n, int m, int nload, const int64_t *__restrict__ tab, int64_t ncols, const double *__restrict__ Xc,
                                    const double *__restrict__ Bc, double *__restrict__ x, double *__restrict__ b, double *__restrict__ p,
                                    double *__restrict__ scal)
{
  const int64_t gid = blockIdx.x * (int64_t)WG + threadIdx.x;
  if (gid < nload) scal[SCAL_RHOLAST * MULTI_MAX + tab[2 * gid]] = 1.0;
  const int64_t total = n * nload;
  for (int64_t t = gid; t < total; t += (int64_t)gridDim.x * WG) {
    const int64_t i = t / nload;
    const int k = (int)(t - i * nload);
    const int64_t o = i * m + tab[2 * k], src = i * ncols + tab[2 * k + 1];
    x[o] = Xc[src];
    b[o] = Bc[src];
    p[o] = 0.0;
  }
}
// Store: X[:, column] = x_slot for the nstore pairs of tab
__global__ void k_column_store_multi(int64_t n, int m, int nstore, const int64_t *__restrict__ tab, int64_t ncols, const double *__restrict__ x,
                                     double *__restrict__ Xc)
{
  const int64_t total = n * nstore;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    const int64_t i = t / nstore;
    const int k = (int)(t - i * nstore);
    Xc[i * ncols + tab[2 * k + 1]] = x[i * m + tab[2 * k]];
  }
}

// ---- queued BiCGSTAB (ddm_bicgstab_solve_queue, csrc/krylov_bicgstab.hpp) -----------------------------------------------------------------------
// Per-column scalars in ctx->mscal, M = MULTI_MAX: [0..M) rho, [M..2M) alpha, [2M..3M) omega, [3M..4M) beta.  The sums the host
// reads are packed at stride m (the block width), so that one copy takes a group of them:
//   first half step   [4M..): <r, r>, then h = <rt, v>, then the rho and the omega that the direction update used (4 m doubles)
//   second half step  [8M..): <r, r>, then rho_new = <rt, r> of the next iteration (2 m doubles)
//   refill            [10M..): <r, r> of the loaded slots;  [11M..): <t, t>, then <t, r> (2 m doubles)
constexpr int BICG_RHO = 0, BICG_ALPHA = 1, BICG_OMEGA = 2, BICG_BETA = 3, BICG_HALF1 = 4, BICG_HALF2 = 8, BICG_LOAD = 10, BICG_TT = 11;
constexpr int BICG_SCALARS = 13; // ... times MULTI_MAX doubles
static_assert(BICG_SCALARS <= SCAL_ROWS, "queued BiCGSTAB: rows 0 .. BICG_SCALARS - 1 of ctx->mscal, over the CG family's rows (kernels.hpp)");

// beta = (rho_new / rho) (alpha / omega) in the active columns; rho and omega as used go where the host reads them with the first
// half step's defect (its breakdown checks run on exactly these operands)
__global__ void k_bicg_beta_multi(int m, const int32_t *__restrict__ active, double *__restrict__ scal)
{
  const int c = threadIdx.x;
  if (c < m && active[c]) {
    const double rho = scal[BICG_RHO * MULTI_MAX + c], omega = scal[BICG_OMEGA * MULTI_MAX + c];
    const double rho_new = scal[BICG_HALF2 * MULTI_MAX + m + c];
    scal[BICG_BETA * MULTI_MAX + c] = (rho_new / rho) * (scal[BICG_ALPHA * MULTI_MAX + c] / omega);
    scal[BICG_HALF1 * MULTI_MAX + 2 * m + c] = rho;
    scal[BICG_HALF1 * MULTI_MAX + 3 * m + c] = omega;
  }
}
// alpha = rho_new / h
__global__ void k_bicg_alpha_multi(int m, const int32_t *__restrict__ active, double *__restrict__ scal)
{
  const int c = threadIdx.x;
  if (c < m && active[c]) scal[BICG_ALPHA * MULTI_MAX + c] = scal[BICG_HALF2 * MULTI_MAX + m + c] / scal[BICG_HALF1 * MULTI_MAX + m + c];
}
// omega = <t, r> / <t, t>; rho = rho_new
__global__ void k_bicg_omega_multi(int m, const int32_t *__restrict__ active, double *__restrict__ scal)
{
  const int c = threadIdx.x;
  if (c < m && active[c]) {
    scal[BICG_OMEGA * MULTI_MAX + c] = scal[BICG_TT * MULTI_MAX + m + c] / scal[BICG_TT * MULTI_MAX + c];
    scal[BICG_RHO * MULTI_MAX + c] = scal[BICG_HALF2 * MULTI_MAX + m + c];
  }
}
// Load of a BiCGSTAB slot (tab as in k_column_load_multi): x_slot = X[:, column], r_slot = B[:, column], p_slot = v_slot = 0 and
// rho = alpha = omega = 1: the slot's next beta is finite and its next direction p = r + beta (0 - omega 0) is r, the first
// direction of the new column.
__global__ void k_bicg_column_load_multi(int64_t n, int m, int nload, const int64_t *__restrict__ tab, int64_t ncols, const double *__restrict__ Xc,
                                         const double *__restrict__ Bc, double *__restrict__ x, double *__restrict__ r, double *__restrict__ p,
                                         double *__restrict__ v, double *__restrict__ scal)
{
  const int64_t gid = blockIdx.x * (int64_t)WG + threadIdx.x;
  if (gid < nload) {
    const int64_t s = tab[2 * gid];
    scal[BICG_RHO * MULTI_MAX + s] = scal[BICG_ALPHA * MULTI_MAX + s] = scal[BICG_OMEGA * MULTI_MAX + s] = 1.0;
  }
  const int64_t total = n * nload;
  for (int64_t t = gid; t < total; t += (int64_t)gridDim.x * WG) {
    const int64_t i = t / nload;
    const int k = (int)(t - i * nload);
    const int64_t o = i * m + tab[2 * k], src = i * ncols + tab[2 * k + 1];
    x[o] = Xc[src];
    r[o] = Bc[src];
    p[o] = 0.0;
    v[o] = 0.0;
  }
}
// rt = r in the columns of `active` (the slots just loaded, r being their initial defect) and their rho_new = <rt, r> = <r, r>, the
// sum that the defect pass of the refill has just formed on the grid of the block dot
__global__ void k_bicg_shadow_multi(int64_t n, int m, const int32_t *__restrict__ active, const double *__restrict__ r, double *__restrict__ rt,
                                    double *__restrict__ scal)
{
  const int64_t gid = blockIdx.x * (int64_t)WG + threadIdx.x;
  if (gid < m && active[gid]) scal[BICG_HALF2 * MULTI_MAX + m + gid] = scal[BICG_LOAD * MULTI_MAX + gid];
  const int64_t total = n * m;
  for (int64_t t = gid; t < total; t += (int64_t)gridDim.x * WG)
    if (active[t % m]) rt[t] = r[t];
}
// the vector updates, one simple kernel each: y += sign coef_c x (coef null: 1) and y *= coef_c in the active columns, one thread per
// block entry
__global__ void k_axpy_dev_multi(int64_t n, int m, const int32_t *__restrict__ active, const double *__restrict__ coef, double sign,
                                 const double *__restrict__ x, double *__restrict__ y)
{
  const int64_t total = n * m;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    const int c = (int)(t % m);
    if (active[c]) y[t] += (coef ? sign * coef[c] : sign) * x[t];
  }
}
__global__ void k_scal_dev_multi(int64_t n, int m, const int32_t *__restrict__ active, const double *__restrict__ coef, double *__restrict__ y)
{
  const int64_t total = n * m;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    const int c = (int)(t % m);
    if (active[c]) y[t] *= coef[c];
  }
}

// ---- restarted GMRES vector work (ddm_gmres_solve_multi, csrc/krylov_gmres.hpp) -----------------------------------------------------------------------------
// per-column host scalars of one launch, passed by value (no upload, no synchronisation)
struct MultiCoef {
  double a[MULTI_MAX];
};
// The update of one modified Gram-Schmidt step, w -= h v with the coefficients h (m device doubles, already summed over the ranks):
// k_axpy_negdev on every active column, one thread per block entry
__global__ void k_axpy_negdev_multi(int64_t n, int m, const int32_t *__restrict__ active, const double *__restrict__ h, const double *__restrict__ v,
                                    double *__restrict__ w)
{
  const int64_t total = n * m;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    const int c = (int)(t % m);
    if (active[c]) w[t] -= h[c] * v[t];
  }
}
// dst = src * coef in the active columns (v_{i+1} = w / h_{i+1,i} with coef = 1 / h_{i+1,i}, the k_scal of the single-vector loop;
// dst may be src)
__global__ void k_scale_into_multi(int64_t n, int m, const int32_t *__restrict__ active, MultiCoef coef, const double *src, double *dst)
{
  const int64_t total = n * m;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    const int c = (int)(t % m);
    if (active[c]) dst[t] = src[t] * coef.a[c];
  }
}
// End of a restart cycle: W_c = sum_{k < cnt_c} y_{k,c} v_{k,c} (terms added in ascending k, as the AXPY sequence of the
// single-vector loop) and X_c += W_c for the columns with cnt_c > 0.  y: restart x m device doubles; cnt_c = Hessenberg columns of
// column c in this cycle (0: frozen before the cycle, neither X nor the basis is touched).  Columns with keep_c == 0 (frozen, or
// converged in this cycle) get W_c = 0 written, so that the B -= A W that follows leaves their column of B as it is.
// V: basis blocks at stride vstride (= n * m).
__global__ __launch_bounds__(WG) void k_gmres_update_multi(int64_t n, int m, const int32_t *__restrict__ cnt, const int32_t *__restrict__ keep,
                                                           const double *__restrict__ y, const double *__restrict__ V, int64_t vstride,
                                                           double *__restrict__ W, double *__restrict__ X)
{
  const int64_t total = n * m;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    const int c = (int)(t % m);
    const int kc = cnt[c];
    double s = 0.0;
    if (kc > 0) {
      const double *vt = V + t;
      int k = 0;
      for (; k + 3 < kc; k += 4) { // four basis blocks in flight per thread
        double vv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vv[u] = __builtin_nontemporal_load(vt + (int64_t)(k + u) * vstride);
#pragma unroll
        for (int u = 0; u < 4; ++u) s += y[(int64_t)(k + u) * m + c] * vv[u];
      }
      for (; k < kc; ++k) s += y[(int64_t)k * m + c] * vt[(int64_t)k * vstride];
      X[t] += s;
    }
    W[t] = keep[c] ? s : 0.0;
  }
}

// ---- flexible restarted GMRES (ddm_fgmres_solve_multi, csrc/krylov_gmres.hpp) -------------------------------------------------------------
// Restart of the flexible driver for columns [c0, c0 + CB): b -= t (t = A W, the operator applied to the cycle's solution update) in
// the active columns and, in the same pass, the owner-masked partial sums of <b, b> -- the true defect norms the next cycle starts
// from.  The grid, the rows per thread and block_sum are those of k_dot_partial_multi, so b and the sums are bit-identical to
// k_axpy_negdev_multi with unit coefficients followed by k_dot_partial_multi(b, b).  A column that is not active is not written; its
// sum is that of the column as it stands (nobody reads it in the driver).  16 (active) or 8 bytes per block entry instead of 24 + 16.
template <int CB, bool MASKED>
__global__ __launch_bounds__(WG) void k_defect_norm_multi(int64_t n, int m, int c0, const int32_t *__restrict__ active, const uint8_t *__restrict__ mask,
                                                          const double *__restrict__ t, double *__restrict__ b, double *__restrict__ partial)
{
  __shared__ double red[4];
  double s[CB];
  bool on[CB];
#pragma unroll
  for (int u = 0; u < CB; ++u) {
    on[u] = active[c0 + u] != 0;
    s[u] = 0.0;
  }
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) {
    const int64_t o = i * m + c0;
    const bool own = !MASKED || mask[i];
    double bi[CB], ti[CB];
#pragma unroll
    for (int u = 0; u < CB; ++u) { // every load of the row is issued before the first use
      bi[u] = b[o + u];
      ti[u] = on[u] ? t[o + u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < CB; ++u) {
      if (on[u]) {
        bi[u] -= ti[u];
        b[o + u] = bi[u];
      }
      if (own) s[u] += bi[u] * bi[u];
    }
  }
#pragma unroll
  for (int u = 0; u < CB; ++u) {
    const double r = block_sum(s[u], red);
    if (threadIdx.x == 0) partial[(int64_t)(c0 + u) * gridDim.x + blockIdx.x] = r;
  }
}

// ---- flexible CG (ddm_fcg_solve_multi, csrc/krylov_fcg.hpp): the orthogonalisation of a fresh direction block against stored slots ---------
constexpr int FCG_SG = 4; // slots one pass of k_fcg_project_multi takes: FCG_SG x CB accumulators
// Projection for columns [c0, c0 + CB): the owner-masked partial sums of <Ad_j, d> for the set.n <= FCG_SG stored image blocks of the
// set (block j at AD + set.buf[j] * stride) in ONE pass over the block d.  The grid, the rows per thread and block_sum are those of
// k_dot_partial_multi, so every sum is bit-identical to dot_multi_device(Ad_j, d) -- in every column, frozen ones included, as there.
// partial[((j0 + j) * m + c) * gridDim.x + b]
template <int CB, bool MASKED>
__global__ __launch_bounds__(WG) void k_fcg_project_multi(int64_t n, int m, int c0, const uint8_t *__restrict__ mask, const double *__restrict__ AD,
                                                          int64_t stride, FcgSet set, int j0, const double *__restrict__ d, double *__restrict__ partial)
{
  __shared__ double red[4];
  double s[FCG_SG][CB];
  const double *a[FCG_SG];
#pragma unroll
  for (int j = 0; j < FCG_SG; ++j) {
    a[j] = AD + (int64_t)set.buf[j < set.n ? j : 0] * stride; // (past the set: a valid address that is never loaded)
#pragma unroll
    for (int u = 0; u < CB; ++u) s[j][u] = 0.0;
  }
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG)
    if (!MASKED || mask[i]) {
      const int64_t o = i * m + c0;
      double di[CB];
#pragma unroll
      for (int u = 0; u < CB; ++u) di[u] = d[o + u];
#pragma unroll
      for (int j = 0; j < FCG_SG; ++j)
        if (j < set.n) { // (uniform over the grid)
          double ai[CB];
#pragma unroll
          for (int u = 0; u < CB; ++u) ai[u] = a[j][o + u];
#pragma unroll
          for (int u = 0; u < CB; ++u) s[j][u] += ai[u] * di[u];
        }
    }
#pragma unroll
  for (int j = 0; j < FCG_SG; ++j)
#pragma unroll
    for (int u = 0; u < CB; ++u) {
      const double t = block_sum(s[j][u], red);
      if (threadIdx.x == 0 && j < set.n) partial[((int64_t)(j0 + j) * m + c0 + u) * gridDim.x + blockIdx.x] = t;
    }
}
// coef[(j0 + j) * m + c] = num[(j0 + j) * m + c] / g[set.buf[j] * m + c] in the active columns, 0 in the others (their coefficients are
// never applied): the Gram-Schmidt coefficients <Ad_k, d> / <d_k, Ad_k>, formed on the device.  One thread per (j, c).
__global__ void k_fcg_coef_multi(int m, const int32_t *__restrict__ active, FcgSet set, int j0, const double *__restrict__ num, const double *__restrict__ g,
                                 double *__restrict__ coef)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= set.n * m) return;
  const int j = t / m, c = t - j * m;
  coef[(int64_t)(j0 + j) * m + c] = active[c] ? num[(int64_t)(j0 + j) * m + c] / g[(int64_t)set.buf[j] * m + c] : 0.0;
}
// Update: d -= sum_j coef_j d_j in the active columns, in one read-modify-write of the block d, the terms in the order of the set: per
// entry the operations of set.n launches of k_axpy_negdev_multi, so d is bit-identical to them (the build does not contract
// a * b + c).  A column that is not active is neither read nor written.  One thread per block entry.
__global__ __launch_bounds__(WG) void k_fcg_orth_multi(int64_t n, int m, const int32_t *__restrict__ active, const double *__restrict__ D, int64_t stride,
                                                       FcgSet set, int j0, const double *__restrict__ coef, double *__restrict__ d)
{
  const int64_t total = n * m;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
    const int c = (int)(t % m);
    if (!active[c]) continue;
    double w = d[t];
    for (int j = 0; j < set.n; ++j) w -= coef[(int64_t)(j0 + j) * m + c] * D[(int64_t)set.buf[j] * stride + t];
    d[t] = w;
  }
}
// the owner-masked partial sums of <d, Ad> and <d, b> for columns [c0, c0 + CB) in one pass over d, each in the summation order of
// k_dot_partial_multi; partial[(q * m + c) * gridDim.x + b] holds block b's sum for column c, q = 0: <d, Ad>, q = 1: <d, b>.
// Columns that are not active are not read (their partials are 0).
template <int CB, bool MASKED>
__global__ __launch_bounds__(WG) void k_fcg_dots_multi(int64_t n, int m, int c0, const int32_t *__restrict__ active, const uint8_t *__restrict__ mask,
                                                       const double *__restrict__ d, const double *__restrict__ Ad, const double *__restrict__ b,
                                                       double *__restrict__ partial)
{
  __shared__ double red[4];
  double sg[CB], sb[CB];
  bool on[CB];
#pragma unroll
  for (int u = 0; u < CB; ++u) {
    on[u] = active[c0 + u] != 0;
    sg[u] = sb[u] = 0.0;
  }
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG)
    if (!MASKED || mask[i]) {
      const int64_t o = i * m + c0;
#pragma unroll
      for (int u = 0; u < CB; ++u)
        if (on[u]) {
          const double di = d[o + u];
          sg[u] += di * Ad[o + u];
          sb[u] += di * b[o + u];
        }
    }
#pragma unroll
  for (int u = 0; u < CB; ++u) {
    const double x = block_sum(sg[u], red);
    const double y = block_sum(sb[u], red);
    if (threadIdx.x == 0) {
      partial[(int64_t)(c0 + u) * gridDim.x + blockIdx.x] = x;
      partial[(int64_t)(m + c0 + u) * gridDim.x + blockIdx.x] = y;
    }
  }
}
// per active column: g_s = <d, Ad> into its slot (gslot: m doubles) and the step alpha = <d, b> / g_s into the lambda row of scal,
// where k_cg_update_norm_multi reads it; dots: the 2 m sums of k_fcg_dots_multi.  g_s == 0 makes the step NaN (see k_fcg_alpha).
__global__ void k_fcg_alpha_multi(int m, const int32_t *__restrict__ active, const double *__restrict__ dots, double *__restrict__ gslot,
                                  double *__restrict__ scal)
{
  const int c = threadIdx.x;
  if (c < m && active[c]) {
    const double g = dots[c];
    gslot[c] = g;
    scal[SCAL_STEP * MULTI_MAX + c] = g == 0.0 ? __builtin_nan("") : dots[m + c] / g;
  }
}

// ---- block CG (ddm_bcg_solve_multi, csrc/krylov_bcg.hpp): the m x m coupling of the columns ------------------------------------------------
// All three kernels walk the block in tiles of whole rows that one workgroup stages in LDS with contiguous loads (a tile of rows IS a
// contiguous piece of a row-major block), tile tb = blockIdx.x, blockIdx.x + gridDim.x, ...  No atomics: every sum has one owner and a
// fixed order, so the results do not change from call to call.  Plain FP64 multiplies and adds (the build does not contract them); the
// passes are HBM-bound up to m = 32.
constexpr int BCG_TILE = 1024; // block entries of one staged tile (8 KiB per block)

// Owner-masked Gram products of row-major n x m blocks in ONE pass: G1 = U^T V1 and, with TWO, G2 = U^T V2.
// A tile is BCG_TILE / mp rows (mp = m rounded up to even; the LDS rows are mp wide, the pad column is zero; rows that are not owned
// are staged as zeros).  The outputs are cut into NO = (mp / 2)^2 blocks of 2 x 2 entries (x 2 products: 8 accumulators); thread
// (s, o) owns output block o for the tile rows s, s + NS, ... with NS = WG / NO row slices (threads past NS * NO idle: m = 32 uses
// all 256 as 256 x 1, m = 8 as 16 x 16).  At the end the NS slices are summed in ascending s through LDS.
// partial[((p * m + i) * m + j) * gridDim.x + b] = block b's sum for entry (i, j) of product p: the layout k_reduce_final_multi sums.
template <bool TWO, bool MASKED>
__global__ __launch_bounds__(WG) void k_bcg_gram_partial(int64_t n, int m, const uint8_t *__restrict__ mask, const double *__restrict__ U,
                                                         const double *__restrict__ V1, const double *__restrict__ V2, double *__restrict__ partial)
{
  __shared__ double lds[3 * BCG_TILE];
  const int mp = (m + 1) & ~1, hb = mp >> 1, NO = hb * hb, NS = WG / NO, TR = BCG_TILE / mp;
  double *Ut = lds, *V1t = lds + BCG_TILE, *V2t = lds + 2 * BCG_TILE;
  const int t = threadIdx.x;
  const int s = t / NO, o = t - s * NO, oi = o / hb, oj = o - oi * hb;
  double acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.0;
  if (mp != m)
    for (int r = t; r < TR; r += WG) Ut[r * mp + m] = V1t[r * mp + m] = V2t[r * mp + m] = 0.0; // (no staging loop writes the pad column)
  const int64_t ntile = (n + TR - 1) / TR;
  for (int64_t tb = blockIdx.x; tb < ntile; tb += gridDim.x) {
    const int64_t r0 = tb * TR;
    const int rows = (int)(n - r0 < TR ? n - r0 : TR);
    __syncthreads(); // the previous tile is no longer read
    for (int e = t; e < rows * m; e += WG) {
      const int r = e / m, l = r * mp + (e - r * m);
      const int64_t g = r0 * m + e;
      const bool own = !MASKED || mask[r0 + r];
      Ut[l] = own ? U[g] : 0.0;
      V1t[l] = own ? V1[g] : 0.0;
      if (TWO) V2t[l] = own ? V2[g] : 0.0;
    }
    __syncthreads();
    if (s < NS)
      for (int r = s; r < rows; r += NS) {
        const double *u = Ut + r * mp + 2 * oi, *v1 = V1t + r * mp + 2 * oj;
        const double u0 = u[0], u1 = u[1], a0 = v1[0], a1 = v1[1];
        acc[0] += u0 * a0;
        acc[1] += u0 * a1;
        acc[2] += u1 * a0;
        acc[3] += u1 * a1;
        if (TWO) {
          const double *v2 = V2t + r * mp + 2 * oj;
          const double b0 = v2[0], b1 = v2[1];
          acc[4] += u0 * b0;
          acc[5] += u0 * b1;
          acc[6] += u1 * b0;
          acc[7] += u1 * b1;
        }
      }
  }
  __syncthreads(); // the tiles are done with: their LDS takes the accumulators, thread t's at 8 t (t = s * NO + o)
#pragma unroll
  for (int k = 0; k < 8; ++k) lds[t * 8 + k] = s < NS ? acc[k] : 0.0;
  __syncthreads();
  for (int idx = t; idx < NO * 8; idx += WG) {
    const int oo = idx >> 3, k = idx & 7;
    if (!TWO && k >= 4) continue;
    double sum = 0.0;
    for (int ss = 0; ss < NS; ++ss) sum += lds[(ss * NO + oo) * 8 + k];
    const int i = 2 * (oo / hb) + ((k >> 1) & 1), j = 2 * (oo % hb) + (k & 1), p = k >> 2;
    if (i < m && j < m) partial[((int64_t)(p * m + i) * m + j) * gridDim.x + blockIdx.x] = sum;
  }
}

// The tiles of the two update kernels: QR = WG / m rows per quarter, a tile is four quarters (4 QR rows, at most BCG_TILE entries).
// Thread t < QR m owns entry t of every quarter -- row t / m of the quarter, column c = t % m, the same column in all four, so the
// coefficient coef[j][c] is read once for four rows.  Global entry of quarter q: g0 + q QR m + t, consecutive over the threads.
__device__ __forceinline__ void bcg_stage_tile(int64_t g0, int64_t total, int entries, const double *__restrict__ src, double *tile)
{
  for (int e = threadIdx.x; e < entries; e += WG) tile[e] = g0 + e < total ? src[g0 + e] : 0.0;
}
// X += P alpha; R -= Q alpha (alpha: m x m row-major device doubles, staged in LDS; per entry the m products are summed in ascending j
// and the sum is then added to x / taken from r); the owner-masked partial sums of the new <R_c, R_c> from the same pass, a column's
// terms added per thread over the tiles, then over the threads of the column in ascending row: partial[c * gridDim.x + b].
template <bool MASKED>
__global__ __launch_bounds__(WG) void k_bcg_update_norm(int64_t n, int m, const double *__restrict__ alpha, const uint8_t *__restrict__ mask,
                                                        const double *__restrict__ P, const double *__restrict__ Q, double *__restrict__ X,
                                                        double *__restrict__ R, double *__restrict__ partial)
{
  __shared__ double Pt[BCG_TILE], Qt[BCG_TILE], al[MULTI_MAX * MULTI_MAX], red[WG];
  const int QR = WG / m, QE = QR * m, TR = 4 * QR;
  const int t = threadIdx.x, r = t / m, c = t - r * m;
  const bool on = t < QE;
  for (int e = t; e < m * m; e += WG) al[e] = alpha[e];
  double s = 0.0;
  const int64_t total = n * m, ntile = (n + TR - 1) / TR;
  for (int64_t tb = blockIdx.x; tb < ntile; tb += gridDim.x) {
    const int64_t r0 = tb * TR, g0 = r0 * m;
    __syncthreads(); // the previous tile is no longer read (first trip: al is complete)
    bcg_stage_tile(g0, total, 4 * QE, P, Pt);
    bcg_stage_tile(g0, total, 4 * QE, Q, Qt);
    __syncthreads();
    if (on) {
      double xs[4] = {0.0, 0.0, 0.0, 0.0}, rs[4] = {0.0, 0.0, 0.0, 0.0};
      for (int j = 0; j < m; ++j) {
        const double a = al[j * m + c];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          xs[q] += Pt[q * QE + r * m + j] * a;
          rs[q] += Qt[q * QE + r * m + j] * a;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t g = g0 + q * QE + t;
        if (g < total) {
          X[g] += xs[q];
          const double rn = R[g] - rs[q];
          R[g] = rn;
          if (!MASKED || mask[r0 + q * QR + r]) s += rn * rn;
        }
      }
    }
  }
  __syncthreads();
  red[t] = on ? s : 0.0;
  __syncthreads();
  if (t < m) {
    double sum = 0.0;
    for (int k = 0; k < QR; ++k) sum += red[k * m + t];
    partial[(int64_t)t * gridDim.x + blockIdx.x] = sum;
  }
}
// P = Z + P beta, in place (beta: m x m row-major device doubles): a row's m outputs need that row's m inputs only, and the tile is
// staged before any of its entries is written.
__global__ __launch_bounds__(WG) void k_bcg_direction(int64_t n, int m, const double *__restrict__ beta, const double *__restrict__ Z, double *__restrict__ P)
{
  __shared__ double Pt[BCG_TILE], be[MULTI_MAX * MULTI_MAX];
  const int QR = WG / m, QE = QR * m, TR = 4 * QR;
  const int t = threadIdx.x, r = t / m, c = t - r * m;
  for (int e = t; e < m * m; e += WG) be[e] = beta[e];
  const int64_t total = n * m, ntile = (n + TR - 1) / TR;
  for (int64_t tb = blockIdx.x; tb < ntile; tb += gridDim.x) {
    const int64_t g0 = tb * TR * m;
    __syncthreads();
    bcg_stage_tile(g0, total, 4 * QE, P, Pt);
    __syncthreads();
    if (t < QE) {
      double ps[4] = {0.0, 0.0, 0.0, 0.0};
      for (int j = 0; j < m; ++j) {
        const double b = be[j * m + c];
#pragma unroll
        for (int q = 0; q < 4; ++q) ps[q] += Pt[q * QE + r * m + j] * b;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t g = g0 + q * QE + t;
        if (g < total) P[g] = Z[g] + ps[q];
      }
    }
  }
}

// ---- block GMRES (ddm_bgmres_solve_multi, csrc/krylov_bgmres.hpp): block classical Gram-Schmidt against the stored basis blocks ----------------
// Blocks are n x p row-major, 1 <= p <= MULTI_MAX; stored block k starts at V + k * vstride.  As for block CG: LDS-staged tiles of whole
// rows, tile tb = blockIdx.x, blockIdx.x + gridDim.x, ..., no atomics, plain FP64 multiplies and adds in a fixed order.
constexpr int BGM_SG = 4; // stored blocks of one group of k_bgmres_project: BGM_SG x 4 accumulators per thread

// Projection: the owner-masked partial sums of V_k^T W (p x p each) for K stored blocks in one launch.  The stored blocks are taken in
// groups of BGM_SG: for a group the workgroup walks its tiles once, stages the W tile ONCE and the group's V tiles beside it (rows
// that are not owned as zeros), and thread (s, o) -- the layout of k_bcg_gram_partial -- keeps the 2 x 2 output block o of every
// block of the group in registers for the tile rows s, s + NS, ...  The slices are summed in ascending s through LDS.
// partial[(((k * p + i) * p + j) * gridDim.x + b] = workgroup b's sum for entry (i, j) of V_k^T W: the layout k_reduce_final_multi sums.
template <bool MASKED>
__global__ __launch_bounds__(WG) void k_bgmres_project(int64_t n, int p, int K, const uint8_t *__restrict__ mask, const double *__restrict__ V,
                                                       int64_t vstride, const double *__restrict__ W, double *__restrict__ partial)
{
  __shared__ double lds[(BGM_SG + 1) * BCG_TILE];
  const int mp = (p + 1) & ~1, hb = mp >> 1, NO = hb * hb, NS = WG / NO, TR = BCG_TILE / mp;
  const int t = threadIdx.x;
  const int s = t / NO, o = t - s * NO, oi = o / hb, oj = o - oi * hb;
  const int64_t ntile = (n + TR - 1) / TR;
  for (int k0 = 0; k0 < K; k0 += BGM_SG) {
    const int ng = K - k0 < BGM_SG ? K - k0 : BGM_SG;
    double acc[BGM_SG][4];
#pragma unroll
    for (int g = 0; g < BGM_SG; ++g)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[g][k] = 0.0;
    __syncthreads(); // the sums of the previous group have been read
    if (mp != p)
      for (int r = t; r < TR; r += WG)
#pragma unroll
        for (int g = 0; g <= BGM_SG; ++g) lds[g * BCG_TILE + r * mp + p] = 0.0; // (no staging loop writes the pad column)
    for (int64_t tb = blockIdx.x; tb < ntile; tb += gridDim.x) {
      const int64_t r0 = tb * TR;
      const int rows = (int)(n - r0 < TR ? n - r0 : TR);
      __syncthreads(); // the previous tile is no longer read
      for (int e = t; e < rows * p; e += WG) {
        const int r = e / p, l = r * mp + (e - r * p);
        const int64_t gi = r0 * p + e;
        const bool own = !MASKED || mask[r0 + r];
        lds[l] = own ? W[gi] : 0.0;
#pragma unroll
        for (int g = 0; g < BGM_SG; ++g)
          if (g < ng) lds[(g + 1) * BCG_TILE + l] = own ? V[(int64_t)(k0 + g) * vstride + gi] : 0.0;
      }
      __syncthreads();
      if (s < NS)
        for (int r = s; r < rows; r += NS) {
          const double *w = lds + r * mp + 2 * oj;
          const double w0 = w[0], w1 = w[1];
#pragma unroll
          for (int g = 0; g < BGM_SG; ++g)
            if (g < ng) {
              const double *v = lds + (g + 1) * BCG_TILE + r * mp + 2 * oi;
              const double v0 = v[0], v1 = v[1];
              acc[g][0] += v0 * w0;
              acc[g][1] += v0 * w1;
              acc[g][2] += v1 * w0;
              acc[g][3] += v1 * w1;
            }
        }
    }
    __syncthreads(); // the tiles are done with: their LDS takes the accumulators, thread t's at 4 BGM_SG t
#pragma unroll
    for (int g = 0; g < BGM_SG; ++g)
#pragma unroll
      for (int k = 0; k < 4; ++k) lds[t * (4 * BGM_SG) + g * 4 + k] = s < NS ? acc[g][k] : 0.0;
    __syncthreads();
    for (int idx = t; idx < NO * 4 * BGM_SG; idx += WG) {
      const int oo = idx / (4 * BGM_SG), rem = idx - oo * (4 * BGM_SG), g = rem >> 2, k = rem & 3;
      if (g >= ng) continue;
      double sum = 0.0;
      for (int ss = 0; ss < NS; ++ss) sum += lds[(ss * NO + oo) * (4 * BGM_SG) + rem];
      const int i = 2 * (oo / hb) + (k >> 1), j = 2 * (oo % hb) + (k & 1);
      if (i < p && j < p) partial[((int64_t)((k0 + g) * p + i) * p + j) * gridDim.x + blockIdx.x] = sum;
    }
  }
}

// Combination: Out (n x q) = (MODE 0) / += (1) / -= (2) sum_k V_k (n x pin) C_k (pin x q), the K coefficient blocks row-major one after
// the other in device memory (what k_bgmres_project and k_reduce_final_multi leave behind IS that layout).  A tile is
// TR = min(4 (WG / q), BCG_TILE / pin') rows (pin' = pin rounded up to even); thread t < (WG / q) q owns column c = t % q of the
// rows t / q + i (WG / q), i < 4, of every tile.  Per stored block the V tile and C_k are staged; per entry the products are summed in
// ascending k, then ascending row of C_k, and the sum is then applied to Out.  Out must not overlap a stored block.
// GRAM (MODE 2, pin == q == p): the owner-masked partial sums of Out^T Out (p x p, the new Out) from the same pass, summed as
// k_bgmres_project sums one block: partial[((i * p + j) * gridDim.x + b].
template <int MODE, bool GRAM, bool MASKED>
__global__ __launch_bounds__(WG) void k_bgmres_combine(int64_t n, int pin, int q, int K, const double *__restrict__ V, int64_t vstride,
                                                       const double *__restrict__ coef, const uint8_t *__restrict__ mask, double *__restrict__ Out,
                                                       double *__restrict__ partial)
{
  __shared__ double Vt[BCG_TILE], Ck[MULTI_MAX * MULTI_MAX], Ot[GRAM ? BCG_TILE : 1];
  const int QR = WG / q, pe = (pin + 1) & ~1;
  const int TR = 4 * QR < BCG_TILE / pe ? 4 * QR : BCG_TILE / pe;
  const int t = threadIdx.x, r = t / q, c = t - r * q;
  const bool on = r < QR;
  // (GRAM) the layout of k_bcg_gram_partial on the Out tile
  const int mp = (q + 1) & ~1, hb = mp >> 1, NO = hb * hb, NS = WG / NO;
  const int s = t / NO, o = t - s * NO, oi = o / hb, oj = o - oi * hb;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (GRAM && mp != q)
    for (int rr = t; rr < TR; rr += WG) Ot[rr * mp + q] = 0.0; // (the pad column is never written again)
  const int64_t ntile = (n + TR - 1) / TR;
  for (int64_t tb = blockIdx.x; tb < ntile; tb += gridDim.x) {
    const int64_t r0 = tb * TR;
    const int rows = (int)(n - r0 < TR ? n - r0 : TR);
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < K; ++k) {
      __syncthreads(); // the previous V tile and C_k (and, GRAM, the previous Out tile) are no longer read
      const double *vk = V + (int64_t)k * vstride + r0 * pin;
      for (int e = t; e < rows * pin; e += WG) Vt[e] = vk[e];
      for (int e = t; e < pin * q; e += WG) Ck[e] = coef[(int64_t)k * pin * q + e];
      __syncthreads();
      if (on)
        for (int j = 0; j < pin; ++j) {
          const double a = Ck[j * q + c];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int rr = r + i * QR;
            if (rr < rows) sum[i] += Vt[rr * pin + j] * a;
          }
        }
    }
    if (on) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rr = r + i * QR;
        if (rr < rows) {
          const int64_t g = (r0 + rr) * q + c;
          const double v = MODE == 0 ? sum[i] : MODE == 1 ? Out[g] + sum[i] : Out[g] - sum[i];
          Out[g] = v;
          if (GRAM) Ot[rr * mp + c] = (!MASKED || mask[r0 + rr]) ? v : 0.0;
        }
      }
    }
    if (GRAM) {
      __syncthreads();
      if (s < NS)
        for (int rr = s; rr < rows; rr += NS) {
          const double *u = Ot + rr * mp + 2 * oi, *w = Ot + rr * mp + 2 * oj;
          const double u0 = u[0], u1 = u[1], w0 = w[0], w1 = w[1];
          acc[0] += u0 * w0;
          acc[1] += u0 * w1;
          acc[2] += u1 * w0;
          acc[3] += u1 * w1;
        }
    }
  }
  if (GRAM) {
    __syncthreads(); // the tiles are done with: Vt takes the accumulators, thread t's at 4 t
#pragma unroll
    for (int k = 0; k < 4; ++k) Vt[t * 4 + k] = s < NS ? acc[k] : 0.0;
    __syncthreads();
    for (int idx = t; idx < NO * 4; idx += WG) {
      const int oo = idx >> 2, k = idx & 3;
      double tot = 0.0;
      for (int ss = 0; ss < NS; ++ss) tot += Vt[(ss * NO + oo) * 4 + k];
      const int i = 2 * (oo / hb) + (k >> 1), j = 2 * (oo % hb) + (k & 1);
      if (i < q && j < q) partial[((int64_t)(i * q + j)) * gridDim.x + blockIdx.x] = tot;
    }
  }
}

} // namespace ddm
