// Device kernels of the two-level Schwarz hot path (gfx950 / CDNA4, wave64).
// All kernels are HBM-bandwidth or dependency-latency bound FP64 streaming kernels; none is
// GEMM-shaped, so no MFMA here (DESIGN.md section "Kernels").  Launch wrappers are at the
// bottom; every wrapper enqueues on the given stream and never synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ddm {

constexpr int WG = 256;          // 4 waves of 64
constexpr int SPMV_NNZ = 2048;   // non-zeros staged in LDS per workgroup (16 KiB of products)
constexpr int RED_MAX_BLOCKS = 1024;
constexpr int RED_TRIPS = 4;     // grid-stride trips of k_dot_partial whose loads are issued together

// bijective XCD-aware remap (cdna_hip_programming.md T1): consecutive work items of one XCD
// become contiguous, so each XCD's L2 sees one contiguous slab of the matrix / x vector.
__device__ __forceinline__ int xcd_remap(int orig, int nwg)
{
  const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// block-wide sum in a fixed order; result valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *lds4)
{
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) lds4[w] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) r = (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
  __syncthreads();
  return r;
}

// ---------------------------------------------------------------------------------------------
// K1 / K11: CSR SpMV, "CSR-stream": a workgroup owns a block of consecutive rows holding at most
// SPMV_NNZ non-zeros; values / column indices are read fully coalesced, the products are staged
// in LDS and each row is then summed sequentially in column order (deterministic).
// reference: BCRSMatrix::mv / usmv at nonoverlapping_operator.hh:37,47; spectra.hh:100-105.
// The rows [r0, r1) of one such block, by one workgroup (prod: SPMV_NNZ doubles of LDS, red: 4).
template <bool ACC>
__device__ __forceinline__ void spmv_stream_block(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                  const double *__restrict__ va, int r0, int r1, const double *__restrict__ x,
                                                  double *__restrict__ y, double alpha, double *prod, double *red)
{
  const int64_t z0 = rp[r0], z1 = rp[r1];
  const int64_t nz = z1 - z0;
  if (nz > SPMV_NNZ) { // a single long row: strided partial sums + block reduction
    double s = 0.0;
    for (int64_t k = z0 + threadIdx.x; k < z1; k += WG) s += va[k] * x[ci[k]];
    s = block_sum(s, red);
    if (threadIdx.x == 0) y[r0] = ACC ? y[r0] + alpha * s : s;
    return;
  }
  // all loads of a thread are issued before the first one is needed: indices past the block's end are clamped (loaded, not
  // stored) instead of branched around, so that nothing serialises the SPMV_NNZ / WG independent load -> gather chains
  constexpr int U = SPMV_NNZ / WG;
  const int last = (int)nz - 1;
  if (last >= 0) {
    int32_t c[U];
    double v[U], xv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) c[u] = ci[z0 + min((int)threadIdx.x + u * WG, last)];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = va[z0 + min((int)threadIdx.x + u * WG, last)];
#pragma unroll
    for (int u = 0; u < U; ++u) xv[u] = x[c[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = threadIdx.x + u * WG;
      if (k <= last) prod[k] = v[u] * xv[u];
    }
  }
  __syncthreads();
  const int r = r0 + threadIdx.x;
  if (r < r1) {
    const int k0 = (int)(rp[r] - z0), k1 = (int)(rp[r + 1] - z0);
    double s = 0.0;
    for (int kb = k0; kb < k1; kb += 8) { // eight LDS reads in flight, summed in column order
      double q[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) q[j] = prod[min(kb + j, k1 - 1)];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (kb + j < k1) s += q[j];
    }
    y[r] = ACC ? y[r] + alpha * s : s;
  }
}
template <bool ACC>
__global__ __launch_bounds__(WG) void k_spmv_stream(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                     const double *__restrict__ va, const int32_t *__restrict__ blk_row,
                                                     int nblk, const double *__restrict__ x, double *__restrict__ y,
                                                     double alpha)
{
  __shared__ double prod[SPMV_NNZ];
  __shared__ double red[4];
  const int b = xcd_remap(blockIdx.x, nblk);
  spmv_stream_block<ACC>(rp, ci, va, blk_row[b], blk_row[b + 1], x, y, alpha, prod, red);
}

// K1d: the operator product (ddm_op) on diagonal row blocks (layout: dia_build, csr.hpp).  A block of at most WG consecutive rows
// whose entries lie on at most DIA_MAX distinct diagonals (col - row) stores no column indices.  Consecutive blocks form a segment
// with one table record in tab (per diagonal k, ascending: the offset, the slab that holds its values, a row shift) and
// segment-wide value slabs val[slab * rows + row], so a wave reads 512 contiguous bytes per diagonal; a row has a presence mask.
// A symmetric segment keeps the slabs of the offsets >= 0 only: a diagonal below reads the slab of the mirrored offset at the
// partner's row (shift = offset), elsewhere shift = 0.  One thread per row: the value and x loads of DIA_CH diagonals are issued
// before the first use (indices clamped, not branched around), then the present entries are added for ascending k, product
// rounded before the sum -- the operations of k_spmv_stream in its order, hence the same bits.  Absent entries are skipped (not
// added as zero), a stored 0.0 is present.  Blocks that fit no diagonal layout (nd == 0) are CSR-stream blocks of the same
// launch: a uniform branch per workgroup.  5 waves per SIMD (87 VGPRs allow them): the slab branches run as fast with 4, the coded
// branch below 12 % faster with 5; at the default target of 8 the scheduler interleaves loads and uses to save registers and spills.
// Build (with the staged and coded branches below): 87 VGPRs, 78 SGPRs, 0 scratch, 16 544 B LDS.
constexpr int DIA_MAX = 32;  // diagonals of a block (bits of the mask)
constexpr int DIA_CH = 16;   // diagonals whose loads are in flight together; DIA_MAX is a multiple
// Staged blocks (a flag of the segment's record; a third uniform branch): the x entries a block of WG rows reads on neighbouring
// diagonals overlap -- on a 108-wide box the 27 offsets are three runs of span 218 -- so the workgroup loads each run's window
// x[r0 + first ... + WG + span) once, coalesced, into the LDS array the CSR-stream branch owns (DIA_WIN doubles; 1 422 of them at
// 216^3), and thread t reads x[r + off[k]] at win[lds_pos[k] + t]: 28 value + 6 window loads per thread instead of 27 + 27, all
// issued before the one barrier, and the address unit (busy 85 % of the kernel's time before) handles 21 wavefront loads fewer per
// 55.  Same products in the same order, so the same bits; window elements outside the vector are clamped (loaded, never added).
// Segments whose windows exceed DIA_WIN keep the body above.
constexpr int DIA_WIN = SPMV_NNZ;      // doubles of x windows a staged block may hold: the prod array
constexpr int DIA_RUNS = DIA_WIN / WG; // runs of a staged segment at most: every run owns at least WG doubles
// a segment's record in tab: four rows of DIA_MAX (offset, slab, row shift, window position of thread 0), then the staged flag,
// the run count and the doubles of all windows, then three rows of DIA_RUNS (first offset, doubles, window position of each run)
constexpr int DIA_TAB_OFF = 0, DIA_TAB_SLAB = DIA_MAX, DIA_TAB_SHIFT = 2 * DIA_MAX, DIA_TAB_POS = 3 * DIA_MAX;
constexpr int DIA_TAB_STAGED = 4 * DIA_MAX, DIA_TAB_NRUNS = DIA_TAB_STAGED + 1, DIA_TAB_WINDOW = DIA_TAB_STAGED + 2;
constexpr int DIA_TAB_RFIRST = DIA_TAB_STAGED + 4, DIA_TAB_RLEN = DIA_TAB_RFIRST + DIA_RUNS, DIA_TAB_RSTART = DIA_TAB_RLEN + DIA_RUNS;
constexpr int DIA_REC = (DIA_TAB_RSTART + DIA_RUNS + 15) / 16 * 16;
static_assert(DIA_RUNS == 8 && DIA_TAB_RFIRST % 4 == 0, "the run rows are read as two int4 each");
// Coded blocks (dict >= 0; a fourth uniform branch, staged segments only): on a structured grid the values of a block repeat, so
// dia_build stores the at most DIA_DICT distinct bit patterns of a block once and a 4-bit code per (row, diagonal): a row's codes
// are one 16-byte word, nibble k for diagonal k.  The thread issues the code word, the mask and the window loads before the first
// wait (the first wave also the dictionary, which it copies into DIA_DICT doubles of LDS beside the windows), and after the one
// barrier adds dict[code_k] * win[lds_pos[k] + t] for ascending k with the mask bit set: the same doubles in the same order as the
// slab branch, so the same bits, from 8 vector loads per thread instead of 34 and about 36 B of memory per row instead of 139.
// The 16 dictionary entries lie on 32 distinct banks and equal addresses are broadcast, so the reads are conflict-free.
constexpr int DIA_DICT = 16;      // doubles of a block's dictionary
constexpr int DIA_CODE_WORDS = 4; // 32-bit words of a row's codes: DIA_MAX nibbles
static_assert(DIA_CODE_WORDS * 8 == DIA_MAX && DIA_DICT == 16, "a nibble per diagonal");
struct DiaBlock {
  int64_t base;       // slot of (slab 0, row r0) in val
  int32_t r0, r1;     // rows
  int32_t nd, tab;    // diagonals (0: CSR-stream block) and the place of the segment's table in tab
  int32_t t0, stride; // r0's place in the segment; rows of the segment = distance of two slabs
  int32_t dict, pad;  // number of the block's dictionary (DIA_DICT doubles each), -1: not coded
};
__device__ __forceinline__ void dia_load_chunk(const int32_t *__restrict__ p, int (&o)[DIA_CH])
{
  const int4 *__restrict__ q = reinterpret_cast<const int4 *>(p);
  const int4 a = q[0], b = q[1], c = q[2], d = q[3];
  o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w, o[4] = b.x, o[5] = b.y, o[6] = b.z, o[7] = b.w;
  o[8] = c.x, o[9] = c.y, o[10] = c.z, o[11] = c.w, o[12] = d.x, o[13] = d.y, o[14] = d.z, o[15] = d.w;
}
// The x windows of a staged block into win (DIA_WIN doubles of LDS): element e of the array belongs to the last run that starts at
// or before e, and is x[r0 + first + (e - start)].  A run is at least WG long, so the WG elements of one trip lie in at most two
// runs: which two is a scalar computation.  All loads are issued before the first store; the caller's barrier follows.
__device__ __forceinline__ void dia_stage_windows(const int32_t *__restrict__ rec, int r0, int n, const double *__restrict__ x, double *win)
{
  const int4 *__restrict__ rq = reinterpret_cast<const int4 *>(rec + DIA_TAB_RFIRST);
  const int4 f0 = rq[0], f1 = rq[1], s0 = rq[4], s1 = rq[5];
  const int rfirst[DIA_RUNS] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w}, rstart[DIA_RUNS] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  const int nwin = rec[DIA_TAB_WINDOW];
  double xw[DIA_RUNS];
#pragma unroll
  for (int u = 0; u < DIA_RUNS; ++u)
    if (u * WG < nwin) {
      int d0 = rfirst[0] - rstart[0], d1 = d0, split = DIA_WIN;
#pragma unroll
      for (int j = DIA_RUNS - 1; j >= 1; --j)
        if (rstart[j] > u * WG) split = rstart[j], d1 = rfirst[j] - rstart[j];
#pragma unroll
      for (int j = 1; j < DIA_RUNS; ++j)
        if (rstart[j] <= u * WG) d0 = rfirst[j] - rstart[j];
      const int e = u * WG + (int)threadIdx.x;
      xw[u] = x[min(max(r0 + e + (e < split ? d0 : d1), 0), n - 1)];
    }
#pragma unroll
  for (int u = 0; u < DIA_RUNS; ++u)
    if (u * WG < nwin && u * WG + (int)threadIdx.x < nwin) win[u * WG + threadIdx.x] = xw[u];
}
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(5, 5))) void k_spmv_dia(const DiaBlock *__restrict__ blk, int nblk, const int32_t *__restrict__ tab,
                                                  const uint32_t *__restrict__ mask, const double *__restrict__ val,
                                                  const uint4 *__restrict__ code, const double *__restrict__ dict,
                                                  const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                  const double *__restrict__ va, int n, const double *__restrict__ x,
                                                  double *__restrict__ y)
{
  __shared__ double prod[SPMV_NNZ];
  __shared__ double red[4];
  __shared__ double dct[DIA_DICT];
  const DiaBlock B = blk[xcd_remap(blockIdx.x, nblk)];
  if (B.nd == 0) {
    spmv_stream_block<false>(rp, ci, va, B.r0, B.r1, x, y, 0.0, prod, red);
    return;
  }
  const int nr = B.r1 - B.r0, t = min((int)threadIdx.x, nr - 1), r = B.r0 + t;
  const uint32_t m = mask[r];
  double s = 0.0;
  const int32_t *__restrict__ rec = tab + B.tab;
  if (B.dict >= 0) {
    const uint4 cw = code[r];
    double dv = 0.0;
    if (threadIdx.x < 64) dv = dict[(int64_t)B.dict * DIA_DICT + (threadIdx.x & (DIA_DICT - 1))]; // (the first wave)
    dia_stage_windows(rec, B.r0, n, x, prod);
    if (threadIdx.x < DIA_DICT) dct[threadIdx.x] = dv;
    __syncthreads();
    const uint32_t cwd[DIA_CODE_WORDS] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
    for (int k0 = 0; k0 < DIA_MAX; k0 += DIA_CH)
      if (k0 < B.nd) {
        int pos[DIA_CH];
        dia_load_chunk(rec + DIA_TAB_POS + k0, pos);
#pragma unroll
        for (int g = 0; g < DIA_CH; g += 4)
          if (k0 + g < B.nd) {
            double w[4], v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int k = k0 + g + u;
              w[u] = prod[pos[g + u] + t];
              v[u] = dct[(cwd[k / 8] >> (4 * (k % 8))) & (DIA_DICT - 1)];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if ((m >> (k0 + g + u)) & 1u) s = __dadd_rn(s, __dmul_rn(v[u], w[u]));
          }
      }
    if ((int)threadIdx.x < nr) y[r] = s;
    return;
  }
  const int ts = B.t0 + t;
  const double *__restrict__ vs = val + (B.base - B.t0);
  if (rec[DIA_TAB_STAGED]) {
    // values first (groups of four behind a uniform test, so that 27 diagonals cost 28 loads)
    double v[DIA_MAX];
#pragma unroll
    for (int k0 = 0; k0 < DIA_MAX; k0 += DIA_CH)
      if (k0 < B.nd) {
        int slab[DIA_CH], shift[DIA_CH];
        dia_load_chunk(rec + DIA_TAB_SLAB + k0, slab);
        dia_load_chunk(rec + DIA_TAB_SHIFT + k0, shift);
#pragma unroll
        for (int g = 0; g < DIA_CH; g += 4)
          if (k0 + g < B.nd) {
#pragma unroll
            for (int u = g; u < g + 4; ++u) v[k0 + u] = vs[(int64_t)slab[u] * B.stride + min(max(ts + shift[u], 0), B.stride - 1)];
          }
      }
    dia_stage_windows(rec, B.r0, n, x, prod);
    __syncthreads();
#pragma unroll
    for (int k0 = 0; k0 < DIA_MAX; k0 += DIA_CH)
      if (k0 < B.nd) {
        int pos[DIA_CH];
        dia_load_chunk(rec + DIA_TAB_POS + k0, pos);
#pragma unroll
        for (int g = 0; g < DIA_CH; g += 4)
          if (k0 + g < B.nd) {
            double w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = prod[pos[g + u] + t];
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if ((m >> (k0 + g + u)) & 1u) s = __dadd_rn(s, __dmul_rn(v[k0 + g + u], w[u]));
          }
      }
    if ((int)threadIdx.x < nr) y[r] = s;
    return;
  }
  for (int k0 = 0; k0 < B.nd; k0 += DIA_CH) {
    // the chunk's offsets, slab numbers and row shifts in three scalar loads (the tables are DIA_MAX long, the tail repeats the last entry)
    int off[DIA_CH], slab[DIA_CH], shift[DIA_CH];
    dia_load_chunk(tab + B.tab + k0, off);
    dia_load_chunk(tab + B.tab + DIA_MAX + k0, slab);
    dia_load_chunk(tab + B.tab + 2 * DIA_MAX + k0, shift);
    double v[DIA_CH], xv[DIA_CH];
#pragma unroll
    for (int u = 0; u < DIA_CH; ++u) {
      v[u] = vs[(int64_t)slab[u] * B.stride + min(max(ts + shift[u], 0), B.stride - 1)];
      xv[u] = x[min(max(r + off[u], 0), n - 1)];
    }
    const uint32_t mk = m >> k0; // (no bit at or above nd is set: the clamped loads past the last diagonal are never added)
#pragma unroll
    for (int u = 0; u < DIA_CH; ++u)
      if ((mk >> u) & 1u) s = __dadd_rn(s, __dmul_rn(v[u], xv[u]));
  }
  if ((int)threadIdx.x < nr) y[r] = s;
}

// ---------------------------------------------------------------------------------------------
// K3: level-scheduled sparse triangular solves with the ILU(0) factors (schwarz.hh:133).
// Rows of one level are independent; their entries are stored level-by-level in sliced-ELL
// (column-major inside the level) so that a thread-per-row kernel reads them coalesced and sums
// them in the same column order as the sequential back-solve.
// One row of a level: all column indices / values of the row are loaded first, then all x
// gathers are issued together (memory-level parallelism: two dependent round trips per level
// instead of two per entry), then the products are subtracted in column order.
constexpr int TRSV_UNROLL = 16;
template <class IDX>
__device__ __forceinline__ double trsv_row_sum(double s, int w, IDX m, IDX r, const int32_t *__restrict__ cols,
                                               const double *__restrict__ vals, const double *x)
{
  for (int k0 = 0; k0 < w; k0 += TRSV_UNROLL) {
    int32_t c[TRSV_UNROLL];
    double v[TRSV_UNROLL], xv[TRSV_UNROLL];
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) {
      const bool ok = k0 + u < w;
      c[u] = ok ? cols[(IDX)(k0 + u) * m + r] : -1;
      v[u] = ok ? vals[(IDX)(k0 + u) * m + r] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) xv[u] = c[u] >= 0 ? x[c[u]] : 0.0;
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) s -= v[u] * xv[u];
  }
  return s;
}

__global__ __launch_bounds__(WG) void k_trsv_lower_level(int m, int w, const int32_t *__restrict__ rows,
                                                          const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                                          const double *__restrict__ d, double *x)
{
  const int r = blockIdx.x * WG + threadIdx.x;
  if (r >= m) return;
  const int row = rows[r];
  x[row] = trsv_row_sum<int64_t>(d[row], w, m, r, cols, vals, x);
}

__global__ __launch_bounds__(WG) void k_trsv_upper_level(int m, int w, const int32_t *__restrict__ rows,
                                                          const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                                          const double *__restrict__ dinv, double *x)
{
  const int r = blockIdx.x * WG + threadIdx.x;
  if (r >= m) return;
  const int row = rows[r];
  x[row] = trsv_row_sum<int64_t>(x[row], w, m, r, cols, vals, x) * dinv[r];
}

// Multi-right-hand-side variants (GenEO setup: block eigensolver; cf. the reference's own
// multi-RHS triangular solve, eigensolvers/umfpack.hh:131-197).  Block vectors are row-major
// n x nrhs, a thread owns one (row, rhs) pair; the nrhs lanes of a row read the same factor
// entries (broadcast) and gather nrhs consecutive doubles of x (coalesced).
template <class IDX>
__device__ __forceinline__ double trsv_row_sum_multi(double s, int w, IDX m, IDX r, int64_t nrhs, int j,
                                                     const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                                     const double *x)
{
  for (int k0 = 0; k0 < w; k0 += TRSV_UNROLL) {
    int32_t c[TRSV_UNROLL];
    double v[TRSV_UNROLL], xv[TRSV_UNROLL];
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) {
      const bool ok = k0 + u < w;
      c[u] = ok ? cols[(IDX)(k0 + u) * m + r] : -1;
      v[u] = ok ? vals[(IDX)(k0 + u) * m + r] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) xv[u] = c[u] >= 0 ? x[(int64_t)c[u] * nrhs + j] : 0.0;
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) s -= v[u] * xv[u];
  }
  return s;
}

// ldd / ldx: leading dimensions of the row-major blocks d and x (>= nrhs)
template <bool UPPER>
__global__ __launch_bounds__(WG) void k_trsv_level_multi(int m, int w, int nrhs, const int32_t *__restrict__ rows,
                                                          const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                                          const double *__restrict__ dinv, const double *__restrict__ d, int64_t ldd, double *x, int64_t ldx)
{
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  const int r = (int)(t / nrhs);
  if (r >= m) return;
  const int j = (int)(t - (int64_t)r * nrhs);
  const int64_t o = (int64_t)rows[r] * ldx + j;
  const double s = trsv_row_sum_multi<int64_t>(UPPER ? x[o] : d[(int64_t)rows[r] * ldd + j], w, m, r, ldx, j, cols, vals, x);
  x[o] = UPPER ? s * dinv[r] : s;
}
// nrhs % 4 == 0 and 32-byte aligned rows: one thread per (row, group of 4 right-hand sides) -- a quarter of the index / value /
// gather instructions and wavefronts per level (the 24-column solves of the block eigensolver move 27 GB of gathered x rows per
// triangle through the caches at 216^3: the large levels are throughput-bound).  Same sums in the same order as the scalar kernel.
template <bool UPPER>
__global__ __launch_bounds__(WG) void k_trsv_level_multi4(int m, int w, int nq /* nrhs / 4 */, const int32_t *__restrict__ rows,
                                                           const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                                           const double *__restrict__ dinv, const double *__restrict__ d, int64_t ldd, double *x, int64_t ldx)
{
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  const int r = (int)(t / nq);
  if (r >= m) return;
  const int j = 4 * (int)(t - (int64_t)r * nq);
  const int64_t o = (int64_t)rows[r] * ldx + j;
  d4 s = UPPER ? *reinterpret_cast<const d4 *>(x + o) : *reinterpret_cast<const d4 *>(d + (int64_t)rows[r] * ldd + j);
  for (int k0 = 0; k0 < w; k0 += TRSV_UNROLL) {
    int32_t c[TRSV_UNROLL];
    double v[TRSV_UNROLL];
    d4 xv[TRSV_UNROLL];
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) {
      const bool ok = k0 + u < w;
      c[u] = ok ? cols[(int64_t)(k0 + u) * m + r] : -1;
      v[u] = ok ? vals[(int64_t)(k0 + u) * m + r] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) xv[u] = c[u] >= 0 ? *reinterpret_cast<const d4 *>(x + (int64_t)c[u] * ldx + j) : d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) s -= v[u] * xv[u];
  }
  if (UPPER) s *= dinv[r];
  *reinterpret_cast<d4 *>(x + o) = s;
}
// SINGLE-PRECISION sweeps for uses where the triangular solve is a PRECONDITIONER inside an iteration that only needs a fixed, good
// search direction (the block eigensolver of the GenEO setup: W = T r): factor entries and the work block in float -- half the bytes of
// the gathered x rows, which is what the 24-column level solves are bound by -- right-hand side read and result written in double.
// One thread per (row, 4 right-hand sides); xf: n x nrhs floats (ld = nrhs).
__global__ void k_to_float(int64_t n, const double *__restrict__ src, float *__restrict__ dst)
{
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t < n) dst[t] = (float)src[t];
}
template <bool UPPER>
__global__ __launch_bounds__(WG) void k_trsv_level_multi4_f32(int m, int w, int nq /* nrhs / 4 */, const int32_t *__restrict__ rows, const int32_t *__restrict__ cols,
                                                               const float *__restrict__ vals, const float *__restrict__ dinv, const double *__restrict__ d, int64_t ldd,
                                                               float *xf, int64_t ldf, double *__restrict__ xout, int64_t ldx)
{
  typedef float f4 __attribute__((ext_vector_type(4)));
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  const int r = (int)(t / nq);
  if (r >= m) return;
  const int j = 4 * (int)(t - (int64_t)r * nq);
  const int64_t row = rows[r], o = row * ldf + j;
  f4 s;
  if (UPPER) s = *reinterpret_cast<const f4 *>(xf + o);
  else {
    const d4 dv = *reinterpret_cast<const d4 *>(d + row * ldd + j);
    s = f4{(float)dv[0], (float)dv[1], (float)dv[2], (float)dv[3]};
  }
  for (int k0 = 0; k0 < w; k0 += TRSV_UNROLL) {
    int32_t c[TRSV_UNROLL];
    float v[TRSV_UNROLL];
    f4 xv[TRSV_UNROLL];
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) {
      const bool ok = k0 + u < w;
      c[u] = ok ? cols[(int64_t)(k0 + u) * m + r] : -1;
      v[u] = ok ? vals[(int64_t)(k0 + u) * m + r] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) xv[u] = c[u] >= 0 ? *reinterpret_cast<const f4 *>(xf + (int64_t)c[u] * ldf + j) : f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) s -= v[u] * xv[u];
  }
  if (UPPER) {
    s *= dinv[r];
    *reinterpret_cast<d4 *>(xout + row * ldx + j) = d4{(double)s[0], (double)s[1], (double)s[2], (double)s[3]};
  }
  *reinterpret_cast<f4 *>(xf + o) = s;
}
// The same for levels of WIDE rows (factors of the sparse direct solver: separator rows have thousands of entries and a
// level often holds a single row): one workgroup per row, the 256 threads split the row's entries into 256 / nrhs slices
// per right-hand side, slice sums meet in LDS and are added in slice order (deterministic).
template <bool UPPER>
__global__ __launch_bounds__(WG) void k_trsv_level_multi_wide(int m, int w, int nrhs, const int32_t *__restrict__ rows,
                                                               const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                                               const double *__restrict__ dinv, const double *__restrict__ d, int64_t ldd, double *x, int64_t ldx)
{
  __shared__ double part[WG];
  const int r = blockIdx.x;
  const int nsl = WG / nrhs;
  const int sl = threadIdx.x / nrhs, j = threadIdx.x - sl * nrhs;
  double s = 0.0;
  if (sl < nsl)
    for (int k = sl; k < w; k += nsl) {
      const double v = vals[(int64_t)k * m + r];
      s += v * x[(int64_t)cols[(int64_t)k * m + r] * ldx + j];
    }
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < nrhs) {
    const int64_t o = (int64_t)rows[r] * ldx + threadIdx.x;
    double acc = UPPER ? x[o] : d[(int64_t)rows[r] * ldd + threadIdx.x];
    for (int q = 0; q < nsl; ++q) acc -= part[q * nrhs + threadIdx.x];
    x[o] = UPPER ? acc * dinv[r] : acc;
  }
}

// Y = A X for row-major block vectors (n x nrhs): one thread per (row, rhs)
__global__ __launch_bounds__(WG) void k_spmm_rowmajor(int64_t n, int nrhs, const int64_t *__restrict__ rp,
                                                       const int32_t *__restrict__ ci, const double *__restrict__ va,
                                                       const double *__restrict__ x, int64_t ldx, double *__restrict__ y, int64_t ldy)
{
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  const int64_t row = t / nrhs;
  if (row >= n) return;
  const int j = (int)(t - row * nrhs);
  const int64_t k0 = rp[row], k1 = rp[row + 1];
  double s = 0.0;
  for (int64_t kb = k0; kb < k1; kb += 8) {
    int32_t c[8];
    double v[8], xv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool ok = kb + u < k1;
      c[u] = ok ? ci[kb + u] : -1;
      v[u] = ok ? va[kb + u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) xv[u] = c[u] >= 0 ? x[(int64_t)c[u] * ldx + j] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u] * xv[u];
  }
  y[row * ldy + j] = s;
}

// The same for nrhs % 4 == 0 and 32-byte aligned rows: one thread per (row, group of 4 columns) -- a quarter of the index / value /
// gather instructions per product; optionally TWO matrices on one pattern (va2, y2: the pencil matrices A~ and C~ of the block
// eigensolver share their pattern), which reads the block X once for both products.  Row sums in entry order, as above.
template <bool TWO>
__global__ __launch_bounds__(WG) void k_spmm_rowmajor4(int64_t n, int nq /* nrhs / 4 */, const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                        const double *__restrict__ va, const double *__restrict__ va2, const double *__restrict__ x, int64_t ldx,
                                                        double *__restrict__ y, double *__restrict__ y2, int64_t ldy)
{
  typedef double d4 __attribute__((ext_vector_type(4)));
  // (An XCD-contiguous block order was measured in round 3 and changes nothing: 29.7 GB of L2 fills per call either way, 8.7 ms.  The
  // misses are not the eight L2s duplicating each other but the reuse distance itself -- two grid planes of X rows, 8 MB with the
  // 576-byte row stride of the [X | W | P] array, against 4 MB of L2: every row of X is fetched once per plane.  What would help is a
  // cache-blocked ROW ORDER (bricks instead of planes), i.e. a host-side permutation of the processing order.)
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  const int64_t row = t / nq;
  if (row >= n) return;
  const int j = 4 * (int)(t - row * nq);
  const int64_t k0 = rp[row], k1 = rp[row + 1];
  d4 s = {0.0, 0.0, 0.0, 0.0}, s2 = {0.0, 0.0, 0.0, 0.0};
  for (int64_t kb = k0; kb < k1; kb += 4) {
    int32_t c[4];
    double v[4], w[4];
    d4 xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool ok = kb + u < k1;
      c[u] = ok ? ci[kb + u] : -1;
      v[u] = ok ? va[kb + u] : 0.0;
      if (TWO) w[u] = ok ? va2[kb + u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) xv[u] = c[u] >= 0 ? *reinterpret_cast<const d4 *>(x + (int64_t)c[u] * ldx + j) : d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      s += v[u] * xv[u];
      if (TWO) s2 += w[u] * xv[u];
    }
  }
  *reinterpret_cast<d4 *>(y + row * ldy + j) = s;
  if (TWO) *reinterpret_cast<d4 *>(y2 + row * ldy + j) = s2;
}

// The same product with the rows processed in a CACHE-BLOCKED order (order[]: a permutation of the rows, csr_row_order_tiled): rows of
// a 16 x 4 x 4 brick of a structured grid are neighbours in order[], a workgroup takes 64 of them (blockDim = 64 nq threads), and the
// workgroups of one XCD take a contiguous range of bricks (xcd_remap) -- the 27 gathered X rows of a row are then shared inside the
// brick and with the bricks running beside it on the same L2, instead of being fetched once per grid plane (29.7 GB of L2 fills per
// call for 12 GB of algorithmic traffic with the natural order at 216^3).  Every row is computed as before: same sums, same order.
template <bool TWO>
__global__ __launch_bounds__(512) void k_spmm_rowmajor4_tiled(int64_t n, int nq /* nrhs / 4 */, const int32_t *__restrict__ order, const int64_t *__restrict__ rp,
                                                               const int32_t *__restrict__ ci, const double *__restrict__ va, const double *__restrict__ va2,
                                                               const double *__restrict__ x, int64_t ldx, double *__restrict__ y, double *__restrict__ y2, int64_t ldy)
{
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int rows_per_wg = blockDim.x / nq;
  const int64_t wg = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int lr = threadIdx.x / nq;
  const int64_t pos = wg * rows_per_wg + lr;
  if (lr >= rows_per_wg || pos >= n) return;
  const int64_t row = order[pos];
  const int j = 4 * (threadIdx.x - lr * nq);
  const int64_t k0 = rp[row], k1 = rp[row + 1];
  d4 s = {0.0, 0.0, 0.0, 0.0}, s2 = {0.0, 0.0, 0.0, 0.0};
  constexpr int CH = 8; // entries whose gathers are in flight together (the kernel is bound by these dependent gathers, not by bytes)
  for (int64_t kb = k0; kb < k1; kb += CH) {
    int32_t c[CH];
    double v[CH], w[CH];
    d4 xv[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const bool ok = kb + u < k1;
      c[u] = ok ? ci[kb + u] : -1;
      v[u] = ok ? va[kb + u] : 0.0;
      if (TWO) w[u] = ok ? va2[kb + u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < CH; ++u) xv[u] = c[u] >= 0 ? *reinterpret_cast<const d4 *>(x + (int64_t)c[u] * ldx + j) : d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      s += v[u] * xv[u];
      if (TWO) s2 += w[u] * xv[u];
    }
  }
  *reinterpret_cast<d4 *>(y + row * ldy + j) = s;
  if (TWO) *reinterpret_cast<d4 *>(y2 + row * ldy + j) = s2;
}

// Several consecutive small levels (each <= WG*TRSV_SMALL_ROWS rows) in ONE workgroup: the levels
// are separated by workgroup barriers instead of kernel boundaries.  desc[l] = {m, w, row_off,
// ent_off}.  All data of these levels is produced and consumed by this workgroup only.
struct LevelDesc {
  int32_t m, w;
  int64_t row_off, ent_off;
};
constexpr int TRSV_SMALL_WG = 1024;

template <bool UPPER>
__global__ __launch_bounds__(TRSV_SMALL_WG) void k_trsv_small_levels(int nlev, const LevelDesc *__restrict__ desc,
                                                                      const int32_t *__restrict__ rows,
                                                                      const int32_t *__restrict__ cols,
                                                                      const double *__restrict__ vals,
                                                                      const double *__restrict__ dinv,
                                                                      const double *__restrict__ d, double *x)
{
  for (int l = 0; l < nlev; ++l) {
    const LevelDesc L = desc[l];
    if (L.w >= 32 && 2 * L.m <= TRSV_SMALL_WG) {
      // few wide rows (separator rows of a sparse direct factor: thousands of entries, often one row per level): S lanes
      // of one wavefront share a row, each sums every S-th product, a butterfly adds the S partial sums (fixed order)
      int S = 64;
      while (S * L.m > TRSV_SMALL_WG) S >>= 1;
      const int r = threadIdx.x / S, sl = threadIdx.x - r * S;
      const bool act = r < L.m;
      double s = 0.0;
      if (act) {
        const int32_t *cl = cols + L.ent_off;
        const double *vl = vals + L.ent_off;
        for (int k = sl; k < L.w; k += S) s += vl[(int64_t)k * L.m + r] * x[cl[(int64_t)k * L.m + r]];
      }
      for (int o = S >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (act && sl == 0) {
        const int row = rows[L.row_off + r];
        const double t = (UPPER ? x[row] : d[row]) - s;
        x[row] = UPPER ? t * dinv[L.row_off + r] : t;
      }
    } else {
      for (int r = threadIdx.x; r < L.m; r += TRSV_SMALL_WG) {
        const int row = rows[L.row_off + r];
        const double s = trsv_row_sum<int>(UPPER ? x[row] : d[row], L.w, L.m, r, cols + L.ent_off, vals + L.ent_off, x);
        x[row] = UPPER ? s * dinv[L.row_off + r] : s;
      }
    }
    __syncthreads(); // workgroup-scope release/acquire of the x entries just written
  }
}

// ---------------------------------------------------------------------------------------------
// Level-scheduled triangular solves for factors of the SPARSE DIRECT solver (csrc/sparse_chol_host.hpp).  Their rows differ from
// ILU(0) rows: a level near the root of the elimination tree holds a handful of rows with thousands of entries, a leaf level
// thousands of short rows, and there are thousands of levels -- sliced ELL would pad every level to its longest row.  Layout:
// rows sorted by level, entries of a row contiguous (CSR in level order: lrp); S lanes (a power of two <= 64, chosen per level
// from its row count) share a row, each sums every S-th product, a butterfly adds the S partial sums in a fixed order.
struct CsrLevel {
  int32_t m, S;
  int64_t row_off;
};
template <bool UPPER>
__device__ __forceinline__ void trsv_csr_rows(const CsrLevel L, int first_group, int ngroups_step, int tid, const int32_t *__restrict__ rows,
                                              const int32_t *__restrict__ rhs, const int64_t *__restrict__ lrp, const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                              const double *__restrict__ dinv, const double *__restrict__ d, double *x)
{
  const int S = L.S;
  const int g = tid / S, sl = tid - g * S;
  for (int base = first_group; base < L.m; base += ngroups_step) { // every lane of a wavefront runs the same number of rounds
    const int r = base + g;
    const bool act = r < L.m;
    double s = 0.0;
    if (act) {
      const int64_t k1 = lrp[L.row_off + r + 1];
      // eight entries of the lane in flight: all column and value loads, then all gathers, then the products (in order)
      for (int64_t k = lrp[L.row_off + r] + sl; k < k1; k += 8 * (int64_t)S) {
        int32_t c[8];
        double v[8], xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int64_t kk = k + (int64_t)u * S;
          const bool ok = kk < k1;
          c[u] = ok ? cols[kk] : -1;
          v[u] = ok ? vals[kk] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) xv[u] = c[u] >= 0 ? x[c[u]] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u] * xv[u];
      }
    }
    for (int o = S >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (act && sl == 0) { // rhs: index of the right-hand side (lower sweep: in d; upper sweep: in x, the forward result) or -1
      const int ri = rhs[L.row_off + r];
      const double t = (ri >= 0 ? (UPPER ? x[ri] : d[ri]) : 0.0) - s;
      x[rows[L.row_off + r]] = UPPER ? t * dinv[L.row_off + r] : t;
    }
  }
}
// a run of consecutive small levels in ONE workgroup (levels separated by workgroup barriers)
template <bool UPPER>
__global__ __launch_bounds__(TRSV_SMALL_WG) void k_trsv_csr_fused(int nlev, const CsrLevel *__restrict__ desc, const int32_t *__restrict__ rows,
                                                                   const int32_t *__restrict__ rhs, const int64_t *__restrict__ lrp, const int32_t *__restrict__ cols,
                                                                   const double *__restrict__ vals, const double *__restrict__ dinv,
                                                                   const double *__restrict__ d, double *x)
{
  for (int l = 0; l < nlev; ++l) {
    const CsrLevel L = desc[l];
    trsv_csr_rows<UPPER>(L, 0, TRSV_SMALL_WG / L.S, threadIdx.x, rows, rhs, lrp, cols, vals, dinv, d, x);
    __syncthreads();
  }
}
// one workgroup per independent diagonal block (subdomain): the whole triangular solve of the block, level after level
template <bool UPPER>
__global__ __launch_bounds__(TRSV_SMALL_WG) void k_trsv_csr_blocks(const int32_t *__restrict__ blk_lev_ptr, const CsrLevel *__restrict__ desc,
                                                                    const int32_t *__restrict__ rows, const int32_t *__restrict__ rhs, const int64_t *__restrict__ lrp,
                                                                    const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                                                    const double *__restrict__ dinv, const double *__restrict__ d, double *x)
{
  const int l1 = blk_lev_ptr[blockIdx.x + 1];
  for (int l = blk_lev_ptr[blockIdx.x]; l < l1; ++l) {
    const CsrLevel L = desc[l];
    trsv_csr_rows<UPPER>(L, 0, TRSV_SMALL_WG / L.S, threadIdx.x, rows, rhs, lrp, cols, vals, dinv, d, x);
    __syncthreads();
  }
}
// one large level over the whole grid
template <bool UPPER>
__global__ __launch_bounds__(WG) void k_trsv_csr_level(CsrLevel L, const int32_t *__restrict__ rows, const int32_t *__restrict__ rhs, const int64_t *__restrict__ lrp,
                                                       const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                                       const double *__restrict__ dinv, const double *__restrict__ d, double *x)
{
  const int gpb = WG / L.S;
  trsv_csr_rows<UPPER>(L, blockIdx.x * gpb, gridDim.x * gpb, threadIdx.x, rows, rhs, lrp, cols, vals, dinv, d, x);
}
// multi-right-hand-side level (row-major n x nrhs blocks): S slices x nrhs columns of threads per row, slice sums meet in LDS
template <bool UPPER>
__global__ __launch_bounds__(WG) void k_trsv_csr_level_multi(CsrLevel L, int S, int nrhs, const int32_t *__restrict__ rows, const int32_t *__restrict__ rhs, const int64_t *__restrict__ lrp,
                                                             const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                                             const double *__restrict__ dinv, const double *__restrict__ d, int64_t ldd, double *x, int64_t ldx)
{
  __shared__ double part[WG];
  const int per_row = S * nrhs, rpb = WG / per_row;
  const int g = threadIdx.x / per_row, u = threadIdx.x - g * per_row;
  const int sl = u / nrhs, j = u - sl * nrhs;
  const int r = blockIdx.x * rpb + g;
  const bool act = g < rpb && r < L.m;
  double s = 0.0;
  if (act) {
    const int64_t k1 = lrp[L.row_off + r + 1];
    for (int64_t k = lrp[L.row_off + r] + sl; k < k1; k += 8 * (int64_t)S) {
      int32_t c[8];
      double v[8], xv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t kk = k + (int64_t)u * S;
        const bool ok = kk < k1;
        c[u] = ok ? cols[kk] : -1;
        v[u] = ok ? vals[kk] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) xv[u] = c[u] >= 0 ? x[(int64_t)c[u] * ldx + j] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u] * xv[u];
    }
  }
  part[threadIdx.x] = s;
  __syncthreads();
  if (act && sl == 0) {
    const int ri = rhs[L.row_off + r];
    double t = ri >= 0 ? (UPPER ? x[(int64_t)ri * ldx + j] : d[(int64_t)ri * ldd + j]) : 0.0;
    for (int q = 0; q < S; ++q) t -= part[g * per_row + q * nrhs + j];
    x[(int64_t)rows[L.row_off + r] * ldx + j] = UPPER ? t * dinv[L.row_off + r] : t;
  }
}

// ---------------------------------------------------------------------------------------------
// Coherent accesses for hand-overs between waves inside one launch (cdna_hip_programming.md Guideline 16):
// sc1 loads bypass the non-coherent L1, sc1 stores are written through.
__device__ __forceinline__ double ld_sc1(const double *p)
{
  return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st_sc1(double *p, double v)
{
  __hip_atomic_store((unsigned long long *)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------
// XCD-local placement shared by the single-launch engines (xcd2 fallback, pipe).  Measured on MI355X
// (tools/xcd_handoff_bench.hip): a hand-off between waves costs 0.9 us when producers and consumers share one XCD
// (plain stores stay in that XCD's L2, consumers read them with sc1 loads that bypass only L1) against 2.0 us across
// XCDs (write-through) and 7-9 us for a kernel boundary or a counter barrier.  Each independent diagonal block
// (= subdomain) is therefore solved by the waves of ONE XCD: every workgroup reads its XCD from HW_REG_XCC_ID and
// draws a ticket on that XCD; after a grid barrier it knows how many workgroups its XCD has and works only on the
// groups owned by its XCD (group % 8 == xcc).  If some XCD that owns a group received no workgroup, all take the
// placement-independent path (write-through stores).  epoch comes from a device word bumped by
// k_trsv_xcd_prologue, so flags never need zeroing.
constexpr int TRSV_X_MAXW = 64;
struct GroupDesc {
  int32_t nlevL, nlevU;
  int64_t lev_off; // first LevelDesc of the group (L levels, then U levels)
};
struct XcdState {
  unsigned tickets[8];
  unsigned global_ticket, arrived, epoch, pad;
};
__global__ void k_trsv_xcd_prologue(XcdState *st)
{
  if (threadIdx.x < 8) st->tickets[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    st->global_ticket = 0;
    st->arrived = 0;
    st->epoch += 1;
  }
}
__device__ __forceinline__ unsigned hw_xcc_id() { return __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u; } // HW_REG_XCC_ID[3:0]

// ---------------------------------------------------------------------------------------------
// Block solve of a plain ILU(0) factor in ONE launch (engine `xcd` of the multi-RHS path; host side: engine_multi_xcd.hpp, plan and
// team arithmetic: trsv_multi_plan.hpp).  The kernel walks the level engine's own arrays (TriSchedule: rows, cols, vals, dinv and
// their float copies) with the strides, widths and padding of k_trsv_level_multi4 / k_trsv_level_multi / k_trsv_level_multi4_f32, and
// sums every row over the same entries in the same order: its results are the bits of the level launches.  Teams of workgroups
// (team_of) take the diagonal blocks in turn; inside a team the (row, column quad) items of a level are dealt as those kernels deal
// them to their grids, and the levels are separated by the all-to-all flag barrier of k_sn_top1 in place of a kernel boundary.
// Visibility: X (f32: the work block xf) is written by one workgroup and read by others inside the launch, so EVERY load of it is
// an sc1 load (also the upper sweep's own row) and every store is written through and drained before the flag; D, the factor
// arrays and the plan are constant during the launch (plain loads); xout is only written (plain stores).
constexpr int MULTI_XCD_TEAMS = 8;
constexpr int MULTI_XCD_FLAG_STRIDE = 16; // unsigned long long words between two flags (128 bytes)
constexpr unsigned MULTI_XCD_SPINS = 1u << 22;
constexpr unsigned MULTI_XCD_ERR_RESIDENCY = 12, MULTI_XCD_ERR_BARRIER = 13, MULTI_XCD_ERR_SLOTS = 14; // codes left in the status word
template <class T>
struct MultiXcdTri { // views of one TriSchedule
  const LevelDesc *desc;
  const int32_t *rows, *cols;
  const T *vals, *dinv;
  const int32_t *blk_off, *blk_nlev;
};
template <class T>
struct MultiXcdArgs {
  int nb, nrhs, force_one, slots; // diagonal blocks; columns; one team forced (tests); flag slots per team (= the grid)
  MultiXcdTri<T> tri[2];          // L, U
  const double *D;
  int64_t ldd;
  T *X;                           // double: the result block; float: the work block xf
  int64_t ldx;
  double *xout;                   // float only: the result block, written in the upper sweep
  int64_t ldo;
  XcdState *st;
  unsigned long long *flags;
  unsigned *err, *report;
};
typedef double mx_d4 __attribute__((ext_vector_type(4)));
typedef double mx_d2 __attribute__((ext_vector_type(2)));
typedef float mx_f4 __attribute__((ext_vector_type(4)));
typedef unsigned mx_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ mx_d4 mx_ld_sc1(const double *p, mx_d4) { return mx_d4{ld_sc1(p), ld_sc1(p + 1), ld_sc1(p + 2), ld_sc1(p + 3)}; }
__device__ __forceinline__ mx_f4 mx_ld_sc1(const float *p, mx_f4)
{
  const unsigned long long a = __hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long b = __hip_atomic_load((const unsigned long long *)(p + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return mx_f4{__uint_as_float((unsigned)a), __uint_as_float((unsigned)(a >> 32)), __uint_as_float((unsigned)b), __uint_as_float((unsigned)(b >> 32))};
}
// 16-byte write-through store (p 16-byte aligned); the two idle cycles keep the data registers untouched while the store reads them
__device__ __forceinline__ void mx_st16_sc1(void *p, mx_u4 v)
{
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void mx_st_sc1(double *p, mx_d4 s)
{
  mx_st16_sc1(p, __builtin_bit_cast(mx_u4, mx_d2{s[0], s[1]}));
  mx_st16_sc1(p + 2, __builtin_bit_cast(mx_u4, mx_d2{s[2], s[3]}));
}
__device__ __forceinline__ void mx_st_sc1(float *p, mx_f4 s) { mx_st16_sc1(p, __builtin_bit_cast(mx_u4, s)); }

// one (row, column quad) item of a level: k_trsv_level_multi4 (T = double) / k_trsv_level_multi4_f32 (T = float) with coherent accesses
template <class T, bool UPPER>
__device__ __forceinline__ void mx_item_quad(int m, int w, int r, int j, const int32_t *__restrict__ rows, const int32_t *__restrict__ cols, const T *__restrict__ vals,
                                             const T *__restrict__ dinv, const double *__restrict__ d, int64_t ldd, T *x, int64_t ldx, double *__restrict__ xout, int64_t ldo)
{
  typedef T V4 __attribute__((ext_vector_type(4)));
  const int64_t row = rows[r], o = row * ldx + j;
  V4 s;
  if (UPPER) s = mx_ld_sc1(x + o, V4{});
  else {
    const mx_d4 dv = *reinterpret_cast<const mx_d4 *>(d + row * ldd + j);
    s = V4{(T)dv[0], (T)dv[1], (T)dv[2], (T)dv[3]};
  }
  for (int k0 = 0; k0 < w; k0 += TRSV_UNROLL) {
    int32_t c[TRSV_UNROLL];
    T v[TRSV_UNROLL];
    V4 xv[TRSV_UNROLL];
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) {
      const bool ok = k0 + u < w;
      c[u] = ok ? cols[(int64_t)(k0 + u) * m + r] : -1;
      v[u] = ok ? vals[(int64_t)(k0 + u) * m + r] : (T)0;
    }
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) { // (k0 + u < w is uniform: a scalar branch around the coherent loads; c[u] >= 0 says the same)
      if (k0 + u < w) xv[u] = mx_ld_sc1(x + (int64_t)c[u] * ldx + j, V4{});
      else xv[u] = V4{(T)0, (T)0, (T)0, (T)0};
    }
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) s -= v[u] * xv[u];
  }
  if (UPPER) {
    s *= dinv[r];
    if (sizeof(T) == 4) *reinterpret_cast<mx_d4 *>(xout + row * ldo + j) = mx_d4{(double)s[0], (double)s[1], (double)s[2], (double)s[3]};
  }
  mx_st_sc1(x + o, s);
}
// one (row, column) item: k_trsv_level_multi over trsv_row_sum_multi
template <bool UPPER>
__device__ __forceinline__ void mx_item_scalar(int m, int w, int r, int j, const int32_t *__restrict__ rows, const int32_t *__restrict__ cols, const double *__restrict__ vals,
                                               const double *__restrict__ dinv, const double *__restrict__ d, int64_t ldd, double *x, int64_t ldx)
{
  const int64_t o = (int64_t)rows[r] * ldx + j;
  double s = UPPER ? ld_sc1(x + o) : d[(int64_t)rows[r] * ldd + j];
  for (int k0 = 0; k0 < w; k0 += TRSV_UNROLL) {
    int32_t c[TRSV_UNROLL];
    double v[TRSV_UNROLL], xv[TRSV_UNROLL];
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) {
      const bool ok = k0 + u < w;
      c[u] = ok ? cols[(int64_t)(k0 + u) * m + r] : -1;
      v[u] = ok ? vals[(int64_t)(k0 + u) * m + r] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) xv[u] = k0 + u < w ? ld_sc1(x + (int64_t)c[u] * ldx + j) : 0.0;
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) s -= v[u] * xv[u];
  }
  st_sc1(x + o, UPPER ? s * dinv[r] : s);
}

template <class T, bool QUAD>
__global__ __launch_bounds__(WG) void k_trsv_multi_xcd(MultiXcdArgs<T> A)
{
  static_assert(QUAD || sizeof(T) == 8, "the single-precision sweeps exist in the quad form only");
  __shared__ unsigned sh_xcc, sh_xt, sh_gt, sh_fail;
  const int tid = threadIdx.x, lane = tid & 63;
  XcdState *st = A.st;
  // ---- placement: ticket on the own XCD, then a bounded grid barrier (k_sn_top1) ----
  if (tid == 0) {
    const unsigned xcc = hw_xcc_id();
    sh_xcc = xcc;
    sh_xt = __hip_atomic_fetch_add(&st->tickets[xcc], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh_gt = __hip_atomic_fetch_add(&st->global_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&st->arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned fail_ = 0;
    for (unsigned spins = 0; __hip_atomic_load(&st->arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x; ++spins) {
      if (spins > MULTI_XCD_SPINS) { // the workgroups are not co-resident (another process on the GPU?)
        __hip_atomic_store(A.err, MULTI_XCD_ERR_RESIDENCY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        fail_ = 1;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    sh_fail = fail_;
  }
  __syncthreads();
  if (sh_fail) return;
  const unsigned epoch = __hip_atomic_load(&st->epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned tks[8];
#pragma unroll
  for (int x = 0; x < 8; ++x) tks[x] = __hip_atomic_load(&st->tickets[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const multi_xcd::Team tm = multi_xcd::team_of(tks, A.nb, A.force_one, sh_xcc, sh_xt, sh_gt, gridDim.x);
  if (sh_gt == 0 && tid == 0) { // the report of ddm_ilu0_multi_info
#pragma unroll
    for (int x = 0; x < 8; ++x) __hip_atomic_store(A.report + x, tks[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(A.report + 8, (unsigned)tm.nteams, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(A.report + 9, (unsigned)tm.one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (tm.size > A.slots || tm.rank >= tm.size) { // (cannot happen with slots = the grid; the same verdict in every workgroup of a team)
    if (tid == 0) __hip_atomic_store(A.err, MULTI_XCD_ERR_SLOTS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  unsigned long long *gflags = A.flags + (size_t)tm.team * (size_t)A.slots * MULTI_XCD_FLAG_STRIDE;
  const unsigned W = (unsigned)tm.size;
  unsigned count = 0;
  bool failed = false;
  // all-to-all flag barrier among the W workgroups of the team: every storing wave drains, one lane publishes, wave 0 polls all flags
  auto team_barrier = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    ++count;
    if (tid == 0) __hip_atomic_store(gflags + (size_t)tm.rank * MULTI_XCD_FLAG_STRIDE, ((unsigned long long)epoch << 32) | count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < 64) {
      for (unsigned spins = 0;; ++spins) {
        bool ok = true;
        for (unsigned j = (unsigned)lane; j < W; j += 64u) {
          const unsigned long long v = __hip_atomic_load(gflags + (size_t)j * MULTI_XCD_FLAG_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ok = ok && (unsigned)(v >> 32) == epoch && (unsigned)v >= count;
        }
        if (__all(ok)) break;
        if (spins > MULTI_XCD_SPINS) {
          if (lane == 0) {
            __hip_atomic_store(A.err, MULTI_XCD_ERR_BARRIER, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            sh_fail = 1;
          }
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    __syncthreads();
    if (sh_fail) failed = true;
  };
  // (Measured and not kept, tools/multi_trsv_bench.py, DESIGN.md section 9: plain stores and a plain flag where a team is one XCD,
  //  together with the barrier split into arrive / wait and the next level's plan loaded and its first factor entries touched in
  //  between -- 38.8 against 29.6 ms at 216^3, m = 8.)
  const int nq = QUAD ? A.nrhs / 4 : A.nrhs;
  for (int b = tm.team; b < A.nb && !failed; b += tm.nteams)
    for (int pass = 0; pass < 2 && !failed; ++pass) {
      const MultiXcdTri<T> &S = A.tri[pass];
      const int nl = S.blk_nlev[b];
      for (int l = 0; l < nl && !failed; ++l) {
        const LevelDesc Ld = S.desc[l];
        const int p0 = S.blk_off[(int64_t)l * (A.nb + 1) + b], p1 = S.blk_off[(int64_t)l * (A.nb + 1) + b + 1];
        const int64_t nitem = (int64_t)(p1 - p0) * nq;
        const int32_t *rows = S.rows + Ld.row_off, *cols = S.cols + Ld.ent_off;
        const T *vals = S.vals + Ld.ent_off, *dinv = pass ? S.dinv + Ld.row_off : nullptr;
        for (int64_t it = (int64_t)tm.rank * WG + tid; it < nitem; it += (int64_t)W * WG) {
          const int r = p0 + (int)(it / nq);
          const int jq = (int)(it - (int64_t)(r - p0) * nq);
          if constexpr (QUAD) {
            if (pass) mx_item_quad<T, true>(Ld.m, Ld.w, r, 4 * jq, rows, cols, vals, dinv, A.D, A.ldd, A.X, A.ldx, A.xout, A.ldo);
            else mx_item_quad<T, false>(Ld.m, Ld.w, r, 4 * jq, rows, cols, vals, dinv, A.D, A.ldd, A.X, A.ldx, A.xout, A.ldo);
          } else {
            if (pass) mx_item_scalar<true>(Ld.m, Ld.w, r, jq, rows, cols, vals, dinv, A.D, A.ldd, A.X, A.ldx);
            else mx_item_scalar<false>(Ld.m, Ld.w, r, jq, rows, cols, vals, dinv, A.D, A.ldd, A.X, A.ldx);
          }
        }
        team_barrier();
      }
    }
}

// ---------------------------------------------------------------------------------------------
// XCD-local solve with a dedicated LOADER wave per workgroup ("xcd2" engine).
// vmcnt retires in order, so a wave that both streams factor entries from HBM and polls flags pays
// the HBM latency on every level.  Here each workgroup has two waves: wave 1 streams the tiles of
// the workgroup's chunks (row ids, permuted right-hand side / inverse pivots, 16 entries per row)
// from HBM into an LDS ring several levels ahead; wave 0 takes a tile from LDS (lgkmcnt), polls the
// previous level's flags, gathers x from L2, stores, drains only its own store and sets its flag.
// The two waves synchronise through two LDS words per ring (produced / consumed counts); they never
// meet at a barrier.  Cross-workgroup protocol and XCD grouping are those of k_trsv_xcd.
constexpr int TRSV_L_SLOTS = 8;
struct TrsvTileHdr { // everything the compute wave needs to know about a work item: no descriptor loads on its path
  int32_t valid, grp, lev, c, m, w, upper, nact_prev, level_done, pad;
  int64_t flag_base, ent_off;
};
struct TrsvLdsTile {
  int32_t row[64];
  double s0[64];  // L: right-hand side d[row];  U: inverse pivot
  int32_t cc[TRSV_UNROLL][64];
  double vv[TRSV_UNROLL][64];
  TrsvTileHdr hdr;
};
constexpr int TRSV_L_LOADERS = 2;
struct TrsvLds {
  TrsvLdsTile tile[TRSV_L_SLOTS];
  unsigned ready[TRSV_L_SLOTS]; // ready[slot] = seq + 1 once work item seq is in the slot (several loader waves)
  unsigned produced, consumed;  // work items written by the (single) loader / released by the compute wave
};
__global__ void k_permute_rhs(int64_t n, const int32_t *__restrict__ rows, const double *__restrict__ d, double *__restrict__ dperm)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) dperm[i] = d[rows[i]];
}

// enumerates the work items (level, chunk) of one wave in processing order
struct TrsvWork {
  const GroupDesc *groups;
  const LevelDesc *desc;
  int ngroups, gstep, grp, lev, c, rank, W;
  __device__ bool valid() const { return grp < ngroups; }
  __device__ void init(const GroupDesc *g, const LevelDesc *d_, int ng, int first, int step, int rank_, int W_)
  {
    groups = g; desc = d_; ngroups = ng; gstep = step; grp = first; lev = 0; c = rank_; rank = rank_; W = W_;
    settle();
  }
  __device__ void settle()
  { // move to the next existing (level, chunk)
    while (grp < ngroups) {
      const GroupDesc G = groups[grp];
      const int nlev = G.nlevL + G.nlevU;
      while (lev < nlev) {
        const int nchunk = (desc[G.lev_off + lev].m + 63) >> 6;
        if (c < nchunk) return;
        ++lev;
        c = rank;
      }
      grp += gstep;
      lev = 0;
      c = rank;
    }
  }
  __device__ void advance()
  {
    c += W;
    settle();
  }
};

__global__ __launch_bounds__(64 * (1 + TRSV_L_LOADERS)) void k_trsv_xcd2(int ngroups, const GroupDesc *__restrict__ groups, const LevelDesc *__restrict__ desc,
                                                    const int64_t *__restrict__ flag_off, const int32_t *__restrict__ rowsA,
                                                    const int32_t *__restrict__ colsA, const double *__restrict__ valsA,
                                                    const double *__restrict__ dinvA, const double *__restrict__ dperm, double *x,
                                                    unsigned *flags, XcdState *st, unsigned *err, unsigned long long *stamps)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  TrsvLds &S = *reinterpret_cast<TrsvLds *>(smem_raw);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (threadIdx.x < TRSV_L_SLOTS) S.ready[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    S.produced = 0;
    S.consumed = 0;
  }
  // ---- placement: ticket on the own XCD, then a grid barrier (wave 0 lane 0 acts for the workgroup)
  __shared__ unsigned sh_xcc, sh_t, sh_gt, sh_fail;
  if (threadIdx.x == 0) {
    const unsigned xcc = hw_xcc_id();
    sh_xcc = xcc;
    sh_t = __hip_atomic_fetch_add(&st->tickets[xcc], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh_gt = __hip_atomic_fetch_add(&st->global_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&st->arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned fail_ = 0;
    for (unsigned spins = 0; __hip_atomic_load(&st->arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x; ++spins) {
      if (spins > (1u << 22)) {
        __hip_atomic_store(err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        fail_ = 1;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    sh_fail = fail_;
  }
  __syncthreads(); // the only workgroup barrier: publishes the placement to both waves
  if (sh_fail) return;
  const unsigned xcc = sh_xcc, t = sh_t, gt = sh_gt;
  const unsigned epoch = __hip_atomic_load(&st->epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned tk = lane < 8 ? __hip_atomic_load(&st->tickets[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 1u;
  const int owners = ngroups < 8 ? ngroups : 8;
  const bool local_ok = __all(lane >= owners || tk > 0u);
  int W, rank, first, step;
  bool wt;
  if (local_ok) {
    W = (int)__shfl((int)tk, (int)xcc, 64);
    if (W > TRSV_X_MAXW) W = TRSV_X_MAXW;
    rank = (int)t; first = (int)xcc; step = 8; wt = false;
  } else {
    W = (int)gridDim.x < TRSV_X_MAXW ? (int)gridDim.x : TRSV_X_MAXW;
    rank = (int)gt; first = 0; step = 1; wt = true;
  }
  if (rank >= W) return;
  TrsvWork wk;
  wk.init(groups, desc, ngroups, first, step, rank, W);
  volatile unsigned *ready = S.ready;
  volatile unsigned *consumed = &S.consumed;

  if (wave >= 1) {
    // =========================== loaders: HBM -> LDS ring ===========================
    // TRSV_L_LOADERS loader waves; loader j handles the work items seq = j, j + L, j + 2L, ... and announces each
    // slot separately (ready[slot] = seq + 1), so tiles of different loaders may land out of order.
    const int lj = wave - 1;
    // two tiles in flight: the loads of item seq+1 are issued before item seq is written to LDS.  The loader also
    // resolves all schedule descriptors and hands them over in the tile header.
    struct Regs {
      int32_t rowm;
      double s0;
      int32_t cc[TRSV_UNROLL];
      double vv[TRSV_UNROLL];
      TrsvTileHdr h;
    };
    auto issue = [&](Regs &R, const TrsvWork &k) {
      const GroupDesc G = groups[k.grp];
      const LevelDesc D = desc[G.lev_off + k.lev];
      const bool upper = k.lev >= G.nlevL;
      const int r = (k.c << 6) + lane;
      const int rr = r < D.m ? r : D.m - 1;
      const int32_t row = rowsA[D.row_off + rr];
      R.rowm = r < D.m ? row : -1 - row; // negative = shadow lane (no store)
      R.s0 = upper ? dinvA[D.row_off + rr] : dperm[D.row_off + rr];
      (void)*(volatile const unsigned long long *)(x + row); // warm this XCD's L2 with the line of x[row]
      const int32_t *cols = colsA + D.ent_off;
      const double *vals = valsA + D.ent_off;
#pragma unroll
      for (int u = 0; u < TRSV_UNROLL; ++u) {
        R.cc[u] = 0;
        R.vv[u] = 0.0;
        if (u < D.w) {
          R.cc[u] = cols[(int64_t)u * D.m + rr];
          R.vv[u] = vals[(int64_t)u * D.m + rr];
        }
      }
      const int nchunk = (D.m + 63) >> 6;
      int ncp = 0;
      if (k.lev > 0) ncp = (desc[G.lev_off + k.lev - 1].m + 63) >> 6;
      R.h.valid = 1;
      R.h.grp = k.grp;
      R.h.lev = k.lev;
      R.h.c = k.c;
      R.h.m = D.m;
      R.h.w = D.w;
      R.h.upper = upper ? 1 : 0;
      R.h.nact_prev = (k.lev > 0 && k.c == k.rank) ? (ncp < k.W ? ncp : k.W) : 0; // > 0: poll the previous level's flags first
      R.h.level_done = (k.c + k.W >= nchunk) ? 1 : 0;                               // last chunk of this wave in this level
      R.h.pad = 0;
      R.h.flag_base = flag_off[k.grp] + (int64_t)k.lev * TRSV_X_MAXW;
      R.h.ent_off = D.ent_off;
    };
    Regs A, B;
    for (int q = 0; q < lj && wk.valid(); ++q) wk.advance(); // first item of this loader
    unsigned seq = (unsigned)lj;
    auto end_marker = [&](unsigned sq) { // the first loader that runs out of items writes the end marker at its next sequence number
      for (unsigned spins = 0; sq >= *consumed + TRSV_L_SLOTS; ++spins) {
        if (spins > (1u << 24)) return;
        __builtin_amdgcn_s_sleep(1);
      }
      if (lane == 0) {
        S.tile[sq % TRSV_L_SLOTS].hdr.valid = 0;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        ready[sq % TRSV_L_SLOTS] = sq + 1;
      }
    };
    if (!wk.valid()) {
      end_marker(seq);
      return;
    }
    issue(A, wk);
    for (;; seq += TRSV_L_LOADERS) {
      for (int q = 0; q < TRSV_L_LOADERS && wk.valid(); ++q) wk.advance();
      const bool more = wk.valid();
      if (more) issue(B, wk);
      for (unsigned spins = 0; seq >= *consumed + TRSV_L_SLOTS; ++spins) { // free ring slot?
        if (spins > (1u << 24)) {
          if (lane == 0) __hip_atomic_store(err, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          return;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      TrsvLdsTile &T = S.tile[seq % TRSV_L_SLOTS];
      T.row[lane] = A.rowm;
      T.s0[lane] = A.s0;
#pragma unroll
      for (int u = 0; u < TRSV_UNROLL; ++u)
        if (u < A.h.w) {
          T.cc[u][lane] = A.cc[u];
          T.vv[u][lane] = A.vv[u];
        }
      if (lane == 0) T.hdr = A.h;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // tile is in LDS before it is announced
      if (lane == 0) ready[seq % TRSV_L_SLOTS] = seq + 1;
      if (!more) {
        end_marker(seq + TRSV_L_LOADERS);
        return;
      }
      A = B;
    }
  }

  // =========================== compute wave ===========================
  // diagnostic stamps (only when a buffer is passed; production launches pass nullptr)
  const bool stamp = stamps != nullptr && rank == 0 && (local_ok ? xcc == 0 : true);
  unsigned long long t_tile = 0, t_poll = 0, t_gather = 0, t_drain = 0, n_items = 0, t_begin = 0, tq = 0;
#define DDM_STAMP(acc)                                                 \
  if (stamp) {                                                         \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();      \
    acc += now_ - tq;                                                  \
    tq = now_;                                                         \
  }
  if (stamp) t_begin = tq = __builtin_amdgcn_s_memtime();
  for (unsigned seq = 0;; ++seq) {
    for (unsigned spins = 0; ready[seq % TRSV_L_SLOTS] != seq + 1; ++spins) {
      if (spins > (1u << 24)) {
        if (lane == 0) __hip_atomic_store(err, 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    const TrsvLdsTile &T = S.tile[seq % TRSV_L_SLOTS];
    const TrsvTileHdr H = T.hdr;
    if (!H.valid) break;
    const bool upper = H.upper != 0;
    const int32_t rowm = T.row[lane];
    const bool act = rowm >= 0;
    const int32_t row = act ? rowm : -1 - rowm;
    const double s0 = T.s0[lane];
    int32_t cc[TRSV_UNROLL];
    double vv[TRSV_UNROLL], xv[TRSV_UNROLL];
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) {
      cc[u] = 0;
      vv[u] = 0.0;
      if (u < H.w) {
        cc[u] = T.cc[u][lane];
        vv[u] = T.vv[u][lane];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) *consumed = seq + 1; // slot may be refilled
    DDM_STAMP(t_tile)
    // previous level of this group complete?
    if (H.nact_prev > 0) {
      const unsigned *fp = flags + H.flag_base - TRSV_X_MAXW;
      for (unsigned spins = 0;; ++spins) {
        const unsigned v = lane < H.nact_prev ? __hip_atomic_load(fp + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : epoch;
        if (__all(v == epoch)) break;
        if (spins > (1u << 22)) {
          if (lane == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          break;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    DDM_STAMP(t_poll)
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) {
      xv[u] = 0.0;
      if (u < H.w) xv[u] = ld_sc1(x + cc[u]);
    }
    double s = upper ? ld_sc1(x + row) : s0;
#pragma unroll
    for (int u = 0; u < TRSV_UNROLL; ++u) s -= vv[u] * xv[u];
    if (H.w > TRSV_UNROLL) { // rows wider than a tile: the rest straight from global memory (rare)
      const int r = (H.c << 6) + lane;
      const int rr = r < H.m ? r : H.m - 1;
      for (int k = TRSV_UNROLL; k < H.w; ++k)
        s -= valsA[H.ent_off + (int64_t)k * H.m + rr] * ld_sc1(x + colsA[H.ent_off + (int64_t)k * H.m + rr]);
    }
    if (stamp) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      DDM_STAMP(t_gather)
    }
    const double out = upper ? s * s0 : s;
    if (act) {
      if (wt) st_sc1(x + row, out);
      else x[row] = out;
    }
    if (H.level_done) { // last chunk of this wave in this level -> drain and raise the flag
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) {
        unsigned *f = flags + H.flag_base + rank;
        if (wt) __hip_atomic_store(f, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *(volatile unsigned *)f = epoch;
      }
    }
    DDM_STAMP(t_drain)
    n_items += 1;
  }
  if (stamp && lane == 0) {
    stamps[0] = t_tile;
    stamps[1] = t_poll;
    stamps[2] = t_gather;
    stamps[3] = t_drain;
    stamps[4] = n_items;
    stamps[5] = __builtin_amdgcn_s_memtime() - t_begin;
  }
#undef DDM_STAMP
}

// ---------------------------------------------------------------------------------------------
// xp[pos] <- d[row(pos)] for the L positions of every group; x[row(pos)] <- xp[pos] for the U positions
__global__ void k_w_permute_in(int64_t n, const int64_t *__restrict__ lpos, const int32_t *__restrict__ rows, const double *__restrict__ d,
                               double *__restrict__ dperm)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) dperm[lpos[i]] = d[rows[lpos[i]]];
}
__global__ void k_w_permute_out(int64_t n, const int64_t *__restrict__ upos, const int32_t *__restrict__ rows, const double *__restrict__ xp,
                                double *__restrict__ x)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) x[rows[upos[i]]] = xp[upos[i]];
}

// ---------------------------------------------------------------------------------------------
// K2 extend (schwarz.hh:121-122), K5 restrict (schwarz.hh:146), K4 POU scaling (schwarz.hh:141)
// dst[i,:] = src[perm[i],:] / dst[perm[i],:] = src[i,:] for row-major n x nrhs blocks (fill-reducing order of the direct solver)
// (src / dst of the un-permuted side have leading dimension ld; the permuted side is packed, ld = nrhs)
__global__ void k_perm_gather(int64_t n, int nrhs, const int32_t *__restrict__ perm, const double *__restrict__ src, int64_t ld, double *__restrict__ dst)
{
  const int64_t tot = n * nrhs;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < tot; t += (int64_t)gridDim.x * WG) {
    const int64_t i = t / nrhs;
    dst[t] = src[(int64_t)perm[i] * ld + (t - i * nrhs)];
  }
}
__global__ void k_perm_scatter(int64_t n, int nrhs, const int32_t *__restrict__ perm, const double *__restrict__ src, double *__restrict__ dst, int64_t ld)
{
  const int64_t tot = n * nrhs;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < tot; t += (int64_t)gridDim.x * WG) {
    const int64_t i = t / nrhs;
    dst[(int64_t)perm[i] * ld + (t - i * nrhs)] = src[t];
  }
}
// dst[perm[i]] += src[i] (the correction of an iterative-refinement step, scattered back into the solution)
__global__ void k_perm_scatter_add(int64_t n, int nrhs, const int32_t *__restrict__ perm, const double *__restrict__ src, double *__restrict__ dst, int64_t ld)
{
  const int64_t tot = n * nrhs;
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < tot; t += (int64_t)gridDim.x * WG) {
    const int64_t i = t / nrhs;
    dst[(int64_t)perm[i] * ld + (t - i * nrhs)] += src[t];
  }
}
// R = D - A X for row-major blocks (n x nrhs): the residual of an iterative-refinement step (dune/ddm/eigensolvers/umfpack.hh:55-60);
// one thread per (row, rhs), row sums in column order
__global__ __launch_bounds__(WG) void k_residual_rowmajor(int64_t n, int nrhs, const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const double *__restrict__ va,
                                                          const double *__restrict__ x, int64_t ldx, const double *__restrict__ d, int64_t ldd, double *__restrict__ r, int64_t ldr)
{
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  const int64_t row = t / nrhs;
  if (row >= n) return;
  const int j = (int)(t - row * nrhs);
  double s = d[row * ldd + j];
  for (int64_t k = rp[row]; k < rp[row + 1]; ++k) s -= va[k] * x[(int64_t)ci[k] * ldx + j];
  r[row * ldr + j] = s;
}
__global__ void k_extend(int64_t n, const int32_t *__restrict__ ext_map, const double *__restrict__ d, double *__restrict__ dov)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) {
    const int32_t m = ext_map[i];
    dov[i] = m >= 0 ? d[m] : 0.0;
  }
}
// x[m] = (ACC ? x[m] : 0) + w[i]*xov[i] for the rows that have a non-overlapping image
template <bool ACC, bool SCALE>
__global__ void k_restrict(int64_t n, const int32_t *__restrict__ ext_map, const double *__restrict__ xov,
                           const double *__restrict__ w, double *__restrict__ x)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) {
    const int32_t m = ext_map[i];
    if (m >= 0) {
      const double v = SCALE ? xov[i] * w[i] : xov[i];
      x[m] = ACC ? x[m] + v : v;
    }
  }
}
__global__ void k_scale(int64_t n, const double *__restrict__ w, double *__restrict__ x)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) x[i] *= w[i];
}
__global__ void k_fill(int64_t n, double v, double *__restrict__ x)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) x[i] = v;
}
// y = a*x + y  (a from host) ; z = x + y
__global__ void k_axpy(int64_t n, double a, const double *__restrict__ x, double *__restrict__ y)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) y[i] += a * x[i];
}

// y -= (*h) x with the coefficient in device memory (modified Gram-Schmidt of restarted GMRES), x *= a
__global__ void k_axpy_negdev(int64_t n, const double *__restrict__ h, const double *__restrict__ x, double *__restrict__ y)
{
  const double a = h[0];
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) y[i] -= a * x[i];
}
__global__ void k_scal(int64_t n, double a, double *__restrict__ x)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) x[i] *= a;
}

// ---------------------------------------------------------------------------------------------
// halo exchange: pack (gather) and deterministic unpack (copy / add), SURVEY.md 2.3 C1-C4
__global__ void k_pack(int64_t n, const int64_t *__restrict__ idx, const double *__restrict__ v, double *__restrict__ buf)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) buf[i] = v[idx[i]];
}
template <bool ADD>
__global__ void k_unpack(int64_t ndst, const int64_t *__restrict__ dst_idx, const int64_t *__restrict__ dst_ptr,
                         const int64_t *__restrict__ src_pos, const double *__restrict__ buf, double *__restrict__ v)
{
  for (int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x; t < ndst; t += (int64_t)gridDim.x * WG) {
    const int64_t i = dst_idx[t];
    double s = ADD ? v[i] : 0.0;
    for (int64_t k = dst_ptr[t]; k < dst_ptr[t + 1]; ++k) s = ADD ? s + buf[src_pos[k]] : buf[src_pos[k]];
    v[i] = s;
  }
}

// ---------------------------------------------------------------------------------------------
// K20 / a3: owner-masked dot products (nonoverlapping_operator.hh:76-83), two-stage and
// deterministic: partial[b] per workgroup, then one workgroup sums the partials in index order.
// a thread's share of sum_i [mask_i] x_i y_i: rows blockIdx.x * WG + threadIdx.x + t * gridDim.x * WG for ascending t
template <bool MASKED>
__device__ __forceinline__ double dot_thread_sum(int64_t n, const uint8_t *__restrict__ mask, const double *__restrict__ x, const double *__restrict__ y)
{
  double s = 0.0;
  const int64_t step = (int64_t)gridDim.x * WG;
  int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x;
  for (; i + (RED_TRIPS - 1) * step < n; i += RED_TRIPS * step) { // the loads of RED_TRIPS trips in flight, added in trip order
    double a[RED_TRIPS], b[RED_TRIPS];
    bool own[RED_TRIPS];
#pragma unroll
    for (int u = 0; u < RED_TRIPS; ++u) a[u] = x[i + u * step], b[u] = y[i + u * step], own[u] = !MASKED || mask[i + u * step];
#pragma unroll
    for (int u = 0; u < RED_TRIPS; ++u)
      if (own[u]) s += a[u] * b[u];
  }
  for (; i < n; i += step)
    if (!MASKED || mask[i]) s += x[i] * y[i];
  return s;
}
template <bool MASKED>
__global__ __launch_bounds__(WG) void k_dot_partial(int64_t n, const uint8_t *__restrict__ mask, const double *__restrict__ x,
                                                     const double *__restrict__ y, double *__restrict__ partial)
{
  __shared__ double red[4];
  const double s = block_sum(dot_thread_sum<MASKED>(n, mask, x, y), red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(WG) void k_reduce_final(int nb, const double *__restrict__ partial, double *__restrict__ out)
{
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += WG) s += partial[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}
// A reduction that finishes itself (the *_fin kernels): the workgroup's sum s (valid in thread 0) goes to partial[blockIdx.x], and
// the workgroup that arrives last -- told by the value its add to *ticket returned -- sums the gridDim.x partials as k_reduce_final
// does (same strides, same block_sum: the same bits), writes out[0] and puts the ticket back to 0 for the next launch on the stream.
// Nobody waits.  The hand-off (MI355X: the L2s of the XCDs are not coherent with each other, a CU's L1 with nobody): thread 0 stores
// its partial write-through and drains the store before its agent-scope add; the last arriver's thread 0 invalidates its CU's L1
// after the add has returned, the other waves load behind the barrier it then joins; the partials are read past L1.
__device__ __forceinline__ void reduce_finish(double s, double *partial, unsigned *ticket, double *out, double *red)
{
  __shared__ unsigned last;
  if (threadIdx.x == 0) {
    st_sc1(partial + blockIdx.x, s);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == gridDim.x - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    last = t == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  double v = 0.0;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += WG) v += ld_sc1(partial + i);
  v = block_sum(v, red);
  if (threadIdx.x == 0) {
    out[0] = v;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// k_dot_partial + k_reduce_final in one launch: out[0] = sum_i [mask_i] x_i y_i
template <bool MASKED>
__global__ __launch_bounds__(WG) void k_dot_fin(int64_t n, const uint8_t *__restrict__ mask, const double *__restrict__ x, const double *__restrict__ y,
                                                 double *partial, unsigned *ticket, double *out)
{
  __shared__ double red[4];
  const double s = block_sum(dot_thread_sum<MASKED>(n, mask, x, y), red);
  reduce_finish(s, partial, ticket, out, red);
}

// ---------------------------------------------------------------------------------------------
// Rank-local forms of the two halo passes of a Schwarz apply, for a plan whose copies all live on this rank (LocalMaps, halo.hpp).
// Defect: every row of the overlapping defect is a copy of one entry of the non-overlapping one (k_extend, then owner copied to all).
__global__ void k_defect_gather(int64_t n, const int32_t *__restrict__ src_of, const double *__restrict__ d, double *__restrict__ dov)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) {
    const int32_t m = src_of[i];
    dov[i] = m >= 0 ? d[m] : 0.0;
  }
}
// Solution: z[m] = xov[own_of[m]] + the other copies of that row in the order k_unpack<true> adds them (cp_idx[cp_ptr[m] ..
// cp_ptr[m + 1])), which is what k_pack + k_unpack<true> + k_restrict<false, false> leave in z; the non-owner rows of xov are not
// updated.  DOT: also out[0] = sum_m [mask_m] z_m r_m on the grid and with the rows per thread of k_dot_partial, a thread's products
// added in ascending trip order as there, finished by reduce_finish: the bits of dot_device(z, r).
// A thread takes HALO_TRIPS of its rows at a time: their table entries, then their owner values, then copy j of every row that has
// one for ascending j (most rows have none, rows on a face one, on a corner seven) -- four dependent round trips per group where a
// row-by-row loop makes as many per row with copies.  Rows past the end are clamped to the group's first row, loaded and dropped.
constexpr int HALO_TRIPS = 8;
template <bool MASKED, bool DOT>
__global__ __launch_bounds__(WG) void k_halo_sum_restrict(int64_t n, const int32_t *__restrict__ own_of, const int32_t *__restrict__ cp_ptr,
                                                           const int32_t *__restrict__ cp_idx, const double *__restrict__ xov, double *__restrict__ z,
                                                           const uint8_t *__restrict__ mask, const double *__restrict__ r, double *partial, unsigned *ticket,
                                                           double *out)
{
  __shared__ double red[4];
  double s = 0.0;
  const int64_t step = (int64_t)gridDim.x * WG;
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += HALO_TRIPS * step) {
    int64_t row[HALO_TRIPS];
    int32_t o[HALO_TRIPS], k0[HALO_TRIPS], k1[HALO_TRIPS];
    double v[HALO_TRIPS], b[HALO_TRIPS];
    bool ok[HALO_TRIPS], own[HALO_TRIPS];
#pragma unroll
    for (int u = 0; u < HALO_TRIPS; ++u) ok[u] = i + u * step < n, row[u] = ok[u] ? i + u * step : i;
#pragma unroll
    for (int u = 0; u < HALO_TRIPS; ++u) o[u] = own_of[row[u]], k0[u] = cp_ptr[row[u]], k1[u] = cp_ptr[row[u] + 1];
#pragma unroll
    for (int u = 0; u < HALO_TRIPS; ++u) {
      v[u] = xov[o[u]];
      if (DOT) b[u] = r[row[u]], own[u] = ok[u] && (!MASKED || mask[row[u]]);
    }
    int cmax = 0;
#pragma unroll
    for (int u = 0; u < HALO_TRIPS; ++u) {
      if (!ok[u]) k1[u] = k0[u];
      cmax = max(cmax, k1[u] - k0[u]);
    }
    for (int j = 0; j < cmax; ++j) {
      int32_t c[HALO_TRIPS];
      double w[HALO_TRIPS];
#pragma unroll
      for (int u = 0; u < HALO_TRIPS; ++u) c[u] = k0[u] + j < k1[u] ? cp_idx[k0[u] + j] : -1;
#pragma unroll
      for (int u = 0; u < HALO_TRIPS; ++u) w[u] = c[u] >= 0 ? xov[c[u]] : 0.0;
#pragma unroll
      for (int u = 0; u < HALO_TRIPS; ++u)
        if (c[u] >= 0) v[u] = v[u] + w[u];
    }
#pragma unroll
    for (int u = 0; u < HALO_TRIPS; ++u)
      if (ok[u]) {
        z[row[u]] = v[u];
        if (DOT && own[u]) s += v[u] * b[u];
      }
  }
  if (!DOT) return;
  s = block_sum(s, red);
  reduce_finish(s, partial, ticket, out, red);
}

// The device scalars of the Krylov drivers, one numbering for slot s of ctx->scal (SCAL_SLOTS doubles) and row s of ctx->mscal (SCAL_ROWS
// rows of MULTI_MAX doubles): rho of the last iteration, <p, q>, the step length (CG's lambda, flexible CG's alpha), rho, beta, <b, b>;
// then the output row of ddm_dot_multi and ddm_fgmres_defect_multi and the output slot of ddm_dot.
constexpr int SCAL_RHOLAST = 0, SCAL_PQ = 1, SCAL_STEP = 2, SCAL_RHO = 3, SCAL_BETA = 4, SCAL_DEF2 = 5, SCAL_DOT_MULTI = 6, SCAL_DOT = 8;
constexpr int SCAL_SLOTS = 16, SCAL_ROWS = 13; // what ddm_ctx_create and ctx_multi_scratch allocate
// CG, queued CG, flexible CG and ddm_fgmres_defect_multi use 0 .. SCAL_DOT_MULTI; queued BiCGSTAB names its own rows 0 .. BICG_SCALARS - 1
// (multi_kernels.hpp) ON TOP of them: its rows 4 .. 12 cover SCAL_BETA .. SCAL_DOT_MULTI.  The overlap is meant: one driver runs at a
// time on a context, and each writes a scalar before it reads it (a fresh CG slot's SCAL_RHOLAST = 1: k_column_load_multi).
static_assert(SCAL_DEF2 < SCAL_DOT_MULTI && SCAL_DOT_MULTI < SCAL_ROWS && SCAL_DOT < SCAL_SLOTS, "CG family: rows 0 .. 6 of ctx->mscal, slots 0 .. 5 and 8 of ctx->scal");

// CG scalar recurrences on the device (dune-istl CGSolver), one thread.
__global__ void k_cg_lambda(double *scal) { scal[SCAL_STEP] = scal[SCAL_RHOLAST] / scal[SCAL_PQ]; }
__global__ void k_cg_beta(double *scal)
{
  scal[SCAL_BETA] = scal[SCAL_RHO] / scal[SCAL_RHOLAST];
  scal[SCAL_RHOLAST] = scal[SCAL_RHO];
}
// x += lambda p ; b -= lambda q
__global__ void k_cg_update(int64_t n, const double *__restrict__ scal, const double *__restrict__ p,
                            const double *__restrict__ q, double *__restrict__ x, double *__restrict__ b)
{
  const double lam = scal[SCAL_STEP];
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) {
    x[i] += lam * p[i];
    b[i] -= lam * q[i];
  }
}
// the same update followed by the owner-masked partial sums of <b, b> (same grid and summation order as k_dot_partial,
// so the norm is bit-identical to the separate dot product; saves its pass over b)
template <bool MASKED>
__global__ __launch_bounds__(WG) void k_cg_update_norm(int64_t n, const double *__restrict__ scal, const uint8_t *__restrict__ mask,
                                                        const double *__restrict__ p, const double *__restrict__ q, double *__restrict__ x,
                                                        double *__restrict__ b, double *__restrict__ partial)
{
  __shared__ double red[4];
  const double lam = scal[SCAL_STEP];
  double s = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) {
    x[i] += lam * p[i];
    const double bi = b[i] - lam * q[i];
    b[i] = bi;
    if (!MASKED || mask[i]) s += bi * bi;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// p = beta p + q
__global__ void k_cg_direction(int64_t n, const double *__restrict__ scal, const double *__restrict__ q, double *__restrict__ p)
{
  const double beta = scal[SCAL_BETA];
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) p[i] = beta * p[i] + q[i];
}
// The loop of ddm_cg_steps without k_cg_beta, k_cg_lambda and k_reduce_final: the consumer of a quotient forms it itself, every
// thread by the division k_cg_beta / k_cg_lambda make on the same two operands, and one thread stores it for later readers.
// k_cg_beta's second statement, rholast = rho, moves to the update kernel: no thread of THAT launch reads SCAL_RHOLAST (the threads
// of k_cg_direction_beta do), and behind it lambda = rholast / <p, q> is rho / <p, q>.
// p = (rho / rholast) p + q
__global__ void k_cg_direction_beta(int64_t n, double *scal, const double *__restrict__ q, double *__restrict__ p)
{
  const double beta = scal[SCAL_RHO] / scal[SCAL_RHOLAST];
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) p[i] = beta * p[i] + q[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) scal[SCAL_BETA] = beta;
}
// k_cg_update_norm with lambda = scal[num] / scal[SCAL_PQ] (num: SCAL_RHOLAST in the first iteration, where nothing has written
// SCAL_RHO, SCAL_RHO afterwards), rholast = scal[num], and the sum finished by reduce_finish into out[0]
template <bool MASKED>
__global__ __launch_bounds__(WG) void k_cg_update_norm_fin(int64_t n, double *scal, int num, const uint8_t *__restrict__ mask, const double *__restrict__ p,
                                                            const double *__restrict__ q, double *__restrict__ x, double *__restrict__ b, double *partial,
                                                            unsigned *ticket, double *out)
{
  __shared__ double red[4];
  const double rho = scal[num];
  const double lam = rho / scal[SCAL_PQ];
  double s = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) {
    x[i] += lam * p[i];
    const double bi = b[i] - lam * q[i];
    b[i] = bi;
    if (!MASKED || mask[i]) s += bi * bi;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    scal[SCAL_STEP] = lam;
    if (num != SCAL_RHOLAST) scal[SCAL_RHOLAST] = rho;
  }
  s = block_sum(s, red);
  reduce_finish(s, partial, ticket, out, red);
}

// ---------------------------------------------------------------------------------------------
// Flexible CG (ddm_fcg_solve, csrc/krylov_fcg.hpp): the orthogonalisation of a fresh direction d against stored slots.
// The stored vectors of a launch, passed by value: vector j of the set is base + buf[j] * stride.
constexpr int FCG_SET_MAX = 16;  // entries of one FcgSet (k_fcg_coef, k_fcg_orth and their block forms take that many per launch)
constexpr int FCG_SG1 = 8;       // slots one pass of k_fcg_project takes (one accumulator each)
struct FcgSet {
  int32_t n;
  int32_t buf[FCG_SET_MAX];
};
// Projection: the owner-masked partial sums of <Ad_j, d> for the set.n <= FCG_SG1 stored images of the set in ONE pass over d; the
// grid, rows per thread, summation order and block_sum of k_dot_partial, so each sum is bit-identical to dot_device(Ad_j, d).
// partial[(j0 + j) * gridDim.x + b]
template <bool MASKED>
__global__ __launch_bounds__(WG) void k_fcg_project(int64_t n, const uint8_t *__restrict__ mask, const double *__restrict__ AD, int64_t stride, FcgSet set,
                                                     int j0, const double *__restrict__ d, double *__restrict__ partial)
{
  __shared__ double red[4];
  double s[FCG_SG1];
  const double *a[FCG_SG1];
#pragma unroll
  for (int j = 0; j < FCG_SG1; ++j) {
    s[j] = 0.0;
    a[j] = AD + (int64_t)set.buf[j < set.n ? j : 0] * stride; // (past the set: a valid address that is never loaded)
  }
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG)
    if (!MASKED || mask[i]) {
      const double di = d[i];
      double ai[FCG_SG1];
#pragma unroll
      for (int j = 0; j < FCG_SG1; ++j) ai[j] = j < set.n ? a[j][i] : 0.0; // every load of the row is issued before the first use
#pragma unroll
      for (int j = 0; j < FCG_SG1; ++j) s[j] += ai[j] * di;
    }
#pragma unroll
  for (int j = 0; j < FCG_SG1; ++j) {
    const double t = block_sum(s[j], red);
    if (threadIdx.x == 0 && j < set.n) partial[(int64_t)(j0 + j) * gridDim.x + blockIdx.x] = t;
  }
}
// coef[j0 + j] = num[j0 + j] / g[set.buf[j]]: the Gram-Schmidt coefficients <Ad_k, d> / <d_k, Ad_k>, formed on the device
__global__ void k_fcg_coef(FcgSet set, int j0, const double *__restrict__ num, const double *__restrict__ g, double *__restrict__ coef)
{
  const int j = threadIdx.x;
  if (j < set.n) coef[j0 + j] = num[j0 + j] / g[set.buf[j]];
}
// Update: d -= sum_j coef[j0 + j] d_j in one read-modify-write of d, the terms in the order of the set: per entry the operations of
// set.n launches of k_axpy_negdev, so d is bit-identical to them (the build does not contract a * b + c)
__global__ __launch_bounds__(WG) void k_fcg_orth(int64_t n, const double *__restrict__ D, int64_t stride, FcgSet set, int j0, const double *__restrict__ coef,
                                                  double *__restrict__ d)
{
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) {
    double w = d[i];
    for (int j = 0; j < set.n; ++j) w -= coef[j0 + j] * D[(int64_t)set.buf[j] * stride + i];
    d[i] = w;
  }
}
// the owner-masked partial sums of <d, Ad> (partial[b]) and <d, b> (partial[gridDim.x + b]) in one pass over d; each in the summation
// order of k_dot_partial
template <bool MASKED>
__global__ __launch_bounds__(WG) void k_fcg_dots(int64_t n, const uint8_t *__restrict__ mask, const double *__restrict__ d, const double *__restrict__ Ad,
                                                  const double *__restrict__ b, double *__restrict__ partial)
{
  __shared__ double red[4];
  double sg = 0.0, sb = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG)
    if (!MASKED || mask[i]) {
      const double di = d[i];
      sg += di * Ad[i];
      sb += di * b[i];
    }
  sg = block_sum(sg, red);
  sb = block_sum(sb, red);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = sg;
    partial[gridDim.x + blockIdx.x] = sb;
  }
}
// g_s = <d, Ad> into its slot and the step alpha = <d, b> / g_s into scal[SCAL_STEP], where k_cg_update_norm reads it; dots: the two sums of
// k_fcg_dots.  g_s == 0 makes the step NaN whatever <d, b> is, so that the driver's NaN test on the defect reports the breakdown.
__global__ void k_fcg_alpha(const double *__restrict__ dots, double *__restrict__ gslot, double *__restrict__ scal)
{
  const double g = dots[0];
  gslot[0] = g;
  scal[SCAL_STEP] = g == 0.0 ? __builtin_nan("") : dots[1] / g;
}

// ---------------------------------------------------------------------------------------------
// K6 coarse restriction d0[(s,j)] = <r_j^s, d_ovlp^s>  (galerkin_preconditioner.hh:165-167):
// a tall-skinny GEMV.  Work item = (chunk of rows inside one subdomain); wave w of the
// workgroup handles vectors w, w+4, ...; lanes stride the rows (coalesced).
static constexpr int COARSE_KMAX = 256; // basis vectors per subdomain (GenEO threshold mode doubles nev up to nev_max, spectra.hh:157-163)
struct RowChunk {
  int64_t r0, r1;
  int32_t sub, pad;
};
// a wave-uniform global pointer in scalar registers: loads through it take the scalar base + 32-bit lane offset form
typedef const __attribute__((address_space(1))) double *uniform_gptr;
__device__ __forceinline__ uniform_gptr uniform_global(const double *p)
{
  const uint64_t v = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (uniform_gptr)(((uint64_t)hi << 32) | lo);
}
// Vectors of one group of a restriction pass: the defect is loaded once per group, not once per vector.  10 is the largest count with
// which k_coarse_restrict_spread stays within its 80 VGPRs (make resource-usage); the full-grid kernel's waves take five vectors each
// at the usual 20 (82 VGPRs there, no scratch; about 50 instead of 64 us per launch in the setup's Galerkin products at 216^3).
constexpr int COARSE_JG = 10, COARSE_JG_FULL = 5;
// One wave, the JG vectors b0, b0 + vstride, ... over the rows of chunk `c`: out[jj * ostride] = <b_jj, d>.  Per trip of 8 x 64 rows a
// lane loads its 8 defect values once, then the 8 basis values of each vector (two vectors = 16 loads in flight) and adds
// s_jj += b * d in ascending row; the rows of an incomplete last trip one by one.  Per (lane, vector) that is rows r0 + l + 64 t in
// ascending t, then wave_sum: whatever JG, the sums of the one-vector-at-a-time loop (JG = 1) in the same order.
template <int JG>
__device__ __forceinline__ void restrict_group(const double *__restrict__ b0, int64_t vstride, const RowChunk c, int lane,
                                               const double *__restrict__ d, double *__restrict__ out, int ostride)
{
  double s[JG];
#pragma unroll
  for (int jj = 0; jj < JG; ++jj) s[jj] = 0.0;
  int64_t rb = c.r0;
  for (; rb + 8 * 64 <= c.r1; rb += 8 * 64) { // (the wave's trip base: uniform, the lane is a 32-bit offset)
    const uniform_gptr dc = uniform_global(d + rb);
    double dv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) dv[u] = __builtin_nontemporal_load(dc + (unsigned)(lane + u * 64));
#pragma unroll
    for (int p = 0; p < JG; p += 2) {
      const int nv = p + 1 < JG ? 2 : 1;
      double bv[2][8];
#pragma unroll
      for (int v = 0; v < nv; ++v) {
        const uniform_gptr bc = uniform_global(b0 + (int64_t)(p + v) * vstride + rb);
#pragma unroll
        for (int u = 0; u < 8; ++u) bv[v][u] = __builtin_nontemporal_load(bc + (unsigned)(lane + u * 64));
      }
#pragma unroll
      for (int v = 0; v < nv; ++v)
#pragma unroll
        for (int u = 0; u < 8; ++u) s[p + v] += bv[v][u] * dv[u];
      __builtin_amdgcn_sched_barrier(0); // (two vectors' loads in flight, not more: the register budget)
    }
  }
  for (; rb < c.r1; rb += 64) {
    if (rb + lane >= c.r1) continue;
    const double dr = __builtin_nontemporal_load(d + rb + lane);
    const uniform_gptr bc = uniform_global(b0 + rb);
#pragma unroll
    for (int jj = 0; jj < JG; ++jj) s[jj] += bc[(int64_t)jj * vstride + lane] * dr;
  }
#pragma unroll
  for (int jj = 0; jj < JG; ++jj) {
    const double t = wave_sum(s[jj]);
    if (lane == 0) out[(int64_t)jj * ostride] = t;
  }
}
__global__ __launch_bounds__(WG) void k_coarse_restrict_partial(int kmax, int64_t ld, const double *__restrict__ basis,
                                                                 const double *__restrict__ d, const RowChunk *__restrict__ chunks,
                                                                 double *__restrict__ partial /* [nchunk][kmax] */, int nchunk)
{
  // (grid-stride over the chunks: a small grid keeps the kernel's footprint per CU low when it runs beside the local solve)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const RowChunk c = chunks[ch];
    int j = w; // the wave's vectors w, w + 4, ...: in groups, the rest one by one
    for (; j + 4 * (COARSE_JG_FULL - 1) < kmax; j += 4 * COARSE_JG_FULL)
      restrict_group<COARSE_JG_FULL>(basis + (int64_t)j * ld, 4 * ld, c, lane, d, partial + (int64_t)ch * kmax + j, 4);
    for (; j < kmax; j += 4) restrict_group<1>(basis + (int64_t)j * ld, 4 * ld, c, lane, d, partial + (int64_t)ch * kmax + j, 4);
  }
}
// one workgroup: sums the chunk partials of each (subdomain, vector) in chunk order and scatters
// them to the global coarse vector (zero elsewhere, so that an all-reduce assembles d0)
__global__ __launch_bounds__(WG) void k_coarse_restrict_final(int nsub, int kmax, const int32_t *__restrict__ sub_chunk_ptr,
                                                               const double *__restrict__ partial,
                                                               const int64_t *__restrict__ coarse_index, int64_t K,
                                                               double *__restrict__ d0)
{
  for (int64_t i = threadIdx.x; i < K; i += WG) d0[i] = 0.0;
  __syncthreads();
  for (int t = threadIdx.x; t < nsub * kmax; t += WG) {
    const int s = t / kmax, j = t % kmax;
    const int64_t gi = coarse_index[t];
    if (gi < 0) continue;
    double acc = 0.0;
    for (int c = sub_chunk_ptr[s]; c < sub_chunk_ptr[s + 1]; ++c) acc += partial[(int64_t)c * kmax + j];
    d0[gi] = acc;
  }
}
// K8: x0 = A0^-1 d0 with the replicated explicit inverse (K x K, row-major); one wave per row
__global__ __launch_bounds__(WG) void k_dense_mv(int64_t K, const double *__restrict__ M, const double *__restrict__ v,
                                                  double *__restrict__ out)
{
  const int lane = threadIdx.x & 63;
  const int64_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= K) return;
  double s = 0.0;
  for (int64_t c = lane; c < K; c += 64) s += M[row * K + c] * v[c];
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}
// K7 prolongation x_ovlp = sum_j c_j r_j  (galerkin_preconditioner.hh:186-188)
__global__ __launch_bounds__(WG) void k_coarse_prolong(int kmax, int64_t ld, const double *__restrict__ basis,
                                                        const double *__restrict__ x0, const int64_t *__restrict__ coarse_index,
                                                        const RowChunk *__restrict__ chunks, double *__restrict__ xov, int nchunk)
{
  __shared__ double cj[COARSE_KMAX];
  static_assert(COARSE_KMAX <= WG, "one thread per coefficient");
  for (int ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
  const RowChunk c = chunks[ch];
  __syncthreads(); // cj of the previous chunk is no longer read
  if (threadIdx.x < kmax) {
    const int64_t gi = coarse_index[(int64_t)c.sub * kmax + threadIdx.x];
    cj[threadIdx.x] = gi >= 0 ? x0[gi] : 0.0;
  }
  __syncthreads();
  // two rows per thread and trip, four basis vectors of each in flight (added in order; kmax is usually a multiple of 4)
  for (int64_t r = c.r0 + threadIdx.x; r < c.r1; r += 2 * WG) {
    const int64_t r2 = r + WG < c.r1 ? r + WG : r; // (the second row of the last trip may not exist: computed twice, stored once)
    double s = 0.0, s2 = 0.0;
    int j = 0;
    for (; j + 4 <= kmax; j += 4) {
      double bv[4], bw[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) bv[u] = __builtin_nontemporal_load(basis + (int64_t)(j + u) * ld + r);
#pragma unroll
      for (int u = 0; u < 4; ++u) bw[u] = __builtin_nontemporal_load(basis + (int64_t)(j + u) * ld + r2);
#pragma unroll
      for (int u = 0; u < 4; ++u) s += cj[j + u] * bv[u];
#pragma unroll
      for (int u = 0; u < 4; ++u) s2 += cj[j + u] * bw[u];
    }
    for (; j < kmax; ++j) {
      s += cj[j] * basis[(int64_t)j * ld + r];
      s2 += cj[j] * basis[(int64_t)j * ld + r2];
    }
    xov[r] = s;
    if (r2 != r) xov[r2] = s2;
  }
  }
}

// ---- the two passes over the basis, spread: for the coarse chain that runs on a side stream BESIDE the single-launch local solve.
// Workgroups of ONE wave (how many, the launch decides), persistent over the work items in grid-stride order: the CUs carry a
// small share of the stream each, and a wave needs few enough registers (at most 80; make resource-usage: 80 the restriction, 66 the
// prolongation, no scratch) to fit on a SIMD next to two waves of k_trsv_pipe.  128 bytes per lane are in flight.  Same sums in the
// same order as the full-grid kernels above.
constexpr int SPREAD_WG = 64;
// one partial per (chunk, j), a work item is (chunk, group of COARSE_JG consecutive vectors): restrict_group above
__global__ __launch_bounds__(SPREAD_WG) void k_coarse_restrict_spread(int kmax, int64_t ld, const double *__restrict__ basis,
                                                                       const double *__restrict__ d, const RowChunk *__restrict__ chunks,
                                                                       double *__restrict__ partial /* [nchunk][kmax] */, int nchunk)
{
  const int lane = threadIdx.x;
  const int nfull = kmax / COARSE_JG, ngroup = nfull + (kmax % COARSE_JG != 0); // (the vectors of a short last group: one by one)
  const int64_t nitem = (int64_t)nchunk * ngroup; // (item = chunk * ngroup + group: the waves that run together share few chunks of d)
  for (int64_t item = blockIdx.x; item < nitem; item += gridDim.x) {
    const int ch = (int)(item / ngroup), g = (int)(item % ngroup);
    const RowChunk c = chunks[ch];
    const double *b0 = basis + (int64_t)g * COARSE_JG * ld;
    double *out = partial + (int64_t)ch * kmax + g * COARSE_JG;
    if (g < nfull)
      restrict_group<COARSE_JG>(b0, ld, c, lane, d, out, 1);
    else
      for (int j = 0; j < kmax - nfull * COARSE_JG; ++j) restrict_group<1>(b0 + (int64_t)j * ld, ld, c, lane, d, out + j, 1);
  }
}
// Two neighbouring rows per lane and 16-byte load: a trip is two strips of 128 rows, four basis vectors of each in flight; per row the
// vectors are added in ascending j.  The basis' leading dimension is a multiple of 64 rows, so that an even row is 16-byte aligned in
// every vector: a chunk that starts at an odd row has that row taken alone, and so is an odd last row.
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) double2_t *uniform_gptr2;
__global__ __launch_bounds__(SPREAD_WG) void k_coarse_prolong_spread(int kmax, int64_t ld, const double *__restrict__ basis,
                                                                      const double *__restrict__ x0, const int64_t *__restrict__ coarse_index,
                                                                      const RowChunk *__restrict__ chunks, double *__restrict__ xov, int nchunk)
{
  __shared__ double cj[COARSE_KMAX];
  const int lane = threadIdx.x;
  for (int ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const RowChunk c = chunks[ch];
    __syncthreads(); // cj of the previous chunk is no longer read
    for (int j = lane; j < kmax; j += SPREAD_WG) {
      const int64_t gi = coarse_index[(int64_t)c.sub * kmax + j];
      cj[j] = gi >= 0 ? x0[gi] : 0.0;
    }
    __syncthreads();
    const int64_t ra = c.r0 + (c.r0 & 1), re = ra + ((c.r1 - ra) & ~(int64_t)1); // the row pairs are [ra, re), ra even
    {
      const int64_t rs = lane == 0 && ra != c.r0 ? c.r0 : lane == 1 && re < c.r1 ? re : -1; // the single rows, one lane each
      if (rs >= 0) {
        double s = 0.0;
        for (int j = 0; j < kmax; ++j) s += cj[j] * basis[(int64_t)j * ld + rs];
        xov[rs] = s;
      }
    }
    for (int64_t rb = ra; rb < re; rb += 4 * SPREAD_WG) { // (uniform trip base + 32-bit lane offsets: scalar-base addressing, few registers)
      const int npair = (int)(re - rb < 4 * SPREAD_WG ? re - rb : 4 * SPREAD_WG) / 2;
      if (lane >= npair) continue;
      unsigned lo[2]; // (a pair of the last trip that does not exist: the lane's first pair, computed again and not stored)
#pragma unroll
      for (int q = 0; q < 2; ++q) lo[q] = (unsigned)(lane + q * SPREAD_WG < npair ? lane + q * SPREAD_WG : lane);
      double2_t s[2] = {{0.0, 0.0}, {0.0, 0.0}};
      int j = 0;
#pragma unroll 1
      for (; j + 4 <= kmax; j += 4) {
        double2_t bv[2][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uniform_gptr2 bc = (uniform_gptr2)uniform_global(basis + (int64_t)(j + u) * ld + rb);
#pragma unroll
          for (int q = 0; q < 2; ++q) bv[q][u] = __builtin_nontemporal_load(bc + lo[q]);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const double cu = cj[j + u];
            s[q].x += cu * bv[q][u].x;
            s[q].y += cu * bv[q][u].y;
          }
      }
      for (; j < kmax; ++j) {
        const double2_t *bc = (const double2_t *)(basis + (int64_t)j * ld + rb);
        const double cu = cj[j];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const double2_t b = bc[lo[q]];
          s[q].x += cu * b.x;
          s[q].y += cu * b.y;
        }
      }
      double2_t *xo = (double2_t *)(xov + rb);
      xo[lo[0]] = s[0];
      if (lo[1] != (unsigned)lane) xo[lo[1]] = s[1];
    }
  }
}

} // namespace ddm
