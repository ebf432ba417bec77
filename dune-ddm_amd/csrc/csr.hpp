// Sparse matrices (struct ddm_csr): creation and validation, the row-block schedule of the CSR-stream product, the cache-blocked
// row order of the block products, library-internal adoption of host arrays with a background upload, and the products up to
// ddm_csr_mm.  Also host_threads / hvec_copy, which the setup phases of the later files share.  Needs context.hpp.
#pragma once

// ---- CSR ---------------------------------------------------------------------------------------
// Worker threads of the host-side setup phases (factorisations, schedules, assembly): the cores of the machine, but never more than
// 16 per process -- a node runs one process per GPU, and several of these pools are alive at the same time (DDM_HOST_THREADS overrides).
static unsigned host_threads()
{
  static const unsigned n = []() {
    if (const char *e = std::getenv("DDM_HOST_THREADS")) return (unsigned)std::max(1, std::atoi(e));
    return std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  }();
  return n;
}

// dst = src with `threads` memcpy workers (fresh pages: the copy is page-fault bound on one thread)
template <class T>
static void hvec_copy(hvec<T> &dst, const T *src, size_t n)
{
  dst.resize(n);
  const size_t nth = std::min<size_t>(host_threads(), std::max<size_t>(1, n >> 22));
  if (nth <= 1) {
    if (n) std::memcpy(dst.data(), src, sizeof(T) * n);
    return;
  }
  std::vector<std::thread> th;
  for (size_t t = 0; t < nth; ++t)
    th.emplace_back([&, t]() {
      const size_t a = n * t / nth, b = n * (t + 1) / nth;
      std::memcpy(dst.data() + a, src + a, sizeof(T) * (b - a));
    });
  for (auto &t : th) t.join();
}

struct ddm_csr {
  int64_t nrows = 0, ncols = 0, nnz = 0;
  hvec<int64_t> h_rp; // host copies are kept for the ILU(0) factorisation / analysis
  hvec<int32_t> h_ci;
  hvec<double> h_va;
  // Device arrays.  The pattern is read through the views rp / ci / blk_row: they point at this matrix's own arrays (own_*) or, for
  // a values-only companion on another matrix's pattern (csr_adopt), at that matrix's, which has to outlive the companion.
  dbuf<int64_t> own_rp;
  dbuf<int32_t> own_ci, own_blk_row;
  int64_t *rp = nullptr;
  int32_t *ci = nullptr;
  dbuf<double> va;
  int32_t *blk_row = nullptr;
  int nblk = 0;
  bool host_only = false;       // created by ddm_csr_create_host: no device arrays
  dbuf<int32_t> row_order;      // cache-blocked processing order of the rows for the block products (csr_row_order_tiled), or empty
  std::thread uploader;          // device copies still in flight (csr_adopt): csr_wait_upload joins it
  int upload_rc = 0;
  std::string upload_err;
  void view_pattern_of(const ddm_csr &P) { rp = P.own_rp, ci = P.own_ci, blk_row = P.own_blk_row, nblk = P.nblk; }
};

// row-block schedule of the CSR-stream kernel: <= SPMV_NNZ non-zeros and <= WG rows per block, a row longer than SPMV_NNZ gets a
// block of its own
static std::vector<int32_t> csr_row_blocks(int64_t nrows, const int64_t *rowptr)
{
  std::vector<int32_t> blk;
  blk.push_back(0);
  int64_t r = 0;
  while (r < nrows) {
    int64_t r1 = r;
    const int64_t z0 = rowptr[r];
    while (r1 < nrows && r1 - r < WG && rowptr[r1 + 1] - z0 <= SPMV_NNZ) ++r1;
    if (r1 == r) r1 = r + 1; // long row
    blk.push_back((int32_t)r1);
    r = r1;
  }
  return blk;
}
static int csr_create_impl(ddm_ctx *ctx, int64_t nrows, int64_t ncols, const int64_t *rowptr, const int32_t *col, const double *val, bool host_only, ddm_csr **out)
{
  if (!ctx || !out || nrows < 0 || !rowptr) return fail(ctx, DDM_EINVAL, "ddm_csr_create: bad arguments");
  if (nrows >= (int64_t)1 << 31 || ncols >= (int64_t)1 << 31) return fail(ctx, DDM_EINVAL, "matrix dimension exceeds int32 columns");
  const int64_t nnz = rowptr[nrows];
  for (int64_t i = 0; i < nrows; ++i)
    if (rowptr[i + 1] < rowptr[i]) return fail(ctx, DDM_EINVAL, "row pointers not monotone at row %lld", (long long)i);
  for (int64_t k = 0; k < nnz; ++k)
    if (col[k] < 0 || col[k] >= ncols) return fail(ctx, DDM_EINVAL, "column index out of range at entry %lld", (long long)k);
  auto A = std::make_unique<ddm_csr>();
  A->nrows = nrows;
  A->ncols = ncols;
  A->nnz = nnz;
  hvec_copy(A->h_rp, rowptr, (size_t)nrows + 1);
  hvec_copy(A->h_ci, col, (size_t)nnz);
  hvec_copy(A->h_va, val, (size_t)nnz);
  const std::vector<int32_t> blk = csr_row_blocks(nrows, rowptr);
  A->nblk = (int)blk.size() - 1;
  if (host_only) { // analysis / assembly input only (the GenEO pencil is built from the host arrays): no device copy
    A->host_only = true;
    A->nblk = 0;
    *out = A.release();
    return DDM_OK;
  }
  DDMCHECK(upload(ctx, rowptr, nrows + 1, A->own_rp));
  DDMCHECK(upload(ctx, col, nnz, A->own_ci));
  DDMCHECK(upload(ctx, val, nnz, A->va));
  DDMCHECK(upload(ctx, blk.data(), (int64_t)blk.size(), A->own_blk_row));
  A->view_pattern_of(*A);
  *out = A.release();
  return DDM_OK;
}
extern "C" int ddm_csr_create(ddm_ctx *ctx, int64_t nrows, int64_t ncols, const int64_t *rowptr, const int32_t *col, const double *val, ddm_csr **out)
{
  return csr_create_impl(ctx, nrows, ncols, rowptr, col, val, false, out);
}
// the same object WITHOUT device arrays: valid as A_neu / B_neu of ddm_geneo_basis (the pencil is assembled from the host arrays) and
// of the other coarse-space builders' host inputs; every entry point that would touch the device arrays returns DDM_EINVAL
extern "C" int ddm_csr_create_host(ddm_ctx *ctx, int64_t nrows, int64_t ncols, const int64_t *rowptr, const int32_t *col, const double *val, ddm_csr **out)
{
  return csr_create_impl(ctx, nrows, ncols, rowptr, col, val, true, out);
}
extern "C" void ddm_csr_destroy(ddm_csr *A)
{
  if (!A) return;
  if (A->uploader.joinable()) A->uploader.join(); // (it writes the members)
  delete A;
}
// Library-internal constructors for matrices the library assembled itself (GenEO pencil): the host arrays are MOVED in (no copy, no
// validation pass), and the device copies are made by a helper thread while the caller goes on with host work on the host arrays
// (factorisation, analysis).  Everything that touches the device arrays calls csr_wait_upload first.
static int csr_wait_upload(ddm_ctx *ctx, const ddm_csr *A)
{
  ddm_csr *M = const_cast<ddm_csr *>(A);
  if (M->uploader.joinable()) M->uploader.join();
  if (M->upload_rc) return fail(ctx, M->upload_rc, "%s", M->upload_err.c_str());
  return DDM_OK;
}
// New values in the pattern the matrix has (Newton step, time step): h_va, and the device `va` on the context's stream.  Objects
// built on the matrix keep what they made of the old values until their own refresh is called (ddm_op_refresh, ddm_ilu0_refresh,
// ddm_schwarz_refresh).  Synchronous: the host array is free again when the call returns.
extern "C" int ddm_csr_set_values(ddm_ctx *ctx, ddm_csr *A, const double *val_host)
{
  if (!ctx || !A || (!val_host && A->nnz > 0)) return fail(ctx, DDM_EINVAL, "ddm_csr_set_values: bad arguments");
  DDMCHECK(csr_wait_upload(ctx, A)); // (a helper thread may still be reading h_va)
  if (A->nnz == 0) return DDM_OK;
  if (val_host != A->h_va.data()) hvec_copy(A->h_va, val_host, (size_t)A->nnz);
  if (A->host_only) return DDM_OK;
  HIPCHECK(ctx, hipMemcpyAsync(A->va, A->h_va.data(), sizeof(double) * (size_t)A->nnz, hipMemcpyHostToDevice, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DDM_OK;
}
// Cache-blocked processing order of the rows of a block-diagonal matrix whose blocks come from a STRUCTURED grid in lexicographic
// numbering (possibly followed by irregularly numbered rows, e.g. an overlap shell): the strides s2 (one grid line) and s3 (one grid
// plane) are read off the column offsets that most rows share; rows are then visited brick by brick (16 x 4 x 4 points, bricks in
// lexicographic order), rows that fit no brick keep their place at the end.  Purely a performance hint -- any permutation is valid.
// Returns false (order untouched) when no such structure is found.
static bool csr_row_order_tiled(int64_t nblocks, const int64_t *block_ptr, const int64_t *rp, const int32_t *ci, std::vector<int32_t> &order)
{
  const int64_t n = block_ptr[nblocks];
  order.resize((size_t)n);
  std::vector<uint8_t> seen((size_t)n, 0);
  int64_t out = 0;
  bool any = false;
  for (int64_t b = 0; b < nblocks; ++b) {
    const int64_t r0 = block_ptr[b], r1 = block_ptr[b + 1], nb = r1 - r0;
    int64_t s2 = 0, s3 = 0;
    if (nb >= 4096) { // positive column offsets shared by most of a sample of rows from the first half of the block
      std::map<int64_t, int> hist;
      const int64_t sample = 2048, start = r0 + nb / 4;
      for (int64_t i = start; i < start + sample; ++i)
        for (int64_t k = rp[i]; k < rp[i + 1]; ++k)
          if (ci[k] > i) hist[ci[k] - i]++;
      std::vector<int64_t> P;
      for (auto &kv : hist)
        if (kv.second > sample / 2) P.push_back(kv.first);
      auto has = [&](int64_t o) { return std::binary_search(P.begin(), P.end(), o); };
      // 5- / 7-point stencils share the offsets {1, s2, s3}; 9- / 27-point ones {1, s2 - 1, s2, s2 + 1, s3 - s2 - 1, ..., s3 + s2 + 1}
      if (P.size() >= 2 && P[0] == 1) {
        const int64_t a = P[1];
        if (has(a + 1) && has(a + 2)) s2 = a + 1;
        else if (!has(a + 1)) s2 = a;
        if (s2 > 1) {
          auto it = std::upper_bound(P.begin(), P.end(), s2 + 1);
          if (it == P.end()) s3 = ((nb + s2 - 1) / s2) * s2; // two-dimensional: one plane
          else {
            const int64_t c = *it;
            if (has(c + 1) && has(c + 2)) s3 = has(c + s2 + 1) ? c + s2 + 1 : 0;
            else if (!has(c + 1)) s3 = c;
          }
        }
      }
      if (s2 < 4 || s3 < 2 * s2) s2 = s3 = 0;
    }
    if (!s2) {
      for (int64_t r = r0; r < r1; ++r) order[(size_t)out++] = (int32_t)r;
      continue;
    }
    any = true;
    const int64_t ny = s3 / s2, nz = (nb + s3 - 1) / s3;
    constexpr int64_t TX = 16, TY = 4, TZ = 4;
    for (int64_t z0 = 0; z0 < nz; z0 += TZ)
      for (int64_t y0 = 0; y0 < ny; y0 += TY)
        for (int64_t x0 = 0; x0 < s2; x0 += TX)
          for (int64_t z = z0; z < std::min(z0 + TZ, nz); ++z)
            for (int64_t y = y0; y < std::min(y0 + TY, ny); ++y)
              for (int64_t x = x0; x < std::min(x0 + TX, s2); ++x) {
                const int64_t r = x + y * s2 + z * s3;
                if (r < nb && !seen[(size_t)(r0 + r)]) {
                  seen[(size_t)(r0 + r)] = 1;
                  order[(size_t)out++] = (int32_t)(r0 + r);
                }
              }
    for (int64_t r = r0; r < r1; ++r) // (planes with s3 % s2 leftovers)
      if (!seen[(size_t)r]) order[(size_t)out++] = (int32_t)r;
  }
  return any && out == n;
}
// host-only entry for the CPU tests: order_out[n]; returns 1 when a grid structure was found (else order_out is the identity)
extern "C" int ddm_csr_row_order_tiled_host(int64_t nblocks, const int64_t *block_ptr, const int64_t *rowptr, const int32_t *col, int32_t *order_out)
{
  if (nblocks < 1 || !block_ptr || !rowptr || !col || !order_out || block_ptr[0] != 0) return DDM_EINVAL;
  std::vector<int32_t> order;
  const bool found = csr_row_order_tiled(nblocks, block_ptr, rowptr, col, order);
  std::memcpy(order_out, order.data(), sizeof(int32_t) * order.size());
  return found ? 1 : 0;
}
static ddm_csr *csr_adopt(ddm_ctx *ctx, int64_t n, hvec<int64_t> &&rp, hvec<int32_t> &&ci, hvec<double> &&va, hvec<double> &&companion_values, ddm_csr **companion,
                          int64_t nblocks = 0, const int64_t *block_ptr = nullptr /* diagonal blocks: builds the cache-blocked row order of the block products */)
{
  ddm_csr *A = new ddm_csr, *C = new ddm_csr;
  A->nrows = A->ncols = C->nrows = C->ncols = n;
  A->nnz = C->nnz = rp[(size_t)n];
  A->h_rp = std::move(rp);
  A->h_ci = std::move(ci);
  A->h_va = std::move(va);
  *companion = C; // values only: views A's pattern
  const int device = ctx->device;
  auto cv = std::make_shared<hvec<double>>(std::move(companion_values));
  std::vector<int64_t> bp(block_ptr ? block_ptr : nullptr, block_ptr ? block_ptr + nblocks + 1 : nullptr);
  A->uploader = std::thread([A, C, cv, device, bp]() {
    auto up = [&](const auto &src, auto &dst) {
      if (A->upload_rc) return;
      hipError_t e = dst.alloc((int64_t)src.size());
      if (e == hipSuccess && src.size()) e = hipMemcpy(dst, src.data(), sizeof(src[0]) * src.size(), hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        A->upload_rc = DDM_EHIP;
        A->upload_err = std::string("matrix upload failed: ") + hipGetErrorString(e);
      }
    };
    (void)hipSetDevice(device);
    const std::vector<int32_t> blk = csr_row_blocks(A->nrows, A->h_rp.data());
    A->nblk = (int)blk.size() - 1;
    up(A->h_rp, A->own_rp);
    up(A->h_ci, A->own_ci);
    up(A->h_va, A->va);
    up(blk, A->own_blk_row);
    up(*cv, C->va);
    if (bp.size() >= 2 && !std::getenv("DDM_SPMM_NATURAL_ORDER")) {
      std::vector<int32_t> order;
      if (csr_row_order_tiled((int64_t)bp.size() - 1, bp.data(), A->h_rp.data(), A->h_ci.data(), order)) up(order, A->row_order);
    }
    A->view_pattern_of(*A);
    C->view_pattern_of(*A);
  });
  return A;
}
extern "C" int64_t ddm_csr_rows(const ddm_csr *A) { return A->nrows; }
extern "C" int64_t ddm_csr_nnz(const ddm_csr *A) { return A->nnz; }

static int csr_mv_impl(ddm_ctx *ctx, const ddm_csr *A, double alpha, const double *x, double *y, bool acc)
{
  if (A->host_only) return fail(ctx, DDM_EINVAL, "the matrix was created without device arrays (ddm_csr_create_host)");
  if (A->nblk == 0) return DDM_OK;
  if (acc)
    hipLaunchKernelGGL(k_spmv_stream<true>, dim3(A->nblk), dim3(WG), 0, ctx->stream, A->rp, A->ci, A->va, A->blk_row, A->nblk, x, y, alpha);
  else
    hipLaunchKernelGGL(k_spmv_stream<false>, dim3(A->nblk), dim3(WG), 0, ctx->stream, A->rp, A->ci, A->va, A->blk_row, A->nblk, x, y, alpha);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_csr_mv(ddm_ctx *ctx, const ddm_csr *A, const double *x, double *y)
{
  if (x == y) return fail(ctx, DDM_EINVAL, "ddm_csr_mv: x and y alias");
  return csr_mv_impl(ctx, A, 1.0, x, y, false);
}
extern "C" int ddm_csr_usmv(ddm_ctx *ctx, const ddm_csr *A, double alpha, const double *x, double *y)
{
  if (x == y) return fail(ctx, DDM_EINVAL, "ddm_csr_usmv: x and y alias");
  return csr_mv_impl(ctx, A, alpha, x, y, true);
}

// Y = A X, row-major n x nrhs block vectors with leading dimensions ldx / ldy (MatOp::perform_op on a block; spectra.hh:100-105)
static int csr_mm_ld(ddm_ctx *ctx, const ddm_csr *A, int nrhs, const double *X, int64_t ldx, double *Y, int64_t ldy)
{
  if (!A || !X || !Y || X == Y || nrhs < 1 || ldx < nrhs || ldy < nrhs) return fail(ctx, DDM_EINVAL, "ddm_csr_mm: bad arguments");
  if (A->host_only) return fail(ctx, DDM_EINVAL, "the matrix was created without device arrays (ddm_csr_create_host)");
  const int64_t threads = A->nrows * (int64_t)nrhs;
  if (threads == 0) return DDM_OK;
  if (nrhs % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)X & 31) == 0 && ((uintptr_t)Y & 31) == 0) {
    hipLaunchKernelGGL(k_spmm_rowmajor4<false>, dim3((unsigned)((threads / 4 + WG - 1) / WG)), dim3(WG), 0, ctx->stream, A->nrows, nrhs / 4, A->rp, A->ci, A->va,
                       (const double *)nullptr, X, ldx, Y, (double *)nullptr, ldy);
    HIPCHECK(ctx, hipGetLastError());
    return DDM_OK;
  }
  hipLaunchKernelGGL(k_spmm_rowmajor, dim3((unsigned)((threads + WG - 1) / WG)), dim3(WG), 0, ctx->stream, A->nrows, nrhs, A->rp, A->ci,
                     A->va, X, ldx, Y, ldy);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
// Y1 = A1 X, Y2 = A2 X for two matrices on ONE pattern (same rp / ci arrays in value; checked by size only: internal use)
static int csr_mm2_ld(ddm_ctx *ctx, const ddm_csr *A1, const ddm_csr *A2, int nrhs, const double *X, int64_t ldx, double *Y1, double *Y2, int64_t ldy)
{
  const bool fast = A1->nrows == A2->nrows && A1->nnz == A2->nnz && nrhs % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)X & 31) == 0 && ((uintptr_t)Y1 & 31) == 0 &&
                    ((uintptr_t)Y2 & 31) == 0 && X != Y1 && X != Y2;
  if (!fast) {
    DDMCHECK(csr_mm_ld(ctx, A1, nrhs, X, ldx, Y1, ldy));
    return csr_mm_ld(ctx, A2, nrhs, X, ldx, Y2, ldy);
  }
  if (A1->host_only || A2->host_only) return fail(ctx, DDM_EINVAL, "the matrix was created without device arrays (ddm_csr_create_host)");
  const int64_t threads = A1->nrows * (int64_t)(nrhs / 4);
  if (threads == 0) return DDM_OK;
  if (A1->row_order && nrhs / 4 <= 8) { // cache-blocked row order: 64 rows per workgroup
    const int nq = nrhs / 4;
    hipLaunchKernelGGL(k_spmm_rowmajor4_tiled<true>, dim3((unsigned)((A1->nrows + 63) / 64)), dim3(64 * nq), 0, ctx->stream, A1->nrows, nq, A1->row_order, A1->rp, A1->ci, A1->va,
                       (const double *)A2->va, X, ldx, Y1, Y2, ldy);
    HIPCHECK(ctx, hipGetLastError());
    return DDM_OK;
  }
  hipLaunchKernelGGL(k_spmm_rowmajor4<true>, dim3((unsigned)((threads + WG - 1) / WG)), dim3(WG), 0, ctx->stream, A1->nrows, nrhs / 4, A1->rp, A1->ci, A1->va,
                     (const double *)A2->va, X, ldx, Y1, Y2, ldy);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_csr_mm(ddm_ctx *ctx, const ddm_csr *A, int nrhs, const double *X, double *Y) { return csr_mm_ld(ctx, A, nrhs, X, nrhs, Y, nrhs); }

// ---- diagonal row blocks (the layout of k_spmv_dia; ddm_op builds one of its matrix) ---------------------------------------------
// Rows are split greedily into blocks of at most WG consecutive rows whose entries lie on at most DIA_MAX distinct diagonals.  A
// block ends early before the row that would exceed the table, and before a row that brings a diagonal in where the matrix
// decouples (no entry joins the rows before with the rows from there on: a subdomain boundary of a concatenated matrix).
// A row that cannot join any block (more than DIA_MAX entries, columns not strictly ascending) and blocks whose slabs would be
// less than half full (irregular rows: a few rows on DIA_MAX diagonals) stay CSR-stream blocks, cut as csr_row_blocks cuts them.
// The split restarts every DIA_SPLIT_ROWS rows so that it runs on host_threads() workers and does not depend on their number.
// Consecutive diagonal blocks between two decoupling ends whose offsets together stay within DIA_MAX form a segment on the union
// table; its slabs are laid out segment-wide, val[slab * rows + row].  A segment keeps only the slabs of the offsets >= 0 when
// its table is its own mirror image and every entry (r, c) below the diagonal has c inside the segment and a partner (c, r) of
// the same bits: a(r, r + d), d < 0, is then read as val[slab of -d][r + d].
// x windows: the ascending offsets of a segment are grouped into runs, offset k joining the run of k - 1 when off[k] - off[k-1] <= WG
// (joining costs that many doubles of window, a new run costs WG).  A block reads, per run with first offset f and last offset l,
// the WG + (l - f) consecutive doubles x[r0 + f ...] (clamped to the vector): its window; the windows lie back to back, thread t
// finds x[r + off[k]] at lds_pos[k] + t.  A segment whose windows fit DIA_WIN doubles is staged: its blocks load the windows into
// LDS once instead of one x load per diagonal and row (stage_x = false, DDM_SPMV_STAGE_X=0: no segment is).
// Coded blocks: the values of a structured operator repeat, so a block of a staged segment whose rows read at most DIA_DICT distinct
// bit patterns (compared as uint64: +0.0 and -0.0 differ, NaN payloads are kept) stores them once, in a dictionary of DIA_DICT
// doubles in order of first appearance (rows ascending, diagonals ascending inside a row; padded with +0.0), and every row a
// 128-bit word of 4-bit codes, nibble k for diagonal k of the segment's table (absent entries and slots from nd on: code 0, the
// mask decides).  The words are indexed by global row like the mask.  A segment whose blocks are all coded builds no slabs; one
// with any uncoded block keeps them all.  Each block is coded on its own, so the result does not depend on host_threads()
// (code = false, DDM_SPMV_CODE=0: no block is coded).
constexpr int64_t DIA_SPLIT_ROWS = 256 * WG;
struct DiaRun {
  int32_t first, len, start; // first offset, window doubles WG + (last - first), window position
};
struct DiaSegWindows {
  bool staged = false;
  int32_t window = 0; // doubles of all runs
  std::vector<DiaRun> runs;
};
struct DiaLayout {
  std::vector<DiaBlock> blk;
  std::vector<int32_t> stored; // per block: slabs its segment keeps (nd, or the offsets >= 0 of a symmetric segment; 0: CSR-stream)
  std::vector<int32_t> tab;    // per segment: a record of DIA_REC ints (kernels.hpp: DIA_TAB_*; tails of the rows repeat the last entry)
  std::vector<DiaSegWindows> win; // per segment: the runs of its offset table (all of them, staged or not)
  hvec<uint32_t> mask;         // per row: bit k set = the row has an entry on diagonal k of its block's table
  hvec<double> val;            // absent entries 0.0 (loaded, never added); the segments whose blocks are all coded have no slabs
  hvec<uint32_t> code;         // per row: DIA_CODE_WORDS words of 4-bit codes (rows of uncoded blocks: 0), or empty: no block is coded
  hvec<double> dict;           // per coded block, in block order: DIA_DICT doubles
  std::vector<int32_t> ndict;  // per block: dictionary entries in use (0: not coded)
  std::vector<uint8_t> slabs;  // per block: its segment has value slabs (a diagonal block that is not coded reads them)
  int64_t ncoded = 0, slots_slab = 0; // coded blocks; the value slots of the slab layout (what val would hold with no segment coded)
  int64_t ndia = 0, ncsr = 0, rows_dia = 0, nseg = 0, nseg_half = 0; // blocks of either kind, rows in diagonal blocks, segments, symmetric ones
};
template <class F>
static void dia_parallel_for(unsigned threads, int64_t njobs, F &&job)
{
  const unsigned nth = (unsigned)std::max<int64_t>(1, std::min<int64_t>(threads, njobs));
  std::atomic<int64_t> next{0};
  auto work = [&]() {
    for (int64_t j; (j = next.fetch_add(1)) < njobs;) job(j);
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nth; ++t) th.emplace_back(work);
  work();
  for (auto &t : th) t.join();
}
// DDM_SPMV_STAGE_X=0 (read where the layout is built: ddm_op_create, the host entries): no segment stages x (A/B runs, tests)
static bool dia_stage_x_from_env()
{
  const char *e = std::getenv("DDM_SPMV_STAGE_X");
  return !(e && !std::strcmp(e, "0"));
}
// DDM_SPMV_CODE=0 (read at the same places): no block is coded by a dictionary, every segment keeps its slabs
static bool dia_code_from_env()
{
  const char *e = std::getenv("DDM_SPMV_CODE");
  return !(e && !std::strcmp(e, "0"));
}
static void dia_build(int64_t n, const int64_t *rp, const int32_t *ci, const double *va, DiaLayout &L, bool stage_x = true, bool code = true,
                      unsigned threads = host_threads())
{
  L = DiaLayout();
  if (n <= 0 || n >= (int64_t)1 << 30) return; // (row + offset is computed in 32 bits)
  struct Part {
    std::vector<DiaBlock> blk;
    std::vector<int32_t> off; // nd offsets per diagonal block, one after the other
  };
  const int64_t nparts = (n + DIA_SPLIT_ROWS - 1) / DIA_SPLIT_ROWS;
  std::vector<Part> parts((size_t)nparts);
  std::vector<uint8_t> cut((size_t)n, 0); // the matrix decouples before row r (first / last column of the rows: a hint, any value is valid)
  {
    std::vector<int32_t> sufmin((size_t)n + 1, INT32_MAX);
    for (int64_t r = n - 1; r >= 0; --r) sufmin[(size_t)r] = std::min(sufmin[(size_t)r + 1], rp[r + 1] > rp[r] ? ci[rp[r]] : INT32_MAX);
    int32_t prefmax = -1;
    for (int64_t r = 0; r < n; ++r) {
      cut[(size_t)r] = prefmax < r && sufmin[(size_t)r] >= r;
      if (rp[r + 1] > rp[r]) prefmax = std::max(prefmax, ci[rp[r + 1] - 1]);
    }
  }
  dia_parallel_for(threads, nparts, [&](int64_t p) {
    Part &P = parts[(size_t)p];
    const int64_t c0 = p * DIA_SPLIT_ROWS, c1 = std::min(n, c0 + DIA_SPLIT_ROWS);
    int64_t csr_from = -1;
    auto flush_csr = [&](int64_t end) {
      for (int64_t r = csr_from; csr_from >= 0 && r < end;) {
        int64_t r1 = r;
        while (r1 < end && r1 - r < WG && rp[r1 + 1] - rp[r] <= SPMV_NNZ) ++r1;
        if (r1 == r) r1 = r + 1; // long row
        P.blk.push_back(DiaBlock{0, (int32_t)r, (int32_t)r1, 0, 0, 0, 0, -1, 0});
        r = r1;
      }
      csr_from = -1;
    };
    int32_t T[DIA_MAX], R[DIA_MAX], U[2 * DIA_MAX];
    for (int64_t r = c0; r < c1;) {
      int nt = 0; // T[0..nt): the block's offsets so far
      int64_t r1 = r, entries = 0;
      for (; r1 < c1 && r1 - r < WG; ++r1) {
        const int64_t z0 = rp[r1], len = rp[r1 + 1] - z0;
        if (len > DIA_MAX) break;
        bool ascending = true;
        for (int64_t j = 0; j < len; ++j) R[j] = (int32_t)(ci[z0 + j] - r1), ascending = ascending && (j == 0 || R[j] > R[j - 1]);
        const int nu = (int)(std::set_union(T, T + nt, R, R + len, U) - U);
        if (!ascending || nu > DIA_MAX || (r1 > r && nu > nt && cut[(size_t)r1])) break;
        std::copy(U, U + nu, T);
        nt = nu;
        entries += len;
      }
      if (entries > 0 && 2 * entries >= (r1 - r) * nt) {
        flush_csr(r);
        P.blk.push_back(DiaBlock{0, (int32_t)r, (int32_t)r1, nt, (int32_t)P.off.size(), cut[(size_t)r] /* a segment starts here */, 0, -1, 0});
        P.off.insert(P.off.end(), T, T + nt);
        r = r1;
      } else {
        if (csr_from < 0) csr_from = r;
        r = std::max(r1, r + 1);
      }
    }
    flush_csr(c1);
  });
  // segments: runs of diagonal blocks whose tables together stay within DIA_MAX offsets
  struct Seg {
    int64_t r0, r1, base = 0;
    int32_t off[DIA_MAX];
    int nd = 0, nlow = 0; // nlow > 0: symmetric, the nlow offsets < 0 are not stored
    bool staged = false, slabs = true; // slabs = false: every block is coded
    std::atomic<bool> full{false};
    Seg(int64_t a) : r0(a), r1(a) {}
  };
  std::deque<Seg> segs;
  std::vector<int32_t> seg_of;
  for (Part &P : parts)
    for (DiaBlock &B : P.blk) {
      if (B.nd) {
        const int32_t *off = P.off.data() + B.tab;
        int32_t U[2 * DIA_MAX];
        int nu = DIA_MAX + 1;
        if (!segs.empty() && segs.back().r1 == B.r0 && !B.t0) nu = (int)(std::set_union(segs.back().off, segs.back().off + segs.back().nd, off, off + B.nd, U) - U);
        if (nu > DIA_MAX) segs.emplace_back(B.r0), nu = B.nd, std::copy(off, off + B.nd, U);
        std::copy(U, U + nu, segs.back().off);
        segs.back().nd = nu, segs.back().r1 = B.r1;
        ++L.ndia, L.rows_dia += B.r1 - B.r0;
      } else ++L.ncsr;
      seg_of.push_back(B.nd ? (int32_t)segs.size() - 1 : -1);
      L.blk.push_back(B);
    }
  L.stored.assign(L.blk.size(), 0), L.ndict.assign(L.blk.size(), 0), L.slabs.assign(L.blk.size(), 0);
  if (!L.ndia) return; // all CSR: the caller keeps the CSR product
  for (Seg &S : segs) { // a table that is its own mirror image, else full storage
    bool mirror = true;
    for (int k = 0; k < S.nd; ++k) mirror = mirror && S.off[k] == -S.off[S.nd - 1 - k];
    S.full = !mirror;
  }
  dia_parallel_for(threads, (int64_t)L.blk.size(), [&](int64_t b) { // every entry below the diagonal has its partner in the segment, bit for bit
    if (seg_of[(size_t)b] < 0) return;
    Seg &S = segs[(size_t)seg_of[(size_t)b]];
    const DiaBlock &B = L.blk[(size_t)b];
    for (int64_t r = B.r0; r < B.r1 && !S.full; ++r)
      for (int64_t z = rp[r]; z < rp[r + 1] && ci[z] < r; ++z) {
        const int64_t c = ci[z];
        const int32_t *row = ci + rp[c], *end = ci + rp[c + 1], *hit = std::lower_bound(row, end, (int32_t)r);
        if (c < S.r0 || hit == end || *hit != r || std::memcmp(va + (hit - ci), va + z, sizeof(double))) {
          S.full = true;
          break;
        }
      }
  });
  L.nseg = (int64_t)segs.size();
  for (Seg &S : segs) {
    if (!S.full)
      while (S.off[S.nlow] < 0) ++S.nlow;
    L.nseg_half += S.nlow > 0;
    L.slots_slab += (S.nd - S.nlow) * (S.r1 - S.r0);
    DiaSegWindows Wd;
    int32_t pos[DIA_MAX];
    for (int k = 0; k < S.nd; ++k) {
      if (k == 0 || S.off[k] - S.off[k - 1] > WG) Wd.runs.push_back(DiaRun{S.off[k], WG, Wd.window}), Wd.window += WG;
      else Wd.runs.back().len += S.off[k] - S.off[k - 1], Wd.window += S.off[k] - S.off[k - 1];
      pos[k] = Wd.runs.back().start + (S.off[k] - Wd.runs.back().first);
    }
    // (a staged block computes r0 + first + i, i < len, in 32 bits)
    Wd.staged = stage_x && Wd.window <= DIA_WIN && n <= ((int64_t)1 << 30) - WG;
    int32_t rec[DIA_REC] = {};
    for (int k = 0; k < DIA_MAX; ++k) {
      const int q = std::min(k, S.nd - 1);
      rec[DIA_TAB_OFF + k] = S.off[q];
      rec[DIA_TAB_SLAB + k] = q < S.nlow ? S.nd - 1 - q - S.nlow : q - S.nlow; // below the diagonal: the slab of the mirrored offset ...
      rec[DIA_TAB_SHIFT + k] = q < S.nlow ? S.off[q] : 0;                      // ... at the partner's row
      rec[DIA_TAB_POS + k] = Wd.staged ? pos[q] : 0;
    }
    rec[DIA_TAB_STAGED] = S.staged = Wd.staged;
    for (int j = 0; j < DIA_RUNS; ++j) rec[DIA_TAB_RSTART + j] = DIA_WIN; // (a run that is not there starts behind every window)
    if (Wd.staged) { // (at most DIA_RUNS runs fit DIA_WIN doubles: each owns at least WG)
      rec[DIA_TAB_NRUNS] = (int32_t)Wd.runs.size(), rec[DIA_TAB_WINDOW] = Wd.window;
      for (size_t j = 0; j < Wd.runs.size(); ++j)
        rec[DIA_TAB_RFIRST + j] = Wd.runs[j].first, rec[DIA_TAB_RLEN + j] = Wd.runs[j].len, rec[DIA_TAB_RSTART + j] = Wd.runs[j].start;
    }
    L.tab.insert(L.tab.end(), rec, rec + DIA_REC);
    L.win.push_back(std::move(Wd));
  }
  // dictionaries and code words of the blocks of staged segments, block by block
  bool any_staged = false;
  for (const Seg &S : segs) any_staged = any_staged || S.staged;
  if (code && any_staged) {
    L.code.resize((size_t)n * DIA_CODE_WORDS);
    hvec<double> found(L.blk.size() * (size_t)DIA_DICT); // (per block: the patterns in order of first appearance)
    dia_parallel_for(threads, (int64_t)L.blk.size(), [&](int64_t b) {
      const DiaBlock &B = L.blk[(size_t)b];
      uint32_t *words = L.code.data() + (size_t)B.r0 * DIA_CODE_WORDS;
      std::fill(words, words + (size_t)(B.r1 - B.r0) * DIA_CODE_WORDS, 0u);
      if (seg_of[(size_t)b] < 0 || !segs[(size_t)seg_of[(size_t)b]].staged) return;
      const Seg &S = segs[(size_t)seg_of[(size_t)b]];
      uint64_t pat[DIA_DICT];
      int np = 0;
      for (int64_t r = B.r0; r < B.r1 && np <= DIA_DICT; ++r) {
        int k = 0;
        for (int64_t z = rp[r]; z < rp[r + 1]; ++z) {
          while (S.off[k] < ci[z] - r) ++k; // both ascending; the offset is in the table
          uint64_t bits;
          std::memcpy(&bits, va + z, sizeof bits);
          int c = 0;
          while (c < np && pat[c] != bits) ++c;
          if (c == np) {
            if (np == DIA_DICT) { // the 17th pattern: not coded
              np = DIA_DICT + 1;
              break;
            }
            pat[np++] = bits;
          }
          words[(size_t)(r - B.r0) * DIA_CODE_WORDS + k / 8] |= (uint32_t)c << (4 * (k % 8));
        }
      }
      if (np > DIA_DICT) {
        std::fill(words, words + (size_t)(B.r1 - B.r0) * DIA_CODE_WORDS, 0u);
        return;
      }
      L.ndict[(size_t)b] = np; // (a block of a diagonal segment has an entry: np >= 1)
      std::fill(pat + np, pat + DIA_DICT, (uint64_t)0);
      std::memcpy(found.data() + (size_t)b * DIA_DICT, pat, sizeof pat);
    });
    for (Seg &S : segs) S.slabs = false;
    for (size_t b = 0; b < L.blk.size(); ++b) {
      if (seg_of[b] >= 0 && !L.ndict[b]) segs[(size_t)seg_of[b]].slabs = true; // one uncoded block: the segment keeps its slabs
      L.ncoded += L.ndict[b] > 0;
    }
    if (!L.ncoded) L.code = hvec<uint32_t>();
    else {
      L.dict.resize((size_t)L.ncoded * DIA_DICT);
      int32_t at = 0;
      for (size_t b = 0; b < L.blk.size(); ++b)
        if (L.ndict[b]) {
          std::memcpy(L.dict.data() + (size_t)at * DIA_DICT, found.data() + b * DIA_DICT, sizeof(double) * DIA_DICT);
          L.blk[b].dict = at++;
        }
    }
  }
  int64_t slots = 0;
  for (Seg &S : segs) {
    S.base = slots;
    if (S.slabs) slots += (S.nd - S.nlow) * (S.r1 - S.r0);
  }
  for (size_t b = 0; b < L.blk.size(); ++b) {
    if (seg_of[b] < 0) continue;
    const Seg &S = segs[(size_t)seg_of[b]];
    DiaBlock &B = L.blk[b];
    B.nd = S.nd, B.tab = seg_of[b] * DIA_REC;
    B.t0 = (int32_t)(B.r0 - S.r0), B.stride = (int32_t)(S.r1 - S.r0);
    B.base = S.slabs ? S.base + B.t0 : 0;
    L.stored[b] = S.nd - S.nlow, L.slabs[b] = S.slabs;
  }
  L.mask.resize((size_t)n);
  L.val.resize((size_t)slots);
  dia_parallel_for(threads, (int64_t)L.blk.size(), [&](int64_t b) {
    const DiaBlock &B = L.blk[(size_t)b];
    if (!B.nd) {
      std::fill(L.mask.begin() + B.r0, L.mask.begin() + B.r1, 0u);
      return;
    }
    const bool slabs = L.slabs[(size_t)b];
    const int nlow = B.nd - L.stored[(size_t)b];
    double *v = L.val.data() + B.base; // (slab 0, row r0)
    for (int j = 0; slabs && j < B.nd - nlow; ++j) std::fill(v + (int64_t)j * B.stride, v + (int64_t)j * B.stride + (B.r1 - B.r0), 0.0);
    const int32_t *off = L.tab.data() + B.tab + DIA_TAB_OFF;
    for (int64_t r = B.r0; r < B.r1; ++r) {
      uint32_t m = 0;
      int k = 0;
      for (int64_t z = rp[r]; z < rp[r + 1]; ++z) {
        while (off[k] < ci[z] - r) ++k; // both ascending; the offset is in the table
        if (slabs && k >= nlow) v[(int64_t)(k - nlow) * B.stride + (r - B.r0)] = va[z];
        m |= 1u << k;
      }
      L.mask[(size_t)r] = m;
    }
  });
}
// y = A x on the host, indexed as k_spmv_dia indexes (CSR-stream blocks: the row sum in column order)
static void dia_apply_host(const DiaLayout &L, int64_t n, const int64_t *rp, const int32_t *ci, const double *va, const double *x, double *y)
{
  std::vector<double> win((size_t)DIA_WIN);
  for (const DiaBlock &B : L.blk) {
    const int nr = B.r1 - B.r0;
    const int32_t *rec = L.tab.data() + B.tab, *off = rec + DIA_TAB_OFF, *slab = rec + DIA_TAB_SLAB, *shift = rec + DIA_TAB_SHIFT, *pos = rec + DIA_TAB_POS;
    const bool staged = B.nd && rec[DIA_TAB_STAGED];
    if (staged) { // the block's x windows, as the kernel loads them into LDS (every element written before any is read)
      std::fill(win.begin(), win.end(), std::numeric_limits<double>::quiet_NaN());
      for (int j = 0; j < rec[DIA_TAB_NRUNS]; ++j)
        for (int i = 0; i < rec[DIA_TAB_RLEN + j]; ++i)
          win.at((size_t)(rec[DIA_TAB_RSTART + j] + i)) = x[std::min<int64_t>(std::max<int64_t>((int64_t)B.r0 + rec[DIA_TAB_RFIRST + j] + i, 0), n - 1)];
    }
    for (int t = 0; t < nr; ++t) {
      const int r = B.r0 + t;
      double s = 0.0;
      if (!B.nd)
        for (int64_t z = rp[r]; z < rp[r + 1]; ++z) s += va[z] * x[ci[z]];
      else
        for (int k = 0; k < B.nd; ++k) {
          double v;
          if (B.dict >= 0) { // coded (and staged): nibble k of the row's word, through the block's dictionary
            const uint32_t c = (L.code.at((size_t)r * DIA_CODE_WORDS + k / 8) >> (4 * (k % 8))) & (DIA_DICT - 1);
            v = L.dict.at((size_t)B.dict * DIA_DICT + c);
          } else {
            const int64_t at = (int64_t)slab[k] * B.stride + std::min(std::max(B.t0 + t + shift[k], 0), B.stride - 1);
            v = L.val.at((size_t)(B.base - B.t0 + at));
          }
          const double xv = staged ? win.at((size_t)(pos[k] + t)) : x[std::min<int64_t>(std::max<int64_t>(r + off[k], 0), n - 1)];
          if ((L.mask[(size_t)r] >> k) & 1u) s += v * xv; // (-ffp-contract=off: product rounded, then added)
        }
      y[r] = s;
    }
  }
}
// host-only entry for the CPU tests: builds the layout of a square matrix and applies it on the host.  kinds_out (may be null)
// receives up to max_blocks (r0, r1, nd, slabs stored) quadruples; counts_out = {blocks, diagonal blocks, CSR-stream blocks, rows in
// diagonal blocks, value slots, segments, symmetric segments}.  With no diagonal block the operator keeps the CSR product.
extern "C" int ddm_dia_build_and_apply_host(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, const double *x, double *y,
                                            int64_t max_blocks, int32_t *kinds_out, int64_t *counts_out)
{
  if (n < 0 || !rowptr || !x || !y || !counts_out || (rowptr[n] > 0 && (!col || !val))) return DDM_EINVAL;
  for (int64_t z = 0; z < rowptr[n]; ++z)
    if (col[z] < 0 || col[z] >= n) return DDM_EINVAL;
  DiaLayout L;
  dia_build(n, rowptr, col, val, L, dia_stage_x_from_env(), dia_code_from_env());
  dia_apply_host(L, n, rowptr, col, val, x, y);
  for (size_t b = 0; kinds_out && b < L.blk.size() && (int64_t)b < max_blocks; ++b)
    kinds_out[4 * b] = L.blk[b].r0, kinds_out[4 * b + 1] = L.blk[b].r1, kinds_out[4 * b + 2] = L.blk[b].nd, kinds_out[4 * b + 3] = L.stored[b];
  const int64_t counts[7] = {(int64_t)L.blk.size(), L.ndia, L.ncsr, L.rows_dia, L.slots_slab, L.nseg, L.nseg_half};
  std::copy(counts, counts + 7, counts_out);
  return DDM_OK;
}
// host-only entry for the CPU tests: the x windows of the same layout (DDM_SPMV_STAGE_X as above).  segs_out receives, for the first
// max_segments segments, (staged, runs, window doubles, place of the first run in runs_out); runs_out (first offset, doubles, window
// position) of the first max_runs runs, segment after segment; counts_out = {segments, runs of all segments, DIA_WIN: the doubles a
// staged segment's windows may take, WG}.
extern "C" int ddm_dia_windows_host(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int64_t max_segments, int32_t *segs_out,
                                    int64_t max_runs, int32_t *runs_out, int64_t *counts_out)
{
  if (n < 0 || !rowptr || !counts_out || (rowptr[n] > 0 && (!col || !val)) || (max_segments > 0 && !segs_out) || (max_runs > 0 && !runs_out)) return DDM_EINVAL;
  for (int64_t z = 0; z < rowptr[n]; ++z)
    if (col[z] < 0 || col[z] >= n) return DDM_EINVAL;
  DiaLayout L;
  dia_build(n, rowptr, col, val, L, dia_stage_x_from_env(), dia_code_from_env());
  int64_t nruns = 0;
  for (size_t s = 0; s < L.win.size(); ++s) {
    const DiaSegWindows &W = L.win[s];
    if ((int64_t)s < max_segments)
      segs_out[4 * s] = W.staged, segs_out[4 * s + 1] = (int32_t)W.runs.size(), segs_out[4 * s + 2] = W.window, segs_out[4 * s + 3] = (int32_t)nruns;
    for (const DiaRun &R : W.runs) {
      if (nruns < max_runs) runs_out[3 * nruns] = R.first, runs_out[3 * nruns + 1] = R.len, runs_out[3 * nruns + 2] = R.start;
      ++nruns;
    }
  }
  const int64_t counts[4] = {(int64_t)L.win.size(), nruns, DIA_WIN, WG};
  std::copy(counts, counts + 4, counts_out);
  return DDM_OK;
}
// host-only entry for the CPU tests: the dictionaries and code words of the same layout (DDM_SPMV_STAGE_X and DDM_SPMV_CODE as above),
// built on `threads` host workers (0: the library's own number).  blocks_out (may be null) receives, for the first max_blocks blocks,
// (number of the block's dictionary or -1: not coded, dictionary entries in use, 1 when the block's segment has value slabs);
// dict_out (may be null) the DIA_DICT doubles of every dictionary whose number is below max_blocks, one after the other; code_out
// (may be null) DIA_CODE_WORDS words per row, all 0 when no block is coded; counts_out = {blocks, coded blocks, value slots in the
// slabs that were built, entries of a dictionary, words of a row}.
extern "C" int ddm_dia_codes_host(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int threads, int64_t max_blocks,
                                  int32_t *blocks_out, double *dict_out, uint32_t *code_out, int64_t *counts_out)
{
  if (n < 0 || !rowptr || !counts_out || threads < 0 || (rowptr[n] > 0 && (!col || !val)) || (max_blocks > 0 && !blocks_out)) return DDM_EINVAL;
  for (int64_t z = 0; z < rowptr[n]; ++z)
    if (col[z] < 0 || col[z] >= n) return DDM_EINVAL;
  DiaLayout L;
  dia_build(n, rowptr, col, val, L, dia_stage_x_from_env(), dia_code_from_env(), threads ? (unsigned)threads : host_threads());
  for (size_t b = 0; b < L.blk.size() && (int64_t)b < max_blocks; ++b) {
    const DiaBlock &B = L.blk[b];
    blocks_out[3 * b] = B.dict, blocks_out[3 * b + 1] = L.ndict[b], blocks_out[3 * b + 2] = L.slabs[b];
    if (dict_out && B.dict >= 0 && B.dict < max_blocks) std::memcpy(dict_out + (size_t)B.dict * DIA_DICT, L.dict.data() + (size_t)B.dict * DIA_DICT, sizeof(double) * DIA_DICT);
  }
  if (code_out) {
    if (L.code.empty()) std::fill(code_out, code_out + (size_t)n * DIA_CODE_WORDS, 0u);
    else std::memcpy(code_out, L.code.data(), sizeof(uint32_t) * L.code.size());
  }
  const int64_t counts[5] = {(int64_t)L.blk.size(), L.ncoded, (int64_t)L.val.size(), DIA_DICT, DIA_CODE_WORDS};
  std::copy(counts, counts + 5, counts_out);
  return DDM_OK;
}
