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
