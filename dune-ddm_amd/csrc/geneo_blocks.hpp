// Dense contractions on row-major block vectors, per subdomain (included by geneo.hpp; C ABI: ddm_blockvec_* in include/ddm_hip.h).
//
// GeneoWork cuts the rows of all subdomains into chunks and launches the kernels of geneo_kernels.hpp over them: Gram matrices
// U^T V (gram, gram2_sym: FP64 MFMA, split over the chunks and reduced per subdomain) and the basis update Out = U Y (rotate).
// The GenEO eigensolver (GeneoRun in geneo.hpp) holds one; the three ddm_blockvec_* exports at the end run one contraction each.
#pragma once
#include "geneo_kernels.hpp"

static constexpr int64_t GENEO_CHUNK_ROWS = 2048;

namespace {

struct GeneoWork {
  ddm_ctx *ctx = nullptr;
  int64_t n = 0;
  int nsub = 0, nchunk = 0;
  dbuf<GChunk> chunks;
  dbuf<int32_t> sub_chunk_ptr, sub_of_row;
  dbuf<double> partial;
  template <class T>
  int alloc(dbuf<T> &buf, size_t count)
  {
    if (buf.alloc((int64_t)count) != hipSuccess) return fail(ctx, DDM_EHIP, "GenEO: device allocation of %zu bytes failed", sizeof(T) * count);
    return DDM_OK;
  }
  // The chunk table: chunks of at most GENEO_CHUNK_ROWS rows, none across two subdomains, and `partial_per_chunk` doubles per chunk
  // for the partial sums of the Gram kernels.  rows_to_sub: also the subdomain of every row (the eigensolver's kernels read it).
  int setup(ddm_ctx *c, int64_t nsubdomains, const int64_t *sub_ptr, size_t partial_per_chunk, bool rows_to_sub = false)
  {
    ctx = c;
    nsub = (int)nsubdomains;
    n = sub_ptr[nsub];
    std::vector<GChunk> ch;
    std::vector<int32_t> scp((size_t)nsub + 1, 0), sor(rows_to_sub ? (size_t)n : 0);
    for (int64_t s = 0; s < nsub; ++s) {
      for (int64_t r = sub_ptr[s]; r < sub_ptr[s + 1]; r += GENEO_CHUNK_ROWS) ch.push_back(GChunk{r, std::min(r + GENEO_CHUNK_ROWS, sub_ptr[s + 1]), (int32_t)s, 0});
      scp[(size_t)s + 1] = (int32_t)ch.size();
      if (rows_to_sub) std::fill(sor.begin() + sub_ptr[s], sor.begin() + sub_ptr[s + 1], (int32_t)s);
    }
    nchunk = (int)ch.size();
    DDMCHECK(alloc(chunks, ch.size()));
    DDMCHECK(alloc(sub_chunk_ptr, scp.size()));
    if (rows_to_sub) DDMCHECK(alloc(sub_of_row, sor.size()));
    DDMCHECK(alloc(partial, (size_t)std::max(nchunk, 1) * partial_per_chunk));
    HIPCHECK(ctx, hipMemcpy(chunks, ch.data(), sizeof(GChunk) * ch.size(), hipMemcpyHostToDevice));
    HIPCHECK(ctx, hipMemcpy(sub_chunk_ptr, scp.data(), sizeof(int32_t) * scp.size(), hipMemcpyHostToDevice));
    if (rows_to_sub) HIPCHECK(ctx, hipMemcpy(sub_of_row, sor.data(), sizeof(int32_t) * sor.size(), hipMemcpyHostToDevice));
    return DDM_OK;
  }
  // G[sub] = U^T V per subdomain (pu x pv row-major, nsub matrices).  Blocks wider than the register tiles of the kernel (128 x 80)
  // are computed in column panels that land in their sub-block of the per-chunk partial matrices.
  int gram(const double *U, int64_t ldu, int pu, const double *V, int64_t ldv, int pv, double *G)
  {
    const int64_t pp = (int64_t)pu * pv;
    if (pu <= 32 && pv <= 32) {
      const bool same = U == V && ldu == ldv && pu == pv;
#define DDM_GRAM_SMALL(SAME, A1, B1) hipLaunchKernelGGL((k_gram_small<SAME, A1, B1>), dim3(nchunk), dim3(256), 0, ctx->stream, chunks, U, ldu, pu, V, ldv, pv, partial, pp, pv)
      if (same) {
        if (pu > 16) DDM_GRAM_SMALL(true, true, true);
        else DDM_GRAM_SMALL(true, false, false);
      } else if (pu > 16) {
        if (pv > 16) DDM_GRAM_SMALL(false, true, true);
        else DDM_GRAM_SMALL(false, true, false);
      } else {
        if (pv > 16) DDM_GRAM_SMALL(false, false, true);
        else DDM_GRAM_SMALL(false, false, false);
      }
#undef DDM_GRAM_SMALL
    } else if (pu <= 128 && pv <= 80)
      hipLaunchKernelGGL((k_gram_mfma<2, 5>), dim3(nchunk), dim3(256), 0, ctx->stream, chunks, U, ldu, pu, V, ldv, pv, partial, pp, pv, 0, 0);
    else if (pu <= 144 && pv <= 144)
      hipLaunchKernelGGL((k_gram_mfma<3, 9>), dim3(nchunk), dim3(256), 0, ctx->stream, chunks, U, ldu, pu, V, ldv, pv, partial, pp, pv, 0, 0);
    else
      for (int i0 = 0; i0 < pu; i0 += 128)
        for (int j0 = 0; j0 < pv; j0 += 80)
          hipLaunchKernelGGL((k_gram_mfma<2, 5>), dim3(nchunk), dim3(256), 0, ctx->stream, chunks, U + i0, ldu, std::min(128, pu - i0), V + j0, ldv, std::min(80, pv - j0),
                             partial, pp, pv, i0, j0);
    hipLaunchKernelGGL(k_gram_reduce, dim3((unsigned)((nsub * pp + 255) / 256)), dim3(256), 0, ctx->stream, nsub, sub_chunk_ptr, pp, partial, pp, G);
    HIPCHECK(ctx, hipGetLastError());
    return DDM_OK;
  }
  // G1[sub] = U^T V1, G2[sub] = U^T V2 (p x p each) for products that are symmetric by construction (V1 = A~ U, V2 = C~ U): one pass over
  // U, upper tiles only -- the entries BELOW the diagonal tiles of G1 / G2 are not defined, the caller mirrors the upper triangle
  // (gram2_mirror_host).  The partial buffer must hold 2 p p doubles per chunk.  p > 80: two general products.
  bool gram2_sym(const double *U, int64_t ldu, const double *V1, const double *V2, int64_t ldv, int p, double *G1, double *G2)
  {
    const int64_t pp = (int64_t)p * p;
    if (p > 80) {
      (void)gram(U, ldu, p, V1, ldv, p, G1);
      (void)gram(U, ldu, p, V2, ldv, p, G2);
      return false;
    }
    switch ((p + 15) >> 4) {
    case 1: hipLaunchKernelGGL(k_gram2_sym<1>, dim3(nchunk), dim3(256), 0, ctx->stream, chunks, U, ldu, V1, V2, ldv, p, partial); break;
    case 2: hipLaunchKernelGGL(k_gram2_sym<2>, dim3(nchunk), dim3(256), 0, ctx->stream, chunks, U, ldu, V1, V2, ldv, p, partial); break;
    case 3: hipLaunchKernelGGL(k_gram2_sym<3>, dim3(nchunk), dim3(256), 0, ctx->stream, chunks, U, ldu, V1, V2, ldv, p, partial); break;
    case 4: hipLaunchKernelGGL(k_gram2_sym<4>, dim3(nchunk), dim3(256), 0, ctx->stream, chunks, U, ldu, V1, V2, ldv, p, partial); break;
    default: hipLaunchKernelGGL(k_gram2_sym<5>, dim3(nchunk), dim3(256), 0, ctx->stream, chunks, U, ldu, V1, V2, ldv, p, partial); break;
    }
    hipLaunchKernelGGL(k_gram_reduce, dim3((unsigned)((nsub * pp + 255) / 256)), dim3(256), 0, ctx->stream, nsub, sub_chunk_ptr, pp, (const double *)partial, 2 * pp, G1);
    hipLaunchKernelGGL(k_gram_reduce, dim3((unsigned)((nsub * pp + 255) / 256)), dim3(256), 0, ctx->stream, nsub, sub_chunk_ptr, pp, (const double *)(partial + pp), 2 * pp, G2);
    return true;
  }
  static void gram2_mirror_host(int p, double *G)
  {
    for (int i = 1; i < p; ++i)
      for (int j = 0; j < i; ++j) G[(size_t)i * p + j] = G[(size_t)j * p + i];
  }
  // Out_k[:, 0:q) = (Base_k -) U_k[:, 0:pk) Y[sub]  for k < narr.  Y: nsub matrices pk x q, row-major.  More than 48 output columns
  // or more than 80 inner columns run as panels: 48 output columns per launch, the inner dimension in pieces of 72 whose products are
  // added onto the output.
  int rotate(int narr, const double *const *U, double *const *Out, const double *const *Base, int64_t ldu, int pk, const double *Y, int q, int64_t ldo, int64_t ldb,
             int gap_from = 1 << 30, int gap = 0)
  {
    const int KP = pk <= 80 ? pk : 72;
    for (int j0 = 0; j0 < q; j0 += 16 * ROT_TQ) {
      const int qq = std::min(16 * ROT_TQ, q - j0);
      for (int k0 = 0; k0 < pk; k0 += KP) {
        const int kk = std::min(KP, pk - k0);
        RotArgs a;
        for (int k = 0; k < 3; ++k) {
          a.U[k] = k < narr ? U[k] + k0 : nullptr;
          a.Out[k] = k < narr ? Out[k] : nullptr;
          a.Base[k] = (k < narr && Base) ? Base[k] : nullptr;
        }
        const int mode = k0 == 0 ? (Base ? 1 : 0) : (Base ? 2 : 3);
        const int p4 = (kk + 3) & ~3, q16 = ((qq + 15) >> 4) << 4;
        const size_t lds = sizeof(double) * ((size_t)p4 * q16 + 4 * 16 * (size_t)(p4 + 1));
#define DDM_ROTATE(PRE, TQ) hipLaunchKernelGGL((k_rotate_mfma<PRE, TQ>), dim3(nchunk, narr), dim3(256), lds, ctx->stream, chunks, a, ldu, kk, Y, qq, ldo, ldb, gap_from, gap, q, pk, k0, j0, mode)
        const int tq = q16 >> 4;
        if (16 * p4 <= 20 * 64) {
          if (tq == 1) DDM_ROTATE(20, 1);
          else if (tq == 2) DDM_ROTATE(20, 2);
          else DDM_ROTATE(20, 3);
        } else {
          if (tq == 1) DDM_ROTATE(0, 1);
          else if (tq == 2) DDM_ROTATE(0, 2);
          else DDM_ROTATE(0, 3);
        }
#undef DDM_ROTATE
      }
    }
    HIPCHECK(ctx, hipGetLastError());
    return DDM_OK;
  }
};

} // namespace

// ---- the dense block kernels on their own (parity tests against an FP64 host reference; also usable by callers that keep their
//      block vectors on the device) --------------------------------------------------------------------------------------------
extern "C" int ddm_blockvec_gram(ddm_ctx *ctx, int64_t nsub, const int64_t *sub_ptr, const double *U, int64_t ldu, int pu, const double *V, int64_t ldv,
                                 int pv, double *G_host)
{
  if (!ctx || !sub_ptr || !U || !V || !G_host || nsub < 1 || pu < 1 || pv < 1 || ldu < pu || ldv < pv) return fail(ctx, DDM_EINVAL, "ddm_blockvec_gram: bad arguments");
  GeneoWork W;
  DDMCHECK(W.setup(ctx, nsub, sub_ptr, (size_t)(pu * pv)));
  dbuf<double> G;
  DDMCHECK(W.alloc(G, (size_t)nsub * pu * pv));
  DDMCHECK(W.gram(U, ldu, pu, V, ldv, pv, G));
  return ddm_memcpy_d2h(ctx, G_host, G, (int64_t)sizeof(double) * nsub * pu * pv);
}
extern "C" int ddm_blockvec_gram2_sym(ddm_ctx *ctx, int64_t nsub, const int64_t *sub_ptr, const double *U, int64_t ldu, const double *V1, const double *V2, int64_t ldv, int p,
                                      double *G1_host, double *G2_host)
{
  if (!ctx || !sub_ptr || !U || !V1 || !V2 || !G1_host || !G2_host || nsub < 1 || p < 1 || ldu < p || ldv < p) return fail(ctx, DDM_EINVAL, "ddm_blockvec_gram2_sym: bad arguments");
  GeneoWork W;
  DDMCHECK(W.setup(ctx, nsub, sub_ptr, (size_t)(2 * p * p)));
  dbuf<double> G;
  DDMCHECK(W.alloc(G, (size_t)nsub * p * p * 2));
  const bool upper_only = W.gram2_sym(U, ldu, V1, V2, ldv, p, G, G + (size_t)nsub * p * p);
  HIPCHECK(ctx, hipGetLastError());
  DDMCHECK(ddm_memcpy_d2h(ctx, G1_host, G, (int64_t)sizeof(double) * nsub * p * p));
  DDMCHECK(ddm_memcpy_d2h(ctx, G2_host, G + (size_t)nsub * p * p, (int64_t)sizeof(double) * nsub * p * p));
  if (upper_only)
    for (int64_t s = 0; s < nsub; ++s) {
      GeneoWork::gram2_mirror_host(p, G1_host + (size_t)s * p * p);
      GeneoWork::gram2_mirror_host(p, G2_host + (size_t)s * p * p);
    }
  return DDM_OK;
}
extern "C" int ddm_blockvec_rotate(ddm_ctx *ctx, int64_t nsub, const int64_t *sub_ptr, const double *U, int64_t ldu, int p, const double *Y_host, int q,
                                   const double *Base, int64_t ldb, double *Out, int64_t ldo)
{
  if (!ctx || !sub_ptr || !U || !Y_host || !Out || nsub < 1 || p < 1 || q < 1 || ldu < p || ldo < q || (Base && ldb < q) || U == Out)
    return fail(ctx, DDM_EINVAL, "ddm_blockvec_rotate: bad arguments");
  GeneoWork W;
  DDMCHECK(W.setup(ctx, nsub, sub_ptr, 1));
  dbuf<double> Y;
  DDMCHECK(W.alloc(Y, (size_t)nsub * p * q));
  DDMCHECK(ddm_memcpy_h2d(ctx, Y, Y_host, (int64_t)sizeof(double) * nsub * p * q));
  const double *Ux[1] = {U};
  double *Ox[1] = {Out};
  const double *Bx[1] = {Base};
  DDMCHECK(W.rotate(1, Ux, Ox, Base ? Bx : nullptr, ldu, p, Y, q, ldo, ldb));
  return ddm_ctx_sync(ctx);
}
