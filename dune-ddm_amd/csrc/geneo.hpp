// GenEO coarse-basis builder on the device (included by ddm_hip.hip after csr.hpp and the local solver, local_factor.hpp .. local_solver.hpp; pulls in geneo_blocks.hpp, the dense block contractions; C ABI: ddm_geneo_basis in include/ddm_hip.h).
//
// Reference: GenEOCoarseSpace::setup_geneo_impl (dune/ddm/coarsespaces/coarse_spaces.hh:319-331): C = D B_neu D
// (detail::scale_matrix_with_pou, :74-96), the lowest nev eigenpairs of A_neu x = lambda C x (solve_gevp ->
// spectra_gevp_op, dune/ddm/eigensolvers/spectra.hh:111-254: shift-invert implicitly restarted Lanczos, one vector at a
// time, on a sparse LU of A - sigma C), then v <- D v / ||D v||_2 (detail::finalize_eigenvectors, :52-61); the caller zeroes
// the Dirichlet entries (examples/poisson.cc:235-238).
//
// Here (SURVEY.md App. A.9 allows a block method whose span matches): LOBPCG on the reciprocal pencil
//     C~ x = mu A~ x,   A~ = A_neu + sigma C~   (largest mu;  lambda = 1 / mu - sigma,  identical eigenvectors),
// all subdomains of the rank in lock-step on their concatenated row-major blocks S = [X | W | P] (n x 3m, m = nev + extra):
//   * products with A~ and C~: row-major SpMM (k_spmm_rowmajor);
//   * preconditioner T ~ A~^-1 applied to all m columns at once by the multi-RHS triangular solves: the sparse Cholesky factor
//     of A~ when the symbolic analysis says it is affordable (ddm_chol_create: T is then exact and the iteration is block
//     inverse iteration with Rayleigh-Ritz acceleration -- the device analogue of the reference's shift-invert), else ILU(0);
//   * Gram matrices S^T (A~ S), S^T (C~ S) and all inner products by the FP64-MFMA split-K kernel k_gram_mfma; the basis update
//     [X P] <- S Y by k_rotate_mfma (S, A~S, C~S rotated in one launch);
//   * only the p x p (p = 3m) projected eigenproblems run on the host (dense_host.hpp, one thread per subdomain), in the
//     rank-revealing form of the robust LOBPCG (basis truncation instead of Cholesky factorisations that break down).
// C~ is C without the rows / columns of global Dirichlet DoFs: after the symmetric elimination (examples/pdelab_helper.hh:33-46)
// those are decoupled unit modes that zero_at_dirichlet turns into zero vectors (a singular R A R^T in the reference).
//
// Convergence test per wanted pair, for all subdomains: with the exact T the relative residual of the inverted operator in the
// A~-norm, sqrt(r^T A~^-1 r) / mu  (r = C~ x - mu A~ x, x^T A~ x = 1) -- the quantity Spectra bounds by tol for its B-norm
// Lanczos residual (HermEigsBase.h:158-175); with ILU(0) the Euclidean relative residual ||r|| / (mu ||A~ x||).
//
// In this file: GeneoProblem (what an entry point asks for), GeneoSetup (pencil and preconditioner: what outlives a run), GeneoRun (the
// state of one run at a fixed block width, one method per phase), the entry points ddm_geneo_basis / ddm_msgfem_basis / ddm_svd_basis,
// and before them the harmonic extension the last two iterate with.  geneo_solver.hpp, included below GeneoRun, has geneo_run (the loop
// above, phase by phase), the kept object ddm_geneo with its value refresh and warm start, and the threshold mode around the runs.
#pragma once
#include <functional>

#include "dense_host.hpp"
#include "geneo_blocks.hpp"

// Owners of the C-ABI objects this file creates for itself: a unique_ptr whose deleter is the object's destroy function.
// out_ptr(owner) stands in for the `T **out` of a create call: the owner takes what the call stored.
template <auto Destroy>
struct Destroyer {
  template <class T>
  void operator()(T *p) const { Destroy(p); }
};
using csr_ptr = std::unique_ptr<ddm_csr, Destroyer<ddm_csr_destroy>>;
using ilu0_ptr = std::unique_ptr<ddm_ilu0, Destroyer<ddm_ilu0_destroy>>;
template <class Owner>
struct OutPtr {
  Owner &owner;
  typename Owner::pointer raw = nullptr;
  ~OutPtr() { owner.reset(raw); }
  operator typename Owner::pointer *() { return &raw; }
};
template <class Owner>
OutPtr<Owner> out_ptr(Owner &owner)
{
  return OutPtr<Owner>{owner};
}

extern "C" int ddm_geneo_params_default(ddm_geneo_params *p)
{
  if (!p) return DDM_EINVAL;
  p->nev = 16;            // eigensolver_params.hh:11
  p->nev_max = 32;        // 2 nev (:24)
  p->tolerance = 1e-5;    // :14
  p->shift = 1e-3;        // :15
  p->threshold = -0.5;    // :16
  p->maxit = 400;
  p->extra = 4;
  p->seed = 0;
  p->preconditioner = 0;
  // The exact preconditioner (sparse Cholesky of the pencil) is decided PER RANK by time and memory, not by a fixed size: a time budget
  // (DDM_GENEO_DIRECT_SECONDS, default 6 s: what the ILU(0)-preconditioned iteration costs at the headline size) times the measured
  // rate of the device factorisation (1.1e13 multiply-adds / s, sn_chol.hpp) gives this bound on the multiply-adds -- 8 x 111^3 blocks
  // on one GPU (2.1e14, 154 GB) stay with ILU(0), ONE 111^3 block per GPU (2.6e13, 19 GB: the 8-GPU layout) gets the exact factor
  // in ~2.4 s and ~20 block iterations -- and the panels must fit into 85 % of the free device memory (sn_direct_create).
  {
    double seconds = 6.0;
    if (const char *e = std::getenv("DDM_GENEO_DIRECT_SECONDS")) seconds = std::atof(e);
    p->max_direct_flops = seconds * 1.1e13;
  }
  p->verbose = 0;
  p->raw = 0;
  return DDM_OK;
}

namespace {

__global__ void k_geneo_random(int64_t n, int m, int64_t ld, unsigned long long seed, const double *__restrict__ mask, double *__restrict__ X)
{
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n * m) return;
  const int64_t i = t / m;
  const int j = (int)(t - i * m);
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(t + 1); // splitmix64 of the entry index
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  X[i * ld + j] = ((double)(z >> 11) * (1.0 / 9007199254740992.0) - 0.5) * mask[i];
}

// The launches of the column-wise helper kernels (geneo_kernels.hpp and k_geneo_random above), one function per kernel: GeneoRun and the
// test exports at the end of this file (ddm_geneo_debug_helper) go through these, so that both run the same grids.
static unsigned geneo_grid(int64_t threads) { return (unsigned)((threads + 255) / 256); }
static void launch_geneo_random(ddm_ctx *ctx, int64_t n, int m, int64_t ld, unsigned long long seed, const double *mask, double *X)
{
  hipLaunchKernelGGL(k_geneo_random, dim3(geneo_grid(n * (int64_t)m)), dim3(256), 0, ctx->stream, n, m, ld, seed, mask, X);
}
static void launch_geneo_residual(ddm_ctx *ctx, int64_t n, int m, const int32_t *sub_of_row, const double *mu, const double *AX, int64_t lda, const double *CX, int64_t ldc,
                                  double *R, int64_t ldr)
{
  hipLaunchKernelGGL(k_geneo_residual, dim3(geneo_grid(n * (int64_t)m)), dim3(256), 0, ctx->stream, n, m, sub_of_row, mu, AX, lda, CX, ldc, R, ldr);
}
static void launch_geneo_copy_cols(ddm_ctx *ctx, int64_t n, int m, const double *src, int64_t lds, double *dst, int64_t ldd)
{
  hipLaunchKernelGGL(k_geneo_copy_cols, dim3(geneo_grid(n * (int64_t)m)), dim3(256), 0, ctx->stream, n, m, src, lds, dst, ldd);
}
static void launch_geneo_rowscale(ddm_ctx *ctx, int64_t n, int m, const double *w, double *X, int64_t ldx)
{
  hipLaunchKernelGGL(k_geneo_rowscale, dim3(geneo_grid(n * (int64_t)m)), dim3(256), 0, ctx->stream, n, m, w, X, ldx);
}
static void launch_geneo_invsqrt_diag(ddm_ctx *ctx, int64_t nsub, int m, const double *G, double *s)
{
  hipLaunchKernelGGL(k_geneo_invsqrt_diag, dim3(geneo_grid(nsub * m)), dim3(256), 0, ctx->stream, (int)nsub, m, G, s);
}
static void launch_geneo_finalize(ddm_ctx *ctx, int64_t n, int nev, const int32_t *sub_of_row, const double *scale, int mscale, const double *V, int64_t ldv, double *basis)
{
  hipLaunchKernelGGL(k_geneo_finalize, dim3(geneo_grid(n)), dim3(256), 0, ctx->stream, n, nev, sub_of_row, scale, mscale, V, ldv, basis);
}

// widest block the eigensolver iterates (nev + extra): the dense kernels work in column panels beyond 48 (round 3; the threshold mode
// of the reference doubles nev up to nev_max, spectra.hh:157-163), the limit is the memory of the six n x 3m blocks
constexpr int GENEO_MAX_BLOCK = 132;

// A~ = A + sigma C~ and C~ = D B D without Dirichlet rows / columns, on the union pattern, as host CSR.  origin (optional): per pencil
// entry where it comes from, as geneo_pencil_refresh_host and k_geneo_pencil_refresh read it -- low 16 bits: 1 + the entry's offset
// inside A's row, high 16 bits: 1 + the offset inside B's row, 0 = absent there.  Returns false when a row of A or B has more
// entries than 16 bits address (origin is then not filled).
struct PencilInput {
  int64_t n;
  const int64_t *a_rp;
  const int32_t *a_ci;
  const double *a_va;
  const int64_t *b_rp;
  const int32_t *b_ci;
  const double *b_va;
};
constexpr int64_t GENEO_ORIGIN_MAX_ROW = 65535;
// (WITH_ORIGIN = false compiles the loops of the one-call entry points without the map's bookkeeping)
template <bool WITH_ORIGIN>
static bool build_pencil_host_impl(const PencilInput &M, const double *pou, const uint8_t *dir, double sigma, hvec<int64_t> &rpT, hvec<int32_t> &ciT, hvec<double> &vaT,
                                   hvec<double> &vaC, hvec<uint32_t> *origin)
{
  const int64_t n = M.n;
  rpT.resize((size_t)n + 1);
  rpT[0] = 0;
  const unsigned hw = host_threads();
  const int nth = (int)std::min<int64_t>(hw, std::max<int64_t>(1, n / 65536));
  std::vector<std::thread> th;
  std::atomic<bool> origin_fits{true};
  // pass 1: sizes of the merged rows (threads), then the prefix sum
  for (int t = 0; t < nth; ++t)
    th.emplace_back([&, t]() {
      for (int64_t i = n * t / nth; i < n * (t + 1) / nth; ++i) {
        int64_t a = M.a_rp[i], b = M.b_rp[i], cnt = 0;
        const int64_t a1 = M.a_rp[i + 1], b1 = M.b_rp[i + 1];
        if (WITH_ORIGIN && (a1 - a > GENEO_ORIGIN_MAX_ROW || b1 - b > GENEO_ORIGIN_MAX_ROW)) origin_fits = false;
        while (a < a1 || b < b1) {
          const int32_t ca = a < a1 ? M.a_ci[a] : INT32_MAX, cb = b < b1 ? M.b_ci[b] : INT32_MAX;
          a += ca <= cb;
          b += cb <= ca;
          ++cnt;
        }
        rpT[i + 1] = cnt;
      }
    });
  for (auto &t : th) t.join();
  th.clear();
  for (int64_t i = 0; i < n; ++i) rpT[i + 1] += rpT[i];
  ciT.resize((size_t)rpT[n]);
  vaT.resize((size_t)rpT[n]);
  vaC.resize((size_t)rpT[n]);
  uint32_t *const org = WITH_ORIGIN && origin_fits ? (origin->resize((size_t)rpT[n]), origin->data()) : nullptr;
  for (int t = 0; t < nth; ++t)
    th.emplace_back([&, t]() {
      for (int64_t i = n * t / nth; i < n * (t + 1) / nth; ++i) {
        const int64_t a0 = M.a_rp[i], b0 = M.b_rp[i];
        int64_t a = a0, b = b0, q = rpT[i];
        const int64_t a1 = M.a_rp[i + 1], b1 = M.b_rp[i + 1];
        const bool di = dir && dir[i];
        while (a < a1 || b < b1) {
          const int32_t ca = a < a1 ? M.a_ci[a] : INT32_MAX, cb = b < b1 ? M.b_ci[b] : INT32_MAX;
          const int32_t c = std::min(ca, cb);
          double va = 0.0, vc = 0.0;
          uint32_t o = 0;
          if (ca == c) {
            if (WITH_ORIGIN) o |= (uint32_t)(a - a0 + 1);
            va = M.a_va[a++];
          }
          if (cb == c) {
            if (WITH_ORIGIN) o |= (uint32_t)(b - b0 + 1) << 16;
            vc = (di || (dir && dir[c])) ? 0.0 : M.b_va[b] * pou[i] * pou[c]; // scale_matrix_with_pou (coarse_spaces.hh:74-96)
            ++b;
          }
          ciT[(size_t)q] = c;
          vaC[(size_t)q] = vc;
          vaT[(size_t)q] = va + sigma * vc;
          if (WITH_ORIGIN && org) org[(size_t)q] = o;
          ++q;
        }
      }
    });
  for (auto &t : th) t.join();
  return origin_fits;
}
static bool build_pencil_host(const PencilInput &M, const double *pou, const uint8_t *dir, double sigma, hvec<int64_t> &rpT, hvec<int32_t> &ciT, hvec<double> &vaT,
                              hvec<double> &vaC, hvec<uint32_t> *origin = nullptr)
{
  return origin ? build_pencil_host_impl<true>(M, pou, dir, sigma, rpT, ciT, vaT, vaC, origin) : build_pencil_host_impl<false>(M, pou, dir, sigma, rpT, ciT, vaT, vaC, nullptr);
}
static PencilInput pencil_input(const ddm_csr *A, const ddm_csr *B)
{
  return PencilInput{A->nrows, A->h_rp.data(), A->h_ci.data(), A->h_va.data(), B->h_rp.data(), B->h_ci.data(), B->h_va.data()};
}
// New values of A and / or B through the origin map, in place: the formula and the operation order of build_pencil_host entry by
// entry.  The device twin is k_geneo_pencil_refresh.
static void geneo_pencil_refresh_host(int64_t n, const int64_t *rpT, const int32_t *ciT, const uint32_t *origin, const int64_t *a_rp, const double *a_va, const int64_t *b_rp,
                                      const double *b_va, const double *pou, const uint8_t *dir, double sigma, double *vaT, double *vaC)
{
  for (int64_t i = 0; i < n; ++i) {
    const bool di = dir && dir[i];
    for (int64_t q = rpT[i]; q < rpT[i + 1]; ++q) {
      const uint32_t oa = origin[q] & 0xffffu, ob = origin[q] >> 16;
      const int32_t c = ciT[q];
      double va = 0.0, vc = 0.0;
      if (oa) va = a_va[a_rp[i] + oa - 1];
      if (ob) vc = (di || (dir && dir[c])) ? 0.0 : b_va[b_rp[i] + ob - 1] * pou[i] * pou[c];
      vaC[q] = vc;
      vaT[q] = va + sigma * vc;
    }
  }
}
// One wave per row, the lanes over the row's pencil entries (in rounds of 64).  mask: 0.0 on Dirichlet rows, 1.0 elsewhere.  The two
// patterns need not be equal and neither needs the diagonal: absent entries (origin half 0) contribute 0.
constexpr int PENCIL_WAVES = 4;
__global__ __launch_bounds__(64 * PENCIL_WAVES) void k_geneo_pencil_refresh(int64_t n, const int64_t *__restrict__ rpT, const int32_t *__restrict__ ciT,
                                                                             const uint32_t *__restrict__ origin, const int64_t *__restrict__ a_rp,
                                                                             const double *__restrict__ a_va, const int64_t *__restrict__ b_rp,
                                                                             const double *__restrict__ b_va, const double *__restrict__ pou,
                                                                             const double *__restrict__ mask, double sigma, double *__restrict__ vaT,
                                                                             double *__restrict__ vaC)
{
  const int64_t i = blockIdx.x * (int64_t)PENCIL_WAVES + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const int64_t q1 = rpT[i + 1], a0 = a_rp[i], b0 = b_rp[i];
  const double pi = pou[i];
  const bool di = mask[i] == 0.0;
  for (int64_t q = rpT[i] + lane; q < q1; q += 64) {
    const uint32_t o = origin[q], oa = o & 0xffffu, ob = o >> 16;
    const int32_t c = ciT[q];
    double va = 0.0, vc = 0.0;
    if (oa) va = a_va[a0 + oa - 1];
    if (ob) vc = (di || mask[c] == 0.0) ? 0.0 : b_va[b0 + ob - 1] * pi * pou[c];
    vaC[q] = vc;
    vaT[q] = va + sigma * vc;
  }
}
// The start block of a warm run at the eigensolver's strides: S is n x 3m (ld = 3m).  Columns [0, mk) of the X slot come from the kept
// block (n x ldk, its first mk columns), columns [mk, m) from the generator of k_geneo_random at the same entry index i m + j, the W and
// P slots [m, 3m) are zero; Dirichlet rows (mask 0) are zero.
__global__ void k_geneo_start_block(int64_t n, int m, int mk, int64_t ldk, unsigned long long seed, const double *__restrict__ mask, const double *__restrict__ kept,
                                    double *__restrict__ S)
{
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int p = 3 * m;
  if (t >= n * p) return;
  const int64_t i = t / p;
  const int j = (int)(t - i * p);
  double v = 0.0;
  if (j < mk) v = mask[i] == 0.0 ? 0.0 : kept[i * ldk + j];
  else if (j < m) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i * m + j + 1); // splitmix64 of the entry index, as k_geneo_random
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    v = ((double)(z >> 11) * (1.0 / 9007199254740992.0) - 0.5) * mask[i];
  }
  S[t] = v;
}
static void launch_geneo_start_block(ddm_ctx *ctx, int64_t n, int m, int mk, int64_t ldk, unsigned long long seed, const double *mask, const double *kept, double *S)
{
  hipLaunchKernelGGL(k_geneo_start_block, dim3(geneo_grid(n * 3 * (int64_t)m)), dim3(256), 0, ctx->stream, n, m, mk, ldk, seed, mask, kept, S);
}

// X = (keep ? X : 0) - Y  (rows: keep = 0 / 1): tail of the harmonic projection / extension.  Rows with keep = 0 are OUTPUTS: what
// they held does not enter (a product 0 * X would carry a NaN or Inf left there into the result).
__global__ void k_geneo_project(int64_t n, int m, const double *__restrict__ keep, const double *__restrict__ Y, int64_t ldy, double *__restrict__ X, int64_t ldx)
{
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n * m) return;
  const int64_t i = t / m;
  const int j = (int)(t - i * m);
  X[i * ldx + j] = (keep[i] != 0.0 ? X[i * ldx + j] : 0.0) - Y[i * ldy + j];
}
// Y = w .* X
__global__ void k_geneo_rowscale_to(int64_t n, int m, const double *__restrict__ w, const double *__restrict__ X, int64_t ldx, double *__restrict__ Y, int64_t ldy)
{
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n * m) return;
  const int64_t i = t / m;
  const int j = (int)(t - i * m);
  Y[i * ldy + j] = w[i] * X[i * ldx + j];
}

static bool csr_values_symmetric(const ddm_csr *A)
{
  const int64_t n = A->nrows;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = A->h_rp[i]; k < A->h_rp[i + 1]; ++k) {
      const int64_t j = A->h_ci[k];
      if (j <= i) continue;
      const auto b = A->h_ci.begin() + A->h_rp[j], e = A->h_ci.begin() + A->h_rp[j + 1];
      const auto it = std::lower_bound(b, e, (int32_t)i);
      const double vt = (it != e && *it == i) ? A->h_va[(size_t)(it - A->h_ci.begin())] : 0.0;
      if (std::fabs(vt - A->h_va[k]) > 1e-12 * (std::fabs(vt) + std::fabs(A->h_va[k]))) return false;
    }
  return true;
}

} // namespace

// Energy-minimal (a-harmonic) extension u_i = -A_ii^-1 A_ib u_b (EnergyMinimalExtension, energy_minimal_extension.hh:36-229) for
// row-major device blocks: the interior block is factorised once by the sparse direct solver, as part of the n x n matrix
//     A^ = [A_ii 0; 0 I]   (rows / columns outside the interior replaced by the identity),
// so that every operand is a full-length block and no index gathers are needed:  X <- keep .* X - A^^-1 (G_ib X)  with G_ib the
// interior rows x boundary columns of A.  The same object projects onto the a-harmonic subspace in the constrained eigensolver
// (MsGFEMCoarseSpace): P X = keep_b .* X - A^^-1 G_ib X,  P^T R = keep_b .* R - G_bi A^^-T (interior .* R).
struct ddm_harmonic {
  int64_t n = 0;
  csr_ptr Gib, Gbi;
  ilu0_ptr F;
  dbuf<double> keep;   // 1 outside the interior (rows the extension leaves alone)
  dbuf<double> keep_b; // 1 on boundary rows only (projection: rows that are neither interior nor boundary are zeroed)
  dbuf<double> isint;  // 1 on interior rows
  dbuf<double> t1, t2; // work blocks (n x tcols)
  int tcols = 0;
  bool symmetric = true;
};
extern "C" void ddm_harmonic_destroy(ddm_harmonic *H) { delete H; }
using harmonic_ptr = std::unique_ptr<ddm_harmonic, Destroyer<ddm_harmonic_destroy>>;
// cls[i]: 0 = interior, 1 = boundary, anything else = neither (its values count as zero in the right-hand side, :109-118)
static int harmonic_create_impl(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, const uint8_t *cls, bool want_transpose, ddm_harmonic **out)
{
  const int64_t n = A->nrows;
  std::vector<int64_t> rpI((size_t)n + 1, 0), rpG((size_t)n + 1, 0), rpT((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    int64_t ci = 0, cg = 0;
    if (cls[i] == 0) {
      for (int64_t k = A->h_rp[i]; k < A->h_rp[i + 1]; ++k) {
        const uint8_t c = cls[A->h_ci[k]];
        ci += c == 0;
        cg += c == 1;
        if (c == 1) rpT[(size_t)A->h_ci[k] + 1] += 1;
      }
      if (ci == 0) return fail(ctx, DDM_ENUMERIC, "harmonic extension: interior row %lld has no interior entries", (long long)i);
    } else ci = 1;
    rpI[(size_t)i + 1] = rpI[(size_t)i] + ci;
    rpG[(size_t)i + 1] = rpG[(size_t)i] + cg;
  }
  for (int64_t i = 0; i < n; ++i) rpT[(size_t)i + 1] += rpT[(size_t)i];
  std::vector<int32_t> ciI((size_t)rpI[n]), ciG((size_t)rpG[n]), ciT((size_t)rpT[n]);
  std::vector<double> vaI((size_t)rpI[n]), vaG((size_t)rpG[n]), vaT((size_t)rpT[n]);
  std::vector<int64_t> fill(rpT.begin(), rpT.end() - 1);
  for (int64_t i = 0; i < n; ++i) {
    int64_t qi = rpI[(size_t)i], qg = rpG[(size_t)i];
    if (cls[i] != 0) {
      ciI[(size_t)qi] = (int32_t)i;
      vaI[(size_t)qi] = 1.0;
      continue;
    }
    for (int64_t k = A->h_rp[i]; k < A->h_rp[i + 1]; ++k) {
      const int32_t j = A->h_ci[k];
      if (cls[j] == 0) {
        ciI[(size_t)qi] = j;
        vaI[(size_t)qi++] = A->h_va[k];
      } else if (cls[j] == 1) {
        ciG[(size_t)qg] = j;
        vaG[(size_t)qg++] = A->h_va[k];
        const int64_t q = fill[(size_t)j]++; // rows i ascending => sorted columns in the transpose
        ciT[(size_t)q] = (int32_t)i;
        vaT[(size_t)q] = A->h_va[k];
      }
    }
  }
  harmonic_ptr H(new ddm_harmonic);
  H->n = n;
  csr_ptr Ahat;
  int rc = ddm_csr_create(ctx, n, n, rpI.data(), ciI.data(), vaI.data(), out_ptr(Ahat));
  if (!rc) {
    H->symmetric = csr_values_symmetric(Ahat.get());
    rc = direct_create_impl(ctx, Ahat.get(), nblocks, block_ptr, H->symmetric ? 0 : 1, 0.0, /*setup_use=*/true, out_ptr(H->F));
  }
  Ahat.reset();
  if (!rc) rc = ddm_csr_create(ctx, n, n, rpG.data(), ciG.data(), vaG.data(), out_ptr(H->Gib));
  if (!rc && want_transpose) rc = ddm_csr_create(ctx, n, n, rpT.data(), ciT.data(), vaT.data(), out_ptr(H->Gbi));
  if (!rc) {
    std::vector<double> k0((size_t)n), k1((size_t)n), k2((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      k0[(size_t)i] = cls[i] == 0 ? 0.0 : 1.0;
      k1[(size_t)i] = cls[i] == 1 ? 1.0 : 0.0;
      k2[(size_t)i] = cls[i] == 0 ? 1.0 : 0.0;
    }
    rc = upload(ctx, k0.data(), n, H->keep);
    if (!rc) rc = upload(ctx, k1.data(), n, H->keep_b);
    if (!rc) rc = upload(ctx, k2.data(), n, H->isint);
  }
  if (rc) return rc;
  *out = H.release();
  return DDM_OK;
}
// X <- keep .* X - A^^-1 G_ib X  (keep = rows outside the interior, or boundary rows only)
static int harmonic_apply(ddm_ctx *ctx, ddm_harmonic *H, int m, double *X, int64_t ldx, bool boundary_only)
{
  HIPCHECK(ctx, reserve_cols<double>(H->tcols, m, {{H->t1, H->n}, {H->t2, H->n}}));
  DDMCHECK(csr_mm_ld(ctx, H->Gib.get(), m, X, ldx, H->t1, m));
  DDMCHECK(ilu0_solve_multi_ld(ctx, H->F.get(), m, H->t1, m, H->t2, m));
  hipLaunchKernelGGL(k_geneo_project, dim3((unsigned)((H->n * (int64_t)m + 255) / 256)), dim3(256), 0, ctx->stream, H->n, m, boundary_only ? H->keep_b : H->keep,
                     (const double *)H->t2, (int64_t)m, X, ldx);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
// R <- keep_b .* R - G_bi A^^-1 (interior .* R)   (transpose of the projection; symmetric A only)
static int harmonic_apply_transposed(ddm_ctx *ctx, ddm_harmonic *H, int m, double *R, int64_t ldr)
{
  HIPCHECK(ctx, reserve_cols<double>(H->tcols, m, {{H->t1, H->n}, {H->t2, H->n}}));
  const unsigned g = (unsigned)((H->n * (int64_t)m + 255) / 256);
  hipLaunchKernelGGL(k_geneo_rowscale_to, dim3(g), dim3(256), 0, ctx->stream, H->n, m, H->isint, (const double *)R, ldr, H->t1, (int64_t)m);
  DDMCHECK(ilu0_solve_multi_ld(ctx, H->F.get(), m, H->t1, m, H->t2, m));
  DDMCHECK(csr_mm_ld(ctx, H->Gbi.get(), m, H->t2, m, H->t1, m));
  hipLaunchKernelGGL(k_geneo_project, dim3(g), dim3(256), 0, ctx->stream, H->n, m, H->keep_b, (const double *)H->t1, (int64_t)m, R, ldr);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_harmonic_create(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, int64_t n_interior, const int64_t *interior_host,
                                   int64_t n_boundary, const int64_t *boundary_host, ddm_harmonic **out)
{
  if (!ctx || !A || !out || nblocks < 1 || !block_ptr || n_interior < 0 || n_boundary < 0 || (n_interior && !interior_host) || (n_boundary && !boundary_host))
    return fail(ctx, DDM_EINVAL, "ddm_harmonic_create: bad arguments");
  if (A->nrows != A->ncols) return fail(ctx, DDM_EINVAL, "ddm_harmonic_create: square matrix expected");
  const int64_t n = A->nrows;
  std::vector<uint8_t> cls((size_t)n, 2);
  for (int64_t k = 0; k < n_boundary; ++k) {
    if (boundary_host[k] < 0 || boundary_host[k] >= n) return fail(ctx, DDM_EINVAL, "ddm_harmonic_create: boundary index out of range");
    cls[(size_t)boundary_host[k]] = 1; // listed twice is fine (coarse_spaces.hh:582-589 produces duplicates)
  }
  for (int64_t k = 0; k < n_interior; ++k) {
    if (interior_host[k] < 0 || interior_host[k] >= n) return fail(ctx, DDM_EINVAL, "ddm_harmonic_create: interior index out of range");
    if (cls[(size_t)interior_host[k]] == 1) return fail(ctx, DDM_EINVAL, "ddm_harmonic_create: index %lld is both interior and boundary", (long long)interior_host[k]);
    cls[(size_t)interior_host[k]] = 0;
  }
  return harmonic_create_impl(ctx, A, nblocks, block_ptr, cls.data(), false, out);
}
extern "C" int ddm_harmonic_extend(ddm_ctx *ctx, ddm_harmonic *H, int nrhs, double *X, int64_t ldx)
{
  if (!ctx || !H || !X || nrhs < 1 || ldx < nrhs) return fail(ctx, DDM_EINVAL, "ddm_harmonic_extend: bad arguments");
  for (int c0 = 0; c0 < nrhs; c0 += 48) DDMCHECK(harmonic_apply(ctx, H, std::min(48, nrhs - c0), X + c0, ldx, false));
  return DDM_OK;
}

// Y = Op X on row-major blocks: (columns, X, ldx, Y, ldy)
using BlockOp = std::function<int(int, const double *, int64_t, double *, int64_t)>;

// What the eigensolver is asked for: ddm_geneo_basis, ddm_msgfem_basis and ddm_svd_basis fill it.
struct GeneoProblem {
  const char *who = "";                     // the entry point, for its messages
  const ddm_csr *A = nullptr, *B = nullptr; // A x = lambda (D B D) x; only the host arrays are read
  int64_t nsub = 0;
  const int64_t *sub_ptr = nullptr;
  const double *pou = nullptr;         // D of the finalisation v <- D v, and of the pencil unless pou_pencil is given
  const uint8_t *dirichlet = nullptr;  // optional: rows / columns taken out of C~, zeroed in the basis
  ddm_harmonic *con = nullptr;         // optional: iterate in the a-harmonic subspace
  const double *pou_pencil = nullptr;  // optional: D of the pencil
  const BlockOp *op_C = nullptr;       // optional: replaces the product with C~
};

static double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// Helper thread that an early error return cannot leave running
struct GeneoHelper {
  std::thread t;
  void join()
  {
    if (t.joinable()) t.join();
  }
  ~GeneoHelper() { join(); }
};

// What outlives a run of the block eigensolver: the pencil, the chosen preconditioner, the Dirichlet mask and the POU on the device.
// Built once per problem (geneo_setup_create); every block width of the threshold mode and every later compute of a kept ddm_geneo
// iterate on it.  refresh_pencil_and_preconditioner (geneo_solver.hpp) gives it new values in place.
struct GeneoSetup {
  ddm_ctx *const ctx;
  const GeneoProblem Q;          // (a copy: the pointers in it are borrowed)
  const ddm_geneo_params *const P; // borrowed: read again by every compute
  const int64_t n, nsub;
  const double sigma;            // the shift the pencil was assembled with
  std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
  double t_pencil = 0.0, t_upload = 0.0, t_direct = 0.0, t_prec = 0.0, t_setup = 0.0; // ends of the setup intervals, seconds after t_begin
  // a value refresh that builds the preconditioner anew: its intervals count from here, the pencil was not assembled again
  void restart_clock()
  {
    t_begin = std::chrono::steady_clock::now();
    t_pencil = t_upload = 0.0;
  }
  // ORDER OF THE MEMBERS BELOW = reverse order of destruction, on every return path.  The two helper threads are declared last, so
  // they are joined first: the probe reads Q.A and writes probe_flops, the ILU(0) build reads At's host arrays and writes T_ilu,
  // rc_ilu and err_ilu.  Then the preconditioner(s) go, then At, whose deleter (ddm_csr_destroy) joins the upload thread that fills
  // the device arrays of At AND of C -- which is why C is declared before At and outlives it.
  dbuf<double> maskd, poud; // Dirichlet mask (0 on Dirichlet rows, else 1), POU of the finalisation
  csr_ptr C, At;      // the pencil: C~ (values only, on At's pattern) and A~ = A + sigma C~
  ilu0_ptr T, T_ilu;  // the chosen preconditioner; the speculative ILU(0) until the choice is made
  double probe_flops = 0.0;
  int rc_ilu = DDM_OK;
  std::string err_ilu;
  int direct = 0; // T is the sparse direct factor of A~
  bool prec_f32 = false;
  int refresh_period = 0, orth_passes = 0;
  GeneoHelper probe_thread, ilu_thread;

  GeneoSetup(ddm_ctx *c, const GeneoProblem &q, const ddm_geneo_params *par) : ctx(c), Q(q), P(par), n(q.A->nrows), nsub(q.nsub), sigma(par->shift) {}

  // ---- pencil ----
  void assemble_pencil(hvec<uint32_t> *origin, bool *origin_fits)
  {
    // "auto": whether the sparse direct factor of A~ is affordable at all is estimated on a helper thread from the first separator of the
    // largest block of A's pattern (the pencil's pattern, or a superset of B's), while the pencil is being assembled
    if (P->preconditioner == 0 && P->max_direct_flops > 0.0 && nsub > 1 && !std::getenv("DDM_DIRECT_ENGINE"))
      probe_thread.t = std::thread([this]() { probe_flops = sn_probe_largest_block(Q.A->h_rp.data(), Q.A->h_ci.data(), nsub, Q.sub_ptr, false); });
    hvec<int64_t> rpT;
    hvec<int32_t> ciT;
    hvec<double> vaT, vaC;
    const bool fits = build_pencil_host(pencil_input(Q.A, Q.B), Q.pou_pencil ? Q.pou_pencil : Q.pou, Q.dirichlet, sigma, rpT, ciT, vaT, vaC, origin);
    if (origin_fits) *origin_fits = fits;
    t_pencil = seconds_since(t_begin);
    // the host arrays move into At; its device copy and the values of C~ (same pattern, device only) are uploaded by a helper thread
    // while this one factorises / analyses on the host
    At.reset(csr_adopt(ctx, n, std::move(rpT), std::move(ciT), std::move(vaT), std::move(vaC), out_ptr(C), nsub, Q.sub_ptr));
    t_upload = seconds_since(t_begin);
  }

  // ---- preconditioner ----
  // "auto": the ILU(0) factorisation starts on a helper thread while this one orders and analyses for the sparse direct factor
  // (at the headline size the analysis ends in "too expensive" after 0.9 s and the ILU(0) setup takes 2.3 s); whichever is not
  // needed is dropped.  Called again by a value refresh whose factor cannot be refreshed in place: T and T_ilu are empty then.
  int choose_preconditioner()
  {
    direct = 0;
    rc_ilu = DDM_OK;
    err_ilu.clear();
    if (P->preconditioner != 2)
      ilu_thread.t = std::thread([this]() {
        (void)hipSetDevice(ctx->device);
        rc_ilu = ilu0_create_impl(ctx, At.get(), nsub, Q.sub_ptr, /*multi_rhs_only=*/true, out_ptr(T_ilu));
        if (rc_ilu) err_ilu = last_error_of_this_thread();
      });
    int rc_direct = DDM_OK;
    std::string why_not;
    probe_thread.join();
    if (P->preconditioner == 0 && probe_flops > 4.0 * P->max_direct_flops) { // declined by the early probe: no second analysis
      char buf[256];
      std::snprintf(buf, sizeof buf, "sparse direct solver: the factorisation needs about %.1g flops (estimate from the first separator of the largest block; limit %.3g)",
                    probe_flops, P->max_direct_flops);
      why_not = buf;
      rc_direct = DDM_ENOTIMPL;
    } else if (P->preconditioner != 1) {
      rc_direct = direct_create_impl(ctx, At.get(), nsub, Q.sub_ptr, 0, P->preconditioner == 2 ? 0.0 : P->max_direct_flops, /*setup_use=*/true, out_ptr(T));
      if (rc_direct == DDM_OK) direct = 1;
      else why_not = last_error_of_this_thread();
    }
    t_direct = seconds_since(t_begin);
    ilu_thread.join();
    if (direct) {
      T_ilu.reset(); // (speculative work, not needed)
    } else {
      if (P->preconditioner != 1 && (P->preconditioner == 2 || (rc_direct != DDM_ENOTIMPL && rc_direct != DDM_ENUMERIC))) return fail(ctx, rc_direct, "%s", why_not.c_str());
      if (P->preconditioner != 1 && P->verbose) std::fprintf(stderr, "[ddm geneo] sparse Cholesky not used (%s): ILU(0) preconditioner\n", why_not.c_str());
      if (rc_ilu) return fail(ctx, rc_ilu, "%s", err_ilu.c_str());
      T = std::move(T_ilu);
    }
    // ILU(0) as the preconditioner of the block iteration: single-precision sweeps (the iteration only needs a fixed search direction
    // W = T r; eigenpairs and residuals are computed in double).  DDM_GENEO_ILU_F64=1 keeps the sweeps in double.
    prec_f32 = !direct && !std::getenv("DDM_GENEO_ILU_F64");
    refresh_period = std::getenv("DDM_GENEO_REFRESH") ? std::max(1, std::atoi(std::getenv("DDM_GENEO_REFRESH"))) : (direct ? 2 : 8);
    // W <- W - X (A~X)^T W before the Rayleigh-Ritz step: twice with the exact T (W = A~^-1 r lies almost in span X near convergence: on
    // the elasticity pencil one pass gave 68-81 block iterations in two of eight runs, none 133 in one, against 12-18 -- measured before the products of P were refreshed, see below), once with
    // ILU(0) (216^3: the same 109 iterations and residuals with two, one or no pass; 5.6 / 5.2 / 4.9 s).  DDM_GENEO_ORTH_PASSES overrides.
    orth_passes = std::getenv("DDM_GENEO_ORTH_PASSES") ? std::max(0, std::atoi(std::getenv("DDM_GENEO_ORTH_PASSES"))) : (direct ? 2 : 1);
    t_prec = seconds_since(t_begin);
    DDMCHECK(csr_wait_upload(ctx, At.get()));
    t_setup = seconds_since(t_begin);
    if (P->verbose)
      std::fprintf(stderr, "[ddm geneo] setup: pencil %.2f s, sparse direct attempt %.2f s (%s), rest of the ILU(0) setup (helper thread) %.2f s, rest of the matrix upload (helper thread) %.2f s\n",
                   t_pencil, t_direct - t_upload, direct ? "used" : "declined", t_prec - t_direct, t_setup - t_prec);
    return DDM_OK;
  }

  // ---- Dirichlet mask and POU on the device ----
  int upload_masks()
  {
    std::vector<double> mk((size_t)n);
    for (int64_t i = 0; i < n; ++i) mk[(size_t)i] = (Q.dirichlet && Q.dirichlet[i]) ? 0.0 : 1.0;
    DDMCHECK(upload(ctx, mk.data(), n, maskd));
    return upload(ctx, Q.pou, n, poud);
  }
};

// One run of the block eigensolver at a fixed block width on a GeneoSetup: the work space and the loop.  geneo_run calls the phases in order.
struct GeneoRun {
  static constexpr double tau = 1e-11; // rank tolerance of the Rayleigh-Ritz step
  ddm_ctx *const ctx;
  GeneoSetup &K;
  const GeneoProblem &Q;
  const ddm_geneo_params &P;
  const int64_t n, nsub;
  const int nev, m, p, q2; // block width m = nev + extra, p = 3 m columns of S = [X | W | P], q2 = 2 m: the fused rotation [X_new | P_new]
  const int64_t ld;
  const csr_ptr &C, &At; // the setup's pencil and preconditioner, under the names the phases use
  const ilu0_ptr &T;
  const int direct;
  const bool prec_f32;
  const int refresh_period, orth_passes;
  const double *const maskd, *const poud;
  GeneoWork W;
  dbuf<double> S[2], AS[2], CS[2], R; // double-buffered [X | W | P] and its products, residual block
  dbuf<double> gA, gC, gmm[5], svec[2], Yd, mud;
  std::vector<double> hA, hC, hY, hmu, h_rr, h_rw, h_aa;
  std::vector<double> dscale; // column scaling of S = [X | W | P] folded into the projected problem
  int cur = 0, rank_min = 0;
  double worst = 0.0;

  GeneoRun(GeneoSetup &k, int nev_)
      : ctx(k.ctx), K(k), Q(k.Q), P(*k.P), n(k.n), nsub(k.nsub), nev(nev_), m(nev_ + std::max(k.P->extra, 1)), p(3 * m), q2(2 * m), ld(p), C(k.C), At(k.At), T(k.T),
        direct(k.direct), prec_f32(k.prec_f32), refresh_period(k.refresh_period), orth_passes(k.orth_passes), maskd(k.maskd), poud(k.poud), rank_min(p)
  {
  }
  // A~ X and C~ X of the same m-column block in one pass (the two matrices share their pattern: build_pencil_host)
  int apply_AC(const double *X, double *YA, double *YC)
  {
    if (!Q.op_C) return csr_mm2_ld(ctx, At.get(), C.get(), m, X, ld, YA, YC, ld);
    DDMCHECK(csr_mm_ld(ctx, At.get(), m, X, ld, YA, ld));
    return (*Q.op_C)(m, X, ld, YC, ld);
  }

  // ---- work space ----
  int allocate()
  {
    DDMCHECK(W.setup(ctx, nsub, Q.sub_ptr, (size_t)p * p * 2, /*rows_to_sub=*/true)); // (two products per chunk: gram2_sym)
    for (int b = 0; b < 2; ++b) {
      DDMCHECK(W.alloc(S[b], (size_t)n * p));
      DDMCHECK(W.alloc(AS[b], (size_t)n * p));
      DDMCHECK(W.alloc(CS[b], (size_t)n * p));
      HIPCHECK(ctx, hipMemsetAsync(S[b], 0, sizeof(double) * (size_t)n * p, ctx->stream));
      HIPCHECK(ctx, hipMemsetAsync(AS[b], 0, sizeof(double) * (size_t)n * p, ctx->stream));
      HIPCHECK(ctx, hipMemsetAsync(CS[b], 0, sizeof(double) * (size_t)n * p, ctx->stream));
    }
    DDMCHECK(W.alloc(R, (size_t)n * m));
    DDMCHECK(W.alloc(gA, (size_t)nsub * p * p));
    DDMCHECK(W.alloc(gC, (size_t)nsub * p * p));
    for (int k = 0; k < 5; ++k) DDMCHECK(W.alloc(gmm[k], (size_t)nsub * m * m));
    for (int k = 0; k < 2; ++k) DDMCHECK(W.alloc(svec[k], (size_t)nsub * m));
    DDMCHECK(W.alloc(Yd, (size_t)nsub * p * q2));
    DDMCHECK(W.alloc(mud, (size_t)nsub * m));
    for (auto *h : {&hA, &hC}) h->resize((size_t)nsub * p * p);
    for (auto *h : {&h_rr, &h_rw, &h_aa}) h->resize((size_t)nsub * m * m);
    hY.resize((size_t)nsub * p * q2);
    hmu.resize((size_t)nsub * m);
    dscale.assign((size_t)nsub * p, 1.0);
    return DDM_OK;
  }

  // ---- initial block: random on the free DoFs (the first pass of the loop is then a Rayleigh-Ritz step on span X alone) ----
  // kept (optional): an n x ldk block whose first mk columns start the run instead (a warm run: the previous eigenvectors of a slightly
  // changed pencil); the remaining columns are drawn as in the cold start, the products are computed fresh.
  int start_block(const double *kept = nullptr, int mk = 0, int64_t ldk = 0)
  {
    const unsigned long long seed = 0x5DEECE66Dull + (unsigned long long)P.seed;
    if (kept && mk > 0) launch_geneo_start_block(ctx, n, m, std::min(mk, m), ldk, seed, maskd, kept, S[0]);
    else launch_geneo_random(ctx, n, m, ld, seed, maskd, S[0]);
    if (Q.con) DDMCHECK(harmonic_apply(ctx, Q.con, m, S[0], ld, true));
    return apply_AC(S[0], AS[0], CS[0]);
  }

  // ---- search directions: R = C X - mu A~ X ; column norms ; W = T R, orthogonalised against X, and its products ----
  int search_directions()
  {
    launch_geneo_residual(ctx, n, m, W.sub_of_row, mud, AS[cur], ld, CS[cur], ld, R, m);
    if (Q.con) DDMCHECK(harmonic_apply_transposed(ctx, Q.con, m, R, m)); // residual of the constrained problem: P^T r
    DDMCHECK(W.gram(R, m, m, R, m, m, gmm[0]));
    HIPCHECK(ctx, hipMemcpyAsync(h_rr.data(), gmm[0], sizeof(double) * h_rr.size(), hipMemcpyDeviceToHost, ctx->stream));
    // (W = T r with the residual columns as they are: their scaling is folded into the projected problem below, like W's and P's)
    double *Wb = S[cur] + m, *AWb = AS[cur] + m, *CWb = CS[cur] + m;
    DDMCHECK(ilu0_solve_multi_ld(ctx, T.get(), m, R, m, Wb, ld, prec_f32));
    DDMCHECK(W.gram(R, m, m, Wb, ld, m, gmm[1])); // r^T T r per column (diagonal)
    HIPCHECK(ctx, hipMemcpyAsync(h_rw.data(), gmm[1], sizeof(double) * h_rw.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (Q.con) DDMCHECK(harmonic_apply(ctx, Q.con, m, Wb, ld, true)); // W = P T P^T r stays in the subspace
    DDMCHECK(W.gram(AS[cur], ld, m, AS[cur], ld, m, gmm[2]));
    HIPCHECK(ctx, hipMemcpyAsync(h_aa.data(), gmm[2], sizeof(double) * h_aa.size(), hipMemcpyDeviceToHost, ctx->stream));
    // W <- W - X (A~X)^T W   (orth_passes times), then A~-normalise the columns of W
    for (int pass = 0; pass < orth_passes; ++pass) {
      DDMCHECK(W.gram(AS[cur], ld, m, Wb, ld, m, gmm[3]));
      const double *Ux[1] = {S[cur]};
      double *Ox[1] = {Wb};
      const double *Bx[1] = {Wb};
      DDMCHECK(W.rotate(1, Ux, Ox, Bx, ld, m, gmm[3], m, ld, ld));
    }
    // A~-normalisation of the columns of W and P (zero columns stay zero): the blocks themselves are NOT rescaled (six passes over
    // n x m blocks per iteration in round 2) -- the diagonal scaling D is applied where it is cheap: to the p x p Gram matrices
    // (D G D) and to the rows of the Ritz coefficients (S D) Y = S (D Y), on the host; the norms W^T A~ W, P^T A~ P are the diagonal
    // of the unscaled S^T A~ S that is computed next anyway (two separate m x m products until round 3)
    return apply_AC(Wb, AWb, CWb); // both products of W in one pass over it
  }

  // ---- projected problem: S^T (A~ S) and S^T (C~ S) per subdomain, on the host when this returns ----
  int projected_problem()
  {
    const bool upper_only = W.gram2_sym(S[cur], ld, AS[cur], CS[cur], ld, p, gA, gC);
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipMemcpyAsync(hA.data(), gA, sizeof(double) * hA.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipMemcpyAsync(hC.data(), gC, sizeof(double) * hC.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (upper_only)
      for (int64_t s = 0; s < nsub; ++s) {
        GeneoWork::gram2_mirror_host(p, hA.data() + (size_t)s * p * p);
        GeneoWork::gram2_mirror_host(p, hC.data() + (size_t)s * p * p);
      }
    return DDM_OK;
  }

  // ---- residual test: the residuals of the block that entered this iteration (its Ritz values are still in hmu); true = converged ----
  bool residual_test(int it)
  {
    worst = 0.0;
    int64_t nconv_cols = 0;
    int lead_min = nev; // converged columns in front of the first unconverged one, minimum over the subdomains
    for (int64_t s = 0; s < nsub; ++s) {
      int lead = 0;
      bool leading = true;
      for (int j = 0; j < nev; ++j) {
        const size_t dj = ((size_t)s * m + j) * m + j;
        const double rn = std::sqrt(std::max(h_rr[dj], 0.0)), mu = std::fabs(hmu[(size_t)s * m + j]);
        const double res = direct ? std::sqrt(std::fabs(h_rw[dj])) / std::max(mu, 1e-300) // sqrt(r^T T r) / mu
                                  : rn / std::max(mu * std::sqrt(std::max(h_aa[dj], 0.0)), 1e-300);
        worst = std::max(worst, res);
        if (res < P.tolerance) {
          ++nconv_cols;
          if (leading) ++lead;
        } else
          leading = false;
      }
      lead_min = std::min(lead_min, lead);
    }
    if (P.verbose)
      std::fprintf(stderr, "[ddm geneo] it %3d  worst residual %.3e  rank >= %d  lambda_min(sub 0) %.6g  converged columns %lld of %lld, leading (min over subdomains) %d\n", it, worst,
                   rank_min, 1.0 / hmu[0] - P.shift, (long long)nconv_cols, (long long)(nsub * nev), lead_min);
    return worst < P.tolerance;
  }

  // ---- Rayleigh-Ritz per subdomain on host threads, the column scaling folded in (with_wp: the W and P columns are there) ----
  int rayleigh_ritz(bool with_wp)
  {
    const int nth = (int)std::min<int64_t>(nsub, host_threads());
    std::vector<std::thread> th;
    std::vector<int> ranks((size_t)nsub, 0);
    for (int t = 0; t < nth; ++t)
      th.emplace_back([&, t]() {
        std::vector<double> Y1((size_t)p * m);
        for (int64_t s = t; s < nsub; s += nth) {
          double *d = dscale.data() + (size_t)s * p;
          for (int i = 0; i < p; ++i) d[i] = 1.0;
          if (with_wp)
            for (int j = 0; j < m; ++j) {
              const double gw = hA[(size_t)s * p * p + (size_t)(m + j) * p + (m + j)], gp = hA[(size_t)s * p * p + (size_t)(2 * m + j) * p + (2 * m + j)];
              d[m + j] = gw > 1e-300 ? 1.0 / std::sqrt(gw) : 0.0;
              d[2 * m + j] = gp > 1e-300 ? 1.0 / std::sqrt(gp) : 0.0;
            }
          double *gAs = hA.data() + (size_t)s * p * p, *gCs = hC.data() + (size_t)s * p * p;
          for (int i = 0; i < p; ++i)
            for (int j = 0; j < p; ++j) {
              gAs[(size_t)i * p + j] *= d[i] * d[j];
              gCs[(size_t)i * p + j] *= d[i] * d[j];
            }
          const int r = dense::rayleigh_ritz(p, gAs, gCs, m, tau, hmu.data() + (size_t)s * m, Y1.data());
          ranks[(size_t)s] = r;
          if (r < m) continue;
          double *Y = hY.data() + (size_t)s * p * q2; // [Y | Y with the X rows zeroed]: X_new = S Y, P_new = [W P] Y_{W,P}
          for (int i = 0; i < p; ++i)
            for (int j = 0; j < m; ++j) {
              const double y = d[i] * Y1[(size_t)i * m + j];
              Y[(size_t)i * q2 + j] = y;
              Y[(size_t)i * q2 + m + j] = i < m ? 0.0 : y;
            }
        }
      });
    for (auto &t : th) t.join();
    rank_min = p;
    for (int64_t s = 0; s < nsub; ++s) {
      if (ranks[(size_t)s] < m) return fail(ctx, DDM_ENUMERIC, "GenEO: Rayleigh-Ritz failed in subdomain %lld (rank %d of the block basis)", (long long)s, ranks[(size_t)s]);
      rank_min = std::min(rank_min, ranks[(size_t)s]);
    }
    return DDM_OK;
  }

  // ---- rotation: [X | . | P] of the other buffer <- S [Y | Y_wp]: two column blocks of one rotation (q = 2m, written with a gap of m columns) ----
  int rotate_blocks()
  {
    HIPCHECK(ctx, hipMemcpyAsync(Yd, hY.data(), sizeof(double) * hY.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(ctx, hipMemcpyAsync(mud, hmu.data(), sizeof(double) * hmu.size(), hipMemcpyHostToDevice, ctx->stream));
    const int nxt = cur ^ 1;
    const double *U3[3] = {S[cur], AS[cur], CS[cur]};
    double *O3[3] = {S[nxt], AS[nxt], CS[nxt]};
    // first m output columns -> X slot, the other m -> P slot (the W slot in between is overwritten by the next preconditioner solve)
    DDMCHECK(W.rotate(3, U3, O3, nullptr, ld, p, Yd, q2, ld, ld, /*gap_from=*/m, /*gap=*/m));
    cur = nxt;
    return DDM_OK;
  }

  // ---- refresh A~X, C X from X and A~P, C P from P: the products are carried along by the rotations and drift.  With the exact T every
  // second iteration: W and P shrink geometrically there (their scaling lives in the projected problem, the blocks are not
  // renormalised), the Ritz coefficients of such columns are large, and products of P that are never recomputed went wrong often
  // enough to matter -- on the elasticity pencil 12-18 block iterations in most runs but 36-120 or no convergence within 400 in
  // about one run of seven (the device factor's atomics make every run round differently); with P refreshed as well: 12-16 in 28
  // of 28 runs, refreshing X alone does not help (tools/geneo_variability.sh).  With ILU(0) every eighth iteration, as before.
  int refresh()
  {
    if (Q.con) DDMCHECK(harmonic_apply(ctx, Q.con, m, S[cur], ld, true));
    DDMCHECK(apply_AC(S[cur], AS[cur], CS[cur]));
    return apply_AC(S[cur] + 2 * m, AS[cur] + 2 * m, CS[cur] + 2 * m);
  }

  // ---- output: eigenvalues lambda = 1 / mu - sigma, finalised basis (nev x n on the device) ----
  int output(double *basis_dev, double *eig_host)
  {
    for (int64_t s = 0; s < nsub; ++s)
      for (int j = 0; j < nev; ++j) eig_host[(size_t)s * nev + j] = 1.0 / hmu[(size_t)s * m + j] - P.shift;
    launch_geneo_copy_cols(ctx, n, m, S[cur], ld, R, m);
    if (!P.raw) launch_geneo_rowscale(ctx, n, m, poud, R, m); // v <- D v
    DDMCHECK(W.gram(R, m, m, R, m, m, gmm[0]));
    launch_geneo_invsqrt_diag(ctx, nsub, m, gmm[0], svec[0]); // 1 / ||D v||_2  (raw: 1 / ||v||_2)
    launch_geneo_rowscale(ctx, n, m, maskd, R, m);            // zero_at_dirichlet
    launch_geneo_finalize(ctx, n, nev, W.sub_of_row, svec[0], m, R, m, basis_dev);
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    return DDM_OK;
  }
};

#include "geneo_solver.hpp"

// One path for every entry point: an object without origin map, one cold compute, gone.
static int geneo_basis_impl(ddm_ctx *ctx, const GeneoProblem &Q, const ddm_geneo_params *params, int64_t kmax, double *basis_host, int32_t *nconv, double *eigenvalues_host,
                            ddm_geneo_info *info)
{
  if (!basis_host || !nconv || !eigenvalues_host) return fail(ctx, DDM_EINVAL, "%s: bad arguments", Q.who);
  geneo_ptr G;
  DDMCHECK(geneo_create_impl(ctx, Q, params, /*want_origin=*/false, out_ptr(G)));
  return geneo_compute_impl(ctx, G.get(), /*start=*/0, /*keep=*/false, kmax, basis_host, nconv, eigenvalues_host, info);
}

extern "C" int ddm_geneo_basis(ddm_ctx *ctx, const ddm_csr *A_neu, const ddm_csr *B_neu, int64_t nsub, const int64_t *sub_ptr, const double *pou_host,
                               const uint8_t *dirichlet_host, const ddm_geneo_params *params, int64_t kmax, double *basis_host, int32_t *nconv,
                               double *eigenvalues_host, ddm_geneo_info *info)
{
  const GeneoProblem Q{"ddm_geneo_basis", A_neu, B_neu, nsub, sub_ptr, pou_host, dirichlet_host};
  return geneo_basis_impl(ctx, Q, params, kmax, basis_host, nconv, eigenvalues_host, info);
}

// Rows as MsGFEM (coarse_spaces.hh:722-740) and the SVD space (:1293-1309) sort them: cls = 0 interior, 1 subdomain boundary, 2 global
// Dirichlet; pou_int = the partition of unity on the interior rows, zero elsewhere
static void classify_rows(int64_t n, const uint8_t *dirichlet, const uint8_t *boundary, const double *pou, std::vector<uint8_t> &cls, std::vector<double> &pou_int)
{
  cls.resize((size_t)n);
  pou_int.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    cls[(size_t)i] = (dirichlet && dirichlet[i]) ? 2 : boundary[i] ? 1 : 0;
    pou_int[(size_t)i] = cls[(size_t)i] == 0 ? pou[i] : 0.0;
  }
}

// MsGFEMCoarseSpace::setup_msgfem_impl (coarse_spaces.hh:712-826).  The reference assembles the saddle-point pencil
//     [A_nn  G^T; G  0] [u; p] = lambda [D A_ii D  0; 0  0] [u; p],      G = interior rows of A_dir (a-harmonicity),
// on the non-Dirichlet DoFs and hands it to the shift-invert Lanczos with an LU of the indefinite matrix.  Here the multipliers are
// eliminated instead: the same eigenpairs are the stationary points of the Rayleigh quotient of (A_neu, D A_ii D) on the
// a-harmonic subspace {u : G u = 0, u = 0 on Dirichlet DoFs}, and the block iteration of geneo_run stays inside that subspace
// with the projection P = [0 -A_ii^-1 A_ib; 0 I] (ddm_harmonic: one sparse Cholesky of the interior block, multi-RHS solves):
// start block P X0, search directions P T P^T r.  With the exact T = (A_neu + sigma C)^-1 the preconditioned operator is the
// inverse of the Schur complement onto the boundary unknowns, i.e. the iteration is the device analogue of the shift-invert.
extern "C" int ddm_msgfem_basis(ddm_ctx *ctx, const ddm_csr *A_neu, const ddm_csr *A_dir, int64_t nsub, const int64_t *sub_ptr, const double *pou_host,
                                const uint8_t *dirichlet_host, const uint8_t *boundary_host, const ddm_geneo_params *params, int64_t kmax, double *basis_host,
                                int32_t *nconv, double *eigenvalues_host, ddm_geneo_info *info)
{
  if (!ctx || !A_neu || !A_dir || !sub_ptr || !pou_host || !boundary_host || !params || nsub < 1) return fail(ctx, DDM_EINVAL, "ddm_msgfem_basis: bad arguments");
  if (A_dir->nrows != A_neu->nrows || A_dir->ncols != A_dir->nrows) return fail(ctx, DDM_EINVAL, "The two matrices must have the same size"); // :714
  std::vector<uint8_t> cls;
  std::vector<double> pou_int; // the right-hand side has interior x interior entries only (:801-811)
  classify_rows(A_dir->nrows, dirichlet_host, boundary_host, pou_host, cls, pou_int);
  harmonic_ptr H;
  DDMCHECK(harmonic_create_impl(ctx, A_dir, nsub, sub_ptr, cls.data(), true, out_ptr(H)));
  if (!H->symmetric) return fail(ctx, DDM_ENOTIMPL, "ddm_msgfem_basis: the interior block of A_dir is not symmetric");
  const GeneoProblem Q{"ddm_msgfem_basis", A_neu, A_neu, nsub, sub_ptr, pou_host, dirichlet_host, H.get(), pou_int.data()};
  return geneo_basis_impl(ctx, Q, params, kmax, basis_host, nconv, eigenvalues_host, info);
}

// Y = T T^T X = D A^^-1 G_ib G_bi A^^-T D X for the symmetric interior block of H (d: DEVICE vector D, zero outside the interior)
static int harmonic_apply_ttt(ddm_ctx *ctx, ddm_harmonic *H, const double *d, int m, const double *X, int64_t ldx, double *Y, int64_t ldy)
{
  const int64_t n = H->n;
  HIPCHECK(ctx, reserve_cols<double>(H->tcols, m, {{H->t1, H->n}, {H->t2, H->n}}));
  const unsigned gr = (unsigned)((n * (int64_t)m + 255) / 256);
  hipLaunchKernelGGL(k_geneo_rowscale_to, dim3(gr), dim3(256), 0, ctx->stream, n, m, d, X, ldx, H->t1, (int64_t)m); // D x
  DDMCHECK(ilu0_solve_multi_ld(ctx, H->F.get(), m, H->t1, m, H->t2, m));                                           // A_ii^-T
  DDMCHECK(csr_mm_ld(ctx, H->Gbi.get(), m, H->t2, m, H->t1, m));                                                   // A_{i,Gamma}^T
  DDMCHECK(csr_mm_ld(ctx, H->Gib.get(), m, H->t1, m, H->t2, m));                                                   // A_{i,Gamma}
  DDMCHECK(ilu0_solve_multi_ld(ctx, H->F.get(), m, H->t2, m, H->t1, m));                                           // A_ii^-1
  hipLaunchKernelGGL(k_geneo_rowscale_to, dim3(gr), dim3(256), 0, ctx->stream, n, m, d, (const double *)H->t1, (int64_t)m, Y, ldy); // D
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}

// SVDCoarseSpace (coarse_spaces.hh:1268-1407): the leading left singular vectors of T = D A_ii^-1 A_{i,Gamma} (interior x subdomain
// boundary; the reference forms T densely column by column and calls Eigen's bdcSvd).  Here: the leading eigenvectors of
//     T T^T = D A_ii^-1 (A_{i,Gamma} A_{i,Gamma}^T) A_ii^-T D
// by the block eigensolver of geneo_run with the identity as left-hand matrix and T T^T applied as an operator -- two multi-RHS
// interior solves (the sparse direct factor of ddm_harmonic) around two sparse products per application; T is never formed.
extern "C" int ddm_svd_basis(ddm_ctx *ctx, const ddm_csr *A_dir, int64_t nsub, const int64_t *sub_ptr, const double *pou_host, const uint8_t *dirichlet_host,
                             const uint8_t *boundary_host, int n_vectors, int mult_pou, double tolerance, int maxit, double *basis_host, double *singular_values_host,
                             ddm_geneo_info *info)
{
  if (!ctx || !A_dir || !sub_ptr || !pou_host || !boundary_host || !basis_host || !singular_values_host || nsub < 1 || n_vectors < 1)
    return fail(ctx, DDM_EINVAL, "ddm_svd_basis: bad arguments");
  if (A_dir->nrows != A_dir->ncols || sub_ptr[0] != 0 || sub_ptr[nsub] != A_dir->nrows) return fail(ctx, DDM_EINVAL, "ddm_svd_basis: sub_ptr does not cover the matrix");
  const int64_t n = A_dir->nrows;
  std::vector<uint8_t> cls, notint((size_t)n);
  std::vector<double> pou_int, ones((size_t)n, 1.0);
  classify_rows(n, dirichlet_host, boundary_host, pou_host, cls, pou_int);
  for (int64_t i = 0; i < n; ++i) notint[(size_t)i] = cls[(size_t)i] != 0;
  harmonic_ptr Hown;
  DDMCHECK(harmonic_create_impl(ctx, A_dir, nsub, sub_ptr, cls.data(), true, out_ptr(Hown)));
  ddm_harmonic *const H = Hown.get();
  if (!H->symmetric) return fail(ctx, DDM_ENOTIMPL, "ddm_svd_basis: the interior block of A_dir is not symmetric");
  std::vector<int64_t> rp((size_t)n + 1);
  std::vector<int32_t> ci((size_t)n);
  for (int64_t i = 0; i <= n; ++i) rp[(size_t)i] = i;
  for (int64_t i = 0; i < n; ++i) ci[(size_t)i] = (int32_t)i;
  csr_ptr I;
  dbuf<double> d;
  DDMCHECK(ddm_csr_create(ctx, n, n, rp.data(), ci.data(), ones.data(), out_ptr(I)));
  DDMCHECK(upload(ctx, pou_int.data(), n, d));
  const BlockOp op = [&](int m, const double *X, int64_t ldx, double *Y, int64_t ldy) -> int { return harmonic_apply_ttt(ctx, H, d, m, X, ldx, Y, ldy); };
  ddm_geneo_params P;
  ddm_geneo_params_default(&P);
  P.nev = n_vectors;
  P.extra = std::max(4, n_vectors / 2);
  P.shift = 0.0;            // A~ = I
  P.tolerance = tolerance > 0.0 ? tolerance : 1e-8;
  P.maxit = maxit > 0 ? maxit : 400;
  P.preconditioner = 1;     // ILU(0) of the identity: no preconditioner
  P.raw = mult_pou ? 0 : 1; // :1403: finalize_eigenvectors only with mult_pou
  std::vector<int32_t> nconv((size_t)nsub);
  std::vector<double> eig((size_t)nsub * n_vectors);
  const GeneoProblem Q{"ddm_svd_basis", I.get(), I.get(), nsub, sub_ptr, pou_host, notint.data(), nullptr, ones.data(), &op};
  DDMCHECK(geneo_basis_impl(ctx, Q, &P, n_vectors, basis_host, nconv.data(), eig.data(), info));
  for (size_t k = 0; k < eig.size(); ++k) singular_values_host[k] = 1.0 / std::sqrt(std::max(eig[k], 1e-300)); // mu = sigma^2 = 1 / lambda
  return DDM_OK;
}

// ---- ddm_harmonic read-only and step by step (for tests: tests/test_gpu_harmonic_shapes.py) -----------------------------------------
// Each export forwards to the function the builders call -- harmonic_create_impl, harmonic_apply, harmonic_apply_transposed,
// harmonic_apply_ttt -- with the caller's classes, DEVICE pointers, widths and leading dimensions; none chunks, dispatches or sizes a grid.
extern "C" int ddm_harmonic_create_classes(ddm_ctx *ctx, const ddm_csr *A, int64_t nblocks, const int64_t *block_ptr, const uint8_t *cls_host, int want_transpose,
                                           ddm_harmonic **out)
{
  if (!ctx || !A || !out || nblocks < 1 || !block_ptr || !cls_host) return fail(ctx, DDM_EINVAL, "ddm_harmonic_create_classes: bad arguments");
  if (A->nrows != A->ncols) return fail(ctx, DDM_EINVAL, "ddm_harmonic_create_classes: square matrix expected");
  return harmonic_create_impl(ctx, A, nblocks, block_ptr, cls_host, want_transpose != 0, out);
}
// op 0: X <- extension (harmonic_apply, keep); 1: X <- P X (keep_b); 2: X <- P^T X; 3: Y = T T^T X with D = pou_int (HOST, n entries;
// synchronous).  Ops 0 .. 2 work in place and ignore pou_int, Y and ldy.
extern "C" int ddm_harmonic_debug_apply(ddm_ctx *ctx, ddm_harmonic *H, int op, int nrhs, double *X, int64_t ldx, const double *pou_int, double *Y, int64_t ldy)
{
  if (!ctx || !H || !X || op < 0 || op > 3 || nrhs < 1 || ldx < nrhs) return fail(ctx, DDM_EINVAL, "ddm_harmonic_debug_apply: bad arguments");
  if (op <= 1) return harmonic_apply(ctx, H, nrhs, X, ldx, op == 1);
  if (!H->symmetric) return fail(ctx, DDM_ENOTIMPL, "ddm_harmonic_debug_apply: the interior block is not symmetric");
  if (!H->Gbi) return fail(ctx, DDM_EINVAL, "ddm_harmonic_debug_apply: the object was created without G_bi");
  if (op == 2) return harmonic_apply_transposed(ctx, H, nrhs, X, ldx);
  if (!pou_int || !Y || Y == X || ldy < nrhs) return fail(ctx, DDM_EINVAL, "ddm_harmonic_debug_apply: bad arguments");
  dbuf<double> d;
  DDMCHECK(upload(ctx, pou_int, H->n, d));
  DDMCHECK(harmonic_apply_ttt(ctx, H, d, nrhs, X, ldx, Y, ldy));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream)); // (d goes out of scope)
  return DDM_OK;
}
// out: n, symmetric, nnz(G_ib), nnz(G_bi) (-1: absent), 1 = device supernodal factor, the factor's nnz, its refinement steps, columns
// the work blocks hold
extern "C" int ddm_harmonic_info(const ddm_harmonic *H, int64_t *out)
{
  if (!H || !out) return DDM_EINVAL;
  out[0] = H->n;
  out[1] = H->symmetric ? 1 : 0;
  out[2] = H->Gib ? H->Gib->nnz : -1;
  out[3] = H->Gbi ? H->Gbi->nnz : -1;
  out[4] = H->F && H->F->sn ? 1 : 0;
  out[5] = ddm_ilu0_nnz(H->F.get());
  out[6] = ddm_ilu0_refinement(H->F.get(), nullptr);
  out[7] = H->tcols;
  return DDM_OK;
}
// the host arrays of G_ib (which = 0) or G_bi (1): rowptr[n + 1], col[nnz], val[nnz], each copied where not NULL
extern "C" int ddm_harmonic_get_host(const ddm_harmonic *H, int which, int64_t *rowptr, int32_t *col, double *val)
{
  if (!H || which < 0 || which > 1) return DDM_EINVAL;
  const ddm_csr *G = which ? H->Gbi.get() : H->Gib.get();
  if (!G) return DDM_EINVAL;
  if (rowptr) std::copy(G->h_rp.begin(), G->h_rp.end(), rowptr);
  if (col) std::copy(G->h_ci.begin(), G->h_ci.end(), col);
  if (val) std::copy(G->h_va.begin(), G->h_va.end(), val);
  return DDM_OK;
}

// ---- the device steps of GeneoRun on their own (for tests: tests/test_gpu_geneo_steps.py) -------------------------------------------
// Each export forwards to the function GeneoRun calls -- csr_mm_ld, csr_adopt + csr_mm2_ld, ilu0_solve_multi_ld, GeneoWork::rotate,
// the launch_geneo_* functions -- with the caller's pointers and leading dimensions; none repeats a dispatch or a grid computation.
// Block pointers are DEVICE pointers; nothing synchronises unless said.
extern "C" int ddm_csr_mm_ld(ddm_ctx *ctx, const ddm_csr *A, int nrhs, const double *X, int64_t ldx, double *Y, int64_t ldy)
{
  if (!ctx) return DDM_EINVAL;
  return csr_mm_ld(ctx, A, nrhs, X, ldx, Y, ldy);
}
extern "C" int ddm_csr_pair_create(ddm_ctx *ctx, int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, const double *val2, int64_t nblocks,
                                   const int64_t *block_ptr, ddm_csr **out, ddm_csr **companion)
{
  if (!ctx || !rowptr || !out || !companion || n < 1 || n >= (int64_t)1 << 31 || rowptr[0] != 0 || (nblocks > 0 && (!block_ptr || block_ptr[0] != 0 || block_ptr[nblocks] != n)))
    return fail(ctx, DDM_EINVAL, "ddm_csr_pair_create: bad arguments");
  for (int64_t i = 0; i < n; ++i)
    if (rowptr[i + 1] < rowptr[i]) return fail(ctx, DDM_EINVAL, "ddm_csr_pair_create: row pointers not monotone at row %lld", (long long)i);
  const int64_t nnz = rowptr[n];
  if (nnz > 0 && (!col || !val || !val2)) return fail(ctx, DDM_EINVAL, "ddm_csr_pair_create: bad arguments");
  for (int64_t k = 0; k < nnz; ++k)
    if (col[k] < 0 || col[k] >= n) return fail(ctx, DDM_EINVAL, "ddm_csr_pair_create: column index out of range at entry %lld", (long long)k);
  hvec<int64_t> rp;
  hvec<int32_t> ci;
  hvec<double> va, vc;
  hvec_copy(rp, rowptr, (size_t)n + 1);
  hvec_copy(ci, col, (size_t)nnz);
  hvec_copy(va, val, (size_t)nnz);
  hvec_copy(vc, val2, (size_t)nnz);
  csr_ptr C, A;
  A.reset(csr_adopt(ctx, n, std::move(rp), std::move(ci), std::move(va), std::move(vc), out_ptr(C), nblocks, nblocks > 0 ? block_ptr : nullptr));
  DDMCHECK(csr_wait_upload(ctx, A.get()));
  *out = A.release();
  *companion = C.release();
  return DDM_OK;
}
extern "C" int ddm_csr_has_row_order(const ddm_csr *A) { return (A && A->row_order) ? 1 : 0; }
extern "C" int ddm_csr_mm2_ld(ddm_ctx *ctx, const ddm_csr *A1, const ddm_csr *A2, int nrhs, const double *X, int64_t ldx, double *Y1, double *Y2, int64_t ldy)
{
  if (!ctx || !A1 || !A2 || !X || !Y1 || !Y2 || Y1 == Y2) return fail(ctx, DDM_EINVAL, "ddm_csr_mm2_ld: bad arguments");
  return csr_mm2_ld(ctx, A1, A2, nrhs, X, ldx, Y1, Y2, ldy);
}
extern "C" int ddm_ilu0_solve_multi_ld(ddm_ctx *ctx, ddm_ilu0 *F, int nrhs, const double *D, int64_t ldd, double *X, int64_t ldx, int f32)
{
  if (!ctx) return DDM_EINVAL;
  return ilu0_solve_multi_ld(ctx, F, nrhs, D, ldd, X, ldx, f32 != 0);
}
// Out_k = (Base_k -) U_k Y[sub] for k < narr <= 3 arrays that share Y (nsub matrices p x q, host), output columns >= gap_from written
// gap columns further right: GeneoWork::rotate with all its arguments.  Base: null, or narr pointers.  Synchronous.
extern "C" int ddm_blockvec_rotate_multi(ddm_ctx *ctx, int64_t nsub, const int64_t *sub_ptr, int narr, const double *const *U, int64_t ldu, int p, const double *Y_host,
                                         int q, const double *const *Base, int64_t ldb, double *const *Out, int64_t ldo, int gap_from, int gap)
{
  if (!ctx || !sub_ptr || !U || !Y_host || !Out || nsub < 1 || narr < 1 || narr > 3 || p < 1 || q < 1 || ldu < p || gap_from < 0 || gap < 0 ||
      ldo < q + (gap_from < q ? gap : 0) || (Base && ldb < q))
    return fail(ctx, DDM_EINVAL, "ddm_blockvec_rotate_multi: bad arguments");
  for (int k = 0; k < narr; ++k)
    if (!U[k] || !Out[k] || (Base && !Base[k])) return fail(ctx, DDM_EINVAL, "ddm_blockvec_rotate_multi: bad arguments");
  GeneoWork W;
  DDMCHECK(W.setup(ctx, nsub, sub_ptr, 1));
  dbuf<double> Y;
  DDMCHECK(W.alloc(Y, (size_t)nsub * p * q));
  DDMCHECK(ddm_memcpy_h2d(ctx, Y, Y_host, (int64_t)sizeof(double) * nsub * p * q));
  DDMCHECK(W.rotate(narr, U, Out, Base, ldu, p, Y, q, ldo, ldb, gap_from, gap));
  return ddm_ctx_sync(ctx);
}
// One helper kernel of the eigensolver through its launch function.  sub_of_row comes from GeneoWork::setup(.., rows_to_sub = true) on
// sub_ptr.  n = sub_ptr[nsub]; a, b, s, out are device pointers.  Synchronous.
//   op 0  k_geneo_random      out[i, j] (ld ldo) = uniform(seed, i m + j) * a[i]                         a: mask (n)
//   op 1  k_geneo_residual    out[i, j] = b[i, j] - s[sub(i), j] a[i, j]                                  a: A~X (lda), b: C~X (ldb), s: mu (nsub x m)
//   op 2  k_geneo_copy_cols   out[i, j] = a[i, j]
//   op 3  k_geneo_rowscale    out[i, j] *= s[i]                                                           s: weights (n)
//   op 4  k_geneo_invsqrt_diag  out[sub, j] = 1 / sqrt(a[sub, j, j]) or 0                                 a: nsub Gram matrices m x m
//   op 5  k_geneo_finalize    out[j, i] = s[sub(i), j] a[i, j], j < nev  (out: nev x n)                   s: scales (nsub x m)
extern "C" int ddm_geneo_debug_helper(ddm_ctx *ctx, int op, int64_t nsub, const int64_t *sub_ptr, int m, int nev, uint64_t seed, const double *a, int64_t lda,
                                      const double *b, int64_t ldb, const double *s, double *out, int64_t ldo)
{
  if (!ctx || !sub_ptr || !out || nsub < 1 || m < 1 || op < 0 || op > 5 || sub_ptr[0] != 0) return fail(ctx, DDM_EINVAL, "ddm_geneo_debug_helper: bad arguments");
  const bool need_a = op != 3, need_b = op == 1, need_s = op == 1 || op == 3 || op == 5;
  if ((need_a && !a) || (need_b && !b) || (need_s && !s) || (op <= 3 && ldo < m) || ((op == 1 || op == 2 || op == 5) && lda < m) || (need_b && ldb < m) ||
      (op == 5 && (nev < 1 || nev > m)))
    return fail(ctx, DDM_EINVAL, "ddm_geneo_debug_helper: bad arguments");
  GeneoWork W;
  DDMCHECK(W.setup(ctx, nsub, sub_ptr, 1, /*rows_to_sub=*/true));
  const int64_t n = W.n;
  switch (op) {
  case 0: launch_geneo_random(ctx, n, m, ldo, (unsigned long long)seed, a, out); break;
  case 1: launch_geneo_residual(ctx, n, m, W.sub_of_row, s, a, lda, b, ldb, out, ldo); break;
  case 2: launch_geneo_copy_cols(ctx, n, m, a, lda, out, ldo); break;
  case 3: launch_geneo_rowscale(ctx, n, m, s, out, ldo); break;
  case 4: launch_geneo_invsqrt_diag(ctx, nsub, m, a, out); break;
  default: launch_geneo_finalize(ctx, n, nev, W.sub_of_row, s, m, a, lda, out); break;
  }
  HIPCHECK(ctx, hipGetLastError());
  return ddm_ctx_sync(ctx);
}
