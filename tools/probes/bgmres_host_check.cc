// Host check of the dense algebra behind block GMRES (dense::bgmres_factor and dense::BlockHessenberg, csrc/dense_host.hpp) under the
// sanitizers.  The factor: S^T S = G, C^T G C = I and the rank on a full-rank Gram matrix, one with a duplicated column, one with a zero
// column, p = 1, p = 32, a noise column judged against its scale before orthogonalisation (rank drops), the zero matrix (rank 0) and a
// NaN (refused).  The least squares: random block Hessenberg matrices (p = 1, 3, 8; up to 7 blocks; a rank-deficient sub-diagonal block
// at the end), the reported residual against the recomputed || E_1 T - Hbar Y || and the normal equations Hbar^T (E_1 T - Hbar Y) = 0.
// No device is touched.  From the repository root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o bgmres_host_check tools/probes/bgmres_host_check.cc
//   ./bgmres_host_check
#include "../../dune-ddm_amd/csrc/dense_host.hpp"

#include <cstdio>
#include <limits>
#include <random>

namespace {
using Mat = std::vector<double>;
Mat gram(int rows, int p, const Mat &W)
{
  Mat G((size_t)p * p, 0.0);
  for (int r = 0; r < rows; ++r)
    for (int i = 0; i < p; ++i)
      for (int j = 0; j < p; ++j) G[(size_t)i * p + j] += W[(size_t)r * p + i] * W[(size_t)r * p + j];
  return G;
}
Mat randn(size_t n, unsigned seed)
{
  std::mt19937_64 g(seed);
  std::normal_distribution<double> N;
  Mat A(n);
  for (double &a : A) a = N(g);
  return A;
}
int check_factor(const char *name, int p, const Mat &G, const double *scale2, int want_rank)
{
  Mat S((size_t)p * p, std::numeric_limits<double>::quiet_NaN()), C = S;
  int rank = -1;
  if (!dense::bgmres_factor(p, G.data(), scale2, 1e-12, S.data(), C.data(), &rank)) {
    std::printf("%s: refused\n", name);
    return 1;
  }
  double gmax = 0.0, e1 = 0.0, e2 = 0.0;
  for (double g : G) gmax = std::max(gmax, std::fabs(g));
  for (int i = 0; i < p; ++i)
    for (int j = 0; j < p; ++j) {
      double s = 0.0;
      for (int a = 0; a < p; ++a) s += S[(size_t)a * p + i] * S[(size_t)a * p + j];
      const double di = std::sqrt(std::fabs(scale2 ? scale2[i] : G[(size_t)i * p + i])), dj = std::sqrt(std::fabs(scale2 ? scale2[j] : G[(size_t)j * p + j]));
      e1 = std::max(e1, std::fabs(s - G[(size_t)i * p + j]) / ((di > 0 ? di : 1.0) * (dj > 0 ? dj : 1.0)));
    }
  for (int a = 0; a < rank; ++a)
    for (int b = 0; b < rank; ++b) {
      double s = 0.0;
      for (int i = 0; i < p; ++i)
        for (int j = 0; j < p; ++j) s += C[(size_t)i * p + a] * G[(size_t)i * p + j] * C[(size_t)j * p + b];
      e2 = std::max(e2, std::fabs(s - (a == b ? 1.0 : 0.0)));
    }
  std::printf("%s: p %d rank %d (want %d), |S^T S - G| %.2e (scaled), |C^T G C - I| %.2e\n", name, p, rank, want_rank, e1, e2);
  return rank == want_rank && e1 <= 1e-11 && e2 <= 1e-10 ? 0 : 1; // (e1 carries the dropped eigenvalues, below rank_tol = 1e-12)
}
int check_least_squares(int p, int m, int nblocks, bool deficient, unsigned seed)
{
  const int rows = (nblocks + 1) * p, cols = nblocks * p;
  Mat H((size_t)rows * cols, 0.0), T = randn((size_t)p * m, seed + 1);
  dense::BlockHessenberg ls;
  ls.start(p, m, T.data());
  for (int j = 0; j < nblocks; ++j) {
    Mat blk = randn((size_t)(j + 2) * p * p, seed + 10 + j);
    if (deficient && j == nblocks - 1)
      for (int i = 0; i < p; ++i) blk[(size_t)((j + 2) * p - 1) * p + i] = 0.0; // last row of S zero: a rank drop
    for (int i = 0; i < (j + 2) * p; ++i)
      for (int b = 0; b < p; ++b) H[(size_t)i * cols + j * p + b] = blk[(size_t)i * p + b];
    ls.add_block(blk.data());
  }
  Mat Y((size_t)cols * m, std::numeric_limits<double>::quiet_NaN());
  if (!ls.solve(Y.data())) return 1;
  double worst_res = 0.0, worst_normal = 0.0;
  for (int c = 0; c < m; ++c) {
    Mat r(rows, 0.0);
    for (int i = 0; i < rows; ++i) {
      r[i] = i < p ? T[(size_t)i * m + c] : 0.0;
      for (int a = 0; a < cols; ++a) r[i] -= H[(size_t)i * cols + a] * Y[(size_t)a * m + c];
    }
    double nr = 0.0;
    for (double e : r) nr += e * e;
    worst_res = std::max(worst_res, std::fabs(std::sqrt(nr) - ls.residual(c)));
    for (int a = 0; a < cols; ++a) {
      double s = 0.0;
      for (int i = 0; i < rows; ++i) s += H[(size_t)i * cols + a] * r[i];
      worst_normal = std::max(worst_normal, std::fabs(s));
    }
  }
  std::printf("least squares p %d m %d blocks %d%s: |residual - recomputed| %.2e, |Hbar^T r| %.2e\n", p, m, nblocks, deficient ? " (deficient)" : "", worst_res,
              worst_normal);
  return worst_res <= 1e-12 && worst_normal <= 1e-10 ? 0 : 1;
}
} // namespace

int main()
{
  int bad = 0;
  const int p = 8, rows = 40;
  const Mat W = randn((size_t)rows * p, 11);
  bad += check_factor("full rank", p, gram(rows, p, W), nullptr, 8);
  Mat Wd = W;
  for (int r = 0; r < rows; ++r) Wd[(size_t)r * p + 5] = Wd[(size_t)r * p + 2];
  bad += check_factor("duplicate", p, gram(rows, p, Wd), nullptr, 7);
  Mat Wz = W;
  for (int r = 0; r < rows; ++r) Wz[(size_t)r * p + 3] = 0.0;
  bad += check_factor("zero column", p, gram(rows, p, Wz), nullptr, 7);
  bad += check_factor("p1", 1, Mat{3.5}, nullptr, 1);
  bad += check_factor("p32", 32, gram(100, 32, randn((size_t)100 * 32, 12)), nullptr, 32);
  Mat Wn = W;
  for (int r = 0; r < rows; ++r) Wn[(size_t)r * p + 6] *= 1e-15; // what is left of a column of size one after the orthogonalisation
  Mat scale2(p);
  const Mat Gn = gram(rows, p, Wn);
  for (int i = 0; i < p; ++i) scale2[i] = i == 6 ? 1.0 : Gn[(size_t)i * p + i];
  bad += check_factor("noise column, own scale", p, Gn, nullptr, 8);
  bad += check_factor("noise column, earlier scale", p, Gn, scale2.data(), 7);
  bad += check_factor("all zero", 4, Mat(16, 0.0), nullptr, 0);
  Mat nan = gram(rows, p, W), S((size_t)p * p), C((size_t)p * p);
  nan[1 * p + 2] = std::numeric_limits<double>::quiet_NaN();
  int rank = -1;
  const bool refused = !dense::bgmres_factor(p, nan.data(), nullptr, 1e-12, S.data(), C.data(), &rank);
  std::printf("NaN entry: %s\n", refused ? "refused" : "ACCEPTED");
  bad += refused ? 0 : 1;
  bad += check_least_squares(1, 1, 7, false, 100);
  bad += check_least_squares(3, 5, 4, false, 200);
  bad += check_least_squares(8, 8, 3, false, 300);
  bad += check_least_squares(3, 5, 2, true, 400);
  bad += check_least_squares(32, 32, 2, false, 500);
  std::printf(bad ? "FAILED %d\n" : "bgmres_host_check ok\n", bad);
  return bad ? 1 : 0;
}
