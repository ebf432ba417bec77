// Host check of the pseudo-inverse behind block CG's coupling (dense::sym_pinv, csrc/dense_host.hpp) under the sanitizers: the Penrose
// conditions W W+ W = W and W+ W W+ = W+ and the returned rank on an SPD 8 x 8 matrix, the same with a duplicated row and column, with a
// zero row and column, with diagonal entries spread over 1e-20 .. 1, on m = 1, m = 32, the zero matrix (rank 0) and a matrix with a
// NaN (refused).  No device is touched.  From the repository root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o sym_pinv_host_check tools/probes/sym_pinv_host_check.cc
//   ./sym_pinv_host_check
#include "../../dune-ddm_amd/csrc/dense_host.hpp"

#include <cstdio>
#include <limits>
#include <random>

namespace {
using Mat = std::vector<double>;
Mat mul(int m, const Mat &A, const Mat &B)
{
  Mat C((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i)
    for (int k = 0; k < m; ++k)
      for (int j = 0; j < m; ++j) C[(size_t)i * m + j] += A[(size_t)i * m + k] * B[(size_t)k * m + j];
  return C;
}
Mat spd(int m, unsigned seed)
{
  std::mt19937_64 g(seed);
  std::normal_distribution<double> N;
  Mat A((size_t)m * m), S((size_t)m * m, 0.0);
  for (double &a : A) a = N(g);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) {
      for (int k = 0; k < m; ++k) S[(size_t)i * m + j] += A[(size_t)i * m + k] * A[(size_t)j * m + k];
      if (i == j) S[(size_t)i * m + j] += m;
    }
  return S;
}
// largest |E_ij| / (d_i d_j) with d the Jacobi scale of W (for W+ the scale is inverted): the metric the pseudo-inverse works in
double scaled_dev(int m, const Mat &A, const Mat &B, const Mat &W, bool inverse)
{
  double worst = 0.0;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) {
      double di = std::sqrt(std::fabs(W[(size_t)i * m + i])), dj = std::sqrt(std::fabs(W[(size_t)j * m + j]));
      if (di == 0.0) di = 1.0;
      if (dj == 0.0) dj = 1.0;
      const double s = inverse ? 1.0 / (di * dj) : di * dj;
      worst = std::max(worst, std::fabs(A[(size_t)i * m + j] - B[(size_t)i * m + j]) / s);
    }
  return worst;
}
int check(const char *name, int m, const Mat &W, int want_rank)
{
  Mat P((size_t)m * m, std::numeric_limits<double>::quiet_NaN());
  int rank = -1;
  if (!dense::sym_pinv(m, W.data(), 1e-12, P.data(), &rank)) {
    std::printf("%s: refused\n", name);
    return 1;
  }
  const double e1 = scaled_dev(m, mul(m, mul(m, W, P), W), W, W, false), e2 = scaled_dev(m, mul(m, mul(m, P, W), P), P, W, true);
  std::printf("%s: m %d rank %d (want %d), |W W+ W - W| %.2e, |W+ W W+ - W+| %.2e (Jacobi-scaled)\n", name, m, rank, want_rank, e1, e2);
  return rank == want_rank && e1 <= 1e-14 * m && e2 <= 1e-14 * m ? 0 : 1;
}
} // namespace

int main()
{
  int bad = 0;
  const int m = 8;
  const Mat S = spd(m, 11);
  bad += check("spd", m, S, 8);
  Mat dup = S;
  for (int j = 0; j < m; ++j) dup[5 * m + j] = dup[2 * m + j];
  for (int i = 0; i < m; ++i) dup[i * m + 5] = dup[i * m + 2];
  dup[5 * m + 5] = dup[2 * m + 2];
  bad += check("duplicate", m, dup, 7);
  Mat zero = S;
  for (int j = 0; j < m; ++j) zero[3 * m + j] = zero[j * m + 3] = 0.0;
  bad += check("zero row", m, zero, 7);
  Mat spread = S;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) spread[i * m + j] *= std::pow(10.0, -10.0 * (7 - i) / 7.0) * std::pow(10.0, -10.0 * (7 - j) / 7.0);
  bad += check("spread", m, spread, 8);
  bad += check("m1", 1, Mat{3.5}, 1);
  bad += check("m32", 32, spd(32, 12), 32);
  bad += check("all zero", 4, Mat(16, 0.0), 0);
  Mat nan = S;
  nan[1 * m + 2] = std::numeric_limits<double>::quiet_NaN();
  Mat P((size_t)m * m);
  int rank = -1;
  const bool refused = !dense::sym_pinv(m, nan.data(), 1e-12, P.data(), &rank);
  std::printf("NaN entry: %s\n", refused ? "refused" : "ACCEPTED");
  bad += refused ? 0 : 1;
  std::printf(bad ? "FAILED %d\n" : "sym_pinv_host_check ok\n", bad);
  return bad ? 1 : 0;
}
