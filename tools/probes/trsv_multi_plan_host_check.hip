// Host check of the plan of the single-launch block solve under the sanitizers: ddm_trsv_multi_plan_host (engine_multi_xcd.hpp over
// trsv_multi_plan.hpp: tri_levels, plan_tables) on block-diagonal patterns with uneven blocks (a one-row block, a chain, random bands),
// both triangles, against a per-block recomputation; malformed patterns are refused; team_of over even and uneven tickets: the ranks
// of every team are a permutation.  No device is touched.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -o trsv_multi_plan_host_check tools/probes/trsv_multi_plan_host_check.hip -lpthread -ldl
//   ./trsv_multi_plan_host_check
#include "../../dune-ddm_amd/csrc/ddm_hip.hip"

#include <random>
#include <set>

namespace {
struct Pattern {
  int64_t n = 0;
  std::vector<int64_t> rp, bp;
  std::vector<int32_t> ci;
};
// symmetric pattern, full diagonal; block b of sizes[b] rows: a chain (kind 0) or a random band of half-width 7 (kind 1)
Pattern make(const std::vector<int> &sizes, const std::vector<int> &kinds, unsigned seed)
{
  Pattern P;
  std::mt19937 g(seed);
  P.bp.push_back(0);
  for (int s : sizes) P.bp.push_back(P.bp.back() + s);
  P.n = P.bp.back();
  std::vector<std::set<int32_t>> row((size_t)P.n);
  for (size_t b = 0; b < sizes.size(); ++b)
    for (int64_t i = P.bp[b]; i < P.bp[b + 1]; ++i) {
      row[(size_t)i].insert((int32_t)i);
      for (int64_t j = std::max(P.bp[b], i - 7); j < i; ++j)
        if (kinds[b] == 0 ? j == i - 1 : g() % 3 == 0) {
          row[(size_t)i].insert((int32_t)j);
          row[(size_t)j].insert((int32_t)i);
        }
    }
  P.rp.push_back(0);
  for (const auto &r : row) {
    P.ci.insert(P.ci.end(), r.begin(), r.end());
    P.rp.push_back((int64_t)P.ci.size());
  }
  return P;
}
int check_plan(const char *name, const Pattern &P)
{
  int bad = 0;
  const int64_t nb = (int64_t)P.bp.size() - 1;
  for (int upper = 0; upper < 2; ++upper) {
    int64_t nlev = -1;
    if (ddm_trsv_multi_plan_host(P.n, P.rp.data(), P.ci.data(), nb, P.bp.data(), upper, nullptr, 0, nullptr, &nlev) != DDM_OK) return 1;
    std::vector<int32_t> off((size_t)(nlev * (nb + 1))), bn((size_t)nb);
    if (ddm_trsv_multi_plan_host(P.n, P.rp.data(), P.ci.data(), nb, P.bp.data(), upper, off.data(), (int64_t)off.size() - 1, bn.data(), &nlev) != DDM_EINVAL) ++bad; // short
    if (ddm_trsv_multi_plan_host(P.n, P.rp.data(), P.ci.data(), nb, P.bp.data(), upper, off.data(), (int64_t)off.size(), bn.data(), &nlev) != DDM_OK) return 1;
    // per block: levels by the definition, rows per level
    std::vector<int> lev((size_t)P.n, 0);
    for (int64_t b = 0; b < nb; ++b) {
      int top = -1;
      std::vector<int> cnt((size_t)nlev, 0);
      for (int64_t q = P.bp[(size_t)b]; q < P.bp[(size_t)b + 1]; ++q) {
        const int64_t i = upper ? P.bp[(size_t)b] + P.bp[(size_t)b + 1] - 1 - q : q;
        int l = 0;
        for (int64_t k = P.rp[(size_t)i]; k < P.rp[(size_t)i + 1]; ++k)
          if (upper ? P.ci[(size_t)k] > i : P.ci[(size_t)k] < i) l = std::max(l, lev[(size_t)P.ci[(size_t)k]] + 1);
        lev[(size_t)i] = l;
        top = std::max(top, l);
        if (l < nlev) cnt[(size_t)l]++;
        else ++bad;
      }
      if (bn[(size_t)b] != top + 1) ++bad;
      for (int64_t l = 0; l < nlev; ++l)
        if (off[(size_t)(l * (nb + 1) + b + 1)] - off[(size_t)(l * (nb + 1) + b)] != cnt[(size_t)l]) ++bad;
    }
    int64_t total = 0;
    for (int64_t l = 0; l < nlev; ++l) {
      if (off[(size_t)(l * (nb + 1))] != 0) ++bad;
      total += off[(size_t)(l * (nb + 1) + nb)];
    }
    if (total != P.n) ++bad;
  }
  std::printf("%-10s n = %lld, %lld blocks: %s\n", name, (long long)P.n, (long long)nb, bad ? "FAILED" : "ok");
  return bad;
}
int check_refusals()
{
  Pattern P = make({5, 1, 9}, {1, 1, 0}, 3);
  int64_t nlev = 0;
  int bad = 0;
  auto call = [&](const Pattern &Q) { return ddm_trsv_multi_plan_host(Q.n, Q.rp.data(), Q.ci.data(), (int64_t)Q.bp.size() - 1, Q.bp.data(), 0, nullptr, 0, nullptr, &nlev); };
  Pattern Q = P;
  std::swap(Q.ci[(size_t)Q.rp[8]], Q.ci[(size_t)Q.rp[8] + 1]); // unsorted row
  bad += call(Q) != DDM_EINVAL;
  Q = P;
  Q.ci[(size_t)Q.rp[6]] = (int32_t)Q.n; // column out of range (the one-row block's diagonal)
  bad += call(Q) != DDM_EINVAL;
  Q = P;
  Q.bp[1] = 7, Q.bp[2] = 6; // decreasing block pointer
  bad += call(Q) != DDM_EINVAL;
  Q = P;
  Q.bp.back() -= 1; // does not cover the matrix
  bad += call(Q) != DDM_EINVAL;
  bad += ddm_trsv_multi_plan_host(P.n, nullptr, P.ci.data(), 3, P.bp.data(), 0, nullptr, 0, nullptr, &nlev) != DDM_EINVAL;
  bad += call(P) != DDM_OK;
  std::printf("refusals: %s\n", bad ? "FAILED" : "ok");
  return bad;
}
int check_teams()
{
  int bad = 0;
  const std::vector<std::vector<unsigned>> tickets = {{32, 32, 32, 32, 32, 32, 32, 32}, {31, 33, 32, 30, 34, 32, 32, 32}, {8, 0, 8, 8, 8, 8, 8, 8}, {1, 1, 1, 1, 1, 1, 1, 1}};
  for (const auto &tk : tickets)
    for (int nb = 1; nb <= 17; ++nb)
      for (int force = 0; force < 2; ++force) {
        unsigned grid = 0;
        for (unsigned t : tk) grid += t;
        std::vector<std::set<int>> seen(8);
        std::vector<int> size(8, -1);
        unsigned gt = 0;
        int nteams = -1;
        for (unsigned x = 0; x < 8; ++x)
          for (unsigned t = 0; t < tk[x]; ++t, ++gt) {
            int32_t o[5];
            if (ddm_trsv_multi_team_host(tk.data(), nb, force, (int)x, t, gt, grid, o) != DDM_OK) return 1;
            if (nteams < 0) nteams = o[0];
            if (o[0] != nteams || o[1] < 0 || o[1] >= o[0] || o[2] < 0 || o[2] >= o[3]) { ++bad; continue; }
            if (size[(size_t)o[1]] < 0) size[(size_t)o[1]] = o[3];
            if (size[(size_t)o[1]] != o[3] || !seen[(size_t)o[1]].insert(o[2]).second) ++bad;
          }
        int sum = 0;
        for (int t = 0; t < nteams; ++t) {
          if ((int)seen[(size_t)t].size() != size[(size_t)t]) ++bad;
          sum += size[(size_t)t];
        }
        if (sum != (int)grid) ++bad;
      }
  std::printf("teams: %s\n", bad ? "FAILED" : "ok");
  return bad;
}
} // namespace

int main()
{
  int bad = 0;
  bad += check_plan("uneven", make({40, 1, 300, 7, 64, 65, 129, 2, 90}, {1, 1, 0, 0, 1, 1, 1, 0, 1}, 1));
  bad += check_plan("one block", make({257}, {1}, 2));
  bad += check_plan("one row", make({1}, {0}, 3));
  bad += check_plan("chains", make({30, 30, 5}, {0, 0, 0}, 4));
  bad += check_refusals();
  bad += check_teams();
  std::printf(bad ? "FAILED\n" : "all checks passed\n");
  return bad ? 1 : 0;
}
