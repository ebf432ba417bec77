// Host check of the x windows of the diagonal-row-block layout under the sanitizers: dia_build and dia_apply_host (csr.hpp) on a
// symmetric 27-point box of 40 x 9 x 3 (three runs, half storage, a last block of 56 rows), on offsets whose windows exactly fill
// DIA_WIN and the same plus one far diagonal (unstaged), and on n = 1 and n = 63 (windows clamped at both ends), each against the
// CSR row sum, bit for bit.  No device is touched.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -o dia_window_host_check tools/probes/dia_window_host_check.hip -lpthread -ldl
//   ./dia_window_host_check
#include "../../dune-ddm_amd/csrc/ddm_hip.hip"

#include <functional>
#include <random>

namespace {
struct Csr {
  int64_t n = 0;
  std::vector<int64_t> rp;
  std::vector<int32_t> ci;
  std::vector<double> va;
};
// rows with one entry at each of the ascending offsets where the column exists; symmetric: a(r, c) = a(c, r) bit for bit
Csr from_offsets(int64_t n, const std::vector<int64_t> &off, bool symmetric, unsigned seed, const std::function<bool(int64_t, int64_t)> &has)
{
  Csr M;
  M.n = n;
  M.rp.push_back(0);
  for (int64_t r = 0; r < n; ++r) {
    for (int64_t o : off) {
      const int64_t c = r + o;
      if (c < 0 || c >= n || !has(r, c)) continue;
      std::mt19937_64 g(seed + (uint64_t)(symmetric ? std::min(r, c) * n + std::max(r, c) : r * n + c));
      M.ci.push_back((int32_t)c);
      M.va.push_back(std::normal_distribution<double>()(g));
    }
    M.rp.push_back((int64_t)M.ci.size());
  }
  return M;
}
int check(const char *name, const Csr &M, bool want_staged, size_t want_runs, int want_window)
{
  std::vector<double> x((size_t)M.n), y((size_t)M.n), ref((size_t)M.n);
  std::mt19937_64 g(7);
  for (double &v : x) v = std::normal_distribution<double>()(g);
  for (int64_t r = 0; r < M.n; ++r) {
    double s = 0.0;
    for (int64_t z = M.rp[(size_t)r]; z < M.rp[(size_t)r + 1]; ++z) s += M.va[(size_t)z] * x[(size_t)M.ci[(size_t)z]];
    ref[(size_t)r] = s;
  }
  int bad = 0;
  for (bool stage : {true, false}) {
    DiaLayout L;
    dia_build(M.n, M.rp.data(), M.ci.data(), M.va.data(), L, stage);
    dia_apply_host(L, M.n, M.rp.data(), M.ci.data(), M.va.data(), x.data(), y.data());
    const bool same = !std::memcmp(y.data(), ref.data(), sizeof(double) * y.size());
    const bool shape = L.win.size() == 1 && L.win[0].staged == (stage && want_staged) && L.win[0].runs.size() == want_runs && L.win[0].window == want_window;
    std::printf("%-18s stage_x=%d  blocks %zu  segments %zu  runs %zu  window %d  staged %d  bit-equal %d\n", name, (int)stage, L.blk.size(), L.win.size(),
                L.win.empty() ? (size_t)0 : L.win[0].runs.size(), L.win.empty() ? 0 : L.win[0].window, L.win.empty() ? 0 : (int)L.win[0].staged, (int)same);
    bad += !same || !shape;
  }
  return bad;
}
} // namespace

int main()
{
  int bad = 0;
  const auto all = [](int64_t, int64_t) { return true; };
  {
    const int64_t nx = 40, ny = 9, nz = 3;
    std::vector<int64_t> off;
    for (int64_t dz = -1; dz <= 1; ++dz)
      for (int64_t dy = -1; dy <= 1; ++dy)
        for (int64_t dx = -1; dx <= 1; ++dx) off.push_back(dz * nx * ny + dy * nx + dx);
    const auto in_box = [&](int64_t r, int64_t c) {
      const int64_t rx = r % nx, ry = r / nx % ny, rz = r / (nx * ny), cx = c % nx, cy = c / nx % ny, cz = c / (nx * ny);
      return std::abs(rx - cx) <= 1 && std::abs(ry - cy) <= 1 && std::abs(rz - cz) <= 1;
    };
    bad += check("box 40 x 9 x 3", from_offsets(nx * ny * nz, off, true, 1, in_box), true, 3, 3 * (WG + 82));
  }
  {
    std::vector<int64_t> off = {0, WG};
    for (int j = 0; j < DIA_WIN / WG - 2; ++j) off.push_back(off.back() + 2 * WG + 88);
    bad += check("fills the capacity", from_offsets(10000, off, false, 2, all), true, (size_t)(DIA_WIN / WG - 1), DIA_WIN);
    off.push_back(off.back() + 3 * WG);
    bad += check("one past capacity", from_offsets(10000, off, false, 3, all), false, (size_t)(DIA_WIN / WG), DIA_WIN + WG);
  }
  bad += check("n = 1", from_offsets(1, {0}, false, 4, all), true, 1, WG);
  bad += check("n = 63", from_offsets(63, {-3, -2, -1, 0, 1, 2, 3}, false, 5, all), true, 1, WG + 6);
  std::printf(bad ? "FAILED: %d\n" : "all equal\n", bad);
  return bad ? 1 : 0;
}
