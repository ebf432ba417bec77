// Host check of the coded blocks of the diagonal-row-block layout under the sanitizers: dia_build and dia_apply_host (csr.hpp) on
// a 27-point box of 12 x 11 x 10 whose values come from a pool of 5 (every block coded, no slabs, a last block of 40 rows), and on
// the same pattern with 16 values in the first block and 17 in the second (one coded with a full dictionary, one not, the segment
// keeps its slabs), each against the CSR row sum, bit for bit, coded and with the codes switched off, on 1 and on 5 host threads.
// No device is touched.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -o dia_code_host_check tools/probes/dia_code_host_check.hip -lpthread -ldl
//   ./dia_code_host_check
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
// 27-point box, x fastest, truncated at the faces; value(row, generator) gives the entries of a row one after the other
Csr stencil_box(int64_t nx, int64_t ny, int64_t nz, const std::function<double(int64_t, std::mt19937_64 &)> &value)
{
  Csr M;
  M.n = nx * ny * nz;
  M.rp.push_back(0);
  std::mt19937_64 g(11);
  for (int64_t r = 0; r < M.n; ++r) {
    const int64_t x = r % nx, y = r / nx % ny, z = r / (nx * ny);
    for (int64_t dz = -1; dz <= 1; ++dz)
      for (int64_t dy = -1; dy <= 1; ++dy)
        for (int64_t dx = -1; dx <= 1; ++dx) {
          if (x + dx < 0 || x + dx >= nx || y + dy < 0 || y + dy >= ny || z + dz < 0 || z + dz >= nz) continue;
          M.ci.push_back((int32_t)(r + dz * nx * ny + dy * nx + dx));
          M.va.push_back(value(r, g));
        }
    M.rp.push_back((int64_t)M.ci.size());
  }
  return M;
}
int check(const char *name, const Csr &M, const std::vector<int> &want_entries, bool want_slabs)
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
  hvec<uint32_t> code1;
  hvec<double> dict1;
  for (bool code : {true, false})
    for (unsigned threads : {1u, 5u}) {
      DiaLayout L;
      dia_build(M.n, M.rp.data(), M.ci.data(), M.va.data(), L, true, code, threads);
      dia_apply_host(L, M.n, M.rp.data(), M.ci.data(), M.va.data(), x.data(), y.data());
      const bool same = !std::memcmp(y.data(), ref.data(), sizeof(double) * y.size());
      bool shape = L.blk.size() == want_entries.size();
      for (size_t b = 0; shape && b < L.blk.size(); ++b)
        shape = L.ndict[b] == (code ? want_entries[b] : 0) && (L.blk[b].dict >= 0) == (L.ndict[b] > 0) && L.slabs[b] == (code ? want_slabs : true);
      shape = shape && (L.val.empty() == (code && !want_slabs)) && L.dict.size() == (size_t)L.ncoded * DIA_DICT && L.code.size() == (L.ncoded ? (size_t)M.n * DIA_CODE_WORDS : 0);
      if (code && threads == 1) code1 = L.code, dict1 = L.dict;
      const bool threads_agree = !code || (code1 == L.code && dict1.size() == L.dict.size() && !std::memcmp(dict1.data(), L.dict.data(), sizeof(double) * dict1.size()));
      std::printf("%-22s code=%d threads=%u  blocks %zu  coded %lld  slab slots %zu  bit-equal %d  as expected %d  threads agree %d\n", name, (int)code, threads,
                  L.blk.size(), (long long)L.ncoded, L.val.size(), (int)same, (int)shape, (int)threads_agree);
      bad += !same || !shape || !threads_agree;
    }
  return bad;
}
} // namespace

int main()
{
  int bad = 0;
  const double pool[17] = {32.0, 0.0, -2.0, -1.0, 1.0, -0.0, 0.375, 0.75, 1.125, 1.5, 1.875, 2.25, 2.625, 3.0, 3.375, 3.75, 4.125};
  // five values drawn at random: every block (the last has 40 rows of 8 to 18 entries) sees them all
  bad += check("five values", stencil_box(12, 11, 10, [&](int64_t, std::mt19937_64 &g) { return pool[g() % 5]; }), {5, 5, 5, 5, 5, 5}, false);
  // rows [0, 256): 16 values, rows [256, 512): 17, the rest 3; a row's first entries walk through its pool, so every value occurs
  int64_t at = 0;
  bad += check("16 and 17 values", stencil_box(12, 11, 10, [&](int64_t r, std::mt19937_64 &) { return pool[at++ % (r < 256 ? 16 : r < 512 ? 17 : 3)]; }), {16, 0, 3, 3, 3, 3}, true);
  std::printf(bad ? "FAILED: %d\n" : "all equal\n", bad);
  return bad ? 1 : 0;
}
