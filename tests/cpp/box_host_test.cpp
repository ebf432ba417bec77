// Host-only test harness of the "box" triangular-solve schedule builder (dune-ddm_amd/csrc/trsv_box_host.hpp): builds the streams and
// the shell system for given ILU(0) factors and runs the CPU walk of the device data flow (the nested shell solver is a sequential
// solve here).  Test infrastructure; the product library compiles the same header into libddm_hip.so.
#include "trsv_box_host.hpp"
#include <cstdio>

// the nested solver of the CPU walks: sequential solve with the shell's own factor, ascending columns
static auto sequential_shell_solve(const box::Schedule &S)
{
  return [&S](const double *ds, double *xs) {
    const int64_t ns = (int64_t)S.srow.size();
    for (int64_t t = 0; t < ns; ++t) {
      double s = ds[t];
      for (int64_t p = S.frp[(size_t)t]; p < S.fdiag[(size_t)t]; ++p) {
        const double prod = S.fva[(size_t)p] * xs[S.fci[(size_t)p]];
        s -= prod;
      }
      xs[t] = s;
    }
    for (int64_t t = ns - 1; t >= 0; --t) {
      double s = xs[t];
      for (int64_t p = S.fdiag[(size_t)t] + 1; p < S.frp[(size_t)t + 1]; ++p) {
        const double prod = S.fva[(size_t)p] * xs[S.fci[(size_t)p]];
        s -= prod;
      }
      xs[t] = s * S.fva[(size_t)S.fdiag[(size_t)t]];
    }
  };
}

extern "C" int box_test_build_and_emulate(int64_t n, const int64_t *rp, const int32_t *ci, const double *lu, const int64_t *diag, int nblocks,
                                          const int64_t *block_ptr, const double *d, double *x, int64_t *stats, char *err, int errlen)
{
  box::Schedule S;
  if (!box::build(n, rp, ci, lu, diag, nblocks, block_ptr, S)) {
    std::snprintf(err, errlen, "%s", S.error.c_str());
    return 1;
  }
  const box::Block &B0 = S.blocks[0];
  const int64_t v[10] = {S.stats.box_rows, S.stats.shell_rows, S.stats.stream_bytes, S.stats.ext_products, S.stats.shell_lower_entries,
                         B0.nx, B0.ny, B0.nz, B0.nsteps, (int64_t)S.fci.size()};
  for (int k = 0; k < 10; ++k) stats[k] = v[k];
  auto shell_solve = sequential_shell_solve(S);
  std::vector<double> y1((size_t)n, 0.0), y2((size_t)n, 0.0);
  const std::string e = box::emulate(S, n, d, x, shell_solve, y1.data());
  if (!e.empty()) {
    std::snprintf(err, errlen, "%s", e.c_str());
    return 2;
  }
  // the lane-by-lane walk (the kernel's index arithmetic) must give the same bits
  std::vector<double> x2((size_t)n, 0.0);
  box::emulate_lanes(S, n, d, x2.data(), shell_solve, y2.data());
  for (int64_t r = 0; r < n; ++r)
    if (std::memcmp(&y2[(size_t)r], &y1[(size_t)r], 8) != 0) {
      std::snprintf(err, errlen, "lane-by-lane walk: forward sweep differs at row %lld (%.17g vs %.17g)", (long long)r, y2[(size_t)r], y1[(size_t)r]);
      return 3;
    }
  for (int64_t r = 0; r < n; ++r)
    if (std::memcmp(&x2[(size_t)r], &x[r], 8) != 0) {
      std::snprintf(err, errlen, "lane-by-lane walk differs from the row walk at row %lld (%.17g vs %.17g)", (long long)r, x2[(size_t)r], x[r]);
      return 3;
    }
  return 0;
}

// The case harness of tests/box_cases.py: box::build on the given factor, per block what the builder made of it, and the CPU walks of the
// device data flow into x (which the caller fills with NaN).
//   stats[0..7]  = box rows, shell rows, stream bytes, product slots, shell-box lower entries, entries of the nested factor, blocks,
//                  widest triangle row of the nested factor (strict lower or strict upper entries of one shell row)
//   stats[8..14] = the mutation that was made: row, block, plane K, step l, lane, value slot (0 .. 13, or the row's product index), 1 if a
//                  product; row = -1: none found
//   stats[16 + 32 b ..] per block b = nx, ny, nz, steps per plane, shell rows, rows with 0 .. 20 shell entries (21 numbers), planes that
//                  conform on their own and were given back by detect, lines per lane (ceil(ny / 64))
// mutate (may be null) = {sweep, e, Jmin, Jmax}: ZEROES one value before the lane-by-lane walk, which alone then writes x:
//   e = 0 .. 13: stream value e (13 = the stored inverse pivot of the upper stream) of the first row of the sweep's walk whose line J
//                (sweep coordinates) lies in [Jmin, Jmax] and whose value there is not zero;
//   e = -1 / -2: a product of the upper sweep in the slots q < 7 / q >= 7 (product index m, q = m / 2), same choice of the row.
extern "C" int box_test_case(int64_t n, const int64_t *rp, const int32_t *ci, const double *lu, const int64_t *diag, int nblocks, const int64_t *block_ptr,
                             const double *d, double *x, int64_t *stats, int64_t cap, const int64_t *mutate, char *err, int errlen)
{
  box::Schedule S;
  if (!box::build(n, rp, ci, lu, diag, nblocks, block_ptr, S)) {
    std::snprintf(err, errlen, "%s", S.error.c_str());
    return 1;
  }
  if (cap < 16 + 32 * (int64_t)nblocks) return 4;
  int64_t widest = 0;
  for (size_t t = 0; t + 1 < S.frp.size(); ++t) widest = std::max({widest, S.fdiag[t] - S.frp[t], S.frp[t + 1] - S.fdiag[t] - 1});
  const int64_t v[8] = {S.stats.box_rows, S.stats.shell_rows, S.stats.stream_bytes, S.stats.ext_products, S.stats.shell_lower_entries,
                        (int64_t)S.fci.size(), nblocks, widest};
  for (int k = 0; k < 8; ++k) stats[k] = v[k];
  stats[8] = -1;
  for (int b = 0; b < nblocks; ++b) {
    const box::Block &B = S.blocks[(size_t)b];
    int64_t *o = stats + 16 + 32 * (int64_t)b;
    o[0] = B.nx; o[1] = B.ny; o[2] = B.nz; o[3] = B.nsteps; o[4] = B.nloc - B.nb;
    for (int64_t q = 0; q < B.nb; ++q) {
      const int64_t r = B.r0 + q;
      int64_t p = rp[r + 1];
      while (p > diag[r] + 1 && ci[p - 1] >= B.r0 + B.nb) --p;
      const int64_t cnt = rp[r + 1] - p;
      if (cnt > box::MAX_EXT) return 4;
      ++o[5 + cnt];
    }
    int nx, ny, nz, back = 0;
    std::string why;
    if (!box::detect(rp, ci, diag, block_ptr[b], block_ptr[b + 1], nx, ny, nz, why, &back) || nz != B.nz) return 4;
    o[26] = back;
    o[27] = (B.ny + box::LANES - 1) / box::LANES;
  }
  auto shell_solve = sequential_shell_solve(S);
  if (mutate) {
    const int sweep = (int)mutate[0], e = (int)mutate[1];
    const int64_t Jmin = mutate[2], Jmax = mutate[3];
    if (sweep < 0 || sweep > 1 || e < -2 || e > 13 || (e < 0 && sweep != 1)) return 4;
    bool done = false;
    for (int b = 0; b < nblocks && !done; ++b) {
      const box::Block &B = S.blocks[(size_t)b];
      const box::StepTab *T = S.steps.data() + B.step_off;
      for (int K = 0; K < B.nz && !done; ++K)
        for (int l = 0; l < B.nsteps && !done; ++l)
          for (int a = 0; a < T[l].nact && !done; ++a) {
            const int J = T[l].jlo + a, I = l - 2 * J;
            if (J < Jmin || J > Jmax) continue;
            const int i = sweep ? B.nx - 1 - I : I, j = sweep ? B.ny - 1 - J : J, k = sweep ? B.nz - 1 - K : K;
            const int64_t row = B.r0 + i + (int64_t)B.nx * (j + (int64_t)B.ny * k);
            int64_t slot = e;
            if (e >= 0) {
              double *val = S.stream.data() + B.stream_off[sweep] + (int64_t)K * B.plane_len[sweep] + (int64_t)T[l].off * box::NV +
                            ((int64_t)(e / 2) * T[l].nact + a) * 2 + e % 2;
              if (*val == 0.0) continue;
              *val = 0.0;
            } else {
              const uint64_t info = S.einfo[(size_t)(B.einfo_off + ((int64_t)K * B.nsteps + l) * box::LANES + J % box::LANES)];
              const int64_t e0 = (int64_t)(uint32_t)info, cnt = (int64_t)(info >> 32);
              const int64_t m = e == -1 ? 0 : 14;               // the first product of the class
              if (m >= cnt || (e == -1 && cnt > 14) || S.ext_val[(size_t)(e0 + m)] == 0.0) continue;   // (q < 7: a row that ends there)
              S.ext_val[(size_t)(e0 + m)] = 0.0;
              slot = m;
            }
            const int64_t w[7] = {row, b, K, l, J % box::LANES, slot, e < 0};
            for (int q = 0; q < 7; ++q) stats[8 + q] = w[q];
            done = true;
          }
    }
    if (!done) {
      std::snprintf(err, errlen, "no value of that kind in the schedule");
      return 5;
    }
    box::emulate_lanes(S, n, d, x, shell_solve);
    return 0;
  }
  std::vector<double> y1((size_t)n, 0.0), y2((size_t)n, 0.0), x2((size_t)n, 0.0);
  for (int64_t r = 0; r < n; ++r) x2[(size_t)r] = x[r];   // (both walks start from the caller's fill)
  const std::string e = box::emulate(S, n, d, x, shell_solve, y1.data());
  if (!e.empty()) {
    std::snprintf(err, errlen, "%s", e.c_str());
    return 2;
  }
  box::emulate_lanes(S, n, d, x2.data(), shell_solve, y2.data());
  for (int64_t r = 0; r < n; ++r)
    if (std::memcmp(&y2[(size_t)r], &y1[(size_t)r], 8) != 0 || std::memcmp(&x2[(size_t)r], &x[r], 8) != 0) {
      std::snprintf(err, errlen, "lane-by-lane walk differs from the row walk at row %lld (forward %.17g vs %.17g, result %.17g vs %.17g)", (long long)r,
                    y2[(size_t)r], y1[(size_t)r], x2[(size_t)r], x[r]);
      return 3;
    }
  return 0;
}

// the shell's own factor of a schedule (for tests that feed it to the other engines): sizes first (rp == NULL), then the arrays
extern "C" int box_test_shell_system(int64_t n, const int64_t *rp, const int32_t *ci, const double *lu, const int64_t *diag, int nblocks, const int64_t *block_ptr,
                                     int64_t *sizes, int64_t *frp, int32_t *fci, double *fva, int64_t *fdiag, int64_t *fbp)
{
  box::Schedule S;
  if (!box::build(n, rp, ci, lu, diag, nblocks, block_ptr, S)) return 1;
  sizes[0] = (int64_t)S.srow.size();
  sizes[1] = (int64_t)S.fci.size();
  if (!frp) return 0;
  std::copy(S.frp.begin(), S.frp.end(), frp);
  std::copy(S.fci.begin(), S.fci.end(), fci);
  std::copy(S.fva.begin(), S.fva.end(), fva);
  std::copy(S.fdiag.begin(), S.fdiag.end(), fdiag);
  std::copy(S.fblock_ptr.begin(), S.fblock_ptr.end(), fbp);
  return 0;
}
