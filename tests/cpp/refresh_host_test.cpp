// Host-only test harness of the pipe engine's value refresh (dune-ddm_amd/csrc/trsv_pipe_host.hpp: pipe::refresh_values, the host
// twin of the device scatter k_pipe_scatter): a tile stream built from one factor and refreshed with another against the stream
// built from the other.  Test infrastructure; compiled by tests/test_refresh_cpu.py with the flags of libpipe_host_test.so.
#include "trsv_pipe_host.hpp"
#include <cstdio>

// Builds the schedule of lu1 and of lu2 (same pattern, the device's default options unless given), refreshes the first stream with
// lu2 and emulates the solve of d on it into x.  out[0] stream bytes, out[1] bytes in which the two streams differ BEFORE the
// refresh, out[2] the same AFTER it, out[3] whether every other array of the two schedules (tasks, koff, rowL, posU, slot words) is
// the same.  Returns 0, 1 when the builder declines the matrix (err: its reason, the same for both factors or "verdicts differ"),
// 2 when the emulation finds a violation.
extern "C" int refresh_test_case(int64_t n, const int64_t *rp, const int32_t *ci, const double *lu1, const double *lu2, const int64_t *diag, int nblocks,
                                 const int64_t *block_ptr, int delta, int max_span, int vote, int pack_steps, const double *d, double *x, int64_t *out, char *err,
                                 int errlen)
{
  pipe::Options opt;
  opt.delta = delta;
  opt.max_span = max_span;
  opt.vote = vote;
  opt.pack_steps = pack_steps;
  pipe::Schedule S1, S2;
  const bool ok1 = pipe::build(n, rp, ci, lu1, diag, nblocks, block_ptr, opt, S1);
  const bool ok2 = pipe::build(n, rp, ci, lu2, diag, nblocks, block_ptr, opt, S2);
  for (int k = 0; k < 4; ++k) out[k] = 0;
  if (!ok1 || !ok2) {
    std::snprintf(err, errlen, "%s", ok1 != ok2 || S1.error != S2.error ? "verdicts differ" : S1.error.c_str());
    return 1;
  }
  auto differing = [&]() {
    if (S1.stream.size() != S2.stream.size()) return (int64_t)-1;
    int64_t c = 0;
    for (size_t k = 0; k < S1.stream.size(); ++k) c += S1.stream[k] != S2.stream[k];
    return c;
  };
  out[0] = (int64_t)S1.stream.size();
  out[1] = differing();
  pipe::refresh_values(S1.stream.data(), S1.slot[0].data(), S1.slot[1].data(), n, rp, diag, lu2);
  out[2] = differing();
  out[3] = S1.tasks.size() == S2.tasks.size() && (S1.tasks.empty() || !std::memcmp(S1.tasks.data(), S2.tasks.data(), sizeof(pipe::Task) * S1.tasks.size())) &&
           S1.koff == S2.koff && S1.rowL == S2.rowL && S1.posU == S2.posU && S1.slot[0] == S2.slot[0] && S1.slot[1] == S2.slot[1];
  const std::string e = pipe::emulate(S1, n, d, x);
  if (!e.empty()) {
    std::snprintf(err, errlen, "%s", e.c_str());
    return 2;
  }
  return 0;
}
