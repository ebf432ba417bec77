// Host-only test harness of the "pipe" triangular-solve schedule builder (dune-ddm_amd/csrc/trsv_pipe_host.hpp):
// builds the schedule for given ILU(0) factors and runs the CPU emulation of the device data flow.
// Test infrastructure; the product library compiles the same header into libddm_hip.so.
#include "trsv_pipe_host.hpp"
#include <cstdio>
#include <cstdlib>

namespace {

const unsigned char *tile_of(const pipe::Schedule &S, const pipe::Task &T, int t)
{
  return S.stream.data() + T.tile_off + (int64_t)S.koff[(size_t)T.koff_base + t] * 1024;
}
int width_class(int w) { return w <= pipe::MIN_W ? 0 : (w <= pipe::MIN_W + 6 ? 1 : 2); } // <= 14 | 15..20 | 21..26: the kernel's register chunk and its two wide halves
int slot_class(int u) { return u < pipe::MIN_W ? 0 : (u < pipe::MIN_W + 6 ? 1 : 2); }

// what an operand word is: 0 ring, 1 self-global (a position of the task itself), 2 remote (a position of another task), 3 padding
struct Operand {
  int kind;
  int64_t pos; // position in the sweep's result array the operand stands for (ring operands: the step that wrote the ring row last)
};
Operand decode(const pipe::Task &T, int t, int32_t op)
{
  if (op == pipe::PAD_OP) return {3, -1};
  if (op < pipe::RING_Z) {
    const int row = op / (pipe::LANES * 8), lane = (op / 8) % pipe::LANES;
    int back = (t % pipe::RING) - row;
    if (back <= 0) back += pipe::RING;
    return {0, T.pos_base + (int64_t)(t - back) * pipe::LANES + lane};
  }
  const int64_t pos = op / 8;
  const bool self = pos >= T.pos_base && pos < T.pos_base + (int64_t)T.nsteps * pipe::LANES;
  return {self ? 1 : 2, pos};
}

} // namespace

// Stats slots of pipe_test_case behind the 20 of pipe_test_build_and_emulate (tests/pipe_cases.py names them):
//   20 + 3 sweep + c            steps of width class c (<= 14, 15..20, 21..26)
//   26 + 12 sweep + 4 s + k     operand words of slot class s (entries 0..13, 14..19, 20..25) and kind k (ring, self-global, remote,
//                               padding) over all 64 lanes of every tile, slots below the tile's W only
//   50, 51                      fewest / most steps of a task
//   52                          packed tasks (no operand at all: dependency-free rows only)
//   53                          rows that start a further chain in a lane an earlier chain of the task has used (no operand from the
//                               lane's previous step): lane re-use
//   54, 55, 56                  tasks of 1, 2, 3 steps
//   57                          int32 words written to `widths` (or needed, when the capacity was too small)
//   58 .. 63                    the mutation: natural row, task, step, lane, entry slot, operand kind (-1: none was asked for or found)
// widths: per task sweep, group, nsteps, nprod, then the width (header word [2]) of every step.
// mutate (or null): {sweep, slot class, operand kind or -1 for any}: before the emulation the factor value of the first entry of
// that class in queue order is set to zero -- an active lane, no padding operand, and a non-zero operand value in the sequential
// solve of d (computed here from lu).  The emulated kernel then drops that operand, as a device kernel would that skips a wide
// half, reads a zeroed ring slot or misses a producer's result.
extern "C" int pipe_test_case(int64_t n, const int64_t *rp, const int32_t *ci, const double *lu, const int64_t *diag, int nblocks,
                              const int64_t *block_ptr, int delta, int max_span, int vote, int pack_steps, const double *d, double *x,
                              int64_t *stats, int32_t *widths, int64_t widths_cap, const int64_t *mutate, char *err, int errlen)
{
  pipe::Options opt;
  opt.delta = delta;
  opt.max_span = max_span;
  opt.vote = vote;
  opt.pack_steps = pack_steps;
  pipe::Schedule S;
  for (int k = 0; k < 64; ++k) stats[k] = 0;
  for (int k = 58; k < 64; ++k) stats[k] = -1;
  if (!pipe::build(n, rp, ci, lu, diag, nblocks, block_ptr, opt, S)) {
    std::snprintf(err, errlen, "%s", S.error.c_str());
    return 1;
  }
  const pipe::Stats &st = S.stats;
  const int64_t v[20] = {st.ntasks[0], st.ntasks[1], st.nsteps[0], st.nsteps[1], st.rows, st.entries, st.entries_local, st.entries_self_global,
                         st.entries_remote, st.max_prod, st.max_steps, st.regrouped, st.nchains[0], st.nchains[1], S.geo.W, S.geo.tile_bytes,
                         (int64_t)S.stream.size(), S.nposL, S.nposU, (int64_t)S.tasks.size()};
  for (int k = 0; k < 20; ++k) stats[k] = v[k];
  // the sequential solve, for the mutation's "operand is not zero": y by natural row, x by natural row
  std::vector<double> ys, xs;
  std::vector<int32_t> rowU;
  if (mutate) {
    ys.assign((size_t)n, 0.0);
    xs.assign((size_t)n, 0.0);
    for (int64_t i = 0; i < n; ++i) {
      double s = d[i];
      for (int64_t k = rp[i]; k < diag[i]; ++k) s -= lu[k] * ys[(size_t)ci[k]];
      ys[(size_t)i] = s;
    }
    for (int64_t i = n - 1; i >= 0; --i) {
      double s = ys[(size_t)i];
      for (int64_t k = diag[i] + 1; k < rp[i + 1]; ++k) s -= lu[k] * xs[(size_t)ci[k]];
      xs[(size_t)i] = s * lu[diag[i]];
    }
    rowU.assign((size_t)S.nposU, -1);
    for (int64_t i = 0; i < n; ++i) rowU[(size_t)S.posU[(size_t)i]] = (int32_t)i;
  }
  auto row_at = [&](int sweep, int64_t pos) { return sweep ? rowU[(size_t)pos] : S.rowL[(size_t)pos]; };
  int64_t nw = 0, min_steps = -1, max_steps = 0;
  bool mutated = false;
  for (size_t q = 0; q < S.tasks.size(); ++q) {
    const pipe::Task &T = S.tasks[q];
    min_steps = min_steps < 0 ? T.nsteps : std::min<int64_t>(min_steps, T.nsteps);
    max_steps = std::max<int64_t>(max_steps, T.nsteps);
    if (T.nsteps >= 1 && T.nsteps <= 3) stats[54 + T.nsteps - 1] += 1;
    const int32_t head[4] = {T.sweep, T.group, T.nsteps, T.nprod};
    for (int k = 0; k < 4; ++k, ++nw)
      if (nw < widths_cap) widths[nw] = head[k];
    bool any_operand = false, used[pipe::LANES] = {};
    int64_t reused = 0;
    for (int t = 0; t < T.nsteps; ++t) {
      unsigned char *tile = const_cast<unsigned char *>(tile_of(S, T, t));
      const int32_t *hdr = reinterpret_cast<const int32_t *>(tile);
      const int32_t *own = reinterpret_cast<const int32_t *>(tile + 256);
      const pipe::Geometry G(hdr[2]);
      if (nw < widths_cap) widths[nw] = hdr[2];
      ++nw;
      stats[20 + 3 * T.sweep + width_class(hdr[2])] += 1;
      for (int l = 0; l < pipe::LANES; ++l) {
        const int64_t pos = T.pos_base + (int64_t)t * pipe::LANES + l;
        const bool active = T.sweep ? own[l] != pipe::ZERO_POS * 8 : S.rowL[(size_t)pos] >= 0; // (U: a real row reads its own forward value, never the reserved zero)
        bool from_prev = false;
        for (int u = 0; u < G.W; ++u) {
          const int32_t op = *reinterpret_cast<const int32_t *>(tile + G.idx_off(u, l));
          const Operand o = decode(T, t, op);
          stats[26 + 12 * T.sweep + 4 * slot_class(u) + o.kind] += 1;
          if (o.kind == 3) continue;
          any_operand = true;
          if (t > 0 && op == pipe::ring_op(t - 1, l)) from_prev = true;
          if (mutate && !mutated && active && T.sweep == mutate[0] && slot_class(u) == mutate[1] && (mutate[2] < 0 || o.kind == mutate[2])) {
            const int32_t r = row_at(T.sweep, o.pos);
            double &a = *reinterpret_cast<double *>(tile + G.val_off(u, l));
            if (r >= 0 && (T.sweep ? xs : ys)[(size_t)r] != 0.0 && a != 0.0) {
              a = 0.0;
              mutated = true;
              const int64_t m[6] = {row_at(T.sweep, pos), (int64_t)q, t, l, u, o.kind};
              for (int k = 0; k < 6; ++k) stats[58 + k] = m[k];
            }
          }
        }
        if (active && used[l] && !from_prev) ++reused;
        used[l] = used[l] || active;
      }
    }
    if (!any_operand) stats[52] += 1;
    else stats[53] += reused; // (the rows of a packed task are no chains)
  }
  stats[50] = min_steps < 0 ? 0 : min_steps;
  stats[51] = max_steps;
  stats[57] = nw;
  const std::string e = pipe::emulate(S, n, d, x);
  if (!e.empty()) {
    std::snprintf(err, errlen, "%s", e.c_str());
    return 2;
  }
  return 0;
}

extern "C" int pipe_test_build_and_emulate(int64_t n, const int64_t *rp, const int32_t *ci, const double *lu, const int64_t *diag,
                                           int nblocks, const int64_t *block_ptr, int delta, int vote, const double *d, double *x,
                                           int64_t *stats, char *err, int errlen)
{
  pipe::Options opt;
  opt.delta = delta;
  opt.vote = vote;
  if (const char *e = std::getenv("PIPE_TEST_SPAN")) opt.max_span = std::atoi(e);   // (diagnostic sweeps of the schedule options: tools/pipe_sim.py)
  if (const char *e = std::getenv("PIPE_TEST_PACK")) opt.pack_steps = std::atoi(e);
  pipe::Schedule S;
  if (!pipe::build(n, rp, ci, lu, diag, nblocks, block_ptr, opt, S)) {
    std::snprintf(err, errlen, "%s", S.error.c_str());
    return 1;
  }
  const pipe::Stats &st = S.stats;
  const int64_t v[20] = {st.ntasks[0], st.ntasks[1], st.nsteps[0], st.nsteps[1], st.rows, st.entries, st.entries_local, st.entries_self_global,
                         st.entries_remote, st.max_prod, st.max_steps, st.regrouped, st.nchains[0], st.nchains[1], S.geo.W, S.geo.tile_bytes,
                         (int64_t)S.stream.size(), S.nposL, S.nposU, (int64_t)S.tasks.size()};
  for (int k = 0; k < 20; ++k) stats[k] = v[k];
  if (const char *f = std::getenv("PIPE_DEBUG_TASKS")) { // per task: group sweep W nsteps active-rows nprod
    FILE *fp = std::fopen(f, "w");
    for (const pipe::Task &T : S.tasks) {
      int64_t active = 0, wide = 0, remote_slots = 0;
      for (int t = 0; t < T.nsteps; ++t) {
        const int32_t *hdr = reinterpret_cast<const int32_t *>(S.stream.data() + T.tile_off + (int64_t)S.koff[(size_t)T.koff_base + t] * 1024);
        active += hdr[0];
        wide += hdr[2] > pipe::MIN_W;
        { // slots of the first MIN_W entries that hold a gathered operand in some lane
          const pipe::Geometry G(hdr[2]);
          const unsigned char *tile = reinterpret_cast<const unsigned char *>(hdr);
          for (int u = 0; u < pipe::MIN_W; ++u) {
            bool any = false;
            for (int l = 0; l < pipe::LANES; ++l) any |= *reinterpret_cast<const int32_t *>(tile + G.idx_off(u, l)) > pipe::RING_Z;
            remote_slots += any;
          }
        }
      }
      std::fprintf(fp, "%d %d %d %d %lld %d %lld %d %lld", T.group, T.sweep, T.W, T.nsteps, (long long)active, T.nprod, (long long)wide, T.start_level, (long long)remote_slots);
      if (std::getenv("PIPE_DEBUG_NEEDS")) { // producers with the steps of each that the first / the middle / the last step of the task requires
        for (int j = 0; j < T.nprod; ++j) {
          std::fprintf(fp, " %d", T.prod[j]);
          for (int t : {0, T.nsteps / 2, T.nsteps - 1}) {
            const uint32_t *hdr = reinterpret_cast<const uint32_t *>(S.stream.data() + T.tile_off + (int64_t)S.koff[(size_t)T.koff_base + t] * 1024);
            std::fprintf(fp, ":%u", (hdr[pipe::HDR_REQ0 + j / 2] >> (16 * (j & 1))) & 0xffffu);
          }
        }
      }
      std::fprintf(fp, "\n");
    }
    std::fclose(fp);
    if (const char *nf = std::getenv("PIPE_DEBUG_NEEDS_BIN")) { // per task: nprod, nsteps, producer ids, then per step the steps required of each producer, the step's W and its active rows
      FILE *fb = std::fopen(nf, "wb");
      for (const pipe::Task &T : S.tasks) {
        std::fwrite(&T.nprod, 4, 1, fb);
        std::fwrite(&T.nsteps, 4, 1, fb);
        std::fwrite(T.prod, 4, (size_t)T.nprod, fb);
        for (int t = 0; t < T.nsteps; ++t) {
          const uint32_t *hdr = reinterpret_cast<const uint32_t *>(S.stream.data() + T.tile_off + (int64_t)S.koff[(size_t)T.koff_base + t] * 1024);
          for (int j = 0; j < T.nprod; ++j) {
            const uint16_t rq = (uint16_t)((hdr[pipe::HDR_REQ0 + j / 2] >> (16 * (j & 1))) & 0xffffu);
            std::fwrite(&rq, 2, 1, fb);
          }
          const uint16_t w = (uint16_t)hdr[2], act = (uint16_t)hdr[0]; // widest row and active rows of the step
          std::fwrite(&w, 2, 1, fb);
          std::fwrite(&act, 2, 1, fb);
        }
      }
      std::fclose(fb);
    }
  }
  const std::string e = pipe::emulate(S, n, d, x);
  if (!e.empty()) {
    std::snprintf(err, errlen, "%s", e.c_str());
    return 2;
  }
  return 0;
}
