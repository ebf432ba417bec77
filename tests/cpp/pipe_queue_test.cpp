// Host-only test harness of the pipe schedule's QUEUE ORDER (dune-ddm_amd/csrc/trsv_pipe_host.hpp, "Queue order"): builds the
// schedule with given move_gap / move_max and runs the slot-limited CPU emulation of the device data flow with a given number of
// workgroups per queue.  Test infrastructure; the product library compiles the same header into libddm_hip.so.
#include "trsv_pipe_host.hpp"
#include <cstdio>

// out: [0] [1] tasks moved in the forward / backward sweeps, [2] most in one queue, [3] tasks, [4] tasks that stand in front of one of
//      their producers, [5] those of them that are not flagged as moved, [6] producers outside the task's own queue, [7] stream bytes
// taskinfo (capacity cap tasks): per task group, sweep, start level, moved flag
// slots: workgroups per queue in the emulation (<= 0: the queue's moved tasks + 1)
// returns 0, 1 (the builder declined: err), 2 (the emulation found a violation: err)
extern "C" int pipe_queue_case(int64_t n, const int64_t *rp, const int32_t *ci, const double *lu, const int64_t *diag, int nblocks,
                               const int64_t *block_ptr, int delta, int move_gap, int move_max, int slots, const double *d, double *x,
                               int64_t *out, int32_t *taskinfo, int64_t cap, char *err, int errlen)
{
  pipe::Options opt;
  opt.delta = delta;
  opt.move_gap = move_gap;
  opt.move_max = move_max;
  pipe::Schedule S;
  for (int k = 0; k < 8; ++k) out[k] = 0;
  if (!pipe::build(n, rp, ci, lu, diag, nblocks, block_ptr, opt, S)) {
    std::snprintf(err, errlen, "%s", S.error.c_str());
    return 1;
  }
  out[0] = S.stats.moved[0];
  out[1] = S.stats.moved[1];
  out[2] = S.stats.max_moved;
  out[3] = (int64_t)S.tasks.size();
  out[7] = (int64_t)S.stream.size();
  for (size_t t = 0; t < S.tasks.size(); ++t) {
    const pipe::Task &T = S.tasks[t];
    const pipe::Group &G = S.groups[(size_t)T.group];
    bool behind = false;
    for (int p = 0; p < T.nprod; ++p) {
      if (T.prod[p] > (int32_t)t) behind = true;
      if (T.prod[p] < G.task0[T.sweep] || T.prod[p] >= G.task0[T.sweep] + G.ntask[T.sweep]) out[6] += 1;
    }
    out[4] += behind;
    out[5] += behind && !T.moved;
    if ((int64_t)t < cap) {
      const int32_t v[4] = {T.group, T.sweep, T.start_level, T.moved};
      for (int k = 0; k < 4; ++k) taskinfo[4 * t + k] = v[k];
    }
  }
  const std::string e = pipe::emulate(S, n, d, x, slots);
  if (!e.empty()) {
    std::snprintf(err, errlen, "%s", e.c_str());
    return 2;
  }
  return 0;
}

// The schedule for tools/pipe_sim.py, in the formats of PIPE_DEBUG_TASKS / PIPE_DEBUG_NEEDS_BIN of pipe_host_test.cpp: tasks_txt per
// task "group sweep W nsteps active-rows nprod wide-steps start-level 0 moved"; needs_bin per task nprod, nsteps, producer ids, then per
// step the steps required of each producer, the step's W and its active rows (16 bit each).  out: [0] [1] moved per sweep, [2] tasks.
extern "C" int pipe_queue_dump(int64_t n, const int64_t *rp, const int32_t *ci, const double *lu, const int64_t *diag, int nblocks,
                               const int64_t *block_ptr, int delta, int move_gap, int move_max, const char *tasks_txt, const char *needs_bin,
                               int64_t *out)
{
  pipe::Options opt;
  opt.delta = delta;
  opt.move_gap = move_gap;
  opt.move_max = move_max;
  pipe::Schedule S;
  if (!pipe::build(n, rp, ci, lu, diag, nblocks, block_ptr, opt, S)) return 1;
  out[0] = S.stats.moved[0];
  out[1] = S.stats.moved[1];
  out[2] = (int64_t)S.tasks.size();
  FILE *fp = std::fopen(tasks_txt, "w"), *fb = std::fopen(needs_bin, "wb");
  if (!fp || !fb) return 3;
  for (const pipe::Task &T : S.tasks) {
    int64_t active = 0, wide = 0;
    std::fwrite(&T.nprod, 4, 1, fb);
    std::fwrite(&T.nsteps, 4, 1, fb);
    std::fwrite(T.prod, 4, (size_t)T.nprod, fb);
    for (int t = 0; t < T.nsteps; ++t) {
      const uint32_t *hdr = reinterpret_cast<const uint32_t *>(S.stream.data() + T.tile_off + (int64_t)S.koff[(size_t)T.koff_base + t] * 1024);
      active += hdr[0];
      wide += (int)hdr[2] > pipe::MIN_W;
      for (int j = 0; j < T.nprod; ++j) {
        const uint16_t rq = (uint16_t)((hdr[pipe::HDR_REQ0 + j / 2] >> (16 * (j & 1))) & 0xffffu);
        std::fwrite(&rq, 2, 1, fb);
      }
      const uint16_t w = (uint16_t)hdr[2], act = (uint16_t)hdr[0];
      std::fwrite(&w, 2, 1, fb);
      std::fwrite(&act, 2, 1, fb);
    }
    std::fprintf(fp, "%d %d %d %d %lld %d %lld %d 0 %d\n", T.group, T.sweep, T.W, T.nsteps, (long long)active, T.nprod, (long long)wide, T.start_level, T.moved);
  }
  std::fclose(fp);
  std::fclose(fb);
  return 0;
}

// move_max = 0 against what the builder makes with the tasks moved: the same tasks (steps, producers by count, tiles) in another
// order -- out: [0] tasks, [1] 1 when the multisets of (sweep, group, start level, steps, producers, W) agree, [2] [3] stream bytes
extern "C" int pipe_queue_same_tasks(int64_t n, const int64_t *rp, const int32_t *ci, const double *lu, const int64_t *diag, int nblocks,
                                     const int64_t *block_ptr, int delta, int move_gap, int move_max, int64_t *out)
{
  pipe::Options a, b;
  a.delta = b.delta = delta;
  a.move_max = 0;
  b.move_gap = move_gap;
  b.move_max = move_max;
  pipe::Schedule SA, SB;
  if (!pipe::build(n, rp, ci, lu, diag, nblocks, block_ptr, a, SA) || !pipe::build(n, rp, ci, lu, diag, nblocks, block_ptr, b, SB)) return 1;
  auto key = [](const pipe::Schedule &S) {
    std::vector<std::vector<int64_t>> k;
    for (const pipe::Task &T : S.tasks) k.push_back({T.sweep, T.group, T.start_level, T.nsteps, T.nprod, T.W, T.first_kib});
    std::sort(k.begin(), k.end());
    return k;
  };
  out[0] = (int64_t)SA.tasks.size();
  out[1] = SA.tasks.size() == SB.tasks.size() && key(SA) == key(SB);
  out[2] = (int64_t)SA.stream.size();
  out[3] = (int64_t)SB.stream.size();
  return 0;
}
