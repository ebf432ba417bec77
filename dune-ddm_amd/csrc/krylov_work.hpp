// KrylovWork: the n x width work blocks that the block Krylov drivers (krylov_*.hpp) keep between calls, one pool per preconditioner
// object (ddm_combined::work).  A driver opens with ONE reserve call and names its blocks by local pointers; what a block holds on
// entry is whatever the last driver left there.  Needs device_buffer.hpp and MULTI_MAX (multi_kernels.hpp).
#pragma once

struct KrylovWork {
  static constexpr int MAX_BLOCKS = 7; // queued BiCGSTAB: x, r, rt, p, v, y, t
  dbuf<double> block[MAX_BLOCKS];      // block[i]: rows x width doubles for i < nblocks
  dbuf<int64_t> tab;                   // the queued drivers' (slot, column) pairs of one load or store launch, 2 * MULTI_MAX entries
  int width = 0, nblocks = 0;          // both read 0 until every block of a request is there
  // Grow-only: blocks 0 .. want - 1 of rows x (at least cols) doubles.  A wider request drops every block and allocates afresh, one
  // for more blocks adds them at the pool's width; contents are never kept.
  hipError_t reserve(int cols, int64_t rows, int want)
  {
    if (cols <= width && want <= nblocks) return hipSuccess;
    const int w = std::max(cols, width), first = cols > width ? 0 : nblocks;
    width = nblocks = 0;
    hipError_t e = tab ? hipSuccess : tab.alloc(2 * MULTI_MAX);
    for (int i = first; i < MAX_BLOCKS && e == hipSuccess; ++i) e = i < want ? block[i].alloc(rows * w) : block[i].reset();
    if (e == hipSuccess) width = w, nblocks = want;
    return e;
  }
};
