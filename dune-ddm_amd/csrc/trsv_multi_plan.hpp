// Plan of the single-launch block solve (engine `xcd` of the multi-RHS path: engine_multi_xcd.hpp; kernel k_trsv_multi_xcd in
// kernels.hpp): the dependency levels of a triangle, the per-block sub-ranges of the level engine's levels, and the team arithmetic
// of the kernel.  Plain C++ (standard headers only), so that the host parts compile into a stand-alone program
// (tools/probes/trsv_multi_plan_host_check.hip).  Needs <algorithm>, <cstdint>, <vector>.
#pragma once

#if defined(__HIPCC__)
#define DDM_MULTI_HD __host__ __device__
#else
#define DDM_MULTI_HD
#endif

namespace multi_xcd {

// level[i] of every row of the lower (upper = false: rows ascending) or upper (rows descending) triangle of a CSR pattern with
// sorted rows; diag[i] = position of the diagonal entry of row i.  Returns the highest level (-1 for n = 0).
inline int32_t tri_levels(int64_t n, const int64_t *rp, const int32_t *ci, const int64_t *diag, bool upper, int32_t *level)
{
  int32_t maxlev = -1;
  if (!upper) {
    for (int64_t i = 0; i < n; ++i) {
      int32_t l = 0;
      for (int64_t k = rp[i]; k < diag[i]; ++k) l = std::max(l, level[ci[k]] + 1);
      level[i] = l;
      maxlev = std::max(maxlev, l);
    }
  } else {
    for (int64_t i = n - 1; i >= 0; --i) {
      int32_t l = 0;
      for (int64_t k = diag[i] + 1; k < rp[i + 1]; ++k) l = std::max(l, level[ci[k]] + 1);
      level[i] = l;
      maxlev = std::max(maxlev, l);
    }
  }
  return maxlev;
}

// The level engine sorts the rows of a level in ascending order and blocks are contiguous row ranges, so the rows of block b are
// positions [off[l (nb + 1) + b], off[l (nb + 1) + b + 1]) of level l (off[l (nb + 1) + nb] = rows of the level); no entry couples
// two blocks, so levels 0 .. blk_nlev[b] - 1 are the block's own levels and each of them holds at least one of its rows.
inline void plan_tables(int64_t nlev, int64_t nb, const int64_t *block_ptr, const int32_t *level, std::vector<int32_t> &off, std::vector<int32_t> &blk_nlev)
{
  off.assign((size_t)(nlev * (nb + 1)), 0);
  blk_nlev.assign((size_t)nb, 0);
  for (int64_t b = 0; b < nb; ++b)
    for (int64_t i = block_ptr[b]; i < block_ptr[b + 1]; ++i) {
      off[(size_t)((int64_t)level[i] * (nb + 1) + b + 1)] += 1;
      blk_nlev[(size_t)b] = std::max(blk_nlev[(size_t)b], level[i] + 1);
    }
  for (int64_t l = 0; l < nlev; ++l)
    for (int64_t b = 0; b < nb; ++b) off[(size_t)(l * (nb + 1) + b + 1)] += off[(size_t)(l * (nb + 1) + b)];
}

// Who shares a barrier.  T = min(nblocks, 8) teams; XCD x belongs to team x % T, team t solves blocks t, t + T, ...  A workgroup's
// rank inside its team counts the workgroups of the team's lower XCDs, then its own ticket.  If some team got no workgroup (or
// force_one is set), all workgroups form ONE team that solves every block: rank = global ticket, size = the grid.
struct Team {
  int nteams, team, rank, size, one;
};
DDM_MULTI_HD inline Team team_of(const unsigned tickets[8], int nblocks, int force_one, unsigned xcc, unsigned xcd_ticket, unsigned global_ticket, unsigned grid)
{
  const int T = nblocks < 8 ? (nblocks < 1 ? 1 : nblocks) : 8;
  unsigned size[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int x = 0; x < 8; ++x) size[x % T] += tickets[x];
  bool empty = false;
  for (int t = 0; t < T; ++t) empty = empty || size[t] == 0;
  Team R;
  if (force_one || empty) {
    R.nteams = 1, R.team = 0, R.rank = (int)global_ticket, R.size = (int)grid, R.one = 1;
    return R;
  }
  R.nteams = T, R.team = (int)(xcc % (unsigned)T), R.one = 0;
  unsigned before = 0;
  for (unsigned x = 0; x < xcc; ++x)
    if ((int)(x % (unsigned)T) == R.team) before += tickets[x];
  R.rank = (int)(before + xcd_ticket);
  R.size = (int)size[R.team];
  return R;
}

} // namespace multi_xcd
