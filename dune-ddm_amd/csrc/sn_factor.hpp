// Host driver of the supernodal factor on the device: the Factor object (everything the kernels of sn_chol.hpp and sn_solve1.hpp read,
// host and device side), its plans (top levels, chains, colours), and build / factorize / reserve / solve, which only enqueue.
// Needs sn_chol.hpp (Meta, the block kernels) and sn_solve1.hpp (TopPlan, ChainDev, ChainPlan, the single-vector kernels).
#pragma once

namespace sn {

// chains of the top levels, host side (sn_solve1.hpp: "CHAINS")
struct ChainHost {
  std::vector<int32_t> chain_of;                                                     // [nsn]: chain of a top supernode, -1 below the top levels
  std::vector<int32_t> first_sn, nlinks, col0, ncol, last_sn, nE, clevel, colour, block; // [nchain]
  std::vector<int64_t> woff, eoff;                                                   // [nchain] offsets (doubles) of the n x n triangle / the n_E x n block
  int32_t nclev = 0, max_vec = 0, max_links = 0;
  int64_t wtot = 0, etot = 0;
  // setup work lists: links of all chains (scatter) and the (chain, i) pairs of every distance d (inversion)
  std::vector<int32_t> link_sn, link_chain, link_pre, inv_chain, inv_i, inv_ptr;
  int nchain() const { return (int)first_sn.size(); }
};

// ---- host driver -------------------------------------------------------------------------------------------------------------------
struct Factor {
  int64_t n = 0, entries = 0;
  int nblocks = 1;
  int32_t nsn = 0, nlev = 0;
  double flops = 0.0;
  Meta M{};
  std::vector<int32_t> h_perm;           // perm[new] = old (global)
  std::vector<int32_t> lev_ptr;          // [nlev + 1] into lev_sn
  std::vector<int32_t> lev_big_ptr;      // [nlev + 1] into big_sn
  std::vector<int32_t> lev_maxnc;        // widest supernode of the level
  std::vector<int32_t> lev_maxnr;        // longest row list of the level
  // Colours (deterministic updates): supernodes of one level whose row lists intersect would subtract from the same ancestor entries.
  // They get different colours; the level's list in lev_sn is sorted by colour and the update kernels run colour by colour, so every
  // panel entry receives its contributions in ONE order (level, colour) whatever the hardware does -- no atomics.
  std::vector<int32_t> lev_phase_ptr;    // [nlev + 1] into phase_k
  std::vector<int32_t> phase_k;          // first position (relative to lev_ptr[l]) of every colour of every level, plus the level's end
  std::vector<int32_t> h_preU, h_preUF, h_preT; // host copies of the tile prefixes (launch bounds of a colour)
  std::vector<int32_t> h_colour;         // colour of every supernode
  std::vector<int32_t> h_first;          // host copy of `first`
  // device
  dbuf<int32_t> d_first, d_nrow, d_rows, d_sn_of_col, d_iperm, d_perm;
  dbuf<int64_t> d_rptr, d_pptr;
  dbuf<double> d_panels;
  dbuf<int32_t> d_lev_sn;   // supernodes sorted by level
  dbuf<int32_t> d_preT;     // per level: exclusive prefix of the row-tile counts (lev_ptr[l] + l .. : cnt + 1 entries)
  dbuf<int32_t> d_preU;     // the same for the update tiles T (T + 1) / 2
  dbuf<int32_t> d_big_sn, d_big_index, d_preB; // supernodes with more than BWD_SMALL row tiles, per level
  std::vector<int32_t> h_tilesT, h_tilesU, h_tilesB; // totals per level
  dbuf<unsigned> d_err;
  bool lu = false;               // L U variant
  dbuf<double> d_upanels;
  dbuf<int64_t> d_uptr;
  dbuf<int32_t> d_piv;
  int64_t uentries = 0;
  std::vector<int32_t> h_tilesUF; // L U: all T x T update tiles per level
  dbuf<int32_t> d_preUF;
  dbuf<double> d_partial;
  int64_t partial_cap = 0; // doubles
  // single-vector solves: the persistent kernel for the top levels (sn_solve1.hpp)
  std::vector<int32_t> sn_block;  // block of every supernode
  int32_t ltop = 0, ntop = 0;     // tree levels ltop .. nlev - 1 are walked by k_sn_top1 (ntop = 0: level kernels only)
  TopPlan top{};
  dbuf<int32_t> d_top_ints;  // all integer arrays of the plan in one allocation
  dbuf<double> d_top_partial;
  dbuf<TopSync> d_top_sync;
  dbuf<unsigned long long> d_top_flags, d_top_stamps; // stamps: diagnostics (DDM_SN_TOP_STAMPS)
  int top_grid = 0, top_spread = 0, chain_grid = 0;
  // CHAINS of the top levels (sn_solve1.hpp): a separator wider than SN_MAX_COLS is a chain of links s -> s + 1 = parent(s), each the
  // only child of the next.  For the single-vector solves a chain is ONE dense unit with an explicitly inverted triangle.
  ChainHost ch;
  ChainDev chd{};
  ChainPlan chp{};
  const int32_t *ch_link_sn = nullptr, *ch_link_chain = nullptr, *ch_link_pre = nullptr, *ch_inv_chain = nullptr, *ch_inv_i = nullptr;
  dbuf<int32_t> d_chain_ints;
  dbuf<int64_t> d_chain_offs;
  dbuf<double> d_chain_w, d_chain_e, d_chain_v, d_chain_u; // inverse triangles / blocks of the external rows (L; L U: also U^T)
  bool chains_ready = false;
  double chain_setup_s = 0.0;    // host seconds of the last chain_setup (temporaries, kernels, synchronisation): diagnostics
  dbuf<int64_t> d_tptr, d_tmid;  // transposed row lists (Meta::tptr / tmid / tidx)
  dbuf<int32_t> d_tidx, d_tpos;
  dbuf<double> d_contrib; // slots of the forward sweep: one per entry of `rows` and right-hand side
  int64_t contrib_cap = 0, nrows_total = 0;
  int64_t max_big_tiles = 0;
  ~Factor()
  {
    if (d_top_stamps) { // diagnostics: barrier log of the LAST launch of the persistent kernel
      std::vector<unsigned long long> h(4000);
      if (hipMemcpy(h.data(), d_top_stamps, 8 * h.size(), hipMemcpyDeviceToHost) == hipSuccess) {
        std::fprintf(stderr, "[ddm] k_sn_top1 barrier log (us since the first barrier; work = arrival - previous release, wait = release - arrival):\n");
        const unsigned long long t0 = h[3];
        for (int c = 1; c < 2000 && h[2 * c + 1]; ++c)
          std::fprintf(stderr, "  barrier %3d: arrive %8.2f release %8.2f  work %6.2f wait %6.2f\n", c, (double)(h[2 * c] - t0) / 100.0, (double)(h[2 * c + 1] - t0) / 100.0,
                       c > 1 ? (double)(h[2 * c] - h[2 * c - 1]) / 100.0 : 0.0, (double)(h[2 * c + 1] - h[2 * c]) / 100.0);
      }
    }
  }
};

template <class T>
static inline bool up(const std::vector<T> &h, dbuf<T> &d)
{
  if (d.alloc((int64_t)h.size()) != hipSuccess) return false;
  return h.empty() || hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice) == hipSuccess;
}

// Top levels of the single-vector solve (sn_solve1.hpp): those from the first level on which every later level has at most
// `top_max` supernodes (the separator chains: one supernode per block and level); fewer than four such levels are not worth a launch
// of their own.  DDM_SN_TOP_MAX overrides the bound (0: level kernels only).  Needs lev_ptr; sets ltop / ntop.
static inline void decide_top_levels(Factor &F)
{
  int top_max = 128; // (measured: DG 512^2 1.51 / 1.46 / 1.54 / 1.75 ms per solve at 32 / 128 / 512 / 2048, elasticity 1.31 / 1.29 / 1.28 / 1.39; tools/gpu_r04_i.sh)
  if (const char *e = std::getenv("DDM_SN_TOP_MAX")) top_max = std::atoi(e);
  int32_t ltop = F.nlev;
  while (ltop > 0 && F.lev_ptr[(size_t)ltop] - F.lev_ptr[(size_t)ltop - 1] <= top_max) --ltop;
  F.ltop = F.nlev;
  F.ntop = 0;
  if (F.nlev - ltop < 4) return;
  int dev = 0, ncu = 0, per_cu = 0;
  (void)hipGetDevice(&dev);
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) return; // (no device: host-only use)
  const void *fn = F.lu ? (const void *)k_sn_top1<true> : (const void *)k_sn_top1<false>;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, TOP_THREADS, 0) != hipSuccess || per_cu < 1) return;
  F.top_grid = std::min(per_cu, 2) * (ncu / 8 * 8); // co-resident: at most two workgroups of 512 threads per CU
  if (F.top_grid < 8 || F.top_grid > TOP_MAX_WG) return;
  F.ltop = ltop;
  F.ntop = F.nlev - ltop;
}
// Plan of the persistent kernel: per class (block % 8) the top supernodes by level, their forward tiles by (level, colour), their
// backward chunks by level, and the 16-column pieces of all their columns for the gather of the bottom levels' slots.
static inline bool build_top_plan(Factor &F, const std::vector<int32_t> &lev_sn, const std::vector<int32_t> &nrow, const std::vector<int32_t> &first)
{
  if (F.ntop == 0) return true;
  const int32_t ntop = F.ntop, ltop = F.ltop;
  // colours per top level (global over the classes: the barrier count of a level must not depend on the class)
  std::vector<int32_t> fph((size_t)ntop + 1, 0);
  for (int32_t j = 0; j < ntop; ++j) {
    int nc = 1;
    for (int32_t k = F.lev_ptr[(size_t)(ltop + j)]; k < F.lev_ptr[(size_t)(ltop + j) + 1]; ++k) nc = std::max(nc, F.h_colour[(size_t)lev_sn[(size_t)k]] + 1);
    fph[(size_t)j + 1] = fph[(size_t)j] + nc;
  }
  const int32_t nph = fph[(size_t)ntop];
  std::vector<int32_t> a_ptr((size_t)8 * ntop + 1, 0), f_ptr((size_t)8 * nph + 1, 0), p_ptr((size_t)8 * ntop + 1, 0), g_ptr(9, 0), a_sn, f_items, p_items, g_items,
      p_first((size_t)F.nsn, 0);
  for (int c = 0; c < 8; ++c) {
    for (int32_t j = 0; j < ntop; ++j) {
      const int32_t l = ltop + j;
      for (int32_t k = F.lev_ptr[(size_t)l]; k < F.lev_ptr[(size_t)l + 1]; ++k) {
        const int32_t s = lev_sn[(size_t)k];
        if (F.sn_block[(size_t)s] % 8 != c) continue;
        a_sn.push_back(s);
        const int32_t nr = nrow[(size_t)s], ncs = first[(size_t)s + 1] - first[(size_t)s];
        p_first[(size_t)s] = (int32_t)(p_items.size() / 2);
        for (int32_t q = 0; q < (nr + TILE - 1) / TILE; ++q) { // backward: one partial product per 64-row tile
          p_items.push_back(s);
          p_items.push_back(q);
        }
        for (int32_t q = 0; q < (ncs + 15) / 16; ++q) {
          g_items.push_back(s);
          g_items.push_back(q);
        }
      }
      a_ptr[(size_t)c * ntop + j + 1] = (int32_t)a_sn.size();
      p_ptr[(size_t)c * ntop + j + 1] = (int32_t)(p_items.size() / 2);
      for (int32_t col = 0; col < fph[(size_t)j + 1] - fph[(size_t)j]; ++col) { // forward tiles, colour by colour
        for (int32_t k = F.lev_ptr[(size_t)l]; k < F.lev_ptr[(size_t)l + 1]; ++k) {
          const int32_t s = lev_sn[(size_t)k];
          if (F.sn_block[(size_t)s] % 8 != c || F.h_colour[(size_t)s] != col) continue;
          for (int32_t t = 0; t < (nrow[(size_t)s] + TILE - 1) / TILE; ++t) {
            f_items.push_back(s);
            f_items.push_back(t);
          }
          if (nrow[(size_t)s] == 0) { // no rows below (a root): the pseudo tile -1 computes and stores y_s
            f_items.push_back(s);
            f_items.push_back(-1);
          }
        }
        f_ptr[(size_t)c * nph + fph[(size_t)j] + col + 1] = (int32_t)(f_items.size() / 2);
      }
    }
    g_ptr[(size_t)c + 1] = (int32_t)(g_items.size() / 2);
  }
  std::vector<int32_t> all;
  auto put = [&](const std::vector<int32_t> &v) {
    const size_t o = all.size();
    all.insert(all.end(), v.begin(), v.end());
    return o;
  };
  const size_t o_ap = put(a_ptr), o_as = put(a_sn), o_fh = put(fph), o_fp = put(f_ptr), o_fi = put(f_items), o_pp = put(p_ptr), o_pi = put(p_items), o_pf = put(p_first),
               o_gp = put(g_ptr), o_gi = put(g_items);
  if (!up(all, F.d_top_ints)) return false;
  if (F.d_top_partial.alloc((int64_t)std::max<size_t>(p_items.size() / 2, 1) * SN_MAX_COLS) != hipSuccess) return false;
  if (F.d_top_sync.alloc(1) != hipSuccess || hipMemset(F.d_top_sync, 0, sizeof(TopSync)) != hipSuccess) return false;
  const int64_t fwords = (int64_t)9 * TOP_MAX_WG * TOP_FLAG_STRIDE;
  if (F.d_top_flags.alloc(fwords) != hipSuccess || hipMemset(F.d_top_flags, 0, sizeof(unsigned long long) * (size_t)fwords) != hipSuccess) return false;
  if (std::getenv("DDM_SN_TOP_STAMPS")) {
    if (F.d_top_stamps.alloc(4000) != hipSuccess || hipMemset(F.d_top_stamps, 0, 8 * 4000) != hipSuccess) return false;
  }
  F.top.ntop = ntop;
  F.top.nph = nph;
  F.top.a_ptr = F.d_top_ints + o_ap;
  F.top.a_sn = F.d_top_ints + o_as;
  F.top.fph = F.d_top_ints + o_fh;
  F.top.f_ptr = F.d_top_ints + o_fp;
  F.top.f_items = F.d_top_ints + o_fi;
  F.top.p_ptr = F.d_top_ints + o_pp;
  F.top.p_items = F.d_top_ints + o_pi;
  F.top.p_first = F.d_top_ints + o_pf;
  F.top.g_ptr = F.d_top_ints + o_gp;
  F.top.g_items = F.d_top_ints + o_gi;
  // one block over all XCDs (write-through hand-overs, one barrier group) only when a block is too large for the bandwidth of one
  // XCD; otherwise block b lives on XCD b % 8 also when fewer than 8 blocks leave XCDs idle
  F.top_spread = (F.nblocks < 8 && (double)F.entries * 8.0 / std::max(1, F.nblocks) > 256e6) ? 1 : 0;
  if (const char *e = std::getenv("DDM_SN_TOP_SPREAD")) F.top_spread = std::atoi(e) != 0;
  return true;
}

// Chains among the top supernodes: s -> s + 1 = parent(s) while the parent has no other child (the links a wide separator was cut
// into).  Chain levels: a chain is one level above the highest chain hanging below it.  Colours inside a chain level: chains whose
// external row sets intersect subtract from the same entries and run one after the other.
static inline bool build_chains(Factor &F, int64_t n, const std::vector<int32_t> &level, const std::vector<int32_t> &first, const std::vector<int32_t> &nrow,
                                const std::vector<int64_t> &rptr, const std::vector<int32_t> &rows, const std::vector<int32_t> &parent_g)
{
  ChainHost &H = F.ch;
  H = ChainHost();
  if (F.ntop == 0) return true;
  if (const char *e = std::getenv("DDM_SN_CHAINS"))
    if (e[0] == '0') return true;
  const int32_t nsn = F.nsn;
  std::vector<int32_t> nchild((size_t)nsn, 0);
  for (int32_t s = 0; s < nsn; ++s)
    if (parent_g[(size_t)s] >= 0) nchild[(size_t)parent_g[(size_t)s]]++;
  H.chain_of.assign((size_t)nsn, -1);
  for (int32_t s = 0; s < nsn; ++s) {
    if (level[(size_t)s] < F.ltop || H.chain_of[(size_t)s] >= 0) continue;
    const int32_t c = H.nchain();
    int32_t cur = s, links = 1;
    H.chain_of[(size_t)s] = c;
    for (;;) {
      const int32_t p = parent_g[(size_t)cur];
      if (p != cur + 1 || nchild[(size_t)p] != 1 || level[(size_t)p] < F.ltop || F.sn_block[(size_t)p] != F.sn_block[(size_t)s]) break;
      H.chain_of[(size_t)p] = c;
      cur = p;
      ++links;
    }
    H.first_sn.push_back(s);
    H.nlinks.push_back(links);
    H.col0.push_back(first[(size_t)s]);
    H.ncol.push_back(first[(size_t)cur + 1] - first[(size_t)s]);
    H.last_sn.push_back(cur);
    H.nE.push_back(nrow[(size_t)cur]);
    H.block.push_back(F.sn_block[(size_t)s]);
    H.max_links = std::max(H.max_links, links);
    H.max_vec = std::max(H.max_vec, std::max(H.ncol.back(), H.nE.back()));
  }
  const int nch = H.nchain();
  H.clevel.assign((size_t)nch, 0);
  for (int c = 0; c < nch; ++c) { // (ascending first supernode: every chain below has been seen)
    const int32_t p = parent_g[(size_t)H.last_sn[(size_t)c]];
    if (p >= 0 && H.chain_of[(size_t)p] >= 0) H.clevel[(size_t)H.chain_of[(size_t)p]] = std::max(H.clevel[(size_t)H.chain_of[(size_t)p]], H.clevel[(size_t)c] + 1);
  }
  // a chain hanging below an INNER link cannot exist (inner links have one child), but one below the first link raises the level
  // only through the loop above: levels are final because children have smaller numbers than the first link of their parent chain
  H.nclev = 0;
  for (int c = 0; c < nch; ++c) H.nclev = std::max(H.nclev, H.clevel[(size_t)c] + 1);
  H.colour.assign((size_t)nch, 0);
  {
    std::vector<uint64_t> rowmask((size_t)n, 0);
    std::vector<int32_t> rowstamp((size_t)n, -1);
    for (int32_t L = 0; L < H.nclev; ++L)
      for (int c = 0; c < nch; ++c) {
        if (H.clevel[(size_t)c] != L) continue;
        const int32_t sl = H.last_sn[(size_t)c];
        uint64_t used = 0;
        for (int64_t q = rptr[(size_t)sl]; q < rptr[(size_t)sl + 1]; ++q)
          if (rowstamp[(size_t)rows[(size_t)q]] == L) used |= rowmask[(size_t)rows[(size_t)q]];
        if (~used == 0) return false;
        const int col = __builtin_ctzll(~used);
        H.colour[(size_t)c] = col;
        for (int64_t q = rptr[(size_t)sl]; q < rptr[(size_t)sl + 1]; ++q) {
          const int32_t r = rows[(size_t)q];
          if (rowstamp[(size_t)r] != L) {
            rowstamp[(size_t)r] = L;
            rowmask[(size_t)r] = 0;
          }
          rowmask[(size_t)r] |= 1ull << col;
        }
      }
  }
  H.woff.assign((size_t)nch, 0);
  H.eoff.assign((size_t)nch, 0);
  for (int c = 0; c < nch; ++c) {
    H.woff[(size_t)c] = H.wtot;
    H.eoff[(size_t)c] = H.etot;
    H.wtot += (int64_t)H.ncol[(size_t)c] * H.ncol[(size_t)c];
    H.etot += (int64_t)H.nE[(size_t)c] * H.ncol[(size_t)c];
  }
  // setup work lists
  H.link_pre.push_back(0);
  for (int c = 0; c < nch; ++c)
    for (int32_t k = 0; k < H.nlinks[(size_t)c]; ++k) {
      const int32_t s = H.first_sn[(size_t)c] + k;
      H.link_sn.push_back(s);
      H.link_chain.push_back(c);
      H.link_pre.push_back(H.link_pre.back() + (first[(size_t)s + 1] - first[(size_t)s] + nrow[(size_t)s] + TILE - 1) / TILE);
    }
  H.inv_ptr.assign((size_t)std::max(H.max_links, 1) + 1, 0);
  for (int32_t d = 1; d < H.max_links; ++d) {
    for (int c = 0; c < nch; ++c)
      for (int32_t i = d; i < H.nlinks[(size_t)c]; ++i) {
        H.inv_chain.push_back(c);
        H.inv_i.push_back(i);
      }
    H.inv_ptr[(size_t)d + 1] = (int32_t)H.inv_chain.size();
  }
  if (H.max_links >= 1) H.inv_ptr[1] = 0;
  return true;
}
// device side of the chains: arrays, the plan of k_sn_top_chain (one allocation of integers)
static inline bool upload_chains(Factor &F)
{
  ChainHost &H = F.ch;
  const int nch = H.nchain();
  if (nch == 0) return true;
  const int nclev = H.nclev;
  // phases of the external-row updates: chain levels x colours
  std::vector<int32_t> eph((size_t)nclev + 1, 0);
  for (int L = 0; L < nclev; ++L) {
    int nc = 1;
    for (int c = 0; c < nch; ++c)
      if (H.clevel[(size_t)c] == L) nc = std::max(nc, H.colour[(size_t)c] + 1);
    eph[(size_t)L + 1] = eph[(size_t)L] + nc;
  }
  const int nph = eph[(size_t)nclev];
  std::vector<int32_t> y_ptr((size_t)8 * nclev + 1, 0), t_ptr((size_t)8 * nclev + 1, 0), x_ptr((size_t)8 * nclev + 1, 0), e_ptr((size_t)8 * nph + 1, 0), y_items, t_items, x_items, e_items;
  for (int cls = 0; cls < 8; ++cls)
    for (int L = 0; L < nclev; ++L) {
      for (int c = 0; c < nch; ++c) {
        if (H.block[(size_t)c] % 8 != cls || H.clevel[(size_t)c] != L) continue;
        const int nb = (H.ncol[(size_t)c] + 63) / 64;
        for (int rb = nb - 1; rb >= 0; --rb) { // the long rows first
          y_items.push_back(c);
          y_items.push_back(rb);
          // columns the rows of the block reach: up to the end of the link of the block's last row (the diagonal blocks of the L U
          // variant are full: the row exchanges are absorbed), for Cholesky the lower triangle is cut by the kernel
          const int32_t lastrow = H.col0[(size_t)c] + std::min(H.ncol[(size_t)c], 64 * rb + 64) - 1;
          int32_t sl = H.first_sn[(size_t)c];
          while (F.h_first[(size_t)sl + 1] <= lastrow) ++sl;
          y_items.push_back(F.h_first[(size_t)sl + 1] - H.col0[(size_t)c]);
        }
        for (int cb = 0; cb < nb; ++cb) { // (the long columns first)
          x_items.push_back(c);
          x_items.push_back(cb);
          if (H.nE[(size_t)c] > 0) {
            t_items.push_back(c);
            t_items.push_back(cb);
          }
        }
      }
      y_ptr[(size_t)cls * nclev + L + 1] = (int32_t)(y_items.size() / 3);
      x_ptr[(size_t)cls * nclev + L + 1] = (int32_t)(x_items.size() / 2);
      t_ptr[(size_t)cls * nclev + L + 1] = (int32_t)(t_items.size() / 2);
      for (int col = 0; col < eph[(size_t)L + 1] - eph[(size_t)L]; ++col) {
        for (int c = 0; c < nch; ++c) {
          if (H.block[(size_t)c] % 8 != cls || H.clevel[(size_t)c] != L || H.colour[(size_t)c] != col) continue;
          for (int t = 0; t < (H.nE[(size_t)c] + 63) / 64; ++t) {
            e_items.push_back(c);
            e_items.push_back(t);
          }
        }
        e_ptr[(size_t)cls * nph + eph[(size_t)L] + col + 1] = (int32_t)(e_items.size() / 2);
      }
    }
  std::vector<int32_t> all;
  auto put = [&](const std::vector<int32_t> &v) {
    const size_t o = all.size();
    all.insert(all.end(), v.begin(), v.end());
    return o;
  };
  const size_t o_c0 = put(H.col0), o_nc = put(H.ncol), o_fs = put(H.first_sn), o_nl = put(H.nlinks), o_ls = put(H.last_sn), o_ne = put(H.nE), o_yp = put(y_ptr), o_yi = put(y_items),
               o_eh = put(eph), o_ep = put(e_ptr), o_ei = put(e_items), o_tp = put(t_ptr), o_ti = put(t_items), o_xp = put(x_ptr), o_xi = put(x_items), o_lsn = put(H.link_sn),
               o_lch = put(H.link_chain), o_lpre = put(H.link_pre), o_ic = put(H.inv_chain), o_ii = put(H.inv_i);
  if (!up(all, F.d_chain_ints)) return false;
  std::vector<int64_t> offs(H.woff);
  offs.insert(offs.end(), H.eoff.begin(), H.eoff.end());
  if (!up(offs, F.d_chain_offs)) return false;
  if (F.d_chain_w.alloc(H.wtot) != hipSuccess || F.d_chain_e.alloc(H.etot) != hipSuccess) return false;
  if (F.lu && (F.d_chain_v.alloc(H.wtot) != hipSuccess || F.d_chain_u.alloc(H.etot) != hipSuccess)) return false;
  const int32_t *I = F.d_chain_ints;
  F.chd.nchain = nch;
  F.chd.col0 = I + o_c0;
  F.chd.ncol = I + o_nc;
  F.chd.first_sn = I + o_fs;
  F.chd.nlinks = I + o_nl;
  F.chd.last_sn = I + o_ls;
  F.chd.nE = I + o_ne;
  F.chd.woff = F.d_chain_offs;
  F.chd.eoff = F.d_chain_offs + nch;
  F.chd.W = F.d_chain_w;
  F.chd.E = F.d_chain_e;
  F.chd.V = F.d_chain_v;
  F.chd.U = F.d_chain_u;
  F.chp.nclev = nclev;
  F.chp.nph = nph;
  F.chp.y_ptr = I + o_yp;
  F.chp.y_items = I + o_yi;
  F.chp.eph = I + o_eh;
  F.chp.e_ptr = I + o_ep;
  F.chp.e_items = I + o_ei;
  F.chp.t_ptr = I + o_tp;
  F.chp.t_items = I + o_ti;
  F.chp.x_ptr = I + o_xp;
  F.chp.x_items = I + o_xi;
  F.chp.g_ptr = F.top.g_ptr;
  F.chp.g_items = F.top.g_items;
  F.ch_link_sn = I + o_lsn;
  F.ch_link_chain = I + o_lch;
  F.ch_link_pre = I + o_lpre;
  F.ch_inv_chain = I + o_ic;
  F.ch_inv_i = I + o_ii;
  { // the chain kernel holds one chain vector in dynamic LDS: it must fit and leave the co-resident grid of the top levels possible
    const void *fn = F.lu ? (const void *)k_sn_top_chain<true> : (const void *)k_sn_top_chain<false>;
    const size_t lds = (size_t)H.max_vec * 8;
    int per_cu = 0;
    if (lds > 150 * 1024 || hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, TOP_THREADS, lds) != hipSuccess || per_cu < 1) {
      H = ChainHost(); // (the link-by-link kernel serves the top levels)
      return true;
    }
    int dev = 0, ncu = 0;
    (void)hipGetDevice(&dev);
    F.chain_grid = F.top_grid;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0) F.chain_grid = std::min(per_cu, 2) * (ncu / 8 * 8);
    if (F.chain_grid > TOP_MAX_WG) F.chain_grid = F.top_grid;
  }
  return true;
}
// after the numeric factorisation: dense copies and the blocked inversion of every chain (enqueued; temporaries freed after a sync)
static inline hipError_t chain_setup(Factor &F, hipStream_t st)
{
  F.chains_ready = false;
  const ChainHost &H = F.ch;
  if (H.nchain() == 0) return hipSuccess;
  hipError_t e;
  dbuf<double> Ltmp, Utmp; // (released when the function returns: after the synchronisation below)
  if ((e = Ltmp.alloc(H.wtot)) != hipSuccess) return e;
  if (F.lu && (e = Utmp.alloc(H.wtot)) != hipSuccess) return e;
  (void)hipMemsetAsync(Ltmp, 0, sizeof(double) * (size_t)H.wtot, st);
  (void)hipMemsetAsync(F.d_chain_w, 0, sizeof(double) * (size_t)H.wtot, st);
  (void)hipMemsetAsync(F.d_chain_e, 0, sizeof(double) * (size_t)std::max<int64_t>(H.etot, 1), st);
  if (F.lu) {
    (void)hipMemsetAsync(Utmp, 0, sizeof(double) * (size_t)H.wtot, st);
    (void)hipMemsetAsync(F.d_chain_v, 0, sizeof(double) * (size_t)H.wtot, st);
    (void)hipMemsetAsync(F.d_chain_u, 0, sizeof(double) * (size_t)std::max<int64_t>(H.etot, 1), st);
  }
  const int nlinks_total = (int)H.link_sn.size();
  const unsigned stiles = (unsigned)H.link_pre.back();
  if (stiles > 0) {
    if (F.lu) hipLaunchKernelGGL(k_chain_scatter<true>, dim3(stiles), dim3(256), 0, st, F.M, F.chd, F.ch_link_sn, F.ch_link_chain, F.ch_link_pre, nlinks_total, Ltmp, Utmp);
    else hipLaunchKernelGGL(k_chain_scatter<false>, dim3(stiles), dim3(256), 0, st, F.M, F.chd, F.ch_link_sn, F.ch_link_chain, F.ch_link_pre, nlinks_total, Ltmp, Utmp);
  }
  static DeviceOnce attr_once;
  constexpr size_t inv_lds = (size_t)(SN_MAX_COLS * 64 + 32 * 64) * 8;
  attr_once.run([]() { (void)hipFuncSetAttribute((const void *)k_chain_invert, hipFuncAttributeMaxDynamicSharedMemorySize, (int)inv_lds); });
  for (int32_t d = 1; d < H.max_links; ++d) {
    const int32_t i0 = H.inv_ptr[(size_t)d], i1 = H.inv_ptr[(size_t)d + 1];
    if (i1 <= i0) continue;
    hipLaunchKernelGGL(k_chain_invert, dim3((unsigned)(2 * (i1 - i0))), dim3(512), inv_lds, st, F.M, F.chd, (int)d, F.ch_inv_chain + i0, F.ch_inv_i + i0, (const double *)Ltmp, F.d_chain_w);
    if (F.lu)
      hipLaunchKernelGGL(k_chain_invert, dim3((unsigned)(2 * (i1 - i0))), dim3(512), inv_lds, st, F.M, F.chd, (int)d, F.ch_inv_chain + i0, F.ch_inv_i + i0, (const double *)Utmp, F.d_chain_v);
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) F.chains_ready = true;
  return e;
}

// symbolic results of all blocks -> one global structure on the device.  Returns false on an allocation failure.
static inline bool build(Factor &F, int64_t n, int64_t nblocks, const int64_t *block_ptr, std::vector<BlockSym> &BS, bool lu = false)
{
  F.n = n;
  F.lu = lu;
  F.nblocks = (int)nblocks;
  std::vector<int32_t> first, nrow, rows, sn_of_col((size_t)n), iperm((size_t)n), level, parent_g;
  std::vector<int64_t> rptr(1, 0), pptr(1, 0);
  F.h_perm.resize((size_t)n);
  for (int64_t b = 0; b < nblocks; ++b) {
    BlockSym &S = BS[(size_t)b];
    const int32_t off = (int32_t)block_ptr[b];
    const int32_t nsn = (int32_t)S.first.size() - 1;
    const int32_t sn_base = (int32_t)first.size();
    for (int32_t s = 0; s < nsn; ++s) {
      const int32_t gs = (int32_t)first.size();
      first.push_back(off + S.first[(size_t)s]);
      const int64_t r0 = S.rptr[(size_t)s], r1 = S.rptr[(size_t)s + 1];
      nrow.push_back((int32_t)(r1 - r0));
      for (int64_t k = r0; k < r1; ++k) rows.push_back(off + S.rows[(size_t)k]);
      rptr.push_back((int64_t)rows.size());
      const int64_t nc = S.first[(size_t)s + 1] - S.first[(size_t)s];
      pptr.push_back(pptr.back() + nc * (nc + (r1 - r0)));
      level.push_back(S.level[(size_t)s]);
      parent_g.push_back(S.parent[(size_t)s] < 0 ? -1 : sn_base + S.parent[(size_t)s]);
      F.sn_block.push_back((int32_t)b);
      for (int32_t c = S.first[(size_t)s]; c < S.first[(size_t)s + 1]; ++c) sn_of_col[(size_t)(off + c)] = gs;
    }
    for (int32_t k = 0; k < S.n; ++k) {
      F.h_perm[(size_t)(off + k)] = off + S.perm[(size_t)k];
      iperm[(size_t)(off + S.perm[(size_t)k])] = off + k;
    }
    F.flops += S.flops;
    S = BlockSym();
  }
  first.push_back((int32_t)n);
  F.nsn = (int32_t)nrow.size();
  F.entries = pptr.back();
  int32_t nlev = 0;
  for (int32_t l : level) nlev = std::max(nlev, l + 1);
  F.nlev = nlev;
  // supernodes by level (stable) and the per-level tile prefixes
  F.lev_ptr.assign((size_t)nlev + 1, 0);
  for (int32_t l : level) F.lev_ptr[(size_t)l + 1]++;
  for (int32_t l = 0; l < nlev; ++l) F.lev_ptr[(size_t)l + 1] += F.lev_ptr[(size_t)l];
  std::vector<int32_t> lev_sn((size_t)F.nsn), pos(F.lev_ptr.begin(), F.lev_ptr.end() - 1);
  for (int32_t s = 0; s < F.nsn; ++s) lev_sn[(size_t)pos[(size_t)level[(size_t)s]]++] = s;
  // colours of the update phases (see Factor::lev_phase_ptr): greedy, in list order; a row remembers which colours of the CURRENT
  // level already subtract from it
  F.lev_phase_ptr.assign((size_t)nlev + 1, 0);
  F.phase_k.clear();
  {
    std::vector<uint64_t> rowmask((size_t)n, 0);
    std::vector<int32_t> rowstamp((size_t)n, -1), colour((size_t)F.nsn, 0), sorted;
    for (int32_t l = 0; l < nlev; ++l) {
      const int32_t k0 = F.lev_ptr[(size_t)l], k1 = F.lev_ptr[(size_t)l + 1];
      int ncol = 1;
      for (int32_t k = k0; k < k1; ++k) {
        const int32_t s = lev_sn[(size_t)k];
        uint64_t used = 0;
        for (int64_t q = rptr[(size_t)s]; q < rptr[(size_t)s + 1]; ++q) {
          const int32_t r = rows[(size_t)q];
          if (rowstamp[(size_t)r] == l) used |= rowmask[(size_t)r];
        }
        if (~used == 0) return false; // more than 64 mutually conflicting supernodes in one level (not seen: <= 11 on 3-D grids)
        const int c = __builtin_ctzll(~used);
        colour[(size_t)s] = c;
        ncol = std::max(ncol, c + 1);
        for (int64_t q = rptr[(size_t)s]; q < rptr[(size_t)s + 1]; ++q) {
          const int32_t r = rows[(size_t)q];
          if (rowstamp[(size_t)r] != l) {
            rowstamp[(size_t)r] = l;
            rowmask[(size_t)r] = 0;
          }
          rowmask[(size_t)r] |= 1ull << c;
        }
      }
      sorted.assign(lev_sn.begin() + k0, lev_sn.begin() + k1);
      std::stable_sort(sorted.begin(), sorted.end(), [&](int32_t a, int32_t b) { return colour[(size_t)a] < colour[(size_t)b]; });
      std::copy(sorted.begin(), sorted.end(), lev_sn.begin() + k0);
      F.lev_phase_ptr[(size_t)l] = (int32_t)F.phase_k.size();
      for (int32_t k = k0; k < k1; ++k)
        if (k == k0 || colour[(size_t)lev_sn[(size_t)k]] != colour[(size_t)lev_sn[(size_t)k - 1]]) F.phase_k.push_back(k - k0);
      F.phase_k.push_back(k1 - k0);
      (void)ncol;
    }
    F.lev_phase_ptr[(size_t)nlev] = (int32_t)F.phase_k.size();
    F.h_colour = colour;
  }
  std::vector<int32_t> preT((size_t)F.nsn + nlev), preU((size_t)F.nsn + nlev), preUF((size_t)F.nsn + nlev), big_sn, big_index((size_t)F.nsn, -1), preB;
  std::vector<int64_t> uptr(1, 0);
  for (int32_t s = 0; s < F.nsn; ++s) uptr.push_back(uptr.back() + (int64_t)nrow[(size_t)s] * (first[(size_t)s + 1] - first[(size_t)s]));
  F.uentries = lu ? uptr.back() : 0;
  F.h_tilesUF.assign((size_t)nlev, 0);
  F.h_tilesT.assign((size_t)nlev, 0);
  F.h_tilesU.assign((size_t)nlev, 0);
  F.h_tilesB.assign((size_t)nlev, 0);
  F.lev_maxnc.assign((size_t)nlev, 0);
  F.lev_maxnr.assign((size_t)nlev, 0);
  F.lev_big_ptr.assign((size_t)nlev + 1, 0);
  for (int32_t l = 0; l < nlev; ++l) {
    int64_t aT = 0, aU = 0, aB = 0, aUF = 0;
    const int32_t base = F.lev_ptr[(size_t)l] + l;
    const int32_t bbase = (int32_t)preB.size();
    preB.push_back(0);
    for (int32_t k = F.lev_ptr[(size_t)l]; k < F.lev_ptr[(size_t)l + 1]; ++k) {
      const int32_t s = lev_sn[(size_t)k];
      const int64_t T = (nrow[(size_t)s] + TILE - 1) / TILE;
      preT[(size_t)(base + k - F.lev_ptr[(size_t)l])] = (int32_t)aT;
      preU[(size_t)(base + k - F.lev_ptr[(size_t)l])] = (int32_t)aU;
      preUF[(size_t)(base + k - F.lev_ptr[(size_t)l])] = (int32_t)aUF;
      aT += T;
      aU += T * (T + 1) / 2;
      aUF += T * T;
      if (T > BWD_SMALL) {
        big_index[(size_t)k] = (int32_t)(big_sn.size() - (size_t)F.lev_big_ptr[(size_t)l]);
        big_sn.push_back(s);
        aB += (nrow[(size_t)s] + BWD_ROWS - 1) / BWD_ROWS;
        preB.push_back((int32_t)aB);
      }
      F.lev_maxnc[(size_t)l] = std::max(F.lev_maxnc[(size_t)l], first[(size_t)s + 1] - first[(size_t)s]);
      F.lev_maxnr[(size_t)l] = std::max(F.lev_maxnr[(size_t)l], nrow[(size_t)s]);
    }
    if (aU > 2000000000ll || (lu && aUF > 2000000000ll)) return false;
    preUF[(size_t)(base + F.lev_ptr[(size_t)l + 1] - F.lev_ptr[(size_t)l])] = (int32_t)aUF;
    F.h_tilesUF[(size_t)l] = (int32_t)aUF;
    preT[(size_t)(base + F.lev_ptr[(size_t)l + 1] - F.lev_ptr[(size_t)l])] = (int32_t)aT;
    preU[(size_t)(base + F.lev_ptr[(size_t)l + 1] - F.lev_ptr[(size_t)l])] = (int32_t)aU;
    F.h_tilesT[(size_t)l] = (int32_t)aT;
    F.h_tilesU[(size_t)l] = (int32_t)aU;
    F.h_tilesB[(size_t)l] = (int32_t)aB;
    F.lev_big_ptr[(size_t)l + 1] = (int32_t)big_sn.size();
    F.max_big_tiles = std::max(F.max_big_tiles, aB);
    (void)bbase;
  }
  F.h_preU = preU;
  F.h_preUF = preUF;
  F.h_preT = preT;
  // transposed row lists (counting sort of the entries of `rows` by value; per column first the entries of bottom-level supernodes,
  // then those of top-level ones, each part in ascending position = ascending source supernode)
  if (rows.size() >= (size_t)0x7fffffff) return false;
  F.nrows_total = (int64_t)rows.size();
  decide_top_levels(F);
  {
    std::vector<int64_t> tptr((size_t)n + 1, 0), tmid((size_t)n, 0);
    for (int32_t s = 0; s < F.nsn; ++s)
      for (int64_t q = rptr[(size_t)s]; q < rptr[(size_t)s + 1]; ++q) {
        tptr[(size_t)rows[(size_t)q] + 1]++;
        if (level[(size_t)s] < F.ltop) tmid[(size_t)rows[(size_t)q]]++;
      }
    for (int64_t c = 0; c < n; ++c) tptr[(size_t)c + 1] += tptr[(size_t)c];
    for (int64_t c = 0; c < n; ++c) tmid[(size_t)c] += tptr[(size_t)c];
    std::vector<int32_t> tidx(rows.size());
    std::vector<int64_t> fill_lo(tptr.begin(), tptr.end() - 1), fill_hi(tmid);
    for (int32_t s = 0; s < F.nsn; ++s)
      for (int64_t q = rptr[(size_t)s]; q < rptr[(size_t)s + 1]; ++q) {
        const int32_t r = rows[(size_t)q];
        if (level[(size_t)s] < F.ltop) tidx[(size_t)fill_lo[(size_t)r]++] = (int32_t)q;
        else tidx[(size_t)fill_hi[(size_t)r]++] = (int32_t)q;
      }
    std::vector<int32_t> tpos(rows.size());
    for (size_t k = 0; k < tidx.size(); ++k) tpos[(size_t)tidx[k]] = (int32_t)k;
    if (!up(tptr, F.d_tptr) || !up(tmid, F.d_tmid) || !up(tidx, F.d_tidx) || !up(tpos, F.d_tpos)) return false;
  }
  bool ok = up(first, F.d_first) && up(nrow, F.d_nrow) && up(rows, F.d_rows) && up(sn_of_col, F.d_sn_of_col) && up(iperm, F.d_iperm) && up(F.h_perm, F.d_perm) &&
            up(rptr, F.d_rptr) && up(pptr, F.d_pptr) && up(lev_sn, F.d_lev_sn) && up(preT, F.d_preT) && up(preU, F.d_preU) && up(big_sn, F.d_big_sn) &&
            up(big_index, F.d_big_index) && up(preB, F.d_preB);
  if (!ok) return false;
  if (F.d_err.alloc(32) != hipSuccess || hipMemset(F.d_err, 0, 128) != hipSuccess) return false;
  if (F.d_panels.alloc(F.entries) != hipSuccess) return false;
  if (lu) {
    if (!up(uptr, F.d_uptr) || !up(preUF, F.d_preUF)) return false;
    if (F.d_upanels.alloc(F.uentries) != hipSuccess) return false;
    if (F.d_piv.alloc(n) != hipSuccess) return false;
  }
  if (!build_top_plan(F, lev_sn, nrow, first)) return false;
  F.h_first = first;
  if (!build_chains(F, n, level, first, nrow, rptr, rows, parent_g) || !upload_chains(F)) return false;
  F.M.nsn = F.nsn;
  F.M.first = F.d_first;
  F.M.nrow = F.d_nrow;
  F.M.rptr = F.d_rptr;
  F.M.rows = F.d_rows;
  F.M.pptr = F.d_pptr;
  F.M.sn_of_col = F.d_sn_of_col;
  F.M.tptr = F.d_tptr;
  F.M.tmid = F.d_tmid;
  F.M.tidx = F.d_tidx;
  F.M.tpos = F.d_tpos;
  F.M.panels = F.d_panels;
  F.M.upanels = F.d_upanels;
  F.M.uptr = F.d_uptr;
  F.M.piv = F.d_piv;
  return true;
}

// numeric factorisation of the matrix (device CSR, original numbering); *bad = supernode + 1 whose diagonal block was not positive definite
// tiny: replacement of a vanishing pivot column in the L U variant; *perturbed: how many were replaced
static inline hipError_t factorize(Factor &F, hipStream_t st, const int64_t *d_rp, const int32_t *d_ci, const double *d_va, unsigned *bad, double tiny = 0.0,
                                   unsigned *perturbed = nullptr)
{
  hipError_t e = hipMemsetAsync(F.d_panels, 0, sizeof(double) * (size_t)std::max<int64_t>(F.entries, 1), st);
  if (e != hipSuccess) return e;
  (void)hipMemsetAsync(F.d_err, 0, 16, st);
  if (F.lu) {
    e = hipMemsetAsync(F.d_upanels, 0, sizeof(double) * (size_t)std::max<int64_t>(F.uentries, 1), st);
    if (e != hipSuccess) return e;
  }
  if (F.n > 0) {
    if (F.lu) hipLaunchKernelGGL(k_sn_assemble_lu, dim3((unsigned)((F.n + 255) / 256)), dim3(256), 0, st, F.M, F.n, d_rp, d_ci, d_va, F.d_iperm);
    else hipLaunchKernelGGL(k_sn_assemble, dim3((unsigned)((F.n + 255) / 256)), dim3(256), 0, st, F.M, F.n, d_rp, d_ci, d_va, F.d_iperm);
  }
  static DeviceOnce attr_once;
  attr_once.run([]() {
    (void)hipFuncSetAttribute((const void *)k_sn_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (SN_MAX_COLS + 1) * SN_MAX_COLS * 8);
    (void)hipFuncSetAttribute((const void *)k_sn_lu_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (SN_MAX_COLS + 1) * SN_MAX_COLS * 8);
  });
  for (int32_t l = 0; l < F.nlev; ++l) {
    const int32_t cnt = F.lev_ptr[(size_t)l + 1] - F.lev_ptr[(size_t)l];
    if (cnt == 0) continue;
    const int32_t *lsn = F.d_lev_sn + F.lev_ptr[(size_t)l];
    const int nc = F.lev_maxnc[(size_t)l];
    if (F.lu) {
      hipLaunchKernelGGL(k_sn_lu_diag, dim3((unsigned)cnt), dim3(256), (size_t)(nc | 1) * nc * 8, st, F.M, lsn, F.d_err, tiny);
      if (F.h_tilesT[(size_t)l] > 0)
        hipLaunchKernelGGL(k_sn_lu_panel, dim3((unsigned)F.h_tilesT[(size_t)l]), dim3(256), 0, st, F.M, lsn, (const int32_t *)(F.d_preT + F.lev_ptr[(size_t)l] + l), cnt);
      for (int32_t ph = F.lev_phase_ptr[(size_t)l]; ph + 1 < F.lev_phase_ptr[(size_t)l + 1]; ++ph) { // colour by colour
        const int32_t b0 = F.h_preUF[(size_t)(F.lev_ptr[(size_t)l] + l + F.phase_k[(size_t)ph])], b1 = F.h_preUF[(size_t)(F.lev_ptr[(size_t)l] + l + F.phase_k[(size_t)ph + 1])];
        if (b1 > b0) hipLaunchKernelGGL(k_sn_lu_update, dim3((unsigned)(b1 - b0)), dim3(256), 0, st, F.M, lsn, (const int32_t *)(F.d_preUF + F.lev_ptr[(size_t)l] + l), cnt, (int)b0);
      }
      continue;
    }
    hipLaunchKernelGGL(k_sn_diag, dim3((unsigned)cnt), dim3(256), (size_t)(nc | 1) * nc * 8, st, F.M, lsn, F.d_err);
    if (F.h_tilesT[(size_t)l] > 0)
      hipLaunchKernelGGL(k_sn_panel, dim3((unsigned)F.h_tilesT[(size_t)l]), dim3(256), 0, st, F.M, lsn, (const int32_t *)(F.d_preT + F.lev_ptr[(size_t)l] + l), cnt);
    for (int32_t ph = F.lev_phase_ptr[(size_t)l]; ph + 1 < F.lev_phase_ptr[(size_t)l + 1]; ++ph) { // colour by colour
      const int32_t b0 = F.h_preU[(size_t)(F.lev_ptr[(size_t)l] + l + F.phase_k[(size_t)ph])], b1 = F.h_preU[(size_t)(F.lev_ptr[(size_t)l] + l + F.phase_k[(size_t)ph + 1])];
      if (b1 > b0) hipLaunchKernelGGL(k_sn_update, dim3((unsigned)(b1 - b0)), dim3(256), 0, st, F.M, lsn, (const int32_t *)(F.d_preU + F.lev_ptr[(size_t)l] + l), cnt, (int)b0);
    }
  }
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  unsigned words[4] = {0, 0, 0, 0};
  e = hipMemcpy(words, F.d_err, 16, hipMemcpyDeviceToHost);
  *bad = words[0];
  if (perturbed) *perturbed = words[2];
  const auto t0 = std::chrono::steady_clock::now();
  if (e == hipSuccess && words[0] == 0) e = chain_setup(F, st); // the dense inverses of the top chains (single-vector solves)
  F.chain_setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return e;
}

// scratch of the backward sweep for m right-hand sides (call OUTSIDE a stream capture)
static inline bool reserve(Factor &F, int m)
{
  const int64_t cneed = F.nrows_total; // slots of the single-vector forward sweep (the block solves push coloured updates)
  if (cneed > F.contrib_cap) {
    F.contrib_cap = 0;
    if (F.d_contrib.alloc(cneed) != hipSuccess) return false;
    F.contrib_cap = cneed;
  }
  const int64_t need = F.max_big_tiles * SN_MAX_COLS * (int64_t)m;
  if (need <= F.partial_cap) return true;
  F.partial_cap = 0;
  if (F.d_partial.alloc(need) != hipSuccess) return false;
  F.partial_cap = need;
  return true;
}

template <bool LU>
static inline void solve_t(const Factor &F, hipStream_t st, int m, double *B, int64_t ldb, double *Yvec, unsigned *err)
{
  if (m == 1 && ldb == 1 && Yvec) { // the single-vector kernels (sn_solve1.hpp): level launches at the bottom, one persistent launch for the top
    const int32_t lbot = F.ntop > 0 ? F.ltop : F.nlev; // levels [0, lbot) by launches
    const char *sk = std::getenv("DDM_SN_SMALL_KERNELS");
    const bool small_kernels = !(sk && sk[0] == '0');
    for (int32_t l = 0; l < lbot; ++l) {
      const int32_t cnt = F.lev_ptr[(size_t)l + 1] - F.lev_ptr[(size_t)l];
      if (cnt == 0) continue;
      const int32_t *lsn = F.d_lev_sn + F.lev_ptr[(size_t)l], *preT = F.d_preT + F.lev_ptr[(size_t)l] + l;
      const unsigned grid = (unsigned)(F.h_tilesT[(size_t)l] + cnt);
      if (F.lev_maxnc[(size_t)l] <= 64 && F.lev_maxnr[(size_t)l] <= 192 && small_kernels) // a wavefront per supernode
        hipLaunchKernelGGL(k_sn_fwd1_small<LU>, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, st, F.M, lsn, cnt, (const double *)B, Yvec, F.d_contrib);
      else if (F.lev_maxnc[(size_t)l] <= 64) hipLaunchKernelGGL((k_sn_fwd1<LU, 64>), dim3(grid), dim3(256), 0, st, F.M, lsn, preT, cnt, (const double *)B, Yvec, F.d_contrib);
      else hipLaunchKernelGGL((k_sn_fwd1<LU, 128>), dim3(grid), dim3(512), 0, st, F.M, lsn, preT, cnt, (const double *)B, Yvec, F.d_contrib);
    }
    if (F.ntop > 0 && F.chains_ready) {
      hipLaunchKernelGGL(k_sn_top_prologue, dim3(1), dim3(64), 0, st, F.d_top_sync);
      hipLaunchKernelGGL(k_sn_top_chain<LU>, dim3((unsigned)F.chain_grid), dim3(TOP_THREADS), (size_t)F.ch.max_vec * 8, st, F.M, F.chd, F.chp, F.nblocks, F.top_spread, B, Yvec,
                         (const double *)F.d_contrib, F.d_top_sync, F.d_top_flags, err ? err : F.d_err + 1, F.d_top_stamps);
    } else if (F.ntop > 0) {
      hipLaunchKernelGGL(k_sn_top_prologue, dim3(1), dim3(64), 0, st, F.d_top_sync);
      hipLaunchKernelGGL(k_sn_top1<LU>, dim3((unsigned)F.top_grid), dim3(TOP_THREADS), 0, st, F.M, F.top, F.nblocks, F.top_spread, B, Yvec, F.d_contrib, F.d_top_partial,
                         F.d_top_sync, F.d_top_flags, err ? err : F.d_err + 1, F.d_top_stamps);
    }
    for (int32_t l = lbot - 1; l >= 0; --l) {
      const int32_t cnt = F.lev_ptr[(size_t)l + 1] - F.lev_ptr[(size_t)l];
      if (cnt == 0) continue;
      const int32_t *lsn = F.d_lev_sn + F.lev_ptr[(size_t)l];
      const int32_t nbig = F.lev_big_ptr[(size_t)l + 1] - F.lev_big_ptr[(size_t)l];
      const int32_t *preB = F.d_preB + F.lev_big_ptr[(size_t)l] + l, *bsn = F.d_big_sn + F.lev_big_ptr[(size_t)l], *bidx = F.d_big_index + F.lev_ptr[(size_t)l];
      const bool small = F.lev_maxnc[(size_t)l] <= 64;
      if (small && F.lev_maxnr[(size_t)l] <= 192 && small_kernels) {
        hipLaunchKernelGGL(k_sn_bwd1_small<LU>, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, st, F.M, lsn, cnt, (const double *)Yvec, B);
        continue;
      }
      if (nbig > 0) {
        if (small) hipLaunchKernelGGL((k_sn_bwd1_partial<LU, 64>), dim3((unsigned)F.h_tilesB[(size_t)l]), dim3(256), 0, st, F.M, bsn, preB, nbig, (const double *)B, F.d_partial);
        else hipLaunchKernelGGL((k_sn_bwd1_partial<LU, 128>), dim3((unsigned)F.h_tilesB[(size_t)l]), dim3(512), 0, st, F.M, bsn, preB, nbig, (const double *)B, F.d_partial);
      }
      if (small) hipLaunchKernelGGL((k_sn_bwd1_diag<LU, 64>), dim3((unsigned)cnt), dim3(256), 0, st, F.M, lsn, bidx, preB, (const double *)F.d_partial, (const double *)Yvec, B);
      else hipLaunchKernelGGL((k_sn_bwd1_diag<LU, 128>), dim3((unsigned)cnt), dim3(512), 0, st, F.M, lsn, bidx, preB, (const double *)F.d_partial, (const double *)Yvec, B);
    }
    return;
  }
  static DeviceOnce attr_once; // (one per instantiation: LU / Cholesky)
  attr_once.run([]() {
    (void)hipFuncSetAttribute((const void *)k_sn_fwd_diag<LU>, hipFuncAttributeMaxDynamicSharedMemorySize, SN_MAX_COLS * 48 * 8);
    (void)hipFuncSetAttribute((const void *)k_sn_fwd_update, hipFuncAttributeMaxDynamicSharedMemorySize, SN_MAX_COLS * 48 * 8);
    (void)hipFuncSetAttribute((const void *)k_sn_bwd_diag<LU>, hipFuncAttributeMaxDynamicSharedMemorySize, (SN_MAX_COLS + TILE) * 48 * 8);
  });
  const int mpad = ((m + 15) / 16) * 16;
  for (int32_t l = 0; l < F.nlev; ++l) {
    const int32_t cnt = F.lev_ptr[(size_t)l + 1] - F.lev_ptr[(size_t)l];
    if (cnt == 0) continue;
    const int32_t *lsn = F.d_lev_sn + F.lev_ptr[(size_t)l];
    const size_t lds = (size_t)F.lev_maxnc[(size_t)l] * mpad * 8;
    hipLaunchKernelGGL(k_sn_fwd_diag<LU>, dim3((unsigned)cnt), dim3(256), lds, st, F.M, lsn, m, B, ldb);
    for (int32_t ph = F.lev_phase_ptr[(size_t)l]; ph + 1 < F.lev_phase_ptr[(size_t)l + 1]; ++ph) { // colour by colour
      const int32_t b0 = F.h_preT[(size_t)(F.lev_ptr[(size_t)l] + l + F.phase_k[(size_t)ph])], b1 = F.h_preT[(size_t)(F.lev_ptr[(size_t)l] + l + F.phase_k[(size_t)ph + 1])];
      if (b1 > b0)
        hipLaunchKernelGGL(k_sn_fwd_update, dim3((unsigned)(b1 - b0)), dim3(256), lds, st, F.M, lsn, (const int32_t *)(F.d_preT + F.lev_ptr[(size_t)l] + l), cnt, m, B, ldb, (int)b0);
    }
  }
  for (int32_t l = F.nlev - 1; l >= 0; --l) {
    const int32_t cnt = F.lev_ptr[(size_t)l + 1] - F.lev_ptr[(size_t)l];
    if (cnt == 0) continue;
    const int32_t *lsn = F.d_lev_sn + F.lev_ptr[(size_t)l];
    const int32_t nbig = F.lev_big_ptr[(size_t)l + 1] - F.lev_big_ptr[(size_t)l];
    const int32_t *preB = F.d_preB + F.lev_big_ptr[(size_t)l] + l;
    if (nbig > 0)
      hipLaunchKernelGGL(k_sn_bwd_partial<LU>, dim3((unsigned)F.h_tilesB[(size_t)l]), dim3(256), (size_t)TILE * mpad * 8, st, F.M, (const int32_t *)(F.d_big_sn + F.lev_big_ptr[(size_t)l]),
                         preB, nbig, m, (const double *)B, ldb, F.d_partial);
    hipLaunchKernelGGL(k_sn_bwd_diag<LU>, dim3((unsigned)cnt), dim3(256), (size_t)(F.lev_maxnc[(size_t)l] + TILE) * mpad * 8, st, F.M, lsn,
                       (const int32_t *)(F.d_big_index + F.lev_ptr[(size_t)l]), preB, (const double *)F.d_partial, m, B, ldb);
  }
}

// in-place solve (L L^T resp. P^T L U) X = B on the permuted row-major work block (n x m, leading dimension ldb); enqueues only
// Yvec: a second n-vector for the single-vector kernels (m == 1), or nullptr = the block kernels
// err: status word of the persistent single-vector kernel (a device-visible word the caller watches; nullptr: the factor's own)
static inline void solve(const Factor &F, hipStream_t st, int m, double *B, int64_t ldb, double *Yvec = nullptr, unsigned *err = nullptr)
{
  if (F.lu) solve_t<true>(F, st, m, B, ldb, Yvec, err);
  else solve_t<false>(F, st, m, B, ldb, Yvec, err);
}

} // namespace sn
