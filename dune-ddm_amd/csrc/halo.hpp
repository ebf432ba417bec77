// Halo exchange (struct ddm_halo) for one vector and for a row-major block of m columns.  Both pack on the device, exchange over the
// in-library RCCL wire (halo_wire_rccl, shared), the caller's all-to-all callback, or nothing at all on a single rank, and unpack.
// Needs context.hpp.
#pragma once

// ---- halo --------------------------------------------------------------------------------------
struct ddm_halo {
  int tag = 0, mode = 0;
  int64_t nsend = 0, nrecv = 0, ndst = 0, self_off_send = 0, self_off_recv = 0, self_count = 0;
  dbuf<int64_t> send_idx, dst_idx, dst_ptr, src_pos;
  dbuf<double> sendbuf, recvbuf;
  bool remote = false; // any traffic to/from other ranks
  std::vector<int64_t> send_counts, recv_counts; // per peer (the layout of sendbuf / recvbuf)
  dbuf<double> msend, mrecv; // multi-RHS buffers (m x the single-vector layout), mcols columns
  int mcols = 0;
  std::vector<int64_t> h_send_idx, h_dst_idx, h_dst_ptr, h_src_pos; // the plan on the host: local_maps_build composes it
};

// ---- rank-local plans composed with the extension map --------------------------------------------
// Where every copy of every overlap row lives on this rank, an exchange is pack -> unpack over the one buffer (src_pos indexes the
// send buffer), and a Schwarz apply's two exchanges compose with k_extend / k_restrict into index tables:
//   src_of[i]  row of the non-overlapping defect that row i of the overlapping one holds after k_extend and the copy exchange
//              (k_unpack<false>: the last source of a destination's list wins), or -1 where it holds 0.0
//   own_of[m]  the overlapping row k_restrict<false, false> reads for non-overlapping row m
//   cp_ptr / cp_idx (CSR over m)  the overlapping rows k_unpack<true> adds into own_of[m], in its order
// Host arrays only; a null plan (copy / add) is an exchange that does nothing.
struct HaloPlanHost {
  int64_t nsend = 0, ndst = 0;
  const int64_t *send_idx = nullptr, *dst_idx = nullptr, *dst_ptr = nullptr, *src_pos = nullptr;
};
struct LocalMapsHost {
  std::vector<int32_t> src_of, own_of, cp_ptr, cp_idx;
};
// false: the tables do not exist (an index out of range, a non-overlapping row with no or several images, a destination listed twice,
// more copies than an int32 counts): the caller keeps the kernels of the general path
static bool local_maps_build(int64_t n, int64_t n_novlp, const int32_t *ext_map, const HaloPlanHost &copy, const HaloPlanHost &add, LocalMapsHost &M)
{
  if (n < 0 || n_novlp < 0 || n > INT32_MAX || n_novlp > INT32_MAX) return false;
  auto plan_ok = [n](const HaloPlanHost &P) {
    for (int64_t j = 0; j < P.nsend; ++j)
      if (P.send_idx[j] < 0 || P.send_idx[j] >= n) return false;
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int64_t t = 0; t < P.ndst; ++t) {
      const int64_t i = P.dst_idx[t];
      if (i < 0 || i >= n || seen[(size_t)i] || P.dst_ptr[t] > P.dst_ptr[t + 1]) return false;
      seen[(size_t)i] = 1;
      for (int64_t k = P.dst_ptr[t]; k < P.dst_ptr[t + 1]; ++k)
        if (P.src_pos[k] < 0 || P.src_pos[k] >= P.nsend) return false;
    }
    return true;
  };
  if (!plan_ok(copy) || !plan_ok(add)) return false;
  M.src_of.assign(ext_map, ext_map + n);
  for (int64_t t = 0; t < copy.ndst; ++t) { // (the pack reads the extended defect before any destination is written)
    const int64_t k0 = copy.dst_ptr[t], k1 = copy.dst_ptr[t + 1];
    M.src_of[(size_t)copy.dst_idx[t]] = k1 > k0 ? ext_map[copy.send_idx[copy.src_pos[k1 - 1]]] : -1;
  }
  M.own_of.assign((size_t)n_novlp, -1);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t m = ext_map[i];
    if (m < 0) continue;
    if (m >= n_novlp || M.own_of[(size_t)m] >= 0) return false;
    M.own_of[(size_t)m] = (int32_t)i;
  }
  std::vector<int64_t> dst_of((size_t)n, -1); // overlapping row -> its place in the add plan's destination list
  for (int64_t t = 0; t < add.ndst; ++t) dst_of[(size_t)add.dst_idx[t]] = t;
  M.cp_ptr.assign((size_t)n_novlp + 1, 0);
  M.cp_idx.clear();
  for (int64_t m = 0; m < n_novlp; ++m) {
    if (M.own_of[(size_t)m] < 0) return false;
    const int64_t t = dst_of[(size_t)M.own_of[(size_t)m]];
    if (t >= 0)
      for (int64_t k = add.dst_ptr[t]; k < add.dst_ptr[t + 1]; ++k) M.cp_idx.push_back((int32_t)add.send_idx[add.src_pos[k]]);
    if (M.cp_idx.size() > (size_t)INT32_MAX) return false;
    M.cp_ptr[(size_t)m + 1] = (int32_t)M.cp_idx.size();
  }
  return true;
}
// The tables for a test: counts[0] = 1 and counts[1] = entries of cp_idx where they exist (cp_idx holds max_cp entries at most),
// counts[0] = 0 where they do not.  Host only, no device needed.
extern "C" int ddm_local_maps_host(int64_t n, int64_t n_novlp, const int32_t *ext_map, int64_t copy_nsend, const int64_t *copy_send_idx, int64_t copy_ndst,
                                   const int64_t *copy_dst_idx, const int64_t *copy_dst_ptr, const int64_t *copy_src_pos, int64_t add_nsend,
                                   const int64_t *add_send_idx, int64_t add_ndst, const int64_t *add_dst_idx, const int64_t *add_dst_ptr,
                                   const int64_t *add_src_pos, int32_t *src_of, int32_t *own_of, int32_t *cp_ptr, int64_t max_cp, int32_t *cp_idx, int64_t *counts)
{
  if (!ext_map || !src_of || !own_of || !cp_ptr || !counts || (max_cp > 0 && !cp_idx)) return DDM_EINVAL;
  const HaloPlanHost copy{copy_nsend, copy_ndst, copy_send_idx, copy_dst_idx, copy_dst_ptr, copy_src_pos};
  const HaloPlanHost add{add_nsend, add_ndst, add_send_idx, add_dst_idx, add_dst_ptr, add_src_pos};
  LocalMapsHost M;
  counts[0] = counts[1] = 0;
  if (!local_maps_build(n, n_novlp, ext_map, copy, add, M)) return DDM_OK;
  if ((int64_t)M.cp_idx.size() > max_cp) return DDM_EINVAL;
  std::copy(M.src_of.begin(), M.src_of.end(), src_of);
  std::copy(M.own_of.begin(), M.own_of.end(), own_of);
  std::copy(M.cp_ptr.begin(), M.cp_ptr.end(), cp_ptr);
  std::copy(M.cp_idx.begin(), M.cp_idx.end(), cp_idx);
  counts[0] = 1;
  counts[1] = (int64_t)M.cp_idx.size();
  return DDM_OK;
}

extern "C" int ddm_halo_create(ddm_ctx *ctx, int tag, int mode, int64_t nsend, const int64_t *send_idx,
                               const int64_t *send_counts, const int64_t *recv_counts, int64_t ndst, const int64_t *dst_idx,
                               const int64_t *dst_ptr, const int64_t *src_pos, ddm_halo **out)
{
  if (!ctx || !out || (mode != 0 && mode != 1)) return fail(ctx, DDM_EINVAL, "ddm_halo_create: bad arguments");
  auto H = std::make_unique<ddm_halo>();
  H->tag = tag;
  H->mode = mode;
  H->nsend = nsend;
  H->ndst = ndst;
  H->send_counts.assign(send_counts, send_counts + ctx->nranks);
  H->recv_counts.assign(recv_counts, recv_counts + ctx->nranks);
  int64_t ssum = 0, rsum = 0;
  for (int r = 0; r < ctx->nranks; ++r) {
    if (r == ctx->rank) {
      H->self_off_send = ssum;
      H->self_off_recv = rsum;
      H->self_count = send_counts[r];
      if (send_counts[r] != recv_counts[r]) return fail(ctx, DDM_EINVAL, "halo: self send/recv counts differ");
    } else if (send_counts[r] || recv_counts[r])
      H->remote = true;
    ssum += send_counts[r];
    rsum += recv_counts[r];
  }
  if (ssum != nsend) return fail(ctx, DDM_EINVAL, "halo: send_counts do not sum to nsend");
  H->nrecv = rsum;
  const int64_t nsrc = ndst > 0 ? dst_ptr[ndst] : 0;
  for (int64_t k = 0; k < nsrc; ++k)
    if (src_pos[k] < 0 || src_pos[k] >= rsum) return fail(ctx, DDM_EINVAL, "halo: src_pos out of range");
  H->h_send_idx.assign(send_idx, send_idx + nsend);
  H->h_dst_idx.assign(dst_idx, dst_idx + ndst);
  if (ndst > 0) H->h_dst_ptr.assign(dst_ptr, dst_ptr + ndst + 1);
  H->h_src_pos.assign(src_pos, src_pos + nsrc);
  int rc = upload(ctx, send_idx, nsend, H->send_idx);
  if (!rc) rc = upload(ctx, dst_idx, ndst, H->dst_idx);
  if (!rc) rc = upload(ctx, dst_ptr, ndst + 1, H->dst_ptr);
  if (!rc) rc = upload(ctx, src_pos, nsrc, H->src_pos);
  if (!rc && H->sendbuf.alloc(nsend) != hipSuccess) rc = DDM_EHIP;
  if (!rc && H->recvbuf.alloc(rsum) != hipSuccess) rc = DDM_EHIP;
  if (rc) return fail(ctx, rc, "halo: device allocation failed");
  *out = H.release();
  return DDM_OK;
}
extern "C" void ddm_halo_destroy(ddm_halo *H) { delete H; }
extern "C" double *ddm_halo_sendbuf(ddm_halo *H) { return H->sendbuf; }
extern "C" double *ddm_halo_recvbuf(ddm_halo *H) { return H->recvbuf; }

// In-library exchange of m interleaved columns (m = 1: one vector): one grouped point-to-point exchange on the context's stream (xGMI
// links are point-to-point: every peer pair is its own transfer); the self segment stays a device copy unless the self test routes it too
static int halo_wire_rccl(ddm_ctx *ctx, const ddm_halo *H, int64_t m, const double *send, double *recv)
{
  if (H->self_count > 0 && !ctx->rccl_self)
    HIPCHECK(ctx, hipMemcpyAsync(recv + H->self_off_recv * m, send + H->self_off_send * m, sizeof(double) * (size_t)(H->self_count * m), hipMemcpyDeviceToDevice, ctx->stream));
  NCCLCHECK(ctx, ctx->nccl.GroupStart());
  int64_t so = 0, ro = 0;
  for (int r = 0; r < ctx->nranks; ++r) {
    const bool self = r == ctx->rank;
    if ((!self || ctx->rccl_self) && H->recv_counts[r] > 0) NCCLCHECK(ctx, ctx->nccl.Recv(recv + ro * m, (size_t)(H->recv_counts[r] * m), ncclDouble, r, ctx->rccl_comm, ctx->stream));
    if ((!self || ctx->rccl_self) && H->send_counts[r] > 0) NCCLCHECK(ctx, ctx->nccl.Send(send + so * m, (size_t)(H->send_counts[r] * m), ncclDouble, r, ctx->rccl_comm, ctx->stream));
    so += H->send_counts[r];
    ro += H->recv_counts[r];
  }
  NCCLCHECK(ctx, ctx->nccl.GroupEnd());
  return DDM_OK;
}

// ---- one vector ----------------------------------------------------------------------------------
static int halo_exchange_impl(ddm_ctx *ctx, ddm_halo *H, const double *src, double *v)
{
  if (!H) return DDM_OK;
  if (H->nsend == 0 && H->ndst == 0 && !H->remote) return DDM_OK;
  if (H->nsend > 0) hipLaunchKernelGGL(k_pack, dim3(grid_for(H->nsend)), dim3(WG), 0, ctx->stream, H->nsend, H->send_idx, src, H->sendbuf);
  const double *rbuf = H->recvbuf;
  ctx->n_halo_groups += 1;
  if (ctx->rccl && (ctx->nranks > 1 || ctx->rccl_self)) {
    DDMCHECK(halo_wire_rccl(ctx, H, 1, H->sendbuf, H->recvbuf));
  } else if (ctx->nranks > 1) {
    if (!ctx->a2a) return fail(ctx, DDM_ECOMM, "multi-rank context without an exchange (ddm_ctx_set_rccl / ddm_ctx_set_comm)");
    if (ctx->a2a(ctx->user, H->tag, H->sendbuf, H->recvbuf) != 0) return fail(ctx, DDM_ECOMM, "alltoall callback failed (tag %d)", H->tag);
  } else {
    rbuf = H->sendbuf; // single rank: the self segment is the whole buffer
  }
  if (H->ndst > 0) {
    if (H->mode == 1)
      hipLaunchKernelGGL(k_unpack<true>, dim3(grid_for(H->ndst)), dim3(WG), 0, ctx->stream, H->ndst, H->dst_idx, H->dst_ptr, H->src_pos, rbuf, v);
    else
      hipLaunchKernelGGL(k_unpack<false>, dim3(grid_for(H->ndst)), dim3(WG), 0, ctx->stream, H->ndst, H->dst_idx, H->dst_ptr, H->src_pos, rbuf, v);
  }
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
// an exchange over H moves nothing between ranks and goes through no transport: halo_exchange_impl is pack -> unpack over sendbuf
static bool halo_is_local(const ddm_ctx *ctx, const ddm_halo *H)
{
  if (!H) return true;
  return !H->remote && !ctx->rccl_self && (ctx->nranks == 1 || ctx->rccl);
}
// what halo_exchange_impl adds to the context's exchange count, for a caller that does a local exchange's work in a kernel of its own
static void halo_count_local(ddm_ctx *ctx, const ddm_halo *H)
{
  if (H && (H->nsend != 0 || H->ndst != 0 || H->remote)) ctx->n_halo_groups += 1;
}
static HaloPlanHost halo_plan_host(const ddm_halo *H)
{
  if (!H) return HaloPlanHost{};
  return HaloPlanHost{H->nsend, H->ndst, H->h_send_idx.data(), H->h_dst_idx.data(), H->h_dst_ptr.data(), H->h_src_pos.data()};
}
extern "C" int ddm_halo_exchange(ddm_ctx *ctx, ddm_halo *H, double *v) { return halo_exchange_impl(ctx, H, v, v); }
extern "C" int ddm_halo_exchange_to(ddm_ctx *ctx, ddm_halo *H, const double *src, double *dst)
{
  if (!src || !dst) return fail(ctx, DDM_EINVAL, "ddm_halo_exchange_to: bad arguments");
  return halo_exchange_impl(ctx, H, src, dst);
}

// ---- m columns -----------------------------------------------------------------------------------
// In-library exchange (RCCL) and a single rank: one message of m x count doubles per peer.  Callback exchange: the callback's buffers
// and counts are fixed at ddm_halo_create, so the block is exchanged column by column through the unchanged callback.
static int halo_exchange_multi(ddm_ctx *ctx, ddm_halo *H, int m, double *v)
{
  if (!H) return DDM_OK;
  if (H->nsend == 0 && H->ndst == 0 && !H->remote) return DDM_OK;
  HIPCHECK(ctx, reserve_cols<double>(H->mcols, m, {{H->msend, H->nsend}, {H->mrecv, H->nrecv}}));
  if (H->nsend > 0) hipLaunchKernelGGL(k_pack_multi, dim3(grid_for(H->nsend * m)), dim3(WG), 0, ctx->stream, H->nsend, m, H->send_idx, (const double *)v, H->msend);
  const double *rbuf = H->mrecv;
  if (ctx->rccl && (ctx->nranks > 1 || ctx->rccl_self)) {
    ctx->n_halo_groups += 1;
    DDMCHECK(halo_wire_rccl(ctx, H, m, H->msend, H->mrecv));
  } else if (ctx->nranks > 1) {
    if (!ctx->a2a) return fail(ctx, DDM_ECOMM, "multi-rank context without an exchange (ddm_ctx_set_rccl / ddm_ctx_set_comm)");
    for (int c = 0; c < m; ++c) {
      ctx->n_halo_groups += 1;
      if (H->nsend > 0)
        hipLaunchKernelGGL(k_column_copy<false>, dim3(grid_for(H->nsend)), dim3(WG), 0, ctx->stream, H->nsend, m, c, (const double *)H->msend, H->sendbuf);
      if (ctx->a2a(ctx->user, H->tag, H->sendbuf, H->recvbuf) != 0) return fail(ctx, DDM_ECOMM, "alltoall callback failed (tag %d, column %d)", H->tag, c);
      if (H->nrecv > 0)
        hipLaunchKernelGGL(k_column_copy<true>, dim3(grid_for(H->nrecv)), dim3(WG), 0, ctx->stream, H->nrecv, m, c, (const double *)H->recvbuf, H->mrecv);
    }
  } else {
    ctx->n_halo_groups += 1;
    rbuf = H->msend; // single rank: the self segment is the whole buffer
  }
  if (H->ndst > 0) {
    if (H->mode == 1)
      hipLaunchKernelGGL(k_unpack_multi<true>, dim3(grid_for(H->ndst * m)), dim3(WG), 0, ctx->stream, H->ndst, m, H->dst_idx, H->dst_ptr, H->src_pos, rbuf, v);
    else
      hipLaunchKernelGGL(k_unpack_multi<false>, dim3(grid_for(H->ndst * m)), dim3(WG), 0, ctx->stream, H->ndst, m, H->dst_idx, H->dst_ptr, H->src_pos, rbuf, v);
  }
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
