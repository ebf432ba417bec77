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
};

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
