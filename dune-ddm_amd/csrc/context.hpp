// The context (struct ddm_ctx) and what every other object reaches the device and the other ranks through: error reporting (fail,
// HIPCHECK / DDMCHECK / NCCLCHECK), grid sizes, uploads (also from background setup threads), HIP-event timers, the RCCL plumbing, the
// all-reduces, and the ddm_ctx_* / ddm_malloc / ddm_memcpy_* / ddm_timing_* entry points.  Included by ddm_hip.hip after the kernels.
#pragma once

struct TimerEntry {
  double ms = 0.0;
  int64_t count = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending; // recorded, not yet resolved (no sync in the hot loop)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;    // recycled event pairs
};

struct ddm_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  int rank = 0, nranks = 1;
  ddm_alltoall_fn a2a = nullptr;
  ddm_allreduce_fn allreduce = nullptr;
  void *user = nullptr;
  // in-library exchange over RCCL (xGMI): ddm_ctx_set_rccl
  struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
  } nccl;
  ncclComm_t rccl_comm = nullptr;
  // collectives of the iteration, counted as a run over several ranks issues them (one count = one RCCL launch: an all-reduce or a
  // grouped send/receive); ddm_ctx_comm_counts
  int64_t n_allreduce = 0, n_allreduce_doubles = 0, n_halo_groups = 0;
  bool rccl = false, rccl_self = false; // rccl_self: route the self segment through RCCL too (single-GPU self test)
  // side stream of the additive combination: the coarse level's restrict / solve / prolong run beside the latency-bound local solve
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  dbuf<double> partial; // RED_MAX_BLOCKS doubles
  dbuf<double> scal;    // SCAL_SLOTS device scalars (the slots SCAL_*, kernels.hpp)
  dbuf<unsigned> ticket; // arrival counter of the one self-finishing reduction in flight on the stream (reduce_finish): 0 between launches
  int num_cu = 256;           // compute units of the device: persistent kernels launch at most this many workgroups
  bool timing = false;
  std::map<std::string, TimerEntry> timers;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_fence = nullptr; // ddm_ctx_fence
  // multi-RHS scratch (ctx_multi_scratch), allocated on first use: dot partials, per-column CG scalars, active-column mask
  dbuf<double> mpartial, mscal;
  dbuf<int32_t> mactive;
};

static std::mutex g_err_mutex;
static thread_local std::string t_last_error;
static int fail(ddm_ctx *ctx, int code, const char *fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  t_last_error = buf;
  if (ctx) { // (setup phases run independent host work on helper threads that may fail at the same time)
    std::lock_guard<std::mutex> lock(g_err_mutex);
    ctx->err = buf;
  }
  return code;
}
// message of the last fail() on the CALLING thread (helper threads report their own failure, not whatever another thread wrote last)
static std::string last_error_of_this_thread() { return t_last_error; }
#define HIPCHECK(ctx, call)                                                                                   \
  do {                                                                                                        \
    hipError_t e_ = (call);                                                                                   \
    if (e_ != hipSuccess) return fail(ctx, DDM_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
#define DDMCHECK(call)            \
  do {                            \
    int rc_ = (call);             \
    if (rc_ != DDM_OK) return rc_; \
  } while (0)

// single-launch triangular solves need every workgroup resident: one workgroup per CU at most
static inline int persistent_grid(const ddm_ctx *ctx) { return std::max(8, std::min(256, ctx->num_cu) / 8 * 8); }

static inline int grid_for(int64_t n, int per_block = WG, int cap = 2048)
{
  int64_t g = (n + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

// Transfers of a BACKGROUND setup thread (the builder of the single-launch engines' schedules runs beside the caller's next setup
// steps): a synchronous hipMemcpy / hipMemset goes through the legacy default stream, and when the caller's stream is that stream and
// is being captured into a graph at that moment (the GenEO block solves capture theirs) the capture is invalidated ("operation failed
// due to a previous error during capture").  The thread therefore moves its data on a non-blocking stream of its own.
static thread_local hipStream_t t_transfer_stream = nullptr;
struct BackgroundTransfers {
  BackgroundTransfers() { (void)hipStreamCreateWithFlags(&t_transfer_stream, hipStreamNonBlocking); }
  ~BackgroundTransfers()
  {
    if (t_transfer_stream) (void)hipStreamDestroy(t_transfer_stream);
    t_transfer_stream = nullptr;
  }
};
template <class T>
static int upload(ddm_ctx *ctx, const T *host, int64_t n, dbuf<T> &dev)
{
  static_assert(std::is_trivially_copyable_v<T>, "uploaded byte by byte: descriptor structs hold views (raw pointers), never owners");
  HIPCHECK(ctx, dev.alloc(n));
  if (n <= 0) return DDM_OK;
  if (t_transfer_stream) { // background setup thread: its own non-blocking stream (see BackgroundTransfers)
    HIPCHECK(ctx, hipMemcpyAsync(dev, host, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, t_transfer_stream));
    HIPCHECK(ctx, hipStreamSynchronize(t_transfer_stream));
  } else
    HIPCHECK(ctx, hipMemcpy(dev, host, sizeof(T) * (size_t)n, hipMemcpyHostToDevice));
  return DDM_OK;
}
// hipMemset that a background setup thread may call (same reason)
static hipError_t dev_memset(void *p, int v, size_t bytes)
{
  if (!t_transfer_stream) return hipMemset(p, v, bytes);
  hipError_t e = hipMemsetAsync(p, v, bytes, t_transfer_stream);
  return e != hipSuccess ? e : hipStreamSynchronize(t_transfer_stream);
}

// HIP-event timer on the context's stream, or on the stream it is given (the side stream).  Nothing synchronises while timing is on:
// the event pairs are resolved (hipEventElapsedTime) when the totals are read, after the stream has drained.
struct ScopedTimer {
  ddm_ctx *ctx;
  hipStream_t stream;
  TimerEntry *t = nullptr;
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  ScopedTimer(ddm_ctx *c, const char *n) : ScopedTimer(c, n, c->stream) {}
  ScopedTimer(ddm_ctx *c, const char *n, hipStream_t s) : ctx(c), stream(s)
  {
    if (!ctx->timing) return;
    t = &ctx->timers[n];
    if (!t->pool.empty()) {
      ev = t->pool.back();
      t->pool.pop_back();
    } else {
      (void)hipEventCreate(&ev.first);
      (void)hipEventCreate(&ev.second);
    }
    (void)hipEventRecord(ev.first, stream);
  }
  ~ScopedTimer()
  {
    if (!t) return;
    (void)hipEventRecord(ev.second, stream);
    t->pending.push_back(ev);
  }
};
static void resolve_timers(ddm_ctx *ctx)
{
  (void)hipStreamSynchronize(ctx->stream);
  for (auto &kv : ctx->timers) {
    for (auto &ev : kv.second.pending) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
        kv.second.ms += ms;
        kv.second.count += 1;
      }
      kv.second.pool.push_back(ev);
    }
    kv.second.pending.clear();
  }
}

// ---- context ---------------------------------------------------------------------------------
extern "C" int ddm_ctx_create(int device, void *hip_stream, ddm_ctx **out)
{
  if (!out) return DDM_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return DDM_EHIP; // no CPU fallback
  if (device < 0 || device >= ndev) return DDM_EINVAL;
  ddm_ctx *ctx = new ddm_ctx;
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess) {
    delete ctx;
    return DDM_EHIP;
  }
  if (hip_stream) ctx->stream = (hipStream_t)hip_stream;
  else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
      delete ctx;
      return DDM_EHIP;
    }
    ctx->own_stream = true;
  }
  if (ctx->partial.alloc(RED_MAX_BLOCKS) != hipSuccess || ctx->scal.alloc(SCAL_SLOTS) != hipSuccess || ctx->ticket.alloc(1) != hipSuccess ||
      hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
    delete ctx;
    return DDM_EHIP;
  }
  (void)hipMemset(ctx->scal, 0, sizeof(double) * SCAL_SLOTS);
  (void)hipMemset(ctx->ticket, 0, sizeof(unsigned));
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ctx->num_cu = prop.multiProcessorCount;
  }
  *out = ctx;
  return DDM_OK;
}

extern "C" void ddm_ctx_destroy(ddm_ctx *ctx)
{
  if (ctx && ctx->side) {
    (void)hipStreamSynchronize(ctx->side);
    (void)hipStreamDestroy(ctx->side);
    (void)hipEventDestroy(ctx->ev_fork);
    (void)hipEventDestroy(ctx->ev_join);
    ctx->side = nullptr;
  }
  if (ctx && ctx->rccl_comm && ctx->nccl.CommDestroy) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx->nccl.CommDestroy(ctx->rccl_comm);
    ctx->rccl_comm = nullptr;
  }
  if (!ctx) return;
  (void)hipStreamSynchronize(ctx->stream); // (before the buffers go: `delete` below releases them)
  if (ctx->ev_fence) (void)hipEventDestroy(ctx->ev_fence);
  (void)hipEventDestroy(ctx->ev0);
  (void)hipEventDestroy(ctx->ev1);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}
extern "C" const char *ddm_last_error(const ddm_ctx *ctx)
{
  if (!ctx) return t_last_error.empty() ? "no context" : t_last_error.c_str();   // context-free entry points: the calling thread's last failure
  static thread_local std::string copy; // (a stable pointer for the caller; ctx->err may be rewritten by a helper thread)
  std::lock_guard<std::mutex> lock(g_err_mutex);
  copy = ctx->err;
  return copy.c_str();
}
extern "C" int ddm_ctx_sync(ddm_ctx *ctx)
{
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DDM_OK;
}
// host waits for the work enqueued on the context's stream SO FAR (an event, not a drain of the stream: work another thread or a
// later call enqueues meanwhile is not waited for, the side stream is left alone) -- what an exchange callback needs before it
// hands the packed buffer to a host-driven transport (MPI)
extern "C" int ddm_ctx_fence(ddm_ctx *ctx)
{
  if (!ctx) return DDM_EINVAL;
  if (!ctx->ev_fence) HIPCHECK(ctx, hipEventCreateWithFlags(&ctx->ev_fence, hipEventDisableTiming));
  HIPCHECK(ctx, hipEventRecord(ctx->ev_fence, ctx->stream));
  HIPCHECK(ctx, hipEventSynchronize(ctx->ev_fence));
  return DDM_OK;
}
extern "C" void *ddm_ctx_stream(ddm_ctx *ctx) { return (void *)ctx->stream; }
extern "C" int ddm_ctx_set_comm(ddm_ctx *ctx, int rank, int nranks, ddm_alltoall_fn a2a, ddm_allreduce_fn allreduce, void *user)
{
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(ctx, DDM_EINVAL, "bad rank %d of %d", rank, nranks);
  if (nranks > 1 && (!a2a || !allreduce)) return fail(ctx, DDM_EINVAL, "multi-rank context needs both callbacks");
  ctx->rank = rank;
  ctx->nranks = nranks;
  ctx->a2a = a2a;
  ctx->allreduce = allreduce;
  ctx->user = user;
  return DDM_OK;
}
// ---- in-library exchange: RCCL over xGMI ------------------------------------------------------------
static void *rccl_open()
{
  for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
    if (void *h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) return h; // an already loaded copy (e.g. the host program's) is reused
  return nullptr;
}
extern "C" int ddm_rccl_unique_id(void *id128)
{
  if (!id128) return DDM_EINVAL;
  void *h = rccl_open();
  if (!h) return DDM_ECOMM;
  auto get = (ncclResult_t(*)(ncclUniqueId *))dlsym(h, "ncclGetUniqueId");
  ncclUniqueId id;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  if (!get || get(&id) != ncclSuccess) return DDM_ECOMM;
  std::memcpy(id128, &id, 128);
  return DDM_OK;
}
extern "C" int ddm_ctx_set_rccl(ddm_ctx *ctx, int rank, int nranks, const void *id128, int self_test)
{
  if (!ctx || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(ctx, DDM_EINVAL, "ddm_ctx_set_rccl: bad rank %d of %d", rank, nranks);
  if (ctx->rccl_comm) return fail(ctx, DDM_EINVAL, "ddm_ctx_set_rccl: the context already has a communicator");
  auto &N = ctx->nccl;
  N.lib = rccl_open();
  if (!N.lib) return fail(ctx, DDM_ECOMM, "librccl.so.1 cannot be loaded: %s", dlerror());
  N.CommInitRank = (decltype(N.CommInitRank))dlsym(N.lib, "ncclCommInitRank");
  N.CommDestroy = (decltype(N.CommDestroy))dlsym(N.lib, "ncclCommDestroy");
  N.GroupStart = (decltype(N.GroupStart))dlsym(N.lib, "ncclGroupStart");
  N.GroupEnd = (decltype(N.GroupEnd))dlsym(N.lib, "ncclGroupEnd");
  N.Send = (decltype(N.Send))dlsym(N.lib, "ncclSend");
  N.Recv = (decltype(N.Recv))dlsym(N.lib, "ncclRecv");
  N.AllReduce = (decltype(N.AllReduce))dlsym(N.lib, "ncclAllReduce");
  N.GetErrorString = (decltype(N.GetErrorString))dlsym(N.lib, "ncclGetErrorString");
  N.CommCount = (decltype(N.CommCount))dlsym(N.lib, "ncclCommCount");
  if (!N.CommInitRank || !N.CommDestroy || !N.GroupStart || !N.GroupEnd || !N.Send || !N.Recv || !N.AllReduce)
    return fail(ctx, DDM_ECOMM, "librccl lacks a required entry point");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  ncclUniqueId id;
  std::memcpy(&id, id128, 128);
  const ncclResult_t r = N.CommInitRank(&ctx->rccl_comm, nranks, id, rank);
  if (r != ncclSuccess) {
    ctx->rccl_comm = nullptr;
    return fail(ctx, DDM_ECOMM, "ncclCommInitRank failed: %s", N.GetErrorString ? N.GetErrorString(r) : "?");
  }
  ctx->rank = rank;
  ctx->nranks = nranks;
  ctx->rccl = true;
  ctx->rccl_self = self_test != 0;
  ctx->a2a = nullptr;
  ctx->allreduce = nullptr;
  return DDM_OK;
}
extern "C" int ddm_ctx_rccl_size(ddm_ctx *ctx, int *count)
{
  if (!ctx || !count) return DDM_EINVAL;
  *count = 0; // no in-library communicator
  if (!ctx->rccl_comm) return DDM_OK;
  if (!ctx->nccl.CommCount) return fail(ctx, DDM_ECOMM, "librccl lacks ncclCommCount");
  const ncclResult_t r = ctx->nccl.CommCount(ctx->rccl_comm, count);
  if (r != ncclSuccess) return fail(ctx, DDM_ECOMM, "ncclCommCount failed: %s", ctx->nccl.GetErrorString ? ctx->nccl.GetErrorString(r) : "?");
  return DDM_OK;
}
#define NCCLCHECK(ctx, call)                                                                                                   \
  do {                                                                                                                         \
    const ncclResult_t r_ = (call);                                                                                            \
    if (r_ != ncclSuccess) return fail(ctx, DDM_ECOMM, "%s failed: %s", #call, ctx->nccl.GetErrorString ? ctx->nccl.GetErrorString(r_) : "?"); \
  } while (0)
// the side stream (and its fork / join events), created on first use: non-blocking, at the DEFAULT priority.  (A stream of the lowest
// priority was measured and loses: with that queue active every kernel boundary of the main stream costs some 40 us more, 5.5 ms per
// iteration of the headline workload against 4.7 ms with this stream and 5.2 ms on one stream -- DESIGN.md section 4.)
static int ctx_side_stream(ddm_ctx *ctx)
{
  if (ctx->side) return DDM_OK;
  hipStream_t s = nullptr;
  HIPCHECK(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming);
  if (e != hipSuccess) {
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    ctx->ev_fork = nullptr;
    (void)hipStreamDestroy(s);
    return fail(ctx, DDM_EHIP, "side stream: hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
  }
  ctx->side = s; // (set last: ddm_ctx_destroy releases the three together)
  return DDM_OK;
}
// in-place sum over all ranks of n doubles at a device pointer, enqueued on `stream`
static int ctx_allreduce(ddm_ctx *ctx, double *buf, int64_t n, const char *what, hipStream_t stream)
{
  ctx->n_allreduce += 1;
  ctx->n_allreduce_doubles += n;
  if (ctx->rccl) {
    if (ctx->nranks > 1 || ctx->rccl_self) NCCLCHECK(ctx, ctx->nccl.AllReduce(buf, buf, (size_t)n, ncclDouble, ncclSum, ctx->rccl_comm, stream));
    return DDM_OK;
  }
  if (ctx->nranks > 1)
    if (ctx->allreduce(ctx->user, buf, n) != 0) return fail(ctx, DDM_ECOMM, "allreduce callback failed (%s)", what);
  return DDM_OK;
}
// ... on the context's stream
static int ctx_allreduce(ddm_ctx *ctx, double *buf, int64_t n, const char *what) { return ctx_allreduce(ctx, buf, n, what, ctx->stream); }

// the coarse defect (K doubles at d0, room for K + 1) summed over the ranks on `stream`; rider, where not null, is a device scalar
// that rides along as element K (one RCCL launch instead of two) and is written back
__global__ void k_copy_scalar(const double *__restrict__ src, double *__restrict__ dst) { *dst = *src; }
static int coarse_allreduce(ddm_ctx *ctx, double *d0, int64_t K, double *rider, hipStream_t stream)
{
  if (!rider) return ctx_allreduce(ctx, d0, K, "coarse defect", stream);
  hipLaunchKernelGGL(k_copy_scalar, dim3(1), dim3(1), 0, stream, (const double *)rider, d0 + K);
  DDMCHECK(ctx_allreduce(ctx, d0, K + 1, "coarse defect + deferred defect norm", stream));
  hipLaunchKernelGGL(k_copy_scalar, dim3(1), dim3(1), 0, stream, (const double *)(d0 + K), rider);
  return DDM_OK;
}
extern "C" int ddm_ctx_comm_counts(ddm_ctx *ctx, int64_t *counts)
{
  if (!ctx || !counts) return DDM_EINVAL;
  counts[0] = ctx->n_allreduce;
  counts[1] = ctx->n_allreduce_doubles;
  counts[2] = ctx->n_halo_groups;
  return DDM_OK;
}

extern "C" int ddm_malloc(ddm_ctx *ctx, int64_t bytes, void **dptr)
{
  dbuf<unsigned char> b;
  HIPCHECK(ctx, b.alloc(std::max<int64_t>(bytes, 8)));
  *dptr = b.release(); // the caller owns it: ddm_free
  return DDM_OK;
}
extern "C" int ddm_free(ddm_ctx *ctx, void *dptr)
{
  HIPCHECK(ctx, dbuf<unsigned char>((unsigned char *)dptr).reset());
  return DDM_OK;
}
extern "C" int ddm_memset_zero(ddm_ctx *ctx, void *dptr, int64_t bytes)
{
  if (!dptr || bytes < 0) return fail(ctx, DDM_EINVAL, "ddm_memset_zero: bad arguments");
  HIPCHECK(ctx, hipMemsetAsync(dptr, 0, (size_t)bytes, ctx->stream));
  return DDM_OK;
}
extern "C" int ddm_memcpy_h2d(ddm_ctx *ctx, void *dst, const void *src, int64_t bytes)
{
  HIPCHECK(ctx, hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DDM_OK;
}
extern "C" int ddm_memcpy_d2h(ddm_ctx *ctx, void *dst, const void *src, int64_t bytes)
{
  HIPCHECK(ctx, hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DDM_OK;
}
extern "C" int ddm_timing_enable(ddm_ctx *ctx, int on)
{
  ctx->timing = on != 0;
  return DDM_OK;
}
extern "C" int ddm_timing_get(ddm_ctx *ctx, const char *name, double *total_ms, int64_t *count)
{
  resolve_timers(ctx);
  auto it = ctx->timers.find(name);
  if (it == ctx->timers.end()) {
    if (total_ms) *total_ms = 0.0;
    if (count) *count = 0;
    return DDM_OK;
  }
  if (total_ms) *total_ms = it->second.ms;
  if (count) *count = it->second.count;
  return DDM_OK;
}
extern "C" int ddm_timing_reset(ddm_ctx *ctx)
{
  resolve_timers(ctx);
  for (auto &kv : ctx->timers) {
    kv.second.ms = 0.0;
    kv.second.count = 0;
  }
  return DDM_OK;
}

// ---- m-column paths: argument check and the context's block scratch ---------------------------
static int multi_check(ddm_ctx *ctx, int m, const char *what)
{
  if (m < 1 || m > MULTI_MAX) return fail(ctx, DDM_EINVAL, "%s: nrhs = %d outside [1, %d]", what, m, MULTI_MAX);
  return DDM_OK;
}
static int ctx_multi_scratch(ddm_ctx *ctx)
{
  if (ctx->mscal) return DDM_OK;
  HIPCHECK(ctx, ctx->mpartial.alloc((int64_t)RED_MAX_BLOCKS * MULTI_MAX * 2)); // (two sums per column in one pass: k_fcg_dots_multi)
  HIPCHECK(ctx, ctx->mactive.alloc(MULTI_MAX));
  HIPCHECK(ctx, ctx->mscal.alloc(SCAL_ROWS * MULTI_MAX)); // (the rows SCAL_* and BICG_*: kernels.hpp, multi_kernels.hpp)
  return DDM_OK;
}
