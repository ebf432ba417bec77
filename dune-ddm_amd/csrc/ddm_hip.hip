// C-ABI implementation of include/ddm_hip.h: host-side runtime (contexts, plans, level schedules,
// HIP graphs, the CG driver) around the kernels in kernels.hpp.  gfx950 only, no fallback path.
#include "../../include/ddm_hip.h"
#include "host_vec.hpp"
#include "device_buffer.hpp"
#include "kernels.hpp"
#include "trsv_pipe.hpp"
#include "trsv_box.hpp"
#include "sparse_chol_host.hpp"
#include "sn_chol.hpp"
#include "synth_host.hpp"

#include <dlfcn.h>
#include <rccl/rccl.h> // types and enums only: the library is opened with dlopen when ddm_ctx_set_rccl is called

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

using namespace ddm;

// ---------------------------------------------------------------------------------------------
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
  // a scalar waiting to ride on the next coarse-defect all-reduce (ddm_cg_steps: the squared defect norm of the previous iteration)
  double *piggy = nullptr;
  bool rccl = false, rccl_self = false; // rccl_self: route the self segment through RCCL too (single-GPU self test)
  // side stream of the additive combination: the coarse level's restrict / solve / prolong run beside the latency-bound local solve
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  dbuf<double> partial; // RED_MAX_BLOCKS doubles
  dbuf<double> scal;    // 16 device scalars
  int num_cu = 256;           // compute units of the device: persistent kernels launch at most this many workgroups
  bool timing = false;
  std::map<std::string, TimerEntry> timers;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_fence = nullptr; // ddm_ctx_fence
  // multi-RHS scratch (csrc/multi_rhs.hpp), allocated on first use: dot partials, per-column CG scalars, active-column mask
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

// HIP-event timer on the context's stream.  Nothing synchronises while timing is on: the event
// pairs are resolved (hipEventElapsedTime) when the totals are read, after the stream has drained.
struct ScopedTimer {
  ddm_ctx *ctx;
  TimerEntry *t = nullptr;
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  ScopedTimer(ddm_ctx *c, const char *n) : ctx(c)
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
    (void)hipEventRecord(ev.first, ctx->stream);
  }
  ~ScopedTimer()
  {
    if (!t) return;
    (void)hipEventRecord(ev.second, ctx->stream);
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
  if (ctx->partial.alloc(RED_MAX_BLOCKS) != hipSuccess || ctx->scal.alloc(16) != hipSuccess ||
      hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
    delete ctx;
    return DDM_EHIP;
  }
  (void)hipMemset(ctx->scal, 0, sizeof(double) * 16);
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
// in-place sum over all ranks of n doubles at a device pointer, enqueued on the context's stream
static int ctx_allreduce(ddm_ctx *ctx, double *buf, int64_t n, const char *what)
{
  ctx->n_allreduce += 1;
  ctx->n_allreduce_doubles += n;
  if (ctx->rccl) {
    if (ctx->nranks > 1 || ctx->rccl_self) NCCLCHECK(ctx, ctx->nccl.AllReduce(buf, buf, (size_t)n, ncclDouble, ncclSum, ctx->rccl_comm, ctx->stream));
    return DDM_OK;
  }
  if (ctx->nranks > 1)
    if (ctx->allreduce(ctx->user, buf, n) != 0) return fail(ctx, DDM_ECOMM, "allreduce callback failed (%s)", what);
  return DDM_OK;
}

// the coarse defect (K doubles at d0, room for K + 1) summed over the ranks; a scalar waiting in ctx->piggy rides along as element K
// (one RCCL launch instead of two) and is written back
__global__ void k_copy_scalar(const double *__restrict__ src, double *__restrict__ dst) { *dst = *src; }
static int coarse_allreduce(ddm_ctx *ctx, double *d0, int64_t K)
{
  double *rider = ctx->piggy;
  ctx->piggy = nullptr;
  if (!rider) return ctx_allreduce(ctx, d0, K, "coarse defect");
  hipLaunchKernelGGL(k_copy_scalar, dim3(1), dim3(1), 0, ctx->stream, (const double *)rider, d0 + K);
  DDMCHECK(ctx_allreduce(ctx, d0, K + 1, "coarse defect + deferred defect norm"));
  hipLaunchKernelGGL(k_copy_scalar, dim3(1), dim3(1), 0, ctx->stream, (const double *)(d0 + K), rider);
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

// ---- CSR ---------------------------------------------------------------------------------------
// Worker threads of the host-side setup phases (factorisations, schedules, assembly): the cores of the machine, but never more than
// 16 per process -- a node runs one process per GPU, and several of these pools are alive at the same time (DDM_HOST_THREADS overrides).
static unsigned host_threads()
{
  static const unsigned n = []() {
    if (const char *e = std::getenv("DDM_HOST_THREADS")) return (unsigned)std::max(1, std::atoi(e));
    return std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  }();
  return n;
}

// dst = src with `threads` memcpy workers (fresh pages: the copy is page-fault bound on one thread)
template <class T>
static void hvec_copy(hvec<T> &dst, const T *src, size_t n)
{
  dst.resize(n);
  const size_t nth = std::min<size_t>(host_threads(), std::max<size_t>(1, n >> 22));
  if (nth <= 1) {
    if (n) std::memcpy(dst.data(), src, sizeof(T) * n);
    return;
  }
  std::vector<std::thread> th;
  for (size_t t = 0; t < nth; ++t)
    th.emplace_back([&, t]() {
      const size_t a = n * t / nth, b = n * (t + 1) / nth;
      std::memcpy(dst.data() + a, src + a, sizeof(T) * (b - a));
    });
  for (auto &t : th) t.join();
}

struct ddm_csr {
  int64_t nrows = 0, ncols = 0, nnz = 0;
  hvec<int64_t> h_rp; // host copies are kept for the ILU(0) factorisation / analysis
  hvec<int32_t> h_ci;
  hvec<double> h_va;
  // Device arrays.  The pattern is read through the views rp / ci / blk_row: they point at this matrix's own arrays (own_*) or, for
  // a values-only companion on another matrix's pattern (csr_adopt), at that matrix's, which has to outlive the companion.
  dbuf<int64_t> own_rp;
  dbuf<int32_t> own_ci, own_blk_row;
  int64_t *rp = nullptr;
  int32_t *ci = nullptr;
  dbuf<double> va;
  int32_t *blk_row = nullptr;
  int nblk = 0;
  bool host_only = false;       // created by ddm_csr_create_host: no device arrays
  dbuf<int32_t> row_order;      // cache-blocked processing order of the rows for the block products (csr_row_order_tiled), or empty
  std::thread uploader;          // device copies still in flight (csr_adopt): csr_wait_upload joins it
  int upload_rc = 0;
  std::string upload_err;
  void view_pattern_of(const ddm_csr &P) { rp = P.own_rp, ci = P.own_ci, blk_row = P.own_blk_row, nblk = P.nblk; }
};

static std::vector<int32_t> csr_row_blocks(int64_t nrows, const int64_t *rowptr);
static int csr_create_impl(ddm_ctx *ctx, int64_t nrows, int64_t ncols, const int64_t *rowptr, const int32_t *col, const double *val, bool host_only, ddm_csr **out)
{
  if (!ctx || !out || nrows < 0 || !rowptr) return fail(ctx, DDM_EINVAL, "ddm_csr_create: bad arguments");
  if (nrows >= (int64_t)1 << 31 || ncols >= (int64_t)1 << 31) return fail(ctx, DDM_EINVAL, "matrix dimension exceeds int32 columns");
  const int64_t nnz = rowptr[nrows];
  for (int64_t i = 0; i < nrows; ++i)
    if (rowptr[i + 1] < rowptr[i]) return fail(ctx, DDM_EINVAL, "row pointers not monotone at row %lld", (long long)i);
  for (int64_t k = 0; k < nnz; ++k)
    if (col[k] < 0 || col[k] >= ncols) return fail(ctx, DDM_EINVAL, "column index out of range at entry %lld", (long long)k);
  auto A = std::make_unique<ddm_csr>();
  A->nrows = nrows;
  A->ncols = ncols;
  A->nnz = nnz;
  hvec_copy(A->h_rp, rowptr, (size_t)nrows + 1);
  hvec_copy(A->h_ci, col, (size_t)nnz);
  hvec_copy(A->h_va, val, (size_t)nnz);
  const std::vector<int32_t> blk = csr_row_blocks(nrows, rowptr);
  A->nblk = (int)blk.size() - 1;
  if (host_only) { // analysis / assembly input only (the GenEO pencil is built from the host arrays): no device copy
    A->host_only = true;
    A->nblk = 0;
    *out = A.release();
    return DDM_OK;
  }
  DDMCHECK(upload(ctx, rowptr, nrows + 1, A->own_rp));
  DDMCHECK(upload(ctx, col, nnz, A->own_ci));
  DDMCHECK(upload(ctx, val, nnz, A->va));
  DDMCHECK(upload(ctx, blk.data(), (int64_t)blk.size(), A->own_blk_row));
  A->view_pattern_of(*A);
  *out = A.release();
  return DDM_OK;
}
extern "C" int ddm_csr_create(ddm_ctx *ctx, int64_t nrows, int64_t ncols, const int64_t *rowptr, const int32_t *col, const double *val, ddm_csr **out)
{
  return csr_create_impl(ctx, nrows, ncols, rowptr, col, val, false, out);
}
// the same object WITHOUT device arrays: valid as A_neu / B_neu of ddm_geneo_basis (the pencil is assembled from the host arrays) and
// of the other coarse-space builders' host inputs; every entry point that would touch the device arrays returns DDM_EINVAL
extern "C" int ddm_csr_create_host(ddm_ctx *ctx, int64_t nrows, int64_t ncols, const int64_t *rowptr, const int32_t *col, const double *val, ddm_csr **out)
{
  return csr_create_impl(ctx, nrows, ncols, rowptr, col, val, true, out);
}
extern "C" void ddm_csr_destroy(ddm_csr *A)
{
  if (!A) return;
  if (A->uploader.joinable()) A->uploader.join(); // (it writes the members)
  delete A;
}
// row-block schedule of the CSR-stream kernel: <= SPMV_NNZ non-zeros and <= WG rows per block, a row longer than SPMV_NNZ gets a
// block of its own
static std::vector<int32_t> csr_row_blocks(int64_t nrows, const int64_t *rowptr)
{
  std::vector<int32_t> blk;
  blk.push_back(0);
  int64_t r = 0;
  while (r < nrows) {
    int64_t r1 = r;
    const int64_t z0 = rowptr[r];
    while (r1 < nrows && r1 - r < WG && rowptr[r1 + 1] - z0 <= SPMV_NNZ) ++r1;
    if (r1 == r) r1 = r + 1; // long row
    blk.push_back((int32_t)r1);
    r = r1;
  }
  return blk;
}
// Library-internal constructors for matrices the library assembled itself (GenEO pencil): the host arrays are MOVED in (no copy, no
// validation pass), and the device copies are made by a helper thread while the caller goes on with host work on the host arrays
// (factorisation, analysis).  Everything that touches the device arrays calls csr_wait_upload first.
static int csr_wait_upload(ddm_ctx *ctx, const ddm_csr *A)
{
  ddm_csr *M = const_cast<ddm_csr *>(A);
  if (M->uploader.joinable()) M->uploader.join();
  if (M->upload_rc) return fail(ctx, M->upload_rc, "%s", M->upload_err.c_str());
  return DDM_OK;
}
// Cache-blocked processing order of the rows of a block-diagonal matrix whose blocks come from a STRUCTURED grid in lexicographic
// numbering (possibly followed by irregularly numbered rows, e.g. an overlap shell): the strides s2 (one grid line) and s3 (one grid
// plane) are read off the column offsets that most rows share; rows are then visited brick by brick (16 x 4 x 4 points, bricks in
// lexicographic order), rows that fit no brick keep their place at the end.  Purely a performance hint -- any permutation is valid.
// Returns false (order untouched) when no such structure is found.
static bool csr_row_order_tiled(int64_t nblocks, const int64_t *block_ptr, const int64_t *rp, const int32_t *ci, std::vector<int32_t> &order)
{
  const int64_t n = block_ptr[nblocks];
  order.resize((size_t)n);
  std::vector<uint8_t> seen((size_t)n, 0);
  int64_t out = 0;
  bool any = false;
  for (int64_t b = 0; b < nblocks; ++b) {
    const int64_t r0 = block_ptr[b], r1 = block_ptr[b + 1], nb = r1 - r0;
    int64_t s2 = 0, s3 = 0;
    if (nb >= 4096) { // positive column offsets shared by most of a sample of rows from the first half of the block
      std::map<int64_t, int> hist;
      const int64_t sample = 2048, start = r0 + nb / 4;
      for (int64_t i = start; i < start + sample; ++i)
        for (int64_t k = rp[i]; k < rp[i + 1]; ++k)
          if (ci[k] > i) hist[ci[k] - i]++;
      std::vector<int64_t> P;
      for (auto &kv : hist)
        if (kv.second > sample / 2) P.push_back(kv.first);
      auto has = [&](int64_t o) { return std::binary_search(P.begin(), P.end(), o); };
      // 5- / 7-point stencils share the offsets {1, s2, s3}; 9- / 27-point ones {1, s2 - 1, s2, s2 + 1, s3 - s2 - 1, ..., s3 + s2 + 1}
      if (P.size() >= 2 && P[0] == 1) {
        const int64_t a = P[1];
        if (has(a + 1) && has(a + 2)) s2 = a + 1;
        else if (!has(a + 1)) s2 = a;
        if (s2 > 1) {
          auto it = std::upper_bound(P.begin(), P.end(), s2 + 1);
          if (it == P.end()) s3 = ((nb + s2 - 1) / s2) * s2; // two-dimensional: one plane
          else {
            const int64_t c = *it;
            if (has(c + 1) && has(c + 2)) s3 = has(c + s2 + 1) ? c + s2 + 1 : 0;
            else if (!has(c + 1)) s3 = c;
          }
        }
      }
      if (s2 < 4 || s3 < 2 * s2) s2 = s3 = 0;
    }
    if (!s2) {
      for (int64_t r = r0; r < r1; ++r) order[(size_t)out++] = (int32_t)r;
      continue;
    }
    any = true;
    const int64_t ny = s3 / s2, nz = (nb + s3 - 1) / s3;
    constexpr int64_t TX = 16, TY = 4, TZ = 4;
    for (int64_t z0 = 0; z0 < nz; z0 += TZ)
      for (int64_t y0 = 0; y0 < ny; y0 += TY)
        for (int64_t x0 = 0; x0 < s2; x0 += TX)
          for (int64_t z = z0; z < std::min(z0 + TZ, nz); ++z)
            for (int64_t y = y0; y < std::min(y0 + TY, ny); ++y)
              for (int64_t x = x0; x < std::min(x0 + TX, s2); ++x) {
                const int64_t r = x + y * s2 + z * s3;
                if (r < nb && !seen[(size_t)(r0 + r)]) {
                  seen[(size_t)(r0 + r)] = 1;
                  order[(size_t)out++] = (int32_t)(r0 + r);
                }
              }
    for (int64_t r = r0; r < r1; ++r) // (planes with s3 % s2 leftovers)
      if (!seen[(size_t)r]) order[(size_t)out++] = (int32_t)r;
  }
  return any && out == n;
}
// host-only entry for the CPU tests: order_out[n]; returns 1 when a grid structure was found (else order_out is the identity)
extern "C" int ddm_csr_row_order_tiled_host(int64_t nblocks, const int64_t *block_ptr, const int64_t *rowptr, const int32_t *col, int32_t *order_out)
{
  if (nblocks < 1 || !block_ptr || !rowptr || !col || !order_out || block_ptr[0] != 0) return DDM_EINVAL;
  std::vector<int32_t> order;
  const bool found = csr_row_order_tiled(nblocks, block_ptr, rowptr, col, order);
  std::memcpy(order_out, order.data(), sizeof(int32_t) * order.size());
  return found ? 1 : 0;
}
static ddm_csr *csr_adopt(ddm_ctx *ctx, int64_t n, hvec<int64_t> &&rp, hvec<int32_t> &&ci, hvec<double> &&va, hvec<double> &&companion_values, ddm_csr **companion,
                          int64_t nblocks = 0, const int64_t *block_ptr = nullptr /* diagonal blocks: builds the cache-blocked row order of the block products */)
{
  ddm_csr *A = new ddm_csr, *C = new ddm_csr;
  A->nrows = A->ncols = C->nrows = C->ncols = n;
  A->nnz = C->nnz = rp[(size_t)n];
  A->h_rp = std::move(rp);
  A->h_ci = std::move(ci);
  A->h_va = std::move(va);
  *companion = C; // values only: views A's pattern
  const int device = ctx->device;
  auto cv = std::make_shared<hvec<double>>(std::move(companion_values));
  std::vector<int64_t> bp(block_ptr ? block_ptr : nullptr, block_ptr ? block_ptr + nblocks + 1 : nullptr);
  A->uploader = std::thread([A, C, cv, device, bp]() {
    auto up = [&](const auto &src, auto &dst) {
      if (A->upload_rc) return;
      hipError_t e = dst.alloc((int64_t)src.size());
      if (e == hipSuccess && src.size()) e = hipMemcpy(dst, src.data(), sizeof(src[0]) * src.size(), hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        A->upload_rc = DDM_EHIP;
        A->upload_err = std::string("matrix upload failed: ") + hipGetErrorString(e);
      }
    };
    (void)hipSetDevice(device);
    const std::vector<int32_t> blk = csr_row_blocks(A->nrows, A->h_rp.data());
    A->nblk = (int)blk.size() - 1;
    up(A->h_rp, A->own_rp);
    up(A->h_ci, A->own_ci);
    up(A->h_va, A->va);
    up(blk, A->own_blk_row);
    up(*cv, C->va);
    if (bp.size() >= 2 && !std::getenv("DDM_SPMM_NATURAL_ORDER")) {
      std::vector<int32_t> order;
      if (csr_row_order_tiled((int64_t)bp.size() - 1, bp.data(), A->h_rp.data(), A->h_ci.data(), order)) up(order, A->row_order);
    }
    A->view_pattern_of(*A);
    C->view_pattern_of(*A);
  });
  return A;
}
extern "C" int64_t ddm_csr_rows(const ddm_csr *A) { return A->nrows; }
extern "C" int64_t ddm_csr_nnz(const ddm_csr *A) { return A->nnz; }

static int csr_mv_impl(ddm_ctx *ctx, const ddm_csr *A, double alpha, const double *x, double *y, bool acc)
{
  if (A->host_only) return fail(ctx, DDM_EINVAL, "the matrix was created without device arrays (ddm_csr_create_host)");
  if (A->nblk == 0) return DDM_OK;
  if (acc)
    hipLaunchKernelGGL(k_spmv_stream<true>, dim3(A->nblk), dim3(WG), 0, ctx->stream, A->rp, A->ci, A->va, A->blk_row, A->nblk, x, y, alpha);
  else
    hipLaunchKernelGGL(k_spmv_stream<false>, dim3(A->nblk), dim3(WG), 0, ctx->stream, A->rp, A->ci, A->va, A->blk_row, A->nblk, x, y, alpha);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_csr_mv(ddm_ctx *ctx, const ddm_csr *A, const double *x, double *y)
{
  if (x == y) return fail(ctx, DDM_EINVAL, "ddm_csr_mv: x and y alias");
  return csr_mv_impl(ctx, A, 1.0, x, y, false);
}
extern "C" int ddm_csr_usmv(ddm_ctx *ctx, const ddm_csr *A, double alpha, const double *x, double *y)
{
  if (x == y) return fail(ctx, DDM_EINVAL, "ddm_csr_usmv: x and y alias");
  return csr_mv_impl(ctx, A, alpha, x, y, true);
}

// Y = A X, row-major n x nrhs block vectors with leading dimensions ldx / ldy (MatOp::perform_op on a block; spectra.hh:100-105)
static int csr_mm_ld(ddm_ctx *ctx, const ddm_csr *A, int nrhs, const double *X, int64_t ldx, double *Y, int64_t ldy)
{
  if (!A || !X || !Y || X == Y || nrhs < 1 || ldx < nrhs || ldy < nrhs) return fail(ctx, DDM_EINVAL, "ddm_csr_mm: bad arguments");
  if (A->host_only) return fail(ctx, DDM_EINVAL, "the matrix was created without device arrays (ddm_csr_create_host)");
  const int64_t threads = A->nrows * (int64_t)nrhs;
  if (threads == 0) return DDM_OK;
  if (nrhs % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)X & 31) == 0 && ((uintptr_t)Y & 31) == 0) {
    hipLaunchKernelGGL(k_spmm_rowmajor4<false>, dim3((unsigned)((threads / 4 + WG - 1) / WG)), dim3(WG), 0, ctx->stream, A->nrows, nrhs / 4, A->rp, A->ci, A->va,
                       (const double *)nullptr, X, ldx, Y, (double *)nullptr, ldy);
    HIPCHECK(ctx, hipGetLastError());
    return DDM_OK;
  }
  hipLaunchKernelGGL(k_spmm_rowmajor, dim3((unsigned)((threads + WG - 1) / WG)), dim3(WG), 0, ctx->stream, A->nrows, nrhs, A->rp, A->ci,
                     A->va, X, ldx, Y, ldy);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
// Y1 = A1 X, Y2 = A2 X for two matrices on ONE pattern (same rp / ci arrays in value; checked by size only: internal use)
static int csr_mm2_ld(ddm_ctx *ctx, const ddm_csr *A1, const ddm_csr *A2, int nrhs, const double *X, int64_t ldx, double *Y1, double *Y2, int64_t ldy)
{
  const bool fast = A1->nrows == A2->nrows && A1->nnz == A2->nnz && nrhs % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)X & 31) == 0 && ((uintptr_t)Y1 & 31) == 0 &&
                    ((uintptr_t)Y2 & 31) == 0 && X != Y1 && X != Y2;
  if (!fast) {
    DDMCHECK(csr_mm_ld(ctx, A1, nrhs, X, ldx, Y1, ldy));
    return csr_mm_ld(ctx, A2, nrhs, X, ldx, Y2, ldy);
  }
  if (A1->host_only || A2->host_only) return fail(ctx, DDM_EINVAL, "the matrix was created without device arrays (ddm_csr_create_host)");
  const int64_t threads = A1->nrows * (int64_t)(nrhs / 4);
  if (threads == 0) return DDM_OK;
  if (A1->row_order && nrhs / 4 <= 8) { // cache-blocked row order: 64 rows per workgroup
    const int nq = nrhs / 4;
    hipLaunchKernelGGL(k_spmm_rowmajor4_tiled<true>, dim3((unsigned)((A1->nrows + 63) / 64)), dim3(64 * nq), 0, ctx->stream, A1->nrows, nq, A1->row_order, A1->rp, A1->ci, A1->va,
                       (const double *)A2->va, X, ldx, Y1, Y2, ldy);
    HIPCHECK(ctx, hipGetLastError());
    return DDM_OK;
  }
  hipLaunchKernelGGL(k_spmm_rowmajor4<true>, dim3((unsigned)((threads + WG - 1) / WG)), dim3(WG), 0, ctx->stream, A1->nrows, nrhs / 4, A1->rp, A1->ci, A1->va,
                     (const double *)A2->va, X, ldx, Y1, Y2, ldy);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_csr_mm(ddm_ctx *ctx, const ddm_csr *A, int nrhs, const double *X, double *Y) { return csr_mm_ld(ctx, A, nrhs, X, nrhs, Y, nrhs); }

#include "local_solver.hpp"

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

static int halo_exchange_impl(ddm_ctx *ctx, ddm_halo *H, const double *src, double *v);
extern "C" int ddm_halo_exchange(ddm_ctx *ctx, ddm_halo *H, double *v) { return halo_exchange_impl(ctx, H, v, v); }
extern "C" int ddm_halo_exchange_to(ddm_ctx *ctx, ddm_halo *H, const double *src, double *dst)
{
  if (!src || !dst) return fail(ctx, DDM_EINVAL, "ddm_halo_exchange_to: bad arguments");
  return halo_exchange_impl(ctx, H, src, dst);
}
static int halo_exchange_impl(ddm_ctx *ctx, ddm_halo *H, const double *src, double *v)
{
  if (!H) return DDM_OK;
  if (H->nsend == 0 && H->ndst == 0 && !H->remote) return DDM_OK;
  if (H->nsend > 0) hipLaunchKernelGGL(k_pack, dim3(grid_for(H->nsend)), dim3(WG), 0, ctx->stream, H->nsend, H->send_idx, src, H->sendbuf);
  const double *rbuf = H->recvbuf;
  ctx->n_halo_groups += 1;
  if (ctx->rccl && (ctx->nranks > 1 || ctx->rccl_self)) {
    // one grouped point-to-point exchange on the context's stream (xGMI links are point-to-point: every peer pair is its own
    // transfer); the self segment stays a device copy unless the single-GPU self test routes it through RCCL as well
    if (H->self_count > 0 && !ctx->rccl_self)
      HIPCHECK(ctx, hipMemcpyAsync(H->recvbuf + H->self_off_recv, H->sendbuf + H->self_off_send, sizeof(double) * (size_t)H->self_count, hipMemcpyDeviceToDevice, ctx->stream));
    NCCLCHECK(ctx, ctx->nccl.GroupStart());
    int64_t so = 0, ro = 0;
    for (int r = 0; r < ctx->nranks; ++r) {
      const bool self = r == ctx->rank;
      if ((!self || ctx->rccl_self) && H->recv_counts[r] > 0) NCCLCHECK(ctx, ctx->nccl.Recv(H->recvbuf + ro, (size_t)H->recv_counts[r], ncclDouble, r, ctx->rccl_comm, ctx->stream));
      if ((!self || ctx->rccl_self) && H->send_counts[r] > 0) NCCLCHECK(ctx, ctx->nccl.Send(H->sendbuf + so, (size_t)H->send_counts[r], ncclDouble, r, ctx->rccl_comm, ctx->stream));
      so += H->send_counts[r];
      ro += H->recv_counts[r];
    }
    NCCLCHECK(ctx, ctx->nccl.GroupEnd());
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

// ---- reductions --------------------------------------------------------------------------------
// result (device scalar) = sum over ranks of sum_i [mask_i] x_i y_i
static int dot_device(ddm_ctx *ctx, int64_t n, const uint8_t *mask, const double *x, const double *y, double *result_dev)
{
  const int nb = grid_for(n, WG * 4, RED_MAX_BLOCKS);
  if (mask)
    hipLaunchKernelGGL(k_dot_partial<true>, dim3(nb), dim3(WG), 0, ctx->stream, n, mask, x, y, ctx->partial);
  else
    hipLaunchKernelGGL(k_dot_partial<false>, dim3(nb), dim3(WG), 0, ctx->stream, n, mask, x, y, ctx->partial);
  hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(WG), 0, ctx->stream, nb, ctx->partial, result_dev);
  HIPCHECK(ctx, hipGetLastError());
  DDMCHECK(ctx_allreduce(ctx, result_dev, 1, "scalar product"));
  return DDM_OK;
}

// ---- NonOverlappingOperator --------------------------------------------------------------------
struct ddm_op {
  const ddm_csr *A = nullptr;
  ddm_halo *halo = nullptr;
  dbuf<uint8_t> owner;
  int64_t n = 0;
  dbuf<double> tmp;
  dbuf<double> mtmp; // multi-RHS block (mcols columns)
  int mcols = 0;
};
extern "C" int ddm_op_create(ddm_ctx *ctx, const ddm_csr *A, ddm_halo *novlp_add, const uint8_t *owner_mask_host, ddm_op **out)
{
  if (!ctx || !A || !out || !owner_mask_host) return fail(ctx, DDM_EINVAL, "ddm_op_create: bad arguments");
  if (A->nrows != A->ncols) return fail(ctx, DDM_EINVAL, "operator matrix must be square");
  if (novlp_add && novlp_add->mode != 1) return fail(ctx, DDM_EINVAL, "operator halo must be an 'add' halo");
  auto op = std::make_unique<ddm_op>();
  op->A = A;
  op->halo = novlp_add;
  op->n = A->nrows;
  int rc = upload(ctx, owner_mask_host, op->n, op->owner);
  if (!rc && op->tmp.alloc(op->n) != hipSuccess) rc = DDM_EHIP;
  if (rc) return fail(ctx, rc, "ddm_op_create: allocation failed");
  *out = op.release();
  return DDM_OK;
}
extern "C" void ddm_op_destroy(ddm_op *op) { delete op; }
extern "C" int ddm_op_apply(ddm_ctx *ctx, ddm_op *op, const double *x, double *y)
{
  ScopedTimer t(ctx, "Operator/apply");
  DDMCHECK(ddm_csr_mv(ctx, op->A, x, y));           // A->mv(x, y)
  return ddm_halo_exchange(ctx, op->halo, y);       // comm->addOwnerCopyToOwnerCopy(y, y)
}
extern "C" int ddm_op_applyscaleadd(ddm_ctx *ctx, ddm_op *op, double alpha, const double *x, double *y)
{
  ScopedTimer t(ctx, "Operator/applyscaleadd");
  // y1 = y; y = 0; usmv; halo; y += y1   (only alpha*A*x is communicated, y is already consistent)
  DDMCHECK(ddm_csr_mv(ctx, op->A, x, op->tmp));
  DDMCHECK(ddm_halo_exchange(ctx, op->halo, op->tmp));
  hipLaunchKernelGGL(k_axpy, dim3(grid_for(op->n)), dim3(WG), 0, ctx->stream, op->n, alpha, op->tmp, y);
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_dot(ddm_ctx *ctx, ddm_op *op, const double *x, const double *y, double *result_host)
{
  DDMCHECK(dot_device(ctx, op->n, op->owner, x, y, ctx->scal + 8));
  return ddm_memcpy_d2h(ctx, result_host, ctx->scal + 8, sizeof(double));
}
extern "C" int ddm_norm(ddm_ctx *ctx, ddm_op *op, const double *x, double *result_host)
{
  DDMCHECK(ddm_dot(ctx, op, x, x, result_host));
  *result_host = std::sqrt(*result_host);
  return DDM_OK;
}

// ---- SchwarzPreconditioner ---------------------------------------------------------------------
struct ddm_schwarz {
  int64_t n = 0, n_novlp = 0;
  int type = 1;
  ddm_ilu0 *solver = nullptr; // owned
  dbuf<int32_t> ext_map;
  dbuf<double> pou;
  dbuf<double> d_ovlp, x_ovlp;
  ddm_halo *copy = nullptr, *add = nullptr;
  dbuf<double> md_ovlp, mx_ovlp; // multi-RHS blocks (mcols columns)
  int mcols = 0;
  ~ddm_schwarz() { ddm_ilu0_destroy(solver); }
};
extern "C" int ddm_schwarz_create(ddm_ctx *ctx, const ddm_csr *A_dir, int64_t nblocks, const int64_t *block_ptr, int64_t n_novlp,
                                  const int32_t *ext_map_host, const double *pou_host, int type, ddm_halo *ovlp_copy,
                                  ddm_halo *ovlp_add, ddm_schwarz **out)
{
  return ddm_schwarz_create_ex(ctx, A_dir, nblocks, block_ptr, n_novlp, ext_map_host, pou_host, type, "ilu0", ovlp_copy, ovlp_add, out);
}
// subdomain_solver: the `type` key of the [schwarz.subdomain_solver] sub-tree (schwarz.hh:85-92): "ilu0" (dune-istl's SeqILU,
// n = 0) or one of "cholmod" / "ldl" / "spqr"-less synonyms "direct", "cholesky" for the sparse direct solver of this library
// (SPD matrices; "umfpack" is accepted for symmetric positive definite input only).
extern "C" int ddm_schwarz_create_ex(ddm_ctx *ctx, const ddm_csr *A_dir, int64_t nblocks, const int64_t *block_ptr, int64_t n_novlp,
                                     const int32_t *ext_map_host, const double *pou_host, int type, const char *subdomain_solver,
                                     ddm_halo *ovlp_copy, ddm_halo *ovlp_add, ddm_schwarz **out)
{
  if (!ctx || !A_dir || !out || !ext_map_host) return fail(ctx, DDM_EINVAL, "ddm_schwarz_create: bad arguments");
  const std::string st = subdomain_solver ? subdomain_solver : "ilu0";
  const bool direct = st == "cholmod" || st == "direct" || st == "cholesky" || st == "umfpack" || st == "ldl";
  if (!direct && st != "ilu0" && st != "ilu") return fail(ctx, DDM_ENOTIMPL, "Unknown subdomain solver type '%s'", st.c_str()); // solver factory lookup (:85-92)
  bool general = st == "umfpack";
  if (st == "direct") { // pick the factorisation by looking at the values: symmetric -> Cholesky
    general = false;
    const int64_t nn = A_dir->nrows;
    for (int64_t i = 0; i < nn && !general; ++i)
      for (int64_t k = A_dir->h_rp[i]; k < A_dir->h_rp[i + 1] && !general; ++k) {
        const int64_t j = A_dir->h_ci[k];
        if (j <= i) continue;
        const auto b = A_dir->h_ci.begin() + A_dir->h_rp[j], e = A_dir->h_ci.begin() + A_dir->h_rp[j + 1];
        const auto it = std::lower_bound(b, e, (int32_t)i);
        const double vt = (it != e && *it == i) ? A_dir->h_va[(size_t)(it - A_dir->h_ci.begin())] : 0.0;
        if (std::fabs(vt - A_dir->h_va[k]) > 1e-12 * (std::fabs(vt) + std::fabs(A_dir->h_va[k]))) general = true;
      }
  }
  if (type != 0 && type != 1) return fail(ctx, DDM_ENOTIMPL, "Unknown Schwarz type %d", type); // schwarz.hh:83
  if (ovlp_copy && ovlp_copy->mode != 0) return fail(ctx, DDM_EINVAL, "ovlp_copy must be a 'copy' halo");
  if (ovlp_add && ovlp_add->mode != 1) return fail(ctx, DDM_EINVAL, "ovlp_add must be an 'add' halo");
  const int64_t n = A_dir->nrows;
  for (int64_t i = 0; i < n; ++i)
    if (ext_map_host[i] >= n_novlp) return fail(ctx, DDM_EINVAL, "ext_map entry out of range"); // size checks, schwarz.hh:186-193
  auto S = std::make_unique<ddm_schwarz>();
  S->n = n;
  S->n_novlp = n_novlp;
  S->type = type;
  S->copy = ovlp_copy;
  S->add = ovlp_add;
  DDMCHECK(direct ? ddm_direct_create(ctx, A_dir, nblocks, block_ptr, general ? 1 : 0, 0.0, &S->solver)
                  : ddm_ilu0_create(ctx, A_dir, nblocks, block_ptr, &S->solver)); // factorisation happens in the ctor (:92)
  DDMCHECK(upload(ctx, ext_map_host, n, S->ext_map));
  if (pou_host) DDMCHECK(upload(ctx, pou_host, n, S->pou));
  if (S->d_ovlp.alloc(n) != hipSuccess || S->x_ovlp.alloc(n) != hipSuccess) return fail(ctx, DDM_EHIP, "alloc");
  *out = S.release();
  return DDM_OK;
}
extern "C" void ddm_schwarz_destroy(ddm_schwarz *S) { delete S; }
extern "C" int64_t ddm_schwarz_num_levels(const ddm_schwarz *S, int upper) { return ddm_ilu0_num_levels(S->solver, upper); }
extern "C" int64_t ddm_schwarz_factor_nnz(const ddm_schwarz *S) { return (S && S->solver) ? S->solver->nnz : 0; } // stored entries of L + U (+ diagonal)
extern "C" int ddm_schwarz_engine(const ddm_schwarz *S) { return S ? ddm_ilu0_engine(S->solver) : -1; }
// Synchronous.  DDM_OK, or DDM_ENUMERIC when a single-launch local solve gave up waiting (its results are invalid: the
// GPU is shared with another process, or the grid was not co-resident) -- the reference's apply has no error return
// (schwarz.hh:131 discards the InverseOperatorResult), so the adaptors poll this in post() and the Krylov drivers at the end.
extern "C" ddm_ilu0 *ddm_schwarz_local_solver(ddm_schwarz *S) { return S ? S->solver : nullptr; } // borrowed (owned by S)
extern "C" int ddm_schwarz_status(ddm_ctx *ctx, const ddm_schwarz *S)
{
  if (!S) return fail(ctx, DDM_EINVAL, "ddm_schwarz_status: bad arguments");
  int st = 0;
  DDMCHECK(ddm_ilu0_status(ctx, S->solver, &st));
  if (st) return fail(ctx, DDM_ENUMERIC, "local triangular solve timed out waiting for a dependency (code %d): results are invalid", st);
  return DDM_OK;
}
// x (= or +=) R~^T [D] A_dir^-1 R~ d
static int schwarz_apply_impl(ddm_ctx *ctx, ddm_schwarz *S, double *x, const double *d, bool acc)
{
  if (const unsigned e = ilu0_peek_status(S->solver)) // fail fast: an earlier local solve gave up (no stream synchronisation here)
    return fail(ctx, DDM_ENUMERIC, "an earlier local triangular solve timed out waiting for a dependency (code %u): results since then are invalid", e);
  {
    ScopedTimer t(ctx, "Schwarz/get defect");
    hipLaunchKernelGGL(k_extend, dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, S->ext_map, d, S->d_ovlp); // :121-122
    DDMCHECK(ddm_halo_exchange(ctx, S->copy, S->d_ovlp));                                                          // :125
  }
  {
    ScopedTimer t(ctx, "Schwarz/local solve");
    DDMCHECK(ddm_ilu0_solve(ctx, S->solver, S->d_ovlp, S->x_ovlp)); // :131-133
  }
  {
    ScopedTimer t(ctx, "Schwarz/add solution");
    if (S->type == 1 && S->pou)
      hipLaunchKernelGGL(k_scale, dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, S->pou, S->x_ovlp); // :139-141
    DDMCHECK(ddm_halo_exchange(ctx, S->add, S->x_ovlp));                                                     // :138/:142
    if (acc)
      hipLaunchKernelGGL((k_restrict<true, false>), dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, S->ext_map, S->x_ovlp, (const double *)nullptr, x);
    else
      hipLaunchKernelGGL((k_restrict<false, false>), dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, S->ext_map, S->x_ovlp, (const double *)nullptr, x); // :146
    HIPCHECK(ctx, hipGetLastError());
  }
  return DDM_OK;
}
extern "C" int ddm_schwarz_apply(ddm_ctx *ctx, ddm_schwarz *S, double *x, const double *d)
{
  ScopedTimer t(ctx, "Schwarz/apply");
  return schwarz_apply_impl(ctx, S, x, d, false);
}

// ---- GalerkinPreconditioner --------------------------------------------------------------------
struct ddm_galerkin {
  int64_t n = 0, n_novlp = 0, nsub = 0, kmax = 0, K = 0, ld = 0;
  dbuf<int32_t> ext_map;
  dbuf<double> basis;       // kmax x ld
  dbuf<int64_t> coarse_index;
  dbuf<double> a0inv;
  dbuf<RowChunk> chunks;
  dbuf<int32_t> sub_chunk_ptr;
  int nchunk = 0;
  dbuf<double> partial, d0, x0;
  dbuf<double> d_ovlp, x_ovlp;
  ddm_halo *copy = nullptr, *add = nullptr;
  dbuf<double> mpartial, md0, mx0, md_ovlp, mx_ovlp; // multi-RHS blocks (mcols columns)
  int mcols = 0;
};
static constexpr int64_t COARSE_CHUNK_ROWS = 8192;

extern "C" int ddm_galerkin_create(ddm_ctx *ctx, int64_t n, int64_t n_novlp, const int32_t *ext_map_host, int64_t nsub,
                                   const int64_t *sub_ptr, int64_t kmax, const double *basis_host, const int64_t *coarse_index,
                                   int64_t K, const double *a0inv_host, ddm_halo *ovlp_copy, ddm_halo *ovlp_add,
                                   ddm_galerkin **out)
{
  if (!ctx || !out || !ext_map_host || !sub_ptr || !basis_host || !coarse_index || !a0inv_host)
    return fail(ctx, DDM_EINVAL, "ddm_galerkin_create: bad arguments");
  if (kmax < 1) return fail(ctx, DDM_EINVAL, "Must at least pass one template vector"); // galerkin_preconditioner.hh:129
  if (kmax > COARSE_KMAX) return fail(ctx, DDM_ENOTIMPL, "more than %d basis vectors per subdomain are not supported", COARSE_KMAX);
  if (sub_ptr[0] != 0 || sub_ptr[nsub] != n) return fail(ctx, DDM_EINVAL, "Template vectors must match size of matrix"); // :131
  for (int64_t t = 0; t < nsub * kmax; ++t)
    if (coarse_index[t] >= K) return fail(ctx, DDM_EINVAL, "coarse_index out of range");
  auto G = std::make_unique<ddm_galerkin>();
  G->n = n;
  G->n_novlp = n_novlp;
  G->nsub = nsub;
  G->kmax = kmax;
  G->K = K;
  G->ld = (n + 63) / 64 * 64;
  G->copy = ovlp_copy;
  G->add = ovlp_add;
  std::vector<RowChunk> chunks;
  std::vector<int32_t> scp(nsub + 1, 0);
  for (int64_t s = 0; s < nsub; ++s) {
    for (int64_t r = sub_ptr[s]; r < sub_ptr[s + 1]; r += COARSE_CHUNK_ROWS)
      chunks.push_back(RowChunk{r, std::min(r + COARSE_CHUNK_ROWS, sub_ptr[s + 1]), (int32_t)s, 0});
    scp[s + 1] = (int32_t)chunks.size();
  }
  G->nchunk = (int)chunks.size();
  DDMCHECK(upload(ctx, ext_map_host, n, G->ext_map));
  DDMCHECK(upload(ctx, coarse_index, nsub * kmax, G->coarse_index));
  DDMCHECK(upload(ctx, a0inv_host, K * K, G->a0inv));
  DDMCHECK(upload(ctx, chunks.data(), (int64_t)chunks.size(), G->chunks));
  DDMCHECK(upload(ctx, scp.data(), nsub + 1, G->sub_chunk_ptr));
  if (G->basis.alloc(kmax * G->ld) != hipSuccess || G->partial.alloc((int64_t)G->nchunk * kmax) != hipSuccess ||
      G->d0.alloc(K + 1) != hipSuccess || // (+ 1: a scalar may ride on the all-reduce, coarse_allreduce)
      G->x0.alloc(K) != hipSuccess || G->d_ovlp.alloc(n) != hipSuccess || G->x_ovlp.alloc(n) != hipSuccess)
    return fail(ctx, DDM_EHIP, "galerkin: allocation failed");
  if (hipMemset(G->basis, 0, sizeof(double) * (size_t)(kmax * G->ld)) != hipSuccess) return DDM_EHIP;
  if (hipMemcpy2D(G->basis, sizeof(double) * (size_t)G->ld, basis_host, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n,
                  (size_t)kmax, hipMemcpyHostToDevice) != hipSuccess)
    return fail(ctx, DDM_EHIP, "galerkin: basis upload failed");
  *out = G.release();
  return DDM_OK;
}
extern "C" void ddm_galerkin_destroy(ddm_galerkin *G) { delete G; }
// d_ovlp_ready: the overlapping defect (extended + owner values copied to all holders) if the caller already has it -- in the
// additive combination both levels start from the same defect (schwarz.hh:121-125 and galerkin_preconditioner.hh:159-162)
static int galerkin_apply_impl(ddm_ctx *ctx, ddm_galerkin *G, double *x, const double *d, bool acc, const double *d_ovlp_ready = nullptr)
{
  ScopedTimer t(ctx, "GalerkinPrec/apply");
  const double *dov = d_ovlp_ready;
  if (!dov) {
    hipLaunchKernelGGL(k_extend, dim3(grid_for(G->n)), dim3(WG), 0, ctx->stream, G->n, G->ext_map, d, G->d_ovlp); // :159
    DDMCHECK(ddm_halo_exchange(ctx, G->copy, G->d_ovlp));                                                         // :162
    dov = G->d_ovlp;
  }
  hipLaunchKernelGGL(k_coarse_restrict_partial, dim3(G->nchunk), dim3(WG), 0, ctx->stream, (int)G->kmax, G->ld, G->basis, dov,
                     G->chunks, G->partial, G->nchunk); // :165-167
  hipLaunchKernelGGL(k_coarse_restrict_final, dim3(1), dim3(WG), 0, ctx->stream, (int)G->nsub, (int)G->kmax, G->sub_chunk_ptr, G->partial,
                     G->coarse_index, G->K, G->d0);
  HIPCHECK(ctx, hipGetLastError());
  DDMCHECK(coarse_allreduce(ctx, G->d0, G->K)); // replaces MPI_Gatherv (:170-171): every rank obtains the full coarse defect
  hipLaunchKernelGGL(k_dense_mv, dim3((unsigned)((G->K + 3) / 4)), dim3(WG), 0, ctx->stream, G->K, G->a0inv, G->d0, G->x0); // :174-179 (replicated)
  hipLaunchKernelGGL(k_coarse_prolong, dim3(G->nchunk), dim3(WG), 0, ctx->stream, (int)G->kmax, G->ld, G->basis, G->x0, G->coarse_index,
                     G->chunks, G->x_ovlp, G->nchunk);       // :186-188
  DDMCHECK(ddm_halo_exchange(ctx, G->add, G->x_ovlp)); // :190
  if (acc)
    hipLaunchKernelGGL((k_restrict<true, false>), dim3(grid_for(G->n)), dim3(WG), 0, ctx->stream, G->n, G->ext_map, G->x_ovlp, (const double *)nullptr, x);
  else
    hipLaunchKernelGGL((k_restrict<false, false>), dim3(grid_for(G->n)), dim3(WG), 0, ctx->stream, G->n, G->ext_map, G->x_ovlp, (const double *)nullptr, x); // :193
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_galerkin_apply(ddm_ctx *ctx, ddm_galerkin *G, double *x, const double *d)
{
  return galerkin_apply_impl(ctx, G, x, d, false);
}

extern "C" int ddm_galerkin_products(ddm_ctx *ctx, const ddm_csr *A_dir, int64_t nleft, const double *left, int64_t nright,
                                     const double *right, int64_t row0, int64_t row1, double *out_host)
{
  // out[j*nleft + i] = <left_i, A_dir right_j> over rows [row0,row1)   (column-major nleft x nright,
  // the slab layout of galerkin_preconditioner.hh:294 / helpers.hh:252)
  if (!A_dir || !left || !right || !out_host || nleft < 1 || nleft > COARSE_KMAX || nright < 1 || row0 < 0 || row1 > A_dir->nrows || row0 > row1)
    return fail(ctx, DDM_EINVAL, "ddm_galerkin_products: bad arguments");
  if (A_dir->host_only) return fail(ctx, DDM_EINVAL, "the matrix was created without device arrays (ddm_csr_create_host)");
  const int64_t n = A_dir->nrows;
  dbuf<double> y, partial, outd;
  dbuf<RowChunk> chunks;
  std::vector<RowChunk> hc;
  for (int64_t r = row0; r < row1; r += COARSE_CHUNK_ROWS) hc.push_back(RowChunk{r, std::min(r + COARSE_CHUNK_ROWS, row1), 0, 0});
  const int nchunk = (int)hc.size();
  HIPCHECK(ctx, y.alloc(n));
  HIPCHECK(ctx, partial.alloc((int64_t)nchunk * nleft));
  HIPCHECK(ctx, outd.alloc(nleft * nright));
  int rc = upload(ctx, hc.data(), (int64_t)hc.size(), chunks);
  std::vector<int32_t> scp = {0, nchunk};
  std::vector<int64_t> cidx(nleft);
  dbuf<int32_t> d_scp;
  dbuf<int64_t> d_cidx;
  if (!rc) rc = upload(ctx, scp.data(), 2, d_scp);
  for (int64_t j = 0; j < nright && !rc; ++j) {
    // y[row0:row1) = (A_dir right_j)[row0:row1): only the rows the products below read (a whole-matrix product per vector and call
    // was 1 s of the headline setup: 1 280 passes over 3.5 GB); same row sums in the same order as ddm_csr_mv
    if (row1 > row0)
      hipLaunchKernelGGL(k_spmm_rowmajor, dim3((unsigned)((row1 - row0 + WG - 1) / WG)), dim3(WG), 0, ctx->stream, row1 - row0, 1, A_dir->rp + row0, A_dir->ci, A_dir->va,
                         right + j * n, (int64_t)1, y + row0, (int64_t)1);
    if (hipGetLastError() != hipSuccess) rc = fail(ctx, DDM_EHIP, "ddm_galerkin_products: kernel launch failed");
    for (int64_t i = 0; i < nleft; ++i) cidx[i] = i;
    if (!d_cidx) rc = upload(ctx, cidx.data(), nleft, d_cidx);
    if (rc) break;
    if (nchunk > 0)
      hipLaunchKernelGGL(k_coarse_restrict_partial, dim3(nchunk), dim3(WG), 0, ctx->stream, (int)nleft, n, left, y, chunks, partial, nchunk);
    hipLaunchKernelGGL(k_coarse_restrict_final, dim3(1), dim3(WG), 0, ctx->stream, 1, (int)nleft, d_scp, partial, d_cidx, nleft, outd + j * nleft);
  }
  if (!rc) rc = ddm_memcpy_d2h(ctx, out_host, outd, sizeof(double) * (size_t)(nleft * nright));
  return rc;
}

// ---- CombinedPreconditioner --------------------------------------------------------------------
struct ddm_combined {
  int mode = 0;
  ddm_op *op = nullptr;
  ddm_schwarz *schwarz = nullptr;
  ddm_galerkin *galerkin = nullptr;
  dbuf<double> dnext;
  int64_t n = 0;
  bool fused = false;   // additive mode: the levels' overlapping results are summed before ONE halo add (combined_apply_fused)
  bool overlap = false; // ... and the coarse chain runs on a side stream beside the local solve (measured slower: off by default)
  dbuf<double> mdnext, mp, mq; // multi-RHS blocks: multiplicative defect (mcols), CG directions (mcg_cols)
  int mcols = 0, mcg_cols = 0;
};
extern "C" int ddm_combined_create(ddm_ctx *ctx, int mode, ddm_op *op, ddm_schwarz *schwarz, ddm_galerkin *galerkin, ddm_combined **out)
{
  if (!ctx || !out || !schwarz) return fail(ctx, DDM_EINVAL, "ERROR: No preconditioners added yet"); // combined_preconditioner.hh:77
  if (mode != 0 && mode != 1) return fail(ctx, DDM_ENOTIMPL, "Unknown apply mode in CombinedPreconditioner, use either additive or multiplicative"); // :68
  if (mode == 1 && galerkin && !op) return fail(ctx, DDM_EINVAL, "ERROR: ApplyMode is multiplicative but operator A is not provided. Set with `set_op`"); // :146
  auto C = std::make_unique<ddm_combined>();
  C->mode = mode;
  C->op = op;
  C->schwarz = schwarz;
  C->galerkin = galerkin;
  C->n = schwarz->n_novlp;
  if (mode == 0 && galerkin) {
    const char *f = std::getenv("DDM_FUSE_LEVELS");    // "0": the two levels one after the other (two halo adds: the reference's order of sums)
    const char *e = std::getenv("DDM_OVERLAP_COARSE"); // "1": coarse chain on a side stream
    C->fused = !(f && f[0] == '0') && galerkin->copy == schwarz->copy && galerkin->add == schwarz->add && galerkin->n == schwarz->n && galerkin->n_novlp == schwarz->n_novlp;
    C->overlap = C->fused && e && e[0] == '1' && (ctx->nranks == 1 || ctx->rccl);
  }
  if (C->dnext.alloc(C->n) != hipSuccess) return fail(ctx, DDM_EHIP, "combined: allocation failed");
  *out = C.release();
  return DDM_OK;
}
extern "C" int ddm_combined_status(ddm_ctx *ctx, const ddm_combined *C)
{
  if (!C) return fail(ctx, DDM_EINVAL, "ddm_combined_status: bad arguments");
  return C->schwarz ? ddm_schwarz_status(ctx, C->schwarz) : DDM_OK;
}
extern "C" void ddm_combined_destroy(ddm_combined *C) { delete C; }
// Additive combination, fused: both levels start from the same extended defect and add over the same interface, so their
// overlapping results are summed BEFORE the exchange (linearity of addOwnerCopyToAll; schwarz.hh:138-146 +
// galerkin_preconditioner.hh:190-193 + combined_preconditioner.hh:136-142) -- one extend, one copy-halo, one halo add and one restrict
// instead of two each; the result differs from the two-pass order by rounding only (measured: 5.54 -> 5.31 ms per iteration at 216^3).
//   extend + copy-halo -> local solve -> (POU scale) -> R d -> all-reduce -> A0^-1 -> R^T x0 -> x_s += x_c -> halo add -> restrict
// two_streams (DDM_OVERLAP_COARSE=1; needs the in-library exchange or a single rank): the coarse chain runs on a side stream BESIDE the
// local solve -- the local solves are latency-bound and leave 85 % of the HBM bandwidth idle, the coarse level is bandwidth-bound.
// Measured at 216^3 it LOSES: the local solve slows from 3.39 to 4.34 ms (its dependent L2 / HBM round trips queue behind the
// basis stream), the coarse chain from 0.87 to 2.2 ms, 5.58 ms per iteration against 5.31 -- off by default.
static int combined_apply_fused(ddm_ctx *ctx, ddm_combined *C, double *x, const double *d, bool two_streams)
{
  ddm_schwarz *S = C->schwarz;
  ddm_galerkin *G = C->galerkin;
  if (two_streams && !ctx->side) {
    HIPCHECK(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    HIPCHECK(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    HIPCHECK(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  }
  {
    ScopedTimer t(ctx, "Schwarz/get defect");
    hipLaunchKernelGGL(k_extend, dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, S->ext_map, d, S->d_ovlp);
    DDMCHECK(ddm_halo_exchange(ctx, S->copy, S->d_ovlp));
  }
  auto coarse_chain = [&](int grid) -> int {
    ScopedTimer t(ctx, "GalerkinPrec/apply");
    hipLaunchKernelGGL(k_coarse_restrict_partial, dim3(grid), dim3(WG), 0, ctx->stream, (int)G->kmax, G->ld, G->basis, (const double *)S->d_ovlp, G->chunks, G->partial, G->nchunk);
    hipLaunchKernelGGL(k_coarse_restrict_final, dim3(1), dim3(WG), 0, ctx->stream, (int)G->nsub, (int)G->kmax, G->sub_chunk_ptr, G->partial, G->coarse_index, G->K, G->d0);
    DDMCHECK(coarse_allreduce(ctx, G->d0, G->K));
    hipLaunchKernelGGL(k_dense_mv, dim3((unsigned)((G->K + 3) / 4)), dim3(WG), 0, ctx->stream, G->K, G->a0inv, G->d0, G->x0);
    hipLaunchKernelGGL(k_coarse_prolong, dim3(grid), dim3(WG), 0, ctx->stream, (int)G->kmax, G->ld, G->basis, G->x0, G->coarse_index, G->chunks, G->x_ovlp, G->nchunk);
    return DDM_OK;
  };
  if (two_streams) {
    // inter-rank operations stay totally ordered: copy-halo (main) -> all-reduce (side) -> [join] -> halo add (main)
    HIPCHECK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    hipStream_t main = ctx->stream;
    HIPCHECK(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
    ctx->stream = ctx->side; // the coarse chain is enqueued on the side stream (kernels, RCCL all-reduce, timer)
    // a small grid: the chain only has to finish within the (latency-bound, ~3 ms) local solve, and a full-rate basis stream would
    // queue in front of the pipe kernel's dependent L2 / HBM round trips (DDM_OVERLAP_GRID: workgroups, default 64)
    static const int side_grid = std::getenv("DDM_OVERLAP_GRID") ? std::max(1, std::atoi(std::getenv("DDM_OVERLAP_GRID"))) : 64;
    const int rc = coarse_chain(std::min(G->nchunk, side_grid));
    const hipError_t e = hipEventRecord(ctx->ev_join, ctx->side);
    ctx->stream = main;
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, DDM_EHIP, "hipEventRecord failed: %s", hipGetErrorString(e));
  }
  const double *pou = S->type == 1 ? S->pou : nullptr;
  // one stream: the coarse chain runs first, so that the local solve's last kernel can also apply "x *= pou; x += x_coarse"
  if (!two_streams) DDMCHECK(coarse_chain(G->nchunk));
  {
    ScopedTimer t(ctx, "Schwarz/local solve");
    DDMCHECK(ilu0_solve_epilogue(ctx, S->solver, S->d_ovlp, S->x_ovlp, two_streams ? nullptr : pou, two_streams ? nullptr : (const double *)G->x_ovlp));
  }
  {
    ScopedTimer t(ctx, "Schwarz/add solution");
    if (two_streams) {
      if (pou) hipLaunchKernelGGL(k_scale, dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, pou, S->x_ovlp);
      HIPCHECK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
      hipLaunchKernelGGL(k_axpy, dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, 1.0, (const double *)G->x_ovlp, S->x_ovlp);
    }
    DDMCHECK(ddm_halo_exchange(ctx, S->add, S->x_ovlp));
    hipLaunchKernelGGL((k_restrict<false, false>), dim3(grid_for(S->n)), dim3(WG), 0, ctx->stream, S->n, S->ext_map, S->x_ovlp, (const double *)nullptr, x);
    HIPCHECK(ctx, hipGetLastError());
  }
  return DDM_OK;
}

extern "C" int ddm_combined_apply(ddm_ctx *ctx, ddm_combined *C, double *x, const double *d)
{
  ScopedTimer t(ctx, "CombinedPreconditioner/apply");
  if (const unsigned e = C->schwarz ? ilu0_peek_status(C->schwarz->solver) : 0u) // fail fast, no synchronisation (see ddm_ilu0_status)
    return fail(ctx, DDM_ENUMERIC, "an earlier local triangular solve timed out waiting for a dependency (code %u): results since then are invalid", e);
  if (C->mode == 0 && C->galerkin && C->fused) return combined_apply_fused(ctx, C, x, d, C->overlap);
  // x = 0; precs[0]->apply(x, d)  (:133-134)  -- the restrict kernel overwrites every entry of x
  DDMCHECK(schwarz_apply_impl(ctx, C->schwarz, x, d, false));
  if (!C->galerkin) return DDM_OK;
  if (C->mode == 0) { // additive: xnext = P1 d; x += xnext (:136-142) -- fused into the restrict of the coarse level
    // both levels extend the same defect over the same interface: the Schwarz level's copy is reused (the local solves read it only)
    static const bool no_share = std::getenv("DDM_NO_SHARED_DEFECT") != nullptr; // diagnostic switch
    const bool share = !no_share && C->galerkin->copy == C->schwarz->copy && C->galerkin->n == C->schwarz->n && C->galerkin->n_novlp == C->schwarz->n_novlp;
    return galerkin_apply_impl(ctx, C->galerkin, x, d, true, share ? C->schwarz->d_ovlp : nullptr);
  }
  // multiplicative: dnext = d - A x; x += P1 dnext (:149-158)
  HIPCHECK(ctx, hipMemcpyAsync(C->dnext, d, sizeof(double) * (size_t)C->n, hipMemcpyDeviceToDevice, ctx->stream));
  DDMCHECK(ddm_op_applyscaleadd(ctx, C->op, -1.0, x, C->dnext));
  return galerkin_apply_impl(ctx, C->galerkin, x, C->dnext, true);
}

// ---- CG ----------------------------------------------------------------------------------------
// dune-istl CGSolver::apply, split so that a caller can time an exact number of
// iterations: begin = "b -= A x; def0 = ||b||", one step = "prec.apply; rho; [beta; p = beta p + q];
// q = A p; alpha; lambda; x += lambda p; b -= lambda q; def = ||b||".
struct ddm_cg {
  ddm_op *op = nullptr;
  ddm_combined *prec = nullptr;
  double *x = nullptr, *b = nullptr; // the caller's
  dbuf<double> p, q;
  int64_t n = 0;
  int it = 0;
  double def0 = 0.0;
};
extern "C" int ddm_cg_begin(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, ddm_cg **out)
{
  if (!ctx || !op || !prec || !x || !b || !out) return fail(ctx, DDM_EINVAL, "ddm_cg_begin: bad arguments");
  auto S = std::make_unique<ddm_cg>();
  S->op = op;
  S->prec = prec;
  S->x = x;
  S->b = b;
  S->n = op->n;
  if (S->p.alloc(S->n) != hipSuccess || S->q.alloc(S->n) != hipSuccess) return fail(ctx, DDM_EHIP, "ddm_cg_begin: allocation failed");
  DDMCHECK(ddm_op_applyscaleadd(ctx, op, -1.0, x, b)); // prec.pre(x,b); b -= A x
  double bb = 0.0;
  DDMCHECK(dot_device(ctx, S->n, op->owner, b, b, ctx->scal + 5));
  DDMCHECK(ddm_memcpy_d2h(ctx, &bb, ctx->scal + 5, sizeof(double)));
  S->def0 = std::sqrt(bb);
  *out = S.release();
  return DDM_OK;
}
extern "C" void ddm_cg_end(ddm_ctx *ctx, ddm_cg *S)
{
  if (!S) return;
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  delete S;
}
extern "C" double ddm_cg_def0(const ddm_cg *S) { return S->def0; }
// Enqueues k iterations without synchronising; the squared defect of the last one is left in
// device scalar 5 (read it with ddm_cg_defect).
extern "C" int ddm_cg_steps(ddm_ctx *ctx, ddm_cg *S, int k)
{
  double *scal = ctx->scal;
  const int G = grid_for(S->n);
  for (int i = 0; i < k; ++i) {
    const bool first = S->it == 0;
    DDMCHECK(ddm_combined_apply(ctx, S->prec, first ? S->p : S->q, S->b));                 // q = M^-1 b  (p on the first step)
    DDMCHECK(dot_device(ctx, S->n, S->op->owner, first ? S->p : S->q, S->b, scal + (first ? 0 : 3))); // rho = <q, b>
    if (!first) {
      hipLaunchKernelGGL(k_cg_beta, dim3(1), dim3(1), 0, ctx->stream, scal);                 // beta = rho / rholast; rholast = rho
      hipLaunchKernelGGL(k_cg_direction, dim3(G), dim3(WG), 0, ctx->stream, S->n, scal, S->q, S->p); // p = beta p + q
    }
    DDMCHECK(ddm_op_apply(ctx, S->op, S->p, S->q));                                          // q = A p
    DDMCHECK(dot_device(ctx, S->n, S->op->owner, S->p, S->q, scal + 1));                     // alpha = <p, q>
    hipLaunchKernelGGL(k_cg_lambda, dim3(1), dim3(1), 0, ctx->stream, scal);                 // lambda = rholast / alpha
    { // x += lambda p; b -= lambda q; def^2 = <b, b> (partial sums in the same kernel)
      const int nb = grid_for(S->n, WG * 4, RED_MAX_BLOCKS);
      if (S->op->owner)
        hipLaunchKernelGGL(k_cg_update_norm<true>, dim3(nb), dim3(WG), 0, ctx->stream, S->n, scal, S->op->owner, S->p, S->q, S->x, S->b, ctx->partial);
      else
        hipLaunchKernelGGL(k_cg_update_norm<false>, dim3(nb), dim3(WG), 0, ctx->stream, S->n, scal, S->op->owner, S->p, S->q, S->x, S->b, ctx->partial);
      hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(WG), 0, ctx->stream, nb, ctx->partial, scal + 5);
      // The rank-local sum is complete; its all-reduce rides on the coarse-defect all-reduce of the NEXT iteration's preconditioner
      // (one RCCL launch saved per iteration) unless this is the chunk's last iteration -- whoever reads the defect (ddm_cg_defect)
      // needs it now -- or there is no coarse level to ride on.
      if (i + 1 < k && S->prec->galerkin) ctx->piggy = scal + 5;
      else DDMCHECK(ctx_allreduce(ctx, scal + 5, 1, "scalar product"));
    }
    S->it += 1;
  }
  if (ctx->piggy) { // (cannot happen: the last iteration of a chunk reduces its own norm)
    ctx->piggy = nullptr;
    DDMCHECK(ctx_allreduce(ctx, scal + 5, 1, "scalar product"));
  }
  HIPCHECK(ctx, hipGetLastError());
  return DDM_OK;
}
extern "C" int ddm_cg_defect(ddm_ctx *ctx, ddm_cg *S, double *def_host) // synchronous
{
  double bb = 0.0;
  DDMCHECK(ddm_memcpy_d2h(ctx, &bb, ctx->scal + 5, sizeof(double)));
  *def_host = std::sqrt(bb);
  (void)S;
  return DDM_OK;
}

extern "C" int ddm_cg_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit,
                            int fixed_iterations, double *hist_host, ddm_solve_result *res)
{
  if (!res) return fail(ctx, DDM_EINVAL, "ddm_cg_solve: bad arguments");
  ddm_cg *S = nullptr;
  DDMCHECK(ddm_cg_begin(ctx, op, prec, x, b, &S));
  const double def0 = S->def0;
  res->def0 = def0;
  res->iterations = 0;
  res->converged = 0;
  res->reduction = 1.0;
  res->elapsed_s = 0.0;
  if (hist_host) hist_host[0] = def0;
  if (!(def0 == def0)) {
    ddm_cg_end(ctx, S);
    return fail(ctx, DDM_ENUMERIC, "initial defect is NaN");
  }
  if (def0 < 1e-30) {
    res->converged = 1;
    ddm_cg_end(ctx, S);
    return DDM_OK;
  }
  (void)hipStreamSynchronize(ctx->stream);
  const auto t0 = std::chrono::steady_clock::now();
  int rc = DDM_OK;
  double deff = def0;
  if (fixed_iterations > 0 && !hist_host) {
    rc = ddm_cg_steps(ctx, S, fixed_iterations);
    if (!rc) rc = ddm_cg_defect(ctx, S, &deff);
    res->iterations = fixed_iterations;
  } else {
    const int iters = fixed_iterations > 0 ? fixed_iterations : maxit;
    for (int i = 1; i <= iters && !rc; ++i) {
      rc = ddm_cg_steps(ctx, S, 1);
      if (!rc) rc = ddm_cg_defect(ctx, S, &deff); // the Krylov loop tests the defect every iteration
      if (rc) break;
      res->iterations = i;
      if (hist_host) hist_host[i] = deff;
      if (!(deff == deff)) {
        rc = fail(ctx, DDM_ENUMERIC, "defect is NaN in iteration %d", i);
        break;
      }
      if (fixed_iterations <= 0 && (deff < def0 * reduction || deff < 1e-30)) {
        res->converged = 1;
        break;
      }
    }
  }
  (void)hipStreamSynchronize(ctx->stream);
  res->elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  res->reduction = deff / def0;
  if (!rc && prec->schwarz) {
    int st = 0;
    rc = ddm_ilu0_status(ctx, prec->schwarz->solver, &st);
    if (!rc && st) rc = fail(ctx, DDM_ENUMERIC, "persistent triangular solve timed out waiting for a level (results invalid)");
  }
  ddm_cg_end(ctx, S);
  return rc;
}

// synchronises the context's stream when it goes out of scope: the Krylov drivers declare it AFTER their work arrays, so that an
// early return waits for the enqueued kernels before the arrays are released
struct StreamDrain {
  ddm_ctx *ctx;
  ~StreamDrain() { (void)hipStreamSynchronize(ctx->stream); }
};

// ---- restarted GMRES -----------------------------------------------------------------------------
// dune-istl RestartedGMResSolver::apply (DUNE 2.10 solvers.hh; not in the snapshot, restated from the
// published implementation): left preconditioning, modified Gram-Schmidt, Givens rotations; the
// monitored quantity is the norm of the PRECONDITIONED defect.  Selected by [solver] type =
// restartedgmressolver in examples/poisson.ini:12-17 (restart = 100) and the default of
// dune/ddm/twolevel_schwarz.hh:121-130 (restart = 30).  Krylov basis, dots and updates stay on the
// device; per iteration the i+2 Hessenberg entries are read back for the rotations on the host.
static void gmres_generate_rotation(double dx, double dy, double &cs, double &sn)
{
  const double ndx = std::fabs(dx), ndy = std::fabs(dy);
  if (ndy < 1e-15) {
    cs = 1.0;
    sn = 0.0;
  } else if (ndx < 1e-15) {
    cs = 0.0;
    sn = 1.0;
  } else if (ndy > ndx) {
    const double t = ndx / ndy;
    cs = 1.0 / std::sqrt(1.0 + t * t);
    sn = cs;
    cs *= t;
    sn *= dx / ndx;
    sn *= dy / ndy;
  } else {
    const double t = ndy / ndx;
    cs = 1.0 / std::sqrt(1.0 + t * t);
    sn = cs;
    sn *= dy / dx;
  }
}
static void gmres_apply_rotation(double &dx, double &dy, double cs, double sn)
{
  const double t = cs * dx + sn * dy;
  dy = -sn * dx + cs * dy;
  dx = t;
}

extern "C" int ddm_gmres_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit,
                               int restart, double *hist_host, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !x || !b || !res || restart < 1) return fail(ctx, DDM_EINVAL, "ddm_gmres_solve: bad arguments");
  const int64_t n = op->n;
  const int m = restart;
  const int G = grid_for(n);
  dbuf<double> V, w, hdev;
  HIPCHECK(ctx, V.alloc(std::max<int64_t>(n, 1) * (m + 1)));
  HIPCHECK(ctx, w.alloc(n));
  HIPCHECK(ctx, hdev.alloc(m + 2));
  StreamDrain drain{ctx}; // (declared after the buffers: from here on every return waits for the stream before they are released)
  auto v = [&](int k) { return V + (size_t)k * (size_t)n; };
  std::vector<double> s(m + 1), cs(m), sn(m), hcol(m + 2), y(m);
  std::vector<std::vector<double>> H(m + 1, std::vector<double>(m, 0.0));
  int rc = ddm_op_applyscaleadd(ctx, op, -1.0, x, b); // b -= A x
  if (!rc) rc = ddm_combined_apply(ctx, prec, v(0), b); // v0 = M^-1 b
  double nn = 0.0;
  if (!rc) rc = dot_device(ctx, n, op->owner, v(0), v(0), hdev);
  if (!rc) rc = ddm_memcpy_d2h(ctx, &nn, hdev, sizeof(double));
  if (rc) return rc;
  double norm = std::sqrt(nn);
  const double def0 = norm;
  res->def0 = def0;
  res->iterations = 0;
  res->converged = 0;
  res->reduction = 1.0;
  res->elapsed_s = 0.0;
  if (hist_host) hist_host[0] = def0;
  if (!(def0 == def0)) return fail(ctx, DDM_ENUMERIC, "initial defect is NaN");
  if (def0 < 1e-30) {
    res->converged = 1;
    return DDM_OK;
  }
  const auto t0 = std::chrono::steady_clock::now();
  int j = 0;
  bool conv = false;
  while (j < maxit && !conv && !rc) {
    hipLaunchKernelGGL(k_scal, dim3(G), dim3(WG), 0, ctx->stream, n, 1.0 / norm, v(0));
    std::fill(s.begin(), s.end(), 0.0);
    s[0] = norm;
    int i = 0;
    for (; i < m && j < maxit && !conv; ++i, ++j) {
      rc = ddm_op_apply(ctx, op, v(i), v(i + 1));                 // v[i+1] = A v[i] (temporary)
      if (!rc) rc = ddm_combined_apply(ctx, prec, w, v(i + 1));   // w = M^-1 A v[i]
      for (int k = 0; k <= i && !rc; ++k) {                       // modified Gram-Schmidt
        rc = dot_device(ctx, n, op->owner, v(k), w, hdev + k);
        hipLaunchKernelGGL(k_axpy_negdev, dim3(G), dim3(WG), 0, ctx->stream, n, hdev + k, v(k), w);
      }
      if (!rc) rc = dot_device(ctx, n, op->owner, w, w, hdev + i + 1);
      if (!rc) rc = ddm_memcpy_d2h(ctx, hcol.data(), hdev, sizeof(double) * (size_t)(i + 2));
      if (rc) break;
      for (int k = 0; k <= i; ++k) H[k][i] = hcol[k];
      H[i + 1][i] = std::sqrt(hcol[i + 1]);
      if (std::fabs(H[i + 1][i]) < 1e-80) {
        rc = fail(ctx, DDM_ENUMERIC, "breakdown in GMRes - |w| == 0.0 after %d iterations", j);
        break;
      }
      HIPCHECK(ctx, hipMemcpyAsync(v(i + 1), w, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
      hipLaunchKernelGGL(k_scal, dim3(G), dim3(WG), 0, ctx->stream, n, 1.0 / H[i + 1][i], v(i + 1));
      for (int k = 0; k < i; ++k) gmres_apply_rotation(H[k][i], H[k + 1][i], cs[k], sn[k]);
      gmres_generate_rotation(H[i][i], H[i + 1][i], cs[i], sn[i]);
      gmres_apply_rotation(H[i][i], H[i + 1][i], cs[i], sn[i]);
      gmres_apply_rotation(s[i], s[i + 1], cs[i], sn[i]);
      norm = std::fabs(s[i + 1]);
      res->iterations = j + 1;
      if (hist_host) hist_host[j + 1] = norm;
      if (!(norm == norm)) {
        rc = fail(ctx, DDM_ENUMERIC, "defect is NaN in iteration %d", j + 1);
        break;
      }
      if (norm < def0 * reduction || norm < 1e-30) conv = true;
    }
    if (rc) break;
    // update(w, i, H, s, v): solve the triangular system, w = sum_k y_k v[k]; x += w
    for (int a = i - 1; a >= 0; --a) {
      double t = s[a];
      for (int c = a + 1; c < i; ++c) t -= H[a][c] * y[c];
      y[a] = t / H[a][a];
    }
    HIPCHECK(ctx, hipMemsetAsync(w, 0, sizeof(double) * (size_t)n, ctx->stream));
    for (int a = 0; a < i; ++a) hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, y[a], v(a), w);
    hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, 1.0, w, x);
    if (!conv && j < maxit) { // restart: b -= A w; v0 = M^-1 b
      rc = ddm_op_applyscaleadd(ctx, op, -1.0, w, b);
      if (!rc) rc = ddm_combined_apply(ctx, prec, v(0), b);
      if (!rc) rc = dot_device(ctx, n, op->owner, v(0), v(0), hdev);
      if (!rc) rc = ddm_memcpy_d2h(ctx, &nn, hdev, sizeof(double));
      norm = std::sqrt(nn);
    }
  }
  if (!rc && hipGetLastError() != hipSuccess) rc = fail(ctx, DDM_EHIP, "kernel launch failed in GMRES");
  (void)hipStreamSynchronize(ctx->stream);
  res->elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  res->converged = conv ? 1 : 0;
  res->reduction = norm / def0;
  if (!rc && prec->schwarz) {
    int st = 0;
    rc = ddm_ilu0_status(ctx, prec->schwarz->solver, &st);
    if (!rc && st) rc = fail(ctx, DDM_ENUMERIC, "persistent triangular solve timed out waiting for a level (results invalid)");
  }
  return rc;
}

// ---- BiCGSTAB ------------------------------------------------------------------------------------
// dune-istl BiCGSTABSolver::apply ([solver] type = bicgstabsolver; DUNE 2.10 solvers.hh, not in the snapshot -- restated in
// oracle/apply_oracle.py::bicgstab_solve): right-preconditioned, two half steps per iteration, the defect norm is tested after each
// half step (hist_host receives both: up to 2 maxit + 1 entries); result.iterations = ceil of the half-step counter, as dune-istl reports.
extern "C" int ddm_bicgstab_solve(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, double *x, double *b, double reduction, int maxit, double *hist_host,
                                  int32_t *nhist, ddm_solve_result *res)
{
  if (!ctx || !op || !prec || !x || !b || !res) return fail(ctx, DDM_EINVAL, "ddm_bicgstab_solve: bad arguments");
  const int64_t n = op->n;
  const int G = grid_for(n);
  const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(n, 1);
  dbuf<double> buf[5]; // rt, p, v, y, t
  StreamDrain drain{ctx}; // (declared after the buffers: every return waits for the stream before they are released)
  for (auto &q : buf)
    if (q.alloc(n) != hipSuccess) return fail(ctx, DDM_EHIP, "ddm_bicgstab_solve: allocation failed");
  double *rt = buf[0], *p = buf[1], *v = buf[2], *y = buf[3], *t = buf[4], *r = b;
  const double EPS = 1e-80;
  const bool verbose = std::getenv("DDM_KRYLOV_VERBOSE") != nullptr;
  int rc = ddm_op_applyscaleadd(ctx, op, -1.0, x, r); // r = b - A x (b is overwritten by the defect, as in dune-istl)
  if (rc) return rc;
  HIPCHECK(ctx, hipMemcpyAsync(rt, r, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  double norm = 0.0;
  if ((rc = ddm_norm(ctx, op, r, &norm))) return rc;
  const double def0 = norm;
  res->def0 = def0;
  res->iterations = 0;
  res->converged = 0;
  res->reduction = 1.0;
  res->elapsed_s = 0.0;
  int nh = 0;
  if (hist_host) hist_host[nh] = def0;
  ++nh;
  if (!(def0 == def0)) return fail(ctx, DDM_ENUMERIC, "initial defect is NaN");
  if (def0 < 1e-30) {
    res->converged = 1;
    if (nhist) *nhist = nh;
    return DDM_OK;
  }
  HIPCHECK(ctx, hipMemsetAsync(p, 0, bytes, ctx->stream));
  HIPCHECK(ctx, hipMemsetAsync(v, 0, bytes, ctx->stream));
  double rho = 1.0, alpha = 1.0, omega = 1.0, rho_new = 0.0, h = 0.0;
  const auto t0 = std::chrono::steady_clock::now();
  double it = 0.5;
  bool conv = false;
  auto record = [&](double nrm) {
    if (hist_host) hist_host[nh] = nrm;
    ++nh;
    res->reduction = nrm / def0;
    return nrm <= def0 * reduction;
  };
  for (; it < maxit && !rc; it += 0.5) {
    if ((rc = ddm_dot(ctx, op, rt, r, &rho_new))) break;
    if (verbose) std::fprintf(stderr, "[ddm bicgstab] it %.1f rho_new %.17g rho %.17g alpha %.17g omega %.17g norm %.17g\n", it, rho_new, rho, alpha, omega, norm);
    if (std::fabs(rho) <= EPS) { rc = fail(ctx, DDM_ENUMERIC, "breakdown in BiCGSTAB - rho %g <= EPSILON after %g iterations", rho, it); break; }
    if (std::fabs(omega) <= EPS) { rc = fail(ctx, DDM_ENUMERIC, "breakdown in BiCGSTAB - omega %g <= EPSILON after %g iterations", omega, it); break; }
    if (it < 1) {
      HIPCHECK(ctx, hipMemcpyAsync(p, r, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
      const double beta = (rho_new / rho) * (alpha / omega);
      hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, -omega, (const double *)v, p); // p = r + beta (p - omega v)
      hipLaunchKernelGGL(k_scal, dim3(G), dim3(WG), 0, ctx->stream, n, beta, p);
      hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, 1.0, (const double *)r, p);
    }
    if ((rc = ddm_combined_apply(ctx, prec, y, p))) break;  // y = W^-1 p
    if ((rc = ddm_op_apply(ctx, op, y, v))) break;           // v = A y
    if ((rc = ddm_dot(ctx, op, rt, v, &h))) break;
    if (std::fabs(h) < EPS) { rc = fail(ctx, DDM_ENUMERIC, "abs(h) < EPSILON in BiCGSTAB - abort"); break; }
    alpha = rho_new / h;
    hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, alpha, (const double *)y, x);
    hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, -alpha, (const double *)v, r);
    if ((rc = ddm_norm(ctx, op, r, &norm))) break;
    if (record(norm)) { conv = true; break; }
    it += 0.5;
    if ((rc = ddm_combined_apply(ctx, prec, y, r))) break;  // y = W^-1 r
    if ((rc = ddm_op_apply(ctx, op, y, t))) break;           // t = A y
    double tt = 0.0, tr = 0.0;
    if ((rc = ddm_dot(ctx, op, t, t, &tt))) break;
    if ((rc = ddm_dot(ctx, op, t, r, &tr))) break;
    omega = tr / tt;
    hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, omega, (const double *)y, x);
    hipLaunchKernelGGL(k_axpy, dim3(G), dim3(WG), 0, ctx->stream, n, -omega, (const double *)t, r);
    rho = rho_new;
    if ((rc = ddm_norm(ctx, op, r, &norm))) break;
    if (record(norm)) { conv = true; break; }
  }
  if (rc) return rc;
  (void)hipStreamSynchronize(ctx->stream);
  res->elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  res->iterations = (int32_t)std::ceil(std::min(it, (double)maxit));
  res->converged = conv ? 1 : 0;
  if (nhist) *nhist = nh;
  int st = 0;
  if (prec->schwarz && !ddm_ilu0_status(ctx, prec->schwarz->solver, &st) && st) return fail(ctx, DDM_ENUMERIC, "local triangular solve timed out (code %d)", st);
  return DDM_OK;
}

#include "geneo.hpp"

// ---- dense host helpers exposed for the CPU tests (host logic of the GenEO Rayleigh-Ritz step) -------------------------
extern "C" int ddm_dense_sym_eig_host(int n, double *V, double *w) { return dense::sym_eig(n, V, w) ? DDM_OK : DDM_ENUMERIC; }
extern "C" int ddm_dense_rayleigh_ritz_host(int p, const double *gA, const double *gC, int keep, double tau, double *mu, double *Y)
{
  return dense::rayleigh_ritz(p, gA, gC, keep, tau, mu, Y);
}

// ---- input synthesis on the host (bench.py / tests: the matrices PDELab's assembler hands to the reference) ----------------------
extern "C" int ddm_synth_q1_matrix(int dim, const int64_t *bshape, const double *ke, const int64_t *eshape, const int64_t *eoff, const double *K,
                                   const uint8_t *inset, const int64_t *loc_of_box, int64_t n, const int64_t *box_index, const uint8_t *dmask,
                                   const double *diag, int64_t *indptr, int32_t *indices, double *data, int nthreads)
{
    if ((dim != 2 && dim != 3) || !bshape || !ke || !eshape || !eoff || !K || !indptr || n < 0 || (indices && !data))
        return fail(nullptr, DDM_EINVAL, "ddm_synth_q1_matrix: bad arguments");
    int64_t nbox = 1;
    for (int d = 0; d < dim; ++d) {
        if (bshape[d] < 1 || eshape[d] < 0 || eoff[d] < 0) return fail(nullptr, DDM_EINVAL, "ddm_synth_q1_matrix: bad box");
        nbox *= bshape[d];
    }
    if (nbox >= INT32_MAX || (!box_index && n != nbox)) return fail(nullptr, DDM_EINVAL, "ddm_synth_q1_matrix: box too large or row count does not match the box");
    synth::Q1Args A{dim, bshape, ke, eshape, eoff, K, inset, loc_of_box, n, box_index, dmask, diag};
    synth::q1_rows(A, indptr, indices, data, nthreads);
    return DDM_OK;
}

#include "multi_rhs.hpp"
#include "multi_gmres.hpp"
