// Device arrays: dbuf<T>, the one owner of a hipMalloc allocation (the device counterpart of hvec in host_vec.hpp).
//
// Ownership rule of the library: every device allocation has exactly one dbuf that frees it; whoever else reads or writes the array
// (kernels, descriptor structs copied to the device, a values-only matrix on another matrix's pattern) holds a raw pointer, a view
// whose lifetime the owner outlives.  A dbuf converts to its raw pointer, so launches and pointer arithmetic read as they would
// with `T *`.  No HIP call of this header knows about ddm_ctx: the caller reports a failure through its own HIPCHECK / fail.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>

template <class T>
class dbuf {
  T *p_ = nullptr;

public:
  dbuf() = default;
  explicit dbuf(T *adopted) : p_(adopted) {} // takes over an allocation made by hipMalloc (release() of another dbuf)
  dbuf(const dbuf &) = delete;
  dbuf &operator=(const dbuf &) = delete;
  dbuf(dbuf &&o) noexcept : p_(o.release()) {}
  dbuf &operator=(dbuf &&o) noexcept
  {
    if (this != &o) {
      (void)reset();
      p_ = o.release();
    }
    return *this;
  }
  ~dbuf() { (void)reset(); }

  hipError_t reset()
  {
    T *p = release();
    return p ? hipFree((void *)p) : hipSuccess;
  }
  T *release()
  {
    T *p = p_;
    p_ = nullptr;
    return p;
  }
  // frees what it holds and allocates max(count, 1) elements (uninitialised); empty when the allocation fails
  hipError_t alloc(int64_t count)
  {
    (void)reset();
    const hipError_t e = hipMalloc((void **)&p_, sizeof(T) * (size_t)std::max<int64_t>(count, 1));
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }
};

// Grow-only column scratch: a group of blocks (rows_i x cols entries each) behind ONE column counter.  When the group holds fewer
// than `cols` columns every block is allocated afresh (contents are not kept); the counter reads 0 until all of them are there.
template <class T>
struct dblock {
  dbuf<T> &buf;
  int64_t rows;
};
template <class T>
inline hipError_t reserve_cols(int &have, int cols, std::initializer_list<dblock<T>> group)
{
  if (have >= cols) return hipSuccess;
  have = 0;
  for (const dblock<T> &b : group)
    if (const hipError_t e = b.buf.alloc(b.rows * cols); e != hipSuccess) return e;
  have = cols;
  return hipSuccess;
}
template <class T>
inline hipError_t reserve_cols(int &have, int cols, dbuf<T> &buf, int64_t rows)
{
  return reserve_cols<T>(have, cols, {{buf, rows}});
}
