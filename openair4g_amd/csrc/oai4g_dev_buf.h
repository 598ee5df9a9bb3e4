/*
 * dev_buf<T>: the one owner of device memory that belongs to a configuration.  Move-only; holds a
 * device pointer and its element count and frees it when it goes.  Include after the HIP runtime
 * header (or a test's stand-ins for hipMalloc / hipFree / hipMemcpy): this header pulls in neither.
 * Blocking copies only, no stream.
 */
#pragma once
#include <stddef.h>

#include <utility>
#include <vector>

template <class T>
class dev_buf {
  T *p_ = nullptr;
  size_t n_ = 0;

public:
  dev_buf() = default;
  dev_buf(const dev_buf &) = delete;
  dev_buf &operator=(const dev_buf &) = delete;
  dev_buf(dev_buf &&o) noexcept : p_(o.p_), n_(o.n_) { o.release(); }
  dev_buf &operator=(dev_buf &&o) noexcept
  {
    if (this != &o) {
      reset();
      n_ = o.n_;
      p_ = o.release();
    }
    return *this;
  }
  ~dev_buf() { reset(); }

  T *get() const { return p_; }
  size_t count() const { return n_; }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() { if (p_) (void)hipFree(p_); release(); }
  /* hands the pointer out: for tables that live as long as the process and are never freed */
  T *release() { n_ = 0; return std::exchange(p_, nullptr); }
  /* a new buffer holding src[0, n); the old one goes only once the new one is complete, so on failure
   * the object keeps what it had and nothing leaks */
  hipError_t upload(const T *src, size_t n)
  {
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e != hipSuccess) return e;
    if ((e = hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice)) != hipSuccess) {
      (void)hipFree(p);
      return e;
    }
    reset();
    p_ = (T *)p;
    n_ = n;
    return hipSuccess;
  }
  hipError_t upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }
  /* room for n elements, contents undefined; grows only, and frees before it allocates (work buffers
   * can be gigabytes), so on failure the object is empty */
  hipError_t reserve(size_t n)
  {
    if (n <= n_) return hipSuccess;
    reset();
    const hipError_t e = hipMalloc((void **)&p_, n * sizeof(T));
    if (e == hipSuccess) n_ = n; else p_ = nullptr;
    return e;
  }
};
