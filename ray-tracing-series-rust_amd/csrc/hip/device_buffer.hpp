// The one owner of device memory on the host side: render.hip (both compilations), progressive.inc, multi.inc and lbvh.hip.
//
// A DeviceBuffer<T> holds one hipMalloc'ed allocation and its capacity in bytes.  It is freed exactly once (destructor or
// release), it cannot be copied, and alloc / grow / upload never overwrite a pointer that is still set.  It reads as its raw
// pointer, so kernel launches and copies take it as they take a T*; a kernel argument struct (rt::SceneView) keeps raw
// pointers and the owner stays with the handle.  It is not a pool and not a cache: alloc is hipMalloc, release is hipFree.
// Nothing here mentions a type of either namespace of render.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

template <class T>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) {
      (void)release();
      p_ = o.p_; bytes_ = o.bytes_;
      o.p_ = nullptr; o.bytes_ = 0;
    }
    return *this;
  }
  ~DeviceBuffer() { (void)release(); }

  operator T*() const { return p_; }
  size_t bytes() const { return bytes_; }

  // Frees the allocation now (a no-op on an empty owner).
  hipError_t release() {
    if (!p_) return hipSuccess;
    const hipError_t e = hipFree((void*)p_);
    p_ = nullptr;
    bytes_ = 0;
    return e;
  }
  // A fresh allocation of `bytes` bytes (what was held is freed first); empty again when hipMalloc fails.
  hipError_t alloc(size_t bytes) {
    hipError_t e = release();
    if (e != hipSuccess) return e;
    e = hipMalloc((void**)&p_, bytes);
    if (e != hipSuccess) p_ = nullptr;
    else bytes_ = bytes;
    return e;
  }
  // Grown to at least `need` bytes (the contents are not kept); the stream's work is finished before the old one is freed.
  hipError_t grow(size_t need, hipStream_t stream) {
    if (need <= bytes_) return hipSuccess;
    if (p_) {
      const hipError_t e = hipStreamSynchronize(stream);
      if (e != hipSuccess) return e;
    }
    return alloc(need);
  }
  // A fresh allocation of count elements and `spare` more bytes, the elements copied from the host array h.
  hipError_t upload(const T* h, size_t count, size_t spare = 0) {
    hipError_t e = alloc(count * sizeof(T) + spare);
    if (e == hipSuccess && count) e = hipMemcpy((void*)p_, h, count * sizeof(T), hipMemcpyHostToDevice);
    return e;
  }

 private:
  T* p_ = nullptr;
  size_t bytes_ = 0;
};
