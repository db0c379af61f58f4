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

// The one owner of a staging pair: a pinned host block, its device twin and the event that marks the end of the copy out of the
// pinned block.  A call fills the block and copies it to the device on its stream; the next call must not write the block
// before that copy has left it.  Same rules as DeviceBuffer: not copyable, freed once, in the destructor.
class StagingBuffer {
 public:
  StagingBuffer() = default;
  StagingBuffer(const StagingBuffer&) = delete;
  StagingBuffer& operator=(const StagingBuffer&) = delete;
  ~StagingBuffer() {
    if (host_) (void)hipHostFree(host_);
    if (copied_) (void)hipEventDestroy(copied_);
  }

  unsigned char* device() const { return device_; }

  // Room for `bytes` on both sides and *host = the pinned block: waits for the previous copy to have left it, then grows the
  // pinned side and the device side (DeviceBuffer::grow on `stream`).  Neither side keeps its contents.
  hipError_t reserve(size_t bytes, hipStream_t stream, void** host) {
    hipError_t e = copied_ ? hipEventSynchronize(copied_) : hipEventCreateWithFlags(&copied_, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    if (bytes > host_bytes_) {
      if (host_) e = hipHostFree(host_);
      host_ = nullptr;
      host_bytes_ = 0;
      if (e == hipSuccess) e = hipHostMalloc(&host_, bytes, hipHostMallocDefault);
      if (e != hipSuccess) { host_ = nullptr; return e; }
      host_bytes_ = bytes;
    }
    *host = host_;
    return device_.grow(bytes, stream);
  }
  // The first `bytes` of the pinned block to the device on `stream`, and the event behind the copy.
  hipError_t copy(size_t bytes, hipStream_t stream) {
    const hipError_t e = hipMemcpyAsync((void*)device(), host_, bytes, hipMemcpyHostToDevice, stream);
    return e != hipSuccess ? e : hipEventRecord(copied_, stream);
  }

 private:
  void* host_ = nullptr;
  size_t host_bytes_ = 0;
  DeviceBuffer<unsigned char> device_;
  hipEvent_t copied_ = nullptr;
};

// The one owner of a small read-back: a pinned host block of 32-bit words, and the event behind the copy INTO it.  fetch enqueues
// the copy of n device words on `stream`; wait blocks the host until the latest fetch has landed and gives the words.  Same
// rules as DeviceBuffer: not copyable, freed once, in the destructor.
class ReadbackWords {
 public:
  ReadbackWords() = default;
  ReadbackWords(const ReadbackWords&) = delete;
  ReadbackWords& operator=(const ReadbackWords&) = delete;
  ~ReadbackWords() {
    if (host_) (void)hipHostFree(host_);
    if (landed_) (void)hipEventDestroy(landed_);
  }

  bool pending() const { return pending_; }

  hipError_t fetch(const unsigned int* d_words, size_t n, hipStream_t stream) {
    hipError_t e = landed_ ? hipSuccess : hipEventCreateWithFlags(&landed_, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    if (n > count_) {
      // (a copy still in flight targets the old block: let it land before the block goes)
      if (pending_) e = hipEventSynchronize(landed_);
      if (e == hipSuccess && host_) e = hipHostFree(host_);
      host_ = nullptr;
      count_ = 0;
      if (e == hipSuccess) e = hipHostMalloc((void**)&host_, n * sizeof(unsigned int), hipHostMallocDefault);
      if (e != hipSuccess) { host_ = nullptr; return e; }
      count_ = n;
    }
    e = hipMemcpyAsync(host_, d_words, n * sizeof(unsigned int), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipEventRecord(landed_, stream);
    if (e == hipSuccess) pending_ = true;
    return e;
  }
  hipError_t wait(const unsigned int** words) {
    const hipError_t e = pending_ ? hipEventSynchronize(landed_) : hipSuccess;
    pending_ = false;
    *words = host_;
    return e;
  }

 private:
  unsigned int* host_ = nullptr;
  size_t count_ = 0;
  hipEvent_t landed_ = nullptr;
  bool pending_ = false;
};
