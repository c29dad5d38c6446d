// devbuf.hpp -- owning device buffer used by the host side of libgpslam_hip.so
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <utility>
#include <vector>

namespace gps {

// Frees in its destructor (with the owner's device current: gpslam_hip_destroy sets it before `delete h`); moves leave the source
// empty; no copies -- a second owner would free twice
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p; bytes = o.bytes;
      o.p = nullptr; o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t reserve(size_t n) {
    if (n <= bytes) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipMalloc(&p, n ? n : 8);
    if (e == hipSuccess) bytes = n ? n : 8;
    return e;
  }
  void release() {   // the deliberate early free (every caller says why it does not wait for the destructor)
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <typename U> U *as() const { return reinterpret_cast<U *>(p); }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && std::is_nothrow_move_constructible<DevBuf>::value, "DevBuf owns its memory");

// synchronous host -> device copy of a vector (the stream is drained so temporaries may die)
template <typename V> inline hipError_t upload_vec(hipStream_t stream, DevBuf &buf, const std::vector<V> &v) {
  hipError_t e = buf.reserve(v.size() * sizeof(V));
  if (e != hipSuccess || v.empty()) return e;
  if ((e = hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
  return hipStreamSynchronize(stream);
}

}  // namespace gps
