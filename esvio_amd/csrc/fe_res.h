// fe_res.h — owners of the HIP resources a handle holds: device memory, pinned host memory, events, streams.
// Each is a pointer (and a size); a member of one of these types needs no line in esvio_fe_destroy.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <utility>

struct esvio_fe_ctx;

namespace esvio {
namespace fe {

// the one place that counts esvio_fe_ctx::n_allocs and words the error (fe_ctx.h, below the handle)
int res_alloc(esvio_fe_ctx* c, void** p, size_t bytes, bool pinned);

template <class T, bool kPinned>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~Buf() { release(); }
  operator T*() const { return p; }
  template <class U>
  explicit operator U*() const {  // (a cast at the point of use: (double*)c->L2)
    return (U*)p;
  }
  void release() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));  // (hipFree waits for the device: the buffer's readers are done)
    p = nullptr;
    cap = 0;
  }
  // exactly `count` elements (one at least); {nullptr, 0} if the allocation fails
  int alloc(esvio_fe_ctx* c, size_t count) {
    release();
    if (int rc = res_alloc(c, (void**)&p, std::max<size_t>(count, 1) * sizeof(T), kPinned)) {
      p = nullptr;
      return rc;
    }
    cap = count;
    return 0;
  }
  // room for n elements, with a quarter to spare when it has to grow
  int grow(esvio_fe_ctx* c, size_t n) { return n <= cap ? 0 : alloc(c, std::max<size_t>(n + n / 4, 1 << 16)); }
};
template <class T>
using DevBuf = Buf<T, false>;  // hipMalloc / hipFree
template <class T>
using PinBuf = Buf<T, true>;  // hipHostMalloc(hipHostMallocDefault) / hipHostFree

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
  Event& operator=(Event&& o) noexcept {
    std::swap(e, o.e);  // (o's destructor takes the old one)
    return *this;
  }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  operator hipEvent_t() const { return e; }
  hipError_t create(unsigned flags = hipEventDisableTiming) { return hipEventCreateWithFlags(&e, flags); }
};

struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
  hipError_t create(unsigned flags = hipStreamNonBlocking) { return hipStreamCreateWithFlags(&s, flags); }
  hipError_t create(unsigned flags, int priority) { return hipStreamCreateWithPriority(&s, flags, priority); }
};

}  // namespace fe
}  // namespace esvio
