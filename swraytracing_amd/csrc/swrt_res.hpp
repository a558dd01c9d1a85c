// swrt_res.hpp — owning handles for the GPU resources of a context.
//
// Four move-only types, null by default, each releasing what it holds in
// reset() and in its destructor: the library's only hipFree, hipHostFree,
// hipEventDestroy and hipStreamDestroy calls.  alloc() / create() release the
// old resource first and return the HIP status; get() is the raw handle for
// kernel arguments and HIP calls.  std::swap and moves transfer ownership.
// Series groups one or two DevBufs of recorded frames with their counting.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

#include "swrt_packet_state.hpp"

namespace swrt {

// the move-only core: one raw handle H and the call that releases it
template <typename H, auto Release>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, H{})) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, H{});
    }
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }
  void reset() {
    if (h_) (void)Release(h_);
    h_ = H{};
  }
  H get() const { return h_; }
  explicit operator bool() const { return h_ != H{}; }

 protected:
  // the status of the call that filled h_: nothing is held after a failure
  hipError_t held(hipError_t e) {
    if (e != hipSuccess) h_ = H{};
    return e;
  }
  H h_{};
};

// device memory (hipMalloc), `count` elements of T
template <typename T>
struct DevBuf : Owned<T*, hipFree> {
  hipError_t alloc(size_t count) {
    this->reset();
    return this->held(hipMalloc((void**)&this->h_, sizeof(T) * count));
  }
};

// pinned host memory (hipHostMalloc); with hipHostMallocMapped in `flags` it
// also carries the device alias of the allocation (dev())
template <typename T>
struct HostBuf : Owned<T*, hipHostFree> {
  hipError_t alloc(size_t count, unsigned flags = hipHostMallocDefault) {
    this->reset();
    d_ = nullptr;
    hipError_t e = this->held(hipHostMalloc((void**)&this->h_, sizeof(T) * count, flags));
    if (e == hipSuccess && (flags & hipHostMallocMapped)) {
      e = hipHostGetDevicePointer((void**)&d_, this->h_, 0);
      if (e != hipSuccess) this->reset();
    }
    return e;
  }
  T* dev() const { return this->h_ ? d_ : nullptr; }  // the device alias (mapped allocations)
  T& operator[](size_t i) const { return this->h_[i]; }

 private:
  T* d_ = nullptr;
};

struct Event : Owned<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDisableTiming) {
    reset();
    return held(hipEventCreateWithFlags(&h_, flags));
  }
};

struct Stream : Owned<hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) {
    reset();
    return held(hipStreamCreateWithFlags(&h_, flags));
  }
  hipError_t create(unsigned flags, int priority) {
    reset();
    return held(hipStreamCreateWithPriority(&h_, flags, priority));
  }
};

// A series of frames recorded on the device: one or two columns, a frame being
// `per` elements of an 8-byte type in each, and how far it has got.  The
// context's series_reserve / series_get / series_release (swrt_ctx.hpp) grow,
// read and drop it; the recorders write at end_a / end_b and commit to ext.
template <typename A, typename B = A>
struct Series {
  static_assert(sizeof(A) == 8 && sizeof(B) == 8, "frames are counted in 8-byte words and copied out as they are");
  DevBuf<A> a;
  DevBuf<B> b;  // (null in a series of one column)
  SeriesExtent ext;
  // the first unrecorded frame of a column whose frames are `per` elements
  A* end_a(size_t per) const { return a.get() + per * ext.frames(); }
  B* end_b(size_t per) const { return b.get() + per * ext.frames(); }
};

}  // namespace swrt
