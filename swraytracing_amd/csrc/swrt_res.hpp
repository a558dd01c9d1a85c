// swrt_res.hpp — owning handles for the GPU resources of a context.
//
// Four move-only types, null by default, each releasing what it holds in
// reset() and in its destructor: the library's only hipFree, hipHostFree,
// hipEventDestroy and hipStreamDestroy calls.  alloc() / create() release the
// old resource first and return the HIP status; get() is the raw handle for
// kernel arguments and HIP calls.  std::swap and moves transfer ownership.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

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

}  // namespace swrt
