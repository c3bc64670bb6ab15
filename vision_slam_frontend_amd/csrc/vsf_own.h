// vsf_own.h -- who owns what: a device buffer, a pinned host buffer, an event or a stream is a MEMBER OF ITS OWNER'S TYPE and
// is released exactly once, when that member dies, is reset or is assigned over.  The kernel argument structs and the
// vsf_launch_* signatures keep raw pointers and handles: they are views, and every owner converts to its view implicitly.
#ifndef VSF_OWN_H_
#define VSF_OWN_H_

#include <cstddef>
#include <utility>

namespace vsfi {

// Traits: `handle` (a pointer type; null = nothing held), acquire(handle*, args...) -> the API's status, release(handle).
// (This template names nothing of HIP: tests/cpp/test_own.cc instantiates it with counting traits under a plain g++.)
template <class Traits>
class Owned {
 public:
  using handle = typename Traits::handle;
  Owned() = default;
  explicit Owned(handle h) : h_(h) {}  // adopts
  Owned(Owned&& o) noexcept : h_(o.release()) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.release();
    }
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }
  // Releases what was held, then acquires; returns the API's status (so it composes with VSF_HIP(...)).
  template <class... A>
  auto alloc(A&&... a) -> decltype(Traits::acquire((handle*)nullptr, std::forward<A>(a)...)) {
    reset();
    return Traits::acquire(&h_, std::forward<A>(a)...);
  }
  void reset() {
    if (h_) Traits::release(h_);
    h_ = nullptr;
  }
  handle release() {  // hands the handle out unreleased (grow_scratch retires a buffer with it)
    handle h = h_;
    h_ = nullptr;
    return h;
  }
  handle get() const { return h_; }
  operator handle() const { return h_; }
  handle operator->() const { return h_; }

 private:
  handle h_ = nullptr;
};

}  // namespace vsfi

#ifndef VSF_OWN_NO_HIP  // ---- the four owners of the library (the host test of the template above defines VSF_OWN_NO_HIP) ----
#include <hip/hip_runtime.h>

namespace vsfi {

template <class T>
struct DevTraits {  // alloc(bytes)
  using handle = T*;
  static hipError_t acquire(T** p, size_t bytes) { return hipMalloc(reinterpret_cast<void**>(p), bytes); }
  static void release(T* p) { (void)hipFree(p); }
};
template <class T>
struct PinnedTraits {  // alloc(bytes, hipHostMallocDefault / hipHostMallocMapped)
  using handle = T*;
  static hipError_t acquire(T** p, size_t bytes, unsigned flags) { return hipHostMalloc(reinterpret_cast<void**>(p), bytes, flags); }
  static void release(T* p) { (void)hipHostFree(p); }
};
struct EventTraits {  // alloc(flags)
  using handle = hipEvent_t;
  static hipError_t acquire(hipEvent_t* e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
  static void release(hipEvent_t e) { (void)hipEventDestroy(e); }
};
struct StreamTraits {  // alloc(flags) or alloc(flags, priority)
  using handle = hipStream_t;
  static hipError_t acquire(hipStream_t* s, unsigned flags) { return hipStreamCreateWithFlags(s, flags); }
  static hipError_t acquire(hipStream_t* s, unsigned flags, int priority) { return hipStreamCreateWithPriority(s, flags, priority); }
  static void release(hipStream_t s) { (void)hipStreamDestroy(s); }
};

template <class T>
using DevBuf = Owned<DevTraits<T>>;
template <class T>
using PinnedBuf = Owned<PinnedTraits<T>>;
using Event = Owned<EventTraits>;
using Stream = Owned<StreamTraits>;

}  // namespace vsfi
#endif

#endif  // VSF_OWN_H_
