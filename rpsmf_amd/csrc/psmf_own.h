// Owning types of the host code: every device buffer, pinned host buffer, event and stream of libpsmf_hip.so belongs to one object
// of a type below, and the object's destructor is what releases it.  This header is the only place that names the HIP functions
// which create or destroy one; a create call with flags stays at its use site and writes through put().  (The one exception is the
// process-lifetime event chain of launch_pstep in psmf_step.hip.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

// A handle of type H and the function that destroys it.  Move-only; empty by default.
template <typename H, hipError_t (*Destroy)(H)>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, H())) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) { reset(); h_ = std::exchange(o.h_, H()); }
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = H();
  }
  H get() const { return h_; }
  operator H() const { return h_; }      // where a HIP call takes the handle
  H* put() { reset(); return &h_; }      // the out-argument of a create call
  explicit operator bool() const { return h_ != H(); }

 private:
  H h_ = H();
};

using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

// A buffer and its size in bytes.  alloc() gives the exact size, reserve() only grows; both release what was held first, and a
// failed allocation leaves the buffer empty with bytes() == 0.  Nothing is zero-filled.  The functions are parameters so that a
// host-only test instantiates the same text with counting allocators.
template <hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
    return *this;
  }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { reset(); }
  void reset() {
    if (p_) (void)Free(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  hipError_t alloc(size_t bytes) {
    reset();
    const hipError_t e = Alloc(&p_, bytes);
    if (e != hipSuccess) p_ = nullptr; else bytes_ = bytes;
    return e;
  }
  hipError_t reserve(size_t bytes) { return bytes_ >= bytes ? hipSuccess : alloc(bytes); }
  size_t bytes() const { return bytes_; }
  template <typename T> T* as() const { return static_cast<T*>(p_); }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

using DevBuf = Buf<hipMalloc, hipFree>;
inline constexpr char kAllocCall[] = "hipMalloc";      // what DevBuf::alloc / reserve call: for the message of a failure

// a DevBuf of T: reads as the T* it owns wherever a pointer is expected
template <typename T>
struct Dev : DevBuf {
  T* get() const { return as<T>(); }
  operator T*() const { return get(); }
  T* operator->() const { return get(); }
};

// Pinned host memory of T.  The flags of hipHostMalloc differ between the users, so the call stays with them: through put().
template <typename T> hipError_t free_pinned(T* p) { return hipHostFree(p); }
template <typename T>
using Pinned = Owned<T*, free_pinned<T>>;
