// device_buffer.h -- the one owner of an allocation on the library's host side: a move-only buffer over a memory policy.
// Free of the device runtime and of library state, like sxmc_plan.h, so that tests/cpp/test_device_buffer.cpp drives it
// over a host policy that logs and fails on demand.  sxmc_host.h supplies the real policies and the aliases
// (DeviceBuffer, PinnedBuffer) the handle structures use.
//
// Mem has two static functions, `int allocate(void** p, size_t bytes)` and `int free(void* p)`; 0 means success, anything
// else is handed back to the caller as it is.  Sizes and capacities are counted in elements of T (bytes for T = void).
// No conversion to T*: kernels' descriptors keep raw pointers, filled from get().
#pragma once

#include <cstddef>
#include <type_traits>

namespace sxbuf {

template <typename T, typename Mem>
class Buffer {
 public:
  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  Buffer(Buffer&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~Buffer() { reset(); }

  T* get() const { return p_; }
  bool empty() const { return p_ == nullptr; }
  explicit operator bool() const { return p_ != nullptr; }
  size_t capacity() const { return cap_; }   // elements; never ahead of the pointer

  // Exactly `n` elements.  Meant for an empty buffer, where it is one call of the policy; what a buffer still holds is
  // freed FIRST (peak memory does not rise) and its contents are not kept.  On failure the buffer is empty.
  // (n == 0 is passed on as it is: what the policy answers for no bytes is the buffer's.)
  int alloc(size_t n) {
    int status = reset();
    if (status != 0) return status;
    void* p = nullptr;
    status = Mem::allocate(&p, n * kElem);
    if (status != 0) return status;
    p_ = static_cast<T*>(p);
    cap_ = p ? n : 0;
    return 0;
  }
  // Grow-only: nothing when `n` fits, otherwise alloc(n).
  int grow(size_t n) { return n <= cap_ ? 0 : alloc(n); }
  int reset() {
    T* const p = p_;
    p_ = nullptr, cap_ = 0;
    return p ? Mem::free(p) : 0;
  }

 private:
  static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
  T* p_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace sxbuf
