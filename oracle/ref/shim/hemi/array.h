// Host-only stand-in for hemi::Array<T>: one heap buffer, every "device" view is the host view.
// Only the members the two compiled translation units call.  Test infrastructure only.
#ifndef ORACLE_REF_SHIM_HEMI_ARRAY_H
#define ORACLE_REF_SHIM_HEMI_ARRAY_H

#include <cstddef>
#include <cstring>

namespace hemi {

template <typename T>
class Array {
 public:
  explicit Array(size_t n, bool /*pinned*/ = true) : n_(0), p_(nullptr) { allocate(n); }
  ~Array() { delete[] p_; }
  Array(const Array&) = delete;
  Array& operator=(const Array&) = delete;

  size_t size() const { return n_; }

  // a copy of another length replaces the storage (the callers rely on it to resize)
  void copyFromHost(const T* src, size_t n) {
    if (n != n_) {
      delete[] p_;
      p_ = nullptr;
      allocate(n);
    }
    for (size_t i = 0; i < n; i++) p_[i] = src[i];
  }
  void copyToHost(T* dst, size_t n) const {
    for (size_t i = 0; i < n && i < n_; i++) dst[i] = p_[i];
  }

  T* ptr() { return p_; }
  T* hostPtr() { return p_; }
  T* devicePtr() { return p_; }
  T* writeOnlyPtr() { return p_; }
  T* writeOnlyHostPtr() { return p_; }
  T* writeOnlyDevicePtr() { return p_; }
  const T* readOnlyPtr() const { return p_; }
  const T* readOnlyHostPtr() const { return p_; }
  const T* readOnlyDevicePtr() const { return p_; }

 private:
  void allocate(size_t n) {
    n_ = n;
    p_ = n ? new T[n]() : nullptr;
  }
  size_t n_;
  T* p_;
};

}  // namespace hemi

#endif
