// Carving one allocation into typed regions (pure host code: includes nothing from HIP).
//
// A layout is written once, as a function that takes a Carve by value, takes its regions
// in order and returns a struct of typed pointers plus `bytes`.  Called on Carve() it only
// measures (every pointer null); called on Carve(base) it binds the same regions onto base.
#pragma once

#include <cstddef>

namespace aiy {

class Carve {
 public:
  static constexpr size_t kAlign = 256;
  explicit Carve(void* base = nullptr) : base_(static_cast<char*>(base)) {}
  // `count` elements of T: the region starts on a multiple of `align` bytes from the base
  // and occupies its size rounded up to `align`, so an empty region consumes nothing.
  template <class T>
  T* take(size_t count, size_t align = kAlign) {
    const size_t at = round_up(off_, align);
    off_ = at + round_up(count * sizeof(T), align);
    return base_ ? reinterpret_cast<T*>(base_ + at) : nullptr;
  }
  size_t bytes() const { return off_; }

 private:
  static size_t round_up(size_t b, size_t a) { return (b + a - 1) / a * a; }
  char* base_;
  size_t off_ = 0;
};

}  // namespace aiy
