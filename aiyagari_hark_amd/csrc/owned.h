// Owning wrappers of the handle's HIP resources: grow-on-demand device / pinned-host
// buffers and lazily created events.  Move-only, released in the destructor, so deleting
// the handle frees everything and no buffer is remembered by hand anywhere else.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "../../include/aiyagari.h"

namespace aiy {

inline int32_t fail(aiy_handle* h, int32_t code, const char* fmt, ...);

template <bool kPinned>   // pinned host memory, or device memory
class Buffer {
 public:
  Buffer() = default;
  Buffer(Buffer&& o) noexcept { swap(o); }
  Buffer& operator=(Buffer&& o) noexcept { swap(o); return *this; }   // (o frees what this held)
  ~Buffer() { reset(); }
  // At least `bytes` of capacity.  A buffer that is too small is freed first and then
  // allocated at exactly `bytes` (contents are not kept; *grew = true); after a failed
  // allocation it is empty with capacity 0.
  int32_t reserve(aiy_handle* h, size_t bytes, bool* grew = nullptr) {
    if (grew) *grew = bytes > cap_;
    if (bytes <= cap_) return AIY_OK;
    reset();
    const hipError_t e = kPinned ? hipHostMalloc(&p_, bytes, hipHostMallocDefault) : hipMalloc(&p_, bytes);
    if (e != hipSuccess) {
      p_ = nullptr;
      return fail(h, AIY_ERR_HIP, "%s(%zu bytes) failed: %s", kPinned ? "hipHostMalloc" : "hipMalloc", bytes,
                  hipGetErrorString(e));
    }
    cap_ = bytes;
    return AIY_OK;
  }
  void reset() {
    if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr, cap_ = 0;
  }
  void* get() const { return p_; }
  template <class T>
  T* as() const { return static_cast<T*>(p_); }

 private:
  void swap(Buffer& o) { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
  void* p_ = nullptr;
  size_t cap_ = 0;
};
using DeviceBuffer = Buffer<false>;
using PinnedBuffer = Buffer<true>;

// A hipEvent_t created on first use.
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept { std::swap(e_, o.e_); }
  Event& operator=(Event&& o) noexcept { std::swap(e_, o.e_); return *this; }
  ~Event() { if (e_) (void)hipEventDestroy(e_); }
  hipError_t ensure(unsigned flags = hipEventDefault) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
  hipEvent_t get() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

// The event pair that brackets a resident launch, with the elapsed milliseconds and the launches
// collected since the last reset (the aiy_*_launch_stats entry points): ensure() once per call,
// begin / end around the launch, collect() after the stream's next synchronisation.
struct LaunchTimer {
  Event ev[2];
  double ms_sum = 0.0;
  long long launches = 0;
  hipError_t ensure() {
    const hipError_t e = ev[0].ensure();
    return e != hipSuccess ? e : ev[1].ensure();
  }
  hipError_t begin(hipStream_t st) { return hipEventRecord(ev[0].get(), st); }
  hipError_t end(hipStream_t st) { return hipEventRecord(ev[1].get(), st); }
  void collect() {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev[0].get(), ev[1].get()) == hipSuccess) ms_sum += ms, launches += 1;
  }
  void read(double* ms_out, int64_t* launches_out, bool reset) {
    if (ms_out) *ms_out = ms_sum;
    if (launches_out) *launches_out = launches;
    if (reset) ms_sum = 0.0, launches = 0;
  }
};

}  // namespace aiy
