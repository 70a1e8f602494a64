// bb_own.h -- owners of what the host side allocates for itself: device buffers, pinned host blocks, events, streams.
//
// Host only; nothing of the kernels or of the context, so that a stand-alone program can include it (tests/own_check.cpp).
// Every owner is move-only (a moved-from owner is empty), releases in its destructor, has an idempotent release(), and is
// empty and consistent after a failed acquisition (handle null, capacity 0).  What is alive in the process is counted
// (bbr_debug_live_resources): one atomic add per acquisition and per release, nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace bbr {

struct LiveCounts {
  std::atomic<uint64_t> device_allocs{0}, device_bytes{0}, pinned_blocks{0}, events{0}, streams{0};
};
inline LiveCounts g_live_counts;

// hipMemset runs on the NULL stream and may return before the fill has happened; the context's streams are created
// hipStreamNonBlocking, i.e. they do NOT order themselves after the NULL stream.  A kernel launched right after an
// allocation could therefore run BEFORE the zero fill and have its counters / fragment counts wiped afterwards
// (seen as an empty first frame when several processes share the GPU).  Every zero fill is completed here.
inline hipError_t zero_fill_sync(void *ptr, size_t bytes) {
  hipError_t e = hipMemset(ptr, 0, bytes);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  return e;
}

// The moves of an owner, from its swap(): the source is left empty.  (Declaring them deletes the copies.)
#define BB_MOVE_ONLY(Owner)                                \
  Owner() = default;                                       \
  Owner(Owner &&o) noexcept { swap(o); }                   \
  Owner &operator=(Owner &&o) noexcept {                   \
    Owner old(std::move(*this));                           \
    swap(o);                                               \
    return *this;                                          \
  }                                                        \
  ~Owner() { release(); }

// hipMalloc / hipFree.  ensure() only grows; what it grows is lost (the callers refill it).
template <typename T>
struct DeviceBuffer {
  T *ptr = nullptr;
  size_t cap = 0;  // elements
  BB_MOVE_ONLY(DeviceBuffer)
  void swap(DeviceBuffer &o) noexcept { std::swap(ptr, o.ptr), std::swap(cap, o.cap); }
  hipError_t ensure(size_t n, bool zero = false) {
    if (n <= cap) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&ptr, n * sizeof(T));
    if (e != hipSuccess) {
      ptr = nullptr;
      return e;
    }
    cap = n;
    ++g_live_counts.device_allocs;
    g_live_counts.device_bytes += n * sizeof(T);
    if (zero) e = zero_fill_sync(ptr, n * sizeof(T));
    return e;
  }
  void release() {
    if (ptr) {
      (void)hipFree(ptr);
      --g_live_counts.device_allocs;
      g_live_counts.device_bytes -= cap * sizeof(T);
    }
    ptr = nullptr;
    cap = 0;
  }
};

// hipHostMalloc / hipHostFree: a pinned host block of `cap` bytes, seen as T.  ensure() only grows, and loses what it grows.
template <typename T = uint8_t>
struct PinnedBlock {
  T *ptr = nullptr;
  size_t cap = 0;  // bytes
  BB_MOVE_ONLY(PinnedBlock)
  void swap(PinnedBlock &o) noexcept { std::swap(ptr, o.ptr), std::swap(cap, o.cap); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc((void **)&ptr, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
      ptr = nullptr;
      return e;
    }
    cap = bytes;
    ++g_live_counts.pinned_blocks;
    return hipSuccess;
  }
  void release() {
    if (ptr) {
      (void)hipHostFree(ptr);
      --g_live_counts.pinned_blocks;
    }
    ptr = nullptr;
    cap = 0;
  }
};

// An event, made on demand with the flags of its site (hipEventDefault: what hipEventCreate makes); used as the handle.
struct Event {
  hipEvent_t ev = nullptr;
  BB_MOVE_ONLY(Event)
  void swap(Event &o) noexcept { std::swap(ev, o.ev); }
  hipError_t ensure(unsigned flags = hipEventDefault) {
    if (ev) return hipSuccess;
    hipError_t e = hipEventCreateWithFlags(&ev, flags);
    if (e != hipSuccess) {
      ev = nullptr;
      return e;
    }
    ++g_live_counts.events;
    return hipSuccess;
  }
  void release() {
    if (ev) {
      (void)hipEventDestroy(ev);
      --g_live_counts.events;
    }
    ev = nullptr;
  }
  operator hipEvent_t() const { return ev; }
};

// A stream with a priority; used as the handle.
struct Stream {
  hipStream_t st = nullptr;
  BB_MOVE_ONLY(Stream)
  void swap(Stream &o) noexcept { std::swap(st, o.st); }
  hipError_t create(unsigned flags, int priority) {
    release();
    hipError_t e = hipStreamCreateWithPriority(&st, flags, priority);
    if (e != hipSuccess) {
      st = nullptr;
      return e;
    }
    ++g_live_counts.streams;
    return hipSuccess;
  }
  void release() {
    if (st) {
      (void)hipStreamDestroy(st);
      --g_live_counts.streams;
    }
    st = nullptr;
  }
  operator hipStream_t() const { return st; }
};

#undef BB_MOVE_ONLY

}  // namespace bbr
