// Stand-alone check of csrc/bb_own.h, for a build with -fsanitize=address,undefined that is run with an EMPTY device list
// (tests/test_own.py compiles and runs it): every acquisition then fails -- hipMalloc, hipHostMalloc, hipEventCreateWithFlags
// and hipStreamCreateWithPriority return an error and leave their output null -- which is the one thing a GPU test cannot
// arrange.  For each owner: a failed acquisition returns the error and leaves the owner empty, also when it held something;
// release() twice is harmless; the moves empty their source and release nothing twice; copying is deleted; and the live
// counts are what they were.  A wrong answer ends the program with exit code 1, a wrong access with the sanitizer's report.
//
// "Held something" without a device: the owners' members are public, so the program puts a
// malloc'd stand-in into one and counts it as the owner would have.  The release functions fail on it like everything else
// here and free nothing; the program frees it itself.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "bb_own.h"

using namespace bbr;

namespace {

int wrong = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("  WRONG line %d: %s\n", __LINE__, #cond);    \
      ++wrong;                                                  \
    }                                                           \
  } while (0)

struct Counts {
  uint64_t v[5];
  bool operator==(const Counts &o) const {
    for (int i = 0; i < 5; ++i)
      if (v[i] != o.v[i]) return false;
    return true;
  }
};
Counts counts() {
  const LiveCounts &n = g_live_counts;
  return {{n.device_allocs.load(), n.device_bytes.load(), n.pinned_blocks.load(), n.events.load(), n.streams.load()}};
}

// What the check needs to know of an owner: its handle, its capacity (0 for those without), how to acquire, and how
// to hold / give back a stand-in with the counts the owner keeps.
template <class T> struct Probe;
template <> struct Probe<DeviceBuffer<float>> {
  using O = DeviceBuffer<float>;
  static void *handle(const O &o) { return (void *)o.ptr; }
  static size_t cap(const O &o) { return o.cap; }
  static hipError_t acquire(O &o) { return o.ensure(64, true); }
  static void hold(O &o, void *p) { o.ptr = (float *)p, o.cap = 8, ++g_live_counts.device_allocs, g_live_counts.device_bytes += 32; }
};
template <> struct Probe<PinnedBlock<uint32_t>> {
  using O = PinnedBlock<uint32_t>;
  static void *handle(const O &o) { return (void *)o.ptr; }
  static size_t cap(const O &o) { return o.cap; }
  static hipError_t acquire(O &o) { return o.ensure(1 << 16); }
  static void hold(O &o, void *p) { o.ptr = (uint32_t *)p, o.cap = 32, ++g_live_counts.pinned_blocks; }
};
template <> struct Probe<Event> {
  using O = Event;
  static void *handle(const O &o) { return (void *)o.ev; }
  static size_t cap(const O &) { return 0; }
  static hipError_t acquire(O &o) { return o.ensure(hipEventDisableTiming); }
  static void hold(O &o, void *p) { o.ev = (hipEvent_t)p, ++g_live_counts.events; }
};
template <> struct Probe<Stream> {
  using O = Stream;
  static void *handle(const O &o) { return (void *)o.st; }
  static size_t cap(const O &) { return 0; }
  static hipError_t acquire(O &o) { return o.create(hipStreamNonBlocking, 0); }
  static void hold(O &o, void *p) { o.st = (hipStream_t)p, ++g_live_counts.streams; }
};

template <class O>
void check(const char *name) {
  using P = Probe<O>;
  static_assert(!std::is_copy_constructible<O>::value && !std::is_copy_assignable<O>::value, "an owner is not copied");
  static_assert(std::is_nothrow_move_constructible<O>::value && std::is_nothrow_move_assignable<O>::value, "an owner moves");
  const int before = wrong;
  const Counts base = counts();
  auto empty = [](O &o) { return P::handle(o) == nullptr && P::cap(o) == 0; };
  void *const stand_in = std::malloc(32);
  {
    O a;
    CHECK(empty(a));
    CHECK(P::acquire(a) != hipSuccess);  // no device: the acquisition fails ...
    CHECK(empty(a));                     // ... and leaves the owner empty,
    CHECK(counts() == base);             //     the counts as they were
    a.release();
    a.release();
    CHECK(empty(a) && counts() == base);

    // an owner that holds something (an event is made once: ensure() on a live one is no acquisition)
    P::hold(a, stand_in);
    CHECK(!(counts() == base));
    if (!std::is_same<O, Event>::value) {
      CHECK(P::acquire(a) != hipSuccess);  // a failed growth: what it held is released, nothing is held now
      CHECK(empty(a) && counts() == base);
      P::hold(a, stand_in);
    }
    const Counts held = counts();
    O b(std::move(a));  // move construction
    CHECK(empty(a) && P::handle(b) == stand_in && counts() == held);
    O c;
    c = std::move(b);  // move assignment into an empty owner
    CHECK(empty(b) && P::handle(c) == stand_in && counts() == held);
    O d;
    P::hold(d, stand_in);  // ... and into one that holds something: that is released, once
    d = std::move(c);
    CHECK(empty(c) && P::handle(d) == stand_in && counts() == held);
    d.release();
    CHECK(empty(d) && counts() == base);
    d.release();
    CHECK(empty(d) && counts() == base);
  }  // (four destructors of empty owners)
  CHECK(counts() == base);
  std::free(stand_in);
  std::printf("%s%s\n", name, wrong == before ? " ok" : "");
}

}  // namespace

int main() {
  int n = -1;
  if (hipGetDeviceCount(&n) == hipSuccess && n > 0) {
    std::printf("WRONG: %d device(s) visible; run with an empty HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES\n", n);
    return 1;
  }
  check<DeviceBuffer<float>>("DeviceBuffer");
  check<PinnedBlock<uint32_t>>("PinnedBlock");
  check<Event>("Event");
  check<Stream>("Stream");
  const Counts end = counts();
  for (uint64_t v : end.v) CHECK(v == 0);
  std::printf("counts%s\n", wrong ? "" : " ok");
  return wrong ? 1 : 0;
}
