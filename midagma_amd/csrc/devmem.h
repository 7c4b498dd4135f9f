// Ownership of HIP resources: device and pinned buffers (OwnedBuf over the policy below) and
// events.  Each frees itself in its destructor and is move-only, so a struct that holds them
// needs no release list and cannot be copied by accident.
//
// No owning object may have static storage duration: the HIP runtime can be gone by the time
// static destructors run.
#pragma once

#include <atomic>

#include "launch.h"
#include "owned_buf.h"

namespace midagma {

// Bytes the live buffers of the process asked for, device plus pinned (midagma_debug_live_bytes).
// Atomic: a group's member threads allocate concurrently.
inline std::atomic<int64_t> g_live_bytes{0};

// OwnedBuf's memory: hipMalloc / hipFree, or hipHostMalloc / hipHostFree
template <bool Pinned>
struct HipMem {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    if constexpr (Pinned)
      HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    else
      HIP_TRY(hipMalloc(&p, bytes));
    g_live_bytes += (int64_t)bytes;
    return p;
  }
  static void free(void* p, size_t bytes) noexcept {
    (void)(Pinned ? hipHostFree(p) : hipFree(p));
    g_live_bytes -= (int64_t)bytes;
  }
};

template <class T = double>
using DevBuf = OwnedBuf<T, HipMem<false>>;
template <class T>
using PinBuf = OwnedBuf<T, HipMem<true>>;

// an owned hipEvent_t; empty until create()
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }  // (and so no copy: std::vector<Event> moves)
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  void create(unsigned flags = hipEventDefault) {
    if (e) return;
    HIP_TRY(hipEventCreateWithFlags(&e, flags));
  }
  operator hipEvent_t() const { return e; }
};

}  // namespace midagma
