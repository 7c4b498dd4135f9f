// An owning, move-only, grow-only buffer of T in memory from Mem.  Plain C++ (no HIP header): the
// memory kinds are policies (devmem.h), so tests/owned/owned_test.cpp runs it on malloc under ASan.
//
// Mem supplies   static void* alloc(size_t bytes);                  // throws on failure
//                static void free(void* p, size_t bytes) noexcept;  // bytes: as allocated
#pragma once

#include <algorithm>
#include <cstddef>

namespace midagma {

template <class T, class Mem>
struct OwnedBuf {
  T* p = nullptr;
  size_t n = 0;

  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  OwnedBuf(OwnedBuf&& o) noexcept : p(o.p), n(o.n), base(o.base) { o.forget(); }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, n = o.n, base = o.base;
      o.forget();
    }
    return *this;
  }
  ~OwnedBuf() { release(); }

  // grows only: an unshifted allocation of at least count entries is kept
  void alloc(size_t count) {
    if (count <= n && p && p == base) return;
    fresh(count, 0);
  }
  // count entries starting `off` entries into a fresh allocation (placement experiments)
  void alloc_shifted(size_t count, size_t off) {
    if (off == 0) return alloc(count);
    fresh(count, off);
  }
  void release() noexcept {
    if (base) Mem::free(base, bytes(n, p - base));
    forget();
  }

 private:
  T* base = nullptr;  // the allocation (p = base + an offset, alloc_shifted)
  static size_t bytes(size_t count, size_t off) { return std::max<size_t>(count + off, 1) * sizeof(T); }
  void forget() noexcept {
    base = p = nullptr;
    n = 0;
  }
  void fresh(size_t count, size_t off) {
    release();
    base = static_cast<T*>(Mem::alloc(bytes(count, off)));
    p = base + off;
    n = count;
  }
};

}  // namespace midagma
