// The owning buffer (midagma_amd/csrc/owned_buf.h) on the CPU, over a malloc-backed policy that
// counts live bytes.  Built and run by tests/test_owned_buf.py with -fsanitize=address,undefined:
// ASan reports a double free or a use after free, the counter a leak.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

#include "owned_buf.h"

using namespace midagma;

namespace {

int g_fail = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                             \
    }                                                                       \
  } while (0)

// malloc with the size in a 16-byte header: free must be told the size that was allocated
struct HostMem {
  static inline int64_t live = 0;
  static inline int64_t allocs = 0;
  static inline bool fail_next = false;
  static void* alloc(size_t bytes) {
    if (fail_next) {
      fail_next = false;
      throw std::bad_alloc();
    }
    char* raw = static_cast<char*>(std::malloc(bytes + 16));
    if (!raw) throw std::bad_alloc();
    std::memcpy(raw, &bytes, sizeof(bytes));
    live += static_cast<int64_t>(bytes);
    ++allocs;
    return raw + 16;
  }
  static void free(void* p, size_t bytes) noexcept {
    char* raw = static_cast<char*>(p) - 16;
    size_t allocated = 0;
    std::memcpy(&allocated, raw, sizeof(allocated));
    CHECK(bytes == allocated);
    live -= static_cast<int64_t>(allocated);
    std::free(raw);
  }
};

using Buf = OwnedBuf<double, HostMem>;

static_assert(!std::is_copy_constructible_v<Buf>, "an owning buffer must not be copyable");
static_assert(!std::is_copy_assignable_v<Buf>, "an owning buffer must not be copy-assignable");
static_assert(std::is_nothrow_move_constructible_v<Buf>, "std::vector<Buf> moves on growth");
static_assert(std::is_nothrow_move_assignable_v<Buf>, "move assignment must not throw");

void fill(Buf& b) {  // every entry written: ASan checks the extent
  for (size_t i = 0; i < b.n; ++i) b.p[i] = static_cast<double>(i);
}

void test_alloc_grows_only() {
  Buf b;
  CHECK(b.p == nullptr && b.n == 0);
  b.alloc(10);
  CHECK(b.p != nullptr && b.n == 10 && HostMem::live == 80);
  fill(b);
  double* first = b.p;
  const int64_t allocs = HostMem::allocs;
  b.alloc(10);
  b.alloc(3);
  CHECK(b.p == first && b.n == 10 && HostMem::allocs == allocs && HostMem::live == 80);
  b.alloc(11);
  CHECK(b.n == 11 && HostMem::allocs == allocs + 1 && HostMem::live == 88);
  fill(b);
  // a zero count still yields a pointer (one entry), as kernels are handed p unconditionally
  Buf z;
  z.alloc(0);
  CHECK(z.p != nullptr && z.n == 0 && HostMem::live == 88 + 8);
}

void test_alloc_shifted() {
  Buf b;
  b.alloc_shifted(8, 4);
  CHECK(b.n == 8 && HostMem::live == 12 * 8);
  fill(b);
  double* shifted = b.p;
  const int64_t allocs = HostMem::allocs;
  b.alloc(8);  // a shifted buffer is never kept by a plain alloc
  CHECK(HostMem::allocs == allocs + 1 && b.n == 8 && HostMem::live == 8 * 8);
  fill(b);
  (void)shifted;
  double* plain = b.p;
  b.alloc_shifted(5, 0);  // offset 0 is a plain alloc: kept
  CHECK(b.p == plain && b.n == 8);
  // the offset is in entries of T
  OwnedBuf<char, HostMem> c;
  c.alloc_shifted(3, 5);
  const int64_t live = HostMem::live;
  CHECK(live == 8 * 8 + 8);
  c.p[0] = c.p[2] = 1;
  c.p[-5] = 2;  // the allocation starts 5 entries before p
}

void test_release_twice() {
  Buf b;
  b.release();
  b.alloc(4);
  b.release();
  CHECK(b.p == nullptr && b.n == 0 && HostMem::live == 0);
  b.release();
  CHECK(HostMem::live == 0);
  b.alloc(2);  // usable again
  CHECK(b.p != nullptr && HostMem::live == 16);
}

void test_moves() {
  Buf a;
  a.alloc(6);
  fill(a);
  double* pa = a.p;
  Buf b(std::move(a));
  CHECK(a.p == nullptr && a.n == 0);
  CHECK(b.p == pa && b.n == 6 && HostMem::live == 48);
  a.alloc(1);  // the emptied source allocates afresh, independent of b
  CHECK(a.p != pa && HostMem::live == 56);

  Buf c;
  c.alloc(100);
  CHECK(HostMem::live == 856);
  c = std::move(b);  // frees c's old block
  CHECK(c.p == pa && c.n == 6 && b.p == nullptr && b.n == 0 && HostMem::live == 56);
  fill(c);
  Buf& self = c;
  c = std::move(self);  // self-assignment keeps the block
  CHECK(c.p == pa && c.n == 6 && HostMem::live == 56);

  Buf s;
  s.alloc_shifted(4, 2);
  Buf t(std::move(s));  // the base travels with p: t frees the whole allocation
  CHECK(t.n == 4 && HostMem::live == 56 + 48);
}

void test_vector_growth() {
  {
    std::vector<Buf> v;
    for (int i = 0; i < 100; ++i) {
      Buf b;
      b.alloc(static_cast<size_t>(i) + 1);
      fill(b);
      v.push_back(std::move(b));
    }
    int64_t want = 0;
    for (int i = 0; i < 100; ++i) {
      want += 8 * (i + 1);
      CHECK(v[i].n == static_cast<size_t>(i) + 1 && v[i].p[i] == static_cast<double>(i));
    }
    CHECK(HostMem::live == want);
    v.resize(150);  // default-constructed tail, then grown in place (midagma_solver::tbufs)
    for (Buf& b : v) b.alloc(200);
    CHECK(HostMem::live == 150 * 200 * 8);
  }
  CHECK(HostMem::live == 0);
}

void test_throwing_alloc() {
  Buf b;
  HostMem::fail_next = true;
  bool threw = false;
  try {
    b.alloc(5);
  } catch (const std::bad_alloc&) {
    threw = true;
  }
  CHECK(threw && b.p == nullptr && b.n == 0 && HostMem::live == 0);
  // growing a held buffer: the old block is gone, the buffer empty, nothing counted
  b.alloc(5);
  CHECK(HostMem::live == 40);
  HostMem::fail_next = true;
  threw = false;
  try {
    b.alloc(50);
  } catch (const std::bad_alloc&) {
    threw = true;
  }
  CHECK(threw && b.p == nullptr && b.n == 0 && HostMem::live == 0);
  HostMem::fail_next = true;
  threw = false;
  try {
    b.alloc_shifted(5, 3);
  } catch (const std::bad_alloc&) {
    threw = true;
  }
  CHECK(threw && b.p == nullptr && HostMem::live == 0);
  b.alloc(7);  // and it recovers
  CHECK(b.n == 7 && HostMem::live == 56);
}

}  // namespace

int main() {
  void (*const tests[])() = {test_alloc_grows_only, test_alloc_shifted, test_release_twice,
                             test_moves,            test_vector_growth, test_throwing_alloc};
  for (auto t : tests) {
    t();
    CHECK(HostMem::live == 0);  // every test's buffers freed themselves on scope exit
  }
  if (g_fail) {
    std::fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
#if defined(__SANITIZE_ADDRESS__)
  std::printf("owned_test: AddressSanitizer on\n");
#endif
  std::printf("owned_test: all checks passed, live bytes at exit %lld\n", static_cast<long long>(HostMem::live));
  return 0;
}
