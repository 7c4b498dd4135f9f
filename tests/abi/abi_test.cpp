// The entry-point layer of the C ABI (midagma_amd/csrc/abi.h) on the CPU, over stand-in handle
// types whose device hooks only count.  Built and run by tests/test_abi_layer.py with
// -fsanitize=address,undefined; no HIP header is read.
#include <cstdio>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>

#include "abi.h"

// midagma_hip.h only declares it; its null handle shares the handle-less slot
struct midagma_solver {
  std::string err;
};

namespace {

int g_fail = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                             \
    }                                                                       \
  } while (0)

}  // namespace

struct Alpha {
  std::string err;
  int device = 0;
};
struct Beta {
  std::string err;
  bool opened = false;
};
static int g_selected = -1, g_selects = 0;
static void abi_select_device(const Alpha* h) {
  if (h->device < 0) throw midagma::DeviceError("HIP error invalid device ordinal");
  g_selected = h->device;
  ++g_selects;
}
// (as midagma_dcor: nothing to select before the handle has opened its device)
static void abi_select_device(const Beta* h) {
  if (h->opened) ++g_selects;
}
static void abi_select_device(const midagma_solver*) { ++g_selects; }

using namespace midagma;

namespace {

bool is(const char* got, const char* want) { return std::strcmp(got, want) == 0; }

void lambdas_and_the_device_hook() {
  Alpha a;
  a.device = 3;
  int ran = 0;
  CHECK(abi_guarded(&a, [&] { ++ran; }) == MIDAGMA_OK);  // void
  CHECK(ran == 1 && g_selected == 3 && g_selects == 1);
  CHECK(abi_guarded(&a, [&] { return 7; }) == 7);  // int: handed through
  CHECK(abi_guarded(&a, [&] { return MIDAGMA_E_STATE; }) == MIDAGMA_E_STATE);
  CHECK(g_selects == 3 && a.err.empty());
  // no handle: nothing is selected, the work still runs
  CHECK(abi_guarded(no_handle<Alpha>, [&] { ++ran; }) == MIDAGMA_OK);
  CHECK(abi_guarded(nullptr, [&] { return 5; }) == 5);
  CHECK(ran == 2 && g_selects == 3);
  // a handle that has not opened its device
  Beta b;
  CHECK(abi_guarded(&b, [&] { ++ran; }) == MIDAGMA_OK && g_selects == 3);
  b.opened = true;
  CHECK(abi_guarded(&b, [&] { ++ran; }) == MIDAGMA_OK && g_selects == 4);
  // a hook that throws: the work does not run, the failure is the handle's
  a.device = -1;
  CHECK(abi_guarded(&a, [&] { ++ran; }) == MIDAGMA_E_HIP);
  CHECK(ran == 4 && is(abi_last_error(&a), "HIP error invalid device ordinal"));
}

void every_class_of_throw() {
  Alpha a;
  CHECK(abi_guarded(&a, [] { throw DeviceError("device"); }) == MIDAGMA_E_HIP && a.err == "device");
  CHECK(abi_guarded(&a, [] { throw std::invalid_argument("argument"); }) == MIDAGMA_E_ARG && a.err == "argument");
  CHECK(abi_guarded(&a, [] { throw std::runtime_error("state"); }) == MIDAGMA_E_STATE && a.err == "state");
  CHECK(abi_guarded(&a, [] { throw std::bad_alloc(); }) == MIDAGMA_E_STATE && !a.err.empty());
  CHECK(abi_guarded(&a, [] { throw 42; }) == MIDAGMA_E_STATE && a.err == "unknown error");
  CHECK(abi_guarded(&a, []() -> int { throw std::invalid_argument("from int"); }) == MIDAGMA_E_ARG);
  CHECK(is(abi_last_error(&a), "from int"));
}

void handle_or_slot() {
  Alpha a;
  Beta b;
  CHECK(abi_fail(&a, MIDAGMA_E_ARG, "on alpha") == MIDAGMA_E_ARG);
  CHECK(is(abi_last_error(&a), "on alpha") && is(abi_last_error(no_handle<Alpha>), ""));
  // two handle types do not share a slot, and neither is the handle-less one
  CHECK(abi_fail(no_handle<Alpha>, MIDAGMA_E_ARG, "no alpha") == MIDAGMA_E_ARG);
  CHECK(abi_fail(no_handle<Beta>, MIDAGMA_E_STATE, "no beta") == MIDAGMA_E_STATE);
  CHECK(abi_fail(nullptr, MIDAGMA_E_HIP, "no handle at all") == MIDAGMA_E_HIP);
  CHECK(is(abi_last_error(no_handle<Alpha>), "no alpha") && is(abi_last_error(no_handle<Beta>), "no beta"));
  CHECK(is(abi_last_error(no_handle<NoHandle>), "no handle at all"));
  CHECK(is(abi_last_error(&a), "on alpha") && b.err.empty());
  // a throw without a handle lands in the family's slot
  CHECK(abi_guarded(no_handle<Beta>, [] { throw std::invalid_argument("beta threw"); }) == MIDAGMA_E_ARG);
  CHECK(is(abi_last_error(no_handle<Beta>), "beta threw") && is(abi_last_error(no_handle<Alpha>), "no alpha"));
  CHECK(abi_guarded(nullptr, [] { throw std::runtime_error("nobody threw"); }) == MIDAGMA_E_STATE);
  CHECK(is(abi_last_error(no_handle<NoHandle>), "nobody threw"));
  // midagma_solver's null handle is the handle-less slot: midagma_last_error(NULL) serves both
  CHECK(is(abi_last_error(no_handle<midagma_solver>), "nobody threw"));
  CHECK(abi_fail(no_handle<midagma_solver>, MIDAGMA_E_ARG, "create failed") == MIDAGMA_E_ARG);
  CHECK(is(abi_last_error(no_handle<NoHandle>), "create failed"));
  midagma_solver s;
  CHECK(abi_guarded(&s, [] { throw std::invalid_argument("on the solver"); }) == MIDAGMA_E_ARG);
  CHECK(s.err == "on the solver" && is(abi_last_error(no_handle<midagma_solver>), "create failed"));
}

void slots_are_per_thread() {
  abi_fail(no_handle<Alpha>, MIDAGMA_E_ARG, "main thread");
  std::string seen_at_start = "?", seen_at_end;
  std::thread t([&] {
    seen_at_start = abi_last_error(no_handle<Alpha>);
    abi_fail(no_handle<Alpha>, MIDAGMA_E_ARG, "other thread");
    seen_at_end = abi_last_error(no_handle<Alpha>);
  });
  t.join();
  CHECK(seen_at_start.empty() && seen_at_end == "other thread");
  CHECK(is(abi_last_error(no_handle<Alpha>), "main thread"));
}

}  // namespace

int main() {
  lambdas_and_the_device_hook();
  every_class_of_throw();
  handle_or_slot();
  slots_are_per_thread();
#if defined(__SANITIZE_ADDRESS__)
  std::printf("AddressSanitizer on\n");
#endif
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
