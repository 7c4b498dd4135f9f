// The entry-point layer of the C ABI (include/midagma_hip.h), once for every handle family: an
// entry checks its arguments (no device call before that: the checks run on a machine without a
// GPU), fails with a code and a message, and runs its device work under abi_guarded, which selects
// the handle's device and turns a throw into a code and a message.
//
// The message of a failed call lands on the handle (its `err` member); of a call without a handle,
// in a slot of the calling thread, one per handle type, so each family's *_last_error(NULL) reads
// its own.  Entries that take no handle at all pass nullptr and share midagma_solver's slot:
// midagma_last_error(NULL) serves them.
//
// A handle type names how its device is selected by an overload, in the namespace of the type, of
//   void abi_select_device(const H* h);   // may throw; called with h != nullptr only
//
// The first part is plain C++ (tests/abi/abi_test.cpp builds it with g++ under ASan/UBSan); the
// device helpers at the end are for the translation units hipcc builds.
#pragma once

#include <exception>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "../../include/midagma_hip.h"

namespace midagma {

constexpr const char* kNonFinite = "array must not contain infs or NaNs";

// a failed call of the device runtime (launch-time HipError: below)
struct DeviceError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// an exception as a C ABI code with its message: what every entry point returns for a throw
inline int classify(std::exception_ptr e, std::string& msg) {
  try {
    std::rethrow_exception(e);
  } catch (const DeviceError& x) {
    msg = x.what();
    return MIDAGMA_E_HIP;
  } catch (const std::invalid_argument& x) {
    msg = x.what();
    return MIDAGMA_E_ARG;
  } catch (const std::exception& x) {
    msg = x.what();
    return MIDAGMA_E_STATE;
  } catch (...) {
    msg = "unknown error";
    return MIDAGMA_E_STATE;
  }
}

// the handle type of the entries that take none
struct NoHandle {
  std::string err;
};
inline void abi_select_device(const NoHandle*) {}

// the calling thread's message slot for calls of H's family without a handle
template <class H>
std::string& abi_slot() {
  thread_local std::string slot;
  return slot;
}
template <>
inline std::string& abi_slot<midagma_solver>() {
  return abi_slot<NoHandle>();
}

// the null handle of H's family, for a failure before there is one: abi_fail(no_handle<H>, ...)
template <class H>
constexpr H* no_handle = nullptr;

template <class H>
int abi_fail(H* h, int code, const std::string& msg) {
  (h ? h->err : abi_slot<H>()) = msg;
  return code;
}
inline int abi_fail(std::nullptr_t, int code, const std::string& msg) {
  return abi_fail(static_cast<NoHandle*>(nullptr), code, msg);
}

template <class H>
const char* abi_last_error(const H* h) {
  return (h ? h->err : abi_slot<H>()).c_str();
}

// f() on h's device (h may be null: no device is selected); f returns a code, or nothing for
// MIDAGMA_OK.  A throw becomes its code (classify) and its message h's, as abi_fail leaves it.
template <class H, class F>
int abi_guarded(H* h, F&& f) {
  try {
    if (h) abi_select_device(h);
    if constexpr (std::is_void_v<decltype(f())>) {
      f();
      return MIDAGMA_OK;
    } else {
      return f();
    }
  } catch (...) {
    std::string msg;
    const int rc = classify(std::current_exception(), msg);
    return abi_fail(h, rc, msg);
  }
}
template <class F>
int abi_guarded(std::nullptr_t, F&& f) {
  return abi_guarded(static_cast<NoHandle*>(nullptr), std::forward<F>(f));
}

}  // namespace midagma

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "common.h"

namespace midagma {

struct HipError : DeviceError {
  hipError_t code;
  HipError(hipError_t e, const char* what, const char* file, int line)
      : DeviceError(std::string("HIP error ") + hipGetErrorString(e) + " at " + file + ":" + std::to_string(line) +
                    " (" + what + ")"),
        code(e) {}
};

// select `device` for the calling thread, or invalid_argument (who + "no such device")
inline void open_device(int device, const char* who) {
  int count = 0;
  HIP_TRY(hipGetDeviceCount(&count));
  if (device >= count) throw std::invalid_argument(std::string(who) + "no such device");
  HIP_TRY(hipSetDevice(device));
}

// invalid_argument unless ptr is device memory of `device`
inline void require_device_memory(const void* ptr, int device, const char* who) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, ptr) != hipSuccess || attr.type != hipMemoryTypeDevice ||
      attr.device != device) {
    (void)hipGetLastError();  // (a host pointer leaves a sticky error behind)
    throw std::invalid_argument(std::string(who) + ": X is not memory of the handle's device");
  }
}

// A device int that kernels raise on a bad value: cleared on st before them ...
inline void flag_clear(int* flag, hipStream_t st) { HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), st)); }
// ... and read back behind them: synchronises st, invalid_argument(msg) if it was raised
inline void flag_check(const int* flag, hipStream_t st, const std::string& msg) {
  int bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (bad) throw std::invalid_argument(msg);
}

}  // namespace midagma
#endif  // __HIPCC__
