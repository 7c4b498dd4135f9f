// What the pairwise test engines over the columns of one X share (dcor.hip, hsic.hip and, for the
// reductions, the bandwidths and the column lists, indep.hip), once: the limits and the shape
// check, the list of columns an entry names, the host's count of a permutation test, the
// fixed-order workgroup reductions, the device permutations (Philox keys through colsort.h's
// segmented sort), and the handle scaffolding of midagma_dcor and midagma_hsic, whose extern "C"
// entries forward to the templates here with the entry's name for the messages.
//
// The first part is plain C++ (tests/abi/coltest_test.cpp builds it with g++ under ASan/UBSan); the
// second is for the translation units hipcc builds.
#pragma once

#include <cstdint>
#include <vector>

namespace midagma {

constexpr int64_t kMaxD = 65535, kMaxP = 65535;
constexpr int64_t kMaxN = (int64_t(1) << 31) - 1;  // (indep.hip, the n^2 kernel, has its own)
constexpr int64_t kDefaultBudget = int64_t(2) << 30;

// why X (n x d, leading dimension ld) is no data for a handle, or nullptr
inline const char* bad_shape(const void* X, int64_t n, int64_t d, int64_t ld, int64_t max_n = kMaxN) {
  if (!X) return "null pointer";
  if (n < 2 || n > max_n) return "need 2 <= n < 2^31 rows";
  if (d < 1 || d > kMaxD) return "need 1 <= d <= 65535 columns";
  if (ld < d) return "the leading dimension is below d";
  return nullptr;
}

// list = the listed columns, each once, ascending (cols null: all d); or why not, and list is empty
inline const char* listed_columns(const int64_t* cols, int64_t ncols, int64_t d, std::vector<int64_t>& list) {
  list.clear();
  if (cols && ncols < 0) return "ncols < 0";
  std::vector<uint8_t> mark((size_t)d, cols ? 0 : 1);
  for (int64_t k = 0; cols && k < ncols; ++k) {
    if (cols[k] < 0 || cols[k] >= d) return "column index outside [0, d)";
    mark[cols[k]] = 1;
  }
  for (int64_t v = 0; v < d; ++v)
    if (mark[v]) list.push_back(v);
  return nullptr;
}

// The reference's permutation count of the pairs of a run, from the evaluations in order (of pair q
// the observed one, p = 0, first): stat[q] and null_out[q P + p - 1] (nullable) are the values
// reported, ge[q] = #{p >= 1 : compared_p >= compared_0}; a pair with a zero-range column
// (`zero`: the reference's centred matrix is exactly 0, mi_tests.py:21-27, 99-100) counts ge = P.
struct NullCount {
  double* stat;
  int64_t* ge;
  double* null_out;
  int64_t P;
  double obs = 0.0;  // the observed value of the pair whose permutations are being counted
  void add(int64_t q, int64_t p, double compared, double reported, bool zero) {
    if (p == 0) {
      obs = compared;
      stat[q] = reported;
      ge[q] = zero ? P : 0;
    } else {
      if (!zero && compared >= obs) ++ge[q];
      if (null_out) null_out[q * P + p - 1] = reported;
    }
  }
};

}  // namespace midagma

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "colsort.h"
#include "devmem.h"
#include "launch.h"
#include "philox.h"

namespace midagma {

// --- reductions over the workgroup (any multiple of 64 threads; w: a word a wave of LDS) ----------
// NW: the waves of the workgroup, for a kernel that every launch gives as many (0: blockDim.x / 64).
//
// the sum of v in a fixed order: the butterfly within a wave, then the waves ascending (4 waves:
// ((w0 + w1) + w2) + w3); valid in every thread
template <int NW = 0>
__device__ __forceinline__ double wg_sum(double v, double* w) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();  // (w may still be read from a previous call)
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = w[0];
  for (int k = 1, nw = NW ? NW : blockDim.x >> 6; k < nw; ++k) s += w[k];
  return s;
}

// (integer sums and minima do not depend on the order)
template <int NW = 0>
__device__ __forceinline__ long long wg_sum_ll(long long v, long long* w) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
  for (int k = 0, nw = NW ? NW : blockDim.x >> 6; k < nw; ++k) s += w[k];
  return s;
}

template <int NW = 0>
__device__ __forceinline__ double wg_min(double v, double* w) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = w[0];
  for (int k = 1, nw = NW ? NW : blockDim.x >> 6; k < nw; ++k) s = fmin(s, w[k]);
  return s;
}

// --- device permutations --------------------------------------------------------------------------
// Permutation f = q P + p - 1 of a run (pair q, p = 1 .. P) is the stable argsort over the rows a of
// the 64 Philox bits key(a) = (o.x << 32) | o.y, o = Philox4x32-10(counter (q, p - 1, a, 0), key
// (seed low word, seed high word)), at any n.
//
// the sort records of permutations f0 .. f0 + nseg - 1: K0[seg n + a] = key(a), I0[seg n + a] = a.
// grid (ceil(n / KT), nseg), KT threads.  (A template, as PermSort::run is: only a file that sorts
// permutations carries the kernel.)
template <int KT>
__global__ __launch_bounds__(KT) void perm_keys_kernel(uint32_t k0, uint32_t k1, int64_t f0, int64_t n, int64_t P,
                                                       uint64_t* __restrict__ K0, uint32_t* __restrict__ I0) {
  const int64_t a = (int64_t)blockIdx.x * KT + threadIdx.x, f = f0 + blockIdx.y;
  if (a >= n) return;
  const U4 o = philox4x32_10(U4{(uint32_t)(f / P), (uint32_t)(f % P), (uint32_t)a, 0u}, k0, k1);
  K0[(int64_t)blockIdx.y * n + a] = ((uint64_t)o.x << 32) | o.y;
  I0[(int64_t)blockIdx.y * n + a] = (uint32_t)a;
}

// bytes of sort scratch a permutation takes: the sort's two sides, its histogram, the OR and AND
inline int64_t perm_sort_bytes(int64_t n) { return 2 * n * 8 + 2 * n * 4 + segsort_hist_per_segment(n) * 4 + 16; }

// the sort's scratch (kept between runs, grow-only) and the launches
struct PermSort {
  DevBuf<uint64_t> keys;
  DevBuf<uint32_t> idx, hist;
  DevBuf<unsigned long long> oa;
  // permutations f0 .. f0 + nf - 1 of (seed) into perm (nf x n) and their inverses (nullable), on st
  template <int KT = 256>
  void run(uint64_t seed, int64_t f0, int64_t nf, int64_t P, int64_t n, int32_t* perm, int32_t* inverse,
           hipStream_t st) {
    keys.alloc((size_t)(2 * nf * n)), idx.alloc((size_t)(2 * nf * n));
    hist.alloc((size_t)(nf * segsort_hist_per_segment(n))), oa.alloc((size_t)(2 * nf));
    const SegSort s{keys.p, keys.p + nf * n, idx.p, idx.p + nf * n, oa.p, oa.p + nf, hist.p};
    // (every pass live: random keys share no digit, and a pass that moves nothing is still a stable pass)
    HIP_TRY(hipMemsetAsync(s.key_or, 0xff, (size_t)nf * 8, st));
    HIP_TRY(hipMemsetAsync(s.key_and, 0, (size_t)nf * 8, st));
    hipLaunchKernelGGL(perm_keys_kernel<KT>, dim3((unsigned)((n + KT - 1) / KT), (unsigned)nf), dim3(KT), 0, st,
                       (uint32_t)seed, (uint32_t)(seed >> 32), f0, n, P, s.K0, s.I0);
    HIP_TRY(hipGetLastError());
    launch_segsort(s, n, nf, st);
    launch_segsort_payload(s, n, nf, perm, inverse, st);
  }
};

// --- the handle of an engine over the columns of one X --------------------------------------------
// The device is opened by the first set_data*, not at create: until then no entry makes a device
// call, so the argument checks of every entry can be exercised on a machine without one.  A handle
// type H derives from ColHandle and has  void prepare(X_dev, n, d, ld, budget_bytes, stream):  the
// per-column pre-pass on `stream`, which it synchronises; it sets n, d and hzr.
struct ColHandle {
  int device = 0;
  int64_t n = 0, d = 0;  // 0 until a set_data* succeeded
  std::string err;
  hipStream_t comp = nullptr;  // null until the device is open
  std::vector<int32_t> hzr;    // d: the zero-range marks
  PermSort sort;
  DevBuf<int32_t> perm;
};

// abi.h's hook: an entry's device work runs on the handle's device once a set_data* has opened it
// (before that the handle's index may name no device, and no entry has device work)
inline void abi_select_device(const ColHandle* h) {
  if (h->comp) HIP_TRY(hipSetDevice(h->device));
}

inline std::string says(const char* who, const char* what) { return std::string(who) + ": " + what; }

template <class H>
int col_create(H** out, int device, const char* who) {
  if (!out || device < 0) return abi_fail(no_handle<H>, MIDAGMA_E_ARG, says(who, "bad arguments"));
  *out = new H;
  (*out)->device = device;
  return MIDAGMA_OK;
}

template <class H>
void col_destroy(H* h) {
  if (!h) return;
  if (h->comp) {  // (a handle that never opened its device owns nothing there, and its index may name none)
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->comp);
    (void)hipStreamDestroy(h->comp);
  }
  delete h;
}

// the first set_data* opens the handle's device and makes its stream
inline void col_open(ColHandle* h) {
  open_device(h->device, "");
  if (!h->comp) HIP_TRY(hipStreamCreateWithFlags(&h->comp, hipStreamNonBlocking));
}

template <class H>
int col_set_data(H* h, const char* who, const double* X, int64_t n, int64_t d, int64_t budget_bytes) {
  if (!h) return abi_fail(no_handle<H>, MIDAGMA_E_ARG, says(who, "null handle"));
  if (const char* why = bad_shape(X, n, d, d)) return abi_fail(h, MIDAGMA_E_ARG, says(who, why));
  h->n = h->d = 0;
  return abi_guarded(h, [&] {
    col_open(h);
    HIP_TRY(hipStreamSynchronize(h->comp));
    DevBuf<double> Xd;
    Xd.alloc((size_t)n * d);
    HIP_TRY(hipMemcpyAsync(Xd.p, X, (size_t)n * d * sizeof(double), hipMemcpyHostToDevice, h->comp));
    h->prepare(Xd.p, n, d, d, budget_bytes, h->comp);
  });
}

template <class H>
int col_set_data_dev(H* h, const char* who, const double* X_dev, int64_t n, int64_t d, int64_t ld,
                     int64_t budget_bytes, void* hip_stream) {
  if (!h) return abi_fail(no_handle<H>, MIDAGMA_E_ARG, says(who, "null handle"));
  if (const char* why = bad_shape(X_dev, n, d, ld)) return abi_fail(h, MIDAGMA_E_ARG, says(who, why));
  h->n = h->d = 0;  // the handle holds no data until the new one is checked
  return abi_guarded(h, [&] {
    col_open(h);
    require_device_memory(X_dev, h->device, who);
    HIP_TRY(hipStreamSynchronize(h->comp));  // nothing of an earlier run still reads the columns' arrays
    // on the caller's stream, behind X's producer; prepare's synchronise (the marks are read on the
    // host) also orders the arrays before everything the handle's own stream runs later
    h->prepare(X_dev, n, d, ld, budget_bytes, static_cast<hipStream_t>(hip_stream));
  });
}

// the P device permutations of pair q (P x n) to the host, with their inverses when `inverse`
// (its n words of device scratch) is given; inverse_out is nullable
template <class H>
int col_perms(H* h, const char* who, int64_t q, int64_t P, uint64_t seed, int32_t* perms_out,
              DevBuf<int32_t>* inverse, int32_t* inverse_out) {
  if (!h) return abi_fail(no_handle<H>, MIDAGMA_E_ARG, says(who, "null handle"));
  if (h->n == 0) return abi_fail(h, MIDAGMA_E_ARG, says(who, "set the data first"));
  if (q < 0 || q > 0xffffffffll || P < 1 || P > kMaxP || !perms_out)
    return abi_fail(h, MIDAGMA_E_ARG, says(who, "need 0 <= q < 2^32, 1 <= P <= 65535 and an output"));
  const int64_t n = h->n;
  return abi_guarded(h, [&] {
    for (int64_t p = 0; p < P; ++p) {  // (one at a time: the scratch of one evaluation)
      h->perm.alloc((size_t)n);
      if (inverse) inverse->alloc((size_t)n);
      h->sort.run(seed, q * P + p, 1, P, n, h->perm.p, inverse ? inverse->p : nullptr, h->comp);
      HIP_TRY(hipMemcpyAsync(perms_out + p * n, h->perm.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->comp));
      if (inverse_out)
        HIP_TRY(hipMemcpyAsync(inverse_out + p * n, inverse->p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->comp));
      HIP_TRY(hipStreamSynchronize(h->comp));
    }
  });
}

// c = 1 / (2 sigma^2) per column on the device of a handle with RBF bandwidths (d, comp, c,
// have_bw), then after(): what of the handle's the old bandwidths made is dropped
template <class H, class F>
int install_bandwidths(H* h, const double* sigma2, const char* who, F&& after) {
  const int64_t d = h->d;
  std::vector<double> c(d);
  for (int64_t v = 0; v < d; ++v) {
    if (!(sigma2[v] > 0.0) || !std::isfinite(sigma2[v]))
      return abi_fail(h, MIDAGMA_E_ARG, says(who, "squared bandwidths must be finite and > 0"));
    c[v] = 1.0 / (2.0 * sigma2[v]);
  }
  return abi_guarded(h, [&] {
    HIP_TRY(hipStreamSynchronize(h->comp));
    h->c.alloc(d);
    HIP_TRY(hipMemcpy(h->c.p, c.data(), d * sizeof(double), hipMemcpyHostToDevice));
    h->have_bw = true;
    after();
  });
}

}  // namespace midagma
#endif  // __HIPCC__
