// Pairwise permutation independence tests on the GPU (include/midagma_hip.h, midagma_indep_*):
// the reference's notreks/mi_tests.py, hsic_stat / dcor_stat under permutation_pvalue, for every
// pair of a pair list at once.  Everything is FP64.
//
// For a pair (i, j), x = X[:, i], y = X[:, j], and a permutation pi of the rows of y:
//   HSIC(x, y[pi])  = (1/n^2) sum_{a,b} Kc[a,b] exp(-(y[pi_a] - y[pi_b])^2 / (2 sigma_y^2))
//   dcov^2(x, y[pi]) = (1/n^2) sum_{a,b} Ax[a,b] |y[pi_a] - y[pi_b]|
// with Kc the double-centred RBF Gram of x and Ax its double-centred distance matrix.  The
// reference centres the y matrix too (mi_tests.py:21-27, 63-65, 92-95); those terms multiply the
// row sums of Kc / Ax, which are zero, so they drop out and nothing is re-centred per permutation.
// No n x n matrix is stored:
//   1. a per-variable pre-pass leaves the row means and the grand mean of the Gram / distance
//      matrix (and dvar^2 for dCor);
//   2. the main kernel's grid is (tile of the upper triangle a-tile <= b-tile, pair): a workgroup
//      builds its 64 x 64 tile of Kc / Ax once in registers (16 per thread; off-diagonal tiles
//      carry the weight 2 of their mirror image), then for the identity and every permutation
//      gathers the 64 + 64 values of y through the permutation into LDS, G permutations per
//      round, and leaves one partial sum per (pair, permutation, tile);
//   3. the final kernel sums the tiles of every (pair, permutation) in a fixed order and counts
//      ge = #{p : stat_p >= stat_obs}.
// No floating-point atomics: every sum has one fixed order that depends on n alone, so results
// are bit-identical from run to run and do not depend on how the pairs are split into batches.
//
// Device permutations (perms == NULL): pi for (pair q of the call, permutation p) is the stable
// argsort over a of the 64-bit key(a) = (((o.x << 32) | o.y) & ~0x3fff) | a, o = Philox4x32-10(
// counter = (q, p, a, 0), key = (seed low word, seed high word)): 50 random bits, then a itself
// (a < 2^14), so the keys are distinct and one unsigned compare orders them.  rank(a) is counted
// against every b, and pi[rank(a)] = a.
//
// Device data (midagma_indep_set_data_dev): indep_transpose_kernel writes XT from a row-major
// device X and ORs two flags per column (non-finite, differs from row 0) in a fixed order.
//
// Median bandwidths (midagma_indep_median_bandwidths): sigma^2 of a column is the median of its
// n (n - 1) / 2 squared differences.  With the column sorted, fl(x_b - x_a) is non-decreasing in b
// for fixed a and fl(t t) is monotone in |t|, so the k-th smallest squared difference is the square
// of the k-th smallest sorted-order difference, and #{a < b : fl(x_b - x_a) <= t} is a sum of
// per-row prefix lengths, each a binary search.  One workgroup per column sorts it in LDS and
// bisects over the bit pattern of the non-negative doubles: no n^2 values exist anywhere and the
// result is numpy's median bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../include/midagma_hip.h"
#include "coltest.h"

namespace midagma {
namespace {

constexpr int IT = 64;  // tile edge
constexpr int IG = 8;   // permutations per LDS round
constexpr int KIND_HSIC = 0, KIND_DCOR = 1;

template <int KIND>
__device__ __forceinline__ double kern(double dlt, double c) {
  if constexpr (KIND == KIND_HSIC)
    return exp(-(dlt * dlt) * c);
  else
    return fabs(dlt);
}

// PHASE 0: out[v][a] = mean_b k(x_a, x_b);  PHASE 1 (dCor): out[v][a] = sum_b Ax[a,b]^2.
// grid (n, d), 256 threads.
template <int KIND, int PHASE>
__global__ __launch_bounds__(256) void indep_row_kernel(const double* __restrict__ XT, const double* __restrict__ c,
                                                        const double* __restrict__ rm, const double* __restrict__ gm,
                                                        int n, double* __restrict__ out) {
  __shared__ double w[4];
  const int v = blockIdx.y, a = blockIdx.x;
  const double* x = XT + static_cast<int64_t>(v) * n;
  const double xa = x[a];
  const double cv = KIND == KIND_HSIC ? c[v] : 0.0;
  double s = 0.0;
  for (int b = threadIdx.x; b < n; b += 256) {
    const double k = kern<KIND>(xa - x[b], cv);
    if constexpr (PHASE == 0) {
      s += k;
    } else {
      const double* r = rm + static_cast<int64_t>(v) * n;
      const double ax = ((k - r[a]) - r[b]) + gm[v];
      s += ax * ax;
    }
  }
  s = wg_sum<4>(s, w);
  if (threadIdx.x == 0) out[static_cast<int64_t>(v) * n + a] = PHASE == 0 ? s / n : s;
}

// out[v] = (sum_a in[v][a]) / div: the grand mean from the row means, dvar^2 from the row sums
__global__ __launch_bounds__(256) void indep_col_kernel(const double* __restrict__ in, int n, double div,
                                                        double* __restrict__ out) {
  __shared__ double w[4];
  const int v = blockIdx.x;
  double s = 0.0;
  for (int a = threadIdx.x; a < n; a += 256) s += in[static_cast<int64_t>(v) * n + a];
  s = wg_sum<4>(s, w);
  if (threadIdx.x == 0) out[v] = s / div;
}

// perms[q][p][rank(a)] = a (see the head of the file); grid (ceil(n / (256 IPA)), P, pairs): a
// thread ranks IPA values of a against every b, the keys of 256 b at a time in LDS (each read is
// a broadcast)
constexpr int IPA = 4;
__global__ __launch_bounds__(256) void indep_perm_kernel(uint32_t k0, uint32_t k1, int64_t q0, int n, int P,
                                                         int32_t* __restrict__ perms) {
  __shared__ uint64_t keys[256];
  const int64_t ql = blockIdx.z;
  const uint32_t q = static_cast<uint32_t>(q0 + ql), p = blockIdx.y;
  auto key = [&](int i) -> uint64_t {
    const U4 o = philox4x32_10(U4{q, p, static_cast<uint32_t>(i), 0u}, k0, k1);
    return (((static_cast<uint64_t>(o.x) << 32) | o.y) & ~uint64_t(0x3fff)) | static_cast<uint64_t>(i);
  };
  int a[IPA], rank[IPA];
  uint64_t ka[IPA];
#pragma unroll
  for (int k = 0; k < IPA; ++k) {
    a[k] = (blockIdx.x * IPA + k) * 256 + threadIdx.x;
    ka[k] = key(a[k]);
    rank[k] = 0;
  }
  for (int c0 = 0; c0 < n; c0 += 256) {
    __syncthreads();
    keys[threadIdx.x] = key(c0 + threadIdx.x);
    __syncthreads();
    const int lim = min(256, n - c0);
    for (int b = 0; b < lim; ++b) {
      const uint64_t kb = keys[b];
#pragma unroll
      for (int k = 0; k < IPA; ++k) rank[k] += kb < ka[k] ? 1 : 0;
    }
  }
  // rank < n for a < n: it counts the b < n whose key is smaller, and a itself is not among them
#pragma unroll
  for (int k = 0; k < IPA; ++k)
    if (a[k] < n) perms[(ql * P + p) * n + rank[k]] = a[k];
}

// partial[q][p][t] for p = 0 (identity), 1 .. P; grid (ntiles, pairs), 256 threads.
// Thread (tx, ty) = (tid & 15, tid >> 4) holds rows r0 + ty + 16 u, columns c0 + tx + 16 v.
template <int KIND>
__global__ __launch_bounds__(256) void indep_main_kernel(const double* __restrict__ XT, const double* __restrict__ rm,
                                                         const double* __restrict__ gm, const double* __restrict__ c,
                                                         const int64_t* __restrict__ pairs,
                                                         const int32_t* __restrict__ perms, int n, int nt, int P,
                                                         double* __restrict__ partial) {
  __shared__ double yr[IG][IT], yc[IG][IT];
  __shared__ double wsum[IG][4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t q = blockIdx.y;
  const int t = blockIdx.x, ntiles = gridDim.x;
  int ti = 0, rem = t;
  while (rem >= nt - ti) {
    rem -= nt - ti;
    ++ti;
  }
  const int tj = ti + rem;
  const int r0 = ti * IT, c0 = tj * IT;
  const int64_t vi = pairs[2 * q], vj = pairs[2 * q + 1];
  const double* x = XT + vi * n;
  const double* y = XT + vj * n;
  const double* rx = rm + vi * n;
  const double gx = gm[vi];
  const double cx = KIND == KIND_HSIC ? c[vi] : 0.0, cy = KIND == KIND_HSIC ? c[vj] : 0.0;
  const double wt = ti == tj ? 1.0 : 2.0;

  double kc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int a = r0 + ty + 16 * u;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int b = c0 + tx + 16 * v;
      double val = 0.0;
      if (a < n && b < n) val = wt * (((kern<KIND>(x[a] - x[b], cx) - rx[a]) - rx[b]) + gx);
      kc[u][v] = val;
    }
  }

  for (int p0 = 0; p0 <= P; p0 += IG) {
    const int ng = min(IG, P + 1 - p0);
    for (int e = tid; e < IG * 2 * IT; e += 256) {
      const int g = e >> 7, k = e & 127, kk = k & 63;
      const bool row = k < 64;
      const int idx = (row ? r0 : c0) + kk;
      double val = 0.0;
      if (g < ng && idx < n) {
        const int p = p0 + g;
        const int src = p == 0 ? idx : perms[(q * P + (p - 1)) * n + idx];
        val = y[src];
      }
      if (row)
        yr[g][kk] = val;
      else
        yc[g][kk] = val;
    }
    __syncthreads();
    for (int g = 0; g < ng; ++g) {
      double ycv[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) ycv[v] = yc[g][tx + 16 * v];
      double s = 0.0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double yu = yr[g][ty + 16 * u];
#pragma unroll
        for (int v = 0; v < 4; ++v) s += kc[u][v] * kern<KIND>(yu - ycv[v], cy);
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
      if ((tid & 63) == 0) wsum[g][tid >> 6] = s;
    }
    __syncthreads();
    if (tid < ng)
      partial[(q * (P + 1) + p0 + tid) * ntiles + t] = ((wsum[tid][0] + wsum[tid][1]) + wsum[tid][2]) + wsum[tid][3];
  }
}

// vals[q][p] = the statistic of permutation p (0: observed) and ge[q]; grid (pairs), 256 threads:
// wave w sums the tiles of p = w, w + 4, ... (lane-strided, then the butterfly).  dCor: the count
// orders by dcov^2, the values are sqrt(max(dcov^2, 0)) / sqrt(sqrt(dvar_x^2 dvar_y^2)).
template <int KIND>
__global__ __launch_bounds__(256) void indep_final_kernel(const double* __restrict__ partial,
                                                          const int64_t* __restrict__ pairs,
                                                          const double* __restrict__ dvar, int n, int ntiles, int P,
                                                          double* __restrict__ vals, int64_t* __restrict__ ge) {
  __shared__ int cnt[4];
  const int64_t q = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* out = vals + q * (P + 1);
  const double nn = static_cast<double>(n) * static_cast<double>(n);
  for (int p = wave; p <= P; p += 4) {
    const double* src = partial + (q * (P + 1) + p) * ntiles;
    double s = 0.0;
    for (int t = lane; t < ntiles; t += 64) s += src[t];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[p] = s / nn;
  }
  __syncthreads();
  const double obs = out[0];
  int k = 0;
  for (int p = 1 + threadIdx.x; p <= P; p += 256) k += out[p] >= obs ? 1 : 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) k += __shfl_xor(k, off);
  if (lane == 0) cnt[wave] = k;
  __syncthreads();
  if (threadIdx.x == 0) ge[q] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
  if constexpr (KIND == KIND_DCOR) {
    const double vx = dvar[pairs[2 * q]], vy = dvar[pairs[2 * q + 1]];
    const bool degenerate = vx <= 0.0 || vy <= 0.0;
    const double den = degenerate ? 1.0 : sqrt(sqrt(vx * vy));
    for (int p = threadIdx.x; p <= P; p += 256) out[p] = degenerate ? 0.0 : sqrt(fmax(out[p], 0.0)) / den;
  }
}

// XT[v][a] = X[a][v] (X row-major n x d, row stride ld) and per-(row chunk, column) flag bytes:
// pflag[(chunk * 2 + 0) * d + v] = the chunk's rows of column v hold a non-finite value,
// pflag[(chunk * 2 + 1) * d + v] = one of them differs from row 0's.  grid (ceil(d / 32), chunks),
// 256 threads = 32 columns x 8 rows, 32 x 32 tiles through LDS (stride 33).
constexpr int TT = 32;
constexpr int TCHUNK = 1024;  // rows per workgroup
__global__ __launch_bounds__(256) void indep_transpose_kernel(const double* __restrict__ X, int n, int d, int64_t ld,
                                                              double* __restrict__ XT, uint8_t* __restrict__ pflag) {
  __shared__ double tile[TT][TT + 1];
  __shared__ uint32_t fl[8][TT];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = blockIdx.x * TT;
  const int rbeg = blockIdx.y * TCHUNK, rend = min(n, rbeg + TCHUNK);
  const int col = c0 + tx;
  const double first = col < d ? X[col] : 0.0;
  uint32_t f = 0;
  for (int r0 = rbeg; r0 < rend; r0 += TT) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + ty + 8 * u;
      double val = 0.0;
      if (r < rend && col < d) {
        val = X[static_cast<int64_t>(r) * ld + col];
        f |= (isfinite(val) ? 0u : 1u) | (val != first ? 2u : 0u);
      }
      tile[ty + 8 * u][tx] = val;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + ty + 8 * u, r = r0 + tx;
      if (c < d && r < rend) XT[static_cast<int64_t>(c) * n + r] = tile[tx][ty + 8 * u];
    }
    __syncthreads();
  }
  fl[ty][tx] = f;
  __syncthreads();
  if (ty == 0 && col < d) {
    uint32_t g = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) g |= fl[k][tx];
    const int64_t base = static_cast<int64_t>(blockIdx.y) * 2 * d;
    pflag[base + col] = g & 1u;
    pflag[base + d + col] = (g >> 1) & 1u;
  }
}

// flag[k * d + v] = OR over the chunks of pflag[(chunk * 2 + k) * d + v], k = 0, 1
__global__ __launch_bounds__(256) void indep_flag_kernel(const uint8_t* __restrict__ pflag, int chunks, int d,
                                                         uint8_t* __restrict__ flag) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= 2 * static_cast<int64_t>(d)) return;
  uint8_t g = 0;
  for (int c = 0; c < chunks; ++c) g |= pflag[static_cast<int64_t>(c) * 2 * d + i];
  flag[i] = g;
}

// rows a < b of the sorted column xs[0 .. n) with fl(xs[b] - xs[a]) <= t, for this thread's rows
// a = tid, tid + threads, ...: per row the length of the prefix of b = a + 1 .. n - 1 (the
// differences are non-decreasing in b), by binary search.  MINNEXT: also the smallest difference
// above t over these rows (+inf when there is none).
template <bool MINNEXT>
__device__ __forceinline__ long long median_count(const double* xs, int n, double t, double* next) {
  long long cnt = 0;
  double mn = INFINITY;
  for (int a = threadIdx.x; a < n - 1; a += blockDim.x) {
    const double xa = xs[a];
    int lo = a + 1, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (xs[mid] - xa <= t)
        lo = mid + 1;
      else
        hi = mid;
    }
    cnt += lo - (a + 1);
    if constexpr (MINNEXT)
      if (lo < n) mn = fmin(mn, xs[lo] - xa);
  }
  if constexpr (MINNEXT) *next = mn;
  return cnt;
}

// med[v] = the reference's median-heuristic sigma^2 of column v = cols[blockIdx.x] (cols null:
// blockIdx.x): the median of the squared differences of all pairs of rows, 1.0 when that is not
// > 0.  One workgroup per column, blockDim.x threads (a multiple of 64), sz doubles of dynamic LDS,
// sz the power of two >= n.  The column is sorted by a bitonic network (padding +inf), then the
// k-th smallest sorted-order difference is the smallest non-negative double t (bisection over
// its 63-bit pattern) with #{a < b : fl(x_b - x_a) <= t} >= k + 1.  M = n (n - 1) / 2 odd: element
// M / 2; even: numpy's mean of elements M / 2 - 1 and M / 2, the second being the first again when
// more than M / 2 differences are <= it, else the smallest difference above it.
__global__ __launch_bounds__(1024) void indep_median_kernel(const double* __restrict__ XT,
                                                            const int64_t* __restrict__ cols, int n, int sz,
                                                            double* __restrict__ med) {
  extern __shared__ double xs[];
  __shared__ long long wsum[16];
  __shared__ double wmin[16];
  const int64_t v = cols ? cols[blockIdx.x] : blockIdx.x;
  const double* x = XT + v * n;
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int i = tid; i < sz; i += nthr) xs[i] = i < n ? x[i] : INFINITY;
  __syncthreads();
  for (int k = 2; k <= sz; k <<= 1)
    for (int j = k >> 1; j >= 1; j >>= 1) {
      for (int t = tid; t < (sz >> 1); t += nthr) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;  // bit j of i is clear
        const double p = xs[i], q = xs[l];
        if ((p > q) == ((i & k) == 0)) {
          xs[i] = q;
          xs[l] = p;
        }
      }
      __syncthreads();
    }
  const long long M = static_cast<long long>(n) * (n - 1) / 2;
  const long long k = (M & 1) ? M / 2 : M / 2 - 1;
  // count(+inf) = M >= k + 1: every difference of finite values is <= +inf
  unsigned long long lo = 0, hi = 0x7ff0000000000000ull;
  while (lo < hi) {
    const unsigned long long mid = lo + ((hi - lo) >> 1);
    const long long c = wg_sum_ll(median_count<false>(xs, n, __longlong_as_double(mid), nullptr), wsum);
    if (c >= k + 1)
      hi = mid;
    else
      lo = mid + 1;
  }
  const double vk = __longlong_as_double(lo);
  double m = vk * vk;
  if (!(M & 1)) {
    double next;
    const long long c = wg_sum_ll(median_count<true>(xs, n, vk, &next), wsum);
    const double above = wg_min(next, wmin);
    const double vn = c > M / 2 ? vk : above;
    m = (m + vn * vn) / 2.0;
  }
  if (tid == 0) med[v] = m > 0.0 ? m : 1.0;
}

}  // namespace
}  // namespace midagma

using namespace midagma;

namespace {

constexpr int64_t kMaxRows = 16384, kMaxBatchPairs = 32768;  // (the n^2 kernel; kMaxD and kMaxP are coltest.h's)
constexpr int64_t kBatchBudget = int64_t(128) << 20;

struct Slot {
  PinBuf<int32_t> hperm;
  PinBuf<int64_t> hpairs, hge;
  PinBuf<double> hvals;
  DevBuf<int32_t> dperm;
  DevBuf<int64_t> dpairs, dge;
  DevBuf<double> partial, dvals;
  // up0 .. up: the batch's upload (copy stream); k0 .. k1: its permutation kernel; k1 .. k2: its
  // statistic kernels; done: its results are on the host (compute stream)
  Event up0, up, k0, k1, k2, done;
  int64_t q0 = 0, mb = 0;
  bool busy = false;
};

}  // namespace

struct midagma_indep {
  int device = 0;
  int64_t n = 0, d = 0;
  std::string err;
  hipStream_t comp = nullptr, copy = nullptr;
  DevBuf<double> XT, rm[2], gm[2], dvar, c, rowtmp, med;
  DevBuf<uint8_t> pflag, flag;    // set_data_dev: per-chunk and per-column flag bytes
  DevBuf<int64_t> dcols;          // median_bandwidths: the listed columns
  std::vector<uint8_t> constant;  // zero-range columns: the reference's all-zero centred matrix
  bool have_bw = false, have_stats[2] = {false, false};
  Slot slot[2];
  double prof[4] = {0, 0, 0, 0};  // the last run's stage times (midagma_indep_profile), ms
  Event bw0, bw1;      // around the median kernel
  double bw_ms = 0.0;  // the last median_bandwidths' kernel time, ms
};

// abi.h's hook: an entry's device work runs on the handle's device
static void abi_select_device(const midagma_indep* h) { HIP_TRY(hipSetDevice(h->device)); }

namespace {

int64_t tiles_of(int64_t n) {
  const int64_t nt = (n + IT - 1) / IT;
  return nt * (nt + 1) / 2;
}

// device + pinned bytes one pair of a batch takes in one of the two slots
int64_t pair_bytes(int64_t n, int64_t P) {
  return P * n * 4 + (P + 1) * tiles_of(n) * 8 + (P + 1) * 8 + 24;
}

int64_t batch_pairs(int64_t n, int64_t P, int64_t budget) {
  if (budget <= 0) budget = kBatchBudget;
  return std::min<int64_t>(kMaxBatchPairs, std::max<int64_t>(1, budget / (2 * pair_bytes(n, P))));
}

// the per-variable pre-pass of one kind, on the compute stream
void prepare_stats(midagma_indep* h, int kind) {
  if (h->have_stats[kind]) return;
  const int n = static_cast<int>(h->n), d = static_cast<int>(h->d);
  const size_t nd = static_cast<size_t>(n) * d;
  h->rm[kind].alloc(nd);
  h->gm[kind].alloc(d);
  const dim3 grid(n, d);
  if (kind == KIND_HSIC) {
    hipLaunchKernelGGL((indep_row_kernel<KIND_HSIC, 0>), grid, dim3(256), 0, h->comp, h->XT.p, h->c.p, nullptr, nullptr,
                       n, h->rm[kind].p);
    hipLaunchKernelGGL(indep_col_kernel, dim3(d), dim3(256), 0, h->comp, h->rm[kind].p, n, static_cast<double>(n),
                       h->gm[kind].p);
  } else {
    h->dvar.alloc(d);
    h->rowtmp.alloc(nd);
    hipLaunchKernelGGL((indep_row_kernel<KIND_DCOR, 0>), grid, dim3(256), 0, h->comp, h->XT.p, nullptr, nullptr,
                       nullptr, n, h->rm[kind].p);
    hipLaunchKernelGGL(indep_col_kernel, dim3(d), dim3(256), 0, h->comp, h->rm[kind].p, n, static_cast<double>(n),
                       h->gm[kind].p);
    hipLaunchKernelGGL((indep_row_kernel<KIND_DCOR, 1>), grid, dim3(256), 0, h->comp, h->XT.p, nullptr, h->rm[kind].p,
                       h->gm[kind].p, n, h->rowtmp.p);
    hipLaunchKernelGGL(indep_col_kernel, dim3(d), dim3(256), 0, h->comp, h->rowtmp.p, n,
                       static_cast<double>(n) * static_cast<double>(n), h->dvar.p);
  }
  HIP_TRY(hipGetLastError());
  h->have_stats[kind] = true;
}

}  // namespace

extern "C" const char* midagma_indep_last_error(const midagma_indep* h) { return abi_last_error(h); }

extern "C" int midagma_indep_create(midagma_indep** out, int device) {
  if (!out || device < 0) return abi_fail(no_handle<midagma_indep>, MIDAGMA_E_ARG, "indep_create: bad arguments");
  *out = nullptr;
  midagma_indep* h = nullptr;
  const int rc = abi_guarded(no_handle<midagma_indep>, [&] {
    open_device(device, "indep_create: ");
    h = new midagma_indep;
    h->device = device;
    HIP_TRY(hipStreamCreateWithFlags(&h->comp, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&h->copy, hipStreamNonBlocking));
    for (Slot& s : h->slot) {
      for (Event* e : {&s.up0, &s.up, &s.k0, &s.k1, &s.k2}) e->create();
      s.done.create(hipEventDisableTiming);
    }
    h->bw0.create();
    h->bw1.create();
  });
  if (rc != MIDAGMA_OK) {
    midagma_indep_destroy(h);
    return rc;
  }
  *out = h;
  return MIDAGMA_OK;
}

extern "C" void midagma_indep_destroy(midagma_indep* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->comp) (void)hipStreamSynchronize(h->comp);
  if (h->copy) (void)hipStreamSynchronize(h->copy);
  if (h->comp) (void)hipStreamDestroy(h->comp);
  if (h->copy) (void)hipStreamDestroy(h->copy);
  delete h;
}

extern "C" int midagma_indep_set_data(midagma_indep* h, const double* X, int64_t n, int64_t d) {
  if (!h) return abi_fail(no_handle<midagma_indep>, MIDAGMA_E_ARG, "indep_set_data: null handle");
  if (!X || n < 2 || n > kMaxRows || d < 1 || d > kMaxD)
    return abi_fail(h, MIDAGMA_E_ARG, "indep_set_data: need X, 2 <= n <= 16384 and 1 <= d <= 65535");
  std::vector<double> xt(static_cast<size_t>(n) * d);
  std::vector<uint8_t> constant(d, 1);
  for (int64_t a = 0; a < n; ++a)
    for (int64_t v = 0; v < d; ++v) {
      const double val = X[a * d + v];
      if (!std::isfinite(val)) return abi_fail(h, MIDAGMA_E_ARG, "indep_set_data: X holds inf or nan");
      xt[v * n + a] = val;
      if (val != X[v]) constant[v] = 0;
    }
  return abi_guarded(h, [&] {
    HIP_TRY(hipStreamSynchronize(h->comp));
    h->XT.alloc(xt.size());
    HIP_TRY(hipMemcpy(h->XT.p, xt.data(), xt.size() * sizeof(double), hipMemcpyHostToDevice));
    h->n = n;
    h->d = d;
    h->constant.swap(constant);
    h->have_bw = h->have_stats[0] = h->have_stats[1] = false;
  });
}

extern "C" int midagma_indep_set_data_dev(midagma_indep* h, const double* X_dev, int64_t n, int64_t d, int64_t ld,
                                          void* hip_stream) {
  if (!h) return abi_fail(no_handle<midagma_indep>, MIDAGMA_E_ARG, "indep_set_data_dev: null handle");
  if (!X_dev || n < 2 || n > kMaxRows || d < 1 || d > kMaxD || ld < d)
    return abi_fail(h, MIDAGMA_E_ARG, "indep_set_data_dev: need X, 2 <= n <= 16384, 1 <= d <= 65535 and ld >= d");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  std::vector<uint8_t> flags(2 * d);
  h->n = h->d = 0;  // the handle holds no data until the new one is checked
  h->have_bw = h->have_stats[0] = h->have_stats[1] = false;
  const int rc = abi_guarded(h, [&] {
    require_device_memory(X_dev, h->device, "indep_set_data_dev");
    HIP_TRY(hipStreamSynchronize(h->comp));  // nothing of an earlier run still reads XT
    const int chunks = static_cast<int>((n + TCHUNK - 1) / TCHUNK);
    h->XT.alloc(static_cast<size_t>(n) * d);
    h->pflag.alloc(static_cast<size_t>(chunks) * 2 * d);
    h->flag.alloc(2 * d);
    // on the caller's stream, behind X's producer; the synchronise below (the flags are read on the
    // host) also orders XT before everything the handle's own streams run later
    hipLaunchKernelGGL(indep_transpose_kernel, dim3((d + TT - 1) / TT, chunks), dim3(256), 0, s, X_dev,
                       static_cast<int>(n), static_cast<int>(d), ld, h->XT.p, h->pflag.p);
    hipLaunchKernelGGL(indep_flag_kernel, dim3((2 * d + 255) / 256), dim3(256), 0, s, h->pflag.p, chunks,
                       static_cast<int>(d), h->flag.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(flags.data(), h->flag.p, 2 * d, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  });
  if (rc != MIDAGMA_OK) return rc;
  for (int64_t v = 0; v < d; ++v)
    if (flags[v]) return abi_fail(h, MIDAGMA_E_ARG, "indep_set_data_dev: X holds inf or nan");
  h->constant.assign(d, 0);
  for (int64_t v = 0; v < d; ++v) h->constant[v] = flags[d + v] ? 0 : 1;
  h->n = n;
  h->d = d;
  return MIDAGMA_OK;
}

extern "C" int midagma_indep_set_bandwidths(midagma_indep* h, const double* sigma2, int64_t d) {
  if (!h) return abi_fail(no_handle<midagma_indep>, MIDAGMA_E_ARG, "indep_set_bandwidths: null handle");
  if (h->n == 0) return abi_fail(h, MIDAGMA_E_ARG, "indep_set_bandwidths: set the data first");
  if (!sigma2 || d != h->d) return abi_fail(h, MIDAGMA_E_ARG, "indep_set_bandwidths: need d squared bandwidths");
  // (the HSIC pre-pass is redone)
  return install_bandwidths(h, sigma2, "indep_set_bandwidths", [h] { h->have_stats[KIND_HSIC] = false; });
}

extern "C" int midagma_indep_median_bandwidths(midagma_indep* h, const int64_t* cols, int64_t ncols,
                                               double* sigma2_out) {
  if (!h) return abi_fail(no_handle<midagma_indep>, MIDAGMA_E_ARG, "indep_median_bandwidths: null handle");
  if (h->n == 0) return abi_fail(h, MIDAGMA_E_ARG, "indep_median_bandwidths: set the data first");
  const int64_t n = h->n, d = h->d;
  std::vector<int64_t> list;  // (a column's value does not depend on the list)
  if (const char* why = listed_columns(cols, ncols, d, list))
    return abi_fail(h, MIDAGMA_E_ARG, says("indep_median_bandwidths", why));
  const int64_t m = static_cast<int64_t>(list.size());
  std::vector<double> med(d), s2(d, 1.0);
  h->bw_ms = 0.0;
  if (m > 0) {
    const int rc = abi_guarded(h, [&] {
      int sz = 2;
      while (sz < n) sz <<= 1;
      const int threads = sz <= 2048 ? 256 : 1024;
      const size_t lds = static_cast<size_t>(sz) * sizeof(double);
      if (lds > (size_t(48) << 10))
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(indep_median_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
      h->med.alloc(d);
      if (cols) {
        h->dcols.alloc(list.size());
        HIP_TRY(hipMemcpyAsync(h->dcols.p, list.data(), list.size() * sizeof(int64_t), hipMemcpyHostToDevice,
                               h->comp));
      }
      HIP_TRY(hipEventRecord(h->bw0, h->comp));
      hipLaunchKernelGGL(indep_median_kernel, dim3(m), dim3(threads), lds, h->comp, h->XT.p,
                         cols ? h->dcols.p : nullptr, static_cast<int>(n), sz, h->med.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(h->bw1, h->comp));
      HIP_TRY(hipMemcpyAsync(med.data(), h->med.p, d * sizeof(double), hipMemcpyDeviceToHost, h->comp));
      HIP_TRY(hipStreamSynchronize(h->comp));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, h->bw0, h->bw1));
      h->bw_ms = ms;
    });
    if (rc != MIDAGMA_OK) return rc;
    for (int64_t v : list) s2[v] = med[v];
  }
  const int rc =
      install_bandwidths(h, s2.data(), "indep_median_bandwidths", [h] { h->have_stats[KIND_HSIC] = false; });
  if (rc != MIDAGMA_OK) return rc;
  if (sigma2_out) std::copy(s2.begin(), s2.end(), sigma2_out);
  return MIDAGMA_OK;
}

extern "C" int midagma_indep_bandwidth_profile(const midagma_indep* h, double* ms_out) {
  if (!h || !ms_out) return abi_fail(no_handle<midagma_indep>, MIDAGMA_E_ARG, "indep_bandwidth_profile: bad arguments");
  *ms_out = h->bw_ms;
  return MIDAGMA_OK;
}

extern "C" int64_t midagma_indep_batch_pairs(const midagma_indep* h, int64_t P, int64_t budget_bytes) {
  if (!h || h->n == 0 || P < 0 || P > kMaxP) return 0;
  return batch_pairs(h->n, P, budget_bytes);
}

extern "C" int midagma_indep_profile(const midagma_indep* h, double* ms_out) {
  if (!h || !ms_out) return abi_fail(no_handle<midagma_indep>, MIDAGMA_E_ARG, "indep_profile: bad arguments");
  std::copy(h->prof, h->prof + 4, ms_out);
  return MIDAGMA_OK;
}

extern "C" int midagma_indep_run(midagma_indep* h, int kind, const int64_t* pairs, int64_t m, int64_t P,
                                 const int32_t* perms, uint64_t seed, int64_t budget_bytes, double* stat, int64_t* ge,
                                 double* null_out, int32_t* perms_out) {
  if (!h) return abi_fail(no_handle<midagma_indep>, MIDAGMA_E_ARG, "indep_run: null handle");
  if ((kind != KIND_HSIC && kind != KIND_DCOR) || m < 0 || P < 0 || P > kMaxP || (m > 0 && (!pairs || !stat || !ge)))
    return abi_fail(h, MIDAGMA_E_ARG, "indep_run: bad arguments (kind 0 hsic / 1 dcor, 0 <= P <= 65535)");
  if (h->n == 0) return abi_fail(h, MIDAGMA_E_ARG, "indep_run: set the data first");
  if (kind == KIND_HSIC && !h->have_bw) return abi_fail(h, MIDAGMA_E_ARG, "indep_run: hsic needs the bandwidths");
  const int64_t n = h->n, d = h->d;
  for (int64_t k = 0; k < 2 * m; ++k)
    if (pairs[k] < 0 || pairs[k] >= d) return abi_fail(h, MIDAGMA_E_ARG, "indep_run: pair index outside [0, d)");
  if (2 * pair_bytes(n, P) > (int64_t(8) << 30)) return abi_fail(h, MIDAGMA_E_ARG, "indep_run: P too large for this n");
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
  h->prof[0] = h->prof[1] = h->prof[2] = h->prof[3] = 0.0;
  const clock::time_point t_check = clock::now();
  if (perms)  // every index is read as an address offset on the device
    for (int64_t k = 0, e = m * P * n; k < e; ++k)
      if (perms[k] < 0 || perms[k] >= n)
        return abi_fail(h, MIDAGMA_E_ARG, "indep_run: permutation index outside [0, n)");
  h->prof[0] += ms_since(t_check);
  if (m == 0) return MIDAGMA_OK;

  const int64_t mbmax = std::min(m, batch_pairs(n, P, budget_bytes));
  const int64_t ntiles = tiles_of(n), nt = (n + IT - 1) / IT, P1 = P + 1;
  const bool device_perms = perms == nullptr;

  auto collect = [&](Slot& s) {
    if (!s.busy) return;
    HIP_TRY(hipEventSynchronize(s.done));
    s.busy = false;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s.up0, s.up));
    h->prof[1] += ms;
    HIP_TRY(hipEventElapsedTime(&ms, s.k0, s.k1));
    h->prof[2] += ms;
    HIP_TRY(hipEventElapsedTime(&ms, s.k1, s.k2));
    h->prof[3] += ms;
    for (int64_t k = 0; k < s.mb; ++k) {
      const int64_t q = s.q0 + k;
      // a zero-range column: the reference's centred matrix is exactly 0 (mi_tests.py:21-27, 99-100)
      const bool zero = h->constant[pairs[2 * q]] || h->constant[pairs[2 * q + 1]];
      stat[q] = zero ? 0.0 : s.hvals.p[k * P1];
      ge[q] = zero ? P : s.hge.p[k];
      if (null_out)
        for (int64_t p = 0; p < P; ++p) null_out[q * P + p] = zero ? 0.0 : s.hvals.p[k * P1 + 1 + p];
    }
    if (perms_out && device_perms && P > 0)
      HIP_TRY(hipMemcpy(perms_out + s.q0 * P * n, s.dperm.p, s.mb * P * n * sizeof(int32_t), hipMemcpyDeviceToHost));
  };

  const int rc = abi_guarded(h, [&] {
    prepare_stats(h, kind);
    int64_t b = 0;
    for (int64_t q0 = 0; q0 < m; q0 += mbmax, ++b) {
      Slot& s = h->slot[b & 1];
      collect(s);  // batch b - 2: its kernels are done, its buffers free
      const int64_t mb = std::min(mbmax, m - q0);
      s.q0 = q0;
      s.mb = mb;
      s.hpairs.alloc(2 * mb), s.dpairs.alloc(2 * mb);
      s.hge.alloc(mb), s.dge.alloc(mb);
      s.hvals.alloc(mb * P1), s.dvals.alloc(mb * P1);
      s.partial.alloc(mb * P1 * ntiles);
      s.dperm.alloc(mb * P * n);
      std::memcpy(s.hpairs.p, pairs + 2 * q0, 2 * mb * sizeof(int64_t));
      HIP_TRY(hipEventRecord(s.up0, h->copy));
      HIP_TRY(hipMemcpyAsync(s.dpairs.p, s.hpairs.p, 2 * mb * sizeof(int64_t), hipMemcpyHostToDevice, h->copy));
      if (!device_perms && P > 0) {
        s.hperm.alloc(mb * P * n);
        const clock::time_point t_stage = clock::now();
        std::memcpy(s.hperm.p, perms + q0 * P * n, mb * P * n * sizeof(int32_t));
        h->prof[0] += ms_since(t_stage);
        HIP_TRY(hipMemcpyAsync(s.dperm.p, s.hperm.p, mb * P * n * sizeof(int32_t), hipMemcpyHostToDevice, h->copy));
      }
      HIP_TRY(hipEventRecord(s.up, h->copy));
      HIP_TRY(hipStreamWaitEvent(h->comp, s.up, 0));
      HIP_TRY(hipEventRecord(s.k0, h->comp));
      if (device_perms && P > 0)
        hipLaunchKernelGGL(indep_perm_kernel, dim3((n + 256 * IPA - 1) / (256 * IPA), P, mb), dim3(256), 0, h->comp,
                           static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), q0, static_cast<int>(n),
                           static_cast<int>(P), s.dperm.p);
      HIP_TRY(hipEventRecord(s.k1, h->comp));
      const dim3 grid(ntiles, mb);
      if (kind == KIND_HSIC) {
        hipLaunchKernelGGL(indep_main_kernel<KIND_HSIC>, grid, dim3(256), 0, h->comp, h->XT.p, h->rm[kind].p,
                           h->gm[kind].p, h->c.p, s.dpairs.p, s.dperm.p, static_cast<int>(n), static_cast<int>(nt),
                           static_cast<int>(P), s.partial.p);
        hipLaunchKernelGGL(indep_final_kernel<KIND_HSIC>, dim3(mb), dim3(256), 0, h->comp, s.partial.p, s.dpairs.p,
                           nullptr, static_cast<int>(n), static_cast<int>(ntiles), static_cast<int>(P), s.dvals.p,
                           s.dge.p);
      } else {
        hipLaunchKernelGGL(indep_main_kernel<KIND_DCOR>, grid, dim3(256), 0, h->comp, h->XT.p, h->rm[kind].p,
                           h->gm[kind].p, nullptr, s.dpairs.p, s.dperm.p, static_cast<int>(n), static_cast<int>(nt),
                           static_cast<int>(P), s.partial.p);
        hipLaunchKernelGGL(indep_final_kernel<KIND_DCOR>, dim3(mb), dim3(256), 0, h->comp, s.partial.p, s.dpairs.p,
                           h->dvar.p, static_cast<int>(n), static_cast<int>(ntiles), static_cast<int>(P), s.dvals.p,
                           s.dge.p);
      }
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(s.k2, h->comp));
      HIP_TRY(hipMemcpyAsync(s.hvals.p, s.dvals.p, mb * P1 * sizeof(double), hipMemcpyDeviceToHost, h->comp));
      HIP_TRY(hipMemcpyAsync(s.hge.p, s.dge.p, mb * sizeof(int64_t), hipMemcpyDeviceToHost, h->comp));
      HIP_TRY(hipEventRecord(s.done, h->comp));
      s.busy = true;
    }
    // the two batches still in flight, older first
    collect(h->slot[b & 1]);
    collect(h->slot[(b + 1) & 1]);
  });
  if (rc != MIDAGMA_OK) {
    // leave nothing in flight that reads the slots
    (void)hipStreamSynchronize(h->copy);
    (void)hipStreamSynchronize(h->comp);
    h->slot[0].busy = h->slot[1].busy = false;
  }
  return rc;
}
