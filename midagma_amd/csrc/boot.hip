// Bootstrap covariances for a batch (midagma_boot_*): replicate b of (seed) resamples the n rows of
// one X with replacement, and its covariance goes straight into problem b's cov slab of a
// midagma_batch, so the B resamples are never gathered and X is read from where it lies.
//
// The resampling rule (shared with midagma_amd.batch.bootstrap_indices): draw j of replicate b is
//   o = Philox4x32-10(counter (j, b, 0, 0), key (seed lo, seed hi)),  r = (o0 << 32) | o1,
//   idx[j] = (r * n) >> 64.
// With c_bi = how often row i is drawn and Y = X centred once by its global column mean,
//   cov_b = (S_b - t_b t_b^T / n) / n,   S_b = sum_i c_bi y_i y_i^T,   t_b = sum_i c_bi y_i,
// which is the covariance of the resample (translation invariant; the global centring keeps
// t_b / n at O(n^-1/2) of a column's spread whatever offset X carries).
//
// Three launches per chunk of replicates, none waiting on another workgroup:
//   boot_counts_kernel   one thread per (replicate, draw): Philox, int32 atomicAdd into cnt[b][idx]
//   boot_gram_kernel     a workgroup owns R replicates and one range of rows; every 64-row tile of Y
//                        is staged in LDS once and serves all R replicates (A operand c_bi y_im,
//                        B operand y_in on v_mfma_f64_16x16x4_f64); t_b from VALU sums of the A
//                        operands; one DS x DS + DS partial per (replicate, range)
//   boot_finish_kernel   sums a replicate's partials in ascending range order, applies
//                        (S - t t^T / n) / n and writes the zero-padded slab
// The ranges are a function of n alone and a replicate's sums run over its rows in ascending order,
// so cov_b depends only on (X, seed, b): not on B, the grouping, the chunking or the residency.
// Only the blocks on and above the diagonal are accumulated; the finish mirrors them, so cov_b is
// exactly symmetric.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "batch_impl.h"
#include "mfma64.h"
#include "philox.h"

namespace {

constexpr int BT_ROWS = 64;        // rows of Y per LDS tile
constexpr int BT_MAX_RANGES = 32;  // row ranges (partials) per replicate at most
constexpr int BT_MIN_RANGE = 256;  // rows per range at least (a multiple of BT_ROWS)
constexpr int64_t BT_DEFAULT_BUDGET = int64_t(1) << 30;

// replicates per wave (each wave accumulates whole DS x DS upper triangles of blocks), and the
// row stride of the LDS image of a Y tile: = 16 mod 32 doubles, so the ds_read_b64 of rows
// {k, k + 1} x 16 columns by a 32-lane group is conflict-free (common.h, SB)
__host__ __device__ constexpr int boot_rw(int DS) { return DS == 64 ? 2 : (DS == 32 ? 4 : 8); }
__host__ __device__ constexpr int boot_stride(int DS) { return DS == 16 ? 16 : DS + 16; }

struct BootPlan {
  int64_t range_rows = 0;
  int nranges = 0;
};
BootPlan boot_plan(int64_t n) {
  BootPlan p;
  const int64_t per = std::max<int64_t>((n + BT_MAX_RANGES - 1) / BT_MAX_RANGES, BT_MIN_RANGE);
  p.range_rows = (per + BT_ROWS - 1) / BT_ROWS * BT_ROWS;
  p.nranges = (int)((n + p.range_rows - 1) / p.range_rows);
  return p;
}

// cnt[bl][idx] += 1 for draw j of replicate first + bl.  grid (ceil(n / 256), replicates)
__global__ void boot_counts_kernel(int32_t* __restrict__ cnt, int64_t n, uint32_t first, uint32_t k0, uint32_t k1) {
  const int64_t j = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (j >= n) return;
  const int64_t bl = blockIdx.y;
  const U4 o = philox4x32_10(U4{(uint32_t)j, first + (uint32_t)bl, 0u, 0u}, k0, k1);
  const uint64_t r = ((uint64_t)o.x << 32) | o.y;
  const int64_t idx = (int64_t)__umul64hi(r, (uint64_t)n);  // < n
  atomicAdd(&cnt[bl * n + idx], 1);
}

// part[(bl * nranges + range) * (DS * DS + DS)]: the blocks (i <= j) of S_b over the range's rows,
// then t_b.  grid (ceil(nb / R), nranges), R = 4 boot_rw(DS) replicates per workgroup: wave w owns
// replicates g R + w RW .. + RW - 1.  Y: n x DS row-major, zero padding.
template <int DS>
__global__ __launch_bounds__(NTHREADS) void boot_gram_kernel(const double* __restrict__ Y,
                                                             const int32_t* __restrict__ cnt, int64_t n, int64_t nb,
                                                             int64_t range_rows, int nranges,
                                                             double* __restrict__ part) {
  constexpr int NB = DS / 16, RW = boot_rw(DS), R = 4 * RW, S = boot_stride(DS);
  __shared__ __attribute__((aligned(16))) double Ys[BT_ROWS * S];
  __shared__ double cs[R * BT_ROWS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const int64_t g = blockIdx.x;
  const int range = blockIdx.y;
  const int64_t row0 = (int64_t)range * range_rows, row1 = std::min<int64_t>(n, row0 + range_rows);

  dbl4 acc[RW][NB][NB];
  double tac[RW][NB];
#pragma unroll
  for (int q = 0; q < RW; ++q)
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      tac[q][i] = 0.0;
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[q][i][j] = dbl4{0.0, 0.0, 0.0, 0.0};
    }

  for (int64_t t0 = row0; t0 < row1; t0 += BT_ROWS) {
    __syncthreads();  // the last tile's reads are done
    for (int item = threadIdx.x; item < BT_ROWS * DS / 2; item += NTHREADS) {
      const int row = item / (DS / 2), c = (item % (DS / 2)) * 2;
      double2 v = make_double2(0.0, 0.0);
      if (t0 + row < row1) v = *reinterpret_cast<const double2*>(Y + (t0 + row) * DS + c);
      *reinterpret_cast<double2*>(Ys + row * S + c) = v;
    }
    for (int item = threadIdx.x; item < R * BT_ROWS; item += NTHREADS) {
      const int q = item / BT_ROWS, row = item % BT_ROWS;
      const int64_t bl = g * R + q;
      int32_t c = 0;
      if (bl < nb && t0 + row < row1) c = cnt[bl * n + t0 + row];
      cs[item] = (double)c;
    }
    __syncthreads();
    const int kend = (int)std::min<int64_t>(BT_ROWS, (row1 - t0 + 3) / 4 * 4);
    for (int k0 = 0; k0 < kend; k0 += 4) {
      const int kk = k0 + kq;
      double y[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) y[i] = Ys[kk * S + 16 * i + r];
#pragma unroll
      for (int q = 0; q < RW; ++q) {
        const double c = cs[(w * RW + q) * BT_ROWS + kk];
        double a[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          a[i] = c * y[i];
          tac[q][i] += a[i];
        }
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int j = i; j < NB; ++j)
            acc[q][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], y[j], acc[q][i][j], 0, 0, 0);
      }
    }
  }

  constexpr int64_t PS = DS * DS + DS;
#pragma unroll
  for (int q = 0; q < RW; ++q) {
    const int64_t bl = g * R + w * RW + q;  // (the same in every lane of the wave)
    double ts[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {  // the four k quarters of column 16 i + r, in a fixed order
      double v = tac[q][i];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      ts[i] = v;
    }
    if (bl >= nb) continue;
    double* P = part + (bl * nranges + range) * PS;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
#pragma unroll
      for (int j = i; j < NB; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) P[(16 * i + acc_row(lane, t)) * DS + 16 * j + r] = acc[q][i][j][t];
      if (kq == 0) P[DS * DS + 16 * i + r] = ts[i];
    }
  }
}

// cov[bl] (D x D slab, zero padding) = (S - t t^T / n) / n from replicate bl's partials, summed in
// ascending range order; entry (i, j) from the partial's (min, max), so the slab is symmetric.
// *flag |= 1 on a non-finite value.  grid (replicates)
template <int DS>
__global__ void boot_finish_kernel(const double* __restrict__ part, int nranges, int64_t d, int64_t D, double n,
                                   double* __restrict__ cov, int* __restrict__ flag) {
  constexpr int64_t PS = DS * DS + DS;
  __shared__ double ts[DS];
  const int64_t bl = blockIdx.x;
  const double* P = part + bl * nranges * PS;
  if (threadIdx.x < DS) {
    double s = 0.0;
    for (int rg = 0; rg < nranges; ++rg) s += P[rg * PS + DS * DS + threadIdx.x];
    ts[threadIdx.x] = s;
  }
  __syncthreads();
  int bad = 0;
  for (int64_t e = threadIdx.x; e < D * D; e += NTHREADS) {
    const int64_t i = e / D, j = e % D;
    double v = 0.0;
    if (i < d && j < d) {
      const int64_t lo = std::min(i, j), hi = std::max(i, j);
      double s = 0.0;
      for (int rg = 0; rg < nranges; ++rg) s += P[rg * PS + lo * DS + hi];
      v = (s - ts[lo] * ts[hi] / n) / n;
      bad |= std::isfinite(v) ? 0 : 1;
    }
    cov[bl * D * D + e] = v;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

template <int DS>
void boot_gram(const double* Y, const int32_t* cnt, double* part, int64_t n, int64_t nb, const BootPlan& pl,
               hipStream_t stream) {
  constexpr int R = 4 * boot_rw(DS);
  hipLaunchKernelGGL(boot_gram_kernel<DS>, dim3((unsigned)((nb + R - 1) / R), (unsigned)pl.nranges), dim3(NTHREADS), 0,
                     stream, Y, cnt, n, nb, pl.range_rows, pl.nranges, part);
  HIP_TRY(hipGetLastError());
}
template <int DS>
void boot_finish(const double* part, int64_t nb, const BootPlan& pl, int64_t d, int64_t D, double n, double* cov,
                 int* flag, hipStream_t stream) {
  hipLaunchKernelGGL(boot_finish_kernel<DS>, dim3((unsigned)nb), dim3(NTHREADS), 0, stream, part, pl.nranges, d, D, n,
                     cov, flag);
  HIP_TRY(hipGetLastError());
}

void boot_cov(midagma_batch* h, const void* X, int64_t n, int64_t ldx, bool on_device, uint64_t seed, int64_t first,
              int64_t budget) {
  const int64_t d = h->d, D = h->D, B = h->B;
  const int DS = d <= 16 ? 16 : (d <= 32 ? 32 : 64);  // small_block(d)
  hipStream_t st = h->stream;
  Event ev[5];
  for (Event& e : ev) e.create();
  for (double& ms : h->boot_ms) ms = 0.0;

  // Y = X - mean (n x DS, zero padding); the caller's X is only read.  The same launches for a host
  // and a device X, so the two give the same bits
  DevBuf<> Y, colpart, colsum;
  DevBuf<int32_t> fl;
  Y.alloc((size_t)n * DS);
  colpart.alloc((size_t)colsum_parts(n) * d);
  colsum.alloc(d);
  fl.alloc(1);
  int* flag = reinterpret_cast<int*>(fl.p);
  HIP_TRY(hipEventRecord(ev[0], st));
  HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), st));
  if (d < DS) HIP_TRY(hipMemsetAsync(Y.p, 0, (size_t)n * DS * sizeof(double), st));
  HIP_TRY(hipMemcpy2DAsync(Y.p, DS * sizeof(double), X, ldx * sizeof(double), d * sizeof(double), n,
                           on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  launch_nonfinite_or(Y.p, n, d, DS, flag, st);
  launch_colsum(Y.p, n, d, DS, colpart.p, colsum.p, st);
  launch_center(Y.p, n, d, DS, colsum.p, (double)n, st);
  HIP_TRY(hipEventRecord(ev[1], st));
  int bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (bad) throw std::invalid_argument(std::string("boot_cov: ") + kNonFinite);  // (cov is untouched)
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
  h->boot_ms[0] = ms;

  // replicates per chunk: the counts and the partials of a chunk within the budget
  const BootPlan pl = boot_plan(n);
  const int64_t PS = (int64_t)DS * DS + DS, R = 4 * boot_rw(DS);
  const int64_t per = n * (int64_t)sizeof(int32_t) + pl.nranges * PS * (int64_t)sizeof(double);
  int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(B, (budget > 0 ? budget : BT_DEFAULT_BUDGET) / per));
  if (chunk >= R) chunk = chunk / R * R;
  DevBuf<int32_t> cnt;
  DevBuf<> part;
  cnt.alloc((size_t)chunk * n);
  part.alloc((size_t)chunk * pl.nranges * PS);

  h->has_cov = false;
  for (int64_t c0 = 0; c0 < B; c0 += chunk) {
    const int64_t nb = std::min(chunk, B - c0);
    double* cov = h->cov.p + c0 * D * D;
    HIP_TRY(hipEventRecord(ev[1], st));
    HIP_TRY(hipMemsetAsync(cnt.p, 0, (size_t)nb * n * sizeof(int32_t), st));
    hipLaunchKernelGGL(boot_counts_kernel, dim3((unsigned)((n + NTHREADS - 1) / NTHREADS), (unsigned)nb),
                       dim3(NTHREADS), 0, st, cnt.p, n, (uint32_t)(first + c0), (uint32_t)(seed & 0xffffffffu),
                       (uint32_t)(seed >> 32));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[2], st));
    if (DS == 16) boot_gram<16>(Y.p, cnt.p, part.p, n, nb, pl, st);
    else if (DS == 32) boot_gram<32>(Y.p, cnt.p, part.p, n, nb, pl, st);
    else boot_gram<64>(Y.p, cnt.p, part.p, n, nb, pl, st);
    HIP_TRY(hipEventRecord(ev[3], st));
    if (DS == 16) boot_finish<16>(part.p, nb, pl, d, D, (double)n, cov, flag, st);
    else if (DS == 32) boot_finish<32>(part.p, nb, pl, d, D, (double)n, cov, flag, st);
    else boot_finish<64>(part.p, nb, pl, d, D, (double)n, cov, flag, st);
    HIP_TRY(hipEventRecord(ev[4], st));
    if (c0 + chunk >= B) HIP_TRY(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the next chunk reuses cnt and part, and the events)
    for (int k = 1; k < 4; ++k) {
      HIP_TRY(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
      h->boot_ms[k] += ms;
    }
  }
  if (bad) throw std::invalid_argument(std::string("boot_cov: ") + kNonFinite);
  h->has_cov = true;
}

}  // namespace

extern "C" int midagma_boot_cov(midagma_batch* h, const void* X, int64_t n, int64_t ldx, int on_device,
                                uint64_t seed, int64_t first, int64_t budget_bytes) {
  if (!h || !X) return abi_fail(h, MIDAGMA_E_ARG, "boot_cov: null argument");
  if (n < 1 || n >= (int64_t(1) << 31)) return abi_fail(h, MIDAGMA_E_ARG, "boot_cov: need 1 <= n < 2^31");
  if (ldx < h->d) return abi_fail(h, MIDAGMA_E_ARG, "boot_cov: ldx < d");
  if (first < 0 || first > (int64_t(1) << 32) - h->B)
    return abi_fail(h, MIDAGMA_E_ARG, "boot_cov: need 0 <= first and first + B <= 2^32");
  return abi_guarded(h, [&] { boot_cov(h, X, n, ldx, on_device != 0, seed, first, budget_bytes); });
}

extern "C" int midagma_boot_get_cov(midagma_batch* h, double* out) {
  if (!h || !out) return abi_fail(h, MIDAGMA_E_ARG, "boot_get_cov: null argument");
  if (!h->has_cov) return abi_fail(h, MIDAGMA_E_ARG, "boot_get_cov: no cov (set_cov or boot_cov first)");
  return abi_guarded(h, [&] { h->download_all(h->cov, out); });
}

extern "C" int midagma_boot_profile(const midagma_batch* h, double* ms_out) {
  if (!h || !ms_out) return abi_fail(no_handle<midagma_batch>, MIDAGMA_E_ARG, "boot_profile: null argument");
  for (int k = 0; k < 4; ++k) ms_out[k] = h->boot_ms[k];
  return MIDAGMA_OK;
}

// Test hook (not in the public header): the batch's cov slabs as they lie on the device, B x D x D
// with D = 64, padding included.
extern "C" int midagma_debug_batch_cov_slabs(midagma_batch* h, double* out) {
  if (!h || !out) return abi_fail(h, MIDAGMA_E_ARG, "debug_batch_cov_slabs: null argument");
  return abi_guarded(h, [&] {
    HIP_TRY(hipMemcpyAsync(out, h->cov.p, (size_t)h->B * h->D * h->D * sizeof(double), hipMemcpyDeviceToHost,
                           h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  });
}
