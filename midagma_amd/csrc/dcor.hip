// Distance-covariance permutation tests of pairs of columns without an n x n sum
// (include/midagma_hip.h, midagma_dcor_*): the statistic of csrc/indep.hip's dCor test (the
// reference's notreks/mi_tests.py dcor_stat under permutation_pvalue) and its bias-corrected form,
// exact in O(n m) work and O(n + (n / m)^2) storage an evaluation for a block edge m near sqrt(n),
// at any n < 2^31.  Everything is FP64.
//
// For columns x, y, a_ab = |x_a - x_b|, b_ab = |y_a - y_b|, row sums a_a. and b_a., grand sums a..
// and b.., T = sum_a a_a. b_a. and S = sum_ab a_ab b_ab:
//   dcov^2   = S / n^2 - 2 T / n^3 + a.. b.. / n^4                                (the reference's)
//   dcov^2_U = S / (n (n-3)) - 2 T / (n (n-2) (n-3)) + a.. b.. / (n (n-1) (n-2) (n-3))  (U-centring)
// Row sums: with the column sorted ascending, a_i. = xs_i (2 i - n) + tot - 2 pre_i.
// S: centre both columns; blk(r) = pos_x(r) / m and bin(r) = pos_y(r) / m for the positions in the
// stable argsorts; the ordered pairs (r, r') split into (a) same blk, (b) other blk and same bin,
// both summed term by term, and (c) other blk and other bin, where the sign of
// (x_r - x_r')(y_r - y_r') is sign(blk - blk') sign(bin - bin'), so the term expands over the
// K x K cell sums (K = ceil(n / m)) of 1, x, y, xy and their inclusive 2-D prefix tables.  Ties need
// no special case: a tie that straddles two blocks has a zero difference.
//
// A permutation pi of y's rows changes only the pairing: row r carries y[pi_r], b_{pi_r}. and
// bin = pos_y(pi_r) / m.  The per-column work (argsort, positions, centred values, row sums, a..,
// dvar^2) is done once per column when the data is set.
//
// Launches of one chunk of evaluations (an evaluation = one (pair, permutation), p = 0 the identity):
//   permutations   device: Philox keys, the segmented radix sort of corr.hip (colsort.h), pi and
//                  pi^-1 from the sorted payloads; host: the upload and a scatter for pi^-1
//   block pass     grid (x-block, evaluation): term (a), the block's share of T, the block's row of
//                  the four cell-sum tables (elements ranked by (bin, position) in LDS, one
//                  fixed-order sum per run of equal bins)
//   prefix         the inclusive 2-D prefix of the tables, down the blocks, then along the bins
//   bin pass       grid (y-bin, evaluation): term (b) and every element's term (c)
//   value          dcov^2 or dcov^2_U of every evaluation from its 4 K partials
// The reference's statistic and ge are formed on the host from the values, pair by pair.
// No floating-point atomics: every sum has one order that depends on n and m alone, so results are
// the same run to run and do not depend on how the evaluations are split into chunks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../include/midagma_hip.h"
#include "coltest.h"

namespace midagma {
namespace {

constexpr int DT = 256;      // threads of the pre-pass kernels
constexpr int MAXB = 1024;   // the largest block edge
constexpr int PCH = 4 * DT;  // sorted elements per pre-pass chunk, 4 consecutive ones a thread
constexpr int PT = 64;       // tile edge of the prefix along the bins

// --- the per-column pre-pass --------------------------------------------------------------------
// part[v nch + chunk] = the sum of the chunk's sorted values of column v; CENTRED: of the values
// minus mean[v], which are also written to xc[v][row].  grid (nch, d)
template <bool CENTRED>
__global__ __launch_bounds__(DT) void dcor_chunksum_kernel(const double* __restrict__ X, int64_t ld,
                                                           const int32_t* __restrict__ order, int64_t n, int64_t nch,
                                                           const double* __restrict__ mean, double* __restrict__ xc,
                                                           double* __restrict__ part) {
  __shared__ double w[4];
  const int64_t v = blockIdx.y, i0 = (int64_t)blockIdx.x * PCH + threadIdx.x * 4;
  const double mu = CENTRED ? mean[v] : 0.0;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = i0 + k;
    if (i < n) {
      const int64_t row = order[v * n + i];
      const double val = X[row * ld + v] - mu;
      if constexpr (CENTRED) xc[v * n + row] = val;
      s += val;
    }
  }
  s = wg_sum(s, w);
  if (threadIdx.x == 0) part[v * nch + blockIdx.x] = s;
}

// mean[v] = (the chunk sums ascending) / n; one thread a column
__global__ __launch_bounds__(DT) void dcor_mean_kernel(const double* __restrict__ part, int64_t nch, int64_t d,
                                                       double nrows, double* __restrict__ mean) {
  const int64_t v = (int64_t)blockIdx.x * DT + threadIdx.x;
  if (v >= d) return;
  double s = 0.0;
  for (int64_t c = 0; c < nch; ++c) s += part[v * nch + c];
  mean[v] = s / nrows;
}

// the centred chunk sums of column v -> their exclusive prefix sums in place, tot[v] = the total
__global__ __launch_bounds__(DT) void dcor_scan_kernel(double* __restrict__ part, int64_t nch, int64_t d,
                                                       double* __restrict__ tot) {
  const int64_t v = (int64_t)blockIdx.x * DT + threadIdx.x;
  if (v >= d) return;
  double run = 0.0;
  for (int64_t c = 0; c < nch; ++c) {
    const double t = part[v * nch + c];
    part[v * nch + c] = run;
    run += t;
  }
  tot[v] = run;
}

// rs[v][row] = a_i. = xs_i (2 i - n) + tot - 2 pre_i and pos[v][row] = i for the chunk's sorted
// positions i (pre_i: the chunk's prefix, the wave sums before this wave, the lanes before this
// lane, the thread's values before this one); part3[(v nch + chunk) 3 + ..] = the chunk's sums of
// a_i., a_i.^2 and xs_i^2.  grid (nch, d)
__global__ __launch_bounds__(DT) void dcor_rowsum_kernel(const double* __restrict__ xc,
                                                         const int32_t* __restrict__ order, int64_t n, int64_t nch,
                                                         const double* __restrict__ cpre, const double* __restrict__ tot,
                                                         double* __restrict__ rs, int32_t* __restrict__ pos,
                                                         double* __restrict__ part3) {
  __shared__ double w[4], wt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t v = blockIdx.y, i0 = (int64_t)blockIdx.x * PCH + threadIdx.x * 4;
  double xs[4], loc[4];
  int64_t row[4];
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = i0 + k;
    row[k] = i < n ? order[v * n + i] : -1;
    xs[k] = i < n ? xc[v * n + row[k]] : 0.0;
    loc[k] = run;
    run += xs[k];
  }
  double inc = run;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  const double up = __shfl_up(inc, 1);
  const double excl = lane ? up : 0.0;
  if (lane == 63) wt[wave] = inc;
  __syncthreads();
  double wbase = 0.0;
  for (int k = 0; k < wave; ++k) wbase += wt[k];
  const double base = cpre[v * nch + blockIdx.x] + (wbase + excl);
  const double tv = tot[v], nn = (double)n;
  double s1 = 0.0, s2 = 0.0, sq = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = i0 + k;
    if (i < n) {
      const double pre = base + loc[k];
      const double r = (xs[k] * (2.0 * (double)i - nn) + tv) - 2.0 * pre;
      rs[v * n + row[k]] = r;
      pos[v * n + row[k]] = (int32_t)i;
      s1 += r;
      s2 += r * r;
      sq += xs[k] * xs[k];
    }
  }
  s1 = wg_sum(s1, w);
  s2 = wg_sum(s2, w);
  sq = wg_sum(sq, w);
  if (threadIdx.x == 0) {
    double* o = part3 + (v * nch + blockIdx.x) * 3;
    o[0] = s1, o[1] = s2, o[2] = sq;
  }
}

// cs[v 4 + ..] = a.., dvar^2 (biased), dvar^2 (U; 0 for n < 4), 0; zr[v] = 1 for a zero-range column
// (max == min on the raw values: the two ends of the sorted column); one thread a column
__global__ __launch_bounds__(DT) void dcor_colstat_kernel(const double* __restrict__ part3, const double* __restrict__ tot,
                                                          const double* __restrict__ X, int64_t ld,
                                                          const int32_t* __restrict__ order, int64_t n, int64_t nch,
                                                          int64_t d, double* __restrict__ cs, int32_t* __restrict__ zr) {
  const int64_t v = (int64_t)blockIdx.x * DT + threadIdx.x;
  if (v >= d) return;
  double s1 = 0.0, s2 = 0.0, sq = 0.0;
  for (int64_t c = 0; c < nch; ++c) {
    const double* o = part3 + (v * nch + c) * 3;
    s1 += o[0], s2 += o[1], sq += o[2];
  }
  const double nn = (double)n, t = tot[v];
  const double sxx = 2.0 * nn * sq - 2.0 * t * t;  // sum_ab (x_a - x_b)^2
  cs[v * 4 + 0] = s1;
  cs[v * 4 + 1] = (sxx / (nn * nn) - 2.0 * s2 / (nn * nn * nn)) + (s1 * s1) / (nn * nn * nn * nn);
  cs[v * 4 + 2] = n < 4 ? 0.0
                        : (sxx / (nn * (nn - 3.0)) - 2.0 * s2 / (nn * (nn - 2.0) * (nn - 3.0))) +
                              (s1 * s1) / (nn * (nn - 1.0) * (nn - 2.0) * (nn - 3.0));
  cs[v * 4 + 3] = 0.0;
  zr[v] = X[(int64_t)order[v * n] * ld + v] == X[(int64_t)order[v * n + n - 1] * ld + v] ? 1 : 0;
}

// --- permutations (coltest.h makes the device's) --------------------------------------------------
// inv[seg n + perm[seg n + a]] = a (the host checked that every row is a permutation of [0, n))
__global__ __launch_bounds__(DT) void dcor_invert_kernel(const int32_t* __restrict__ perm, int64_t n,
                                                         int32_t* __restrict__ inv) {
  const int64_t a = (int64_t)blockIdx.x * DT + threadIdx.x, base = (int64_t)blockIdx.y * n;
  if (a >= n) return;
  const int64_t r = perm[base + a];
  if (r >= 0 && r < n) inv[base + r] = (int32_t)a;
}

// --- the passes of an evaluation ----------------------------------------------------------------
// Scratch of local evaluation el: tab + el 4 K K, table w in {1, x, y, xy} at w K K, cell (blk, bin)
// at blk K + bin; part + el 4 K: [0] term (a) by block, [1] T by block, [2] term (b) by bin, [3]
// term (c) by bin.  Evaluation e = e0 + el is (pair q, p) = (e / (P + 1), e % (P + 1)); its
// permutation (p >= 1) is row q P + p - 1 - f0 of perm / inv.
//
// The block pass; grid (K, evaluations), blockDim a multiple of 64 with NE blockDim >= m.  Thread
// tid holds the block's elements t = tid + k blockDim.
template <int NE>
__global__ __launch_bounds__(DT) void dcor_block_kernel(const double* __restrict__ xc, const double* __restrict__ rs,
                                                        const int32_t* __restrict__ pos,
                                                        const int32_t* __restrict__ order,
                                                        const int64_t* __restrict__ pairs,
                                                        const int32_t* __restrict__ perm, int64_t e0, int64_t f0,
                                                        int64_t n, int m, int64_t K, int64_t P,
                                                        double* __restrict__ tab, double* __restrict__ part) {
  __shared__ double sx[MAXB], sy[MAXB];
  __shared__ int sbin[MAXB];
  __shared__ unsigned short sidx[MAXB];
  __shared__ double w[4];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int64_t B = blockIdx.x, el = blockIdx.y, e = e0 + el;
  const int64_t q = e / (P + 1), p = e % (P + 1);
  const int64_t vi = pairs[2 * q], vj = pairs[2 * q + 1];
  const int32_t* pi = p ? perm + (q * P + p - 1 - f0) * n : nullptr;
  const int64_t i0 = B * m;
  const int cnt = (int)std::min<int64_t>(m, n - i0);
  double xt[NE], yt[NE], acc[NE];
  uint64_t key[NE];
  int rank[NE];
  double tsum = 0.0;
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const int t = tid + k * nthr;
    xt[k] = yt[k] = acc[k] = 0.0;
    key[k] = 0;
    rank[k] = 0;
    if (t < cnt) {
      const int64_t r = order[vi * n + i0 + t];
      const int64_t s = pi ? pi[r] : r;
      const int bin = pos[vj * n + s] / m;
      xt[k] = xc[vi * n + r];
      yt[k] = xc[vj * n + s];
      key[k] = ((uint64_t)bin << 10) | (uint64_t)t;
      tsum += rs[vi * n + r] * rs[vj * n + s];
      sx[t] = xt[k];
      sy[t] = yt[k];
      sbin[t] = bin;
    }
  }
  __syncthreads();
  for (int s = 0; s < cnt; ++s) {
    const double xs = sx[s], ys = sy[s];
    const uint64_t ks = ((uint64_t)sbin[s] << 10) | (uint64_t)s;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
      acc[k] += fabs(xs - xt[k]) * fabs(ys - yt[k]);
      rank[k] += ks < key[k] ? 1 : 0;
    }
  }
  double a = 0.0;
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const int t = tid + k * nthr;
    if (t < cnt) {
      a += acc[k];
      sidx[rank[k]] = (unsigned short)t;  // (the keys are distinct: rank is a bijection onto [0, cnt))
    }
  }
  __syncthreads();
  double* T = tab + el * 4 * K * K + B * K;
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const int j = tid + k * nthr;
    if (j < cnt) {
      const int b = sbin[sidx[j]];
      if (j == 0 || sbin[sidx[j - 1]] != b) {  // the head of bin b's run sums it in position order
        double c1 = 0.0, cx = 0.0, cy = 0.0, cxy = 0.0;
        for (int jj = j; jj < cnt; ++jj) {
          const int u = sidx[jj];
          if (sbin[u] != b) break;
          const double ux = sx[u], uy = sy[u];
          c1 += 1.0;
          cx += ux;
          cy += uy;
          cxy += ux * uy;
        }
        T[b] = c1;
        T[K * K + b] = cx;
        T[2 * K * K + b] = cy;
        T[3 * K * K + b] = cxy;
      }
    }
  }
  a = wg_sum(a, w);
  tsum = wg_sum(tsum, w);
  if (tid == 0) {
    part[(el * 4 + 0) * K + B] = a;
    part[(el * 4 + 1) * K + B] = tsum;
  }
}

// the tables' running sums down the blocks; grid (ceil(K / DT), 4 evaluations): thread c
__global__ __launch_bounds__(DT) void dcor_prefix_blk_kernel(double* __restrict__ tab, int64_t K) {
  const int64_t c = (int64_t)blockIdx.x * DT + threadIdx.x;
  if (c >= K) return;
  double* T = tab + (int64_t)blockIdx.y * K * K + c;
  double run = 0.0;
  for (int64_t b = 0; b < K; ++b) {
    run += T[b * K];
    T[b * K] = run;
  }
}

// ... then along the bins; grid (ceil(K / PT), 4 evaluations), PT threads: a workgroup takes PT rows
// through PT x PT tiles in LDS, thread r the serial sum of row r with its carry
__global__ __launch_bounds__(PT) void dcor_prefix_bin_kernel(double* __restrict__ tab, int64_t K) {
  __shared__ double tile[PT][PT + 1];
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * PT;
  double* T = tab + (int64_t)blockIdx.y * K * K;
  double carry = 0.0;
  for (int64_t c0 = 0; c0 < K; c0 += PT) {
    for (int rr = 0; rr < PT; ++rr) {
      const int64_t r = r0 + rr, c = c0 + lane;
      tile[rr][lane] = (r < K && c < K) ? T[r * K + c] : 0.0;
    }
    __syncthreads();
    for (int cc = 0; cc < PT; ++cc) {
      carry += tile[lane][cc];
      tile[lane][cc] = carry;
    }
    __syncthreads();
    for (int rr = 0; rr < PT; ++rr) {
      const int64_t r = r0 + rr, c = c0 + lane;
      if (r < K && c < K) T[r * K + c] = tile[rr][lane];
    }
    __syncthreads();
  }
}

// the inclusive prefix table's value at (b, c); 0 for b or c = -1
__device__ __forceinline__ double pfx(const double* __restrict__ T, int64_t K, int64_t b, int64_t c) {
  return (b < 0 || c < 0) ? 0.0 : T[b * K + c];
}

// The bin pass; grid (K, evaluations), blockDim as the block pass.
template <int NE>
__global__ __launch_bounds__(DT) void dcor_bin_kernel(const double* __restrict__ xc, const int32_t* __restrict__ pos,
                                                      const int32_t* __restrict__ order,
                                                      const int64_t* __restrict__ pairs,
                                                      const int32_t* __restrict__ inv, int64_t e0, int64_t f0,
                                                      int64_t n, int m, int64_t K, int64_t P,
                                                      const double* __restrict__ tab, double* __restrict__ part) {
  __shared__ double sx[MAXB], sy[MAXB];
  __shared__ int sblk[MAXB];
  __shared__ double w[4];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int64_t c = blockIdx.x, el = blockIdx.y, e = e0 + el;
  const int64_t q = e / (P + 1), p = e % (P + 1);
  const int64_t vi = pairs[2 * q], vj = pairs[2 * q + 1];
  const int32_t* pinv = p ? inv + (q * P + p - 1 - f0) * n : nullptr;
  const int64_t i0 = c * m;
  const int cnt = (int)std::min<int64_t>(m, n - i0);
  double xt[NE], yt[NE], acc[NE];
  int bt[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const int t = tid + k * nthr;
    xt[k] = yt[k] = acc[k] = 0.0;
    bt[k] = 0;
    if (t < cnt) {
      const int64_t s = order[vj * n + i0 + t];
      const int64_t r = pinv ? pinv[s] : s;
      xt[k] = xc[vi * n + r];
      yt[k] = xc[vj * n + s];
      bt[k] = pos[vi * n + r] / m;
      sx[t] = xt[k];
      sy[t] = yt[k];
      sblk[t] = bt[k];
    }
  }
  __syncthreads();
  for (int s = 0; s < cnt; ++s) {
    const double xs = sx[s], ys = sy[s];
    const int bs = sblk[s];
#pragma unroll
    for (int k = 0; k < NE; ++k) {
      const double term = fabs(xs - xt[k]) * fabs(ys - yt[k]);
      acc[k] += bs != bt[k] ? term : 0.0;
    }
  }
  const double* T = tab + el * 4 * K * K;
  double bsum = 0.0, csum = 0.0;
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const int t = tid + k * nthr;
    if (t < cnt) {
      bsum += acc[k];
      const int64_t b = bt[k];
      double g[4];
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        const double* Tw = T + ww * K * K;
        const double ll = pfx(Tw, K, b - 1, c - 1);
        const double lg = pfx(Tw, K, b - 1, K - 1) - pfx(Tw, K, b - 1, c);
        const double gl = pfx(Tw, K, K - 1, c - 1) - pfx(Tw, K, b, c - 1);
        const double gg = ((pfx(Tw, K, K - 1, K - 1) - pfx(Tw, K, b, K - 1)) - pfx(Tw, K, K - 1, c)) + pfx(Tw, K, b, c);
        g[ww] = ((ll + gg) - lg) - gl;
      }
      csum += (((xt[k] * yt[k]) * g[0] - xt[k] * g[2]) - yt[k] * g[1]) + g[3];
    }
  }
  bsum = wg_sum(bsum, w);
  csum = wg_sum(csum, w);
  if (tid == 0) {
    part[(el * 4 + 2) * K + c] = bsum;
    part[(el * 4 + 3) * K + c] = csum;
  }
}

// vals[el] = dcov^2 (or dcov^2_U) of evaluation e0 + el: wave w sums partial w over the K blocks or
// bins (lane-strided, then the butterfly); S = ((a) + (b)) + (c), (a) and (b) over ordered pairs.
// grid (evaluations), 256 threads
__global__ __launch_bounds__(DT) void dcor_value_kernel(const double* __restrict__ part,
                                                        const int64_t* __restrict__ pairs,
                                                        const double* __restrict__ cs, int64_t e0, int64_t n,
                                                        int64_t K, int64_t P, int unbiased, double* __restrict__ vals) {
  __shared__ double ws[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t el = blockIdx.x, q = (e0 + el) / (P + 1);
  const double* src = part + (el * 4 + wave) * K;
  double s = 0.0;
  for (int64_t t = lane; t < K; t += 64) s += src[t];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) ws[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double S = (ws[0] + ws[2]) + ws[3], T = ws[1];
    const double gg = cs[pairs[2 * q] * 4] * cs[pairs[2 * q + 1] * 4];
    const double nn = (double)n;
    vals[el] = unbiased ? (S / (nn * (nn - 3.0)) - 2.0 * T / (nn * (nn - 2.0) * (nn - 3.0))) +
                              gg / (nn * (nn - 1.0) * (nn - 2.0) * (nn - 3.0))
                        : (S / (nn * nn) - 2.0 * T / (nn * nn * nn)) + gg / (nn * nn * nn * nn);
  }
}

constexpr int64_t kMaxChunk = 16383;  // (4 tables an evaluation in a grid dimension of 65535)

}  // namespace
}  // namespace midagma

using namespace midagma;

struct midagma_dcor : ColHandle {
  DevBuf<double> xc, rs, cs;       // d x n centred values and row sums (by row), 4 scalars a column
  DevBuf<int32_t> order, pos, zr;  // d x n argsort and positions, the zero-range marks
  std::vector<double> hcs;         // the host copy of cs
  // a run's scratch (kept between runs, grow-only)
  DevBuf<int64_t> dpairs;
  DevBuf<int32_t> inv;
  DevBuf<double> tab, part, vals;
  PinBuf<double> hvals;
  void prepare(const double* X, int64_t n, int64_t d, int64_t ld, int64_t budget, hipStream_t st);
};

// the per-column pre-pass from X_dev (n x d, ld) on stream st; the stream is synchronised
void midagma_dcor::prepare(const double* X, int64_t n, int64_t d, int64_t ld, int64_t budget, hipStream_t st) {
  const size_t nd = (size_t)n * d;
  const int64_t nch = (n + PCH - 1) / PCH;
  order.alloc(nd);
  colargsort_run(X, n, d, ld, order.p, budget, st);  // (throws on inf / nan)
  xc.alloc(nd), rs.alloc(nd), pos.alloc(nd);
  cs.alloc(4 * d), zr.alloc(d);
  DevBuf<double> part, part3, mean, tot;
  part.alloc((size_t)(nch * d)), part3.alloc((size_t)(3 * nch * d)), mean.alloc(d), tot.alloc(d);
  const dim3 chunks((unsigned)nch, (unsigned)d), cols((unsigned)((d + DT - 1) / DT));
  hipLaunchKernelGGL(dcor_chunksum_kernel<false>, chunks, dim3(DT), 0, st, X, ld, order.p, n, nch, nullptr, nullptr,
                     part.p);
  hipLaunchKernelGGL(dcor_mean_kernel, cols, dim3(DT), 0, st, part.p, nch, d, (double)n, mean.p);
  hipLaunchKernelGGL(dcor_chunksum_kernel<true>, chunks, dim3(DT), 0, st, X, ld, order.p, n, nch, mean.p, xc.p,
                     part.p);
  hipLaunchKernelGGL(dcor_scan_kernel, cols, dim3(DT), 0, st, part.p, nch, d, tot.p);
  hipLaunchKernelGGL(dcor_rowsum_kernel, chunks, dim3(DT), 0, st, xc.p, order.p, n, nch, part.p, tot.p, rs.p,
                     pos.p, part3.p);
  hipLaunchKernelGGL(dcor_colstat_kernel, cols, dim3(DT), 0, st, part3.p, tot.p, X, ld, order.p, n, nch, d, cs.p,
                     zr.p);
  HIP_TRY(hipGetLastError());
  hcs.resize(4 * d), hzr.resize(d);
  HIP_TRY(hipMemcpyAsync(hcs.data(), cs.p, 4 * d * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hzr.data(), zr.p, d * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // (the scratch is freed on return)
  this->n = n, this->d = d;
}

namespace {

// the block edge of n: the power of two in [64, 1024] with m^2 >= n, or 1024
int block_edge(int64_t n) {
  int64_t m = 64;
  while (m < MAXB && m * m < n) m <<= 1;
  return (int)m;
}

struct RunPlan {
  int m;
  int64_t K, evals, sort_bytes;
};
// bytes of scratch one evaluation takes: the tables, the partials, its value, and for P > 0 the
// permutation and its inverse (device permutations: plus the sort's two sides and histogram)
RunPlan run_plan(int64_t n, int64_t P, int block, bool device_perms, int64_t budget) {
  RunPlan p;
  if (budget <= 0) budget = kDefaultBudget;
  p.m = block ? block : block_edge(n);
  p.K = (n + p.m - 1) / p.m;
  p.sort_bytes = (P > 0 && device_perms) ? perm_sort_bytes(n) : 0;
  const int64_t per = 4 * p.K * p.K * 8 + 4 * p.K * 8 + 16 + (P > 0 ? 2 * n * 4 : 0) + p.sort_bytes;
  p.evals = std::max<int64_t>(1, std::min<int64_t>(kMaxChunk, budget / per));
  return p;
}

template <int NE>
void launch_passes(midagma_dcor* h, const RunPlan& pl, int threads, int64_t e0, int64_t ne, int64_t f0, int64_t P) {
  const dim3 grid((unsigned)pl.K, (unsigned)ne);
  const int64_t n = h->n, K = pl.K;
  hipLaunchKernelGGL(dcor_block_kernel<NE>, grid, dim3(threads), 0, h->comp, h->xc.p, h->rs.p, h->pos.p, h->order.p,
                     h->dpairs.p, h->perm.p, e0, f0, n, pl.m, K, P, h->tab.p, h->part.p);
  hipLaunchKernelGGL(dcor_prefix_blk_kernel, dim3((unsigned)((K + DT - 1) / DT), (unsigned)(4 * ne)), dim3(DT), 0,
                     h->comp, h->tab.p, K);
  hipLaunchKernelGGL(dcor_prefix_bin_kernel, dim3((unsigned)((K + PT - 1) / PT), (unsigned)(4 * ne)), dim3(PT), 0,
                     h->comp, h->tab.p, K);
  hipLaunchKernelGGL(dcor_bin_kernel<NE>, grid, dim3(threads), 0, h->comp, h->xc.p, h->pos.p, h->order.p, h->dpairs.p,
                     h->inv.p, e0, f0, n, pl.m, K, P, h->tab.p, h->part.p);
  HIP_TRY(hipGetLastError());
}

}  // namespace

extern "C" const char* midagma_dcor_last_error(const midagma_dcor* h) { return abi_last_error(h); }

extern "C" void midagma_dcor_destroy(midagma_dcor* h) { col_destroy(h); }

extern "C" int midagma_dcor_create(midagma_dcor** out, int device) { return col_create(out, device, "dcor_create"); }

extern "C" int midagma_dcor_set_data(midagma_dcor* h, const double* X, int64_t n, int64_t d, int64_t budget_bytes) {
  return col_set_data(h, "dcor_set_data", X, n, d, budget_bytes);
}

extern "C" int midagma_dcor_set_data_dev(midagma_dcor* h, const double* X_dev, int64_t n, int64_t d, int64_t ld,
                                         int64_t budget_bytes, void* hip_stream) {
  return col_set_data_dev(h, "dcor_set_data_dev", X_dev, n, d, ld, budget_bytes, hip_stream);
}

namespace {

const char* bad_run(const midagma_dcor* h, const int64_t* pairs, int64_t m, int64_t P, int unbiased, int block,
                    const double* stat, const int64_t* ge) {
  if (m < 0 || P < 0 || P > kMaxP) return "need m >= 0 and 0 <= P <= 65535";
  if (m > 0 && (!pairs || !stat || !ge)) return "null pointer";
  if (block != 0 && (block < 4 || block > MAXB)) return "block must be 0 or in [4, 1024]";
  if (h->n == 0) return "set the data first";
  if (unbiased && h->n < 4) return "the bias-corrected statistic needs n >= 4";
  for (int64_t k = 0; k < 2 * m; ++k)
    if (pairs[k] < 0 || pairs[k] >= h->d) return "pair index outside [0, d)";
  return nullptr;
}

}  // namespace

extern "C" int midagma_dcor_run(midagma_dcor* h, const int64_t* pairs, int64_t m, int64_t P, const int32_t* perms,
                                uint64_t seed, int unbiased, int block, int64_t budget_bytes, double* stat,
                                int64_t* ge, double* null_out) {
  if (!h) return abi_fail(no_handle<midagma_dcor>, MIDAGMA_E_ARG, "dcor_run: null handle");
  if (const char* why = bad_run(h, pairs, m, P, unbiased, block, stat, ge))
    return abi_fail(h, MIDAGMA_E_ARG, std::string("dcor_run: ") + why);
  const int64_t n = h->n;
  if (perms) {  // every index is read as an address offset on the device, and the inverse needs a bijection
    std::vector<uint8_t> seen((size_t)n);
    for (int64_t f = 0; f < m * P; ++f) {
      std::fill(seen.begin(), seen.end(), 0);
      const int32_t* row = perms + f * n;
      for (int64_t a = 0; a < n; ++a) {
        if (row[a] < 0 || row[a] >= n) return abi_fail(h, MIDAGMA_E_ARG, "dcor_run: permutation index outside [0, n)");
        if (seen[row[a]]) return abi_fail(h, MIDAGMA_E_ARG, "dcor_run: a row of perms is not a permutation");
        seen[row[a]] = 1;
      }
    }
  }
  if (m == 0) return MIDAGMA_OK;
  const bool dev_perms = perms == nullptr;
  const RunPlan pl = run_plan(n, P, block, dev_perms, budget_bytes);
  const int64_t P1 = P + 1, total = m * P1, K = pl.K;
  const int threads = std::min(DT, (pl.m + 63) / 64 * 64);
  const int ne_thr = (pl.m + threads - 1) / threads;  // 1 .. 4

  const int rc = abi_guarded(h, [&] {
    h->dpairs.alloc((size_t)(2 * m));
    HIP_TRY(hipMemcpyAsync(h->dpairs.p, pairs, 2 * m * sizeof(int64_t), hipMemcpyHostToDevice, h->comp));
    NullCount count{stat, ge, null_out, P};
    for (int64_t e0 = 0; e0 < total; e0 += pl.evals) {
      const int64_t ne = std::min(pl.evals, total - e0), e1 = e0 + ne;
      // the chunk's permutations: f = e - q - 1 for p >= 1, ascending with e
      const int64_t qa = e0 / P1, pa = e0 % P1, qb = (e1 - 1) / P1, pb = (e1 - 1) % P1;
      const int64_t f0 = qa * P + (pa ? pa - 1 : 0), f1 = qb * P + pb;  // [f0, f1)
      const int64_t nf = f1 - f0;
      h->tab.alloc((size_t)(ne * 4 * K * K)), h->part.alloc((size_t)(ne * 4 * K));
      h->vals.alloc((size_t)ne), h->hvals.alloc((size_t)ne);
      if (nf > 0) {
        h->perm.alloc((size_t)(nf * n)), h->inv.alloc((size_t)(nf * n));
        if (dev_perms) {
          h->sort.run(seed, f0, nf, P, n, h->perm.p, h->inv.p, h->comp);
        } else {
          HIP_TRY(hipMemcpyAsync(h->perm.p, perms + f0 * n, (size_t)(nf * n) * sizeof(int32_t), hipMemcpyHostToDevice,
                                 h->comp));
          hipLaunchKernelGGL(dcor_invert_kernel, dim3((unsigned)((n + DT - 1) / DT), (unsigned)nf), dim3(DT), 0,
                             h->comp, h->perm.p, n, h->inv.p);
          HIP_TRY(hipGetLastError());
        }
      }
      HIP_TRY(hipMemsetAsync(h->tab.p, 0, (size_t)(ne * 4 * K * K) * sizeof(double), h->comp));
      if (ne_thr == 1)
        launch_passes<1>(h, pl, threads, e0, ne, f0, P);
      else if (ne_thr == 2)
        launch_passes<2>(h, pl, threads, e0, ne, f0, P);
      else
        launch_passes<4>(h, pl, threads, e0, ne, f0, P);
      hipLaunchKernelGGL(dcor_value_kernel, dim3((unsigned)ne), dim3(DT), 0, h->comp, h->part.p, h->dpairs.p, h->cs.p,
                         e0, n, K, P, unbiased, h->vals.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(h->hvals.p, h->vals.p, (size_t)ne * sizeof(double), hipMemcpyDeviceToHost, h->comp));
      HIP_TRY(hipStreamSynchronize(h->comp));
      for (int64_t e = e0; e < e1; ++e) {
        const int64_t q = e / P1, p = e % P1, vi = pairs[2 * q], vj = pairs[2 * q + 1];
        const double v = h->hvals.p[e - e0];
        const bool zero = h->hzr[vi] || h->hzr[vj];
        const double vx = h->hcs[vi * 4 + (unbiased ? 2 : 1)], vy = h->hcs[vj * 4 + (unbiased ? 2 : 1)];
        double s = 0.0;
        if (!zero && vx > 0.0 && vy > 0.0)
          s = unbiased ? v / std::sqrt(vx * vy) : std::sqrt(std::max(v, 0.0)) / std::sqrt(std::sqrt(vx * vy));
        count.add(q, p, v, s, zero);  // (counted by dcov^2, reported as the correlation)
      }
    }
  });
  if (rc != MIDAGMA_OK) (void)hipStreamSynchronize(h->comp);  // leave nothing in flight that reads the scratch
  return rc;
}

extern "C" int midagma_dcor_perms(midagma_dcor* h, int64_t q, int64_t P, uint64_t seed, int32_t* perms_out,
                                  int32_t* inverse_out) {
  return col_perms(h, "dcor_perms", q, P, seed, perms_out, h ? &h->inv : nullptr, inverse_out);
}

extern "C" int midagma_dcor_block(int64_t n) { return n < 1 ? 0 : block_edge(n); }
