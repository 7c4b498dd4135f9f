// HSIC permutation tests of pairs of columns from low-rank factors of the RBF Gram matrices
// (include/midagma_hip.h, midagma_hsic_*): the statistic of csrc/indep.hip's HSIC test (the
// reference's notreks/mi_tests.py hsic_stat under permutation_pvalue) to within 4 eta (1 + eta) of
// the n^2 sum, in O(n r_x r_y) work an evaluation, at any n < 2^31.  Everything is FP64.
//
// On one column the RBF Gram matrix K has a numerically tiny rank.  A pivoted incomplete Cholesky
// factor K ~ F F^T (F is n x r) that stops when the largest residual diagonal entry is <= eta has
// elementwise error <= eta (the residual is positive semidefinite: |R_ab| <= sqrt(R_aa R_bb)).  With
// Fc, Gc the column-centred factors of x and y and pi a permutation of y's rows,
//   HSIC(x, y[pi]) = (1 / n^2) || Fc^T Gc[pi, :] ||_F^2,
// a small GEMM whose contraction runs over the rows; a permutation only gathers rows of Gc.
//
// Launches:
//   set_data       the columns' stable argsort (colsort.h), then XT (d x n) and the sorted columns
//   medians        the reference's median heuristic at any n: indep_median_kernel's counting
//                  argument with the sorted column in global memory and several workgroups a column,
//                  one launch a bisection round; a round applies the decision of the round before
//                  from its per-workgroup counts (double-buffered), so no host synchronise between
//                  rounds; 63 rounds empty the 63-bit range, round 64 counts at the result
//   factorisation  a batch of columns at once, one launch a step, grid (row chunk, column): every
//                  workgroup finds the pivot (largest residual diagonal entry, ties to the smallest
//                  row) from the chunk maxima of the step before, then computes its rows of the new
//                  column c_a = (k(x_a, x_p) - sum_t F[a,t] F[p,t]) / sqrt(d_p) and d_a = max(d_a -
//                  c_a^2, 0) (the pivot's own: 0).  The working factor is column-major (a step reads
//                  and writes whole columns); the finished one is centred and stored row-major
//                  n x r_pad, r_pad the next multiple of 16, zero padded: a gathered row is contiguous
//   permutations   coltest.h's: Philox keys and the segmented radix sort (any n), or the host's,
//                  checked on the device (every index in range, every row marked once)
//   evaluation     grid (row chunk, group of 4 permutations of a pair, 32 x 32 block of M): the A
//                  operand of v_mfma_f64_16x16x4_f64 comes from Fc's rows, loaded once for the
//                  group, the B operand from the gathered rows of Gc; the 4 waves take the chunk's
//                  rows in turn and their tiles are summed wave 0 + 1 + 2 + 3
//   value          the chunk partials of every entry of M summed in ascending chunk order, squared
//                  and summed in a fixed order, / n^2
// No floating-point atomics: every sum has one order that depends on n, the ranks and the chunk size
// alone, so results are the same bits run to run and do not depend on how pairs and permutations
// are batched or how columns are grouped for factorisation.
//
// Every pair at once (midagma_hsic_all_pairs): the chi-square test of the bias-corrected correlation
// (Shen, Panda, Vogelstein) needs one evaluation a pair and no permutation, and for every pair the
// evaluations are one symmetric GEMM.  With D = 1 - K off the diagonal (hyppo's Hsic convention) and
// A~ its U-centred matrix, from the centred factor Fc, the means m and O(n) vectors a column,
//   <A~_x, A~_y> = || Fc_x^T Fc_y ||_F^2 + 2 n v~_x.v~_y + n^2 c_x c_y - a_x.a_y,
//   rho_i = (n - 1) - (n F_i.m - |F_i|^2),  T = sum rho_i,  v = -Fc m - rho / (n - 2),
//   g = 1 - m.m + T / ((n - 1)(n - 2)),  a_i = -|Fc_i|^2 + 2 v_i + g,  v~ = v - mean(v),  c = g + 2 mean(v)
// (the cross terms vanish because Fc^T 1 = 0; the centred form cancels nothing of size n^2).
//   vectors        16 lanes a row of Fc: v and -q + 2 v into a panel (n x 2 columns a column of X,
//                  row-major, padded to 16), chunk sums of rho and Fc m; a thread a column for the
//                  scalars; a shift of the panel by mean(v) and g
//   tiled pass     Phi = [Fc_1 | ... | Fc_k] side by side; a workgroup owns a 128 x 128 tile of
//                  Phi_A^T Phi_B on or above the diagonal and a chunk of rows, stages 16-row slabs of
//                  the two operand panels in LDS (a table maps a 16-column slab of Phi to its factor)
//                  and runs v_mfma_f64_16x16x4_f64, a wave a 64 x 64 quadrant over every row of the
//                  chunk; the same kernel over the vector panels gives the two vector Grams
//   reduce         a sub-tile's entries from the chunk partials in ascending chunk order, squared and
//                  summed in a fixed order (the factors) or kept (the vectors)
//   combine        a thread a pair: its sub-tiles' squared norms in ascending order, plus the rest
// A 16 x 16 sub-tile belongs to one pair and a wave takes all rows of a chunk, so a pair's value
// depends on n, the two ranks, the chunk and nothing else: not on the budget, the column groups, the
// other columns listed or where the pair's sub-tiles fall in a tile.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../include/midagma_hip.h"
#include "coltest.h"
#include "mfma64.h"

namespace midagma {
namespace {

constexpr int HT = 256;      // threads of every kernel here
constexpr int FCH = 4 * HT;  // rows of a column per workgroup of the factor kernels
constexpr int RCAP = 256;    // the rank cap
constexpr int RFIRST = 64;   // columns of the working factor in the first attempt
constexpr int EG = 4;        // permutations that share one load of the Fc chunk
constexpr int MG = 64;       // most workgroups a column of a median round
constexpr int64_t kNoRow = INT64_MAX;

__device__ __forceinline__ bool better(double v, long long i, double ov, long long oi) {
  return ov > v || (ov == v && oi < i);
}

// the largest v of the workgroup and the smallest row that holds it; valid in every thread
__device__ __forceinline__ void wg_argmax(double& v, long long& i, double* wv, long long* wi) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const long long oi = __shfl_xor(i, off);
    if (better(v, i, ov, oi)) v = ov, i = oi;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = v, wi[threadIdx.x >> 6] = i;
  __syncthreads();
  v = wv[0], i = wi[0];
  for (int k = 1; k < 4; ++k)
    if (better(v, i, wv[k], wi[k])) v = wv[k], i = wi[k];
}

// --- the data ------------------------------------------------------------------------------------
// XT[v][a] = X[a][v] and XS[v][i] = X[order[v][i]][v]; grid (ceil(n / HT), d)
__global__ __launch_bounds__(HT) void hsic_cols_kernel(const double* __restrict__ X, int64_t ld,
                                                       const int32_t* __restrict__ order, int64_t n,
                                                       double* __restrict__ XT, double* __restrict__ XS) {
  const int64_t a = (int64_t)blockIdx.x * HT + threadIdx.x, v = blockIdx.y;
  if (a >= n) return;
  XT[v * n + a] = X[a * ld + v];
  XS[v * n + a] = X[(int64_t)order[v * n + a] * ld + v];
}

// zr[v] = 1 for a zero-range column (the two ends of the sorted column are equal)
__global__ __launch_bounds__(HT) void hsic_zero_range_kernel(const double* __restrict__ XS, int64_t n, int64_t d,
                                                             int32_t* __restrict__ zr) {
  const int64_t v = (int64_t)blockIdx.x * HT + threadIdx.x;
  if (v < d) zr[v] = XS[v * n] == XS[v * n + n - 1] ? 1 : 0;
}

// --- the median bandwidths -----------------------------------------------------------------------
struct MedState {
  unsigned long long lo, hi;
};

// the rank (from 0) of the sorted-order difference whose square is the lower median element
__device__ __forceinline__ long long median_rank(int64_t n) {
  const long long M = (long long)n * (n - 1) / 2;
  return (M & 1) ? M / 2 : M / 2 - 1;
}

// One round; grid (G, columns).  State and partials of round r live in half r & 1 of st / cnt / mn.
// A round whose range is empty counts at the result t = lo (and is repeated unchanged by the
// rounds after it): cnt = #{a < b : fl(xs_b - xs_a) <= t}, mn = the smallest difference above t.
__global__ __launch_bounds__(HT) void hsic_median_round_kernel(const double* __restrict__ XS,
                                                               const int64_t* __restrict__ cols, int64_t n,
                                                               int round, int64_t ncols, MedState* __restrict__ st,
                                                               long long* __restrict__ cnt, double* __restrict__ mn) {
  __shared__ long long ws[4];
  __shared__ double wm[4];
  const int64_t col = blockIdx.y, G = gridDim.x;
  const int cur = round & 1, prev = cur ^ 1;
  const double* xs = XS + cols[col] * n;
  unsigned long long lo = 0, hi = 0x7ff0000000000000ull;
  if (round > 0) {
    const MedState s = st[prev * ncols + col];
    lo = s.lo, hi = s.hi;
    if (lo < hi) {
      long long c = 0;
      for (int64_t g = 0; g < G; ++g) c += cnt[(prev * ncols + col) * G + g];
      const unsigned long long mid = lo + ((hi - lo) >> 1);
      if (c >= median_rank(n) + 1)
        hi = mid;
      else
        lo = mid + 1;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) st[cur * ncols + col] = MedState{lo, hi};
  const double t = __longlong_as_double((long long)(lo < hi ? lo + ((hi - lo) >> 1) : lo));
  long long c = 0;
  double m = INFINITY;
  for (int64_t a = (int64_t)blockIdx.x * HT + threadIdx.x; a < n - 1; a += G * HT) {
    const double xa = xs[a];
    int64_t l = a + 1, h = n;
    while (l < h) {
      const int64_t mid = (l + h) >> 1;
      if (xs[mid] - xa <= t)
        l = mid + 1;
      else
        h = mid;
    }
    c += l - (a + 1);
    if (l < n) m = fmin(m, xs[l] - xa);
  }
  c = wg_sum_ll<HT / 64>(c, ws);
  m = wg_min<HT / 64>(m, wm);
  if (threadIdx.x == 0) {
    cnt[(cur * ncols + col) * G + blockIdx.x] = c;
    mn[(cur * ncols + col) * G + blockIdx.x] = m;
  }
}

// med[col] from the last round (`half` of the buffers), numpy's rule for an even count; one thread a column
__global__ __launch_bounds__(HT) void hsic_median_finish_kernel(int64_t n, int half, int64_t ncols, int64_t G,
                                                                const MedState* __restrict__ st,
                                                                const long long* __restrict__ cnt,
                                                                const double* __restrict__ mn, double* __restrict__ med) {
  const int64_t col = (int64_t)blockIdx.x * HT + threadIdx.x;
  if (col >= ncols) return;
  const long long M = (long long)n * (n - 1) / 2;
  const double vk = __longlong_as_double((long long)st[half * ncols + col].lo);
  double m = vk * vk;
  if (!(M & 1)) {
    long long c = 0;
    double above = INFINITY;
    for (int64_t g = 0; g < G; ++g) {
      c += cnt[(half * ncols + col) * G + g];
      above = fmin(above, mn[(half * ncols + col) * G + g]);
    }
    const double vn = c > M / 2 ? vk : above;
    m = (m + vn * vn) / 2.0;
  }
  med[col] = m > 0.0 ? m : 1.0;
}

// --- the factorisation ---------------------------------------------------------------------------
// One step of every column of the batch; grid (nch, nb).  W: nb working factors, column-major
// cap x n each; dres: nb x n residual diagonals; pmax / parg: the chunk maxima and their rows, half
// step & 1 written, the other read; rank[col] < 0 while the column runs.
__global__ __launch_bounds__(HT) void hsic_factor_step_kernel(const double* __restrict__ XT,
                                                              const int64_t* __restrict__ cols,
                                                              const double* __restrict__ cvec, int64_t n,
                                                              int64_t nch, int step, int cap, double eta,
                                                              double* __restrict__ W, double* __restrict__ dres,
                                                              double* __restrict__ pmax, long long* __restrict__ parg,
                                                              int32_t* __restrict__ rank, double* __restrict__ resid) {
  __shared__ double wv[4];
  __shared__ long long wi[4];
  const int tid = threadIdx.x;
  const int64_t col = blockIdx.y, ch = blockIdx.x, nb = gridDim.y, v = cols[col];
  const int64_t cur = ((step & 1) * nb + col) * nch, prev = (((step & 1) ^ 1) * nb + col) * nch;
  double mx = 1.0;  // step 0: the diagonal of K is 1, the pivot is row 0
  long long p = 0;
  if (step > 0) {
    mx = -1.0, p = kNoRow;
    for (int64_t c = tid; c < nch; c += HT)
      if (better(mx, p, pmax[prev + c], parg[prev + c])) mx = pmax[prev + c], p = parg[prev + c];
    wg_argmax(mx, p, wv, wi);
  }
  if (mx <= eta || step >= n || step >= cap) {  // the column is finished (or out of room)
    if (tid == 0) {
      if (ch == 0 && rank[col] < 0) rank[col] = step, resid[col] = mx;
      if (step > 0) pmax[cur + ch] = pmax[prev + ch], parg[cur + ch] = parg[prev + ch];
    }
    return;
  }
  const double* x = XT + v * n;
  double* Wc = W + col * (int64_t)cap * n;
  double* dc = dres + col * n;
  const double xp = x[p], cv = cvec[v], sq = sqrt(mx);
  int64_t a[4];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 4; ++k) a[k] = ch * FCH + tid + k * HT;
  for (int t = 0; t < step; ++t) {
    const double* wt = Wc + (int64_t)t * n;
    const double wp = wt[p];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (a[k] < n) acc[k] += wt[a[k]] * wp;
  }
  double bv = -1.0;
  long long bi = kNoRow;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (a[k] < n) {
      const double dl = x[a[k]] - xp;
      const double ca = (exp(-(dl * dl) * cv) - acc[k]) / sq;
      Wc[(int64_t)step * n + a[k]] = ca;
      const double dold = step ? dc[a[k]] : 1.0;
      const double dn = a[k] == p ? 0.0 : fmax(dold - ca * ca, 0.0);
      dc[a[k]] = dn;
      if (dn > bv) bv = dn, bi = a[k];  // (ascending rows: the first of equal values stays)
    }
  wg_argmax(bv, bi, wv, wi);
  if (tid == 0) pmax[cur + ch] = bv, parg[cur + ch] = bi;
}

// part[t nch + chunk] = the sum of the chunk's rows of column t of the working factor Wc; grid (nch, r)
__global__ __launch_bounds__(HT) void hsic_colsum_kernel(const double* __restrict__ Wc, int64_t n, int64_t nch,
                                                         double* __restrict__ part) {
  __shared__ double w[4];
  const int64_t t = blockIdx.y;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t a = (int64_t)blockIdx.x * FCH + threadIdx.x + k * HT;
    if (a < n) s += Wc[t * n + a];
  }
  s = wg_sum<HT / 64>(s, w);
  if (threadIdx.x == 0) part[t * nch + blockIdx.x] = s;
}

// mean[t] = (the chunk sums ascending) / n for t < r, 0 for the padding; one thread a column of the factor
__global__ __launch_bounds__(HT) void hsic_mean_kernel(const double* __restrict__ part, int64_t nch, int r, int rp,
                                                       double nrows, double* __restrict__ mean) {
  const int t = blockIdx.x * HT + threadIdx.x;
  if (t >= rp) return;
  double s = 0.0;
  if (t < r)
    for (int64_t c = 0; c < nch; ++c) s += part[t * nch + c];
  mean[t] = s / nrows;
}

// Fc[a][t] = Wc[t][a] - mean[t] for t < r, 0 for r <= t < rp; one thread an entry of Fc
__global__ __launch_bounds__(HT) void hsic_centre_kernel(const double* __restrict__ Wc, const double* __restrict__ mean,
                                                         int64_t n, int r, int rp, double* __restrict__ Fc) {
  const int64_t e = (int64_t)blockIdx.x * HT + threadIdx.x;
  if (e >= n * rp) return;
  const int64_t a = e / rp;
  const int t = (int)(e % rp);
  Fc[e] = t < r ? Wc[(int64_t)t * n + a] - mean[t] : 0.0;
}

// --- permutations (coltest.h makes the device's) ---------------------------------------------------
// host permutations: flag[0] for an index outside [0, n), else its row is marked ...
__global__ __launch_bounds__(HT) void hsic_perm_mark_kernel(const int32_t* __restrict__ perm, int64_t n,
                                                            uint8_t* __restrict__ mark, int* __restrict__ flag) {
  const int64_t a = (int64_t)blockIdx.x * HT + threadIdx.x, base = (int64_t)blockIdx.y * n;
  if (a >= n) return;
  const int64_t r = perm[base + a];
  if (r < 0 || r >= n)
    flag[0] = 1;
  else
    mark[base + r] = 1;
}

// ... and flag[1] for a row that no index marked (n indices in range that mark n rows are a bijection)
__global__ __launch_bounds__(HT) void hsic_perm_check_kernel(const uint8_t* __restrict__ mark, int64_t n,
                                                             int* __restrict__ flag) {
  const int64_t a = (int64_t)blockIdx.x * HT + threadIdx.x;
  if (a < n && !mark[(int64_t)blockIdx.y * n + a]) flag[1] = 1;
}

// --- the evaluation ------------------------------------------------------------------------------
// Group g = q NG + k holds the evaluations (pair q, p = EG k .. EG k + EG - 1), p = 0 the identity,
// p <= P; its slot s is evaluation p = EG k + s.  The permutation of (q, p >= 1) is row
// q P + p - 1 - f0 of perm.  partial: [(slot nchunk + chunk) nbmax + block][1024], entry
// tile 256 + reg 64 + lane of the block's 2 x 2 tiles.
//
// grid (nchunk, groups, nbmax): the chunk's share of the 32 x 32 block bz = bx nby + by of
// M = Fc_i^T Gc_j[pi, :] for the group's permutations.  Wave w takes rows 16 i + 4 w + (lane >> 4).
__global__ __launch_bounds__(HT) void hsic_eval_kernel(double* const* __restrict__ fptr, const int32_t* __restrict__ rpad,
                                                       const int64_t* __restrict__ pairs,
                                                       const int32_t* __restrict__ perm, int64_t g0, int64_t f0,
                                                       int64_t n, int64_t chunk, int64_t P, int64_t NG, int nbmax,
                                                       double* __restrict__ partial) {
  __shared__ double red[4][1024];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, kq = lane >> 4;
  const int64_t c = blockIdx.x, lg = blockIdx.y, g = g0 + lg, q = g / NG, p0 = (g % NG) * EG;
  const int np = (int)std::min<int64_t>(EG, P + 1 - p0);
  const int64_t vi = pairs[2 * q], vj = pairs[2 * q + 1];
  const int rx = rpad[vi], ry = rpad[vj];
  const int nby = (ry + 31) / 32, nblk = ((rx + 31) / 32) * nby, bz = blockIdx.z;
  if (bz >= nblk) return;
  const int s0 = (bz / nby) * 32, t0 = (bz % nby) * 32;
  const bool ax1 = s0 + 16 < rx, by1 = t0 + 16 < ry;
  const double* F = fptr[vi];
  const double* Gm = fptr[vj];
  const int32_t* pg[EG];
#pragma unroll
  for (int k = 0; k < EG; ++k) pg[k] = (k < np && p0 + k > 0) ? perm + (q * P + p0 + k - 1 - f0) * n : nullptr;
  dbl4 acc[EG][2][2];
#pragma unroll
  for (int k = 0; k < EG; ++k)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[k][i][j] = dbl4{0.0, 0.0, 0.0, 0.0};
  const int64_t abase = c * chunk + 4 * w + kq;
  for (int64_t i = 0; i < chunk && c * chunk + i < n; i += 16) {
    const int64_t a = abase + i;
    const bool ok = a < n;
    const double* fr = F + a * rx + s0 + r;
    const double a0 = ok ? fr[0] : 0.0;
    const double a1 = (ok && ax1) ? fr[16] : 0.0;
#pragma unroll
    for (int k = 0; k < EG; ++k)
      if (k < np) {
        const int64_t row = ok ? (pg[k] ? (int64_t)pg[k][a] : a) : 0;
        const double* gr = Gm + row * ry + t0 + r;
        const double b0 = gr[0];
        const double b1 = by1 ? gr[16] : 0.0;
        acc[k][0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[k][0][0], 0, 0, 0);
        if (by1) acc[k][0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[k][0][1], 0, 0, 0);
        if (ax1) acc[k][1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[k][1][0], 0, 0, 0);
        if (ax1 && by1) acc[k][1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[k][1][1], 0, 0, 0);
      }
  }
  const int64_t nchunk = gridDim.x;
#pragma unroll
  for (int k = 0; k < EG; ++k)
    if (k < np) {
      __syncthreads();  // (red may still be read for the permutation before)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int t = 0; t < 4; ++t) red[w][(i * 2 + j) * 256 + t * 64 + lane] = acc[k][i][j][t];
      __syncthreads();
      double* dst = partial + (((lg * EG + k) * nchunk + c) * nbmax + bz) * 1024;
      for (int e = tid; e < 1024; e += HT) dst[e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    }
}

// vals[slot] = || M ||_F^2 / n^2: every entry of M from its chunk partials in ascending chunk order,
// squared; a thread sums its entries block by block, then the workgroup.  grid (EG groups)
__global__ __launch_bounds__(HT) void hsic_value_kernel(const double* __restrict__ partial,
                                                        const int32_t* __restrict__ rpad,
                                                        const int64_t* __restrict__ pairs, int64_t g0, int64_t n,
                                                        int64_t nchunk, int64_t P, int64_t NG, int nbmax,
                                                        double* __restrict__ vals) {
  __shared__ double w[4];
  const int64_t slot = blockIdx.x, g = g0 + slot / EG, q = g / NG, p = (g % NG) * EG + slot % EG;
  if (p > P) {
    if (threadIdx.x == 0) vals[slot] = 0.0;
    return;
  }
  const int nblk = ((rpad[pairs[2 * q]] + 31) / 32) * ((rpad[pairs[2 * q + 1]] + 31) / 32);
  double s = 0.0;
  for (int bz = 0; bz < nblk; ++bz)
    for (int e = threadIdx.x; e < 1024; e += HT) {
      double m = 0.0;
      for (int64_t c = 0; c < nchunk; ++c) m += partial[((slot * nchunk + c) * nbmax + bz) * 1024 + e];
      s += m * m;
    }
  s = wg_sum<HT / 64>(s, w);
  if (threadIdx.x == 0) vals[slot] = s / ((double)n * (double)n);
}

// --- every pair at once: the tiled cross-Gram ------------------------------------------------------
// Phi = [Fc_1 | ... | Fc_k], the centred factors of a column group side by side, is n x R.  A slab
// is 16 columns of Phi: 16 columns of one factor (r_pad is a multiple of 16), so a 16 x 16 sub-tile
// of Phi_A^T Phi_B belongs to one pair of columns.
struct Slab {
  const double* p;  // row 0 of the slab's 16 columns (nullptr: past the panel's end)
  int64_t ld;       // doubles from a row to the next (the factor's r_pad)
};

constexpr int TS = 8;                // slabs a tile edge: tiles are 128 x 128
constexpr int KS = 16;               // rows staged in LDS at a time
constexpr int LS = 16 * TS + 16;     // LDS row stride in doubles: 144 (rows kq and kq + 1 of an operand read 32 banks apart)
constexpr int TSUB = TS * TS;        // sub-tiles a tile
constexpr int TILE_E = TSUB * 256;   // doubles a tile

// The share of rows [c chunk, (c + 1) chunk) of tile (ta, tb) of Phi_A^T Phi_B; 1-d grid, block
// c ntiles + tile.  Wave w owns the 64 x 64 quadrant (w >> 1, w & 1) as 4 x 4 accumulators and
// takes every row of the chunk in ascending order, so an entry's value depends on n and the chunk
// alone, not on where its sub-tile lies in a tile.  Rows past the chunk's or n's end are staged as
// zeros.  partial: [(c ntiles + tile) 64 + sub-tile i 8 + j][reg 64 + lane]; sub-tiles past the
// panels' ends are not written.
__global__ __launch_bounds__(HT) void hsic_tile_kernel(const Slab* __restrict__ slabA, const Slab* __restrict__ slabB,
                                                       const int2* __restrict__ tiles, int ntiles, int nsA, int nsB,
                                                       int64_t n, int64_t chunk, double* __restrict__ partial) {
  __shared__ double As[KS * LS], Bs[KS * LS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, kq = lane >> 4;
  const int64_t c = blockIdx.x / ntiles;
  const int tile = (int)(blockIdx.x % ntiles);
  const int2 tt = tiles[tile];
  // staging: pass q moves rows 4 q + (tid >> 6); a thread moves 2 doubles of slab (tid & 63) >> 3
  const int ls = lane >> 3, lc = (lane & 7) * 2;
  const int sa = tt.x * TS + ls, sb = tt.y * TS + ls;
  const Slab SA = sa < nsA ? slabA[sa] : Slab{nullptr, 0};
  const Slab SB = sb < nsB ? slabB[sb] : Slab{nullptr, 0};
  const int64_t r0 = c * chunk, r1 = std::min<int64_t>(n, r0 + chunk);
  // this wave's quadrant: sub-tiles [4 wm, 4 wm + ni) x [4 wn, 4 wn + nj)
  const int wm = w >> 1, wn = w & 1;
  const int ni = std::max(0, std::min(4, nsA - (tt.x * TS + 4 * wm)));
  const int nj = std::max(0, std::min(4, nsB - (tt.y * TS + 4 * wn)));
  dbl4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = dbl4{0.0, 0.0, 0.0, 0.0};
  double2 pa[4], pb[4];
  auto fetch = [&](int64_t base) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t row = base + 4 * q + w;
      const bool ok = row < r1;
      pa[q] = (ok && SA.p) ? *reinterpret_cast<const double2*>(SA.p + row * SA.ld + lc) : double2{0.0, 0.0};
      pb[q] = (ok && SB.p) ? *reinterpret_cast<const double2*>(SB.p + row * SB.ld + lc) : double2{0.0, 0.0};
    }
  };
  fetch(r0);
  for (int64_t base = r0; base < r1; base += KS) {
    __syncthreads();  // (the rows of the step before are no longer read)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *reinterpret_cast<double2*>(&As[(4 * q + w) * LS + ls * 16 + lc]) = pa[q];
      *reinterpret_cast<double2*>(&Bs[(4 * q + w) * LS + ls * 16 + lc]) = pb[q];
    }
    __syncthreads();
    if (base + KS < r1) fetch(base + KS);  // (in flight under the MFMAs)
    if (ni > 0 && nj > 0) {
#pragma unroll
      for (int k0 = 0; k0 < KS; k0 += 4) {
        const double* ar = &As[(k0 + kq) * LS + wm * 64 + r];
        const double* br = &Bs[(k0 + kq) * LS + wn * 64 + r];
        double a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = ar[16 * i], b[i] = br[16 * i];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < ni) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < nj) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
          }
      }
    }
  }
  double* dst = partial + (int64_t)blockIdx.x * TILE_E;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < ni) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nj) {
          double* d = dst + ((4 * wm + i) * TS + 4 * wn + j) * 256 + lane;
#pragma unroll
          for (int t = 0; t < 4; ++t) d[t * 64] = acc[i][j][t];
        }
    }
}

// Every entry of a sub-tile from its chunk partials in ascending chunk order; grid (64, tiles of
// the batch).  SQ: out[sa nsB + sb] = the sum of the squared entries in a fixed order (a wave's
// butterfly, then wave 0 + 1 + 2 + 3); else out[(sa nsB + sb) 256 + e] = the entries.
template <bool SQ>
__global__ __launch_bounds__(HT) void hsic_tile_reduce_kernel(const double* __restrict__ partial,
                                                              const int2* __restrict__ tiles, int ntiles, int nsA,
                                                              int nsB, int64_t nchunk, double* __restrict__ out) {
  __shared__ double ws[4];
  const int tile = blockIdx.y, sub = blockIdx.x;
  const int2 tt = tiles[tile];
  const int sa = tt.x * TS + sub / TS, sb = tt.y * TS + sub % TS;
  if (sa >= nsA || sb >= nsB) return;
  double m = 0.0;
  for (int64_t c = 0; c < nchunk; ++c) m += partial[((c * ntiles + tile) * TSUB + sub) * 256 + threadIdx.x];
  if (SQ) {
    const double s = wg_sum<HT / 64>(m * m, ws);
    if (threadIdx.x == 0) out[(int64_t)sa * nsB + sb] = s;
  } else {
    out[((int64_t)sa * nsB + sb) * 256 + threadIdx.x] = m;
  }
}

// --- every pair at once: the O(n) vectors of the U-centred form -----------------------------------
// With K^ = F F^T, m the column means of F and Fc = F - 1 m^T:  k^_i = |F_i|^2,
// rho_i = (n - 1) - (n F_i . m - k^_i) (row i's sum of D = 1 - K^ off the diagonal), w_i = Fc_i . m,
// q_i = |Fc_i|^2, T = sum rho_i, g = 1 - m.m + T / ((n - 1)(n - 2)).

// a column of the group: its factor and where its means start in the group's list
struct UCol {
  const double* Fc;
  int32_t rp, moff;
};

// The chunk's FCH rows of one column, 16 lanes a row (a 16-lane load is one 128-byte segment of the
// row): lane s sums the entries s, s + 16, ... of its row, then the 16 lanes a butterfly, so a row's
// sums depend on r_pad alone.  panel[a][2 col] = v_a = -w_a - rho_a / (n - 2) and
// panel[a][2 col + 1] = -q_a + 2 v_a (hsic_u_shift_kernel finishes both); part[(col nch + ch) 2 +
// {0, 1}] = the chunk's sums of rho and w.  panel is n x W row-major; grid (nch, columns)
__global__ __launch_bounds__(HT) void hsic_u_rows_kernel(const UCol* __restrict__ cols, const double* __restrict__ means,
                                                         int64_t n, int64_t nch, int W, double* __restrict__ panel,
                                                         double* __restrict__ part) {
  __shared__ double ws[4];
  const int col = blockIdx.y, sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const UCol uc = cols[col];
  const double* mean = means + uc.moff;
  const double nr = (double)n;
  double sr = 0.0, sw = 0.0;
  for (int it = 0; it < FCH / 16; ++it) {
    const int64_t a = (int64_t)blockIdx.x * FCH + it * 16 + grp;
    double kh = 0.0, fm = 0.0, w = 0.0, q = 0.0;
    if (a < n) {
      const double* fr = uc.Fc + a * uc.rp;
      for (int t = sub; t < uc.rp; t += 16) {
        const double fc = fr[t], m = mean[t], f = fc + m;
        kh += f * f, fm += f * m, w += fc * m, q += fc * fc;
      }
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
      kh += __shfl_xor(kh, off), fm += __shfl_xor(fm, off);
      w += __shfl_xor(w, off), q += __shfl_xor(q, off);
    }
    if (a < n && sub == 0) {
      const double rho = (nr - 1.0) - (nr * fm - kh);
      const double v = -w - rho / (nr - 2.0);
      panel[a * W + 2 * col] = v;
      panel[a * W + 2 * col + 1] = -q + 2.0 * v;
      sr += rho, sw += w;
    }
  }
  sr = wg_sum<HT / 64>(sr, ws);
  sw = wg_sum<HT / 64>(sw, ws);
  if (threadIdx.x == 0) {
    part[((int64_t)col * nch + blockIdx.x) * 2] = sr;
    part[((int64_t)col * nch + blockIdx.x) * 2 + 1] = sw;
  }
}

// scal[col 4 + ..] = g, mean(v), c = g + 2 mean(v), T from the chunk sums in ascending order; one thread a column
__global__ __launch_bounds__(HT) void hsic_u_scalars_kernel(const UCol* __restrict__ cols, const double* __restrict__ means,
                                                            const double* __restrict__ part, int64_t n, int64_t nch,
                                                            int ncols, double* __restrict__ scal) {
  const int col = blockIdx.x * HT + threadIdx.x;
  if (col >= ncols) return;
  const UCol uc = cols[col];
  double T = 0.0, sw = 0.0, mm = 0.0;
  for (int64_t c = 0; c < nch; ++c) T += part[((int64_t)col * nch + c) * 2], sw += part[((int64_t)col * nch + c) * 2 + 1];
  for (int t = 0; t < uc.rp; ++t) mm += means[uc.moff + t] * means[uc.moff + t];
  const double nr = (double)n;
  const double g = (1.0 - mm) + T / ((nr - 1.0) * (nr - 2.0));
  const double vbar = (-sw - T / (nr - 2.0)) / nr;
  scal[col * 4] = g, scal[col * 4 + 1] = vbar, scal[col * 4 + 2] = g + 2.0 * vbar, scal[col * 4 + 3] = T;
}

// panel[a][2 col] = v~_a = v_a - mean(v) and panel[a][2 col + 1] = a_a = (-q_a + 2 v_a) + g; one thread a pair of entries
__global__ __launch_bounds__(HT) void hsic_u_shift_kernel(const double* __restrict__ scal, int64_t n, int ncols, int W,
                                                          double* __restrict__ panel) {
  const int64_t e = (int64_t)blockIdx.x * HT + threadIdx.x;
  if (e >= n * ncols) return;
  const int64_t a = e / ncols;
  const int col = (int)(e % ncols);
  panel[a * W + 2 * col] -= scal[col * 4 + 1];
  panel[a * W + 2 * col + 1] += scal[col * 4];
}

// a column's slabs of Phi: [s0, s0 + ns)
struct ColSlabs {
  int32_t s0, ns;
};

// cov[pa nB + pb] = <A~_a, A~_b> / (n (n - 3)) and bia[..] = |Fc_a^T Fc_b|_F^2 / n^2 of every pair of
// the group pair (same: pb >= pa only): the sub-tiles' squared norms in ascending (sa, sb) order
// (a column with itself: sa <= sb, the sub-tiles above the diagonal twice), then
// + 2 n v~_a.v~_b + n^2 c_a c_b - a_a.a_b.  One thread a pair.
__global__ __launch_bounds__(HT) void hsic_u_combine_kernel(const double* __restrict__ S, const double* __restrict__ E,
                                                            const ColSlabs* __restrict__ csA,
                                                            const ColSlabs* __restrict__ csB,
                                                            const double* __restrict__ scalA,
                                                            const double* __restrict__ scalB, int nA, int nB, int nsB,
                                                            int nvB, int same, int64_t n, double* __restrict__ cov,
                                                            double* __restrict__ bia) {
  const int64_t e = (int64_t)blockIdx.x * HT + threadIdx.x;
  if (e >= (int64_t)nA * nB) return;
  const int pa = (int)(e / nB), pb = (int)(e % nB);
  if (same && pb < pa) return;
  const ColSlabs a = csA[pa], b = csB[pb];
  const bool self = same && pa == pb;
  double sq = 0.0;
  for (int i = 0; i < a.ns; ++i)
    for (int j = self ? i : 0; j < b.ns; ++j) {
      const double s = S[(int64_t)(a.s0 + i) * nsB + b.s0 + j];
      sq += (self && j > i) ? 2.0 * s : s;
    }
  // entry (row, col) of a sub-tile is register row >> 2 of lane (row & 3) 16 + col (mfma64.h, acc_row)
  const int ma = 2 * pa, mb = 2 * pb;
  const double* sub = E + ((int64_t)(ma >> 4) * nvB + (mb >> 4)) * 256;
  const int ra = ma & 15, rb = mb & 15;
  const double vv = sub[(ra >> 2) * 64 + (ra & 3) * 16 + rb];
  const double aa = sub[((ra + 1) >> 2) * 64 + ((ra + 1) & 3) * 16 + rb + 1];
  const double nr = (double)n;
  const double u = ((sq + 2.0 * nr * vv) + nr * nr * (scalA[pa * 4 + 2] * scalB[pb * 4 + 2])) - aa;
  cov[e] = u / (nr * (nr - 3.0));
  bia[e] = sq / (nr * nr);
}

constexpr int64_t kMaxGroups = 16383;  // (EG permutations a group in a sort of <= 65535 segments)
constexpr int64_t kMaxChunk = int64_t(1) << 20;
constexpr double kTolMin = 1e-14, kTolMax = 1e-3;

// a column's centred factor
struct Factor {
  DevBuf<double> Fc;         // n x rpad
  std::vector<double> mean;  // rpad column means of the uncentred factor
  int rank = 0, rpad = 0;
  double resid = 0.0;
  bool have = false;
};

}  // namespace
}  // namespace midagma

using namespace midagma;

struct midagma_hsic : ColHandle {
  DevBuf<double> XT, XS, c;  // d x n by row and sorted, 1 / (2 sigma^2) a column
  bool have_bw = false;
  double ftol = 0.0;           // the tolerance of the factors held
  std::vector<Factor> fac;     // d
  std::vector<int> est_rpad;   // d: the padded rank a column had at ftol (0: not factored yet)
  DevBuf<double*> dfptr;       // d: the factors' addresses
  DevBuf<int32_t> drpad;       // d
  // a run's scratch (kept between runs, grow-only)
  DevBuf<int64_t> dpairs;
  DevBuf<uint8_t> mark;
  DevBuf<int> flag;
  DevBuf<double> partial, vals;
  PinBuf<double> hvals;
  Event ev[3];
  double prof[4] = {0, 0, 0, 0};  // ms: medians, factorisation, permutations, evaluation
  // all_pairs' scratch (grow-only) and times
  DevBuf<double> usq, uent, ucov, ubia;
  DevBuf<int2> utiles;
  PinBuf<double> hcov, hbia;
  double uprof[2] = {0, 0};  // ms: the tiled pass over the factors, the vectors and their Grams
  void prepare(const double* X, int64_t n, int64_t d, int64_t ld, int64_t budget, hipStream_t st);
};

namespace {

using clk = std::chrono::steady_clock;
double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

void drop_factors(midagma_hsic* h) {
  h->fac.clear();
  h->fac.resize((size_t)h->d);
  h->est_rpad.assign((size_t)h->d, 0);
  h->ftol = 0.0;
}

}  // namespace

// XT, the sorted columns and the zero-range marks from X_dev (n x d, ld) on stream st; st is synchronised
void midagma_hsic::prepare(const double* X, int64_t n, int64_t d, int64_t ld, int64_t budget, hipStream_t st) {
  for (Event& e : ev) e.create();  // (the first call makes them: the device is open by now)
  const size_t nd = (size_t)n * d;
  DevBuf<int32_t> order, zr;
  order.alloc(nd), zr.alloc(d);
  colargsort_run(X, n, d, ld, order.p, budget, st);  // (throws on inf / nan)
  XT.alloc(nd), XS.alloc(nd);
  hipLaunchKernelGGL(hsic_cols_kernel, dim3((unsigned)((n + HT - 1) / HT), (unsigned)d), dim3(HT), 0, st, X, ld, order.p,
                     n, XT.p, XS.p);
  hipLaunchKernelGGL(hsic_zero_range_kernel, dim3((unsigned)((d + HT - 1) / HT)), dim3(HT), 0, st, XS.p, n, d, zr.p);
  HIP_TRY(hipGetLastError());
  hzr.resize(d);
  HIP_TRY(hipMemcpyAsync(hzr.data(), zr.p, d * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // (the scratch is freed on return)
  this->n = n, this->d = d;
  have_bw = false;
  drop_factors(this);
}

namespace {

int64_t budget_of(int64_t budget) { return budget > 0 ? budget : kDefaultBudget; }

// the factors of the listed columns (each once, none held yet) at tolerance h->ftol, `cap` columns of
// working factor each; the columns that ran out of room are returned in `again`.  Synchronises.
void factor_batch(midagma_hsic* h, const std::vector<int64_t>& cols, int cap, std::vector<int64_t>& again) {
  const int64_t n = h->n, nb = (int64_t)cols.size(), nch = (n + FCH - 1) / FCH;
  const double eta = h->ftol;
  DevBuf<double> W, dres, pmax, resid, part, mean;
  DevBuf<long long> parg;
  DevBuf<int64_t> dcols;
  DevBuf<int32_t> rank;
  W.alloc((size_t)(nb * cap * n)), dres.alloc((size_t)(nb * n)), pmax.alloc((size_t)(2 * nb * nch));
  parg.alloc((size_t)(2 * nb * nch)), dcols.alloc((size_t)nb), rank.alloc((size_t)nb), resid.alloc((size_t)nb);
  HIP_TRY(hipMemcpyAsync(dcols.p, cols.data(), nb * sizeof(int64_t), hipMemcpyHostToDevice, h->comp));
  HIP_TRY(hipMemsetAsync(rank.p, 0xff, nb * sizeof(int32_t), h->comp));
  std::vector<int32_t> hrank((size_t)nb, -1);
  std::vector<double> hresid((size_t)nb, 0.0);
  for (int step = 0; step <= cap; ++step) {
    hipLaunchKernelGGL(hsic_factor_step_kernel, dim3((unsigned)nch, (unsigned)nb), dim3(HT), 0, h->comp, h->XT.p,
                       dcols.p, h->c.p, n, nch, step, cap, eta, W.p, dres.p, pmax.p, parg.p, rank.p, resid.p);
    if (step % 16 == 15 || step == cap) {  // are all columns finished?
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(hrank.data(), rank.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost, h->comp));
      HIP_TRY(hipStreamSynchronize(h->comp));
      if (std::all_of(hrank.begin(), hrank.end(), [](int32_t r) { return r >= 0; })) break;
    }
  }
  HIP_TRY(hipMemcpyAsync(hresid.data(), resid.p, nb * sizeof(double), hipMemcpyDeviceToHost, h->comp));
  HIP_TRY(hipStreamSynchronize(h->comp));
  part.alloc((size_t)(RCAP * nch)), mean.alloc(RCAP);
  for (int64_t k = 0; k < nb; ++k) {
    const int64_t v = cols[k];
    const int r = hrank[k];
    if (hresid[k] > eta && r < n) {  // out of room
      if (cap < RCAP) {
        again.push_back(v);
        continue;
      }
      char msg[200];
      snprintf(msg, sizeof msg, "hsic: column %lld needs a rank above %d at tol %.3g (rank %d, residual %.3g)",
               (long long)v, RCAP, eta, r, hresid[k]);
      throw std::invalid_argument(msg);
    }
    Factor& f = h->fac[v];
    f.rank = r, f.rpad = (r + 15) / 16 * 16, f.resid = hresid[k];
    f.Fc.alloc((size_t)(n * f.rpad));
    f.mean.resize((size_t)f.rpad);
    const double* Wc = W.p + k * (int64_t)cap * n;
    hipLaunchKernelGGL(hsic_colsum_kernel, dim3((unsigned)nch, (unsigned)r), dim3(HT), 0, h->comp, Wc, n, nch, part.p);
    hipLaunchKernelGGL(hsic_mean_kernel, dim3((unsigned)((f.rpad + HT - 1) / HT)), dim3(HT), 0, h->comp, part.p, nch, r,
                       f.rpad, (double)n, mean.p);
    hipLaunchKernelGGL(hsic_centre_kernel, dim3((unsigned)((n * f.rpad + HT - 1) / HT)), dim3(HT), 0, h->comp, Wc,
                       mean.p, n, r, f.rpad, f.Fc.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(f.mean.data(), mean.p, f.rpad * sizeof(double), hipMemcpyDeviceToHost, h->comp));
    HIP_TRY(hipStreamSynchronize(h->comp));  // (part and mean are reused by the next column)
    f.have = true;
    h->est_rpad[v] = f.rpad;
  }
}

// make the factors of the listed columns (each once) that are not held, in batches whose working
// factors stay within `budget` (at least one column a batch)
void ensure_factors(midagma_hsic* h, const std::vector<int64_t>& cols, double tol, int64_t budget) {
  if (h->ftol != tol) {
    drop_factors(h);
    h->ftol = tol;
  }
  const clk::time_point t0 = clk::now();
  std::vector<int64_t> todo, again;
  for (int64_t v : cols)
    if (!h->fac[v].have) todo.push_back(v);
  for (int pass = 0; pass < 2 && !todo.empty(); ++pass) {
    const int cap = pass ? RCAP : RFIRST;
    const int64_t per = h->n * 8 * (cap + 2);
    const int64_t nbmax = std::max<int64_t>(1, std::min<int64_t>(65535, budget / per));
    again.clear();
    for (size_t k0 = 0; k0 < todo.size(); k0 += (size_t)nbmax) {
      const std::vector<int64_t> batch(todo.begin() + k0, todo.begin() + std::min(todo.size(), k0 + (size_t)nbmax));
      factor_batch(h, batch, cap, again);
    }
    todo.swap(again);
  }
  h->prof[1] += ms_since(t0);
}

// the factors' addresses and padded ranks on the device
void upload_factor_table(midagma_hsic* h) {
  const int64_t d = h->d;
  std::vector<double*> fp((size_t)d, nullptr);
  std::vector<int32_t> rp((size_t)d, 0);
  for (int64_t v = 0; v < d; ++v)
    if (h->fac[v].have) fp[v] = h->fac[v].Fc.p, rp[v] = h->fac[v].rpad;
  h->dfptr.alloc((size_t)d), h->drpad.alloc((size_t)d);
  HIP_TRY(hipMemcpyAsync(h->dfptr.p, fp.data(), d * sizeof(double*), hipMemcpyHostToDevice, h->comp));
  HIP_TRY(hipMemcpyAsync(h->drpad.p, rp.data(), d * sizeof(int32_t), hipMemcpyHostToDevice, h->comp));
  HIP_TRY(hipStreamSynchronize(h->comp));  // (the host vectors end here)
}

// the host's permutations f0 .. f0 + nf - 1 into h->perm, checked on the device; synchronises
void host_perms(midagma_hsic* h, const int32_t* perms, int64_t f0, int64_t nf) {
  const int64_t n = h->n;
  h->mark.alloc((size_t)(nf * n)), h->flag.alloc(2);
  HIP_TRY(hipMemcpyAsync(h->perm.p, perms + f0 * n, (size_t)(nf * n) * sizeof(int32_t), hipMemcpyHostToDevice, h->comp));
  HIP_TRY(hipMemsetAsync(h->mark.p, 0, (size_t)(nf * n), h->comp));
  HIP_TRY(hipMemsetAsync(h->flag.p, 0, 2 * sizeof(int), h->comp));
  const dim3 grid((unsigned)((n + HT - 1) / HT), (unsigned)nf);
  hipLaunchKernelGGL(hsic_perm_mark_kernel, grid, dim3(HT), 0, h->comp, h->perm.p, n, h->mark.p, h->flag.p);
  hipLaunchKernelGGL(hsic_perm_check_kernel, grid, dim3(HT), 0, h->comp, h->mark.p, n, h->flag.p);
  HIP_TRY(hipGetLastError());
  int bad[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(bad, h->flag.p, sizeof bad, hipMemcpyDeviceToHost, h->comp));
  HIP_TRY(hipStreamSynchronize(h->comp));  // (no row of Gc is gathered through an index that was not checked)
  if (bad[0]) throw std::invalid_argument("hsic_run: permutation index outside [0, n)");
  if (bad[1]) throw std::invalid_argument("hsic_run: a row of perms is not a permutation");
}

// the row-chunk size of n: 2048 rows, 512 a wave
int64_t chunk_rule(int64_t) { return 2048; }

}  // namespace

extern "C" const char* midagma_hsic_last_error(const midagma_hsic* h) { return abi_last_error(h); }

extern "C" void midagma_hsic_destroy(midagma_hsic* h) { col_destroy(h); }

extern "C" int midagma_hsic_create(midagma_hsic** out, int device) { return col_create(out, device, "hsic_create"); }

extern "C" int midagma_hsic_set_data(midagma_hsic* h, const double* X, int64_t n, int64_t d, int64_t budget_bytes) {
  return col_set_data(h, "hsic_set_data", X, n, d, budget_bytes);
}

extern "C" int midagma_hsic_set_data_dev(midagma_hsic* h, const double* X_dev, int64_t n, int64_t d, int64_t ld,
                                         int64_t budget_bytes, void* hip_stream) {
  return col_set_data_dev(h, "hsic_set_data_dev", X_dev, n, d, ld, budget_bytes, hip_stream);
}

extern "C" int midagma_hsic_set_bandwidths(midagma_hsic* h, const double* sigma2, int64_t d) {
  if (!h) return abi_fail(no_handle<midagma_hsic>, MIDAGMA_E_ARG, "hsic_set_bandwidths: null handle");
  if (h->n == 0) return abi_fail(h, MIDAGMA_E_ARG, "hsic_set_bandwidths: set the data first");
  if (!sigma2 || d != h->d) return abi_fail(h, MIDAGMA_E_ARG, "hsic_set_bandwidths: need d squared bandwidths");
  return install_bandwidths(h, sigma2, "hsic_set_bandwidths", [h] { drop_factors(h); });
}

extern "C" int midagma_hsic_median_bandwidths(midagma_hsic* h, const int64_t* cols, int64_t ncols, double* sigma2_out) {
  if (!h) return abi_fail(no_handle<midagma_hsic>, MIDAGMA_E_ARG, "hsic_median_bandwidths: null handle");
  if (h->n == 0) return abi_fail(h, MIDAGMA_E_ARG, "hsic_median_bandwidths: set the data first");
  const int64_t n = h->n, d = h->d;
  std::vector<int64_t> list;  // (a column's value does not depend on the list)
  if (const char* why = listed_columns(cols, ncols, d, list))
    return abi_fail(h, MIDAGMA_E_ARG, says("hsic_median_bandwidths", why));
  const int64_t m = (int64_t)list.size();
  std::vector<double> med(m), s2(d, 1.0);
  h->prof[0] = 0.0;
  if (m > 0) {
    const clk::time_point t0 = clk::now();
    const int rc = abi_guarded(h, [&] {
      const int64_t G = std::min<int64_t>(MG, (n + HT - 1) / HT);
      DevBuf<int64_t> dcols;
      DevBuf<MedState> st;
      DevBuf<long long> cnt;
      DevBuf<double> mn, dmed;
      dcols.alloc(m), st.alloc(2 * m), cnt.alloc(2 * m * G), mn.alloc(2 * m * G), dmed.alloc(m);
      HIP_TRY(hipMemcpyAsync(dcols.p, list.data(), m * sizeof(int64_t), hipMemcpyHostToDevice, h->comp));
      const int rounds = 64;  // 63 halvings empty a range below 2^63; the last round counts at the result
      for (int r = 0; r < rounds; ++r)
        hipLaunchKernelGGL(hsic_median_round_kernel, dim3((unsigned)G, (unsigned)m), dim3(HT), 0, h->comp, h->XS.p,
                           dcols.p, n, r, m, st.p, cnt.p, mn.p);
      hipLaunchKernelGGL(hsic_median_finish_kernel, dim3((unsigned)((m + HT - 1) / HT)), dim3(HT), 0, h->comp, n,
                         (rounds - 1) & 1, m, G, st.p, cnt.p, mn.p, dmed.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(med.data(), dmed.p, m * sizeof(double), hipMemcpyDeviceToHost, h->comp));
      HIP_TRY(hipStreamSynchronize(h->comp));
    });
    if (rc != MIDAGMA_OK) return rc;
    h->prof[0] = ms_since(t0);
    for (int64_t k = 0; k < m; ++k) s2[list[k]] = med[k];
  }
  const int rc = install_bandwidths(h, s2.data(), "hsic_median_bandwidths", [h] { drop_factors(h); });
  if (rc != MIDAGMA_OK) return rc;
  if (sigma2_out) std::copy(s2.begin(), s2.end(), sigma2_out);
  return MIDAGMA_OK;
}

namespace {

const char* bad_tol(double tol) {
  return (tol >= kTolMin && tol <= kTolMax) ? nullptr : "tol must be in [1e-14, 1e-3]";
}

}  // namespace

extern "C" int midagma_hsic_factor(midagma_hsic* h, const int64_t* cols, int64_t ncols, double tol, int32_t* rank_out,
                                   double* resid_out) {
  if (!h) return abi_fail(no_handle<midagma_hsic>, MIDAGMA_E_ARG, "hsic_factor: null handle");
  if (const char* why = bad_tol(tol)) return abi_fail(h, MIDAGMA_E_ARG, std::string("hsic_factor: ") + why);
  if (ncols < 0 || (ncols > 0 && !cols)) return abi_fail(h, MIDAGMA_E_ARG, "hsic_factor: need ncols >= 0 columns");
  if (h->n == 0) return abi_fail(h, MIDAGMA_E_ARG, "hsic_factor: set the data first");
  if (!h->have_bw) return abi_fail(h, MIDAGMA_E_ARG, "hsic_factor: set the bandwidths first");
  std::vector<int64_t> list;  // (a column's factor does not depend on the list or on its order)
  if (const char* why = ncols ? listed_columns(cols, ncols, h->d, list) : nullptr)
    return abi_fail(h, MIDAGMA_E_ARG, says("hsic_factor", why));
  h->prof[1] = 0.0;
  const int rc = abi_guarded(h, [&] { ensure_factors(h, list, tol, kDefaultBudget / 2); });
  if (rc != MIDAGMA_OK) {
    (void)hipStreamSynchronize(h->comp);
    return rc;
  }
  for (int64_t k = 0; k < ncols; ++k) {
    if (rank_out) rank_out[k] = h->fac[cols[k]].rank;
    if (resid_out) resid_out[k] = h->fac[cols[k]].resid;
  }
  return MIDAGMA_OK;
}

extern "C" int midagma_hsic_get_factor(midagma_hsic* h, int64_t col, double* fc_out, double* mean_out) {
  if (!h) return abi_fail(no_handle<midagma_hsic>, MIDAGMA_E_ARG, "hsic_get_factor: null handle");
  if (h->n == 0 || col < 0 || col >= h->d || !h->fac[col].have || !fc_out)
    return abi_fail(h, MIDAGMA_E_ARG, "hsic_get_factor: need an output and a column that midagma_hsic_factor factored");
  const Factor& f = h->fac[col];
  return abi_guarded(h, [&] {
    HIP_TRY(hipMemcpyAsync(fc_out, f.Fc.p, (size_t)(h->n * f.rpad) * sizeof(double), hipMemcpyDeviceToHost, h->comp));
    HIP_TRY(hipStreamSynchronize(h->comp));
    if (mean_out) std::copy(f.mean.begin(), f.mean.end(), mean_out);
  });
}

extern "C" int midagma_hsic_run(midagma_hsic* h, const int64_t* pairs, int64_t m, int64_t P, const int32_t* perms,
                                uint64_t seed, double tol, int64_t chunk, int64_t budget_bytes, double* stat,
                                int64_t* ge, double* null_out) {
  if (!h) return abi_fail(no_handle<midagma_hsic>, MIDAGMA_E_ARG, "hsic_run: null handle");
  if (m < 0 || P < 0 || P > kMaxP) return abi_fail(h, MIDAGMA_E_ARG, "hsic_run: need m >= 0 and 0 <= P <= 65535");
  if (m > 0 && (!pairs || !stat || !ge)) return abi_fail(h, MIDAGMA_E_ARG, "hsic_run: null pointer");
  if (const char* why = bad_tol(tol)) return abi_fail(h, MIDAGMA_E_ARG, std::string("hsic_run: ") + why);
  if (chunk != 0 && (chunk < 16 || chunk > kMaxChunk || chunk % 16))
    return abi_fail(h, MIDAGMA_E_ARG, "hsic_run: chunk must be 0 or a multiple of 16 in [16, 2^20]");
  if (h->n == 0) return abi_fail(h, MIDAGMA_E_ARG, "hsic_run: set the data first");
  if (!h->have_bw) return abi_fail(h, MIDAGMA_E_ARG, "hsic_run: set the bandwidths first");
  for (int64_t k = 0; k < 2 * m; ++k)
    if (pairs[k] < 0 || pairs[k] >= h->d) return abi_fail(h, MIDAGMA_E_ARG, "hsic_run: pair index outside [0, d)");
  h->prof[1] = h->prof[2] = h->prof[3] = 0.0;
  if (m == 0) return MIDAGMA_OK;
  const int64_t n = h->n, d = h->d, P1 = P + 1, NG = (P1 + EG - 1) / EG;
  const int64_t budget = budget_of(budget_bytes), fbudget = budget / 2, ebudget = budget - fbudget;
  const int64_t ch = chunk ? chunk : chunk_rule(n), nchunk = (n + ch - 1) / ch;
  const bool dev_perms = perms == nullptr;
  const int64_t sort_bytes = (P > 0 && dev_perms) ? perm_sort_bytes(n) : 0;

  const int rc = abi_guarded(h, [&] {
    if (h->ftol != tol) {
      drop_factors(h);
      h->ftol = tol;
    }
    h->dpairs.alloc((size_t)(2 * m));
    HIP_TRY(hipMemcpyAsync(h->dpairs.p, pairs, 2 * m * sizeof(int64_t), hipMemcpyHostToDevice, h->comp));
    std::vector<uint8_t> in_group(d);
    NullCount count{stat, ge, null_out, P};
    for (int64_t qs = 0; qs < m;) {
      // the next column group: consecutive pairs while the factors of their columns (at the padded
      // rank a column had before, 64 for one not factored yet) stay within half the budget
      std::fill(in_group.begin(), in_group.end(), 0);
      std::vector<int64_t> gcols;
      int64_t qe = qs, bytes = 0;
      for (; qe < m; ++qe) {
        int64_t add = 0;
        for (int s = 0; s < 2; ++s) {
          const int64_t v = pairs[2 * qe + s];
          if (!in_group[v] && !(s == 1 && v == pairs[2 * qe])) add += n * 8 * (h->est_rpad[v] ? h->est_rpad[v] : 64);
        }
        if (qe > qs && bytes + add > fbudget) break;
        bytes += add;
        for (int s = 0; s < 2; ++s) {
          const int64_t v = pairs[2 * qe + s];
          if (!in_group[v]) in_group[v] = 1, gcols.push_back(v);
        }
      }
      bool all = true;
      for (int64_t v : gcols) all = all && h->fac[v].have;
      if (!all) {
        HIP_TRY(hipStreamSynchronize(h->comp));
        for (int64_t v = 0; v < d; ++v)  // the factors of the other columns make room
          if (!in_group[v] && h->fac[v].have) h->fac[v] = Factor{};
        ensure_factors(h, gcols, tol, fbudget);
      }
      upload_factor_table(h);
      int nbmax = 1;
      for (int64_t q = qs; q < qe; ++q)
        nbmax = std::max(nbmax, ((h->fac[pairs[2 * q]].rpad + 31) / 32) * ((h->fac[pairs[2 * q + 1]].rpad + 31) / 32));
      // bytes of scratch one group of EG evaluations takes
      const int64_t per = EG * (nchunk * nbmax * 1024 * 8 + 16 + (P > 0 ? n * 4 + (dev_perms ? 0 : n) : 0) + sort_bytes);
      const int64_t ngmax = std::max<int64_t>(1, std::min<int64_t>(kMaxGroups, ebudget / per));
      for (int64_t g0 = qs * NG; g0 < qe * NG; g0 += ngmax) {
        const int64_t ng = std::min(ngmax, qe * NG - g0), g1 = g0 + ng;
        // the chunk's permutations: f = q P + p - 1 for p >= 1, ascending with the evaluations
        const int64_t qa = g0 / NG, pa = (g0 % NG) * EG, qb = (g1 - 1) / NG;
        const int64_t pb = std::min(P, ((g1 - 1) % NG) * EG + EG - 1);
        const int64_t f0 = qa * P + (pa ? pa - 1 : 0), f1 = qb * P + pb, nf = f1 - f0;
        h->partial.alloc((size_t)(ng * EG * nchunk * nbmax * 1024));
        h->vals.alloc((size_t)(ng * EG)), h->hvals.alloc((size_t)(ng * EG));
        HIP_TRY(hipEventRecord(h->ev[0], h->comp));
        if (nf > 0) {
          h->perm.alloc((size_t)(nf * n));
          if (dev_perms)
            h->sort.run(seed, f0, nf, P, n, h->perm.p, nullptr, h->comp);
          else
            host_perms(h, perms, f0, nf);
        }
        HIP_TRY(hipEventRecord(h->ev[1], h->comp));
        hipLaunchKernelGGL(hsic_eval_kernel, dim3((unsigned)nchunk, (unsigned)ng, (unsigned)nbmax), dim3(HT), 0, h->comp,
                           h->dfptr.p, h->drpad.p, h->dpairs.p, h->perm.p, g0, f0, n, ch, P, NG, nbmax, h->partial.p);
        hipLaunchKernelGGL(hsic_value_kernel, dim3((unsigned)(ng * EG)), dim3(HT), 0, h->comp, h->partial.p, h->drpad.p,
                           h->dpairs.p, g0, n, nchunk, P, NG, nbmax, h->vals.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(h->ev[2], h->comp));
        HIP_TRY(hipMemcpyAsync(h->hvals.p, h->vals.p, (size_t)(ng * EG) * sizeof(double), hipMemcpyDeviceToHost,
                               h->comp));
        HIP_TRY(hipStreamSynchronize(h->comp));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        h->prof[2] += ms;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
        h->prof[3] += ms;
        for (int64_t g = g0; g < g1; ++g)
          for (int64_t s = 0; s < EG; ++s) {
            const int64_t q = g / NG, p = (g % NG) * EG + s;
            if (p > P) continue;
            const bool zero = h->hzr[pairs[2 * q]] || h->hzr[pairs[2 * q + 1]];
            const double v = zero ? 0.0 : h->hvals.p[(g - g0) * EG + s];
            count.add(q, p, v, v, zero);
          }
      }
      qs = qe;
    }
  });
  if (rc != MIDAGMA_OK) (void)hipStreamSynchronize(h->comp);  // leave nothing in flight that reads the scratch
  return rc;
}

namespace {

// a column group of all_pairs with what the passes read of it (valid while its factors are held)
struct UGroup {
  std::vector<int64_t> cols;
  int ns = 0, nv = 0;  // slabs of Phi, slabs of the vector panel
  DevBuf<double> panel, scal, means;
  DevBuf<UCol> ucols;
  DevBuf<Slab> slabs, vslabs;
  DevBuf<ColSlabs> cs;
};

float ms_between(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, a, b));
  return ms;
}

// the group's slab tables, the O(n) vectors of its columns (panel: n x 16 nv, column 2 k and
// 2 k + 1 the vectors v~ and a of the group's column k) and their scalars; synchronises
void build_group(midagma_hsic* h, UGroup& g) {
  const int64_t n = h->n, nch = (n + FCH - 1) / FCH;
  const int nc = (int)g.cols.size();
  std::vector<Slab> slabs, vslabs;
  std::vector<ColSlabs> cs;
  std::vector<UCol> uc;
  std::vector<double> means;
  for (int64_t v : g.cols) {
    const Factor& f = h->fac[v];
    cs.push_back(ColSlabs{(int32_t)slabs.size(), f.rpad / 16});
    uc.push_back(UCol{f.Fc.p, f.rpad, (int32_t)means.size()});
    for (int s = 0; s < f.rpad / 16; ++s) slabs.push_back(Slab{f.Fc.p + 16 * s, f.rpad});
    means.insert(means.end(), f.mean.begin(), f.mean.end());
  }
  g.ns = (int)slabs.size(), g.nv = (2 * nc + 15) / 16;
  const int W = 16 * g.nv;
  g.panel.alloc((size_t)(n * W)), g.scal.alloc((size_t)nc * 4), g.means.alloc(means.size());
  g.ucols.alloc((size_t)nc), g.slabs.alloc(slabs.size()), g.vslabs.alloc((size_t)g.nv), g.cs.alloc((size_t)nc);
  for (int s = 0; s < g.nv; ++s) vslabs.push_back(Slab{g.panel.p + 16 * s, W});
  DevBuf<double> part;
  part.alloc((size_t)(nc * nch * 2));
  hipStream_t st = h->comp;
  HIP_TRY(hipEventRecord(h->ev[0], st));
  HIP_TRY(hipMemcpyAsync(g.means.p, means.data(), means.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(g.ucols.p, uc.data(), uc.size() * sizeof(UCol), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(g.slabs.p, slabs.data(), slabs.size() * sizeof(Slab), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(g.vslabs.p, vslabs.data(), vslabs.size() * sizeof(Slab), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(g.cs.p, cs.data(), cs.size() * sizeof(ColSlabs), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(g.panel.p, 0, (size_t)(n * W) * sizeof(double), st));  // (the padding columns)
  hipLaunchKernelGGL(hsic_u_rows_kernel, dim3((unsigned)nch, (unsigned)nc), dim3(HT), 0, st, g.ucols.p, g.means.p, n, nch,
                     W, g.panel.p, part.p);
  hipLaunchKernelGGL(hsic_u_scalars_kernel, dim3((unsigned)((nc + HT - 1) / HT)), dim3(HT), 0, st, g.ucols.p, g.means.p,
                     part.p, n, nch, nc, g.scal.p);
  hipLaunchKernelGGL(hsic_u_shift_kernel, dim3((unsigned)((n * nc + HT - 1) / HT)), dim3(HT), 0, st, g.scal.p, n, nc, W,
                     g.panel.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(h->ev[1], st));
  HIP_TRY(hipStreamSynchronize(st));  // (the host vectors and `part` end here)
  h->uprof[1] += ms_between(h->ev[0], h->ev[1]);
}

// out = the chunk-summed sub-tiles of PA^T PB (squared and summed when sq) for the panels' slab
// tables, the tiles on and above the diagonal only when `same`, in batches of tiles whose chunk
// partials stay within ebudget (at least one tile)
void tiled_gram(midagma_hsic* h, const Slab* sa, int nsA, const Slab* sb, int nsB, bool same, bool sq, int64_t ch,
                int64_t ebudget, double* out) {
  const int64_t n = h->n, nchunk = (n + ch - 1) / ch;
  const int TA = (nsA + TS - 1) / TS, TB = (nsB + TS - 1) / TS;
  std::vector<int2> tiles;
  for (int a = 0; a < TA; ++a)
    for (int b = same ? a : 0; b < TB; ++b) tiles.push_back(int2{a, b});
  const int64_t nt = (int64_t)tiles.size();
  h->utiles.alloc((size_t)nt);
  HIP_TRY(hipMemcpyAsync(h->utiles.p, tiles.data(), nt * sizeof(int2), hipMemcpyHostToDevice, h->comp));
  int64_t tmax = std::max<int64_t>(1, ebudget / (nchunk * TILE_E * 8));
  tmax = std::min<int64_t>(std::min<int64_t>(tmax, 65535), std::max<int64_t>(1, kMaxN / nchunk));
  for (int64_t t0 = 0; t0 < nt; t0 += tmax) {
    const int nb = (int)std::min(tmax, nt - t0);
    h->partial.alloc((size_t)(nchunk * nb * TILE_E));
    hipLaunchKernelGGL(hsic_tile_kernel, dim3((unsigned)(nchunk * nb)), dim3(HT), 0, h->comp, sa, sb, h->utiles.p + t0, nb,
                       nsA, nsB, n, ch, h->partial.p);
    if (sq)
      hipLaunchKernelGGL(hsic_tile_reduce_kernel<true>, dim3(TSUB, (unsigned)nb), dim3(HT), 0, h->comp, h->partial.p,
                         h->utiles.p + t0, nb, nsA, nsB, nchunk, out);
    else
      hipLaunchKernelGGL(hsic_tile_reduce_kernel<false>, dim3(TSUB, (unsigned)nb), dim3(HT), 0, h->comp, h->partial.p,
                         h->utiles.p + t0, nb, nsA, nsB, nchunk, out);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(h->comp));  // (`tiles` ends here; h->partial may be regrown by the next call)
}

// cov_U and the biased statistic of every pair (a in A, b in B; A == B: b >= a) into the host
// matrices (nu x nu, by the columns' places ua / ub in the call's list), mirrored
void group_pair(midagma_hsic* h, const UGroup& A, const UGroup& B, const std::vector<int>& placeA,
                const std::vector<int>& placeB, int64_t ch, int64_t ebudget, int64_t nu, double* cov, double* bia) {
  const bool same = &A == &B;
  const int nA = (int)A.cols.size(), nB = (int)B.cols.size();
  const size_t np = (size_t)nA * nB;
  h->usq.alloc((size_t)A.ns * B.ns), h->uent.alloc((size_t)A.nv * B.nv * 256);
  h->ucov.alloc(np), h->ubia.alloc(np), h->hcov.alloc(np), h->hbia.alloc(np);
  HIP_TRY(hipEventRecord(h->ev[0], h->comp));
  tiled_gram(h, A.slabs.p, A.ns, B.slabs.p, B.ns, same, true, ch, ebudget, h->usq.p);
  HIP_TRY(hipEventRecord(h->ev[1], h->comp));
  tiled_gram(h, A.vslabs.p, A.nv, B.vslabs.p, B.nv, same, false, ch, ebudget, h->uent.p);
  hipLaunchKernelGGL(hsic_u_combine_kernel, dim3((unsigned)((np + HT - 1) / HT)), dim3(HT), 0, h->comp, h->usq.p,
                     h->uent.p, A.cs.p, B.cs.p, A.scal.p, B.scal.p, nA, nB, B.ns, B.nv, same ? 1 : 0, h->n, h->ucov.p,
                     h->ubia.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(h->ev[2], h->comp));
  HIP_TRY(hipMemcpyAsync(h->hcov.p, h->ucov.p, np * sizeof(double), hipMemcpyDeviceToHost, h->comp));
  HIP_TRY(hipMemcpyAsync(h->hbia.p, h->ubia.p, np * sizeof(double), hipMemcpyDeviceToHost, h->comp));
  HIP_TRY(hipStreamSynchronize(h->comp));
  h->uprof[0] += ms_between(h->ev[0], h->ev[1]);
  h->uprof[1] += ms_between(h->ev[1], h->ev[2]);
  for (int a = 0; a < nA; ++a)
    for (int b = same ? a : 0; b < nB; ++b) {
      // a zero-range column: the centred matrix is exactly 0 (as midagma_hsic_run decides it)
      const bool zero = h->hzr[A.cols[a]] || h->hzr[B.cols[b]];
      const double c = zero ? 0.0 : h->hcov.p[(size_t)a * nB + b], s = zero ? 0.0 : h->hbia.p[(size_t)a * nB + b];
      const int64_t ua = placeA[a], ub = placeB[b];
      cov[ua * nu + ub] = cov[ub * nu + ua] = c;
      bia[ua * nu + ub] = bia[ub * nu + ua] = s;
    }
}

}  // namespace

extern "C" int midagma_hsic_all_pairs(midagma_hsic* h, const int64_t* cols, int64_t ncols, double tol, int64_t chunk,
                                      int64_t budget_bytes, double* cov_u_out, double* biased_out) {
  if (!h) return abi_fail(no_handle<midagma_hsic>, MIDAGMA_E_ARG, "hsic_all_pairs: null handle");
  if (!cov_u_out) return abi_fail(h, MIDAGMA_E_ARG, "hsic_all_pairs: null pointer");
  if (cols && ncols < 0) return abi_fail(h, MIDAGMA_E_ARG, "hsic_all_pairs: ncols < 0");
  if (const char* why = bad_tol(tol)) return abi_fail(h, MIDAGMA_E_ARG, std::string("hsic_all_pairs: ") + why);
  if (chunk != 0 && (chunk < 16 || chunk > kMaxChunk || chunk % 16))
    return abi_fail(h, MIDAGMA_E_ARG, "hsic_all_pairs: chunk must be 0 or a multiple of 16 in [16, 2^20]");
  if (h->n == 0) return abi_fail(h, MIDAGMA_E_ARG, "hsic_all_pairs: set the data first");
  if (h->n < 4) return abi_fail(h, MIDAGMA_E_ARG, "hsic_all_pairs: the U-centred statistic needs n >= 4");
  if (!h->have_bw) return abi_fail(h, MIDAGMA_E_ARG, "hsic_all_pairs: set the bandwidths first");
  const int64_t n = h->n, d = h->d, nout = cols ? ncols : d;
  // the listed columns, each once, ascending (a pair's smaller column is always the A side, so its
  // value does not depend on the list); place[k]: where entry k's column is
  std::vector<int64_t> uniq;
  if (const char* why = listed_columns(cols, ncols, d, uniq)) return abi_fail(h, MIDAGMA_E_ARG, says("hsic_all_pairs", why));
  std::vector<int64_t> place((size_t)nout), seen((size_t)d, -1);
  for (size_t u = 0; u < uniq.size(); ++u) seen[uniq[u]] = (int64_t)u;
  for (int64_t k = 0; k < nout; ++k) place[k] = seen[cols ? cols[k] : k];
  h->prof[1] = h->uprof[0] = h->uprof[1] = 0.0;
  if (nout == 0) return MIDAGMA_OK;
  const int64_t nu = (int64_t)uniq.size();
  const int64_t budget = budget_of(budget_bytes), fbudget = budget / 2, ebudget = budget - fbudget;
  const int64_t ch = chunk ? chunk : chunk_rule(n);
  std::vector<double> cov((size_t)(nu * nu), 0.0), bia((size_t)(nu * nu), 0.0);

  const int rc = abi_guarded(h, [&] {
    if (h->ftol != tol) {
      drop_factors(h);
      h->ftol = tol;
    }
    // column groups: every column at once if the factors and vectors fit half the budget (at the
    // padded rank a column had before, 64 for one not factored yet), else consecutive groups of a
    // quarter of it each, two of which are held at a time
    auto bytes_of = [&](int64_t v) { return n * 8 * ((h->est_rpad[v] ? h->est_rpad[v] : 64) + 2); };
    auto total_bytes = [&] {
      int64_t t = 0;
      for (int64_t v : uniq) t += bytes_of(v);
      return t;
    };
    int64_t total = total_bytes();
    if (total > fbudget) {
      // groups are needed: size them by the ranks, not by the estimate (half as many columns a group,
      // so twice the groups and four times the group pairs).  The columns not factored at this tol
      // yet are factored once for their ranks, a budget's worth at a time, the others making room.
      std::vector<int64_t> unknown;
      for (int64_t v : uniq)
        if (!h->est_rpad[v]) unknown.push_back(v);
      for (size_t k0 = 0; k0 < unknown.size();) {
        size_t k1 = k0;
        for (int64_t b = 0; k1 < unknown.size() && (k1 == k0 || b + bytes_of(unknown[k1]) <= fbudget); ++k1)
          b += bytes_of(unknown[k1]);
        HIP_TRY(hipStreamSynchronize(h->comp));
        for (int64_t v = 0; v < d; ++v)
          if (h->fac[v].have) h->fac[v] = Factor{};
        ensure_factors(h, std::vector<int64_t>(unknown.begin() + k0, unknown.begin() + k1), tol, fbudget);
        k0 = k1;
      }
      total = total_bytes();
    }
    const int64_t cap = total <= fbudget ? total : fbudget / 2;
    std::vector<std::vector<int>> groups(1);  // places in uniq
    int64_t bytes = 0;
    for (int64_t u = 0; u < nu; ++u) {
      const int64_t add = bytes_of(uniq[u]);
      if (!groups.back().empty() && bytes + add > cap) groups.emplace_back(), bytes = 0;
      groups.back().push_back((int)u), bytes += add;
    }
    std::vector<uint8_t> keep((size_t)d);
    // hold the factors of the marked columns (the others make room when one is missing), then the group's tables
    auto load = [&](UGroup& g, const std::vector<int>& places) {
      g.cols.clear();
      for (int u : places) g.cols.push_back(uniq[u]);
      bool all = true;
      for (int64_t v : g.cols) all = all && h->fac[v].have;
      if (!all) {
        HIP_TRY(hipStreamSynchronize(h->comp));
        for (int64_t v = 0; v < d; ++v)
          if (!keep[v] && h->fac[v].have) h->fac[v] = Factor{};
        ensure_factors(h, g.cols, tol, fbudget);
      }
      build_group(h, g);
    };
    for (size_t ga = 0; ga < groups.size(); ++ga) {
      UGroup A;
      std::fill(keep.begin(), keep.end(), 0);
      for (int u : groups[ga]) keep[uniq[u]] = 1;
      load(A, groups[ga]);
      group_pair(h, A, A, groups[ga], groups[ga], ch, ebudget, nu, cov.data(), bia.data());
      for (size_t gb = ga + 1; gb < groups.size(); ++gb) {
        UGroup B;
        std::fill(keep.begin(), keep.end(), 0);
        for (int u : groups[ga]) keep[uniq[u]] = 1;
        for (int u : groups[gb]) keep[uniq[u]] = 1;
        load(B, groups[gb]);
        group_pair(h, A, B, groups[ga], groups[gb], ch, ebudget, nu, cov.data(), bia.data());
      }
    }
  });
  if (rc != MIDAGMA_OK) {
    (void)hipStreamSynchronize(h->comp);  // leave nothing in flight that reads the scratch
    return rc;
  }
  for (int64_t k = 0; k < nout; ++k)
    for (int64_t l = 0; l < nout; ++l) {
      cov_u_out[k * nout + l] = cov[(size_t)(place[k] * nu + place[l])];
      if (biased_out) biased_out[k * nout + l] = bia[(size_t)(place[k] * nu + place[l])];
    }
  return MIDAGMA_OK;
}

extern "C" int midagma_hsic_all_pairs_profile(const midagma_hsic* h, double* ms_out) {
  if (!h || !ms_out) return abi_fail(no_handle<midagma_hsic>, MIDAGMA_E_ARG, "hsic_all_pairs_profile: bad arguments");
  ms_out[0] = h->prof[1], ms_out[1] = h->uprof[0], ms_out[2] = h->uprof[1];
  return MIDAGMA_OK;
}

extern "C" int midagma_hsic_perms(midagma_hsic* h, int64_t q, int64_t P, uint64_t seed, int32_t* perms_out) {
  return col_perms(h, "hsic_perms", q, P, seed, perms_out, nullptr, nullptr);
}

extern "C" int midagma_hsic_profile(const midagma_hsic* h, double* ms_out) {
  if (!h || !ms_out) return abi_fail(no_handle<midagma_hsic>, MIDAGMA_E_ARG, "hsic_profile: bad arguments");
  std::copy(h->prof, h->prof + 4, ms_out);
  return MIDAGMA_OK;
}
