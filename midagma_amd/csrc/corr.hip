// Pearson and Spearman on the device: average-tie column ranks of a row-major X (midagma_colrank),
// the columns' stable argsort (midagma_colargsort) and the Pearson correlation matrix of its columns (midagma_corr).  Spearman is midagma_corr on
// the ranks.  The analytic p-values are host work (midagma_amd/mi_tests.py).
//
// Ranks: a chunk of columns at a time (the chunk's scratch fits the byte budget).  The chunk is
// read by 64 x 64 tiles and transposed through LDS into column-major 64-bit keys (an order-
// preserving map of the doubles, -0.0 as +0.0) with the row index as the payload, then sorted per
// column by a stable LSD radix sort, 8 bits a pass: a histogram per (column, 4096-key wave
// segment, digit), an exclusive scan per column in (digit, segment) order, and a scatter in which
// each wave walks its segment 64 keys at a time and ranks equal digits by ballots (no atomics,
// so the sort is stable and the same run to run).  A pass in which every key of a column has the
// same digit is skipped for that column: the OR and AND of the column's keys, gathered while the
// keys are written, say which passes are live, and every kernel derives the column's ping-pong
// side from them.  Tie runs come from head / tail flags of the sorted keys within a wave and, for
// a run that crosses the wave's 64 positions, one binary search on the sorted column, so the cost
// does not depend on the run length.  The ranks are scattered into the column's free key buffer
// (a column-major image) and go to R by tiles through LDS.  midagma_colargsort returns the sorted row
// payloads instead (the stable argsort of every column); the eight passes are launch_segsort of
// colsort.h, which dcor.hip also runs on the keys of its permutations.
//
// Correlations: one pass gives every column's sum, min and max (constant iff max == min on the raw
// values); X minus the column means is staged in zero-padded row chunks and goes through the FP64
// MFMA GEMM of midagma_gram, the chunk Grams summed in a fixed order; Rho = G_ij / sqrt(G_ii G_jj).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include "colsort.h"
#include "devmem.h"

namespace {

using namespace midagma;

constexpr int RT = 64;               // tile edge of the LDS transposes
constexpr int WAVES = NTHREADS / 64;
constexpr int64_t SEG = 4096;        // keys per wave segment of the radix passes
constexpr int RADIX = 256, PASSES = 8;
constexpr int64_t kDefaultBudget = int64_t(2) << 30;

__device__ inline uint64_t key_of(double v) {
  uint64_t b = (uint64_t)__double_as_longlong(v);
  if ((b << 1) == 0) b = 0;  // -0.0 ranks as +0.0
  return (b >> 63) ? ~b : (b ^ 0x8000000000000000ull);
}

// bit p set: pass p moves the column (its keys do not all share digit p)
__device__ inline unsigned live_passes(uint64_t key_or, uint64_t key_and) {
  const uint64_t diff = key_or ^ key_and;
  unsigned m = 0;
#pragma unroll
  for (int p = 0; p < PASSES; ++p) m |= ((diff >> (8 * p)) & 0xff) ? (1u << p) : 0u;
  return m;
}
// the ping-pong side (0 / 1) that holds the column before pass p (p = PASSES: after the sort)
__device__ inline int side_before(unsigned live, int p) { return __popc(live & ((1u << p) - 1u)) & 1; }

__device__ inline uint64_t wave_or(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
  return v;
}
__device__ inline uint64_t wave_and(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v &= (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
  return v;
}

// columns [c0, c0 + nc) of X (n rows, ldx) -> K[c][r] keys, I[c][r] = r (column-major, stride n);
// key_or / key_and (nc each, preset to 0 / ~0) gather the columns' keys; *flag |= 1 on inf / nan
__global__ void __launch_bounds__(NTHREADS)
corr_keys_kernel(const double* __restrict__ X, int64_t n, int64_t ldx, int64_t c0, int64_t nc,
                 uint64_t* __restrict__ K, uint32_t* __restrict__ I, unsigned long long* __restrict__ key_or,
                 unsigned long long* __restrict__ key_and, int* __restrict__ flag) {
  __shared__ uint64_t tile[RT][RT + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * RT, cb = (int64_t)blockIdx.y * RT;
  int bad = 0;
  for (int rr = w; rr < RT; rr += WAVES) {
    const int64_t r = r0 + rr, c = cb + lane;
    uint64_t k = 0;
    if (r < n && c < nc) {
      const double v = X[r * ldx + c0 + c];
      bad |= std::isfinite(v) ? 0 : 1;
      k = key_of(v);
    }
    tile[rr][lane] = k;
  }
  __syncthreads();
  for (int cc = w; cc < RT; cc += WAVES) {
    const int64_t c = cb + cc, r = r0 + lane;
    if (c >= nc) break;
    const bool valid = r < n;
    const uint64_t k = tile[lane][cc];
    if (valid) {
      K[c * n + r] = k;
      I[c * n + r] = (uint32_t)r;
    }
    const uint64_t o = wave_or(valid ? k : 0), a = wave_and(valid ? k : ~0ull);
    if (lane == 0) {
      atomicOr(&key_or[c], (unsigned long long)o);
      atomicAnd(&key_and[c], (unsigned long long)a);
    }
  }
  if (__any(bad) && lane == 0) atomicOr(flag, 1);
}

// H[(c 256 + digit) S + s] = keys of column c's segment s with that digit in pass `pass`
__global__ void __launch_bounds__(NTHREADS)
corr_hist_kernel(const uint64_t* __restrict__ K0, const uint64_t* __restrict__ K1, int64_t n, int64_t S, int pass,
                 const unsigned long long* __restrict__ key_or, const unsigned long long* __restrict__ key_and,
                 uint32_t* __restrict__ H) {
  __shared__ uint32_t h[WAVES][RADIX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t c = blockIdx.y, s = (int64_t)blockIdx.x * WAVES + w;
  const unsigned live = live_passes(key_or[c], key_and[c]);
  if (!((live >> pass) & 1u)) return;
  for (int j = lane; j < RADIX; j += 64) h[w][j] = 0;
  __syncthreads();
  if (s < S) {
    const uint64_t* src = (side_before(live, pass) ? K1 : K0) + c * n;
    const int64_t i1 = std::min<int64_t>(n, (s + 1) * SEG);
    for (int64_t i = s * SEG + lane; i < i1; i += 64) atomicAdd(&h[w][(src[i] >> (8 * pass)) & 0xff], 1u);
  }
  __syncthreads();
  if (s < S)
    for (int j = lane; j < RADIX; j += 64) H[(c * RADIX + j) * S + s] = h[w][j];
}

// column c's counts -> exclusive prefix sums in (digit, segment) order; one workgroup a column
__global__ void __launch_bounds__(RADIX)
corr_scan_kernel(int64_t S, int pass, const unsigned long long* __restrict__ key_or,
                 const unsigned long long* __restrict__ key_and, uint32_t* __restrict__ H) {
  __shared__ uint32_t tot[RADIX];
  const int64_t c = blockIdx.x;
  const int t = threadIdx.x;
  if (!((live_passes(key_or[c], key_and[c]) >> pass) & 1u)) return;
  uint32_t* row = H + (c * RADIX + t) * S;
  uint32_t sum = 0;
  for (int64_t s = 0; s < S; ++s) sum += row[s];
  tot[t] = sum;
  __syncthreads();
  uint32_t run = 0;
  for (int j = 0; j < t; ++j) run += tot[j];
  for (int64_t s = 0; s < S; ++s) {
    const uint32_t v = row[s];
    row[s] = run;
    run += v;
  }
}

// the stable scatter of pass `pass`: a wave walks its segment in order, 64 keys a round; equal
// digits of a round are ranked by lane (8 ballots), rounds by the wave's LDS offsets
__global__ void __launch_bounds__(NTHREADS)
corr_scatter_kernel(uint64_t* __restrict__ K0, uint64_t* __restrict__ K1, uint32_t* __restrict__ I0,
                    uint32_t* __restrict__ I1, int64_t n, int64_t S, int pass,
                    const unsigned long long* __restrict__ key_or, const unsigned long long* __restrict__ key_and,
                    const uint32_t* __restrict__ H) {
  __shared__ uint32_t off[WAVES][RADIX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t c = blockIdx.y, s = (int64_t)blockIdx.x * WAVES + w;
  const unsigned live = live_passes(key_or[c], key_and[c]);
  if (!((live >> pass) & 1u) || s >= S) return;  // (no workgroup barrier below: the waves are independent)
  const int side = side_before(live, pass);
  const uint64_t* srcK = (side ? K1 : K0) + c * n;
  const uint32_t* srcI = (side ? I1 : I0) + c * n;
  uint64_t* dstK = (side ? K0 : K1) + c * n;
  uint32_t* dstI = (side ? I0 : I1) + c * n;
  for (int j = lane; j < RADIX; j += 64) off[w][j] = H[(c * RADIX + j) * S + s];
  __builtin_amdgcn_wave_barrier();
  const int64_t i1 = std::min<int64_t>(n, (s + 1) * SEG);
  const uint64_t below = (1ull << lane) - 1ull;
  for (int64_t i0 = s * SEG; i0 < i1; i0 += 64) {
    const int64_t i = i0 + lane;
    const bool valid = i < i1;
    const uint64_t k = valid ? srcK[i] : 0;
    const uint32_t id = valid ? srcI[i] : 0;
    const unsigned dg = (unsigned)(k >> (8 * pass)) & 0xffu;
    uint64_t same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (dg >> b) & 1u;
      const uint64_t bal = __ballot(valid && bit);
      same &= bit ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(same & below), cnt = (uint32_t)__popcll(same);
    uint32_t base = 0;
    if (valid) base = off[w][dg];
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) off[w][dg] = base + cnt;
    __builtin_amdgcn_wave_barrier();
    const int64_t pos = (int64_t)base + rank;
    if (valid && pos < n) {
      dstK[pos] = k;
      dstI[pos] = id;
    }
  }
}

__device__ inline int64_t lower_bound_key(const uint64_t* K, int64_t lo, int64_t hi, uint64_t k) {
  while (lo < hi) {  // first index in [lo, hi) with K >= k, else hi
    const int64_t mid = lo + (hi - lo) / 2;
    if (K[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ inline int64_t upper_bound_key(const uint64_t* K, int64_t lo, int64_t hi, uint64_t k) {
  while (lo < hi) {  // first index in [lo, hi) with K > k, else hi
    const int64_t mid = lo + (hi - lo) / 2;
    if (K[mid] <= k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the sorted column's tie runs [lo, hi) -> rank (lo + hi + 1) / 2 of every member, written at its
// row in the column's free key buffer (a column-major image of R)
__global__ void __launch_bounds__(NTHREADS)
corr_tie_kernel(uint64_t* __restrict__ K0, uint64_t* __restrict__ K1, const uint32_t* __restrict__ I0,
                const uint32_t* __restrict__ I1, int64_t n, const unsigned long long* __restrict__ key_or,
                const unsigned long long* __restrict__ key_and) {
  const int lane = threadIdx.x & 63;
  const int64_t c = blockIdx.y, i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  const int side = side_before(live_passes(key_or[c], key_and[c]), PASSES);
  const uint64_t* K = (side ? K1 : K0) + c * n;
  const uint32_t* I = (side ? I1 : I0) + c * n;
  double* img = reinterpret_cast<double*>((side ? K0 : K1) + c * n);
  const bool valid = i < n;
  const uint64_t k = valid ? K[i] : 0;
  const bool head = valid && (i == 0 || K[i - 1] != k);
  const bool tail = valid && (i == n - 1 || K[i + 1] != k);
  const uint64_t hb = __ballot(head), tb = __ballot(tail);
  if (!valid) return;
  const int64_t wbase = i - lane;
  const uint64_t upto = hb & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
  const uint64_t from = tb & ~((1ull << lane) - 1ull);
  // (no head at or below this lane: the run began before the wave's positions; no tail at or
  // above: all 64 positions are valid and the run goes on behind them)
  const int64_t lo = upto ? wbase + (63 - __clzll((long long)upto)) : lower_bound_key(K, 0, wbase, k);
  const int64_t hi = from ? wbase + (__ffsll((unsigned long long)from) - 1) + 1
                          : upper_bound_key(K, std::min<int64_t>(n, wbase + 64), n, k);
  const uint32_t row = I[i];
  if (row < (uint64_t)n) img[row] = (double)(lo + hi + 1) * 0.5;
}

// the chunk's column-major rank images -> R[r, c0 + c] (ldr) by tiles
__global__ void __launch_bounds__(NTHREADS)
corr_ranks_out_kernel(const uint64_t* __restrict__ K0, const uint64_t* __restrict__ K1, int64_t n, int64_t c0,
                      int64_t nc, const unsigned long long* __restrict__ key_or,
                      const unsigned long long* __restrict__ key_and, double* __restrict__ R, int64_t ldr) {
  __shared__ double tile[RT][RT + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * RT, cb = (int64_t)blockIdx.y * RT;
  for (int cc = w; cc < RT; cc += WAVES) {
    const int64_t c = cb + cc, r = r0 + lane;
    double v = 0.0;
    if (c < nc && r < n) {
      const int side = side_before(live_passes(key_or[c], key_and[c]), PASSES);
      v = reinterpret_cast<const double*>((side ? K0 : K1) + c * n)[r];
    }
    tile[cc][lane] = v;
  }
  __syncthreads();
  for (int rr = w; rr < RT; rr += WAVES) {
    const int64_t r = r0 + rr, c = cb + lane;
    if (r < n && c < nc) R[r * ldr + c0 + c] = tile[lane][rr];
  }
}

// the sorted payloads of segment c -> order[c n + i] and, with inverse, inverse[c n + payload] = i
__global__ void __launch_bounds__(NTHREADS)
corr_payload_out_kernel(const uint32_t* __restrict__ I0, const uint32_t* __restrict__ I1, int64_t n,
                        const unsigned long long* __restrict__ key_or, const unsigned long long* __restrict__ key_and,
                        int32_t* __restrict__ order, int32_t* __restrict__ inverse) {
  const int64_t c = blockIdx.y, i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= n) return;
  const int side = side_before(live_passes(key_or[c], key_and[c]), PASSES);
  const uint32_t row = ((side ? I1 : I0) + c * n)[i];
  order[c * n + i] = (int32_t)row;
  if (inverse && row < (uint64_t)n) inverse[c * n + row] = (int32_t)i;
}

// --- correlations ------------------------------------------------------------------------------
constexpr int CS_COLS = 64;

// per column j and part p = blockIdx.y * 4 + wave: the sum, min and max of X[r, j] over the
// workgroup's rows r = r0 + wave, r0 + wave + 4, ... (colsum_part_kernel's order); *flag on inf / nan
__global__ void __launch_bounds__(NTHREADS)
corr_colstat_part_kernel(const double* __restrict__ X, int64_t n, int64_t d, int64_t ldx, int64_t rows_per,
                         double* __restrict__ psum, double* __restrict__ pmin, double* __restrict__ pmax,
                         int* __restrict__ flag) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * CS_COLS + lane;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per;
  const int64_t r1 = std::min<int64_t>(n, r0 + rows_per);
  int bad = 0;
  if (j < d) {
    double acc = 0.0, mn = std::numeric_limits<double>::infinity(), mx = -mn;
#pragma unroll 8
    for (int64_t r = r0 + wave; r < r1; r += WAVES) {
      const double v = X[r * ldx + j];
      bad |= std::isfinite(v) ? 0 : 1;
      acc += v;
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
    }
    const int64_t p = ((int64_t)blockIdx.y * WAVES + wave) * d + j;
    psum[p] = acc, pmin[p] = mn, pmax[p] = mx;
  }
  if (__any(bad) && lane == 0) atomicOr(flag, 1);
}

// stat[j], stat[d + j], stat[2 d + j] = the column's sum (ascending parts), min, max
__global__ void corr_colstat_final_kernel(const double* __restrict__ psum, const double* __restrict__ pmin,
                                          const double* __restrict__ pmax, int64_t np, int64_t d,
                                          double* __restrict__ stat) {
  const int64_t j = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (j >= d) return;
  double acc = 0.0, mn = std::numeric_limits<double>::infinity(), mx = -mn;
  for (int64_t p = 0; p < np; ++p) {
    acc += psum[p * d + j];
    mn = pmin[p * d + j] < mn ? pmin[p * d + j] : mn;
    mx = pmax[p * d + j] > mx ? pmax[p * d + j] : mx;
  }
  stat[j] = acc, stat[d + j] = mn, stat[2 * d + j] = mx;
}

// S[r, c] (ld D) = X[r, c] - colsum[c] / nrows for r < rows, c < d; 0 elsewhere in the rpad x D chunk
__global__ void corr_stage_centred_kernel(const double* __restrict__ X, int64_t ldx, int64_t rows, int64_t d,
                                          const double* __restrict__ colsum, double nrows, double* __restrict__ S,
                                          int64_t D, int64_t rpad) {
  const int64_t c = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (c >= D) return;
  const double mean = c < d ? colsum[c] / nrows : 0.0;
  for (int64_t r = blockIdx.y; r < rpad; r += gridDim.y) S[r * D + c] = (r < rows && c < d) ? X[r * ldx + c] - mean : 0.0;
}

// Rho (d x d, ldrho) from the Gram G (ld D) of the centred columns; is_const[c] = 1 for max == min
__global__ void corr_normalise_kernel(const double* __restrict__ G, int64_t D, int64_t d,
                                      const double* __restrict__ stat, double* __restrict__ Rho, int64_t ldrho,
                                      int32_t* __restrict__ is_const) {
  const int64_t j = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (j >= d) return;
  const bool cj = stat[d + j] == stat[2 * d + j];
  const double gjj = G[j * D + j];
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t i = blockIdx.y; i < d; i += gridDim.y) {
    const bool ci = stat[d + i] == stat[2 * d + i];
    double v;
    if (ci || cj) {
      v = nan;
    } else if (i == j) {
      v = 1.0;
    } else {
      v = G[i * D + j] / std::sqrt(G[i * D + i] * gjj);
      v = v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v);
    }
    Rho[i * ldrho + j] = v;
  }
  if (blockIdx.y == 0) is_const[j] = cj ? 1 : 0;
}

// --- plans (host) ------------------------------------------------------------------------------
bool shape_ok(int64_t n, int64_t d) { return n >= 2 && n < (int64_t(1) << 31) && d >= 1 && d <= 65535; }

struct RankPlan {
  int64_t S, cols, key_count, idx_count, hist_count, bytes;
};
RankPlan rank_plan(int64_t n, int64_t d, int64_t budget) {
  RankPlan p;
  if (budget <= 0) budget = kDefaultBudget;
  p.S = (n + SEG - 1) / SEG;
  const int64_t per_col = 2 * n * 8 + 2 * n * 4 + RADIX * p.S * 4 + 16;
  p.cols = std::max<int64_t>(1, std::min<int64_t>(d, budget / per_col));
  if (p.cols >= 32) p.cols = p.cols / 16 * 16;  // (whole 128-byte lines of X's rows, except in the last chunk)
  p.key_count = 2 * p.cols * n;
  p.idx_count = 2 * p.cols * n;
  p.hist_count = p.cols * RADIX * p.S;
  p.bytes = p.key_count * 8 + p.idx_count * 4 + p.hist_count * 4 + p.cols * 16 + 8;
  return p;
}

struct CorrPlan {
  GramPlan g;
  int64_t parts, bytes;
};
CorrPlan corr_plan(int64_t n, int64_t d, int64_t budget) {
  CorrPlan p;
  if (budget <= 0) budget = kDefaultBudget;
  const int64_t D = (d + 127) / 128 * 128;
  const GramPlan shape = gram_plan(n, d, 256);  // (the split does not depend on the chunk rows)
  const int64_t zbytes = (int64_t)(shape.split + 2) * D * D * 8;
  p.g = gram_plan(n, d, std::max<int64_t>(256, (budget - zbytes) / (D * 8)));
  p.parts = colsum_parts(n);
  p.bytes = p.g.chunk * D * 8 + zbytes + 3 * p.parts * d * 8 + 3 * d * 8 + 8;
  return p;
}

unsigned row_blocks(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(rows, 4096)); }

const char* bad_args(const void* X, int64_t n, int64_t d, int64_t ldx, const void* out, int64_t ldo) {
  if (!X || !out) return "null pointer";
  if (!shape_ok(n, d)) return "need 2 <= n < 2^31 rows and 1 <= d <= 65535 columns";
  if (ldx < d || ldo < d) return "a leading dimension is below d";
  return nullptr;
}

}  // namespace

namespace midagma {

int64_t segsort_hist_per_segment(int64_t n) { return RADIX * ((n + SEG - 1) / SEG); }

void launch_segsort(const SegSort& s, int64_t n, int64_t nseg, hipStream_t st) {
  const int64_t S = (n + SEG - 1) / SEG;
  const dim3 segs((unsigned)((S + WAVES - 1) / WAVES), (unsigned)nseg);
  for (int pass = 0; pass < PASSES; ++pass) {
    hipLaunchKernelGGL(corr_hist_kernel, segs, dim3(NTHREADS), 0, st, s.K0, s.K1, n, S, pass, s.key_or, s.key_and,
                       s.hist);
    hipLaunchKernelGGL(corr_scan_kernel, dim3((unsigned)nseg), dim3(RADIX), 0, st, S, pass, s.key_or, s.key_and,
                       s.hist);
    hipLaunchKernelGGL(corr_scatter_kernel, segs, dim3(NTHREADS), 0, st, s.K0, s.K1, s.I0, s.I1, n, S, pass, s.key_or,
                       s.key_and, s.hist);
    HIP_TRY(hipGetLastError());
  }
}

void launch_segsort_payload(const SegSort& s, int64_t n, int64_t nseg, int32_t* order, int32_t* inverse,
                            hipStream_t st) {
  hipLaunchKernelGGL(corr_payload_out_kernel, dim3((unsigned)((n + NTHREADS - 1) / NTHREADS), (unsigned)nseg),
                     dim3(NTHREADS), 0, st, s.I0, s.I1, n, s.key_or, s.key_and, order, inverse);
  HIP_TRY(hipGetLastError());
}

}  // namespace midagma

namespace {

// The columns of X sorted by value, a chunk of the plan's columns at a time: the scratch, the keys
// kernel and the radix passes of each chunk, then after(s, c0, nc, tiles) on the chunk's sorted keys
// and payloads.  Synchronises st (the scratch is freed on return); inf or nan in X throws, with
// `who` in front of the message.
template <class After>
void sorted_columns(const double* X_dev, int64_t n, int64_t d, int64_t ldx, int64_t budget_bytes, hipStream_t st,
                    const char* who, After&& after) {
  const RankPlan p = rank_plan(n, d, budget_bytes);
  DevBuf<uint64_t> keys;
  DevBuf<uint32_t> idx, hist;
  DevBuf<unsigned long long> oa;
  DevBuf<int> fl;
  keys.alloc((size_t)p.key_count);
  idx.alloc((size_t)p.idx_count);
  hist.alloc((size_t)p.hist_count);
  oa.alloc((size_t)(2 * p.cols));
  fl.alloc(1);
  flag_clear(fl.p, st);
  const int64_t half = p.cols * n;
  const SegSort s{keys.p, keys.p + half, idx.p, idx.p + half, oa.p, oa.p + p.cols, hist.p};
  for (int64_t c0 = 0; c0 < d; c0 += p.cols) {
    const int64_t nc = std::min(p.cols, d - c0);
    HIP_TRY(hipMemsetAsync(s.key_or, 0, (size_t)nc * 8, st));
    HIP_TRY(hipMemsetAsync(s.key_and, 0xff, (size_t)nc * 8, st));
    const dim3 tiles((unsigned)((n + RT - 1) / RT), (unsigned)((nc + RT - 1) / RT));
    hipLaunchKernelGGL(corr_keys_kernel, tiles, dim3(NTHREADS), 0, st, X_dev, n, ldx, c0, nc, s.K0, s.I0, s.key_or,
                       s.key_and, fl.p);
    HIP_TRY(hipGetLastError());
    launch_segsort(s, n, nc, st);
    after(s, c0, nc, tiles);
  }
  flag_check(fl.p, st, std::string(who) + kNonFinite);
}

}  // namespace

void midagma::colargsort_run(const double* X_dev, int64_t n, int64_t d, int64_t ldx, int32_t* order_dev,
                             int64_t budget_bytes, hipStream_t st) {
  sorted_columns(X_dev, n, d, ldx, budget_bytes, st, "colargsort: ",
                 [&](const SegSort& s, int64_t c0, int64_t nc, dim3) {
                   launch_segsort_payload(s, n, nc, order_dev + c0 * n, nullptr, st);
                 });
}

extern "C" int midagma_colargsort(const double* X_dev, int64_t n, int64_t d, int64_t ldx, int32_t* order_dev,
                                  int64_t budget_bytes, void* stream) {
  if (const char* why = bad_args(X_dev, n, d, ldx, order_dev, d))
    return abi_fail(nullptr, MIDAGMA_E_ARG, std::string("colargsort: ") + why);
  return abi_guarded(nullptr, [&] {
    colargsort_run(X_dev, n, d, ldx, order_dev, budget_bytes, reinterpret_cast<hipStream_t>(stream));
    return MIDAGMA_OK;
  });
}

extern "C" int64_t midagma_corr_workspace(int64_t n, int64_t d, int64_t budget_bytes) {
  if (!shape_ok(n, d)) return 0;
  return std::max(rank_plan(n, d, budget_bytes).bytes, corr_plan(n, d, budget_bytes).bytes);
}

extern "C" int midagma_colrank(const double* X_dev, int64_t n, int64_t d, int64_t ldx, double* R_dev, int64_t ldr,
                               int64_t budget_bytes, void* stream) {
  if (const char* why = bad_args(X_dev, n, d, ldx, R_dev, ldr))
    return abi_fail(nullptr, MIDAGMA_E_ARG, std::string("colrank: ") + why);
  return abi_guarded(nullptr, [&] {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto ranks_out = [&](const SegSort& s, int64_t c0, int64_t nc, dim3 tiles) {
      hipLaunchKernelGGL(corr_tie_kernel, dim3((unsigned)((n + NTHREADS - 1) / NTHREADS), (unsigned)nc),
                         dim3(NTHREADS), 0, st, s.K0, s.K1, s.I0, s.I1, n, s.key_or, s.key_and);
      hipLaunchKernelGGL(corr_ranks_out_kernel, tiles, dim3(NTHREADS), 0, st, s.K0, s.K1, n, c0, nc, s.key_or,
                         s.key_and, R_dev, ldr);
      HIP_TRY(hipGetLastError());
    };
    sorted_columns(X_dev, n, d, ldx, budget_bytes, st, "colrank: ", ranks_out);
  });
}

extern "C" int midagma_corr(const double* X_dev, int64_t n, int64_t d, int64_t ldx, double* Rho_dev, int64_t ldrho,
                            int32_t* const_col_dev, int64_t budget_bytes, void* stream) {
  if (const char* why = bad_args(X_dev, n, d, ldx, Rho_dev, ldrho))
    return abi_fail(nullptr, MIDAGMA_E_ARG, std::string("corr: ") + why);
  if (!const_col_dev) return abi_fail(nullptr, MIDAGMA_E_ARG, "corr: null pointer");
  return abi_guarded(nullptr, [&] {
    setup_attributes();
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const CorrPlan p = corr_plan(n, d, budget_bytes);
    const int64_t D = p.g.D, DD = D * D;
    DevBuf<> part, stat, S, Z;
    DevBuf<int> fl;
    part.alloc((size_t)(3 * p.parts * d));
    stat.alloc((size_t)(3 * d));
    fl.alloc(1);
    flag_clear(fl.p, st);
    // the column pass, in launch_colsum's partition of the rows
    const int64_t groups = p.parts / WAVES;
    const int64_t rows_per = std::max<int64_t>(1, (n + groups - 1) / groups);
    const int64_t used = std::max<int64_t>(1, (n + rows_per - 1) / rows_per);
    double *psum = part.p, *pmin = part.p + p.parts * d, *pmax = part.p + 2 * p.parts * d;
    hipLaunchKernelGGL(corr_colstat_part_kernel, dim3((unsigned)((d + CS_COLS - 1) / CS_COLS), (unsigned)used),
                       dim3(NTHREADS), 0, st, X_dev, n, d, ldx, rows_per, psum, pmin, pmax, fl.p);
    hipLaunchKernelGGL(corr_colstat_final_kernel, dim3((unsigned)((d + NTHREADS - 1) / NTHREADS)), dim3(NTHREADS), 0,
                       st, psum, pmin, pmax, used * WAVES, d, stat.p);
    HIP_TRY(hipGetLastError());
    flag_check(fl.p, st, std::string("corr: ") + kNonFinite);
    // the Gram of the centred columns: midagma_gram's chunk loop on a centred staging copy
    S.alloc((size_t)(p.g.chunk * D));
    Z.alloc((size_t)((p.g.split + 2) * DD));  // [0] the running sum, [1..split] a chunk's slices, [split+1] the new sum
    HIP_TRY(hipMemsetAsync(Z.p, 0, DD * sizeof(double), st));
    const dim3 colgrid((unsigned)((D + NTHREADS - 1) / NTHREADS));
    for (int64_t c = 0; c < p.g.nchunks; ++c) {
      const int64_t r0 = c * p.g.chunk, rows = std::min(p.g.chunk, n - r0);
      const int64_t rpad = (rows + 255) / 256 * 256;
      hipLaunchKernelGGL(corr_stage_centred_kernel, dim3(colgrid.x, row_blocks(rpad)), dim3(NTHREADS), 0, st,
                         X_dev + r0 * ldx, ldx, rows, d, stat.p, (double)n, S.p, D, rpad);
      HIP_TRY(hipGetLastError());
      launch_gemm(GemmSpec{D, D, rpad, S.p, D, true, S.p, D, B_PLAIN, Z.p + DD, D, p.g.split, DD}, nullptr, st);
      launch_sum_slices(Z.p, p.g.split + 1, DD, DD, Z.p + (p.g.split + 1) * DD, nullptr, st);
      HIP_TRY(hipMemcpyAsync(Z.p, Z.p + (p.g.split + 1) * DD, DD * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(corr_normalise_kernel, dim3((unsigned)((d + NTHREADS - 1) / NTHREADS), row_blocks(d)),
                       dim3(NTHREADS), 0, st, Z.p, D, d, stat.p, Rho_dev, ldrho, const_col_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));  // (the scratch is freed on return)
    return MIDAGMA_OK;
  });
}
