// The owner-tile layer of the one-workgroup small-d kernels (small.hip's slot loop, small_eval.hip's
// evaluation kernels, the pst_blk.h and logit_blk.h bodies): a DS x DS problem (DS = 16, 32, 64) on
// DS * DS / 256 waves, one 16 x 16 tile of the f64 16x16x4 MFMA accumulator map per wave, so every
// product's output lands in the registers of the lane that owns the element.  Wave w owns the tile
// (w / (DS/16), w % (DS/16)); lane l owns column 16 tc + (l & 15), rows 16 tr + (l >> 4) + 4 t for
// t = 0..3.  Here: that map, the LDS image strides, the tile product, the wave reductions, the
// unpivoted Gauss-Jordan on the map and the image writes.  small.hip's slot kernel takes the tile
// product, the reductions and cpos from here but keeps its own map set-up, Gauss-Jordan (with the
// pivots kept) and image writes (its file head says why), so those helpers carry only what their
// callers, pst_blk.h and small_eval.hip, use.
#pragma once

#include "mfma64.h"

namespace midagma {

template <int DS>
struct WgTile {
  static_assert(DS == 16 || DS == 32 || DS == 64, "one workgroup: d <= 64");
  static constexpr int TPR = DS / 16;                     // tiles per row
  static constexpr int NW = TPR * TPR, NT = 64 * NW;      // waves, threads: one tile per wave
  static constexpr int SW = DS + 2;                       // W, cov, [m][k] images: 16 rows x 4 cols per read
  static constexpr int SI = ((DS + 15) / 32) * 32 + 16;   // I - W, [k][n] images: B operand rows, = 16 mod 32
  int q, c, w;     // lane >> 4, lane & 15, the wave
  int row0, col0;  // the wave's tile
  int cj;          // the lane's column
  int ri[4];       // the lane's rows
  bool real[4];    // inside d x d
  __device__ __forceinline__ WgTile(int tid, int di) {
    const int lane = tid & 63;
    q = lane >> 4;
    c = lane & 15;
    w = tid >> 6;
    row0 = 16 * (w / TPR);
    col0 = 16 * (w % TPR);
    cj = col0 + c;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      ri[t] = row0 + q + 4 * t;
      real[t] = ri[t] < di && cj < di;
    }
  }
};

__device__ __forceinline__ double wave_sum(double x) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}
__device__ __forceinline__ double wave_max(double x) {
  for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off));
  return x;
}
__device__ __forceinline__ double wave_min(double x) {
  for (int off = 32; off > 0; off >>= 1) x = fmin(x, __shfl_xor(x, off));
  return x;
}

// acc += A[row0 .. row0+15][0 .. kd) * B[0 .. kd)[col0 .. col0+15] on the f64 16x16x4 MFMA;
// A from an [m][k] image (stride SA_), B from a [k][n] image (stride SB_).  Terms with
// k >= d are exact zeros in every product of the small-d kernels (zero off-diagonal padding).
template <int DS, int SA_, int SB_>
__device__ __forceinline__ dbl4 tile_mma(const double* __restrict__ A, const double* __restrict__ B, int row0,
                                         int col0, int q, int c, int kd, dbl4 acc) {
  if (DS >= 64) {  // (a full unroll keeps 32 operands in flight: the 1024-thread kernel's registers spill)
#pragma unroll 4
    for (int kk = 0; 4 * kk < kd; ++kk)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(row0 + c) * SA_ + 4 * kk + q], B[(4 * kk + q) * SB_ + col0 + c],
                                                 acc, 0, 0, 0);
    return acc;
  }
  // DS <= 32: all DS / 4 k-steps, unguarded (the k >= d terms are the exact zeros above): the
  // operand reads of a branch-free unrolled chain issue together, where a guard per k-step
  // serialised read, wait and MFMA (d = 20: 5 guarded steps cost more than 8 pipelined ones)
  (void)kd;
#pragma unroll
  for (int kk = 0; kk < DS / 4; ++kk)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(row0 + c) * SA_ + 4 * kk + q], B[(4 * kk + q) * SB_ + col0 + c],
                                               acc, 0, 0, 0);
  return acc;
}
// ... of this lane's tile, from zero
template <int DS, int SA_, int SB_>
__device__ __forceinline__ dbl4 tile_mma(const double* __restrict__ A, const double* __restrict__ B,
                                         const WgTile<DS>& T, int kd) {
  return tile_mma<DS, SA_, SB_>(A, B, T.row0, T.col0, T.q, T.c, kd, dbl4{0.0, 0.0, 0.0, 0.0});
}

// colb position of row i: the 4 rows a lane owns (16 tr + q + 4 t) are 4 consecutive slots
__device__ __forceinline__ int cpos(int i) { return (i & ~15) + 4 * (i & 3) + ((i & 15) >> 2); }

// a <- inv(a) on the owner map (a: this lane's four elements, identity outside d x d): in-place
// Gauss-Jordan, no pivoting, d steps of one barrier each.  rowb / colb: the pivot row and column,
// double-buffered (2 x DS doubles each, 32-byte aligned: a lane reads its four column words at
// once).  The pivots are not kept.  Every thread of the workgroup calls it.
template <int DS>
__device__ __forceinline__ void wg_gauss_jordan(double (&a)[4], const WgTile<DS>& T, int di,
                                                double* __restrict__ rowb, double* __restrict__ colb) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (T.ri[t] == 0) rowb[T.cj] = a[t];
    if (T.cj == 0) colb[cpos(T.ri[t])] = a[t];
  }
  __syncthreads();
  for (int k = 0; k < di; ++k) {
    const int b = k & 1;
    const double p = rowb[b * DS + k];
    const double pinv = 1.0 / p;
    const int j = T.cj;
    const double rk = rowb[b * DS + j] * pinv;
    const double4 ck = *reinterpret_cast<const double4*>(&colb[b * DS + T.row0 + 4 * T.q]);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (!T.real[t]) continue;
      const int i = T.ri[t];
      const double cki = t == 0 ? ck.x : (t == 1 ? ck.y : (t == 2 ? ck.z : ck.w));
      if (i == k)
        a[t] = (j == k) ? pinv : a[t] * pinv;
      else if (j == k)
        a[t] = -(a[t] * pinv);
      else
        a[t] = a[t] - cki * rk;
    }
    if (k + 1 < di) {
      const int b1 = b ^ 1;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (T.ri[t] == k + 1) rowb[b1 * DS + T.cj] = a[t];
        if (T.cj == k + 1) colb[b1 * DS + cpos(T.ri[t])] = a[t];
      }
    }
    __syncthreads();
  }
}

// This lane's four (float64) W words into the images: the diagonal (wdiag) and I - W (IWimg, stride
// SI).  Words outside d x d stay as they are (zero).
template <int DS>
__device__ __forceinline__ void wg_store_w(const WgTile<DS>& T, const double (&wv)[4], double* __restrict__ wdiag,
                                           double* __restrict__ IWimg) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (T.real[t]) {
      if (T.ri[t] == T.cj) wdiag[T.ri[t]] = wv[t];
      IWimg[T.ri[t] * WgTile<DS>::SI + T.cj] = one_minus(T.ri[t] == T.cj, wv[t], false);
    }
}

// A d x d matrix (leading dimension d) as a dense DS x DS image, zero outside d x d
template <int DS>
__device__ __forceinline__ void wg_load_dense(double* __restrict__ img, const double* __restrict__ src, int di) {
  for (int e = threadIdx.x; e < DS * DS; e += WgTile<DS>::NT) {
    const int r = e / DS, k = e % DS;
    img[e] = (r < di && k < di) ? src[r * di + k] : 0.0;
  }
}

}  // namespace midagma
