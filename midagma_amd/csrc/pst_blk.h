// PST trek regularizer (trek.hip) for d <= 32 in ONE workgroup: the device
// body the small-d persistent inner loop (small.hip) runs inside its slots and the evaluation
// kernel (small_eval.hip) runs once, on the caller's workgroup, its element ownership and its
// primitives (wgtile.h: the owner map, tile_mma, the wave reductions, the Gauss-Jordan).
//
//     W2 = W o W,  F = f(W2),  H = F^T F,  value = agg(H[i_p, j_p]),
//     C = d value / d H,  G_F = F (C + C^T),  grad = 2 W o L_f(W2, G_F^T)^T
//
// exp: trek_scale_kernel's rule (s squarings, X = 2^-s W2, Taylor degree TREK_TAYLOR_M by Horner).
// trek.hip keeps the 12 + s iterates in global buffers for the directional pass; a workgroup has no
// LDS for them, so the recurrence is run twice: pass 1 for F, pass 2 again together with its
// derivative in the one direction E = 2^-s G_F^T
//     L_12 = 0,  L_{k-1} = (X L_k + E Q_k) / k,  Q_{k-1} = I + X Q_k / k;   L <- Q L + L Q, Q <- Q^2
// which costs 12 + s products in pass 1 and 3 (12 + s) in pass 2, each DS^3 on
// v_mfma_f64_16x16x4f64 with the output in its owner's registers.
// inv: F = ((1 + eps) I - W2)^-1 by the slot's unpivoted Gauss-Jordan (wg_gauss_jordan), L = F E F.
//
// The pair list enters as its multiplicity matrix N (N[i][j]: how often (i, j) occurs), so value
// and C are sums over the lane's own elements in a fixed order, with no atomics:
//     mean / sum: sum_ij N_ij H_ij (/ m);  max: max over N_ij > 0;  lse: max + log sum N_ij exp(H_ij - max)
//     C_ij = N_ij c(H_ij),  c = 1/m | 1 | [H_ij = max] / ties | exp(H_ij - value)
// A problem's result therefore does not depend on which other workgroups run beside it.
//
// Images: an [m][k] image (stride SW) is an MFMA A operand, a [k][n] image a B operand (stride SI,
// or SW for the derivative's).  Each step writes its operands to the buffer pair the step before
// did not read, so one barrier a step orders write and read.
#pragma once

#include <cmath>

#include "launch.h"
#include "wgtile.h"

namespace midagma {
namespace pstb {

// the caller's idle buffers: two [m][k] pairs (DS x SW each) and one [k][n] pair (DS x SI each)
// of the product-form inverse, and the Gauss-Jordan pivot row / column pairs (DS each, 32-byte
// aligned) (each pair contiguous: the second half follows the first)
struct PstBufs {
  double* pa;
  double* pr;
  double* pb;
  double* rowb;
  double* colb;
};

// the body's own LDS
template <int DS, int NW>
struct PstLds {
  static constexpr int SW = WgTile<DS>::SW;
  double nimg[DS * DS];    // N, zero outside d x d (loaded by the caller: wg_load_dense)
  double lb[2][DS * SW];   // the derivative's [k][n] images; H and the result for transposed reads
  double colsum[DS];
  double red[4][NW];
  double val;              // the value of the last run
};

// d value / d H at one entry, times its multiplicity
__device__ __forceinline__ double coef(int agg, double n, double h, double mx, double value, double base) {
  if (!(n > 0.0)) return 0.0;
  if (agg == TREK_MAX) return h == mx ? n * base : 0.0;
  if (agg == TREK_LSE) return n * exp(h - value);
  return n * base;
}

// The PST penalty of the workgroup's W: wv, this lane's four elements (zero outside d x d), Wimg
// their [i][j] image (stride DS + 2).  Leaves the value in L.val and, with want_grad, this lane's
// elements of d value / d W in g (zero otherwise).  Every thread of the 64 NW calls it
// (barriers inside); ps.m > 0.
template <int DS, int NW>
__device__ __forceinline__ void pst_blk_body(const SmallPst& ps, int di, const double (&wv)[4],
                                             const double* __restrict__ Wimg, const PstBufs& B, PstLds<DS, NW>& L,
                                             bool want_grad, double (&g)[4]) {
  static_assert(DS == 16 || DS == 32, "PST in one workgroup: d <= 32");
  static_assert(NW * 256 == DS * DS, "one 16 x 16 tile per wave");
  constexpr int SW = WgTile<DS>::SW, SI = WgTile<DS>::SI;
  const int tid = threadIdx.x, lane = tid & 63;
  const WgTile<DS> T(tid, di);
  const int w = T.w, cj = T.cj;
  const auto& ri = T.ri;
  const auto& real = T.real;
  double dl[4];  // the identity on d x d
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    dl[t] = real[t] && ri[t] == cj ? 1.0 : 0.0;
    g[t] = 0.0;
  }
  // the halves of the caller's buffer pairs
  const auto pa = [&](int x) { return B.pa + x * (DS * SW); };
  const auto pr = [&](int x) { return B.pr + x * (DS * SW); };
  const auto pb = [&](int x) { return B.pb + x * (DS * SI); };
  const bool is_exp = ps.seq == TREK_EXP;
  int p = 0;  // the buffer pair of the next step
  int s = 0;
  double scal = 1.0;
  double f[4];

  // ---- pass 1: F
  if (is_exp) {
    if (tid < DS) {  // ||W2||_1 by columns, rows in order (trek_w2_kernel)
      double cs = 0.0;
      for (int i = 0; i < di; ++i) {
        const double x = Wimg[i * SW + tid];
        cs += tid < di ? x * x : 0.0;
      }
      L.colsum[tid] = cs;
    }
    __syncthreads();
    const double nrm = wave_max(lane < DS ? L.colsum[lane] : 0.0);
    while (s < TREK_SMAX && nrm / ldexp(1.0, s) > 0.25) ++s;  // trek_scale_kernel
    scal = ldexp(1.0, -s);
    double qk[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double x = real[t] ? (wv[t] * wv[t]) * scal : 0.0;
      pa(0)[ri[t] * SW + cj] = x;
      qk[t] = dl[t];
    }
    for (int k = TREK_TAYLOR_M; k >= 1; --k) {  // Q_{k-1} = I + X Q_k / k
#pragma unroll
      for (int t = 0; t < 4; ++t) pb(p)[ri[t] * SI + cj] = qk[t];
      __syncthreads();
      const dbl4 acc = tile_mma<DS, SW, SI>(pa(0), pb(p), T, di);
      const double rk = 1.0 / k;
#pragma unroll
      for (int t = 0; t < 4; ++t) qk[t] = real[t] ? dl[t] + rk * acc[t] : 0.0;
      p ^= 1;
    }
    for (int u = 0; u < s; ++u) {  // Q <- Q^2
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        pr(p)[ri[t] * SW + cj] = qk[t];
        pb(p)[ri[t] * SI + cj] = qk[t];
      }
      __syncthreads();
      const dbl4 acc = tile_mma<DS, SW, SI>(pr(p), pb(p), T, di);
#pragma unroll
      for (int t = 0; t < 4; ++t) qk[t] = real[t] ? acc[t] : 0.0;
      p ^= 1;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) f[t] = qk[t];
  } else {
    // F = ((1 + eps) I - W2)^-1: the slot's in-place Gauss-Jordan, no pivots kept
    const double sd = 1.0 + ps.eps_inv;
    double a[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      a[t] = real[t] ? sw_entry(ri[t] == cj, sd, wv[t], false) : (ri[t] == cj ? 1.0 : 0.0);
    wg_gauss_jordan<DS>(a, T, di, B.rowb, B.colb);
#pragma unroll
    for (int t = 0; t < 4; ++t) f[t] = real[t] ? a[t] : 0.0;
  }

  // ---- H = F^T F
  double h[4];
  {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      pr(p)[cj * SW + ri[t]] = f[t];
      pb(p)[ri[t] * SI + cj] = f[t];
    }
    __syncthreads();
    const dbl4 acc = tile_mma<DS, SW, SI>(pr(p), pb(p), T, di);
#pragma unroll
    for (int t = 0; t < 4; ++t) h[t] = real[t] ? acc[t] : 0.0;
    p ^= 1;
  }

  // ---- value = agg over the pairs, and C + C^T
  double nn[4];
  double sum = 0.0, mx = -INFINITY;
  {
    double ps_ = 0.0, pm = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      nn[t] = L.nimg[ri[t] * DS + cj];
      L.lb[0][ri[t] * SW + cj] = h[t];
      if (nn[t] > 0.0) {
        ps_ += nn[t] * h[t];
        pm = fmax(pm, h[t]);
      }
    }
    ps_ = wave_sum(ps_);
    pm = wave_max(pm);
    if (lane == 0) {
      L.red[0][w] = ps_;
      L.red[1][w] = pm;
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < NW; ++x) {
      sum += L.red[0][x];
      mx = fmax(mx, L.red[1][x]);
    }
  }
  double value = sum, base = 1.0;
  if (ps.agg == TREK_MEAN) {
    value = sum / ps.m;
    base = 1.0 / ps.m;
  } else if (ps.agg >= TREK_MAX) {  // max: the ties share the gradient; lse: c = exp(H - value)
    double se = 0.0, ties = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (nn[t] > 0.0) {
        se += nn[t] * exp(h[t] - mx);
        ties += h[t] == mx ? nn[t] : 0.0;
      }
    se = wave_sum(se);
    ties = wave_sum(ties);
    if (lane == 0) {
      L.red[2][w] = se;
      L.red[3][w] = ties;
    }
    __syncthreads();
    se = 0.0;
    ties = 0.0;
#pragma unroll
    for (int x = 0; x < NW; ++x) {
      se += L.red[2][x];
      ties += L.red[3][x];
    }
    value = ps.agg == TREK_MAX ? mx : mx + log(se);
    base = 1.0 / ties;
  }
  if (tid == 0) L.val = value;
  if (!want_grad) {
    __syncthreads();  // (the caller may rewrite the buffers)
    return;
  }
  double sm[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const double ht = L.lb[0][cj * SW + ri[t]], nt = L.nimg[cj * DS + ri[t]];
    sm[t] = coef(ps.agg, nn[t], h[t], mx, value, base) + coef(ps.agg, nt, ht, mx, value, base);
  }

  // ---- G_F = F (C + C^T);  E = 2^-s G_F^T
  double gf[4];
  const int pf = p;  // F's [m][k] image
  {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      pr(p)[ri[t] * SW + cj] = f[t];
      pb(p)[ri[t] * SI + cj] = sm[t];
    }
    __syncthreads();
    const dbl4 acc = tile_mma<DS, SW, SI>(pr(p), pb(p), T, di);
#pragma unroll
    for (int t = 0; t < 4; ++t) gf[t] = real[t] ? acc[t] : 0.0;
    p ^= 1;
  }

  // ---- pass 2: L = L_f(W2, G_F^T) = G_W2^T
  double lk[4];
  if (is_exp) {
    double qk[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      pa(1)[cj * SW + ri[t]] = scal * gf[t];
      qk[t] = dl[t];
      lk[t] = 0.0;
    }
    for (int k = TREK_TAYLOR_M; k >= 1; --k) {  // L_{k-1} = (X L_k + E Q_k) / k beside Q_{k-1}
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        pb(p)[ri[t] * SI + cj] = qk[t];
        L.lb[p][ri[t] * SW + cj] = lk[t];
      }
      __syncthreads();
      const dbl4 t1 = tile_mma<DS, SW, SW>(pa(0), L.lb[p], T, di);
      const dbl4 t2 = tile_mma<DS, SW, SI>(pa(1), pb(p), T, di);
      const dbl4 tq = tile_mma<DS, SW, SI>(pa(0), pb(p), T, di);
      const double rk = 1.0 / k;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        lk[t] = real[t] ? rk * (t1[t] + t2[t]) : 0.0;
        qk[t] = real[t] ? dl[t] + rk * tq[t] : 0.0;
      }
      p ^= 1;
    }
    if (s > 0) __syncthreads();  // X and E are read no more: their buffers take Q's [m][k] images
    for (int u = 0; u < s; ++u) {  // L <- Q L + L Q, Q <- Q^2
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        pa(p)[ri[t] * SW + cj] = qk[t];
        pb(p)[ri[t] * SI + cj] = qk[t];
        pr(p)[ri[t] * SW + cj] = lk[t];
        L.lb[p][ri[t] * SW + cj] = lk[t];
      }
      __syncthreads();
      const dbl4 t1 = tile_mma<DS, SW, SW>(pa(p), L.lb[p], T, di);
      const dbl4 t2 = tile_mma<DS, SW, SI>(pr(p), pb(p), T, di);
      const dbl4 tq = tile_mma<DS, SW, SI>(pa(p), pb(p), T, di);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        lk[t] = real[t] ? t1[t] + t2[t] : 0.0;
        qk[t] = real[t] ? tq[t] : 0.0;
      }
      p ^= 1;
    }
  } else {
    // L = F E F with E = G_F^T
#pragma unroll
    for (int t = 0; t < 4; ++t) pb(p)[cj * SI + ri[t]] = gf[t];
    __syncthreads();
    const dbl4 t1 = tile_mma<DS, SW, SI>(pr(pf), pb(p), T, di);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      pr(p)[ri[t] * SW + cj] = real[t] ? t1[t] : 0.0;
      pb(p ^ 1)[ri[t] * SI + cj] = f[t];
    }
    __syncthreads();
    const dbl4 t2 = tile_mma<DS, SW, SI>(pr(p), pb(p ^ 1), T, di);
#pragma unroll
    for (int t = 0; t < 4; ++t) lk[t] = real[t] ? t2[t] : 0.0;
  }

  // ---- grad[i][j] = 2 W[i][j] L[j][i]
#pragma unroll
  for (int t = 0; t < 4; ++t) L.lb[p][ri[t] * SW + cj] = lk[t];
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 4; ++t) g[t] = real[t] ? (2.0 * wv[t]) * L.lb[p][cj * SW + ri[t]] : 0.0;
}

}  // namespace pstb
}  // namespace midagma
