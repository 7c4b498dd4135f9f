// The logistic score phase of the one-workgroup small-d kernels (d <= 64): the device body a slot of
// the persistent loop (small.hip) and the score evaluation kernel (small_eval.hip) run on their own
// workgroup, its element ownership (wgtile.h) and the caller's LDS.
//
// The logistic loss (a batch, float64, no regularizer) has no covariance to fold n into:
// its score phase streams the problem's X (n_pad x DS doubles, zero padding) through the workgroup
// in blocks of kLogitRows rows, in ascending order.  Per block, R = X_blk W on the matrix cores
// against the W image in LDS, S = expit(R) staged through LDS (the accumulator layout is not the
// B-operand layout), Z += (mu / n X_blk)^T S into the owner's accumulator (X^T scaled first, as
// the reference scales it), so Z lands where rhs lands for l2.  A block is loaded once: the wave
// takes its X_blk^T fragments for the second product into registers while the block is current,
// which lets two X buffers and two S buffers run at one barrier a block.  In the slot loop the S
// buffers alias the product form's operand images (the inverse and the score phase never overlap),
// the X buffers take the place of the (-mu) cov image.
// On checkpoint slots the lanes also sum logaddexp(0, R) - X o R over the valid n x d entries.
// Every sum has a fixed order (blocks ascending, lanes, waves), so a problem's result does not
// depend on the batch.
#pragma once

#include "launch.h"
#include "logit_math.h"
#include "wgtile.h"

namespace midagma {

// Rows of one X block of the logistic score phase.  DS <= 32: DS rows, so the block's R has one
// 16 x 16 tile per wave; DS = 64: 32 rows (8 of the 16 waves form R), which is what fits beside
// the inverse's images in the CU's 160 KB of LDS.
template <int DS>
constexpr int kLogitRows = DS >= 64 ? 32 : DS;

// The logistic score phase of one workgroup: z += (xscale X)^T expit(X W) over the nb = n_pad / RB
// row blocks of X, for the 16 x 16 tile (tr, tc) this wave owns.  X^T is scaled before the product,
// entry by entry, as the reference's `mu / n * X.T @ sigmoid(X @ W)` scales it (linear.py:246), and
// an element's terms are added in ascending row order: with binary X an exactly cancelling entry of
// G_score keeps the rounding the reference's own sum leaves there, whose sign picks the L1 branch.
// With want_loss also this lane's share of sum(logaddexp(0, R) - X o R) over the rows < n and
// columns < di.  W is read as the B operand from
// the I - W image (off-diagonal entries are -W exactly) and the diagonal words.  Xbuf: 2 x RB x
// (DS + 2) doubles, S0 / S1: RB x SI doubles each.  Stage s (one barrier each): the second product of
// block s - 1 from the wave's registers and S[(s - 1) & 1]; the wave's X^T fragments of block s;
// the first product of block s, its sigmoid into S[s & 1]; block s + 1 from registers into
// Xbuf[(s + 1) & 1] and block s + 2 from global memory into registers.  Block 0 is stored ahead of
// the first barrier, which also ends every wave's earlier reads of whatever S0 / S1 alias.
template <int DS, int NW>
__device__ __forceinline__ void logit_score_phase(const double* __restrict__ X, int64_t n, int64_t n_pad, int di,
                                                  double* __restrict__ Xbuf, double* __restrict__ S0,
                                                  double* __restrict__ S1, const double* __restrict__ IWimg,
                                                  const double* __restrict__ wdiag, bool want_loss, int tr, int tc,
                                                  double xscale, dbl4& z, double& loss) {
  using WT = WgTile<DS>;
  constexpr int RB = kLogitRows<DS>, NT = WT::NT, TPR = WT::TPR, SX = WT::SW, SI = WT::SI;
  constexpr int XE = RB * DS / NT;  // elements of a block per thread
  constexpr bool HOIST = DS <= 32;  // the W fragments stay in registers over the blocks
  static_assert(NW == WT::NW, "one 16 x 16 tile per wave");
  static_assert(XE * NT == RB * DS && RB % 16 == 0 && (RB / 16) * TPR <= NW, "block shape");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, c = lane & 15;
  const int rt = w / TPR, ct = w % TPR;  // this wave's tile of the block's R
  const bool has_r = rt < RB / 16;
  const int64_t nb = n_pad / RB;
  double ga[XE], gb[XE], xt[RB / 4];
  [[maybe_unused]] double wb[HOIST ? DS / 4 : 1];
  auto w_at = [&](int k, int nn) { return k == nn ? wdiag[k] : -IWimg[k * SI + nn]; };
  if constexpr (HOIST) {
#pragma unroll
    for (int kk = 0; kk < DS / 4; ++kk) wb[kk] = w_at(4 * kk + q, 16 * ct + c);
  }
  // a block travels global memory -> registers -> LDS, two blocks ahead of its products: one stage
  // is shorter than a global load's latency
  auto load_blk = [&](double(&gr)[XE], int64_t blk) __attribute__((always_inline)) {
    const double* __restrict__ const Xn = X + blk * (RB * DS);
#pragma unroll
    for (int i = 0; i < XE; ++i) gr[i] = Xn[tid + i * NT];
  };
  auto store_blk = [&](const double(&gr)[XE], int64_t blk) __attribute__((always_inline)) {
    double* __restrict__ const Xw = Xbuf + (blk & 1) * (RB * SX);
#pragma unroll
    for (int i = 0; i < XE; ++i) {
      const int e = tid + i * NT;
      Xw[(e / DS) * SX + e % DS] = gr[i];
    }
  };
  load_blk(ga, 0);
  if (nb > 1) load_blk(gb, 1);
  store_blk(ga, 0);
  z = dbl4{0.0, 0.0, 0.0, 0.0};
  loss = 0.0;
  __syncthreads();
  // stage s; gw holds block s + 1, gl (block s, stored a stage ago) takes block s + 2
  auto stage = [&](int64_t s, const double(&gw)[XE], double(&gl)[XE]) __attribute__((always_inline)) {
    const double* __restrict__ const Xc = Xbuf + (s & 1) * (RB * SX);
    if (s + 2 < nb) load_blk(gl, s + 2);
    if (s >= 1) {
      const double* __restrict__ const Sp = ((s - 1) & 1) ? S1 : S0;
#pragma unroll
      for (int kk = 0; kk < RB / 4; ++kk)
        z = __builtin_amdgcn_mfma_f64_16x16x4f64(xt[kk], Sp[(4 * kk + q) * SI + 16 * tc + c], z, 0, 0, 0);
    }
    if (s == nb) return;
#pragma unroll
    for (int kk = 0; kk < RB / 4; ++kk) xt[kk] = xscale * Xc[(4 * kk + q) * SX + 16 * tr + c];
    if (has_r) {
      dbl4 r = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < DS / 4; ++kk)
        if (DS < 64 || 4 * kk < di) {  // (X's columns and W's rows >= d are zero)
          const double wop = HOIST ? wb[HOIST ? kk : 0] : w_at(4 * kk + q, 16 * ct + c);
          r = __builtin_amdgcn_mfma_f64_16x16x4f64(Xc[(16 * rt + c) * SX + 4 * kk + q], wop, r, 0, 0, 0);
        }
      double* __restrict__ const Sc = (s & 1) ? S1 : S0;
      const int col = 16 * ct + c;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int row = 16 * rt + q + 4 * t;
        Sc[row * SI + col] = expit(r[t]);
        // padded rows and columns have R = 0, logaddexp = log 2: they stay out of the loss
        if (want_loss && s * RB + row < n && col < di) loss += logaddexp0(r[t]) - Xc[row * SX + col] * r[t];
      }
    }
    if (s + 1 < nb) store_blk(gw, s + 1);
    __syncthreads();
  };
  for (int64_t s = 0; s <= nb; s += 2) {
    stage(s, gb, ga);
    if (s + 1 <= nb) stage(s + 1, ga, gb);
  }
}

}  // namespace midagma
