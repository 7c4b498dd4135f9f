// The evaluation kernels of the one-workgroup small-d path (d <= 64): the PST penalty and the
// logistic score of B given matrices, one workgroup each and no Adam step, on the bodies the
// persistent loop's slots run (pst_blk.h, logit_blk.h) and its owner-tile layer (wgtile.h).
#include "launch.h"
#include "logit_blk.h"
#include "pst_blk.h"
#include "wgtile.h"

namespace midagma {
namespace {

// The PST penalty of B given matrices, no Adam step: workgroup b runs pst_blk.h's body on problem
// b's D x D slab of W; value[b], and with grad (D x D slabs) d value / d W on d x d.
template <int DS, int NW>
__global__ __launch_bounds__(64 * NW) void small_pst_eval_kernel(const double* __restrict__ W_, int64_t d, int64_t D,
                                                                  SmallPst ps, double* __restrict__ value,
                                                                  double* __restrict__ grad_) {
  using WT = WgTile<DS>;
  static_assert(NW == WT::NW, "one 16 x 16 tile per wave");
  constexpr int SW = WT::SW, SI = WT::SI;
  __shared__ double Wimg[DS * SW];
  __shared__ double PAbuf[2 * DS * SW], PRbuf[2 * DS * SW], PBbuf[2 * DS * SI];
  __shared__ __attribute__((aligned(32))) double rowb[2][DS];
  __shared__ __attribute__((aligned(32))) double colb[2][DS];
  __shared__ pstb::PstLds<DS, NW> PL;
  const int tid = threadIdx.x, di = (int)d;
  const WT T(tid, di);
  const double* __restrict__ const W = W_ + (int64_t)blockIdx.x * D * D;
  double wv[4], g[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    wv[t] = T.real[t] ? W[(int64_t)T.ri[t] * D + T.cj] : 0.0;
    Wimg[T.ri[t] * SW + T.cj] = wv[t];
  }
  wg_load_dense<DS>(PL.nimg, ps.N, di);
  __syncthreads();
  const pstb::PstBufs pbufs{PAbuf, PRbuf, PBbuf, rowb[0], colb[0]};
  pstb::pst_blk_body<DS, NW>(ps, di, wv, Wimg, pbufs, PL, grad_ != nullptr, g);
  __syncthreads();
  if (tid == 0) value[blockIdx.x] = PL.val;
  if (grad_) {
    double* __restrict__ const G = grad_ + (int64_t)blockIdx.x * D * D;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (T.real[t]) G[(int64_t)T.ri[t] * D + T.cj] = g[t];
  }
}

// The reference's logistic _score (linear.py:89-92) of B given matrices, no Adam step: workgroup b
// runs logit_score_phase on problem b's D x D slab of W and its X; loss[b], and with G (D x D slabs)
// X^T expit(X W) / n - cov on d x d.
template <int DS, int NW>
__global__ __launch_bounds__(64 * NW) void small_logit_eval_kernel(const double* __restrict__ W_,
                                                                    const double* __restrict__ cov_, int64_t d,
                                                                    int64_t D, SmallLogit lg,
                                                                    double* __restrict__ loss_out,
                                                                    double* __restrict__ G_) {
  using WT = WgTile<DS>;
  static_assert(NW == WT::NW, "one 16 x 16 tile per wave");
  constexpr int NT = WT::NT, SW = WT::SW, SI = WT::SI;
  constexpr int RB = kLogitRows<DS>;
  __shared__ double IWimg[DS * SI];
  __shared__ double wdiag[DS];
  __shared__ double Xbuf[2 * RB * SW];
  __shared__ double Sbuf[2][RB * SI];
  __shared__ double red[NW];
  const int tid = threadIdx.x, lane = tid & 63, di = (int)d;
  const WT T(tid, di);
  const int64_t slab = (int64_t)blockIdx.x * D * D;
  const double* __restrict__ const W = W_ + slab;
  for (int e = tid; e < DS * SI; e += NT) IWimg[e] = 0.0;
  for (int e = tid; e < DS; e += NT) wdiag[e] = 0.0;
  double wv[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) wv[t] = T.real[t] ? W[(int64_t)T.ri[t] * D + T.cj] : 0.0;
  __syncthreads();
  wg_store_w<DS>(T, wv, wdiag, IWimg);
  __syncthreads();
  dbl4 z;
  double loss;
  const double inv_n = 1.0 / (double)lg.n;
  logit_score_phase<DS, NW>(lg.X + (int64_t)blockIdx.x * lg.stride, lg.n, lg.n_pad, di, Xbuf, Sbuf[0], Sbuf[1],
                            IWimg, wdiag, true, T.row0 / 16, T.col0 / 16, inv_n, z, loss);
  loss = wave_sum(loss);
  if (lane == 0) red[T.w] = loss;
  __syncthreads();
  if (tid == 0) {
    double x = 0.0;
#pragma unroll 1
    for (int y = 0; y < NW; ++y) x += red[y];
    loss_out[blockIdx.x] = x * inv_n;
  }
  if (G_) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (T.real[t]) {
        const int64_t idx = slab + (int64_t)T.ri[t] * D + T.cj;
        G_[idx] = z[t] - cov_[idx];  // (1 / n X^T) @ expit(X W) - cov, linear.py:92
      }
  }
}

}  // namespace

bool logit_ok(const SmallLogit& lg, int rb) {
  return lg.X && lg.n >= 1 && rb > 0 && lg.n_pad >= lg.n && lg.n_pad % rb == 0 && lg.stride >= 0;
}

void launch_small_pst_eval(const double* W, int64_t d, int64_t D, int64_t n_problems, const SmallPst& ps,
                           double* value, double* grad, hipStream_t stream) {
  const int ds = small_block(d);
  if (ds == 0 || ds > 32 || n_problems < 1 || !ps.N || !(ps.m > 0.0) || (ps.seq != TREK_EXP && ps.seq != TREK_INV) ||
      ps.agg < TREK_MEAN || ps.agg > TREK_LSE)
    throw std::invalid_argument("small_pst_eval: PST needs d <= 32, seq exp or inv and pairs");
  if (ds == 16)
    hipLaunchKernelGGL((small_pst_eval_kernel<16, 1>), dim3((unsigned)n_problems), dim3(64), 0, stream, W, d, D, ps,
                       value, grad);
  else
    hipLaunchKernelGGL((small_pst_eval_kernel<32, 4>), dim3((unsigned)n_problems), dim3(256), 0, stream, W, d, D, ps,
                       value, grad);
  HIP_TRY(hipGetLastError());
}

void launch_small_logit_eval(const double* W, const double* cov, int64_t d, int64_t D, int64_t n_problems,
                             const SmallLogit& lg, double* loss, double* G, hipStream_t stream) {
  const int ds = small_block(d);
  if (ds == 0 || n_problems < 1 || !W || !loss || (G && !cov) || !logit_ok(lg, small_logit_rows(d)))
    throw std::invalid_argument("small_logit_eval: d <= 64 and a padded X");
  const dim3 grid((unsigned)n_problems);
  if (ds == 16)
    hipLaunchKernelGGL((small_logit_eval_kernel<16, 1>), grid, dim3(64), 0, stream, W, cov, d, D, lg, loss, G);
  else if (ds == 32)
    hipLaunchKernelGGL((small_logit_eval_kernel<32, 4>), grid, dim3(256), 0, stream, W, cov, d, D, lg, loss, G);
  else
    hipLaunchKernelGGL((small_logit_eval_kernel<64, 16>), grid, dim3(1024), 0, stream, W, cov, d, D, lg, loss, G);
  HIP_TRY(hipGetLastError());
}

}  // namespace midagma
