// A batch of B independent small-d problems (d <= 64, float64; l2 in cov mode, at d <= 32 with the
// PST trek regularizer, or the logistic loss on each problem's X) behind the midagma_batch_*,
// midagma_btrek_* and midagma_blogit_* entries of the C ABI: the
// small-d persistent loop (small.hip) with one workgroup per problem.  Without a regularizer,
// problem b's result is bit-identical to what a midagma_solver gives for that problem alone: the
// same kernel instantiation runs it, on Params / State / (-mu) cov / W / m / v filled as
// midagma_solver::begin fills them (solver_impl.h's shared helpers), and the kernel's results do
// not depend on how the host splits slots over launches.  With PST (pst_blk.h's body in the
// slots; the single solver runs trek.hip's launch chain) a problem's result does not depend on
// the rest of the batch, and agrees with the single solver's to rounding.  The logistic loss
// (midagma_blogit_*) runs logit_blk.h's row-block score phase over the problem's X inside small.hip's slots,
// where the single solver runs gemm.hip's launch chain: again independent of the rest of the batch
// bit for bit, and equal to the single solver to rounding.
//
// Device layout: every per-problem array of the single solver with a leading problem index
// (D x D slabs with D = 64, as the single solver pads d <= 64).  The host relaunches only the
// problems still ST_RUNNING, through a device index list, so a finished problem costs nothing in
// later launches; workgroups never wait on each other, and a grid beyond the device's residency
// queues.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "batch_impl.h"

namespace {

constexpr int64_t kMaxBatch = 16384;

// The listed problems' d x d blocks between the compact host layout (B x d x d) and the padded
// slabs (B x D x D, zero padding).  grid (D * D / NTHREADS, problems listed).
__global__ void batch_pad_kernel(const double* __restrict__ src, double* __restrict__ dst, int64_t d, int64_t D,
                                 const int32_t* __restrict__ index) {
  const int64_t b = index ? index[blockIdx.y] : blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (e >= D * D) return;
  const int64_t i = e / D, j = e % D;
  dst[b * D * D + e] = (i < d && j < d) ? src[b * d * d + i * d + j] : 0.0;
}
__global__ void batch_unpad_kernel(const double* __restrict__ src, double* __restrict__ dst, int64_t d, int64_t D,
                                   const int32_t* __restrict__ index) {
  const int64_t b = index ? index[blockIdx.y] : blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (e >= d * d) return;
  dst[b * d * d + e] = src[b * D * D + (e / d) * D + e % d];
}
// What midagma_solver::begin enqueues, for the listed problems: (-mu) cov (launch_scale's
// a * x), m = v = 0, no pending norms and no warm start.
__global__ void batch_begin_kernel(const Params* __restrict__ pr, const double* __restrict__ cov,
                                   double* __restrict__ covs, double* __restrict__ m, double* __restrict__ v,
                                   double* __restrict__ carry, int64_t DD, const int32_t* __restrict__ index) {
  const int64_t b = index[blockIdx.y];
  const int64_t e = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (e < NORM_FIELDS + 1) carry[b * (NORM_FIELDS + 1) + e] = 0.0;
  if (e >= DD) return;
  const double a = -pr[b].mu;
  covs[b * DD + e] = a * cov[b * DD + e];
  m[b * DD + e] = 0.0;
  v[b * DD + e] = 0.0;
}

bool finite_block(const double* p, int64_t count) {
  for (int64_t i = 0; i < count; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

}  // namespace

void midagma_batch::alloc() {
  const size_t DD = (size_t)D * D, ds = (size_t)small_block(d);
  for (DevBuf<>* b : {&W, &m, &v, &cov, &covs}) b->alloc((size_t)B * DD);
  carry.alloc((size_t)B * (NORM_FIELDS + 1));
  pstore.alloc((size_t)B * 2 * ds * ds);
  stage.alloc((size_t)B * d * d);
  d_params.alloc(B);
  d_state.alloc(B);
  d_index.alloc(B);
  h_params.alloc(B);
  h_state.alloc(B);
  h_index.alloc(B);
  for (int64_t b = 0; b < B; ++b) {
    h_params.p[b] = Params{};
    h_state.p[b] = State{};
  }
  last_active.assign(B, 0);
}

void midagma_batch::upload_all(DevBuf<>& dst, const double* src) {
  HIP_TRY(hipMemcpyAsync(stage.p, src, (size_t)B * d * d * sizeof(double), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(batch_pad_kernel, grid(D * D, B), dim3(NTHREADS), 0, stream, stage.p, dst.p, d, D, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(stream));
}

void midagma_batch::download_all(const DevBuf<>& src, double* dst) {
  hipLaunchKernelGGL(batch_unpad_kernel, grid(d * d, B), dim3(NTHREADS), 0, stream, src.p, stage.p, d, D, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(dst, stage.p, (size_t)B * d * d * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
}

void midagma_batch::ensure_tables(double b1, double b2, int64_t max_iter, int64_t checkpoint) {
  if (!(b1 == bc_b1 && b2 == bc_b2 && max_iter <= bc_len)) {  // midagma_solver::ensure_bc_table
    const int64_t len = std::max<int64_t>(max_iter, 1);
    const std::vector<double> t = bc_table_values(b1, b2, len);
    bc_table.alloc(2 * len);
    HIP_TRY(hipMemcpy(bc_table.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    bc_b1 = b1;
    bc_b2 = b2;
    bc_len = len;
  }
  const int64_t need = max_iter / checkpoint + 4;  // midagma_solver::ensure_ckpt
  if (need > ckpt_cap) {
    d_ckpt.alloc((size_t)B * need);
    ckpt_cap = need;
  }
}

void midagma_batch::minimize(double* Wh, const double* mu, const double* s_dom, const double* lr,
                             const double* lambda1, int64_t max_iter, double tol, double b1, double b2,
                             int64_t checkpoint, const uint8_t* active, midagma_result* res, bool logistic) {
  ensure_tables(b1, b2, max_iter, checkpoint);
  const SmallLogit lg = logistic ? logit_view() : SmallLogit{};
  int64_t n_run = 0;
  for (int64_t b = 0; b < B; ++b) {
    last_active[b] = !active || active[b];
    if (!last_active[b]) continue;
    h_params.p[b] = cov_l2_params(d, D, mu[b], s_dom[b], lambda1[b], tol, b1, b2, max_iter, checkpoint, bc_len,
                                  has_inc, has_exc);
    if (logistic) logistic_data_params(h_params.p[b], mu[b], (double)x_n);
    if (trek.mode && !logistic) {
      h_params.p[b].trek_weight = trek_weight[b];
      h_params.p[b].trek_mode = trek.mode;
    }
    h_state.p[b] = initial_state(lr[b]);
    h_index.p[n_run++] = (int32_t)b;
  }
  if (n_run == 0) return;
  const int64_t DD = D * D;
  HIP_TRY(hipMemcpyAsync(d_params.p, h_params.p, B * sizeof(Params), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_state.p, h_state.p, B * sizeof(State), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_index.p, h_index.p, n_run * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  // (the stage keeps the caller's W of the inactive problems, which the download hands back)
  HIP_TRY(hipMemcpyAsync(stage.p, Wh, (size_t)B * d * d * sizeof(double), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(batch_pad_kernel, grid(DD, n_run), dim3(NTHREADS), 0, stream, stage.p, W.p, d, D, d_index.p);
  hipLaunchKernelGGL(batch_begin_kernel, grid(DD, n_run), dim3(NTHREADS), 0, stream, d_params.p, cov.p, covs.p, m.p,
                     v.p, carry.p, DD, d_index.p);
  HIP_TRY(hipGetLastError());
  const int64_t n_active = n_run;

  // drive_small over the problems still running: one launch of up to kSmallBatch slots, one
  // copy of every State, one sync
  const int64_t cap = slot_cap(max_iter, checkpoint);
  for (int64_t launched = 0; n_run > 0;) {
    const int64_t slots = small_next_batch(-1, launched, cap, midagma_solver::kSmallBatch);
    // (the logistic slots read the plain cov: G_score = (zscale X)^T expit(X W) + cscale cov)
    const SmallArrays arr{d_params.p, d_state.p, W.p, m.p, v.p, logistic ? cov.p : covs.p,
                          has_inc ? minc.p : nullptr, has_exc ? mexc.p : nullptr, bc_table.p, d_ckpt.p, ckpt_cap,
                          carry.p, pstore.p};
    SmallRun run{d, slots, d_index.p, n_run};
    run.pst = trek.mode && !logistic ? &trek : nullptr;
    run.logit = logistic ? &lg : nullptr;
    launch_small_minimize(arr, run, stream);
    launched += slots;
    HIP_TRY(hipMemcpyAsync(h_state.p, d_state.p, B * sizeof(State), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    int64_t still = 0;
    for (int64_t k = 0; k < n_run; ++k) {
      const int32_t b = h_index.p[k];
      if (h_state.p[b].status == ST_RUNNING) h_index.p[still++] = b;
    }
    n_run = still;
    if (n_run > 0)
      HIP_TRY(hipMemcpyAsync(d_index.p, h_index.p, n_run * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  }

  // hand back the active problems' W (the index list of the call again)
  int64_t k = 0;
  for (int64_t b = 0; b < B; ++b)
    if (last_active[b]) h_index.p[k++] = (int32_t)b;
  HIP_TRY(hipMemcpyAsync(d_index.p, h_index.p, n_active * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(batch_unpad_kernel, grid(d * d, n_active), dim3(NTHREADS), 0, stream, W.p, stage.p, d, D,
                     d_index.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(Wh, stage.p, (size_t)B * d * d * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int64_t b = 0; b < B; ++b)
    if (last_active[b]) midagma_solver::fill_result(h_state.p[b], &res[b]);
}

void midagma_batch::set_trek(int seq, int agg, int mode, const double* weight, double eps_inv, const int64_t* pairs,
                             int64_t m) {
  trek = SmallPst{};
  if (mode == 0 || m == 0) return;
  std::vector<double> N((size_t)d * d, 0.0);
  for (int64_t p = 0; p < m; ++p) N[(size_t)(pairs[2 * p] * d + pairs[2 * p + 1])] += 1.0;
  trek_N.alloc((size_t)d * d);
  trek_val.alloc((size_t)B);
  HIP_TRY(hipMemcpy(trek_N.p, N.data(), N.size() * sizeof(double), hipMemcpyHostToDevice));
  trek_weight.assign(weight, weight + B);
  trek.N = trek_N.p;
  trek.m = (double)m;
  trek.eps_inv = eps_inv;
  trek.seq = seq;
  trek.agg = agg;
  trek.mode = mode;
}

// (W and m serve as the call's scratch slabs: minimize uploads W and zeroes m at its start)
void midagma_batch::trek_value(const double* Wh, double* value, double* grad) {
  upload_all(W, Wh);
  launch_small_pst_eval(W.p, d, D, B, trek, trek_val.p, grad ? m.p : nullptr, stream);
  HIP_TRY(hipMemcpyAsync(value, trek_val.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (grad)
    download_all(m, grad);
  else
    HIP_TRY(hipStreamSynchronize(stream));
}

SmallLogit midagma_batch::logit_view() const {
  SmallLogit lg;
  lg.X = X.p;
  lg.n = x_n;
  lg.n_pad = x_n_pad;
  lg.stride = x_shared ? 0 : x_n_pad * (int64_t)small_block(d);
  return lg;
}

// host X (n x d per problem) -> the device layout: n_pad x DS doubles per problem, zero padding
void midagma_batch::set_data(const double* Xh, int64_t n, bool shared) {
  const int64_t ds = small_block(d), rb = small_logit_rows(d);
  const int64_t n_pad = (n + rb - 1) / rb * rb, count = shared ? 1 : B;
  const size_t slab = (size_t)n_pad * ds, bytes = (size_t)count * slab * sizeof(double);
  has_data = false;
  X.release();  // (the last X does not count against the new one; every entry ends synchronized)
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (bytes > free_b)
    throw std::invalid_argument("blogit_set_data: the padded X (" + std::to_string(bytes) +
                                " bytes) does not fit the device's free memory (" + std::to_string(free_b) + ")");
  X.alloc((size_t)count * slab);
  logit_loss.alloc((size_t)B);
  std::vector<double> pad(slab, 0.0);  // (rows n.., columns d.. stay zero over the problems)
  for (int64_t b = 0; b < count; ++b) {
    const double* src = Xh + b * n * d;
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = 0; j < d; ++j) pad[(size_t)(i * ds + j)] = src[i * d + j];
    HIP_TRY(hipMemcpy(X.p + (size_t)b * slab, pad.data(), slab * sizeof(double), hipMemcpyHostToDevice));
  }
  x_n = n;
  x_n_pad = n_pad;
  x_shared = shared;
  has_data = true;
}

// (W and m serve as the call's scratch slabs, as in trek_value)
void midagma_batch::logit_score(const double* Wh, double* loss, double* G) {
  upload_all(W, Wh);
  launch_small_logit_eval(W.p, cov.p, d, D, B, logit_view(), logit_loss.p, G ? m.p : nullptr, stream);
  HIP_TRY(hipMemcpyAsync(loss, logit_loss.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (G)
    download_all(m, G);
  else
    HIP_TRY(hipStreamSynchronize(stream));
}

extern "C" const char* midagma_batch_last_error(const midagma_batch* h) { return abi_last_error(h); }

extern "C" int midagma_batch_create(midagma_batch** out, int64_t d, int64_t B, int device) {
  if (!out || d < 1 || d > 64 || B < 1 || B > kMaxBatch || device < 0)
    return abi_fail(no_handle<midagma_batch>, MIDAGMA_E_ARG,
                    "batch_create: need 1 <= d <= 64, 1 <= B <= 16384 and a device");
  *out = nullptr;
  midagma_batch* h = nullptr;
  const int rc = abi_guarded(no_handle<midagma_batch>, [&] {
    open_device(device, "batch_create: ");
    h = new midagma_batch;
    h->d = d;
    h->D = round_up64(d);
    h->B = B;
    h->device = device;
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->alloc();
  });
  if (rc != MIDAGMA_OK) {
    midagma_batch_destroy(h);
    return rc;
  }
  *out = h;
  return MIDAGMA_OK;
}

extern "C" void midagma_batch_destroy(midagma_batch* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  delete h;
}

extern "C" int midagma_batch_set_cov(midagma_batch* h, const double* cov) {
  if (!h || !cov) return abi_fail(h, MIDAGMA_E_ARG, "batch_set_cov: null argument");
  if (!finite_block(cov, h->B * h->d * h->d))
    return abi_fail(h, MIDAGMA_E_ARG, "batch_set_cov: array must not contain infs or NaNs");
  return abi_guarded(h, [&] {
    h->upload_all(h->cov, cov);
    h->has_cov = true;
  });
}

extern "C" int midagma_batch_set_masks(midagma_batch* h, const double* mask_inc, const double* mask_exc) {
  if (!h) return abi_fail(h, MIDAGMA_E_ARG, "batch_set_masks: null handle");
  return abi_guarded(h, [&] {
    const size_t n = (size_t)h->B * h->D * h->D;
    if (mask_inc) {
      h->minc.alloc(n);
      h->upload_all(h->minc, mask_inc);
    }
    if (mask_exc) {
      h->mexc.alloc(n);
      h->upload_all(h->mexc, mask_exc);
    }
    h->has_inc = mask_inc != nullptr;
    h->has_exc = mask_exc != nullptr;
  });
}

// The argument checks of the two minimize entries (`what`: the entry's name in the messages)
static int check_minimize_args(midagma_batch* h, const std::string& what, bool logistic, const double* W,
                               const double* mu, const double* s_dom, const double* lr, const double* lambda1,
                               int64_t max_iter, int64_t checkpoint, const uint8_t* active, const midagma_result* res) {
  const auto bad = [&](const char* why) { return abi_fail(h, MIDAGMA_E_ARG, what + ": " + why); };
  if (!h) return bad("null handle");
  if (!W || !mu || !s_dom || !lr || !lambda1 || !res) return bad("null argument");
  if (max_iter < 1 || checkpoint < 1) return bad("max_iter and checkpoint must be >= 1");
  if (!logistic && !h->has_cov) return bad("set_cov before minimize");
  if (logistic && (!h->has_cov || !h->has_data)) return bad("set_cov and blogit_set_data before minimize");
  if (logistic && h->trek.mode) return bad("the logistic loss runs without a trek regularizer");
  const int64_t dd = h->d * h->d;
  for (int64_t b = 0; b < h->B; ++b)
    if ((!active || active[b]) && !finite_block(W + b * dd, dd)) return bad("array must not contain infs or NaNs");
  return MIDAGMA_OK;
}

extern "C" int midagma_batch_minimize(midagma_batch* h, double* W, const double* mu, const double* s_dom,
                                      const double* lr, const double* lambda1, int64_t max_iter, double tol,
                                      double beta1, double beta2, int64_t checkpoint, const uint8_t* active,
                                      midagma_result* res) {
  if (const int rc = check_minimize_args(h, "batch_minimize", false, W, mu, s_dom, lr, lambda1, max_iter, checkpoint,
                                         active, res))
    return rc;
  return abi_guarded(h, [&] {
    h->minimize(W, mu, s_dom, lr, lambda1, max_iter, tol, beta1, beta2, checkpoint, active, res);
  });
}

extern "C" int64_t midagma_batch_checkpoints(midagma_batch* h, int64_t b, midagma_ckpt* out, int64_t cap) {
  if (!h || b < 0 || b >= h->B) return abi_fail(h, MIDAGMA_E_ARG, "batch_checkpoints: bad arguments");
  if (!h->last_active[b] || !h->d_ckpt.p) return 0;
  int64_t n = 0;
  const int rc = abi_guarded(h, [&] {
    n = std::max<int64_t>(0, std::min<int64_t>(std::min<int64_t>(h->h_state.p[b].n_ckpt, h->ckpt_cap), cap));
    static_assert(sizeof(midagma_ckpt) == sizeof(CkptRec), "ckpt layout");
    if (n > 0 && out)
      HIP_TRY(hipMemcpy(out, h->d_ckpt.p + b * h->ckpt_cap, n * sizeof(CkptRec), hipMemcpyDeviceToHost));
  });
  return rc == MIDAGMA_OK ? n : rc;
}

extern "C" int midagma_btrek_set(midagma_batch* h, int seq, int agg, int mode, const double* weight, double eps_inv,
                                 const int64_t* pairs, int64_t m) {
  if (!h) return abi_fail(h, MIDAGMA_E_ARG, "btrek_set: null handle");
  if (mode < 0 || mode > 2 || m < 0) return abi_fail(h, MIDAGMA_E_ARG, "btrek_set: bad mode or pair count");
  if (mode != 0 && m > 0) {
    if (!weight || !pairs) return abi_fail(h, MIDAGMA_E_ARG, "btrek_set: null argument");
    if (h->d > 32) return abi_fail(h, MIDAGMA_E_ARG, "btrek_set: the PST regularizer in a batch needs d <= 32");
    if (seq != midagma::TREK_EXP && seq != midagma::TREK_INV)
      return abi_fail(h, MIDAGMA_E_ARG, "btrek_set: a batch runs seq exp and inv (not log or binom)");
    if (agg < midagma::TREK_MEAN || agg > midagma::TREK_LSE)
      return abi_fail(h, MIDAGMA_E_ARG, "btrek_set: unknown agg");
    for (int64_t p = 0; p < 2 * m; ++p)
      if (pairs[p] < 0 || pairs[p] >= h->d) return abi_fail(h, MIDAGMA_E_ARG, "btrek_set: pair index outside [0, d)");
    if (!finite_block(weight, h->B) || !std::isfinite(eps_inv))
      return abi_fail(h, MIDAGMA_E_ARG, "btrek_set: weight and eps_inv must be finite");
  }
  return abi_guarded(h, [&] { h->set_trek(seq, agg, mode, weight, eps_inv, pairs, m); });
}

extern "C" int midagma_btrek_value(midagma_batch* h, const double* W, double* value, double* grad) {
  if (!h) return abi_fail(h, MIDAGMA_E_ARG, "btrek_value: null handle");
  if (!W || !value) return abi_fail(h, MIDAGMA_E_ARG, "btrek_value: null argument");
  if (!finite_block(W, h->B * h->d * h->d))
    return abi_fail(h, MIDAGMA_E_ARG, "btrek_value: array must not contain infs or NaNs");
  if (!h->trek.mode) {  // no regularizer: notreks gives (0, 0) for an empty pair set
    for (int64_t b = 0; b < h->B; ++b) value[b] = 0.0;
    if (grad)
      for (int64_t e = 0; e < h->B * h->d * h->d; ++e) grad[e] = 0.0;
    return MIDAGMA_OK;
  }
  return abi_guarded(h, [&] { h->trek_value(W, value, grad); });
}

extern "C" int midagma_blogit_set_data(midagma_batch* h, const double* X, int64_t n, int shared) {
  if (!h) return abi_fail(h, MIDAGMA_E_ARG, "blogit_set_data: null handle");
  if (!X) return abi_fail(h, MIDAGMA_E_ARG, "blogit_set_data: null argument");
  if (n < 1 || n >= ((int64_t)1 << 31)) return abi_fail(h, MIDAGMA_E_ARG, "blogit_set_data: need 1 <= n < 2^31");
  if (!finite_block(X, (shared ? 1 : h->B) * n * h->d))
    return abi_fail(h, MIDAGMA_E_ARG, "blogit_set_data: array must not contain infs or NaNs");
  return abi_guarded(h, [&] { h->set_data(X, n, shared != 0); });
}

extern "C" int midagma_blogit_minimize(midagma_batch* h, double* W, const double* mu, const double* s_dom,
                                       const double* lr, const double* lambda1, int64_t max_iter, double tol,
                                       double beta1, double beta2, int64_t checkpoint, const uint8_t* active,
                                       midagma_result* res) {
  if (const int rc = check_minimize_args(h, "blogit_minimize", true, W, mu, s_dom, lr, lambda1, max_iter, checkpoint,
                                         active, res))
    return rc;
  return abi_guarded(h, [&] {
    h->minimize(W, mu, s_dom, lr, lambda1, max_iter, tol, beta1, beta2, checkpoint, active, res, true);
  });
}

extern "C" int midagma_blogit_score(midagma_batch* h, const double* W, double* loss, double* G) {
  if (!h) return abi_fail(h, MIDAGMA_E_ARG, "blogit_score: null handle");
  if (!W || !loss) return abi_fail(h, MIDAGMA_E_ARG, "blogit_score: null argument");
  if (!h->has_data || (G && !h->has_cov))
    return abi_fail(h, MIDAGMA_E_ARG, "blogit_score: blogit_set_data (and set_cov for the gradient) first");
  if (!finite_block(W, h->B * h->d * h->d))
    return abi_fail(h, MIDAGMA_E_ARG, "blogit_score: array must not contain infs or NaNs");
  return abi_guarded(h, [&] { h->logit_score(W, loss, G); });
}

// Test hook (not in the public header): the batch's W slabs as the last minimize call left them on
// the device, B x D x D with D = 64, padding included.
extern "C" int midagma_debug_batch_w_slabs(midagma_batch* h, double* out) {
  if (!h || !out) return abi_fail(h, MIDAGMA_E_ARG, "debug_batch_w_slabs: null argument");
  return abi_guarded(h, [&] {
    HIP_TRY(hipMemcpyAsync(out, h->W.p, (size_t)h->B * h->D * h->D * sizeof(double), hipMemcpyDeviceToHost,
                           h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  });
}
