// The midagma_solver entries of the C ABI (include/midagma_hip.h) and the solver's debug hooks.
// The solver object and its drivers: solver_impl.h; the entry-point layer: abi.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/midagma_hip.h"
#include "solver_impl.h"

namespace {

// scipy's check_finite (linear.py:226 -> sla.inv(..., check_finite=True)): a non-finite input
// is a ValueError, not a singular matrix
bool all_finite(const double* p, int64_t rows, int64_t cols, int64_t ld) {
  for (int64_t i = 0; i < rows; ++i)
    for (int64_t j = 0; j < cols; ++j)
      if (!std::isfinite(p[i * ld + j])) return false;
  return true;
}

__global__ void div_kernel(const double* __restrict__ x, double n, double* __restrict__ y, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; i < count; i += (int64_t)gridDim.x * NTHREADS)
    y[i] = x[i] / n;
}

}  // namespace

// abi.h's hook: an entry's device work runs on the solver's device
static void abi_select_device(const midagma_solver* s) { HIP_TRY(hipSetDevice(s->device)); }

void midagma::setup_attributes() {
  static std::once_flag once;
  std::call_once(once, [] {
    gj_setup_attributes();
    gemm_setup_attributes();
  });
}

namespace {

// A minimize that ended ST_SINGULAR: the reference's sla.inv raised at that step.  scipy
// raises ValueError when sI - W*W has a non-finite entry (check_finite: W itself went
// non-finite, e.g. from non-finite data) and LinAlgError when the finite matrix is singular.
int singular_or_nonfinite(midagma_solver* s, int rc, const midagma_result* res, const double* W) {
  if (rc != MIDAGMA_OK || !res || res->status != MIDAGMA_ST_SINGULAR) return rc;
  if (!all_finite(W, s->d, s->d, s->d)) return abi_fail(s, MIDAGMA_E_ARG, std::string("minimize: ") + kNonFinite);
  return abi_fail(s, MIDAGMA_E_SINGULAR, "singular matrix: inverse of sI - W*W is not finite");
}

}  // namespace

// ---- the handle's evaluations of a given W and its diagnostics (declared in solver_impl.h) ----

// W (d x d, host) zero-padded into scratch
static void upload_scratch(midagma_solver* s, const double* Wh) {
  const int64_t DD = s->D * s->D;
  s->scratch.alloc(DD);
  HIP_TRY(hipMemsetAsync(s->scratch.p, 0, DD * sizeof(double), s->stream));
  s->upload_matrix(s->scratch, Wh, s->d);
}

void midagma_solver::eval_trek(const double* Wh, double* value, double* G) {
  if (!trek.on) {  // trek_value_grad: (0, zeros) when disabled (notreks.py)
    *value = 0.0;
    if (G) std::fill(G, G + d * d, 0.0);
    return;
  }
  upload_scratch(this, Wh);
  // weight 1: the bare gradient, as trek_value_grad returns it
  trek.enqueue(scratch.p, d, D, trek.probe.p, stream, /*weight1=*/true);
  HIP_TRY(hipMemcpyAsync(value, trek.scal(), sizeof(double), hipMemcpyDeviceToHost, stream));
  if (G) {
    if (trek.cfg.mode == 2) {
      HIP_TRY(hipMemcpy2DAsync(G, d * sizeof(double), trek.G.p, D * sizeof(double), d * sizeof(double), d,
                               hipMemcpyDeviceToHost, stream));
    } else {
      std::fill(G, G + d * d, 0.0);
    }
  }
  HIP_TRY(hipStreamSynchronize(stream));
}

void midagma_solver::eval_h(const double* Wh, double s_dom, double* h, double* G) {
  const int64_t DD = D * D;
  upload_scratch(this, Wh);
  DevBuf<> work;
  work.alloc(DD);
  launch_build_at(scratch.p, D, true, work.p, D, d, s_dom, nullptr, nullptr, stream);
  GJWork gw = gj();
  gw.Pstore = nullptr;
  launch_gj_inverse(work.p, D, D, gw, nullptr, stream);
  std::vector<double> pl(D);
  HIP_TRY(hipMemcpyAsync(pl.data(), pivlog.p, D * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (G) {
    Gtmp.alloc((size_t)d * d);
    launch_h_grad(scratch.p, work.p, Gtmp.p, d, D, stream);
    HIP_TRY(hipMemcpyAsync(G, Gtmp.p, (size_t)d * d * sizeof(double), hipMemcpyDeviceToHost, stream));
  }
  HIP_TRY(hipStreamSynchronize(stream));
  double ld = 0.0;
  for (int64_t i = 0; i < d; ++i) ld += pl[i];
  *h = -ld + (double)d * std::log(s_dom);
}

void midagma_solver::trace_l1(const double* Wd, const double* Z, double* sd, double* l1) {
  launch_trace_l1(Wd, Z, partials.p, d, D, stream);
  std::vector<double> part(2 * NRED);
  HIP_TRY(hipMemcpyAsync(part.data(), partials.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  double a = 0.0, b = 0.0;
  for (int i = 0; i < NRED; ++i) {
    a += part[2 * i];
    b += part[2 * i + 1];
  }
  *sd = a;
  if (l1) *l1 = b;
}

void midagma_solver::eval_score(const double* Wh, double* loss_out, double* G) {
  const int64_t DD = D * D;
  upload_scratch(this, Wh);
  DevBuf<> rhs;
  rhs.alloc(DD);
  // rhs = cov @ (I - W)   (linear.py:85-86)
  enqueue_cov_gemm(cov_spec(cov.p, false, scratch.p, B_IMINUS), rhs.p, nullptr);
  double sd = 0;
  trace_l1(scratch.p, rhs.p, &sd, nullptr);
  *loss_out = 0.5 * sd;
  if (G) {
    Gtmp.alloc((size_t)d * d);
    launch_scale(rhs.p, -1.0, rhs.p, DD, stream);  // G_loss = -rhs
    download_matrix(G, rhs.p);
  }
  HIP_TRY(hipStreamSynchronize(stream));
}

void midagma_solver::score_partial(const double* Wh) {
  upload_scratch(this, Wh);
  HIP_TRY(hipMemsetAsync(zbuf + D * D, 0, 64 * sizeof(double), stream));
  // Force loss partials: pass no state (st == nullptr computes them unconditionally).
  enqueue_data_partial(scratch.p, nullptr);
  HIP_TRY(hipStreamSynchronize(stream));
}

void midagma_solver::score_finish(double* loss_out, double* G) {
  const int64_t DD = D * D;
  const double n = (double)data.n_global;
  if (loss == MIDAGMA_LOSS_L2) {
    // loss = 0.5 tr((I-W)^T cov (I-W)) with cov (I-W) = Z / n ; G = -Z / n
    double sd = 0;
    trace_l1(scratch.p, zbuf, &sd, nullptr);
    *loss_out = 0.5 * (sd / n);
    if (G) {
      std::vector<double> z((size_t)d * d);
      download_matrix(z.data(), zbuf);
      HIP_TRY(hipStreamSynchronize(stream));
      for (size_t i = 0; i < z.size(); ++i) G[i] = -(z[i] / n);
    }
  } else {
    double tail = 0;
    HIP_TRY(hipMemcpyAsync(&tail, zbuf + DD, sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *loss_out = 1.0 / n * tail;
    if (G) {
      std::vector<double> z((size_t)d * d), c((size_t)d * d);
      download_matrix(z.data(), zbuf);
      download_matrix(c.data(), cov.p);
      HIP_TRY(hipStreamSynchronize(stream));
      for (size_t i = 0; i < z.size(); ++i) G[i] = (1.0 / n) * z[i] - c[i];
    }
  }
}

// [0] build (sI - W o W)^T   [1] GJ inverse   [2] score GEMM(s)   [3] whole slot (graph)
// data mode: [4] Y = X (I - W) GEMM   [5] Z = X^T Y GEMM (+ slice sum)
// blocked: [6] build + fast blocked inverse, less [0]   [7] whole fast slot (graph)
void midagma_solver::profile_parts(int reps, double* ms_out) {
  Event a, b;
  a.create();
  b.create();
  auto timed = [&](auto&& body) {
    HIP_TRY(hipEventRecord(a, stream));
    for (int r = 0; r < reps; ++r) body();
    HIP_TRY(hipEventRecord(b, stream));
    HIP_TRY(hipEventSynchronize(b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, a, b));
    return (double)ms / reps;
  };
  ms_out[0] = timed([&] { launch_build_at(W.p, D, true, Mt.p, D, d, 0.0, d_params.p, d_state.p, stream, IW.p); });
  ms_out[1] = timed([&] { launch_gj_inverse(Mt.p, D, D, gj(), d_state.p, stream); });
  if (mode == MIDAGMA_MODE_COV) {
    ms_out[2] = timed([&] { enqueue_score_cov(zbuf, d_state.p, true); });
    ms_out[4] = ms_out[5] = 0.0;
  } else {
    ms_out[2] = timed([&] { enqueue_data_partial(W.p, d_state.p, IW.p); });
    ms_out[4] = timed([&] { data.enqueue_xw(W.p, d_state.p, IW.p, stream); });
    ms_out[5] = timed([&] { data.enqueue_xty(zbuf, d_state.p, stream); });
  }
  ms_out[3] = timed([&] { HIP_TRY(hipGraphLaunch(graphs[SlotGraphs::FULL], stream)); });
  ms_out[6] = ms_out[7] = 0.0;
  if (blocked()) {
    // Both need a warm start and no pending checkpoint: one slow slot first.
    HIP_TRY(hipGraphLaunch(graphs[SlotGraphs::FULL], stream));
    ms_out[6] = timed([&] { enqueue_build_inverse(/*fast=*/true, 2); }) - ms_out[0];
    ms_out[7] = timed([&] { HIP_TRY(hipGraphLaunch(graphs[SlotGraphs::FAST], stream)); });
    State st{};
    HIP_TRY(hipMemcpy(&st, d_state.p, sizeof(State), hipMemcpyDeviceToHost));
    if (st.status == ST_NEED_GJ) {  // the fast path did not run: report it, leave a clean state
      ms_out[6] = ms_out[7] = -1.0;
      static const int32_t running = ST_RUNNING;
      HIP_TRY(hipMemcpy(&d_state.p->status, &running, sizeof(int32_t), hipMemcpyHostToDevice));
      binv.fast_ready = false;
    }
  }
}

// ---- the C ABI: argument checks, one abi_guarded, a call on the handle (abi.h) ----------------

extern "C" {

int midagma_abi_version(void) { return MIDAGMA_ABI_VERSION; }

int midagma_device_count(int* n) {
  return abi_guarded(nullptr, [&] {
    HIP_TRY(hipGetDeviceCount(n));
    return MIDAGMA_OK;
  });
}

const char* midagma_last_error(const midagma_solver* s) { return abi_last_error(s); }

int midagma_create(midagma_solver** out, int loss, int mode, int64_t d, int device, void* stream) {
  if (!out || d < 1 || (loss != 0 && loss != 1) || (mode != 0 && mode != 1) ||
      (loss == MIDAGMA_LOSS_LOGISTIC && mode == MIDAGMA_MODE_COV))
    return abi_fail(nullptr, MIDAGMA_E_ARG, "midagma_create: bad arguments (logistic needs data mode)");
  midagma_solver* s = new midagma_solver();
  s->knobs = SolverKnobs::read();
  s->loss = loss;
  s->mode = mode;
  s->d = d;
  s->D = padded_dim(d, mode, s->knobs);
  s->device = device;
  int rc = abi_guarded(s, [&] {
    setup_attributes();
    if (stream) {
      s->stream = reinterpret_cast<hipStream_t>(stream);
    } else {
      HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
      s->own_stream = true;
    }
    s->alloc_core();
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIDAGMA_OK;
  });
  if (rc != MIDAGMA_OK) {
    abi_fail(nullptr, rc, s->err);
    delete s;
    return rc;
  }
  *out = s;
  return MIDAGMA_OK;
}

void midagma_destroy(midagma_solver* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  delete s;
}

void* midagma_stream(midagma_solver* s) { return s ? reinterpret_cast<void*>(s->stream) : nullptr; }
int64_t midagma_padded_dim(const midagma_solver* s) { return s ? s->D : 0; }

int midagma_set_cov(midagma_solver* s, const double* cov, int64_t ld) {
  if (!s || !cov || ld < s->d) return abi_fail(s, MIDAGMA_E_ARG, "set_cov: bad arguments");
  if (!all_finite(cov, s->d, s->d, ld)) return abi_fail(s, MIDAGMA_E_ARG, std::string("set_cov: ") + kNonFinite);
  return abi_guarded(s, [&] {
    s->upload_matrix(s->cov, cov, ld);
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->has_cov = true;
    return MIDAGMA_OK;
  });
}

int midagma_set_masks(midagma_solver* s, const double* mask_inc, const double* mask_exc) {
  if (!s) return abi_fail(s, MIDAGMA_E_ARG, "set_masks: null solver");
  return abi_guarded(s, [&] {
    s->set_masks(mask_inc, mask_exc);
    return MIDAGMA_OK;
  });
}

int midagma_set_data(midagma_solver* s, const double* X, int64_t n_local, int64_t n_global, int on_device) {
  if (!s || !X || n_local < 1 || n_global < n_local || s->mode != MIDAGMA_MODE_DATA)
    return abi_fail(s, MIDAGMA_E_ARG, "set_data: bad arguments (data mode only)");
  if (!on_device && !all_finite(X, n_local, s->d, s->d))
    return abi_fail(s, MIDAGMA_E_ARG, std::string("set_data: ") + kNonFinite);
  return abi_guarded(s, [&] {
    s->set_data(X, n_local, n_global, on_device != 0);
    return MIDAGMA_OK;
  });
}

int midagma_data_gram(midagma_solver* s) {
  if (!s || !s->has_data) return abi_fail(s, MIDAGMA_E_STATE, "data_gram: set_data first");
  return abi_guarded(s, [&] {
    s->data.enqueue_gram(s->zbuf, s->stream);
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIDAGMA_OK;
  });
}

int midagma_cov_from_zbuf(midagma_solver* s, double n) {
  if (!s || !(n > 0)) return abi_fail(s, MIDAGMA_E_ARG, "cov_from_zbuf: n must be > 0");
  return abi_guarded(s, [&] {
    // cov = (X^T X) / float(n), a division as in linear.py:428
    const int64_t DD = s->D * s->D;
    hipLaunchKernelGGL(div_kernel, dim3(4096), dim3(NTHREADS), 0, s->stream, s->zbuf, n, s->cov.p, DD);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->has_cov = true;
    return MIDAGMA_OK;
  });
}

int midagma_get_cov(midagma_solver* s, double* out, int64_t ld) {
  if (!s || !out || ld < s->d) return abi_fail(s, MIDAGMA_E_ARG, "get_cov: bad arguments");
  if (!s->has_cov) return abi_fail(s, MIDAGMA_E_STATE, "get_cov: no cov (set_cov or cov_from_zbuf first)");
  return abi_guarded(s, [&] {
    HIP_TRY(hipMemcpy2DAsync(out, ld * sizeof(double), s->cov.p, s->D * sizeof(double), s->d * sizeof(double), s->d,
                             hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIDAGMA_OK;
  });
}

int midagma_set_cov_dev(midagma_solver* s, const double* G_dev, int64_t ldg, double divisor) {
  if (!s || !G_dev || ldg < s->d || !(divisor > 0)) return abi_fail(s, MIDAGMA_E_ARG, "set_cov_dev: bad arguments");
  return abi_guarded(s, [&] {
    // cov = (X^T X) / float(n), a division as in linear.py:428 (the caller all-reduced the Gram)
    int* flag = reinterpret_cast<int*>(s->partials.p);
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), s->stream));
    launch_div_block(G_dev, ldg, divisor, s->d, s->cov.p, s->D, flag, s->stream);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (bad) throw std::invalid_argument(std::string("set_cov_dev: ") + kNonFinite);
    s->has_cov = true;
    return MIDAGMA_OK;
  });
}

int midagma_comm_unique_id(void* out, int64_t cap) {
  if (!out || cap < 128) return abi_fail(nullptr, MIDAGMA_E_ARG, "comm_unique_id: needs a 128-byte buffer");
  return abi_guarded(nullptr, [&] { return comm_unique_id(out); });
}

int midagma_comm_init(midagma_solver* s, const void* id, int64_t id_len, int nranks, int rank) {
  if (!s || !id || id_len != 128 || nranks < 1 || rank < 0 || rank >= nranks || s->mode != MIDAGMA_MODE_DATA)
    return abi_fail(s, MIDAGMA_E_ARG, "comm_init: bad arguments (data mode, a 128-byte unique id, 0 <= rank < nranks)");
  return abi_guarded(s, [&] {
    s->init_comm(id, nranks, rank);
    return MIDAGMA_OK;
  });
}

int midagma_comm_ranks(const midagma_solver* s) { return s ? (s->comm ? s->comm_ranks : 0) : 0; }

int midagma_comm_allreduce_zbuf(midagma_solver* s) {
  if (!s || !s->comm) return abi_fail(s, MIDAGMA_E_STATE, "comm_allreduce_zbuf: comm_init first");
  return abi_guarded(s, [&] {
    comm_allreduce(s->comm, s->zbuf, (size_t)(s->D * s->D + 64), false, s->stream);
    return MIDAGMA_OK;
  });
}

int64_t midagma_zbuf_len(const midagma_solver* s) { return s ? s->D * s->D + 64 : 0; }

int midagma_bind_zbuf(midagma_solver* s, void* dev_ptr, int64_t len) {
  if (!s || len < s->D * s->D + 64) return abi_fail(s, MIDAGMA_E_ARG, "bind_zbuf: buffer too small");
  return abi_guarded(s, [&] {
    s->zbuf = dev_ptr ? static_cast<double*>(dev_ptr) : s->zown.p;
    s->graphs.valid = false;
    return MIDAGMA_OK;
  });
}

int midagma_minimize(midagma_solver* s, double* W, double mu, int64_t max_iter, double s_dom, double lr, double tol,
                     double beta1, double beta2, double lambda1, int64_t checkpoint, midagma_result* res) {
  if (!s || !W) return abi_fail(s, MIDAGMA_E_ARG, "minimize: null argument");
  if (!all_finite(W, s->d, s->d, s->d)) return abi_fail(s, MIDAGMA_E_ARG, std::string("minimize: ") + kNonFinite);
  int rc = abi_guarded(s, [&] {
    s->begin(W, mu, max_iter, s_dom, lr, tol, beta1, beta2, lambda1, checkpoint);
    s->run_loop(max_iter, checkpoint);
    s->finish(W, res);
    return MIDAGMA_OK;
  });
  return singular_or_nonfinite(s, rc, res, W);
}

int midagma_begin(midagma_solver* s, const double* W, double mu, int64_t max_iter, double s_dom, double lr,
                  double tol, double beta1, double beta2, double lambda1, int64_t checkpoint) {
  if (!s || !W) return abi_fail(s, MIDAGMA_E_ARG, "begin: null argument");
  if (!all_finite(W, s->d, s->d, s->d)) return abi_fail(s, MIDAGMA_E_ARG, std::string("begin: ") + kNonFinite);
  return abi_guarded(s, [&] {
    s->begin(W, mu, max_iter, s_dom, lr, tol, beta1, beta2, lambda1, checkpoint);
    s->ensure_graphs();
    return MIDAGMA_OK;
  });
}

int midagma_run_slots(midagma_solver* s, int64_t n) {
  if (!s || !s->begun || n < 0) return abi_fail(s, MIDAGMA_E_STATE, "run_slots: call begin first");
  return abi_guarded(s, [&] {
    s->run_slots(n);
    return MIDAGMA_OK;
  });
}

int midagma_sync(midagma_solver* s) {
  if (!s) return abi_fail(s, MIDAGMA_E_ARG, "null solver");
  return abi_guarded(s, [&] {
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIDAGMA_OK;
  });
}

int midagma_profile_parts(midagma_solver* s, int reps, double* ms_out) {
  if (!s || !s->begun || reps < 1 || !ms_out) return abi_fail(s, MIDAGMA_E_STATE, "profile_parts: call begin first");
  return abi_guarded(s, [&] {
    s->profile_parts(reps, ms_out);
    return MIDAGMA_OK;
  });
}

int midagma_step_partial(midagma_solver* s) {
  if (!s || !s->begun) return abi_fail(s, MIDAGMA_E_STATE, "step_partial: call begin first");
  return abi_guarded(s, [&] {
    HIP_TRY(hipGraphLaunch(s->graphs[SlotGraphs::PART1], s->stream));
    return MIDAGMA_OK;
  });
}

int midagma_step_finish(midagma_solver* s) {
  if (!s || !s->begun) return abi_fail(s, MIDAGMA_E_STATE, "step_finish: call begin first");
  return abi_guarded(s, [&] {
    HIP_TRY(hipGraphLaunch(s->graphs[SlotGraphs::PART2], s->stream));
    return MIDAGMA_OK;
  });
}

int midagma_poll(midagma_solver* s, midagma_result* res) {
  if (!s) return abi_fail(s, MIDAGMA_E_ARG, "null solver");
  return abi_guarded(s, [&] {
    HIP_TRY(hipMemcpyAsync(&s->h_state.p[1], s->d_state.p, sizeof(State), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->check_handoff(s->h_state.p[1]);
    midagma_solver::fill_result(s->h_state.p[1], res);
    return MIDAGMA_OK;
  });
}

int midagma_end(midagma_solver* s, double* W, midagma_result* res) {
  if (!s || !W || !s->begun) return abi_fail(s, MIDAGMA_E_STATE, "end: call begin first");
  int rc = abi_guarded(s, [&] {
    s->finish(W, res);
    return MIDAGMA_OK;
  });
  return singular_or_nonfinite(s, rc, res, W);
}

int midagma_set_w_float32(midagma_solver* s, int float32) {
  if (!s) return abi_fail(s, MIDAGMA_E_ARG, "null solver");
  return abi_guarded(s, [&] {
    s->set_w_float32(float32 != 0);
    return MIDAGMA_OK;
  });
}

// Test hook (not in the public header): the bytes of every live device and pinned buffer of the
// process (devmem.h), the deliberate log-det workspace cache included.
extern "C" int64_t midagma_debug_live_bytes(void) { return g_live_bytes.load(); }

// Test hook (not in the public header): choose the logistic sigmoid GEMM's form for the next
// set_data (0: the size rule, 1: the one-pass kernel, 2: the serial K split wherever the shape
// allows it; -1: no change).  Returns the form the current data uses (1 or 2).
extern "C" int midagma_debug_sig_split(midagma_solver* s, int mode) {
  if (!s || mode < -1 || mode > 2) return -1;
  if (mode >= 0) s->data.sig_split_force = mode;
  return s->data.sig_split;
}

// The form of the data-mode X^T Y GEMM the current data uses: 1 classical, 2 one level of
// Strassen (0: no data).
int midagma_xty_form(const midagma_solver* s) { return s && s->has_data ? s->data.xty_form : 0; }

// Test hook (not in the public header): choose that form for the next set_data (mode 0: the size
// rule, 1: always classical, 2: Strassen wherever the shape allows it; -1: no change) and the
// split-K of the Strassen products (split 0: the rule's, > 0: at most that many slices; -1: no
// change).  Returns the form the current data uses (1 or 2).
extern "C" int midagma_debug_xty_form(midagma_solver* s, int mode, int split) {
  if (!s || mode < -1 || mode > 2 || split < -1) return -1;
  if (mode >= 0) s->data.xty_form_force = mode;
  if (split >= 0) s->data.xty_split_force = split;
  return s->data.xty_form;
}

// Test hooks (not in the public header) for the hand-back path of the blocked inverse:
// spoil_warm zeroes the stored diagonal-block inverses of the last two slots, so the next fast
// slot's warm start is 0, its residual I, and its first product-form pass hands the slot back
// (ST_NEED_GJ) while the rest of the slot (in data mode: the score GEMMs beside the forked
// inverse) is running; handbacks counts the hand-backs the scheduler has re-run.
extern "C" int midagma_debug_spoil_warm(midagma_solver* s) {
  if (!s || !s->blocked()) return -1;
  return abi_guarded(s, [&] {
    for (DevBuf<>* b : {&s->binv.Pst2, &s->binv.Pst2b})
      if (b->p) HIP_TRY(hipMemsetAsync(b->p, 0, b->n * sizeof(double), s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIDAGMA_OK;
  });
}
extern "C" int64_t midagma_debug_handbacks(const midagma_solver* s) { return s ? s->handback_count : -1; }
// Test hook (not in the public header): the Noda steps a fast cov slot's TCC chain enqueues before
// it hands back (0: the whole gated chain on every slot; < 0: no change).  Returns the old value.
extern "C" int midagma_debug_tcc_fast_steps(midagma_solver* s, int steps) {
  if (!s) return -1;
  const int old = s->knobs.tcc_fast_steps;
  if (steps >= 0 && steps != old) {
    s->knobs.tcc_fast_steps = steps;
    s->graphs.valid = false;
  }
  return old;
}

// Test hook (not in the public header): the TCC fixed-shift stage on (1) or off (0); < 0 leaves
// it.  Returns the old setting.
extern "C" int midagma_debug_tcc_fix(midagma_solver* s, int on) {
  if (!s) return -1;
  const int old = s->knobs.tcc_fix != 0 ? 1 : 0;
  if (on >= 0 && (on != 0 ? 1 : 0) != old) {
    s->knobs.tcc_fix = on != 0 ? 1 : 0;
    s->trek.tcc.w.fix = s->knobs.tcc_fix;
    s->graphs.valid = false;
  }
  return old;
}

// Test hook (not in the public header): the TCC fixed-stage inverse's fast blocks (D2 >= 2048) on (1)
// or off (0) for the next set_trek_tcc; < 0 leaves it.  Returns the old setting.
extern "C" int midagma_debug_tcc_fastblk(midagma_solver* s, int on) {
  if (!s) return -1;
  const int old = s->knobs.tcc_fastblk ? 1 : 0;
  if (on >= 0) s->knobs.tcc_fastblk = on != 0;
  return old;
}

// Test hook (not in the public header): build_at folded into the previous slot's update
// (knobs.at_fold) on (1) or off (0); < 0 leaves it.  Returns the old setting, or -1
// (no handle / the fold cannot apply: not a blocked cov solver).
extern "C" int midagma_debug_at_fold(midagma_solver* s, int on) {
  if (!s || s->begun) return -1;
  const int old = s->knobs.at_fold > 0 ? 1 : 0;
  if (on < 0 || (on != 0) == (old != 0)) return old;
  if (on && !(s->mode == MIDAGMA_MODE_COV && s->blocked())) return -1;
  return abi_guarded(s, [&] {
    if (on && !s->binv.A0.p) s->binv.A0.alloc(s->D * s->D);
    s->knobs.at_fold = on != 0;
    s->graphs.valid = false;
    return old;
  });
}

// Test hook (not in the public header), read-only: the d x d corners of the device W and Mt as
// dense d x d host matrices (either pointer may be null), after the solver's stream and side
// stream have drained.  After a slot Mt holds inv(sI - W∘W)^T of the W that slot started from
// (every inverse path ends in Mt: launch_blocked_inverse's ping-pong starts in
// binv_build_target, so its K2 flips land there, also when outer step 0 read A0; the updates
// only read it) and W the slot's updated W, the next slot's input.  Enqueues no kernel and
// changes no state.  The one-workgroup loop (small.hip) keeps its inverse in registers and has no
// Mt: there Mt is the d x d corner of the first DS x DS image of sprev (row stride DS =
// small_block(d)), the kernel's p1, which every launch writes at its end: the inverse of the W
// its last slot started from, also when that slot halved or reverted.  -1: no handle, or no slot
// run since the last begin (Mt would be stale).
extern "C" int midagma_debug_slot_matrices(midagma_solver* s, double* W_out, double* Mt_out) {
  if (!s || s->bc_len == 0) return -1;  // (bc_len: set by the first begin)
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  if (hipStreamSynchronize(s->stream) != hipSuccess) return -1;
  if (s->side && hipStreamSynchronize(s->side) != hipSuccess) return -1;
  State st{};
  if (hipMemcpy(&st, s->d_state.p, sizeof(State), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (st.slots < 1) return -1;
  const size_t row = (size_t)s->d * sizeof(double), pitch = (size_t)s->D * sizeof(double);
  if (W_out && hipMemcpy2D(W_out, row, s->W.p, pitch, row, s->d, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const bool small = s->small_on();
  if (small && !s->sprev.p) return -1;
  const double* const Mt = small ? s->sprev.p : s->Mt.p;
  const size_t mpitch = small ? (size_t)small_block(s->d) * sizeof(double) : pitch;
  if (Mt_out && hipMemcpy2D(Mt_out, row, Mt, mpitch, row, s->d, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return 0;
}

// Diagnostics of the fast blocked inverse (not in the public header): per outer block g,
// out[g*(NM_PASSES+2) + 0] = done word, out[... + 1 + p] = ||Q_p||_inf of pass p (stale for
// passes that did not run in the last slot).
extern "C" int midagma_debug_blocked(midagma_solver* s, double* out, int64_t cap) {
  if (!s || !s->blocked()) return 0;
  const int B2 = s->binv.B2, NT = B2 / 16;
  const int64_t K2 = s->D / B2, per = NM_PASSES + 2;
  if (cap < K2 * per) return -1;
  std::vector<double> part((size_t)K2 * (NM_PASSES + 1) * PART_STRIDE);
  std::vector<int> done(K2);
  if (hipMemcpy(part.data(), s->binv.nmPart.p, part.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  if (hipMemcpy(done.data(), s->binv.nmDone.p, K2 * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  for (int64_t g = 0; g < K2; ++g) {
    out[g * per] = done[g];
    for (int p = 0; p <= NM_PASSES; ++p) {
      const double* rp = part.data() + ((size_t)g * (NM_PASSES + 1) + p) * PART_STRIDE;
      double m = 0.0;
      for (int r = 0; r < B2; ++r) {
        double acc = 0.0;
        for (int t = 0; t < NT; ++t) acc += rp[r * NT + t];
        m = std::max(m, acc);
      }
      out[g * per + 1 + p] = m;
    }
  }
  return (int)K2;
}

int64_t midagma_checkpoints(midagma_solver* s, midagma_ckpt* out, int64_t cap) {
  if (!s || !s->d_ckpt.p) return 0;
  int64_t n = 0;
  int rc = abi_guarded(s, [&] {
    State st{};
    HIP_TRY(hipMemcpy(&st, s->d_state.p, sizeof(State), hipMemcpyDeviceToHost));
    n = std::min<int64_t>(std::min<int64_t>(st.n_ckpt, s->ckpt_cap), cap);
    static_assert(sizeof(midagma_ckpt) == sizeof(CkptRec), "ckpt layout");
    if (n > 0 && out) HIP_TRY(hipMemcpy(out, s->d_ckpt.p, n * sizeof(CkptRec), hipMemcpyDeviceToHost));
    return MIDAGMA_OK;
  });
  return rc == MIDAGMA_OK ? n : rc;
}

int midagma_set_trek(midagma_solver* s, int seq, int agg, int mode, double weight, double eps_inv, int64_t K,
                     const int64_t* pairs, int64_t m) {
  if (!s || (m > 0 && !pairs) || m < 0) return abi_fail(s, MIDAGMA_E_ARG, "set_trek: bad arguments");
  return abi_guarded(s, [&] {
    s->set_trek(seq, agg, mode, weight, eps_inv, K, pairs, m);
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIDAGMA_OK;
  });
}

int midagma_set_trek_tcc(midagma_solver* s, int mode, double weight, double w, double eps, const int64_t* pairs,
                         int64_t m) {
  if (!s || (m > 0 && !pairs) || m < 0) return abi_fail(s, MIDAGMA_E_ARG, "set_trek_tcc: bad arguments");
  return abi_guarded(s, [&] {
    s->set_trek_tcc(mode, weight, w, eps, pairs, m);
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIDAGMA_OK;
  });
}

int midagma_trek(midagma_solver* s, const double* W, double* value, double* G) {
  if (!s || !W || !value) return abi_fail(s, MIDAGMA_E_ARG, "trek: null argument");
  if (!all_finite(W, s->d, s->d, s->d)) return abi_fail(s, MIDAGMA_E_ARG, std::string("trek: ") + kNonFinite);
  return abi_guarded(s, [&] {
    s->eval_trek(W, value, G);
    return MIDAGMA_OK;
  });
}

int midagma_h(midagma_solver* s, const double* W, double s_dom, double* h, double* G) {
  if (!s || !W || !h) return abi_fail(s, MIDAGMA_E_ARG, "h: null argument");
  if (!all_finite(W, s->d, s->d, s->d)) return abi_fail(s, MIDAGMA_E_ARG, std::string("h: ") + kNonFinite);
  return abi_guarded(s, [&] {
    s->eval_h(W, s_dom, h, G);
    return MIDAGMA_OK;
  });
}

int midagma_score(midagma_solver* s, const double* W, double* loss, double* G) {
  if (!s || !W || !loss) return abi_fail(s, MIDAGMA_E_ARG, "score: null argument");
  if (s->mode != MIDAGMA_MODE_COV || !s->has_cov) return abi_fail(s, MIDAGMA_E_STATE, "score: cov mode with set_cov");
  return abi_guarded(s, [&] {
    s->eval_score(W, loss, G);
    return MIDAGMA_OK;
  });
}

int midagma_score_partial(midagma_solver* s, const double* W) {
  if (!s || !W || s->mode != MIDAGMA_MODE_DATA || !s->has_data)
    return abi_fail(s, MIDAGMA_E_STATE, "score_partial: data mode with set_data");
  return abi_guarded(s, [&] {
    s->score_partial(W);
    return MIDAGMA_OK;
  });
}

int midagma_score_finish(midagma_solver* s, double* loss, double* G) {
  if (!s || !loss || s->mode != MIDAGMA_MODE_DATA) return abi_fail(s, MIDAGMA_E_STATE, "score_finish: data mode");
  return abi_guarded(s, [&] {
    s->score_finish(loss, G);
    return MIDAGMA_OK;
  });
}

}  // extern "C"

#ifdef MIDAGMA_EXPERIMENTS
// Diagnostics (not part of the ABI header): the one-launch inverse's task plan for D, passes
// and nwg workgroups, as planned on the host (no GPU needed).  tasks (12 ints per task, grouped
// by workgroup) and woff (nwg + 1) may be null to query the sizes.  Returns 0, or -1.
extern "C" int midagma_debug_df_plan(int64_t D, int passes, int nwg, double* est_us, int64_t* ntasks, int* tasks,
                                     int* woff, int* nctr) {
  try {
    if (!df_available(D) || (passes != 2 && passes != 3) || nwg < 1) return -1;
    const DfPlanHost p = df_plan(D, passes, nwg);
    if (est_us) *est_us = p.est_us;
    if (ntasks) *ntasks = (int64_t)(p.tasks->size() / 12);
    if (nctr) *nctr = p.nctr;
    if (tasks) std::memcpy(tasks, p.tasks->data(), p.tasks->size() * sizeof(int));
    if (woff) std::memcpy(woff, p.woff->data(), p.woff->size() * sizeof(int));
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "midagma_debug_df_plan: %s\n", e.what());
    return -1;
  }
}

// Diagnostics: the one-launch inverse's per-task timestamps of the last launch (3 per task in
// plan order: wait start, go, done; 100 MHz ticks), with MIDAGMA_DF_STAMPS set at create.
// Returns the number of values copied, or -1.
extern "C" int64_t midagma_debug_df_stamps(midagma_solver* s, unsigned long long* out, int64_t cap) {
  if (!s || !s->df.w.stamps) return -1;
  const int64_t n = std::min<int64_t>(cap, (int64_t)s->df.Stamps.n);
  if (hipStreamSynchronize(s->stream) != hipSuccess) return -1;
  if (hipMemcpy(out, s->df.Stamps.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return n;
}
#endif  // MIDAGMA_EXPERIMENTS
