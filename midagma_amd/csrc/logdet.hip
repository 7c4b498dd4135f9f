// The log-det of sI - A and its inverse on device pointers for torch (DagmaMLP.h_func): the
// midagma_logdet_* entries over a per-device workspace cache, and the midagma_ldfast handle, the
// h log-det's warm-started fast path (its kernels: mlp.hip, gj.hip).  Host code only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "../../include/midagma_hip.h"
#include "devmem.h"
#include "launch.h"

using namespace midagma;

namespace {
struct LogdetWorkspace {
  int device = -1;
  int64_t D = 0;
  DevBuf<> A, P, R, C, piv;
};
std::mutex g_ws_mu;
// The per-device cache, kept for the life of the process.  Pointers that are never deleted, on
// purpose: an owning object with static storage would free its buffers from a static destructor,
// when the HIP runtime may already be gone (devmem.h).
std::vector<LogdetWorkspace*> g_ws;
}  // namespace

// the workspace of padded size D for the current device, created on first use (g_ws_mu held)
static LogdetWorkspace* logdet_ws(int64_t D) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  for (auto* w : g_ws)
    if (w->device == dev && w->D == D) return w;
  LogdetWorkspace* ws = new LogdetWorkspace();
  ws->device = dev;
  ws->D = D;
  ws->A.alloc((size_t)D * D);
  ws->P.alloc(64 * 64);
  ws->R.alloc((size_t)64 * D);
  ws->C.alloc((size_t)D * 64);
  ws->piv.alloc(D);
  g_ws.push_back(ws);
  return ws;
}

// the h log-det's: 32-padded, the 32-block Gauss-Jordan's own granularity
static LogdetWorkspace* logdet_h_ws(int64_t d) {
  std::lock_guard<std::mutex> lock(g_ws_mu);
  return logdet_ws((d + 31) / 32 * 32);
}

// part 0: build + the Gauss-Jordan prologue; parts 1 .. D/32: its block steps; part D/32 + 1: the
// epilogue (h and (sI - A)^-T).  part < 0: all of them.
static void logdet_h_enqueue(const double* A, int64_t d, int64_t lda, double s, double* h_dev, double* Mt_dev,
                             int64_t ldm, hipStream_t st, int part) {
  setup_attributes();
  LogdetWorkspace* ws = logdet_h_ws(d);
  const int64_t D = ws->D;
  const int K = (int)(D / 32);
  const GJWork w{ws->P.p, ws->R.p, ws->C.p, ws->piv.p};
  if (part < 0 || part == 0) {
    launch_build_at(A, lda, false, ws->A.p, D, d, s, nullptr, nullptr, st);
    launch_gj_prologue(ws->A.p, D, D, w, nullptr, st);
  }
  for (int k = 0; k < K; ++k)
    if (part < 0 || part == k + 1) launch_gj_step(ws->A.p, D, D, w, nullptr, k, st);
  if (part < 0 || part == K + 1)
    launch_logdet_post(ws->piv.p, d, (double)d * std::log(s), h_dev, ws->A.p, D, Mt_dev, ldm, st);
}

extern "C" int midagma_logdet_h_dev(const double* A, int64_t d, int64_t lda, double s, double* h_dev, double* Mt_dev,
                                    int64_t ldm, void* stream) {
  if (!A || !h_dev || d < 1 || lda < d || !(s > 0.0) || (Mt_dev && ldm < d))
    return abi_fail(nullptr, MIDAGMA_E_ARG, "logdet_h_dev: bad arguments");
  return abi_guarded(nullptr, [&] {
    logdet_h_enqueue(A, d, lda, s, h_dev, Mt_dev, ldm, reinterpret_cast<hipStream_t>(stream), -1);
    return MIDAGMA_OK;
  });
}

extern "C" int64_t midagma_logdet_h_parts(int64_t d) { return d < 1 ? 0 : (d + 31) / 32 + 2; }

// ---- the h log-det's warm-started fast path (ABI 6; mlp.hip) -------------------------------------
struct midagma_ldfast {
  int device = 0;
  int64_t d = 0, Dgj = 0;  // Gauss-Jordan workspace: 32-padded, as midagma_logdet_h_dev
  int B = 0;               // series block: 128 or 256 (0: d > 256, every step exact)
  DevBuf<> ring0, ring1, Y0, Y1, Q0, Q1, P, part, done, hlast;
  DevBuf<> A, Pgj, Rgj, Cgj, piv;
  DevBuf<State> st;    // the ring's state (slots: step index; warm_run; status of the series)
  DevBuf<State> gjst;  // the Gauss-Jordan gate of a fast step (ST_RUNNING: run the chain)
  int64_t* counter = nullptr;  // advanced by a fast step's end (midagma_ldfast_set_counter)
  std::string err;
  GJWork gjw() const { return GJWork{Pgj.p, Rgj.p, Cgj.p, piv.p}; }
  SeriesWork sw() const {
    return SeriesWork{ring0.p, ring1.p, {Y0.p, Y1.p}, {Q0.p, Q1.p}, P.p, part.p, reinterpret_cast<int*>(done.p)};
  }
};

extern "C" int midagma_ldfast_create(midagma_ldfast** out, int64_t d) {
  if (!out || d < 1) return abi_fail(nullptr, MIDAGMA_E_ARG, "ldfast_create: bad arguments");
  auto* h = new midagma_ldfast();
  int rc = abi_guarded(nullptr, [&] {
    setup_attributes();
    HIP_TRY(hipGetDevice(&h->device));
    h->d = d;
    h->Dgj = (d + 31) / 32 * 32;
    h->B = d <= 128 ? 128 : (d <= 256 ? 256 : 0);
    const size_t DD = (size_t)h->Dgj * h->Dgj;
    h->A.alloc(DD);
    h->Pgj.alloc(64 * 64);
    h->Rgj.alloc((size_t)64 * h->Dgj);
    h->Cgj.alloc((size_t)h->Dgj * 64);
    h->piv.alloc(h->Dgj);
    h->hlast.alloc(1);
    if (h->B) {
      const size_t BB = (size_t)h->B * h->B;
      for (DevBuf<>* b : {&h->ring0, &h->ring1, &h->Y0, &h->Y1, &h->Q0, &h->Q1, &h->P}) b->alloc(BB);
      h->part.alloc((size_t)(NM_PASSES + 1) * PART_STRIDE);
      h->done.alloc(1);
    }
    h->st.alloc(1);
    h->gjst.alloc(1);
    return midagma_ldfast_reset(h);
  });
  if (rc != MIDAGMA_OK) {
    delete h;
    return rc;
  }
  *out = h;
  return MIDAGMA_OK;
}

extern "C" void midagma_ldfast_destroy(midagma_ldfast* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  delete h;
}

extern "C" int midagma_ldfast_reset(midagma_ldfast* h) {
  if (!h) return abi_fail(nullptr, MIDAGMA_E_ARG, "ldfast_reset: null handle");
  return abi_guarded(nullptr, [&] {
    HIP_TRY(hipSetDevice(h->device));
    State st{};
    st.status = ST_RUNNING;
    st.slots = -1;        // step 0: opened by ldfast_begin (exact) or counted by the fast step's end
    st.ckpt_pending = 1;  // no warm start: the first step runs the Gauss-Jordan chain
    State gj{};
    gj.status = ST_DONE;
    HIP_TRY(hipMemcpy(h->st.p, &st, sizeof(State), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->gjst.p, &gj, sizeof(State), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(h->hlast.p, 0, sizeof(double)));
    if (h->done.p) HIP_TRY(hipMemset(h->done.p, 0, sizeof(double)));
    return MIDAGMA_OK;
  });
}

// fast: 0 the series residual (opening the step), 1 .. 3 the passes, 4 certificate + the gated
// chain with the step's end; exact: 0 begin + build + prologue, 1 .. Dgj/32 the block steps, last
// the end
static constexpr int kLdfastPasses = 3;
extern "C" int64_t midagma_ldfast_parts(const midagma_ldfast* h, int exact) {
  if (!h) return 0;
  return (exact || !h->B) ? h->Dgj / 32 + 2 : kLdfastPasses + 2;
}

extern "C" int midagma_ldfast_enqueue(midagma_ldfast* h, const double* A, int64_t d_in, int64_t lda, double s,
                                      double* h_dev, double* Mt_dev, int64_t ldm, void* stream, int exact, int64_t part) {
  if (!h || d_in != h->d)  // the handle's buffers and warm-start ring are sized for its d
    return abi_fail(nullptr, MIDAGMA_E_ARG, "ldfast_enqueue: A's d differs from the handle's");
  if (!A || !h_dev || !Mt_dev || lda < h->d || ldm < h->d || !(s > 0.0) || part >= midagma_ldfast_parts(h, exact))
    return abi_fail(nullptr, MIDAGMA_E_ARG, "ldfast_enqueue: bad arguments");
  return abi_guarded(nullptr, [&] {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t d = h->d, D = h->Dgj;
    const int K = (int)(D / 32);
    const double dls = (double)d * std::log(s);
    const bool ex = exact || !h->B;
    auto want = [&](int64_t p) { return part < 0 || part == p; };
    if (ex) {  // the Gauss-Jordan chain, ungated
      if (want(0)) {
        launch_ldfast_begin(h->st.p, h->gjst.p, st);
        launch_build_at(A, lda, false, h->A.p, D, d, s, nullptr, nullptr, st);
        launch_gj_prologue(h->A.p, D, D, h->gjw(), nullptr, st);
      }
      for (int k = 0; k < K; ++k)
        if (want(k + 1)) launch_gj_step(h->A.p, D, D, h->gjw(), nullptr, k, st);
      if (want(K + 1))
        launch_ldfast_post(h->piv.p, d, dls, h_dev, h->A.p, D, Mt_dev, ldm, h->P.p, h->B, h->ring0.p, h->ring1.p,
                           h->st.p, h->gjst.p, h->hlast.p, true, st);
      return MIDAGMA_OK;
    }
    const SeriesWork w = h->sw();
    if (want(0)) launch_ldfast_resid(A, lda, d, s, h->B, w, h->st.p, h->gjst.p, st);
    // the passes one by one (each its own part: the caller interleaves them)
    for (int p = 1; p <= kLdfastPasses; ++p)
      if (want(p)) launch_series_pass(h->B, w, h->st.p, p, st);
    if (want(kLdfastPasses + 1)) {
      launch_ldfast_certify(h->P.p, h->B, d, Mt_dev, ldm, h->st.p, reinterpret_cast<const int*>(h->done.p), h->gjst.p,
                            h->ring0.p, h->ring1.p, st);
      // gated: opened by the certificate.  One launch, the whole Gauss-Jordan chain in one
      // workgroup (bit-identical; slow when open, which the bench window never is): a closed gate
      // costs one launch instead of the chain's 2 + D/32, and that launch also ends the step
      // (ldfast_post's fast-step work in the same workgroup: one dependent launch fewer)
      const LdfastEnd end{h->piv.p, d, dls, h_dev, Mt_dev, ldm, h->B, h->ring0.p, h->ring1.p, h->st.p, h->hlast.p,
                          h->counter};
      launch_gj_inverse_1wg(A, lda, h->A.p, D, d, s, h->gjw(), h->gjst.p, st, end);
    }
    return MIDAGMA_OK;
  });
}

extern "C" int midagma_ldfast_set_counter(midagma_ldfast* h, int64_t* counter) {
  if (!h) return abi_fail(nullptr, MIDAGMA_E_ARG, "ldfast_set_counter: null handle");
  // a handle without the fast path (d > 256: every step runs the Gauss-Jordan chain, which never
  // advances the counter) cannot honour the contract: refuse instead of stalling the caller's table
  if (counter && !h->B)
    return abi_fail(nullptr, MIDAGMA_E_ARG, "ldfast_set_counter: the handle has no fast path (d > 256)");
  h->counter = counter;
  return MIDAGMA_OK;
}

extern "C" int midagma_ldfast_stats(midagma_ldfast* h, int64_t* steps, int64_t* exact_steps) {
  if (!h) return abi_fail(nullptr, MIDAGMA_E_ARG, "ldfast_stats: null handle");
  return abi_guarded(nullptr, [&] {
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    State st{};
    HIP_TRY(hipMemcpy(&st, h->st.p, sizeof(State), hipMemcpyDeviceToHost));
    if (steps) *steps = st.iter;
    if (exact_steps) *exact_steps = st.halvings;
    return MIDAGMA_OK;
  });
}

extern "C" int midagma_logdet_h_dev_part(const double* A, int64_t d, int64_t lda, double s, double* h_dev,
                                         double* Mt_dev, int64_t ldm, void* stream, int64_t part) {
  if (!A || !h_dev || d < 1 || lda < d || !(s > 0.0) || (Mt_dev && ldm < d) || part < 0 ||
      part >= midagma_logdet_h_parts(d))
    return abi_fail(nullptr, MIDAGMA_E_ARG, "logdet_h_dev_part: bad arguments");
  return abi_guarded(nullptr, [&] {
    logdet_h_enqueue(A, d, lda, s, h_dev, Mt_dev, ldm, reinterpret_cast<hipStream_t>(stream), (int)part);
    return MIDAGMA_OK;
  });
}

extern "C" int midagma_logdet_inv_dev(const double* A, int64_t d, int64_t lda, double s_dom, double* logdet_dev,
                                      double* Mt_dev, int64_t ldm, void* stream) {
  if (!A || d < 1 || lda < d || (Mt_dev && ldm < d))
    return abi_fail(nullptr, MIDAGMA_E_ARG, "logdet_inv_dev: bad arguments");
  return abi_guarded(nullptr, [&] {
    setup_attributes();
    const int64_t D = round_up64(d);
    std::lock_guard<std::mutex> lock(g_ws_mu);
    LogdetWorkspace* ws = logdet_ws(D);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    launch_build_at(A, lda, false, ws->A.p, D, d, s_dom, nullptr, nullptr, st);
    launch_gj_inverse(ws->A.p, D, D, GJWork{ws->P.p, ws->R.p, ws->C.p, ws->piv.p}, nullptr, st);
    if (logdet_dev) launch_sum_vector(ws->piv.p, d, logdet_dev, nullptr, st);
    if (Mt_dev)
      HIP_TRY(hipMemcpy2DAsync(Mt_dev, ldm * sizeof(double), ws->A.p, D * sizeof(double), d * sizeof(double), d,
                               hipMemcpyDeviceToDevice, st));
    return MIDAGMA_OK;
  });
}
