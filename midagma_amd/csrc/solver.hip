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
  s->loss = loss;
  s->mode = mode;
  s->d = d;
  // 128-multiples feed the 128x128 GEMM tiles.  Cov mode pads 129 <= d <= 192 to 256 as well: the
  // blocked inverse then has one 256-wide outer block, and its warm-started product form beats
  // the flat Gauss-Jordan's 6 block steps on 192 (data mode keeps 192: X's columns are GEMM work)
  const bool pad256 = mode == MIDAGMA_MODE_COV && knob("MIDAGMA_EXP_COV_PAD256", 1) != 0;
  s->D = d > 192 || (pad256 && d > 128) ? (d + 127) / 128 * 128 : round_up64(d);
  // Cov mode, 256 < d <= 640: D to a multiple of 256, so the blocked inverse runs B2 = 256 outer
  // blocks (2 instead of 3 at D = 384 -> 512, 3 instead of 5 at 640 -> 768: d=300 11.1k -> 11.3k,
  // d=600 6.4k -> 7.0k steps/s).  Larger D keep B2 = 128 (d=1150 even, d=1400 -3.5%, d=1700
  // even: the padded GEMM work outweighs the saved outer steps).  Knob MIDAGMA_EXP_COV_PAD_B2:
  // 0 off, 1 at every d > 256.
  const int pad_b2 = (int)knob("MIDAGMA_EXP_COV_PAD_B2", -1);
  if (mode == MIDAGMA_MODE_COV && d > 256 && (pad_b2 == 1 || (pad_b2 < 0 && d <= 640)))
    s->D = (d + 255) / 256 * 256;
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
    const size_t DD = (size_t)s->D * s->D;
    const bool inc = mask_inc != nullptr, exc = mask_exc != nullptr;
    if (inc) {
      s->minc.alloc(DD);
      HIP_TRY(hipMemsetAsync(s->minc.p, 0, DD * sizeof(double), s->stream));
      s->upload_matrix(s->minc, mask_inc, s->d);
    }
    if (exc) {
      s->mexc.alloc(DD);
      HIP_TRY(hipMemsetAsync(s->mexc.p, 0, DD * sizeof(double), s->stream));
      s->upload_matrix(s->mexc, mask_exc, s->d);
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    const double* pi = inc ? s->minc.p : nullptr;
    const double* pe = exc ? s->mexc.p : nullptr;
    if (pi != s->cap_minc || pe != s->cap_mexc) s->graphs_valid = false;  // captured pointers changed
    s->cap_minc = pi;
    s->cap_mexc = pe;
    s->has_inc = inc;
    s->has_exc = exc;
    return MIDAGMA_OK;
  });
}

int midagma_set_data(midagma_solver* s, const double* X, int64_t n_local, int64_t n_global, int on_device) {
  if (!s || !X || n_local < 1 || n_global < n_local || s->mode != MIDAGMA_MODE_DATA)
    return abi_fail(s, MIDAGMA_E_ARG, "set_data: bad arguments (data mode only)");
  if (!on_device && !all_finite(X, n_local, s->d, s->d))
    return abi_fail(s, MIDAGMA_E_ARG, std::string("set_data: ") + kNonFinite);
  return abi_guarded(s, [&] {
    const int64_t D = s->D;
    s->n_local = n_local;
    s->n_global = n_global;
    s->n_pad = (n_local + 127) / 128 * 128;
    const size_t nx = (size_t)s->n_pad * D;
    // experiments build: MIDAGMA_EXP_PREPAD_MB of device memory allocated (and kept) before X, to
    // move X, X^T and Y elsewhere (the X^T Y GEMM's fetched bytes against placement)
    if (const long pad = knob("MIDAGMA_EXP_PREPAD_MB", 0); pad > 0 && !s->prepad.p)
      s->prepad.alloc((size_t)pad << 17);
    s->X.alloc(nx);
    // logistic with few 128-tiles: the sigmoid GEMM in two serial K halves when its last round of
    // tiles would be at most half full (n = 1e4, d = 1000: 632 tiles for 512 resident slots)
    const int64_t sig_tiles = (s->n_pad / 128) * (D / 128);
    const int sig_rule = (int)knob("MIDAGMA_EXP_SIG_SPLIT", 1);
    const bool sig_ok = s->loss == MIDAGMA_LOSS_LOGISTIC && D % 128 == 0 && sig_tiles % 8 == 0;
    s->sig_split = sig_ok && sig_rule > 0 && sig_tiles < 2048 && sig_tiles % 512 != 0 && sig_tiles % 512 <= 256 ? 2 : 1;
    if (s->sig_split_force == 1) s->sig_split = 1;  // midagma_debug_sig_split (tests)
    if (s->sig_split_force == 2 && sig_ok) s->sig_split = 2;
    if (s->sig_split == 2) {  // the output, the first halves' partial, then one flag word per tile
      s->Y.alloc(2 * nx + (size_t)(sig_tiles + 1) / 2);
      HIP_TRY(hipMemsetAsync(s->Y.p + 2 * nx, 0, (size_t)(sig_tiles + 1) / 2 * sizeof(double), s->stream));
    } else {
      // experiments build: Y placed MIDAGMA_EXP_Y_OFFSET bytes into its allocation (L2 set
      // aliasing between X and Y in the X^T Y GEMM)
      s->Y.alloc_shifted(nx, (size_t)knob("MIDAGMA_EXP_Y_OFFSET", 0) / sizeof(double));
    }
    HIP_TRY(hipMemsetAsync(s->X.p, 0, nx * sizeof(double), s->stream));
    HIP_TRY(hipMemcpy2DAsync(s->X.p, D * sizeof(double), X, s->d * sizeof(double), s->d * sizeof(double), n_local,
                             on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
    if (on_device) {  // the host path checked before the copy
      int* flag = reinterpret_cast<int*>(s->partials.p);
      launch_any_nonfinite(s->X.p, (int64_t)nx, flag, s->stream);
      int bad = 0;
      HIP_TRY(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      if (bad) throw std::invalid_argument(std::string("set_data: ") + kNonFinite);
    }
    size_t mem_free = 0, mem_total = 0;
    HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
    // (the 128-tile GEMM only: D % 128 == 0; smaller problems are not worth the copy)
    s->use_xt = getenv("MIDAGMA_NO_XT") == nullptr && D % 128 == 0 &&
                mem_free > nx * sizeof(double) + (size_t(2) << 30);
    if (s->use_xt) {
      s->XT.alloc(nx);
      launch_transpose(s->X.p, D, s->n_pad, D, s->XT.p, s->n_pad, s->stream);
    } else {
      s->XT.release();
    }
    if (s->loss == MIDAGMA_LOSS_L2 && (D % 128 == 0 || s->w32))  // (float32 W: I - W from build_at)
      s->IW.alloc((size_t)D * D);
    else
      s->IW.release();
    // split-K over the rows so the X^T Y GEMM fills the chip: (D/64)^2 tiles x split >= ~1024 workgroups
    const int64_t tiles = (D % 128 == 0) ? (D / 128) * (D / 128) : (D / 64) * (D / 64);
    const int64_t ktiles = s->n_pad / 64;
    int split = (int)std::max<int64_t>(1, std::min<int64_t>(ktiles / 8, (1024 + tiles - 1) / tiles));
    s->split = std::min(split, 32);
    if (knob_set("MIDAGMA_EXP_DATA_SPLIT")) s->split = (int)knob("MIDAGMA_EXP_DATA_SPLIT", s->split);
    if (s->split > 1) s->Zparts.alloc((size_t)s->split * D * D);
    // X^T Y by one level of Strassen (gemm.hip): when the shape allows it (D % 256 == 0), every
    // product's K slice is long enough to amortise its tile's prologue and epilogue
    // (kXtyStrassenMinSlice), and the device has room for the five operand sums of X (1.25 x the
    // size of X; the same free-memory rule as X^T).  Everything else keeps the classical GEMM.
    s->xty_form = 1;
    bool strassen = s->xty_form_force != 1 && xty_strassen_shape(D, s->n_pad) && !knob_set("MIDAGMA_EXP_DATA_SPLIT");
    XtyStrassenPlan plan{};
    if (strassen) {
      plan = xty_strassen_plan(D, s->n_pad, s->xty_split_force);
      if (s->xty_form_force != 2 && plan.kslice < kXtyStrassenMinSlice) strassen = false;
    }
    if (strassen) {
      const size_t nsum = (size_t)xty_strassen_sum_count(D, s->n_pad);
      HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
      strassen = mem_free > nsum * sizeof(double) + (size_t(2) << 30);
      if (strassen) {
        try {
          s->Xsums.alloc(nsum);
          s->Sparts.alloc((size_t)xty_strassen_part_count(D, plan.nsplit));
        } catch (const HipError& e) {
          if (e.code != hipErrorOutOfMemory) throw;
          (void)hipGetLastError();
          strassen = false;
        }
      }
    }
    if (strassen) {
      launch_xty_strassen_sums(s->X.p, D, s->n_pad, s->Xsums.p, s->stream);
      s->xty_form = 2;
      s->xty_split = s->xty_split_force;
    } else {
      s->Xsums.release();
      s->Sparts.release();
    }
    s->loss_part_count = (s->n_pad / 64) * (D / 64);
    // small shards run the cov-mode slot structure: the warm-started fast blocked inverse in
    // sequence with the GEMMs (hand-backs and checkpoint slots on the pivoted path).  Forked beside
    // GEMMs that fill the chip, the pivoted inverse's 20-odd dependent launches wait for CU slots
    // and end after the GEMMs (logistic d=1000, n=1e4: 1.01 ms per slot for 0.70 ms of GEMMs);
    // large shards keep the fork, which hides it (MIDAGMA_EXP_DATA_FAST_ROWS: the row bound)
    static const int64_t fast_rows = knob("MIDAGMA_EXP_DATA_FAST_ROWS", 16384);
    const int b2 = binv_block(D);
    const int B2_new = (b2 > 0 && s->n_pad <= fast_rows && s->Malt.p) ? b2 : 0;
    if (B2_new != s->B2) s->graphs_valid = false;
    s->B2 = B2_new;
    if (s->loss == MIDAGMA_LOSS_LOGISTIC) {
      s->loss_part.alloc(s->loss_part_count);
      HIP_TRY(hipMemsetAsync(s->loss_part.p, 0, s->loss_part_count * sizeof(double), s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->has_data = true;
    s->graphs_valid = false;
    return MIDAGMA_OK;
  });
}

int midagma_data_gram(midagma_solver* s) {
  if (!s || !s->has_data) return abi_fail(s, MIDAGMA_E_STATE, "data_gram: set_data first");
  return abi_guarded(s, [&] {
    GemmSpec gs = s->xty_spec();  // X^T X: the X^T Y GEMM with Y = X
    gs.B = s->X.p;
    launch_gemm_summed(gs, s->Zparts.p, s->zbuf, nullptr, s->stream);
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
    HIP_TRY(hipStreamSynchronize(s->stream));
    comm_destroy(s->comm);
    s->comm = nullptr;
    s->comm = comm_create(id, nranks, rank);
    s->comm_ranks = nranks;
    s->agree.alloc(8);
    s->h_agree.alloc(8);
    s->graphs_valid = false;  // the slot graphs now carry the all-reduce
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
    s->graphs_valid = false;
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
    if (s->blocked()) {
      s->drive_blocked(n);
      return MIDAGMA_OK;
    }
    if (s->small_on()) {
      s->drive_small(n);
      return MIDAGMA_OK;
    }
    for (int64_t i = 0; i < n; ++i) HIP_TRY(hipGraphLaunch(s->g_full, s->stream));
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
    Event a, b;
    a.create();
    b.create();
    auto timed = [&](auto&& body) {
      HIP_TRY(hipEventRecord(a, s->stream));
      for (int r = 0; r < reps; ++r) body();
      HIP_TRY(hipEventRecord(b, s->stream));
      HIP_TRY(hipEventSynchronize(b));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, a, b));
      return (double)ms / reps;
    };
    const int64_t D = s->D;
    // [0] build (sI - W o W)^T   [1] GJ inverse   [2] score GEMM(s)   [3] whole slot (graph)
    // data mode: [4] Y = X (I - W) GEMM   [5] Z = X^T Y GEMM (+ slice sum)
    ms_out[0] = timed([&] { launch_build_at(s->W.p, D, true, s->Mt.p, D, s->d, 0.0, s->d_params.p, s->d_state.p,
                                            s->stream, s->IW.p); });
    ms_out[1] = timed([&] { launch_gj_inverse(s->Mt.p, D, D, s->gj(), s->d_state.p, s->stream); });
    if (s->mode == MIDAGMA_MODE_COV) {
      ms_out[2] = timed([&] { s->enqueue_score_cov(s->zbuf, s->d_state.p, true); });
      ms_out[4] = ms_out[5] = 0.0;
    } else {
      ms_out[2] = timed([&] { s->enqueue_data_partial(s->W.p, s->d_state.p, s->IW.p); });
      ms_out[4] = timed([&] { s->enqueue_xw(s->W.p, s->d_state.p, s->IW.p); });
      ms_out[5] = timed([&] { s->enqueue_xty(s->d_state.p); });
    }
    ms_out[3] = timed([&] { HIP_TRY(hipGraphLaunch(s->g_full, s->stream)); });
    ms_out[6] = ms_out[7] = 0.0;
    if (s->blocked()) {
      // [6] build + fast blocked inverse, less [0]   [7] whole fast slot (graph).  Both need a
      // warm start and no pending checkpoint: one slow slot first.
      HIP_TRY(hipGraphLaunch(s->g_full, s->stream));
      ms_out[6] = timed([&] { s->enqueue_build_inverse(/*fast=*/true, 2); }) - ms_out[0];
      ms_out[7] = timed([&] { HIP_TRY(hipGraphLaunch(s->g_fast, s->stream)); });
      State st{};
      HIP_TRY(hipMemcpy(&st, s->d_state.p, sizeof(State), hipMemcpyDeviceToHost));
      if (st.status == ST_NEED_GJ) {  // the fast path did not run: report it, leave a clean state
        ms_out[6] = ms_out[7] = -1.0;
        static const int32_t running = ST_RUNNING;
        HIP_TRY(hipMemcpy(&s->d_state.p->status, &running, sizeof(int32_t), hipMemcpyHostToDevice));
        s->fast_ready = false;
      }
    }
    return MIDAGMA_OK;
  });
}

int midagma_step_partial(midagma_solver* s) {
  if (!s || !s->begun) return abi_fail(s, MIDAGMA_E_STATE, "step_partial: call begin first");
  return abi_guarded(s, [&] {
    HIP_TRY(hipGraphLaunch(s->g_part1, s->stream));
    return MIDAGMA_OK;
  });
}

int midagma_step_finish(midagma_solver* s) {
  if (!s || !s->begun) return abi_fail(s, MIDAGMA_E_STATE, "step_finish: call begin first");
  return abi_guarded(s, [&] {
    HIP_TRY(hipGraphLaunch(s->g_part2, s->stream));
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
    const bool on = float32 != 0;
    if (on != s->w32) s->graphs_valid = false;  // the float32 slots carry numpy's L1 sum
    if (on && !s->l1w.p) s->l1w.alloc((size_t)(1 + (np_l1_chunks(s->d) + 1) / 2));
    if (on && (s->mode == MIDAGMA_MODE_COV || s->loss == MIDAGMA_LOSS_L2) && !s->IW.p) {
      // the score GEMM's I - W (float32 diagonal) comes from build_at, not the GEMM's staging
      s->IW.alloc((size_t)s->D * s->D);
      HIP_TRY(hipMemsetAsync(s->IW.p, 0, (size_t)s->D * s->D * sizeof(double), s->stream));
      s->graphs_valid = false;
    }
    s->w32 = on;
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
  if (mode >= 0) s->sig_split_force = mode;
  return s->sig_split;
}

// The form of the data-mode X^T Y GEMM the current data uses: 1 classical, 2 one level of
// Strassen (0: no data).
int midagma_xty_form(const midagma_solver* s) { return s && s->has_data ? s->xty_form : 0; }

// Test hook (not in the public header): choose that form for the next set_data (mode 0: the size
// rule, 1: always classical, 2: Strassen wherever the shape allows it; -1: no change) and the
// split-K of the Strassen products (split 0: the rule's, > 0: at most that many slices; -1: no
// change).  Returns the form the current data uses (1 or 2).
extern "C" int midagma_debug_xty_form(midagma_solver* s, int mode, int split) {
  if (!s || mode < -1 || mode > 2 || split < -1) return -1;
  if (mode >= 0) s->xty_form_force = mode;
  if (split >= 0) s->xty_split_force = split;
  return s->xty_form;
}

// Test hooks (not in the public header) for the hand-back path of the blocked inverse:
// spoil_warm zeroes the stored diagonal-block inverses of the last two slots, so the next fast
// slot's warm start is 0, its residual I, and its first product-form pass hands the slot back
// (ST_NEED_GJ) while the rest of the slot (in data mode: the score GEMMs beside the forked
// inverse) is running; handbacks counts the hand-backs the scheduler has re-run.
extern "C" int midagma_debug_spoil_warm(midagma_solver* s) {
  if (!s || !s->blocked()) return -1;
  return abi_guarded(s, [&] {
    for (DevBuf<>* b : {&s->Pst2, &s->Pst2b})
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
  const int old = s->tcc_fast_steps;
  if (steps >= 0 && steps != old) {
    s->tcc_fast_steps = steps;
    s->graphs_valid = false;
  }
  return old;
}

// Test hook (not in the public header): the TCC fixed-shift stage on (1) or off (0); < 0 leaves
// it.  Returns the old setting.
extern "C" int midagma_debug_tcc_fix(midagma_solver* s, int on) {
  if (!s) return -1;
  const int old = s->tcc_fix != 0 ? 1 : 0;
  if (on >= 0 && (on != 0 ? 1 : 0) != old) {
    s->tcc_fix = on != 0 ? 1 : 0;
    s->cw.fix = s->tcc_fix;
    s->graphs_valid = false;
  }
  return old;
}

// Test hook (not in the public header): the TCC fixed-stage inverse's fast blocks (D2 >= 2048) on (1)
// or off (0) for the next set_trek_tcc; < 0 leaves it.  Returns the old setting.
extern "C" int midagma_debug_tcc_fastblk(midagma_solver* s, int on) {
  if (!s) return -1;
  const int old = s->tcc_fastblk ? 1 : 0;
  if (on >= 0) s->tcc_fastblk = on != 0;
  return old;
}

// Test hook (not in the public header): build_at folded into the previous slot's update
// (at_fold, MIDAGMA_EXP_AT_FOLD) on (1) or off (0); < 0 leaves it.  Returns the old setting, or -1
// (no handle / the fold cannot apply: not a blocked cov solver).
extern "C" int midagma_debug_at_fold(midagma_solver* s, int on) {
  if (!s || s->begun) return -1;
  const int old = s->at_fold ? 1 : 0;
  if (on < 0 || (on != 0) == s->at_fold) return old;
  if (on && !(s->mode == MIDAGMA_MODE_COV && s->blocked())) return -1;
  return abi_guarded(s, [&] {
    if (on && !s->A0.p) s->A0.alloc(s->D * s->D);
    s->at_fold = on != 0;
    s->graphs_valid = false;
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
  const int64_t K2 = s->D / s->B2, per = NM_PASSES + 2;
  if (cap < K2 * per) return -1;
  std::vector<double> part((size_t)K2 * (NM_PASSES + 1) * PART_STRIDE);
  std::vector<int> done(K2);
  if (hipMemcpy(part.data(), s->nmPart.p, part.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (hipMemcpy(done.data(), s->nmDone.p, K2 * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const int B2 = s->B2, NT = B2 / 16;
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
    const int64_t D = s->D, d = s->d, DD = D * D;
    if (!s->trek_on) {  // trek_value_grad: (0, zeros) when disabled (notreks.py)
      *value = 0.0;
      if (G) std::fill(G, G + d * d, 0.0);
      return MIDAGMA_OK;
    }
    s->scratch.alloc(DD);
    HIP_TRY(hipMemsetAsync(s->scratch.p, 0, DD * sizeof(double), s->stream));
    s->upload_matrix(s->scratch, W, d);
    const double* scal;
    if (s->trek_tcc) {
      TccCfg c = s->ccfg;
      c.weight = 1.0;  // the bare gradient, as trek_value_grad returns it
      launch_trek_tcc(s->scratch.p, d, D, c, s->cw, s->d_state_probe.p, s->Gtrek.p, s->stream);
      scal = s->cw.scal;
    } else {
      TrekCfg c = s->tcfg;
      c.weight = 1.0;
      launch_trek_pst(s->scratch.p, d, D, c, s->tw, s->d_state_probe.p, s->Gtrek.p, s->stream);
      scal = s->tw.scal;
    }
    HIP_TRY(hipMemcpyAsync(value, scal, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (G) {
      if (s->tcfg.mode == 2) {
        HIP_TRY(hipMemcpy2DAsync(G, d * sizeof(double), s->Gtrek.p, D * sizeof(double), d * sizeof(double), d,
                                 hipMemcpyDeviceToHost, s->stream));
      } else {
        std::fill(G, G + d * d, 0.0);
      }
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIDAGMA_OK;
  });
}

int midagma_h(midagma_solver* s, const double* W, double s_dom, double* h, double* G) {
  if (!s || !W || !h) return abi_fail(s, MIDAGMA_E_ARG, "h: null argument");
  if (!all_finite(W, s->d, s->d, s->d)) return abi_fail(s, MIDAGMA_E_ARG, std::string("h: ") + kNonFinite);
  return abi_guarded(s, [&] {
    const int64_t D = s->D, d = s->d, DD = D * D;
    s->scratch.alloc(DD);
    HIP_TRY(hipMemsetAsync(s->scratch.p, 0, DD * sizeof(double), s->stream));
    s->upload_matrix(s->scratch, W, d);
    DevBuf<> work;
    work.alloc(DD);
    launch_build_at(s->scratch.p, D, true, work.p, D, d, s_dom, nullptr, nullptr, s->stream);
    GJWork gw = s->gj();
    gw.Pstore = nullptr;
    launch_gj_inverse(work.p, D, D, gw, nullptr, s->stream);
    std::vector<double> pl(D);
    HIP_TRY(hipMemcpyAsync(pl.data(), s->pivlog.p, D * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (G) {
      s->Gtmp.alloc((size_t)d * d);
      launch_h_grad(s->scratch.p, work.p, s->Gtmp.p, d, D, s->stream);
      HIP_TRY(hipMemcpyAsync(G, s->Gtmp.p, (size_t)d * d * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    double ld = 0.0;
    for (int64_t i = 0; i < d; ++i) ld += pl[i];
    *h = -ld + (double)d * std::log(s_dom);
    return MIDAGMA_OK;
  });
}

static void host_trace_l1(midagma_solver* s, const double* Wd, const double* Z, double* sd, double* l1) {
  launch_trace_l1(Wd, Z, s->partials.p, s->d, s->D, s->stream);
  std::vector<double> part(2 * NRED);
  HIP_TRY(hipMemcpyAsync(part.data(), s->partials.p, part.size() * sizeof(double), hipMemcpyDeviceToHost,
                         s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  double a = 0.0, b = 0.0;
  for (int i = 0; i < NRED; ++i) {
    a += part[2 * i];
    b += part[2 * i + 1];
  }
  *sd = a;
  if (l1) *l1 = b;
}

int midagma_score(midagma_solver* s, const double* W, double* loss, double* G) {
  if (!s || !W || !loss) return abi_fail(s, MIDAGMA_E_ARG, "score: null argument");
  if (s->mode != MIDAGMA_MODE_COV || !s->has_cov) return abi_fail(s, MIDAGMA_E_STATE, "score: cov mode with set_cov");
  return abi_guarded(s, [&] {
    const int64_t D = s->D, d = s->d, DD = D * D;
    s->scratch.alloc(DD);
    HIP_TRY(hipMemsetAsync(s->scratch.p, 0, DD * sizeof(double), s->stream));
    s->upload_matrix(s->scratch, W, d);
    DevBuf<> rhs;
    rhs.alloc(DD);
    // rhs = cov @ (I - W)   (linear.py:85-86)
    s->enqueue_cov_gemm(s->cov_spec(s->cov.p, false, s->scratch.p, B_IMINUS), rhs.p, nullptr);
    double sd = 0;
    host_trace_l1(s, s->scratch.p, rhs.p, &sd, nullptr);
    *loss = 0.5 * sd;
    if (G) {
      s->Gtmp.alloc((size_t)d * d);
      launch_scale(rhs.p, -1.0, rhs.p, DD, s->stream);  // G_loss = -rhs
      s->download_matrix(G, rhs.p);
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIDAGMA_OK;
  });
}

int midagma_score_partial(midagma_solver* s, const double* W) {
  if (!s || !W || s->mode != MIDAGMA_MODE_DATA || !s->has_data)
    return abi_fail(s, MIDAGMA_E_STATE, "score_partial: data mode with set_data");
  return abi_guarded(s, [&] {
    const int64_t DD = s->D * s->D;
    s->scratch.alloc(DD);
    HIP_TRY(hipMemsetAsync(s->scratch.p, 0, DD * sizeof(double), s->stream));
    s->upload_matrix(s->scratch, W, s->d);
    HIP_TRY(hipMemsetAsync(s->zbuf + DD, 0, 64 * sizeof(double), s->stream));
    // Force loss partials: pass no state (st == nullptr computes them unconditionally).
    s->enqueue_data_partial(s->scratch.p, nullptr);
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIDAGMA_OK;
  });
}

int midagma_score_finish(midagma_solver* s, double* loss, double* G) {
  if (!s || !loss || s->mode != MIDAGMA_MODE_DATA) return abi_fail(s, MIDAGMA_E_STATE, "score_finish: data mode");
  return abi_guarded(s, [&] {
    const int64_t D = s->D, d = s->d, DD = D * D;
    const double n = (double)s->n_global;
    if (s->loss == MIDAGMA_LOSS_L2) {
      // loss = 0.5 tr((I-W)^T cov (I-W)) with cov (I-W) = Z / n ; G = -Z / n
      double sd = 0;
      host_trace_l1(s, s->scratch.p, s->zbuf, &sd, nullptr);
      *loss = 0.5 * (sd / n);
      if (G) {
        std::vector<double> z((size_t)d * d);
        s->download_matrix(z.data(), s->zbuf);
        HIP_TRY(hipStreamSynchronize(s->stream));
        for (size_t i = 0; i < z.size(); ++i) G[i] = -(z[i] / n);
      }
    } else {
      double tail = 0;
      HIP_TRY(hipMemcpyAsync(&tail, s->zbuf + DD, sizeof(double), hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      *loss = 1.0 / n * tail;
      if (G) {
        std::vector<double> z((size_t)d * d), c((size_t)d * d);
        s->download_matrix(z.data(), s->zbuf);
        s->download_matrix(c.data(), s->cov.p);
        HIP_TRY(hipStreamSynchronize(s->stream));
        for (size_t i = 0; i < z.size(); ++i) G[i] = (1.0 / n) * z[i] - c[i];
      }
    }
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
  if (!s || !s->dfw.stamps) return -1;
  const int64_t n = std::min<int64_t>(cap, (int64_t)s->dfStamps.n);
  if (hipStreamSynchronize(s->stream) != hipSuccess) return -1;
  if (hipMemcpy(out, s->dfStamps.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return n;
}
#endif  // MIDAGMA_EXPERIMENTS
