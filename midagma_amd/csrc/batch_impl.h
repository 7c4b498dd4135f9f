// The batch of small-d problems behind the midagma_batch_*, midagma_btrek_*, midagma_blogit_* and
// midagma_boot_* entries: the handle that batch.hip (create, set_cov, masks, minimize, the logistic
// loss's X) and boot.hip (the bootstrap covariances written into the handle's cov slabs) share.
#pragma once

#include <hip/hip_runtime.h>

#include <exception>
#include <string>
#include <vector>

#include "../../include/midagma_hip.h"
#include "solver_impl.h"

struct midagma_batch {
  int64_t d = 0, D = 0, B = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  DevBuf<> W, m, v, cov, covs, minc, mexc, carry, pstore, bc_table;
  DevBuf<> stage;  // B x d x d: the compact host layout on the device
  DevBuf<Params> d_params;
  DevBuf<State> d_state;
  DevBuf<CkptRec> d_ckpt;
  DevBuf<int32_t> d_index;
  PinBuf<Params> h_params;  // host mirrors of d_params, d_state; the index list of the next launch
  PinBuf<State> h_state;
  PinBuf<int32_t> h_index;
  int64_t ckpt_cap = 0, bc_len = 0;
  double bc_b1 = -1, bc_b2 = -1;
  bool has_cov = false, has_inc = false, has_exc = false;
  // the PST trek regularizer of the problems (midagma_btrek_set): one pair list, as its d x d
  // multiplicity matrix on the device, and a weight per problem
  DevBuf<> trek_N, trek_val;
  midagma::SmallPst trek{};  // (mode 0: off)
  std::vector<double> trek_weight;
  // the logistic loss (midagma_blogit_*): X padded to n_pad x small_block(d) doubles per problem,
  // stored once when the problems share it
  DevBuf<> X, logit_loss;
  int64_t x_n = 0, x_n_pad = 0;
  bool x_shared = false, has_data = false;
  std::vector<uint8_t> last_active;  // the problems of the last minimize call (their checkpoints)
  double boot_ms[4] = {0, 0, 0, 0};  // the last boot_cov: centring, counts, Gram, finish (device events)

  ~midagma_batch() {
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }

  dim3 grid(int64_t elems, int64_t problems) const {
    return dim3((unsigned)((elems + NTHREADS - 1) / NTHREADS), (unsigned)problems);
  }

  // batch.hip
  void alloc();
  void upload_all(DevBuf<>& dst, const double* src);  // host B x d x d -> every problem's padded slab of dst
  void download_all(const DevBuf<>& src, double* dst);  // every problem's padded slab of src -> host B x d x d
  void ensure_tables(double b1, double b2, int64_t max_iter, int64_t checkpoint);
  void minimize(double* Wh, const double* mu, const double* s_dom, const double* lr, const double* lambda1,
                int64_t max_iter, double tol, double b1, double b2, int64_t checkpoint, const uint8_t* active,
                midagma_result* res, bool logistic = false);
  midagma::SmallLogit logit_view() const;
  void set_data(const double* Xh, int64_t n, bool shared);
  void logit_score(const double* Wh, double* loss, double* G);
  void set_trek(int seq, int agg, int mode, const double* weight, double eps_inv, const int64_t* pairs, int64_t m);
  void trek_value(const double* Wh, double* value, double* grad);
};

// abi.h's hook: an entry's device work runs on the batch's device
inline void abi_select_device(const midagma_batch* h) { HIP_TRY(hipSetDevice(h->device)); }
