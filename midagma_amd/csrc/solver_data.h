// Data mode of the solver handle: the resident row shard X, the buffers of its two GEMMs
// (Y = X (I - W) or expit(X W), then Z = X^T Y), the forms set() chose for them, and the GemmSpec
// of each (launch.h), described once.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "abi.h"
#include "devmem.h"
#include "launch.h"
#include "solver_knobs.h"

namespace midagma {

struct DataMode {
  int loss = 0;
  int64_t d = 0, D = 0;
  int64_t Kd = 0;   // the solver's Kd(): k extent of the GEMMs over the padded node dimension
  int64_t Kxw = 0;  // ... of the X (I - W) GEMM (knobs.xw_fullk: all of D)
  DevBuf<> X, Y, Zparts, loss_part;
  int64_t n_local = 0, n_pad = 0, n_global = 0;
  // X^T (D x n_pad), the xw GEMM's A operand in the m-contiguous layout (the X^T Y GEMM reads
  // X itself that way); kept when the device has the room (MIDAGMA_NO_XT disables it)
  DevBuf<> XT;
  DevBuf<> prepad;  // (knobs.prepad_mb)
  bool use_xt = false;
  int split = 1;  // split-K of the classical X^T Y GEMM
  // X^T Y by one level of Strassen (gemm.hip, launch_xty_strassen): the five X-side operand sums,
  // formed by set for as long as this X is set, and the seven products' split-K slices.
  // xty_form: what the current data uses (1 classical, 2 Strassen).  midagma_debug_xty_form:
  // xty_form_force 0 the size rule, 1 always classical, 2 Strassen wherever the shape allows;
  // xty_split_force > 0: that split-K for the products instead of the rule's, for the next
  // set; xty_split: the one the current data's slices (Sparts) were sized for
  DevBuf<> Xsums, Sparts;
  int xty_form = 1, xty_form_force = 0, xty_split_force = 0, xty_split = 0;
  int sig_split = 1;  // the logistic sigmoid GEMM's serial split-K (launch_gemm; 2: Y holds the partial too)
  int sig_split_force = 0;  // midagma_debug_sig_split: 0 the size rule, 1 never split, 2 split where the shape allows
  int64_t loss_part_count = 0;

  // A new shard of n_local rows (host or device X, row stride d).  IW: the solver's I - W buffer,
  // kept or released for this data; flag: a device int for the non-finite check of a device X.
  // Every pointer the slot graphs captured may change: the caller invalidates its graphs.
  void set(const double* Xin, int64_t n_local_, int64_t n_global_, bool on_device, int loss_, int64_t d_, int64_t D_,
           int64_t Kd_, bool w32, const SolverKnobs& knobs, DevBuf<>& IW, int* flag, hipStream_t stream) {
    loss = loss_, d = d_, D = D_, Kd = Kd_;
    Kxw = knobs.xw_fullk ? D : Kd;
    n_local = n_local_;
    n_global = n_global_;
    n_pad = (n_local + 127) / 128 * 128;
    const size_t nx = (size_t)n_pad * D;
    // knobs.prepad_mb of device memory allocated (and kept) before X, to move X, X^T and Y elsewhere
    // (the X^T Y GEMM's fetched bytes against placement)
    if (knobs.prepad_mb > 0 && !prepad.p) prepad.alloc((size_t)knobs.prepad_mb << 17);
    X.alloc(nx);
    // logistic with few 128-tiles: the sigmoid GEMM in two serial K halves when its last round of
    // tiles would be at most half full (n = 1e4, d = 1000: 632 tiles for 512 resident slots)
    const int64_t sig_tiles = (n_pad / 128) * (D / 128);
    const bool sig_ok = loss == MIDAGMA_LOSS_LOGISTIC && D % 128 == 0 && sig_tiles % 8 == 0;
    sig_split = sig_ok && knobs.sig_split > 0 && sig_tiles < 2048 && sig_tiles % 512 != 0 && sig_tiles % 512 <= 256 ? 2 : 1;
    if (sig_split_force == 1) sig_split = 1;  // midagma_debug_sig_split (tests)
    if (sig_split_force == 2 && sig_ok) sig_split = 2;
    if (sig_split == 2) {  // the output, the first halves' partial, then one flag word per tile
      Y.alloc(2 * nx + (size_t)(sig_tiles + 1) / 2);
      HIP_TRY(hipMemsetAsync(Y.p + 2 * nx, 0, (size_t)(sig_tiles + 1) / 2 * sizeof(double), stream));
    } else {
      // knobs.y_offset: Y placed that many bytes into its allocation (L2 set aliasing between X and
      // Y in the X^T Y GEMM)
      Y.alloc_shifted(nx, (size_t)knobs.y_offset / sizeof(double));
    }
    HIP_TRY(hipMemsetAsync(X.p, 0, nx * sizeof(double), stream));
    HIP_TRY(hipMemcpy2DAsync(X.p, D * sizeof(double), Xin, d * sizeof(double), d * sizeof(double), n_local,
                             on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    if (on_device) {  // the host path checked before the copy
      launch_any_nonfinite(X.p, (int64_t)nx, flag, stream);
      int bad = 0;
      HIP_TRY(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      if (bad) throw std::invalid_argument(std::string("set_data: ") + kNonFinite);
    }
    size_t mem_free = 0, mem_total = 0;
    HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
    // (the 128-tile GEMM only: D % 128 == 0; smaller problems are not worth the copy)
    use_xt = getenv("MIDAGMA_NO_XT") == nullptr && D % 128 == 0 && mem_free > nx * sizeof(double) + (size_t(2) << 30);
    if (use_xt) {
      XT.alloc(nx);
      launch_transpose(X.p, D, n_pad, D, XT.p, n_pad, stream);
    } else {
      XT.release();
    }
    if (loss == MIDAGMA_LOSS_L2 && (D % 128 == 0 || w32))  // (float32 W: I - W from build_at)
      IW.alloc((size_t)D * D);
    else
      IW.release();
    // split-K over the rows so the X^T Y GEMM fills the chip: (D/64)^2 tiles x split >= ~1024 workgroups
    const int64_t tiles = (D % 128 == 0) ? (D / 128) * (D / 128) : (D / 64) * (D / 64);
    const int64_t ktiles = n_pad / 64;
    split = std::min((int)std::max<int64_t>(1, std::min<int64_t>(ktiles / 8, (1024 + tiles - 1) / tiles)), 32);
    if (knobs.data_split >= 0) split = knobs.data_split;
    if (split > 1) Zparts.alloc((size_t)split * D * D);
    // X^T Y by one level of Strassen (gemm.hip): when the shape allows it (D % 256 == 0), every
    // product's K slice is long enough to amortise its tile's prologue and epilogue
    // (kXtyStrassenMinSlice), and the device has room for the five operand sums of X (1.25 x the
    // size of X; the same free-memory rule as X^T).  Everything else keeps the classical GEMM.
    xty_form = 1;
    bool strassen = xty_form_force != 1 && xty_strassen_shape(D, n_pad) && knobs.data_split < 0;
    XtyStrassenPlan plan{};
    if (strassen) {
      plan = xty_strassen_plan(D, n_pad, xty_split_force);
      if (xty_form_force != 2 && plan.kslice < kXtyStrassenMinSlice) strassen = false;
    }
    if (strassen) {
      const size_t nsum = (size_t)xty_strassen_sum_count(D, n_pad);
      HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
      strassen = mem_free > nsum * sizeof(double) + (size_t(2) << 30);
      if (strassen) {
        try {
          Xsums.alloc(nsum);
          Sparts.alloc((size_t)xty_strassen_part_count(D, plan.nsplit));
        } catch (const HipError& e) {
          if (e.code != hipErrorOutOfMemory) throw;
          (void)hipGetLastError();
          strassen = false;
        }
      }
    }
    if (strassen) {
      launch_xty_strassen_sums(X.p, D, n_pad, Xsums.p, stream);
      xty_form = 2;
      xty_split = xty_split_force;
    } else {
      Xsums.release();
      Sparts.release();
    }
    loss_part_count = (n_pad / 64) * (D / 64);
    if (loss == MIDAGMA_LOSS_LOGISTIC) {
      loss_part.alloc(loss_part_count);
      HIP_TRY(hipMemsetAsync(loss_part.p, 0, loss_part_count * sizeof(double), stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
  }

  const double* xw_a() const { return use_xt ? XT.p : X.p; }
  int64_t xw_lda() const { return use_xt ? n_pad : D; }
  // l2: Y = X_k (I - W); iw (nullable): I - W already formed (build_at), the plain-B form
  GemmSpec xw_spec(const double* Wp, const double* iw) const {
    return GemmSpec{n_pad, D, Kxw, xw_a(), xw_lda(), use_xt, iw ? iw : Wp, D, iw ? B_PLAIN : B_IMINUS, Y.p, D, 1, 0};
  }
  // logistic: Y = expit(X_k W) with the loss partials (sig_split = 2: the serial split)
  GemmSpec sigmoid_spec(const double* Wp) const {
    GemmSpec gs{n_pad, D, Kd, xw_a(), xw_lda(), use_xt, Wp, D, B_PLAIN, Y.p, D, sig_split,
                sig_split > 1 ? n_pad * D : 0};
    gs.epi = EPI_SIGMOID;
    gs.loss_part = loss_part.p;
    gs.m_valid = n_local;
    gs.n_valid = d;
    return gs;
  }
  // Z_k = X_k^T Y in `split` K slices (launch_gemm_summed: Zparts -> zbuf); the classical form
  // (enqueue_xty: the Strassen form takes its place when set chose it)
  GemmSpec xty_spec() const {
    return GemmSpec{D, D, n_pad, X.p, D, true, Y.p, D, B_PLAIN, Zparts.p, D, split, D * D};
  }

  // X^T X into zbuf: the X^T Y GEMM with Y = X (midagma_data_gram)
  void enqueue_gram(double* zbuf, hipStream_t stream) const {
    GemmSpec gs = xty_spec();
    gs.B = X.p;
    launch_gemm_summed(gs, Zparts.p, zbuf, nullptr, stream);
  }
  // the two GEMMs (midagma_profile_parts times each alone)
  void enqueue_xw(const double* Wp, const State* st, const double* iw, hipStream_t stream) const {
    launch_gemm(loss == MIDAGMA_LOSS_L2 ? xw_spec(Wp, iw) : sigmoid_spec(Wp), st, stream);
  }
  void enqueue_xty(double* zbuf, const State* st, hipStream_t stream) const {
    if (xty_form == 2)
      launch_xty_strassen(X.p, Xsums.p, Y.p, D, n_pad, xty_split, Sparts.p, zbuf, st, stream);
    else
      launch_gemm_summed(xty_spec(), Zparts.p, zbuf, st, stream);
  }

  // the serial split sigmoid GEMM's per-tile hand-off words (gemm.hip, sig_split_take): after the
  // output and the first halves' partial in Y
  void clear_sig_flags(hipStream_t stream) {
    if (sig_split != 2) return;
    const int64_t tiles = (n_pad / 128) * (D / 128);
    HIP_TRY(hipMemsetAsync(Y.p + 2 * n_pad * D, 0, (size_t)(tiles + 1) / 2 * sizeof(double), stream));
  }
};

}  // namespace midagma
