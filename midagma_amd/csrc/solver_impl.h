// The data-mode / cov-mode solver object behind the C ABI (include/midagma_hip.h): its device
// buffers, the captured slot graphs and the host drivers that replay them.  Shared by solver.hip
// (the C ABI of one solver) and group.hip (ABI 11: a single-process group of data-mode solvers
// over several devices).
//
// One "slot" = one pass of the reference's loop body (linear.py:225-331):
//   part 1  build (sI - W∘W)^T -> blocked GJ inverse (+ log|pivots|) -> score GEMM(s)
//   part 2  domain check / checkpoint partials -> control (1 WG) -> fused update
// The control decision lives in device memory, so slots are replayed from a
// hipGraph in batches with no host round trip per step; the host only polls
// the state every batch.  Slots after termination are
// no-ops (every kernel early-exits on the status word).
//
// The handle is the core step's state plus one member per part, each in its own header, owning
// its buffers and the launch view over them: knobs (solver_knobs.h, read once at creation), trek
// (solver_trek.h), binv (solver_binv.h), data (solver_data.h), graphs (slot_graphs.h) and, in the
// experiments build, df (experiments/solver_df.inc).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/midagma_hip.h"
#include "devmem.h"
#include "launch.h"
#include "slot_graphs.h"
#include "slot_sched.h"
#include "solver_binv.h"
#include "solver_data.h"
#include "solver_knobs.h"
#include "solver_trek.h"

#ifdef MIDAGMA_EXPERIMENTS
#include "../../experiments/solver_df.inc"
#else
namespace midagma {
// the product build has no one-launch inverse (experiments/solver_df.inc): never on
struct DfInverse {
  bool on() const { return false; }
  int timeouts() const { return 0; }
  void setup(int64_t, int, const SolverKnobs&) {}
  void enqueue(const double*, int64_t, int64_t, double*, double*, const Params*, State*, const BInvWork&, int,
               hipStream_t) const {}
};
}  // namespace midagma
#endif

namespace midagma {

// group.hip: the slot graphs of an emulated group (every member on one device, the score sum a
// fixed-order device sum) are captured over all members' streams at once, and a hand-back clears
// every member's status word
hipGraphExec_t group_capture(midagma_group* g, const midagma_solver* caller, int which, int reps, int passes);
void group_clear_handback(midagma_group* g);

// What a minimize call uploads before its first slot, shared by midagma_solver::begin and the
// batch of small-d problems (batch.hip).
// The Params of a float64 cov-mode l2 call without a trek regularizer; begin overrides the
// fields its other modes set differently.
inline Params cov_l2_params(int64_t d, int64_t D, double mu, double s, double lambda1, double tol, double b1,
                            double b2, int64_t max_iter, int64_t checkpoint, int64_t ld_table, bool has_inc,
                            bool has_exc) {
  Params p{};
  p.mu = mu;
  p.s = s;
  p.lambda1 = lambda1;
  p.tol = tol;
  p.beta1 = b1;
  p.beta2 = b2;
  p.c1 = 1 - b1;
  p.c2 = 1 - b2;
  p.mu_l1 = mu * lambda1;
  p.d_log_s = (double)d * std::log(s);
  p.max_iter = max_iter;
  p.checkpoint = checkpoint;
  p.d = d;
  p.D = D;
  p.ld_table = ld_table;
  p.has_inc = has_inc;
  p.has_exc = has_exc;
  p.zscale = 1.0;  // Z already is ((-mu) cov) @ (I - W)
  p.cscale = 0.0;
  p.score_scale = 0.5 / (-mu);
  return p;
}
// cov_l2_params' Params turned into those of a data-mode logistic call over n rows: G_score =
// (mu / n) X^T expit(X W) - mu cov, score = loss / n (linear.py:89-92, 245-246)
inline void logistic_data_params(Params& p, double mu, double n) {
  p.logistic = 1;
  p.zscale = mu / n;
  p.cscale = -mu;
  p.score_scale = 0.0;
  p.logit_scale = 1.0 / n;
}
// the State before a call's first slot
inline State initial_state(double lr) {
  State st{};
  st.status = ST_RUNNING;
  st.lr = lr;
  st.obj_prev = 1e16;
  return st;
}
// (1 - beta ** iter) for iter = 1..len, exactly as Python computes it (linear.py:160-161)
inline std::vector<double> bc_table_values(double b1, double b2, int64_t len) {
  std::vector<double> t(2 * len);
  for (int64_t it = 1; it <= len; ++it) {
    t[2 * (it - 1)] = 1 - ::pow(b1, (double)it);
    t[2 * (it - 1) + 1] = 1 - ::pow(b2, (double)it);
  }
  return t;
}

}  // namespace midagma

using namespace midagma;

struct midagma_solver {
  // ---- shape, streams ---------------------------------------------------------
  int loss = 0, mode = 0, device = 0;
  int64_t d = 0, D = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // the inverse beside the score GEMMs on a side stream (it depends on W only; data mode, and cov
  // mode under knobs.cov_fork / cov_la); fork / join are events inside the captured slot graph
  hipStream_t side = nullptr;
  Event ev_fork, ev_join;
  std::string err;
  SolverKnobs knobs;  // read by midagma_create; the midagma_debug_* hooks write single fields

  // ---- the core step's buffers ----------------------------------------------------
  DevBuf<> W, m, v, Mt, cov, covs, minc, mexc, P, R, C, pivlog, partials, bc_table, zown, scratch, Gtmp, Pstore;
  // ((-mu) cov)^T: the cov-mode score GEMM reads its A operand k-major (coalesced tile rows)
  DevBuf<> covsT;
  DevBuf<> npart;  // checkpoint-step norm partials (fused_update -> control)
  DevBuf<> l1w;    // float32 W: [0] numpy's float32 L1 sum, then its chunk sums (np_l1_kernel)
  // cov mode, l2, d <= 64: the one-workgroup persistent loop (small.hip, small_on)
  DevBuf<> scarry, sprev;  // between two small-loop launches: pending norms + warm count, last inverses
  DevBuf<> IW;  // I - W of the slot, written by build_at (data-mode l2 X (I - W) GEMM; float32 W)
  DevBuf<> cov_parts;  // the cov score GEMM's split-K slices
  int cov_split = 1;
  DevBuf<> cupart_ctr;  // experiments: launch_gemm_cupart's tile counter
  double* zbuf = nullptr;  // d x d (+64 tail) score partial; internal or bound
  int64_t zbuf_cap = 0;
  bool w32 = false;  // midagma_set_w_float32: the reference's float32 W arithmetic (common.h f32r)

  // ---- the parts -----------------------------------------------------------------
  Trek trek;        // PST / TCC regularizer
  BlockedInv binv;  // two-level blocked inverse and its warm-start carry
  DataMode data;    // the row shard and its GEMMs
  SlotGraphs graphs;
  DfInverse df;     // experiments build only (else a stand-in that is never on)

  // ---- what a call uploads, and its mirrors -------------------------------------------
  DevBuf<Params> d_params;
  DevBuf<State> d_state;
  DevBuf<CkptRec> d_ckpt;
  int64_t ckpt_cap = 0;
  PinBuf<State> h_state;  // 2 snapshots
  Event ev[2];
  double bc_b1 = -1, bc_b2 = -1;
  int64_t bc_len = 0;
  bool has_cov = false, has_data = false, has_inc = false, has_exc = false;
  bool begun = false;
  const double* cap_minc = nullptr;  // mask pointers baked into the captured graphs
  const double* cap_mexc = nullptr;
  double mu = 1.0;
  Params hp{};
  bool ctl_folded = false;  // set by enqueue_part1 for the enqueue_part2 of the same slot
  int64_t handback_count = 0;
  int64_t fast_batch = BlockedScheduler::kMaxBatch;

  // ABI 7: the in-library RCCL communicator (data mode over ranks): the score all-reduce inside
  // the captured slot graphs, and an agreement all-reduce of (status, iters) at every poll
  void* comm = nullptr;
  int comm_ranks = 1;
  bool inslot_comm = false;  // set while capturing a whole slot
  DevBuf<> agree;          // 2 x 4 doubles (double-buffered polls)
  PinBuf<double> h_agree;  // 2 x 4
  // ABI 11: member of a single-process device group (group.hip).  group: set in an emulated group
  // (its slot graphs are the group's, captured over every member's stream); group_stop: set while a
  // threaded group's minimize runs, raised when another member failed (checked at every poll)
  midagma_group* group = nullptr;
  const std::atomic<bool>* group_stop = nullptr;
  void check_group_stop() const {
    if (group_stop && group_stop->load()) throw std::runtime_error("device group: another member failed");
  }

  // The graphs go before the buffers they name; every buffer and event frees itself afterwards.
  ~midagma_solver() {
    graphs.destroy();
    if (stream) (void)hipStreamSynchronize(stream);
    comm_destroy(comm);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
    if (side) (void)hipStreamDestroy(side);
    if (graphs.cap) (void)hipStreamDestroy(graphs.cap);
  }

  GJWork gj() { return GJWork{P.p, R.p, C.p, pivlog.p, Pstore.p}; }
  bool blocked() const { return binv.on(); }
  // k extent of the GEMMs whose K is the padded node dimension: the rows of A past d are zero
  // (X^T, ((-mu) cov)^T), so the k loop stops at the first 16-multiple >= d (the pipelined
  // 128-tile kernel, D % 128 == 0; bit-identical: the skipped terms are exact zeros)
  int64_t Kd() const { return D % 128 == 0 ? (d + 15) / 16 * 16 : D; }

  // ---- set-ups ---------------------------------------------------------------------
  // Each ends in graphs.valid = false wherever a pointer or a choice the slot graphs captured may
  // have changed; the parts report that, they do not reach back here.
  void alloc_core() {
    const size_t DD = (size_t)D * D;
    for (DevBuf<>* b : {&W, &m, &v, &Mt, &cov, &covs, &covsT}) {
      b->alloc(DD);
      HIP_TRY(hipMemsetAsync(b->p, 0, DD * sizeof(double), stream));
    }
    P.alloc(64 * 64);
    R.alloc((size_t)64 * D);
    C.alloc((size_t)D * 64);
    pivlog.alloc(D);
    Pstore.alloc((size_t)D * 32);
    partials.alloc(2 * NRED);
    npart.alloc((size_t)((d + NTHREADS - 1) / NTHREADS) * d * NORM_FIELDS);
    HIP_TRY(hipMemsetAsync(npart.p, 0, npart.n * sizeof(double), stream));
    scarry.alloc(NORM_FIELDS + 1);
    HIP_TRY(hipMemsetAsync(scarry.p, 0, scarry.n * sizeof(double), stream));
    if (small_block(d) > 0) sprev.alloc(2 * (size_t)small_block(d) * small_block(d));
    if (D % 128 == 0) {
      // split-K of the cov score GEMM: small grids get slices to fill the chip; large ones the
      // split that best rounds the last wave of 128-tiles (2 workgroups per CU resident:
      // 1600 tiles at d = 5000 leave the 4th wave 1/8 full, split 4 -> 13 full-ish waves)
      const int64_t tiles = (D / 128) * (D / 128), slots = 2 * 256;
      if (tiles < 256) {
        // about one workgroup per CU: round(256 / tiles + 1/4), at most 4 and D / 128 (measured,
        // fused with the last trailing update: D = 1152 split 3 2909 vs 4 2770 steps/s; D = 1408
        // split 2 2016 vs 4 1985; D = 1792 split 2 1480 vs 4 1452 vs 1 1406; D = 1024 split 4)
        cov_split = (int)std::max<int64_t>(
            1, std::min<int64_t>({4, D / 128, (int64_t)(256.0 / (double)tiles + 0.75)}));
      } else if (tiles >= 1024) {  // (256..1023 tiles: split 1 measured best at d = 2000)
        double best = 1e30;
        for (int sp = 1; sp <= 4; ++sp) {
          const double waves = (double)((tiles * sp + slots - 1) / slots) / sp * (1.0 + 0.03 * (sp - 1));
          if (waves < best) best = waves, cov_split = sp;
        }
      }
      if (knobs.cov_split >= 0) cov_split = knobs.cov_split;
      if (cov_split > 1) cov_parts.alloc((size_t)cov_split * DD);
    }
    if (knobs.at_fold < 0) knobs.at_fold = D >= 1024 && D <= 1408;  // the rule (solver_knobs.h)
    binv.alloc(D, mode, knobs, stream);
    if (blocked() && mode == MIDAGMA_MODE_COV) df.setup(D, device, knobs);
    zown.alloc(DD + 64);
    HIP_TRY(hipMemsetAsync(zown.p, 0, (DD + 64) * sizeof(double), stream));
    zbuf = zown.p;
    zbuf_cap = (int64_t)DD + 64;
    d_params.alloc(1);
    d_state.alloc(1);
    h_state.alloc(2);
    for (Event& e : ev) e.create(hipEventDisableTiming);
    if ((mode == MIDAGMA_MODE_DATA && !knobs.no_fork) ||
        (mode == MIDAGMA_MODE_COV && (knobs.cov_fork != 0 || knobs.cov_la) && binv.B2 > 0 &&
         (D - binv.B2 >= 1792 || knobs.cov_fork == 2))) {
      // Default priority: a fork / join between a high-priority stream and another one left the
      // process's later two-stream work ~5x slower (the config-5 step after a data-mode solver:
      // 7.5k -> 1.3k steps/s, also after a plain torch fork / join; tools/probe_after_data.py),
      // and the forked inverse hides just as well without it (config 4: 17.46 vs 17.50 steps/s
      // at n = 1e6, 133.8 vs 133.5 at the 8-GPU shard n = 125k)
      HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
      ev_fork.create(hipEventDisableTiming);
      ev_join.create(hipEventDisableTiming);
      if (kExperiments) cupart_ctr.alloc(1);  // (launch_gemm_cupart's counter; not while capturing)
    }
  }

  void set_trek(int seq, int agg, int tmode, double weight, double eps_inv, int64_t K, const int64_t* pairs,
                int64_t mpairs) {
    trek.set_pst(d, D, gj(), seq, agg, tmode, weight, eps_inv, K, pairs, mpairs, stream);
    graphs.valid = false;
  }
  void set_trek_tcc(int tmode, double weight, double wS, double eps, const int64_t* pairs, int64_t mpairs) {
    trek.set_tcc(d, D, knobs, tmode, weight, wS, eps, pairs, mpairs);
    graphs.valid = false;
  }

  void set_data(const double* X, int64_t n_local, int64_t n_global, bool on_device) {
    data.set(X, n_local, n_global, on_device, loss, d, D, Kd(), w32, knobs, IW, reinterpret_cast<int*>(partials.p),
             stream);
    binv.set_data_rows(D, data.n_pad, knobs);  // (B2 may change: the graphs go either way)
    has_data = true;
    graphs.valid = false;
  }

  void set_masks(const double* mask_inc, const double* mask_exc) {
    const size_t DD = (size_t)D * D;
    const bool inc = mask_inc != nullptr, exc = mask_exc != nullptr;
    if (inc) {
      minc.alloc(DD);
      HIP_TRY(hipMemsetAsync(minc.p, 0, DD * sizeof(double), stream));
      upload_matrix(minc, mask_inc, d);
    }
    if (exc) {
      mexc.alloc(DD);
      HIP_TRY(hipMemsetAsync(mexc.p, 0, DD * sizeof(double), stream));
      upload_matrix(mexc, mask_exc, d);
    }
    HIP_TRY(hipStreamSynchronize(stream));
    const double* pi = inc ? minc.p : nullptr;
    const double* pe = exc ? mexc.p : nullptr;
    if (pi != cap_minc || pe != cap_mexc) graphs.valid = false;  // captured pointers changed
    cap_minc = pi;
    cap_mexc = pe;
    has_inc = inc;
    has_exc = exc;
  }

  void set_w_float32(bool on) {
    if (on != w32) graphs.valid = false;  // the float32 slots carry numpy's L1 sum
    if (on && !l1w.p) l1w.alloc((size_t)(1 + (np_l1_chunks(d) + 1) / 2));
    if (on && (mode == MIDAGMA_MODE_COV || loss == MIDAGMA_LOSS_L2) && !IW.p) {
      // the score GEMM's I - W (float32 diagonal) comes from build_at, not the GEMM's staging
      IW.alloc((size_t)D * D);
      HIP_TRY(hipMemsetAsync(IW.p, 0, (size_t)D * D * sizeof(double), stream));
      graphs.valid = false;
    }
    w32 = on;
  }

  // a communicator over nranks ranks (midagma_comm_init, or the group's): the slot graphs now
  // carry the all-reduce
  void attach_comm(void* c, int nranks) {
    comm = c;
    comm_ranks = nranks;
    agree.alloc(8);
    h_agree.alloc(8);
    graphs.valid = false;
  }

  // midagma_comm_init: a fresh communicator of this rank in place of the one it had
  void init_comm(const void* id, int nranks, int rank) {
    HIP_TRY(hipStreamSynchronize(stream));
    comm_destroy(comm);
    comm = nullptr;
    attach_comm(comm_create(id, nranks, rank), nranks);
  }

  void upload_matrix(DevBuf<>& dst, const double* src, int64_t ld_src) {
    HIP_TRY(hipMemcpy2DAsync(dst.p, D * sizeof(double), src, ld_src * sizeof(double), d * sizeof(double), d,
                             hipMemcpyHostToDevice, stream));
  }

  void download_matrix(double* dst, const double* src) {
    HIP_TRY(hipMemcpy2DAsync(dst, d * sizeof(double), src, D * sizeof(double), d * sizeof(double), d,
                             hipMemcpyDeviceToHost, stream));
  }

  void ensure_bc_table(double b1, double b2, int64_t max_iter) {
    if (b1 == bc_b1 && b2 == bc_b2 && max_iter <= bc_len) return;
    const int64_t len = std::max<int64_t>(max_iter, 1);
    const std::vector<double> t = bc_table_values(b1, b2, len);
    bc_table.alloc(2 * len);
    HIP_TRY(hipMemcpy(bc_table.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    bc_b1 = b1;
    bc_b2 = b2;
    bc_len = len;
    graphs.valid = false;  // table pointer may have changed
  }

  void ensure_ckpt(int64_t max_iter, int64_t checkpoint) {
    const int64_t need = max_iter / std::max<int64_t>(checkpoint, 1) + 4;
    if (need <= ckpt_cap) return;
    d_ckpt.alloc(need);
    ckpt_cap = need;
    graphs.valid = false;
  }

  // ---- the cov GEMMs, each described once (launch.h GemmSpec; data mode's: solver_data.h) ----
  // out = op(Cm) @ (I - W) on the d x d problem, split-K over cov_split fixed slices (in
  // cov_parts) when the tile grid alone cannot fill the chip; a_trans: Cm holds the transpose of
  // the left operand; B_PLAIN: Wp already holds I - W
  GemmSpec cov_spec(const double* Cm, bool a_trans, const double* Wp, GemmB bmode) const {
    return GemmSpec{D, D, Kd(), Cm, D, a_trans, Wp, D, bmode, cov_parts.p, D, cov_split, D * D};
  }
  // the slot's cov score GEMM rhs = ((-mu) cov) @ (I - W): A read k-major from ((-mu) cov)^T
  // (coalesced tile rows), B = I - W formed by build_at (IW, plain B) when the slot keeps it; with
  // the fast slot's folded control for launch_gemm_trail
  GemmSpec score_cov_spec() const {
    GemmSpec gs = cov_spec(covsT.p, true, IW.p ? IW.p : W.p, IW.p ? B_PLAIN : B_IMINUS);
    if (knobs.ctl_fold && binv.ctl_ticket.p) {
      gs.ctl_pr = d_params.p;
      gs.ctl_table = bc_table.p;
      gs.ctl_ticket = reinterpret_cast<int*>(binv.ctl_ticket.p);
    }
    return gs;
  }

  // the slot's cov score GEMM into out; sum = false leaves split-K slices in cov_parts
  void enqueue_score_cov(double* out, const State* st, bool sum) { enqueue_cov_gemm(score_cov_spec(), out, st, sum); }

  // the cov GEMM gs (cov_spec) into out, its slices summed in fixed order (deterministic) unless
  // sum = false
  void enqueue_cov_gemm(GemmSpec gs, double* out, const State* st, bool sum = true) {
#ifdef MIDAGMA_EXPERIMENTS
    // knobs.gemm_ses: the forked score GEMM confined to the first shader engines of every XCD, so
    // the inverse's launches on the side stream keep the other CUs to themselves
    if (knobs.gemm_ses > 0 && cov_fork_on() && D % 128 == 0) {
      if (!cupart_ctr.p) throw std::logic_error("cupart counter not allocated");
      if (cov_split == 1) gs.C = out;
      launch_gemm_cupart(gs, st, knobs.gemm_ses, reinterpret_cast<int*>(cupart_ctr.p), stream);
      if (cov_split > 1 && sum) launch_sum_slices(cov_parts.p, cov_split, D * D, D * D, out, st, stream);
      return;
    }
#endif
    if (cov_split > 1 && !sum)
      launch_gemm(gs, st, stream);  // (the fast slot: fused_update sums the slices)
    else
      launch_gemm_summed(gs, cov_parts.p, out, st, stream);
  }

  // Z_k = X_k^T (X_k (I - W))  (l2)   or   X_k^T expit(X_k W)  (logistic, + loss partial)
  // iw (nullable): I - W already formed (build_at), the plain-B form of the GEMM
  void enqueue_data_partial(const double* Wp, const State* st, const double* iw = nullptr) {
    data.enqueue_xw(Wp, st, iw, stream);
    if (loss != MIDAGMA_LOSS_L2) launch_sum_vector(data.loss_part.p, data.loss_part_count, zbuf + D * D, st, stream);
    data.enqueue_xty(zbuf, st, stream);
  }

  // the score partial (and the logistic loss tail) summed over the ranks, in place on the
  // solver stream, while a whole slot is being captured with a communicator attached
  void enqueue_slot_allreduce() {
    if (inslot_comm) comm_allreduce(comm, zbuf, (size_t)(D * D + 64), false, stream);
  }

  // every rank's (status, iters) at a poll: one max all-reduce into agree[slot], copied to h_agree
  void enqueue_agree(int slot) {
    if (!comm) return;
    launch_agree_pack(d_state.p, agree.p + 4 * slot, stream);
    comm_allreduce(comm, agree.p + 4 * slot, 4, true, stream);
    HIP_TRY(hipMemcpyAsync(h_agree.p + 4 * slot, agree.p + 4 * slot, 4 * sizeof(double), hipMemcpyDeviceToHost,
                           stream));
  }
  void check_agree(int slot) const {
    if (!comm) return;
    const double* a = h_agree.p + 4 * slot;
    if (a[0] != -a[2] || a[1] != -a[3])
      throw std::runtime_error("data-parallel replicas diverged: (status, iters) ranges over ranks [" +
                               std::to_string(-a[2]) + ", " + std::to_string(a[0]) + "], [" + std::to_string(-a[3]) +
                               ", " + std::to_string(a[1]) + "] (pin NCCL_ALGO=Ring)");
  }

  // ---- which slot structure runs: the mode predicates ------------------------------------
  // cov mode, l2, d <= 64: the one-workgroup persistent loop (small.hip) instead of graph slots.
  // (float32 W: DS <= 32, whose LDS has room for the float32 |W| image of numpy's L1 sum; the TCC
  // regularizer runs inside it up to d = 32, tcc_blk.h; PST keeps the graph-replayed slots)
  bool small_on() const {
    const int ds = small_block(d);
    return !knobs.no_small && mode == MIDAGMA_MODE_COV && loss == MIDAGMA_LOSS_L2 && ds > 0 && (!w32 || ds <= 32) &&
           (!trek.on || (trek.use_tcc && ds <= 32 && knobs.small_tcc && !w32));
  }
  // cov mode at large D (the 128-tile trailing update): the score GEMM beside the inverse
  bool cov_fork_on() const {
    return knobs.cov_fork != 0 && side != nullptr && mode == MIDAGMA_MODE_COV && blocked() &&
           (D - binv.B2 >= 1792 || knobs.cov_fork == 2) && !trek.on;
  }
  // cov mode at large D, fast slots: the trailing-update look-ahead on two streams
  bool cov_la_on() const {
    return knobs.cov_la && side != nullptr && mode == MIDAGMA_MODE_COV && blocked() && D - binv.B2 >= 1792;
  }
  // data mode: the two-level inverse (its buffers exist) instead of the flat Gauss-Jordan
  bool data_binv_on() const { return !knobs.data_flat_gj && mode == MIDAGMA_MODE_DATA && binv_block(D) > 0; }
  // large data-mode shards (not on the blocked slot structure): the inverse forked beside the GEMMs
  bool forked_inverse() const { return side != nullptr && !blocked() && mode == MIDAGMA_MODE_DATA; }
  // build_at folded into the previous slot's update: fast slots read outer step 0's A^T from A0,
  // which fused_update_at (fast slots) or a build_at after the update (slow slots) wrote from the
  // slot's new W; every call starts with a slow slot, so A0 is never stale
  bool at_fold_on() const {
    return knobs.at_fold > 0 && binv.A0.p && !cov_fork_on() && !df.on() && !knobs.build_resid0;
  }

  // ---- the slot -----------------------------------------------------------
  // build_at on the main stream, then the inverse forked onto the side stream between ev_fork and
  // ev_join, so the GEMMs the caller enqueues next on the main stream run beside it (the inverse is
  // latency-bound, a few % of the chip); join_inverse before anything reads Mt.
  // two_level: the blocked inverse (fast or pivoted: ~5x fewer workgroup-microseconds taken from
  // the GEMMs than the flat Gauss-Jordan's 32 x 1024 workgroups), else the flat Gauss-Jordan
  void fork_inverse(bool two_level, bool fast, int passes) {
    launch_build_at(W.p, D, /*square=*/true, two_level ? binv_build_target(Mt.p, D, binv.w) : Mt.p, D, d, 0.0,
                    d_params.p, d_state.p, stream, IW.p);
    HIP_TRY(hipEventRecord(ev_fork, stream));
    HIP_TRY(hipStreamWaitEvent(side, ev_fork, 0));
    if (two_level)
      launch_blocked_inverse(Mt.p, D, binv.w, fast, gj(), d_state.p, side, passes, nullptr);
    else
      launch_gj_inverse(Mt.p, D, D, gj(), d_state.p, side);
    HIP_TRY(hipEventRecord(ev_join, side));
  }
  void join_inverse() { HIP_TRY(hipStreamWaitEvent(stream, ev_join, 0)); }

  // fast: the outer diagonal blocks by the warm-started product form (blocked() only)
  void enqueue_part1(bool fast = false, int passes = NM_PASSES_RUN) {
    bool gemm_done = false, trek_done = false;
    ctl_folded = false;
    if (cov_fork_on()) {
      // large D, cov mode: the score GEMM (W and cov only) on the main stream, so its tiles fill
      // the CUs the inverse's serial series / panel phases leave idle
      fork_inverse(true, fast, passes);
      enqueue_score_cov(zbuf, d_state.p, /*sum=*/!fast);
      join_inverse();
      gemm_done = true;
    } else if (blocked() && knobs.data_fork_fast && side != nullptr && mode == MIDAGMA_MODE_DATA) {
      // small data-mode shard: the blocked inverse (fast or pivoted) beside the n x d GEMMs, joined
      // before the update
      fork_inverse(true, fast, passes);
      enqueue_data_partial(W.p, d_state.p, IW.p);
      enqueue_slot_allreduce();
      join_inverse();
      gemm_done = true;
    } else if (blocked()) {
      // TCC ('opt', 2d > 128) on a fast cov slot: first, with a short Noda chain that hands the slot
      // back when it does not converge in time (the inverse, GEMM and control of the slot are then
      // no-ops and the host re-runs it with the whole chain); it reads W only, so its place in the
      // slot does not change any result.  Without the fixed-shift stage (knobs.tcc_fix = 0) the chain
      // is knobs.tcc_fast_steps Noda steps (the full TCC_NODA_MAX on pivoted slots); with the stage
      // it is the stage alone (tcc.hip launch_trek_tcc)
      if (fast && knobs.tcc_fast_steps > 0 && trek.tcc_chain(d) && mode == MIDAGMA_MODE_COV) {
        trek.enqueue(W.p, d, D, d_state.p, stream, false, d_state.p, knobs.tcc_fast_steps);
        trek_done = true;
      }
      // cov fast slot: the score GEMM rides in the last trailing update's launch (its split-K
      // slices are what fused_update sums anyway; knobs.fuse_gemm), and the slot's control is
      // decided by the last workgroup of that launch (control.h; knobs.ctl_fold)
      GemmSpec gs{};
      const bool fuse = fast && mode == MIDAGMA_MODE_COV && cov_split > 1 && knobs.fuse_gemm;
      if (fuse) gs = score_cov_spec();
      gemm_done = enqueue_build_inverse(fast, passes, fuse ? &gs : nullptr);
      ctl_folded = fuse && gemm_done && gs.ctl_ticket != nullptr;
    } else if (forked_inverse()) {
      // large data-mode shard: joined below, after the GEMMs.  With the blocked layout the slow
      // (pivoted, no warm start) two-level inverse
      fork_inverse(data_binv_on(), /*fast=*/false, NM_PASSES_RUN);
    } else {
      launch_build_at(W.p, D, /*square=*/true, Mt.p, D, d, 0.0, d_params.p, d_state.p, stream, IW.p);
      launch_gj_inverse(Mt.p, D, D, gj(), d_state.p, stream);
    }
    // (a fork/join of the score GEMMs onto a second stream inside the graph measured slower:
    // the cross-queue dependencies cost more than the overlap gains)
    if (mode == MIDAGMA_MODE_COV) {
      // rhs = ((-mu) cov) @ (I - W)    (linear.py:244); a fast slot leaves the split-K slices
      // for fused_update to sum (its only reader there)
      if (!gemm_done) enqueue_score_cov(zbuf, d_state.p, /*sum=*/!(fast && blocked()));
    } else if (!gemm_done) {
      enqueue_data_partial(W.p, d_state.p, IW.p);
      enqueue_slot_allreduce();  // beside the forked inverse, before the join
      if (forked_inverse()) join_inverse();
    }
    // trek regularizer of this slot's W (linear.py:251-258): every slot in 'opt' mode; in 'log'
    // mode only checkpoint slots, which are never fast slots
    if (trek.on && !trek_done && (trek.cfg.mode == 2 || !(fast && blocked()))) trek.enqueue(W.p, d, D, d_state.p, stream);
  }

  // blocked layout: build_at and the two-level inverse (fast: warm-started diagonal blocks, as
  // one dataflow launch when df.on())
  // fuse (nullable): a GEMM the inverse may carry in its last trailing launch; returns whether it did
  bool enqueue_build_inverse(bool fast, int passes, const GemmSpec* fuse = nullptr) {
    if (fast && df.on()) {
      df.enqueue(W.p, D, d, Mt.p, IW.p, d_params.p, d_state.p, binv.w, passes, stream);
      return false;
    }
    double* ain0 = fast && at_fold_on() ? binv.A0.p : nullptr;  // (built by the previous slot's update)
    // knobs.build_resid0 (experiments build): outer block 0's residual rides in build_at's launch on
    // fast slots at B2 = 256 (one dependent launch fewer, but measured slower: DESIGN 8)
    const bool resid0 = fast && IW.p == nullptr && binv_block(D) == 256 && !cov_la_on() && knobs.build_resid0;
#ifdef MIDAGMA_EXPERIMENTS
    if (resid0)
      launch_build_resid0(W.p, D, binv_build_target(Mt.p, D, binv.w), D, d, d_params.p, binv.w, d_state.p, stream);
#endif
    if (!resid0 && !ain0)
      launch_build_at(W.p, D, /*square=*/true, binv_build_target(Mt.p, D, binv.w), D, d, 0.0, d_params.p, d_state.p,
                      stream, IW.p);
    if (fast && cov_la_on()) {
      const TrailLookAhead tla = binv.lookahead(D, side);
      return launch_blocked_inverse(Mt.p, D, binv.w, fast, gj(), d_state.p, stream, passes, fuse, &tla, false, ain0);
    }
    return launch_blocked_inverse(Mt.p, D, binv.w, fast, gj(), d_state.p, stream, passes, fuse, nullptr, resid0, ain0);
  }

  // fast (blocked cov slots): the domain flags come from the inverse's last outer step and the
  // score slices are summed inside fused_update; fast slots never carry a checkpoint
  void enqueue_part2(bool fast = false) {
    const bool lean = fast && blocked();
    if (!lean) launch_reduce_check(Mt.p, W.p, zbuf, d_params.p, d_state.p, partials.p, d, D, stream);
    // float32 W: numpy's float32 L1 sum for the checkpoint objective (np_sum.h; checkpoint slots
    // are never lean)
    const bool l1f = w32 && l1w.p && !lean;
    if (l1f) launch_np_l1(W.p, d, D, d_state.p, reinterpret_cast<float*>(l1w.p + 1), l1w.p, stream);
    if (!(lean && ctl_folded))  // (else decided at the end of the slot's last trailing launch)
      launch_control(d_params.p, d_state.p, partials.p, pivlog.p, zbuf + D * D, bc_table.p, d_ckpt.p, ckpt_cap,
                     npart.p, d, trek.scal(), stream, l1f ? l1w.p : nullptr);
    const bool slices = lean && mode == MIDAGMA_MODE_COV && cov_split > 1;
    const double* tg = trek.opt_mode() ? trek.G.p : nullptr;
    if (lean && at_fold_on()) {  // the next slot's build_at in the update
      launch_fused_update_at(d_params.p, d_state.p, W.p, m.p, v.p, Mt.p, slices ? cov_parts.p : zbuf,
                             slices ? cov_split : 1, D * D, cov.p, has_inc ? minc.p : nullptr,
                             has_exc ? mexc.p : nullptr, tg, d, D, binv.A0.p, IW.p, npart.p, stream);
      return;
    }
    launch_fused_update(d_params.p, d_state.p, W.p, m.p, v.p, Mt.p, slices ? cov_parts.p : zbuf,
                        slices ? cov_split : 1, D * D, cov.p, has_inc ? minc.p : nullptr, has_exc ? mexc.p : nullptr,
                        tg, d, D, npart.p, stream);
    if (blocked() && at_fold_on())  // slow slot: the next (fast) slot's A^T and I - W from the new W
      launch_build_at(W.p, D, /*square=*/true, binv.A0.p, D, d, 0.0, d_params.p, d_state.p, stream, IW.p);
  }

  // blocked slots enqueued launch by launch instead of replayed graphs (knobs.eager: at large D
  // the host runs far ahead of a multi-ms slot, and cross-stream waits are plain queue barriers
  // instead of graph edges)
  void run_eager(bool fast, int passes, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
      enqueue_part1(fast, passes);
      enqueue_part2(fast);
    }
  }

  struct StreamSwap {  // `stream` set to another stream for a scope (the captures)
    midagma_solver* s;
    hipStream_t saved;
    StreamSwap(midagma_solver* s_, hipStream_t to) : s(s_), saved(s_->stream) { s->stream = to; }
    ~StreamSwap() { s->stream = saved; }
  };

  // which: 1 part 1, 2 part 2, 4 fast; on graphs' capture stream (slot_graphs.h)
  hipGraphExec_t capture(int which, int reps = 1, int passes = NM_PASSES_RUN) {
    if (group) return group_capture(group, this, which, reps, passes);
    hipGraph_t graph = nullptr;
    StreamSwap on_cap(this, graphs.capture_stream());
    HIP_TRY(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    inslot_comm = comm != nullptr && mode == MIDAGMA_MODE_DATA && (which & 3) == 3;
    try {
      for (int r = 0; r < reps; ++r) {
        if (which & 1) enqueue_part1((which & 4) != 0, passes);
        if (which & 2) enqueue_part2((which & 4) != 0);
      }
      inslot_comm = false;
    } catch (...) {
      inslot_comm = false;
      (void)hipStreamEndCapture(stream, &graph);
      if (graph) (void)hipGraphDestroy(graph);
      throw;
    }
    HIP_TRY(hipStreamEndCapture(stream, &graph));
    hipGraphExec_t exec = nullptr;
    HIP_TRY(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    HIP_TRY(hipGraphDestroy(graph));
    return exec;
  }

  void ensure_graphs() {
    graphs.ensure(blocked(), knobs.fast_group, knobs.nm_adapt,
                  [this](int which, int reps, int passes) { return capture(which, reps, passes); });
  }

  // ---- a call: begin, the drivers, finish ----------------------------------------------
  void begin(const double* Wh, double mu_, int64_t max_iter, double s, double lr, double tol, double b1, double b2,
             double lambda1, int64_t checkpoint) {
    if (mode == MIDAGMA_MODE_COV && !has_cov) throw std::invalid_argument("set_cov before minimize");
    if (mode == MIDAGMA_MODE_DATA && !has_data) throw std::invalid_argument("set_data before minimize");
    if (loss == MIDAGMA_LOSS_LOGISTIC && !has_cov) throw std::invalid_argument("logistic needs cov (cov_from_zbuf)");
    if (max_iter < 1 || checkpoint < 1) throw std::invalid_argument("max_iter and checkpoint must be >= 1");
    mu = mu_;
    ensure_bc_table(b1, b2, max_iter);
    ensure_ckpt(max_iter, checkpoint);
    Params p = cov_l2_params(d, D, mu_, s, lambda1, tol, b1, b2, max_iter, checkpoint, bc_len, has_inc, has_exc);
    // (float32 W: mu * lambda1 * sign(W) is a float32 array, linear.py:248)
    if (w32) p.mu_l1 = f32r(mu_ * lambda1);
    p.w32 = w32 ? 1 : 0;
    p.logistic = loss == MIDAGMA_LOSS_LOGISTIC;
    p.trek_weight = trek.on ? trek.cfg.weight : 0.0;
    p.trek_mode = trek.on ? trek.cfg.mode : 0;
    const double n = (double)data.n_global;
    if (mode == MIDAGMA_MODE_COV) {
      // cov_l2_params' scales: Z already is ((-mu) cov) @ (I - W)
    } else if (loss == MIDAGMA_LOSS_L2) {
      p.zscale = -mu_ / n;
      p.cscale = 0.0;
      p.score_scale = 0.5 / n;
    } else {
      logistic_data_params(p, mu_, n);
    }
    hp = p;
    HIP_TRY(hipMemcpyAsync(d_params.p, &hp, sizeof(Params), hipMemcpyHostToDevice, stream));
    h_state.p[0] = initial_state(lr);
    HIP_TRY(hipMemcpyAsync(d_state.p, &h_state.p[0], sizeof(State), hipMemcpyHostToDevice, stream));
    if (mode == MIDAGMA_MODE_COV) {
      launch_scale(cov.p, -mu_, covs.p, D * D, stream);  // (-mu) * cov
      launch_transpose(covs.p, D, D, D, covsT.p, D, stream);
    }
    upload_matrix(W, Wh, d);
    const size_t DD = (size_t)D * D;
    for (DevBuf<>* b : {&m, &v}) HIP_TRY(hipMemsetAsync(b->p, 0, DD * sizeof(double), stream));
    HIP_TRY(hipMemsetAsync(scarry.p, 0, scarry.n * sizeof(double), stream));  // no warm start yet
    HIP_TRY(hipStreamSynchronize(stream));  // h_state[0] reused as a snapshot slot below
    binv.fast_ready = false;  // the first slot of a call runs the GJ path (warm starts are stale)
    binv.three_pass_left = 0;
    begun = true;
  }

  void snapshot(int slot) {
    HIP_TRY(hipMemcpyAsync(&h_state.p[slot], d_state.p, sizeof(State), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(ev[slot], stream));
  }

  static bool terminal(const State& s) { return s.status != ST_RUNNING; }

  // Cov mode with the blocked inverse: fast slots in batches, a GJ (slow) slot wherever a
  // log-det is due (checkpoint), there is no warm start (first slot) or a fast slot handed
  // back (ST_NEED_GJ).  Batches stop at the next checkpoint iteration, so the host knows
  // when the slow slot is due; one host sync per batch (the choices: slot_sched.h, BlockedScheduler).
  // n_slots < 0: until terminal.
  void drive_blocked(int64_t n_slots) {
    ensure_graphs();
    const int fast_group = knobs.fast_group;
    BlockedScheduler::Carry carry;
    carry.bmax = fast_batch;
    carry.three_pass_left = binv.three_pass_left;
    carry.fast_ready = binv.fast_ready;
    BlockedScheduler sc(hp.max_iter, hp.checkpoint, n_slots, fast_group, graphs[SlotGraphs::FAST2] != nullptr, carry);
    HIP_TRY(hipMemcpyAsync(&h_state.p[1], d_state.p, sizeof(State), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (SlotView cur = view(h_state.p[1]);;) {
      const BlockedPlan p = sc.next(cur);
      if (p.done) break;
      if (p.clear_handback) {
        static const int32_t running = ST_RUNNING;
        if (group)
          group_clear_handback(group);
        else
          HIP_TRY(hipMemcpyAsync(&d_state.p->status, &running, sizeof(int32_t), hipMemcpyHostToDevice, stream));
      }
      if (knobs.eager) {
        if (p.slow) run_eager(false, NM_PASSES_RUN, 1);
        run_eager(true, p.two_pass ? 2 : NM_PASSES_RUN, p.groups * fast_group + p.singles);
      } else {
        if (p.slow) HIP_TRY(hipGraphLaunch(graphs[SlotGraphs::FULL], stream));  // pivots + fresh warm starts
        // (a hand-back inside a group turns the group's later slots into no-op launches)
        hipGraphExec_t one = graphs[p.two_pass ? SlotGraphs::FAST2 : SlotGraphs::FAST];
        hipGraphExec_t grp = graphs[p.two_pass ? SlotGraphs::FASTN2 : SlotGraphs::FASTN];
        for (int64_t b = 0; b < p.groups; ++b) HIP_TRY(hipGraphLaunch(grp, stream));
        for (int64_t b = 0; b < p.singles; ++b) HIP_TRY(hipGraphLaunch(one, stream));
      }
      HIP_TRY(hipMemcpyAsync(&h_state.p[1], d_state.p, sizeof(State), hipMemcpyDeviceToHost, stream));
      enqueue_agree(0);
      HIP_TRY(hipStreamSynchronize(stream));
      check_agree(0);
      check_group_stop();
      cur = view(h_state.p[1]);
      sc.observe(cur);
    }
    fast_batch = sc.carry().bmax;
    binv.three_pass_left = sc.carry().three_pass_left;
    binv.fast_ready = sc.carry().fast_ready;
    handback_count += sc.handbacks();
    if (const int to = df.timeouts()) throw std::runtime_error("one-launch inverse: " + std::to_string(to) + " wait timeouts");
    if (knobs.debug_handbacks)  // diagnostics (experiments build)
      fprintf(stderr, "drive_blocked: %lld slots, %lld hand-backs\n", (long long)sc.launched(), (long long)sc.handbacks());
  }
  static SlotView view(const State& st) {
    SlotView v;
    v.status = st.status;
    v.ckpt_pending = st.ckpt_pending;
    v.iter = st.iter;
    v.slots = st.slots;
    return v;
  }

  // Small d: the whole inner loop in one persistent workgroup, kSmallBatch slots per launch
  // (one host sync per launch).  n_slots < 0: until terminal.
  static constexpr int64_t kSmallBatch = 4096;
  void drive_small(int64_t n_slots) {
    const int64_t cap = slot_cap(hp.max_iter, hp.checkpoint);
    const bool tcc = trek.on && trek.use_tcc;
    for (int64_t launched = 0;;) {
      const int64_t B = small_next_batch(n_slots, launched, cap, kSmallBatch);
      if (B <= 0) break;
      SmallTcc tc{};
      if (tcc) {
        const TccCfg& c = trek.tcc.cfg;
        const TccWork& w = trek.tcc.w;
        tc = SmallTcc{w.S, c.w, c.eps, (double)c.m, c.weight, c.mode, w.scal, w.vprev, w.uprev, w.fix};
      }
      const SmallArrays arr{d_params.p, d_state.p, W.p, m.p, v.p, covs.p, has_inc ? minc.p : nullptr,
                            has_exc ? mexc.p : nullptr, bc_table.p, d_ckpt.p, ckpt_cap, scarry.p, sprev.p};
      SmallRun run{d, B};
      run.w32 = w32;
      run.tcc = tcc ? &tc : nullptr;
      launch_small_minimize(arr, run, stream);
      launched += B;
      HIP_TRY(hipMemcpyAsync(&h_state.p[1], d_state.p, sizeof(State), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      if (terminal(h_state.p[1])) break;
    }
  }

  // n slots of a begun call (midagma_run_slots)
  void run_slots(int64_t n) {
    if (blocked()) return drive_blocked(n);
    if (small_on()) return drive_small(n);
    for (int64_t i = 0; i < n; ++i) HIP_TRY(hipGraphLaunch(graphs[SlotGraphs::FULL], stream));
  }

  void run_loop(int64_t max_iter, int64_t checkpoint) {
    if (blocked()) {
      drive_blocked(-1);
      return;
    }
    if (small_on()) {
      drive_small(-1);
      return;
    }
    ensure_graphs();
    const int64_t cap = slot_cap(max_iter, checkpoint);
    int64_t launched = 0, known_iter = 0;
    int cur = 0, pending = -1;
    bool stop = false;
    while (!stop) {
      const int64_t B = graph_next_batch(max_iter, known_iter);
      for (int64_t b = 0; b < B; ++b) HIP_TRY(hipGraphLaunch(graphs[SlotGraphs::FULL], stream));
      launched += B;
      enqueue_agree(cur);
      snapshot(cur);
      if (pending >= 0) {
        HIP_TRY(hipEventSynchronize(ev[pending]));
        check_agree(pending);
        check_group_stop();
        known_iter = h_state.p[pending].iter;
        if (terminal(h_state.p[pending])) stop = true;
      }
      pending = cur;
      cur ^= 1;
      if (!stop && launched > cap) throw std::runtime_error("minimize: slot budget exceeded (controller stuck)");
    }
    HIP_TRY(hipStreamSynchronize(stream));
  }

  void finish(double* Wh, midagma_result* res) {
    HIP_TRY(hipMemcpyAsync(&h_state.p[0], d_state.p, sizeof(State), hipMemcpyDeviceToHost, stream));
    download_matrix(Wh, W.p);
    HIP_TRY(hipStreamSynchronize(stream));
    begun = false;
    check_handoff(h_state.p[0]);
    fill_result(h_state.p[0], res);
  }

  // A bounded in-kernel hand-off wait expired (ST_HANDOFF_TIMEOUT; never expected): the late
  // first half has finished with its launch, so its word is cleared here, and the call raises
  // instead of reporting a numerical outcome.
  void check_handoff(const State& s) {
    if (s.status != ST_HANDOFF_TIMEOUT) return;
    begun = false;
    data.clear_sig_flags(stream);
    HIP_TRY(hipStreamSynchronize(stream));
    throw std::runtime_error("sigmoid GEMM: a K-half hand-off wait timed out (50 ms); the step was not applied");
  }

  static void fill_result(const State& s, midagma_result* res) {
    if (!res) return;
    res->iters = s.iter;
    res->halvings = s.halvings;
    res->slots = s.slots;
    res->n_checkpoints = s.n_ckpt;
    res->status = s.status == ST_NEED_GJ ? ST_RUNNING : s.status;  // internal hand-back, not an outcome
    res->early_stop = s.early_stop;
    res->lr_final = s.lr;
    res->obj_last = s.obj_last;
    res->score_last = s.score_last;
    res->h_last = s.h_last;
    res->l1_last = s.l1_last;
  }

  // ---- evaluations of a given W and diagnostics: defined in solver.hip -----------------------
  void eval_trek(const double* Wh, double* value, double* G);
  void eval_h(const double* Wh, double s_dom, double* h, double* G);
  void eval_score(const double* Wh, double* loss_out, double* G);
  void score_partial(const double* Wh);
  void score_finish(double* loss_out, double* G);
  void trace_l1(const double* Wd, const double* Z, double* sd, double* l1);
  void profile_parts(int reps, double* ms_out);
};
