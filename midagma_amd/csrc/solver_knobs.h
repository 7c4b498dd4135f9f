// The experiment knobs of the solver handle (solver_impl.h, solver.hip), each once: its name, type,
// default and meaning.  Plain C++ (no HIP header), so tests/test_knobs.py builds it with g++.
//
// midagma_create fills one SolverKnobs by read(), and the handle keeps it as `knobs`: every knob is
// read once per handle, at creation.  The product library's read() returns the defaults and names
// no variable (knobs.h); the experiments build (-DMIDAGMA_EXPERIMENTS) reads MIDAGMA_EXP_<NAME>.
// The launch files' own knobs (blockinv.hip, gemm.hip, tcc.hip, small.hip, step.hip) are not here.
// DESIGN.md section 8 has the measurement behind each default.
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/midagma_hip.h"
#include "knobs.h"

namespace midagma {

struct SolverKnobs {
  // --- which slot structure runs ---
  bool no_fork = false;        // NO_FORK (set): data mode without the side stream (the inverse in sequence)
  bool no_small = false;       // NO_SMALL (set): d <= 64 on the graph slots, not the one-workgroup loop
  bool small_tcc = true;       // SMALL_TCC: 0 keeps TCC (d <= 32) on the graph slots
  bool nm_adapt = true;        // NM_ADAPT: 0 drops the 2-pass fast graphs (always NM_PASSES_RUN passes)
  int cov_fork = 0;            // COV_FORK: 1 the cov score GEMM beside the inverse at D - B2 >= 1792; 2 at every blocked D
  bool cov_la = false;         // COV_LA: 1 the trailing-update look-ahead on two streams (D - B2 >= 1792)
  bool eager = false;          // EAGER: 1 blocked slots enqueued launch by launch instead of replayed graphs
  bool data_flat_gj = false;   // DATA_FLAT_GJ (set): data mode keeps the flat Gauss-Jordan at every D
  bool data_fork_fast = true;  // DATA_FORK_FAST: 0 runs a small shard's blocked inverse in sequence
                               // (forked: logistic d=1000, n=1e4 1085 -> 1118, l2 1130 -> 1168 steps/s)
  int64_t data_fast_rows = 16384;  // DATA_FAST_ROWS: shards up to this n_pad run the cov-mode slot structure
  int fast_group = 4;          // FAST_GROUP: fast slots per grouped graph (>= 1)
  // --- the blocked cov slot ---
  bool fuse_gemm = true;       // FUSE_GEMM: 0 keeps the score GEMM out of the last trailing launch
  bool ctl_fold = true;        // CTL_FOLD: 0 launches control_kernel instead of the folded control
  // AT_FOLD: build_at folded into the previous slot's update: 1 on, 0 off, -1 the rule 1024 <= D <= 1408
  // (D = 1024 +1.7 %, 1408 +0.6 %, 512 -4 %, 2048 -1.2 %); alloc_core resolves -1, and
  // midagma_debug_at_fold writes it
  int at_fold = -1;
  bool build_resid0 = false;   // BUILD_RESID0: 1 block 0's residual in build_at's launch (measured slower)
  int cov_split = -1;          // COV_SPLIT: the cov score GEMM's split-K; -1 (unset) the size rule
  bool cov_pad256 = true;      // COV_PAD256: 0 keeps 129 <= d <= 192 at D = 192 in cov mode
  int cov_pad_b2 = -1;         // COV_PAD_B2: D to a 256-multiple: 0 never, 1 at every d > 256, -1 (unset) d <= 640
  int gemm_ses = 0;            // GEMM_SES: > 0 confines the forked score GEMM to that many shader engines per XCD
  bool df = false;             // DF: 1 the fast inverse as one dataflow launch (dfinv.hip; measured slower)
  int df_per_cu = 2;           // DF_PER_CU: its workgroups per CU (1 or 2)
  // --- TCC on the graph slots (2d > 128) ---
  int tcc_fast_steps = 5;      // TCC_FAST_STEPS: Noda steps of a fast slot's chain; 0 the whole gated chain
  int tcc_fix = 1;             // TCC_FIX: 0 no fixed-shift stage before Noda
  int tcc_fix_pre = 1;         // TCC_FIX_PRE: Noda steps before the stage on fast slots after a hard stage
  int tcc_fix_hold = 8;        // TCC_FIX_HOLD: ... for this many slots (8 against 1: d = 1000 from W = 0
                               // 9.8 -> 8.0 ms a step, d = 300 1.30 -> 0.98)
  int tcc_fix_easy = 0;        // TCC_FIX_EASY: > 0 the sweep count that still counts as easy
  // TCC_FASTBLK: 0 keeps every outer block of the stage's inverse (D2 >= 2048) on the pivoted path
  // (d = 1000: 1.83 -> 1.40 ms a step after 1300 steps; from W = 0 8.0 -> 10.4 over the first 30-odd)
  bool tcc_fastblk = true;
  // TCC_BINV: the shifted inverses on the blocked inverse: 1 from D2 >= 2048, 2 from D2 >= 512, 0 never
  // (d = 1000 6.01 -> 5.36 ms a step, but d = 500 2.04 -> 2.41 and d = 300 1.07 -> 1.34)
  int tcc_binv = 1;
  // --- data mode ---
  int64_t prepad_mb = 0;       // PREPAD_MB: device memory kept allocated before X (placement experiments)
  int sig_split = 1;           // SIG_SPLIT: 0 never splits the logistic sigmoid GEMM in two K halves
  int64_t y_offset = 0;        // Y_OFFSET: bytes Y is shifted into its allocation (L2 set aliasing with X)
  int data_split = -1;         // DATA_SPLIT: the X^T Y split-K (and no Strassen form); -1 (unset) the size rule
  bool xw_fullk = false;       // XW_FULLK: 1 the X (I - W) GEMM's k loop over all of D
  // --- diagnostics (MIDAGMA_DEBUG_HANDBACKS set): drive_blocked prints its hand-back count ---
  bool debug_handbacks = false;

  static SolverKnobs read() {
    SolverKnobs k;
#ifdef MIDAGMA_EXPERIMENTS
    k.no_fork = knob_set("MIDAGMA_EXP_NO_FORK");
    k.no_small = knob_set("MIDAGMA_EXP_NO_SMALL");
    k.small_tcc = knob("MIDAGMA_EXP_SMALL_TCC", 1) != 0;
    k.nm_adapt = knob("MIDAGMA_EXP_NM_ADAPT", 1) != 0;
    k.cov_fork = (int)knob("MIDAGMA_EXP_COV_FORK", 0);
    k.cov_la = knob("MIDAGMA_EXP_COV_LA", 0) != 0;
    k.eager = knob("MIDAGMA_EXP_EAGER", 0) != 0;
    k.data_flat_gj = knob_set("MIDAGMA_EXP_DATA_FLAT_GJ");
    k.data_fork_fast = knob("MIDAGMA_EXP_DATA_FORK_FAST", 1) != 0;
    k.data_fast_rows = knob("MIDAGMA_EXP_DATA_FAST_ROWS", 16384);
    k.fast_group = std::max(1, (int)knob("MIDAGMA_EXP_FAST_GROUP", 4));
    k.fuse_gemm = knob("MIDAGMA_EXP_FUSE_GEMM", 1) != 0;
    k.ctl_fold = knob("MIDAGMA_EXP_CTL_FOLD", 1) != 0;
    k.at_fold = (int)knob("MIDAGMA_EXP_AT_FOLD", -1);
    k.build_resid0 = knob("MIDAGMA_EXP_BUILD_RESID0", 0) != 0;
    k.cov_split = (int)knob("MIDAGMA_EXP_COV_SPLIT", -1);
    k.cov_pad256 = knob("MIDAGMA_EXP_COV_PAD256", 1) != 0;
    k.cov_pad_b2 = (int)knob("MIDAGMA_EXP_COV_PAD_B2", -1);
    k.gemm_ses = (int)knob("MIDAGMA_EXP_GEMM_SES", 0);
    k.df = knob("MIDAGMA_EXP_DF", 0) != 0;
    k.df_per_cu = std::max(1, std::min(2, (int)knob("MIDAGMA_EXP_DF_PER_CU", 2)));
    k.tcc_fast_steps = (int)knob("MIDAGMA_EXP_TCC_FAST_STEPS", 5);
    k.tcc_fix = (int)knob("MIDAGMA_EXP_TCC_FIX", 1);
    k.tcc_fix_pre = (int)knob("MIDAGMA_EXP_TCC_FIX_PRE", 1);
    k.tcc_fix_hold = (int)knob("MIDAGMA_EXP_TCC_FIX_HOLD", 8);
    k.tcc_fix_easy = (int)knob("MIDAGMA_EXP_TCC_FIX_EASY", 0);
    k.tcc_fastblk = knob("MIDAGMA_EXP_TCC_FASTBLK", 1) != 0;
    k.tcc_binv = (int)knob("MIDAGMA_EXP_TCC_BINV", 1);
    k.prepad_mb = knob("MIDAGMA_EXP_PREPAD_MB", 0);
    k.sig_split = (int)knob("MIDAGMA_EXP_SIG_SPLIT", 1);
    k.y_offset = knob("MIDAGMA_EXP_Y_OFFSET", 0);
    k.data_split = (int)knob("MIDAGMA_EXP_DATA_SPLIT", -1);
    k.xw_fullk = knob("MIDAGMA_EXP_XW_FULLK", 0) != 0;
    k.debug_handbacks = knob_set("MIDAGMA_DEBUG_HANDBACKS");
#endif
    return k;
  }
};

// The padded node dimension D of a d-node solver (what midagma_padded_dim returns).
// 128-multiples feed the 128x128 GEMM tiles (d > 192; up to 192 the next 64-multiple).  Cov mode pads
// 129 <= d <= 192 to 256 as well: the blocked inverse then has one 256-wide outer block, and its
// warm-started product form beats the flat Gauss-Jordan's 6 block steps on 192 (data mode keeps 192:
// X's columns are GEMM work).
// Cov mode, 256 < d <= 640: D to a multiple of 256, so the blocked inverse runs B2 = 256 outer
// blocks (2 instead of 3 at D = 384 -> 512, 3 instead of 5 at 640 -> 768: d=300 11.1k -> 11.3k,
// d=600 6.4k -> 7.0k steps/s).  Larger D keep B2 = 128 (d=1150 even, d=1400 -3.5%, d=1700
// even: the padded GEMM work outweighs the saved outer steps).
inline int64_t padded_dim(int64_t d, int mode, const SolverKnobs& k) {
  const bool cov = mode == MIDAGMA_MODE_COV;
  if (cov && d > 256 && (k.cov_pad_b2 == 1 || (k.cov_pad_b2 < 0 && d <= 640))) return (d + 255) / 256 * 256;
  return d > 192 || (cov && k.cov_pad256 && d > 128) ? (d + 127) / 128 * 128 : (d + 63) / 64 * 64;
}

}  // namespace midagma
