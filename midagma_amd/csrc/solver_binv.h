// The two-level blocked inverse of the solver handle (blockinv.hip; cov mode at D >= 256, and
// data mode wherever binv_block(D) > 0): its buffers, the launch view over them (BInvWork, built
// once in alloc), and what the host carries between slots for its warm-started fast path.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "devmem.h"
#include "launch.h"
#include "solver_knobs.h"

namespace midagma {

struct BlockedInv {
  int B2 = 0;  // outer block width of the slots (0: the flat Gauss-Jordan slots)
  DevBuf<> Malt, Pst2, Pst2b, nmY0, nmY1, nmQ0, nmQ1, nmP, nmPart, nmDone, nmLW, nmLZ, nmLPZ, nmSync;
  DevBuf<> A0;          // outer step 0's A^T of the next fast slot (knobs.at_fold; fused_update_at writes it)
  DevBuf<> ctl_ticket;  // the folded control's workgroup ticket (control.h)
  bool fast_ready = false;      // Pst2 holds the previous slot's outer-block inverses
  int64_t three_pass_left = 0;  // fast slots still to run with 3 passes (after a 2-pass hand-back)
  std::vector<Event> la_own;      // the look-ahead's events ...
  std::vector<hipEvent_t> la_ev;  // ... and their handles as one array (TrailLookAhead)
  BInvWork w{};

  bool on() const { return B2 > 0; }
  const BInvWork& work() const { return w; }

  // knobs.at_fold is resolved (0 / 1) by the caller
  void alloc(int64_t D, int mode, const SolverKnobs& knobs, hipStream_t stream) {
    const size_t DD = (size_t)D * D;
    const bool cov = mode == MIDAGMA_MODE_COV;
    if (cov) B2 = binv_block(D);
    if (cov && B2 > 0) {
      ctl_ticket.alloc(1);
      HIP_TRY(hipMemsetAsync(ctl_ticket.p, 0, sizeof(double), stream));
    }
    if (knobs.at_fold > 0 && cov && B2 > 0) A0.alloc(DD);
    if (on() || (!knobs.data_flat_gj && mode == MIDAGMA_MODE_DATA && binv_block(D) > 0)) {
      const int64_t b2 = binv_block(D);
      Malt.alloc(DD);
      Pst2.alloc((size_t)D * b2);
      Pst2b.alloc((size_t)D * b2);
      for (DevBuf<>* b : {&nmY0, &nmY1, &nmQ0, &nmQ1, &nmP, &nmLW, &nmLZ, &nmLPZ}) b->alloc((size_t)b2 * b2);
      nmPart.alloc((size_t)(D / b2) * (NM_PASSES + 1) * PART_STRIDE);
      nmDone.alloc(D / b2);
      nmSync.alloc((size_t)(D / b2) * 128);  // 256 ints per block (launch_trail128_series' counters)
      // the counters must start at 0; the others so that no slot's result depends on what the
      // memory held before (which buffer a solver gets back follows the order of earlier frees)
      for (DevBuf<>* b : {&nmSync, &Malt, &Pst2, &Pst2b, &nmY0, &nmY1, &nmQ0, &nmQ1, &nmP, &nmLW, &nmLZ, &nmLPZ,
                          &nmPart, &nmDone})
        HIP_TRY(hipMemsetAsync(b->p, 0, b->n * sizeof(double), stream));
    }
    w = BInvWork{Malt.p,
                 Pst2.p,
                 Pst2b.p,
                 {nmY0.p, nmY1.p},
                 {nmQ0.p, nmQ1.p},
                 nmP.p,
                 nmPart.p,
                 reinterpret_cast<int*>(nmDone.p),
                 nmLW.p,
                 nmLZ.p,
                 nmLPZ.p,
                 reinterpret_cast<int*>(nmSync.p)};
  }

  // Data mode: small shards (n_pad <= knobs.data_fast_rows) run the cov-mode slot structure: the
  // warm-started fast blocked inverse in sequence with the GEMMs (hand-backs and checkpoint slots on
  // the pivoted path).  Forked beside GEMMs that fill the chip, the pivoted inverse's 20-odd dependent
  // launches wait for CU slots and end after the GEMMs (logistic d=1000, n=1e4: 1.01 ms per slot for
  // 0.70 ms of GEMMs); large shards keep the fork, which hides it.  Returns whether B2 changed.
  bool set_data_rows(int64_t D, int64_t n_pad, const SolverKnobs& knobs) {
    const int b2 = binv_block(D);
    const int B2_new = (b2 > 0 && n_pad <= knobs.data_fast_rows && Malt.p) ? b2 : 0;
    const bool changed = B2_new != B2;
    B2 = B2_new;
    return changed;
  }

  // the 2 K2 + 2 events of the trailing-update look-ahead (blockinv.hip blocked_inverse_lookahead)
  TrailLookAhead lookahead(int64_t D, hipStream_t side) {
    const int64_t K2 = D / B2;
    while ((int64_t)la_ev.size() < 2 * K2 + 2) {
      la_own.emplace_back();
      la_own.back().create(hipEventDisableTiming);
      la_ev.push_back(la_own.back());
    }
    return TrailLookAhead{side, la_ev.data()};
  }
};

}  // namespace midagma
