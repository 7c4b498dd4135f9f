// The captured slot graphs of the solver handle (solver_impl.h) and the stream they are
// captured on.
#pragma once

#include <hip/hip_runtime.h>

#include "launch.h"

namespace midagma {

struct SlotGraphs {
  // FULL / PART1 / PART2: one slot, and its two parts alone (the host-driven all-reduce between)
  // FAST: one fast slot (blocked inverse only); FASTN: fast_group of them in one graph (no
  // inter-graph dispatch gap between them)
  // FAST2 / FASTN2: the same with 2 product-form passes per outer block (the extrapolated warm
  // start usually converges in 2); the host falls back to 3 for a while after a hand-back
  enum Id { FULL, PART1, PART2, FAST, FASTN, FAST2, FASTN2, COUNT };
  hipGraphExec_t g[COUNT] = {};
  bool valid = false;
  // Slot graphs are captured on a stream of the solver's own and launched on its `stream`: a caller
  // (torch's process group, DagmaLinear's host-driven all-reduce) may record events on `stream`, and
  // HIP refuses any query of an event recorded on a stream that is capturing (torch's NCCL
  // watchdog aborted the process on such a query while a capture ran).
  hipStream_t cap = nullptr;

  hipGraphExec_t operator[](Id id) const { return g[id]; }
  hipStream_t capture_stream() {
    if (!cap) HIP_TRY(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
    return cap;
  }
  void destroy() {
    for (hipGraphExec_t& ge : g)
      if (ge) {
        (void)hipGraphExecDestroy(ge);
        ge = nullptr;
      }
    valid = false;
  }
  // capture(which, reps, passes) -> hipGraphExec_t; which: 1 part 1, 2 part 2, 4 a fast slot
  template <class Capture>
  void ensure(bool blocked, int fast_group, bool nm_adapt, Capture&& capture) {
    if (valid) return;
    destroy();
    const bool grp = blocked && fast_group > 1;
    const struct {
      Id id;
      int which, reps, passes;
      bool wanted;
    } table[] = {{FULL, 3, 1, NM_PASSES_RUN, true},
                 {PART1, 1, 1, NM_PASSES_RUN, true},
                 {PART2, 2, 1, NM_PASSES_RUN, true},
                 {FAST, 3 | 4, 1, NM_PASSES_RUN, blocked},
                 {FASTN, 3 | 4, fast_group, NM_PASSES_RUN, grp},
                 {FAST2, 3 | 4, 1, 2, blocked && nm_adapt},
                 {FASTN2, 3 | 4, fast_group, 2, grp && nm_adapt}};
    for (const auto& row : table)
      if (row.wanted) g[row.id] = capture(row.which, row.reps, row.passes);
    valid = true;
  }
};

}  // namespace midagma
