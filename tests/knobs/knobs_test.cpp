// Prints the solver handle's knob table (csrc/solver_knobs.h) as read from this process's
// environment, one "name=value" line per field, then padded_dim for a list of d in both modes.
// Built by tests/test_knobs.py with and without -DMIDAGMA_EXPERIMENTS; plain C++, no HIP.
#include "solver_knobs.h"
#include "solver_knobs.h"  // (twice: the header guards itself)

#include <cstdio>

int main() {
  const midagma::SolverKnobs k = midagma::SolverKnobs::read();
#define SHOW(field) std::printf(#field "=%lld\n", (long long)k.field)
  SHOW(no_fork);
  SHOW(no_small);
  SHOW(small_tcc);
  SHOW(nm_adapt);
  SHOW(cov_fork);
  SHOW(cov_la);
  SHOW(eager);
  SHOW(data_flat_gj);
  SHOW(data_fork_fast);
  SHOW(data_fast_rows);
  SHOW(fast_group);
  SHOW(fuse_gemm);
  SHOW(ctl_fold);
  SHOW(at_fold);
  SHOW(build_resid0);
  SHOW(cov_split);
  SHOW(cov_pad256);
  SHOW(cov_pad_b2);
  SHOW(gemm_ses);
  SHOW(df);
  SHOW(df_per_cu);
  SHOW(tcc_fast_steps);
  SHOW(tcc_fix);
  SHOW(tcc_fix_pre);
  SHOW(tcc_fix_hold);
  SHOW(tcc_fix_easy);
  SHOW(tcc_fastblk);
  SHOW(tcc_binv);
  SHOW(prepad_mb);
  SHOW(sig_split);
  SHOW(y_offset);
  SHOW(data_split);
  SHOW(xw_fullk);
  SHOW(debug_handbacks);
#undef SHOW
  for (const int mode : {MIDAGMA_MODE_COV, MIDAGMA_MODE_DATA})
    for (const long long d : {64, 65, 128, 129, 192, 193, 256, 257, 640, 641, 1100})
      std::printf("D[%s,%lld]=%lld\n", mode == MIDAGMA_MODE_COV ? "cov" : "data", d,
                  (long long)midagma::padded_dim(d, mode, k));
  return 0;
}
