// The fast slot's inverse as one dataflow launch (dfinv.hip; MIDAGMA_EXP_DF=1: measured slower than
// the launch-per-phase inverse, DESIGN.md section 8): its buffers, the two task plans (2 and 3
// product-form passes) and the launch view over them.  Included by solver_impl.h under
// MIDAGMA_EXPERIMENTS; the product build holds an empty stand-in of the same name there.
namespace midagma {

struct DfInverse {
  DevBuf<> A, Y, Q, P, Ctl, Tasks[2], Woff[2], Stamps;
  DfWork w{};
  bool ready = false;

  bool on() const { return ready; }

  // for a blocked cov solver: nothing unless knobs.df and dfinv.hip takes this D
  void setup(int64_t D, int device, const SolverKnobs& knobs) {
    if (!knobs.df || !df_available(D)) return;
    const int64_t K2 = D / 256, BB = 256 * 256, DD = D * D;
    int ncu = 0;
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    // workgroups per CU (the kernel's registers admit 2; every one must be resident)
    ncu *= knobs.df_per_cu;
    A.alloc((size_t)K2 * DD);
    Y.alloc((size_t)K2 * (NM_PASSES + 1) * BB);
    Q.alloc((size_t)K2 * (NM_PASSES + 1) * BB);
    P.alloc((size_t)K2 * BB);
    const int64_t nctl = df_ctl_ints(D);
    Ctl.alloc((size_t)(nctl + 1) / 2);
    HIP_TRY(hipMemset(Ctl.p, 0, (size_t)nctl * sizeof(int)));
    for (int k = 0; k < 2; ++k) {
      const DfPlanHost pl = df_plan(D, k == 0 ? 2 : 3, ncu);
      Tasks[k].alloc((pl.tasks->size() + 1) / 2);
      Woff[k].alloc((pl.woff->size() + 1) / 2);
      HIP_TRY(hipMemcpy(Tasks[k].p, pl.tasks->data(), pl.tasks->size() * sizeof(int), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(Woff[k].p, pl.woff->data(), pl.woff->size() * sizeof(int), hipMemcpyHostToDevice));
      w.tasks[k] = reinterpret_cast<const int*>(Tasks[k].p);
      w.woff[k] = reinterpret_cast<const int*>(Woff[k].p);
    }
    for (int64_t g = 0; g < K2; ++g) w.A[g] = A.p + g * DD;
    w.Y = Y.p;
    w.Q = Q.p;
    w.P = P.p;
    w.ctl = reinterpret_cast<int*>(Ctl.p);
    w.nwg = ncu;
    if (knob_set("MIDAGMA_DF_STAMPS")) {  // diagnostics: per-task timestamps of the last launch
      Stamps.alloc((size_t)3 * std::max(df_plan(D, 3, ncu).tasks->size(), df_plan(D, 2, ncu).tasks->size()) / 12);
      HIP_TRY(hipMemset(Stamps.p, 0, Stamps.n * sizeof(double)));
      w.stamps = reinterpret_cast<unsigned long long*>(Stamps.p);
    }
    ready = true;
  }

  // build_at into the launch's A^0, then the whole fast inverse into Mt
  void enqueue(const double* W, int64_t D, int64_t d, double* Mt, double* IW, const Params* pr, State* st,
               const BInvWork& bw, int passes, hipStream_t stream) const {
    launch_build_at(W, D, /*square=*/true, w.A[0], D, d, 0.0, pr, st, stream, IW);
    launch_df_inverse(Mt, D, w, bw, passes <= 2 ? 2 : 3, st, stream);
  }

  // wait timeouts of the launches so far (a planning bug; the solver raises on it)
  int timeouts() const {
    if (!ready) return 0;
    int t = 0;
    HIP_TRY(hipMemcpy(&t, w.ctl + 2 * 32, sizeof(int), hipMemcpyDeviceToHost));
    return t;
  }
};

}  // namespace midagma
