// The trek regularizers of the solver handle (solver_impl.h): PstTrek (trek.hip) and TccTrek
// (tcc.hip) each own their device buffers and the launch view over them, built once where the
// buffers are allocated; Trek is what the slot sees: which of the two is on, the gradient buffer
// they share, and the one enqueue.  A set-up changes pointers the slot graphs captured: the
// caller invalidates its graphs after every set_pst / set_tcc.
#pragma once

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <vector>

#include "devmem.h"
#include "launch.h"
#include "solver_knobs.h"

namespace midagma {

// PST trek regularizer (trek.hip)
struct PstTrek {
  std::vector<DevBuf<>> bufs;  // every D x D work buffer of the regularizer
  DevBuf<> pairs, small, slices;
  DevBuf<State> gates;
  TrekWork w{};

  // G: the gradient buffer (Trek's), allocated here in its place among the others
  TrekCfg set(int64_t d, int64_t D, const GJWork& gj, int seq, int agg, int tmode, double weight, double eps_inv,
              int64_t K, const int64_t* pr64, int64_t mpairs, DevBuf<>& G, hipStream_t stream) {
    if (seq < 0 || seq > 3 || agg < 0 || agg > 3 || tmode < 1 || tmode > 2)
      throw std::invalid_argument("set_trek: bad seq / agg / mode");
    if (seq == TREK_LOG && K < 1) throw std::invalid_argument("set_trek: K_log must be >= 1");
    const size_t DD = (size_t)D * D;
    int nq = 2;
    if (seq == TREK_EXP) nq = TREK_TAYLOR_M + 1;
    if (seq == TREK_BINOM) nq = 64 - __builtin_clzll((unsigned long long)d) + 2;
    const int nbuf = 11 + nq + TREK_SMAX + 1 + 2;
    if ((int)bufs.size() < nbuf) bufs.resize(nbuf);
    for (int i = 0; i < nbuf; ++i) bufs[i].alloc(DD);
    int b = 0;
    TrekWork w{};  // (local: the stored view changes only after the last check below)
    w.gj = gj;
    for (double** slot : {&w.X, &w.F, &w.H, &w.S, &w.GT, &w.L, &w.tmp, &w.tmp2, &w.tmp3, &w.tmp4}) *slot = bufs[b++].p;
    ++b;  // spare
    for (int i = 0; i < nq; ++i) w.Q[i] = bufs[b++].p;
    for (int i = 0; i <= TREK_SMAX; ++i) w.E[i] = bufs[b++].p;
    w.dQ[0] = bufs[b++].p;
    w.dQ[1] = bufs[b++].p;
    if (D % 128 == 0 && (D / 128) * (D / 128) < 256) {
      slices.alloc(4 * DD);
      w.slices = slices.p;
    }
    small.alloc((size_t)(D / 64) * D + 4 * 256 + 16);
    w.colpart = small.p;
    w.part = small.p + (D / 64) * D;
    w.scal = w.part + 4 * 256;
    HIP_TRY(hipMemsetAsync(small.p, 0, small.n * sizeof(double), stream));
    gates.alloc(1 + 2 * TREK_SMAX);
    HIP_TRY(hipMemsetAsync(gates.p, 0, (1 + 2 * TREK_SMAX) * sizeof(State), stream));
    w.gates = gates.p;
    G.alloc(DD);
    HIP_TRY(hipMemsetAsync(G.p, 0, DD * sizeof(double), stream));
    std::vector<int32_t> pr(2 * mpairs);
    for (int64_t i = 0; i < 2 * mpairs; ++i) {
      if (pr64[i] < 0 || pr64[i] >= d) throw std::invalid_argument("set_trek: pair index out of range");
      pr[i] = (int32_t)pr64[i];
    }
    pairs.alloc((size_t)(mpairs + 1));  // 2 int32 per double slot
    HIP_TRY(hipMemcpy(pairs.p, pr.data(), pr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    TrekCfg c{};
    c.seq = seq;
    c.agg = agg;
    c.mode = tmode;
    c.weight = weight;
    c.eps_inv = eps_inv;
    c.K = seq == TREK_BINOM ? (int)d : (int)K;
    c.smax = TREK_SMAX;
    c.m = mpairs;
    c.pairs = reinterpret_cast<const int32_t*>(pairs.p);
    this->w = w;
    return c;
  }
};

// TCC trek regularizer (tcc.hip; notreks TCCRegularizer as trek_value_grad runs it): w multiplies S,
// eps as the reference
struct TccTrek {
  TccCfg cfg{};
  TccWork w{};
  DevBuf<> A, Mi, S, vec, part, P, R, C, Aalt, Pst, Pst1;
  DevBuf<> Y0, Y1, Q0, Q1, Pb, Part2, Done;  // the fast-block inverse's series buffers
  DevBuf<State> gates;

  void set(int64_t d, int64_t D, const SolverKnobs& knobs, int tmode, double weight, double wS, double eps,
           const int64_t* pairs, int64_t mpairs) {
    if (tmode < 1 || tmode > 2) throw std::invalid_argument("set_trek_tcc: bad mode");
    std::vector<double> Sh((size_t)D * D, 0.0);
    for (int64_t k = 0; k < mpairs; ++k) {
      const int64_t i = pairs[2 * k], j = pairs[2 * k + 1];
      if (i < 0 || i >= d || j < 0 || j >= d) throw std::invalid_argument("set_trek_tcc: pair index out of range");
      Sh[(size_t)i * D + j] = 1.0;  // S[rows, cols] = 1 (notreks _indicator_from_pairs)
    }
    const int64_t D2 = round_up64(2 * d);
    const int64_t nch = (2 * d + 63) / 64;
    A.alloc((size_t)D2 * D2);
    Mi.alloc((size_t)D2 * D2);
    S.alloc((size_t)D * D);
    vec.alloc((size_t)6 * D2 + 32);
    part.alloc((size_t)nch * D2);
    P.alloc(2 * 32 * 32);
    R.alloc((size_t)2 * 32 * D2);
    C.alloc((size_t)2 * D2 * 32);
    HIP_TRY(hipMemcpy(S.p, Sh.data(), Sh.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(vec.p, 0, vec.n * sizeof(double)));  // warm flag off, vectors 0
    gates.alloc(TCC_GATES);
    HIP_TRY(hipMemset(gates.p, 0, TCC_GATES * sizeof(State)));
    TccWork w{};  // (local: stored, with cfg, once every allocation has succeeded)
    w.gj = GJWork{P.p, R.p, C.p, nullptr, nullptr};
    w.D2 = D2;
    w.A = A.p;
    w.Mi = Mi.p;
    w.S = S.p;
    double* v = vec.p;
    for (double** slot : {&w.x, &w.y, &w.u, &w.z, &w.vprev, &w.uprev}) {
      *slot = v;
      v += D2;
    }
    w.scal = v;
    w.part = part.p;
    w.gates = gates.p;
    w.fix = knobs.tcc_fix != 0 ? 1 : 0;
    w.fix_pre = knobs.tcc_fix_pre;
    w.fix_hold = knobs.tcc_fix_hold;
    w.fix_easy = knobs.tcc_fix_easy;
    // D2 >= 2048 (knobs.tcc_binv): the shifted inverses on the two-level blocked inverse (pivoted path)
    if (D2 >= (knobs.tcc_binv == 2 ? 512 : 2048) && binv_block(D2) > 0 && knobs.tcc_binv != 0) {
      const int64_t b2 = binv_block(D2);
      Aalt.alloc((size_t)D2 * D2);
      Pst.alloc((size_t)D2 * b2);
      Pst1.alloc((size_t)D2 * b2);
      w.Aalt = Aalt.p;
      w.Pst = Pst.p;
      w.Pst1 = Pst1.p;
      // fast slots (knobs.tcc_fastblk): every outer block but the last on the product-form series
      // (tcc.hip tcc_inverse_fix); one warm-start slot (Pst1 = Pst)
      if (knobs.tcc_fastblk) {
        for (DevBuf<>* b : {&Y0, &Y1, &Q0, &Q1, &Pb}) b->alloc((size_t)b2 * b2);
        Part2.alloc((size_t)(D2 / b2) * (NM_PASSES + 1) * PART_STRIDE);
        Done.alloc((size_t)(D2 / b2));
        HIP_TRY(hipMemset(Pst.p, 0, (size_t)D2 * b2 * sizeof(double)));
        w.Pst1 = Pst.p;
        w.Y0 = Y0.p;
        w.Y1 = Y1.p;
        w.Q0 = Q0.p;
        w.Q1 = Q1.p;
        w.Pblk = Pb.p;
        w.part2 = Part2.p;
        w.done = reinterpret_cast<int*>(Done.p);
      }
    }
    this->w = w;
    cfg = TccCfg{tmode, weight, wS, eps, mpairs};
  }
};

struct Trek {
  bool on = false;
  bool use_tcc = false;  // TCC instead of PST; mode / weight live in cfg for both
  TrekCfg cfg{};
  DevBuf<> G;            // weight * d value / d W of the slot ('opt' mode)
  DevBuf<State> probe;   // RUNNING + checkpoint: gates the API-call (midagma_trek) path
  PstTrek pst;
  TccTrek tcc;

  // TrekRegularizer.enabled() false, or no pairs
  static bool disabled(int tmode, double weight, int64_t mpairs) { return tmode == 0 || mpairs <= 0 || weight == 0.0; }

  void set_pst(int64_t d, int64_t D, const GJWork& gj, int seq, int agg, int tmode, double weight, double eps_inv,
               int64_t K, const int64_t* pairs, int64_t mpairs, hipStream_t stream) {
    if (disabled(tmode, weight, mpairs)) {
      on = false;
      return;
    }
    cfg = pst.set(d, D, gj, seq, agg, tmode, weight, eps_inv, K, pairs, mpairs, G, stream);
    on = true;
    use_tcc = false;
    ensure_probe();
  }
  void set_tcc(int64_t d, int64_t D, const SolverKnobs& knobs, int tmode, double weight, double wS, double eps,
               const int64_t* pairs, int64_t mpairs) {
    if (disabled(tmode, weight, mpairs)) {
      on = false;
      return;
    }
    tcc.set(d, D, knobs, tmode, weight, wS, eps, pairs, mpairs);
    G.alloc((size_t)D * D);
    HIP_TRY(hipMemset(G.p, 0, (size_t)D * D * sizeof(double)));
    cfg = TrekCfg{};
    cfg.mode = tmode;
    cfg.weight = weight;
    cfg.m = mpairs;
    on = true;
    use_tcc = true;
    ensure_probe();
  }
  void ensure_probe() {
    if (!probe.p) {
      probe.alloc(1);
      State pr{};
      pr.status = ST_RUNNING;
      pr.ckpt_pending = 1;
      HIP_TRY(hipMemcpy(probe.p, &pr, sizeof(State), hipMemcpyHostToDevice));
    }
  }

  // the value (and the Adam-state words) the control kernel reads; null when off
  const double* scal() const { return on ? (use_tcc ? tcc.w.scal : pst.w.scal) : nullptr; }
  bool opt_mode() const { return on && cfg.mode == 2; }
  // TCC ('opt', 2d > 128): the chain form a fast cov slot may shorten
  bool tcc_chain(int64_t d) const { return on && use_tcc && cfg.mode == 2 && 2 * d > 128; }

  // the regularizer of W into G, gated by st; weight1: the bare gradient (midagma_trek).
  // handback / fast_steps: launch_trek_tcc's short chain (TCC only)
  void enqueue(const double* W, int64_t d, int64_t D, const State* st, hipStream_t stream, bool weight1 = false,
               State* handback = nullptr, int fast_steps = TCC_NODA_MAX) const {
    if (use_tcc) {
      TccCfg c = tcc.cfg;
      if (weight1) c.weight = 1.0;
      launch_trek_tcc(W, d, D, c, tcc.w, st, G.p, stream, handback, fast_steps);
    } else {
      TrekCfg c = cfg;
      if (weight1) c.weight = 1.0;
      launch_trek_pst(W, d, D, c, pst.w, st, G.p, stream);
    }
  }
};

}  // namespace midagma
