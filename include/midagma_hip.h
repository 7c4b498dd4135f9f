/*
 * midagma_hip.h -- C ABI of the MI355X-native DAGMA inner solver.
 *
 * The reference (fbleile/midagma) has no native code and no FFI: its hot path
 * is the Python method `DagmaLinear.minimize` (src/dagma/linear.py:165-333)
 * with helpers `_score` (70-94), `_h` (97-116), `_func` (118-135) and
 * `_adam_update` (138-163), reading object state set by `fit()`
 * (linear.py:406-429).  Each entry point below replaces one of those Python
 * call sites; the ctypes binding that makes them a drop-in lives in
 * `midagma_amd/_lib.py` and is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; host arrays are caller-owned, C-contiguous float64;
 *     device pointers (the *_dev entry points, midagma_bind_zbuf) are borrowed.
 *   - every function returns MIDAGMA_OK (0) or a negative error code; the
 *     message is available from midagma_last_error(solver) (or (NULL) for
 *     errors raised before a solver exists).  No C++ exception crosses the ABI.
 *   - a solver is not thread-safe; one host thread drives it.
 */
#ifndef MIDAGMA_HIP_H_
#define MIDAGMA_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIDAGMA_ABI_VERSION 11

/* return codes */
#define MIDAGMA_OK 0
#define MIDAGMA_E_HIP (-1)      /* HIP runtime failure            -> RuntimeError        */
#define MIDAGMA_E_SINGULAR (-2) /* non-finite inverse (scipy getrf info>0) -> LinAlgError */
#define MIDAGMA_E_ARG (-3)      /* bad argument / shape, non-finite input (scipy check_finite) -> ValueError */
#define MIDAGMA_E_STATE (-4)    /* call out of sequence            -> RuntimeError        */

/* loss_type (linear.py:52-53) and score mode */
#define MIDAGMA_LOSS_L2 0
#define MIDAGMA_LOSS_LOGISTIC 1
#define MIDAGMA_MODE_COV 0  /* cov = X^T X / n precomputed (linear.py:428); l2 only   */
#define MIDAGMA_MODE_DATA 1 /* X row shard resident; per-step X^T(...) + all-reduce */

/* minimize outcome (midagma_result.status) */
#define MIDAGMA_ST_RUNNING 0
#define MIDAGMA_ST_DONE 1         /* max_iter or tolerance      -> (W, True)  linear.py:333, 330 */
#define MIDAGMA_ST_FAILED 2       /* out of domain, iter 1 or s<=0.9 -> (W, False) linear.py:233   */
#define MIDAGMA_ST_LR_UNDERFLOW 3 /* lr <= 1e-16               -> (W, True)  linear.py:237-238   */
#define MIDAGMA_ST_SINGULAR 4

typedef struct midagma_solver midagma_solver;

typedef struct {
  int64_t iters;         /* Adam steps applied (pbar.update total, linear.py:332)   */
  int64_t halvings;      /* lr halvings in the domain line search (linear.py:236)   */
  int64_t slots;         /* device step slots consumed (diagnostics)                */
  int64_t n_checkpoints; /* objective evaluations (linear.py:279-280)               */
  int32_t status;        /* MIDAGMA_ST_*                                            */
  int32_t early_stop;    /* 1 if |dobj/obj| <= tol ended the call (linear.py:328)   */
  double lr_final;
  double obj_last, score_last, h_last, l1_last;
} midagma_result;

/* The numeric fields of the reference's `minimize.checkpoint` event (linear.py:290-326):
 * obj_total, score_datafit, reg_dag_value (h), lr, w_abs_sum (l1), W statistics after the
 * step, and the norms of the checkpoint step's gradients (linear.py:262-273). */
typedef struct {
  int64_t iter;
  double obj, score, h, lr, l1;
  double w_norm, max_abs_w, min_abs_w_nonzero;
  double grad_raw_norm, grad_step_norm, grad_score_norm, grad_dag_norm, grad_l1_norm, grad_inc_norm;
  double elapsed; /* seconds since the call's first device slot */
  double reg_trek_value, grad_trek_norm; /* PST trek regularizer (0 when none) */
} midagma_ckpt;

int midagma_abi_version(void);
int midagma_device_count(int* n);
const char* midagma_last_error(const midagma_solver* s);

/* Replaces DagmaLinear.__init__ + the data part of fit() (linear.py:25-67, 406-429).
 * d: number of nodes; device: HIP ordinal; stream: hipStream_t to run on, or NULL
 * for a solver-owned stream (required for the graph-replayed minimize loop). */
int midagma_create(midagma_solver** out, int loss, int mode, int64_t d, int device, void* stream);
void midagma_destroy(midagma_solver* s);
void* midagma_stream(midagma_solver* s);
int64_t midagma_padded_dim(const midagma_solver* s);

/* cov = X^T X / n (linear.py:428), host d x d with leading dimension ld. */
int midagma_set_cov(midagma_solver* s, const double* cov, int64_t ld);
/* mask_inc / mask_exc for the next minimize call (linear.py:217-222), host d x d or NULL. */
int midagma_set_masks(midagma_solver* s, const double* mask_inc, const double* mask_exc);
/* ABI 8: W's dtype in the reference's arithmetic (DagmaLinear(dtype=...), linear.py:29, 408, 429).
 * float32 != 0: the loop emulates numpy's float32 array operations on W and Id -- W rounded to
 * float32 after every in-place update (275, 235, 239), s*Id - W*W and Id - W in float32 (226, 244),
 * M = inv + 1e-16 and 2 W o M^T in float32 (226, 248) -- with the inverse itself in float64 (a
 * float32 getrf's bits cannot be reproduced).  Takes effect at the next minimize / begin. */
int midagma_set_w_float32(midagma_solver* s, int float32);
/* data mode: this rank's row shard of X (n_local x d, ld = d); n_global = rows over all ranks.
 * on_device != 0: X is a device pointer (copied). */
int midagma_set_data(midagma_solver* s, const double* X, int64_t n_local, int64_t n_global, int on_device);
/* data mode: zbuf <- X_k^T X_k (all-reduce it, then midagma_cov_from_zbuf(n): cov = zbuf / n). */
int midagma_data_gram(midagma_solver* s);
int midagma_cov_from_zbuf(midagma_solver* s, double n);
/* The solver's cov (d x d, ld) to the host: the `self.cov` attribute fit() keeps (linear.py:428)
 * when cov was built on the device from the ranks' shards. */
int midagma_get_cov(midagma_solver* s, double* out, int64_t ld);
/* ABI 7: fit()'s data preparation on the device (linear.py:406-428), for a device-resident or
 * row-sharded X in either score mode.  All on `stream` (a hipStream_t, NULL = default).
 * colsum_dev: out_dev[j] = sum_r X[r, j] (n x d, ldx; fixed summation order); returns after it
 *   is written.  Sharded: all-reduce it, then center with n_global.
 * center_dev: X[r, j] -= colsum_dev[j] / nrows in place (the l2 centring, linear.py:411); async.
 * gram: G_dev (d x d, ldg, device) = X^T X (linear.py:428) for X (n x d, ldx) in device memory
 *   (on_device != 0) or host memory, streamed in zero-padded row chunks through the 128 x 128
 *   FP64 MFMA GEMM, chunk sums in a fixed order; MIDAGMA_E_ARG if X holds inf/nan.  Returns
 *   after G is written.  Sharded: all-reduce G over ranks.
 * set_cov_dev: the solver's cov = G_dev / divisor (divisor = n, float(self.n) in linear.py:428),
 *   G_dev d x d (ldg) device memory complete before the call; MIDAGMA_E_ARG on inf/nan. */
int midagma_colsum_dev(const double* X, int64_t n, int64_t d, int64_t ldx, double* out_dev, void* stream);
int midagma_center_dev(double* X, int64_t n, int64_t d, int64_t ldx, const double* colsum_dev, double nrows,
                       void* stream);
int midagma_gram(const double* X, int64_t n, int64_t d, int64_t ldx, int on_device, double* G_dev, int64_t ldg,
                 void* stream);
int midagma_set_cov_dev(midagma_solver* s, const double* G_dev, int64_t ldg, double divisor);
/* ABI 7: the data-mode score all-reduce inside the library (linear.py:244-246 over row
 * shards).  comm_unique_id: RCCL's 128-byte ncclUniqueId (rank 0 makes it, the caller broadcasts
 * it, e.g. over torch.distributed).  comm_init: this solver joins an nranks communicator as `rank`;
 * from then on every captured slot sums the score partial over the ranks (in place, on the solver
 * stream, between the GEMMs and the update), so midagma_minimize / midagma_run_slots drive a
 * multi-rank minimize from replayed graphs, and every host poll all-reduces (status, iters): a
 * divergent replica makes every rank fail with MIDAGMA_E_STATE instead of hanging.  Needs a ring
 * all-reduce for bit-identical replicas (NCCL_ALGO=Ring).  RCCL is loaded at run time (the copy in
 * the process, else ROCm's): MIDAGMA_E_STATE when absent.  comm_ranks: 0 without a communicator. */
int midagma_comm_unique_id(void* out, int64_t cap); /* returns 128 (the id's size) */
int midagma_comm_init(midagma_solver* s, const void* id, int64_t id_len, int nranks, int rank);
int midagma_comm_ranks(const midagma_solver* s);
/* the score partial of midagma_score_partial (or data_gram) summed over the communicator, on the
 * solver stream: `_score` in data mode between score_partial and score_finish */
int midagma_comm_allreduce_zbuf(midagma_solver* s);
/* The d x d (+ tail) device buffer that carries the per-step score partial Z_k.
 * Bind an external buffer (e.g. a torch tensor that torch.distributed all-reduces). */
int64_t midagma_zbuf_len(const midagma_solver* s);
int midagma_bind_zbuf(midagma_solver* s, void* dev_ptr, int64_t len);

/* ABI 11: data mode on several devices from ONE process ("one host thread drives
 * all its devices ... the Python side stays single-process"), behind the reference's single-process
 * DagmaLinear.fit(X) (linear.py:335-351; the per-step score gradient 244-246 summed over row shards).
 * A group holds one data-mode solver per entry of devices[] (member k holds row shard k of X); the
 * score partial is summed over the members inside every captured slot, between the GEMMs and the
 * update:
 *   - devices all distinct: one RCCL communicator per member from ncclCommInitAll over devices[];
 *     each member's slot graphs carry its all-reduce and are replayed by a library thread of its
 *     own, with the (status, iters) agreement all-reduce at every poll (midagma_comm_init's
 *     protocol).  All members finish their setup (begin, graph capture) before any collective is
 *     issued; a member that fails before that point fails the call on every member.
 *   - flags & MIDAGMA_GROUP_EMULATE (every entry of devices[] the same device; tests on one GPU): no
 *     RCCL.  The members' slots are captured as ONE graph over their streams with a fixed-order
 *     device sum of the partials (member 0 + member 1 + ...) in place of the all-reduce, and the
 *     calling thread replays it (test strategy 4).
 * Members are ordinary data-mode solvers (midagma_group_member, owned by the group): set_cov,
 * set_masks, set_w_float32, set_trek*, h, score_partial / score_finish and checkpoints act on one
 * member; apply the loop's settings (cov, masks, dtype, trek) to every member. */
#define MIDAGMA_GROUP_EMULATE 1
typedef struct midagma_group midagma_group;
int midagma_group_create(midagma_group** out, int loss, int64_t d, const int* devices, int ndev, int flags);
void midagma_group_destroy(midagma_group* g);
const char* midagma_group_last_error(const midagma_group* g);
int midagma_group_size(const midagma_group* g);
int midagma_group_emulated(const midagma_group* g);
midagma_solver* midagma_group_member(midagma_group* g, int k);
/* host X (n x d row-major): member k gets rows [lo_k, hi_k) of the even split (the first n % ndev
 * members take one row more), with n_global = n.  MIDAGMA_E_ARG when n < ndev. */
int midagma_group_set_data(midagma_group* g, const double* X, int64_t n);
/* every member's score buffer (score_partial's or data_gram's partial) <- the sum over the members;
 * returns after it is written */
int midagma_group_allreduce_zbuf(midagma_group* g);
/* DagmaLinear.minimize over the group (arguments and result as midagma_minimize).  W: host d x d,
 * in/out, from member 0 after the members were checked to end with the same W bits, status,
 * iterations and halvings (else MIDAGMA_E_STATE: the replicas diverged). */
int midagma_group_minimize(midagma_group* g, double* W, double mu, int64_t max_iter, double s_dom, double lr,
                           double tol, double beta1, double beta2, double lambda1, int64_t checkpoint,
                           midagma_result* res);

/* Replaces DagmaLinear.minimize(W, mu, max_iter, s, lr, tol, beta_1, beta_2)
 * (linear.py:165-333) with trek_reg disabled.  W: host d x d, in/out. */
int midagma_minimize(midagma_solver* s, double* W, double mu, int64_t max_iter, double s_dom, double lr,
                     double tol, double beta1, double beta2, double lambda1, int64_t checkpoint,
                     midagma_result* res);

/* The same loop one step at a time, for an external all-reduce between the halves
 * (data mode on several ranks):  begin; { step_partial; allreduce(zbuf); step_finish }*; end. */
int midagma_begin(midagma_solver* s, const double* W, double mu, int64_t max_iter, double s_dom, double lr,
                  double tol, double beta1, double beta2, double lambda1, int64_t checkpoint);
int midagma_step_partial(midagma_solver* s);
/* enqueue n whole slots (part 1 + part 2); midagma_sync waits.  Without host polling,
 * except in cov mode with the blocked inverse (d > 64, D = 128 or a multiple of 128 from 256), where the host picks the fast or
 * the GJ path per batch (one sync per batch of <= 64 slots). */
int midagma_run_slots(midagma_solver* s, int64_t n);
int midagma_sync(midagma_solver* s);
/* Diagnostics: average device time (hipEvents on the solver stream, `reps` launches each)
 * of the slot's parts: [0] build (sI-WoW)^T, [1] GJ inverse, [2] score GEMM(s), [3] whole
 * slot (GJ path), [4] data-mode X(I-W) GEMM, [5] data-mode X^T Y GEMM, [6] cov-mode fast
 * blocked inverse, [7] whole fast slot ([6], [7]: 0 if not available, -1 if the fast path
 * handed back).  ms_out holds 8 doubles.  Advances the state by up to 3 reps + 1 slots. */
/* ([5] is the X^T Y GEMM with the combine of its split-K slices, in either form below.) */
int midagma_profile_parts(midagma_solver* s, int reps, double* ms_out);
/* The form of the data-mode X^T Y GEMM chosen by the last midagma_set_data: 1 the classical
 * split-K GEMM, 2 one level of Strassen (seven half-size products instead of eight; D % 256 == 0,
 * long row shards, and device memory for the five operand sums of X, 1.25 x the size of X: 10 GB
 * at d = 1000, n = 1e6; when memory is short the classical form is kept).  0: no data set.  The two
 * forms agree to rounding, not bit for bit; each is deterministic and identical across ranks with
 * equal shards.  Purely additive: MIDAGMA_ABI_VERSION stays 11. */
int midagma_xty_form(const midagma_solver* s);
int midagma_step_finish(midagma_solver* s);
int midagma_poll(midagma_solver* s, midagma_result* res); /* synchronizes */
int midagma_end(midagma_solver* s, double* W, midagma_result* res);
int64_t midagma_checkpoints(midagma_solver* s, midagma_ckpt* out, int64_t cap);

/* The PST trek regularizer of notreks.py (pst / trek_value_grad) inside the loop
 * (linear.py:251-258, 131-133).  seq: 0 exp, 1 inv, 2 log, 3 binom; agg: 0 mean, 1 sum,
 * 2 max, 3 lse; mode: 0 off, 1 'log' (value at checkpoints only), 2 'opt' (value and
 * weight * gradient every step, weight * value in the checkpoint objective); K: log series
 * terms (binom: ignored, the exponent is d as in the reference); pairs: m (i, j) int64. */
int midagma_set_trek(midagma_solver* s, int seq, int agg, int mode, double weight, double eps_inv, int64_t K,
                     const int64_t* pairs, int64_t m);
/* The TCC trek regularizer (notreks.py:291-395 as trek_value_grad:667-706 calls it in the loop:
 * spectral penalty, 'approx_trek_graph', Perron pairs) inside the loop; mode as above; w: the
 * multiplier of the pair indicator S; eps: the reference's stabiliser (1e-12). */
int midagma_set_trek_tcc(midagma_solver* s, int mode, double weight, double w, double eps, const int64_t* pairs,
                         int64_t m);
/* trek_value_grad(W, tr) (notreks.py): value and, in 'opt' mode, the gradient (G nullable, d x d;
 * zeros in 'log' mode, as the reference returns). */
int midagma_trek(midagma_solver* s, const double* W, double* value, double* G);

/* Replaces DagmaLinear._h (linear.py:97-116): h and G_h = 2 W o inv(sI - W o W)^T (G nullable). */
int midagma_h(midagma_solver* s, const double* W, double s_dom, double* h, double* G);
/* Replaces DagmaLinear._score (linear.py:70-94) in cov mode (l2). */
int midagma_score(midagma_solver* s, const double* W, double* loss, double* G);
/* _score in data mode: partial into zbuf (all-reduce it), then finish. */
int midagma_score_partial(midagma_solver* s, const double* W);
int midagma_score_finish(midagma_solver* s, double* loss, double* G);

/* DagmaMLP.h_func kernel (nonlinear.py:68-86) on device memory:
 * Mt = (sI - A)^{-T} (ldm) and logdet_dev[0] = log|det(sI - A)| for A (d x d, lda).
 * Enqueued on `stream`, no host synchronization. */
int midagma_logdet_inv_dev(const double* A, int64_t d, int64_t lda, double s_dom, double* logdet_dev,
                           double* Mt_dev, int64_t ldm, void* stream);

/* Linear-SEM samples on the GPU (replaces utils.simulate_linear_sem, utils.py:99-172):
 * rows [row0, row0 + n_rows) of X (row-major, ld = ldx >= d, device memory) for the weighted
 * DAG W (host, d x d row-major, W[p, j] = weight of edge p -> j):
 *   x_j = sum_{p in pa(j)} W[p, j] x_p + z_j   (sem_type 0 gauss, 1 exp, 2 gumbel, 3 uniform)
 *   x_j ~ Bernoulli(sigmoid(.)) (4 logistic),  x_j ~ Poisson(exp(.)) (5 poisson).
 * Noise: Philox4x32-10 keyed by `seed`, counter (row / 2, node, draw) -- row r's values are the
 * same whatever row0 / n_rows split generated it.  noise_scale: d scales or NULL (ones).
 * MIDAGMA_E_ARG if W has a cycle.  Enqueued on `stream`; returns after the rows are written. */
int midagma_sem_linear(const double* W, int64_t d, int64_t row0, int64_t n_rows, int sem_type,
                       const double* noise_scale, uint64_t seed, double* X_dev, int64_t ldx, void* stream);

/* One torch.optim.Adam step (single-tensor algorithm, L2 weight decay wd) on n doubles of
 * device memory, enqueued on `stream`; coefficients host-rounded as torch computes them:
 * step_size = lr / (1 - b1^t), w1 = 1 - b1, c2 = 1 - b2, bc2_sqrt = sqrt(1 - b2^t).
 * Skipped when gate != NULL and *gate < 0 (device scalar: DagmaNonlinear's h, nonlinear.py:216). */
int midagma_adam_step(double* p, const double* g, double* m, double* v, int64_t n, double step_size, double w1,
                      double beta2, double c2, double bc2_sqrt, double eps, double wd, const double* gate,
                      void* stream);

/* The same step with the per-step coefficients from a device table at a device step counter:
 * step_size = table[2 t], sqrt(1 - b2^t) = table[2 t + 1], t = *counter (graph-replayable);
 * midagma_counter_advance adds 1 to *counter on `stream`. */
int midagma_adam_step_table(double* p, const double* g, double* m, double* v, int64_t n, const double* table,
                            const int64_t* counter, double w1, double beta2, double c2, double eps, double wd,
                            const double* gate, void* stream);
int midagma_counter_advance(int64_t* counter, void* stream);
/* midagma_adam_step_table over k <= 8 tensors (host arrays of their device pointers and
 * sizes) in one launch. */
int midagma_adam_step_table_multi(int64_t k, double* const* p, const double* const* g, double* const* m,
                                  double* const* v, const int64_t* n, const double* table, const int64_t* counter,
                                  double w1, double beta2, double c2, double eps, double wd, const double* gate,
                                  void* stream);

/* The DagmaMLP tail of dims [d, m1, 1] (d * m1 <= 7936), fused on torch's device memory and
 * stream (replaces sigmoid -> LocallyConnected(d, m1, 1) -> squared residual sum in
 * nonlinear.py:99-104, 139-159 and their autograd backward; dagma/locally_connected.py:55-85).
 * scratch: midagma_mlp_tail_scratch(n, d, m1) doubles of device memory.
 * fwd: Z (n x d*m1 row-major, plus b1 per column when b1 is given) -> R = Xhat - X (n x d),
 * *ssq = sum R^2 (device).
 * bwd: *g = d loss / d ssq (device) -> dZ (n x d*m1), dw2 (d x m1), db2 (d) and, when db1 is
 * given, db1 = column sums of dZ (d*m1). */
int64_t midagma_mlp_tail_scratch(int64_t n, int64_t d, int64_t m1);
int midagma_mlp_tail_fwd(const double* Z, const double* b1, const double* w2, const double* b2, const double* X,
                         int64_t n, int64_t d, int64_t m1, double* R, double* scratch, double* ssq, void* stream);
/* The rest of the [d, m1, 1] DagmaMLP objective (nonlinear.py:68-86, 139-159, 198-206):
 * fc1_terms: A[i, j] = sum_m W1[j m1 + m, i]^2 (d x d, the log-det operand) and the |W1| partial
 * sums l1part (midagma_fc1_terms_parts(d) doubles); its backward dW1 = 2 W1 gA^T + gl1 sign(W1).
 * mlp_objective: *obj = mu (half_d log(inv_n *ssq) + lambda1 sum(l1part)) + *h, and its
 * backward from *g: *gssq, gl1part[*], *gh (ssq and gssq both NULL: only gl1part and gh).
 * All device pointers, on `stream`. */
int64_t midagma_fc1_terms_parts(int64_t d);
int midagma_fc1_terms(const double* W1, int64_t d, int64_t m1, double* A, double* l1part, void* stream);
int midagma_fc1_terms_bwd(const double* W1, int64_t d, int64_t m1, const double* gA, const double* gscale,
                          const double* gl1part, const double* lin, int64_t nlin, double* dW1, void* stream);
/* h = -log|det(sI - A)| + d log s (DagmaMLP.h_func, nonlinear.py:68-86) into *h_dev and, when
 * Mt_dev is given, (sI - A)^-T (d x d, ldm) -- its gradient -- in four launches (build, GJ,
 * epilogue; the GJ on the 32-padded problem). */
int midagma_logdet_h_dev(const double* A, int64_t d, int64_t lda, double s, double* h_dev, double* Mt_dev, int64_t ldm,
                         void* stream);
/* The same, enqueued in midagma_logdet_h_parts(d) parts that must be issued in order (part 0:
 * build and prologue; parts 1 .. ceil(d/32): the Gauss-Jordan block steps; the last: h and
 * (sI - A)^-T), so a caller can interleave them with other work of its step (DagmaNonlinear's
 * side-stream log-det).  The parts of one h share a per-device workspace: one h at a time. */
int64_t midagma_logdet_h_parts(int64_t d);
int midagma_logdet_h_dev_part(const double* A, int64_t d, int64_t lda, double s, double* h_dev, double* Mt_dev,
                              int64_t ldm, void* stream, int64_t part);
/* ABI 6: the h log-det of consecutive DagmaNonlinear.minimize steps (nonlinear.py:206-217, 85-86)
 * with a warm start.  A handle holds the warm-start ring of one minimize call's A = sum fc1^2
 * (d <= 256; larger d always runs the Gauss-Jordan chain).  A fast step (exact = 0) inverts
 * (sI - A)^T by the product-form series from the last two steps' inverses and keeps the last
 * exact h when that inverse converged and is entrywise >= 0 (then sI - A is a nonsingular
 * M-matrix and h >= 0: the reference's h < 0 exit cannot fire); otherwise it runs the
 * Gauss-Jordan chain on the device and takes its h.  An exact step (exact = 1: the steps whose
 * objective the caller reads) always runs the chain.  Both write (sI - A)^-T to Mt and feed the
 * ring.  midagma_ldfast_reset starts a call (the first step then runs the chain).  Parts as
 * midagma_logdet_h_dev_part: issued in order on one stream; one step at a time per handle. */
typedef struct midagma_ldfast midagma_ldfast;
int midagma_ldfast_create(midagma_ldfast** out, int64_t d);
void midagma_ldfast_destroy(midagma_ldfast* h);
int midagma_ldfast_reset(midagma_ldfast* h);
int64_t midagma_ldfast_parts(const midagma_ldfast* h, int exact);
/* ABI 7: d (A is d x d) must equal the handle's d, else MIDAGMA_E_ARG. */
int midagma_ldfast_enqueue(midagma_ldfast* h, const double* A, int64_t d, int64_t lda, double s, double* h_dev,
                           double* Mt_dev, int64_t ldm, void* stream, int exact, int64_t part);
/* ABI 10: fast steps enqueued from now on also add 1 to *counter (device; null: off) at their
 * end, midagma_counter_advance's work in the end's launch, for a caller that skips the scalar
 * objective on those steps.  Exact steps never touch it. */
int midagma_ldfast_set_counter(midagma_ldfast* h, int64_t* counter);
/* gate-open (Gauss-Jordan) steps and fast steps since the last reset (diagnostics; syncs) */
int midagma_ldfast_stats(midagma_ldfast* h, int64_t* steps, int64_t* exact_steps);
/* ABI 6: the [d, m1, 1] objective with the scalar objective's backward folded into its consumers
 * (no mlp_sum / mlp_objective_bwd launches; bit-identical to the ABI-5 sequence): the tail forward
 * leaves its n row partials (part), the objective sums them and, with a counter, advances the
 * Adam table's step (counter += 1, nullable), the tail backward and the fc1 terms' backward take
 * gobj = d loss / d obj and derive d obj / d ssq, d h = gobj, d l1part = (gobj mu) lambda1. */
int midagma_mlp_tail_fwd_part(const double* Z, const double* b1, const double* w2, const double* b2, const double* X,
                              int64_t n, int64_t d, int64_t m1, double* R, double* part, void* stream);
int midagma_mlp_objective_part(const double* part, int64_t npart, const double* l1part, int64_t np, const double* h,
                               double mu, double lambda1, double half_d, double inv_n, double* obj, int64_t* counter,
                               void* stream);
int midagma_mlp_tail_bwd_obj(const double* Z, const double* b1, const double* w2, const double* R, const double* part,
                             const double* gobj, double mu, double half_d, double inv_n, int64_t n, int64_t d,
                             int64_t m1, double* dZ, double* dw2, double* db2, double* db1, double* scratch,
                             void* stream);
int midagma_fc1_terms_bwd_obj(const double* W1, int64_t d, int64_t m1, const double* gA, const double* gobj, double mu,
                              double lambda1, const double* lin, int64_t nlin, double* dW1, void* stream);
/* ABI 9: one replayed DagmaNonlinear step of a [d, m1, 1] model closed in one launch
 * (nonlinear.py:198-236): the tail's dw2 / db2 / db1 sums from the chunk partials that
 * midagma_mlp_tail_bwd_obj leaves in scratch when dw2 = db2 = db1 = NULL, fc1's weight gradient
 * (midagma_fc1_terms_bwd_obj's arithmetic), the gated table Adam step of the four parameters
 * (params / exp_avg / exp_avg_sq: fc1.weight, fc1.bias, fc2.weight, fc2.bias;
 * midagma_adam_step_table_multi's arithmetic) and the next step's fc1 terms (A, l1part as
 * midagma_fc1_terms computes them, from the updated weights).  Bit-identical to those launches. */
int midagma_mlp_step(double* const* params, double* const* exp_avg, double* const* exp_avg_sq, int64_t n, int64_t d,
                     int64_t m1, const double* gA, const double* gobj, double mu, double lambda1, const double* lin,
                     int64_t nlin, const double* scratch, const double* table, const int64_t* counter, double w1,
                     double beta2, double c2, double eps, double wd, const double* gate, double* A, double* l1part,
                     void* stream);
int midagma_mlp_objective(const double* ssq, const double* l1part, int64_t np, const double* h, double mu,
                          double lambda1, double half_d, double inv_n, double* obj, void* stream);
int midagma_mlp_objective_bwd(const double* g, const double* ssq, int64_t np, double mu, double lambda1, double half_d,
                              double inv_n, double* gssq, double* gl1part, double* gh, void* stream);
int midagma_mlp_tail_bwd(const double* Z, const double* b1, const double* w2, const double* R, const double* g,
                         int64_t n, int64_t d, int64_t m1, double* dZ, double* dw2, double* db2, double* db1,
                         double* scratch, void* stream);

/* Pairwise permutation independence tests (notreks/mi_tests.py: hsic_stat / dcor_stat under
 * permutation_pvalue, as test_pairwise_independence runs them over a pair list), the step that
 * builds the trek regularizers' pair set I.  Purely additive: MIDAGMA_ABI_VERSION stays 11.
 * A handle owns two streams and the device copy of X; one host thread drives it at a time.  Every
 * entry checks its arguments before it touches a device (MIDAGMA_E_ARG); the message comes from
 * midagma_indep_last_error(handle) (or (NULL) for errors raised without a handle).
 * set_data: host X (n x d row-major), 2 <= n <= 16384, d <= 65535, copied; MIDAGMA_E_ARG on inf/nan.
 * set_data_dev: the same from device memory: X_dev is n x d row-major on the handle's device with
 *   row stride ld >= d (checked: memory of that device), and is never written.  Its producer's work
 *   is ordered on hip_stream (NULL: the null stream).  Ordering: the transpose kernel (which also
 *   leaves two flags per column: holds a non-finite value, every value equals row 0's) runs on
 *   hip_stream, behind the producer, and the entry then synchronises hip_stream to read the 2 d
 *   flag bytes, so the handle's copy is complete before any later entry uses it; the caller
 *   synchronises nothing.  MIDAGMA_E_ARG on inf/nan, and the handle then holds no data (every
 *   later entry answers "set the data first" until a set_data* succeeds).
 * set_bandwidths: the RBF kernel's sigma^2 per variable (d values, finite and > 0), for hsic.
 * median_bandwidths: sigma^2 by the reference's median heuristic (mi_tests.py:39-44: the median of
 *   the off-diagonal squared differences of the column, 1.0 when that is not > 0), computed on the
 *   device for the ncols listed columns (cols NULL: all d; duplicates allowed) and 1.0 for the
 *   others, installed as set_bandwidths would and written to sigma2_out (d doubles, nullable).  The
 *   value is numpy's np.median of the squared differences bit for bit and does not depend on which
 *   columns are listed together.  Data from either set_data entry.
 * bandwidth_profile (diagnostics): the last median_bandwidths' kernel time in ms (device events;
 *   0 when no column was listed).  ms_out holds 1 double.
 * run: for each of the m pairs (i, j) (int64 m x 2; i == j and both orders allowed) the observed
 *   statistic stat[q] of (X[:, i], X[:, j]) and ge[q] = #{p < P : stat(X[:, i], X[:, j][perm_qp]) >=
 *   stat[q]}; null_out (nullable, m x P): every permuted statistic.  kind: 0 hsic, 1 dcor (dcor
 *   counts by dcov^2 and returns sqrt(max(dcov^2, 0)) / sqrt(sqrt(dvar_x^2 dvar_y^2)), 0 when a
 *   variance is <= 0).  A pair with a zero-range column gives stat 0, every permuted value 0 and
 *   ge = P, as the reference's all-zero centred matrix does.  perms: m x P x n int32 host array,
 *   each entry in [0, n) (checked), or NULL for device permutations: the stable argsort over a of
 *   the 64-bit key (((o.x << 32) | o.y) & ~0x3fff) | a, o = Philox4x32-10(counter (q, p, a, 0), key
 *   (seed low word, seed high word)), q the pair's index in this call; perms_out (nullable, m x P x n): those
 *   permutations.  Pairs are processed in batches of midagma_indep_batch_pairs(h, P, budget_bytes)
 *   (budget_bytes <= 0: 128 MiB over the two in-flight batches; at least 1 pair), the upload of a
 *   batch overlapping the kernels of the one before; results do not depend on the batch size.
 *   0 <= P <= 65535.
 * profile (diagnostics): the last run's stage times in ms, summed over its batches (stages of
 *   different batches overlap, so the sum can exceed the call's wall time): [0] host checking and
 *   staging of the explicit permutations, [1] uploads, [2] the permutation kernel, [3] the
 *   statistic kernels.  ms_out holds 4 doubles. */
#define MIDAGMA_INDEP_HSIC 0
#define MIDAGMA_INDEP_DCOR 1
typedef struct midagma_indep midagma_indep;
int midagma_indep_create(midagma_indep** out, int device);
void midagma_indep_destroy(midagma_indep* h);
const char* midagma_indep_last_error(const midagma_indep* h);
int midagma_indep_set_data(midagma_indep* h, const double* X, int64_t n, int64_t d);
int midagma_indep_set_data_dev(midagma_indep* h, const double* X_dev, int64_t n, int64_t d, int64_t ld,
                               void* hip_stream);
int midagma_indep_set_bandwidths(midagma_indep* h, const double* sigma2, int64_t d);
int midagma_indep_median_bandwidths(midagma_indep* h, const int64_t* cols, int64_t ncols, double* sigma2_out);
int midagma_indep_bandwidth_profile(const midagma_indep* h, double* ms_out);
int64_t midagma_indep_batch_pairs(const midagma_indep* h, int64_t P, int64_t budget_bytes);
int midagma_indep_profile(const midagma_indep* h, double* ms_out);
int midagma_indep_run(midagma_indep* h, int kind, const int64_t* pairs, int64_t m, int64_t P, const int32_t* perms,
                      uint64_t seed, int64_t budget_bytes, double* stat, int64_t* ge, double* null_out,
                      int32_t* perms_out);

/* A batch of B independent small-d problems (1 <= d <= 64, l2, cov mode, float64 W; the PST trek
 * regularizer at d <= 32 through midagma_btrek_set below, no TCC) that share d, the device and the loop settings and each have their own covariance,
 * lambda1, mu, s and lr: one launch of the small-d persistent loop runs them with one workgroup per
 * problem, so bootstrap resamples, a lambda1 grid or a table over seeds fill the device instead of
 * one compute unit.  Purely additive: MIDAGMA_ABI_VERSION stays 11.
 * Problem b's W, result and checkpoint records are bit-identical to what a cov-mode l2
 * midagma_solver gives for that problem alone with the same arguments (without a regularizer).
 * Every entry checks its arguments before it touches a device (MIDAGMA_E_ARG); the message comes
 * from midagma_batch_last_error(handle) (or (NULL) for errors raised without a handle).  A handle
 * owns one stream and its device and pinned buffers; one host thread drives it at a time.
 * create: 1 <= d <= 64, 1 <= B <= 16384.
 * set_cov: host B x d x d row-major, copied; MIDAGMA_E_ARG on inf/nan.
 * set_masks: host B x d x d each, or NULL to switch that mask off (as midagma_set_masks).
 * minimize: W is B x d x d host, in/out; mu, s_dom, lr, lambda1 hold B values each; res holds B
 *   results.  active (B bytes, NULL: all): a problem whose byte is 0 does not run, and its W and
 *   res entry are left untouched.  The host relaunches only the problems still running, so a
 *   finished problem costs nothing afterwards.  A problem that ends MIDAGMA_ST_SINGULAR (or any
 *   other status) reports it in res[b].status and the call returns MIDAGMA_OK.  MIDAGMA_E_ARG:
 *   max_iter < 1, checkpoint < 1, a null pointer, a non-finite active W, a call before set_cov.
 * checkpoints: the records of problem b from the last minimize call (0 when b was inactive in
 *   it), at most cap; returns their number. */
typedef struct midagma_batch midagma_batch;
int midagma_batch_create(midagma_batch** out, int64_t d, int64_t B, int device);
void midagma_batch_destroy(midagma_batch* h);
const char* midagma_batch_last_error(const midagma_batch* h);
int midagma_batch_set_cov(midagma_batch* h, const double* cov);
int midagma_batch_set_masks(midagma_batch* h, const double* mask_inc, const double* mask_exc);
int midagma_batch_minimize(midagma_batch* h, double* W, const double* mu, const double* s_dom, const double* lr,
                           const double* lambda1, int64_t max_iter, double tol, double beta1, double beta2,
                           int64_t checkpoint, const uint8_t* active, midagma_result* res);
int64_t midagma_batch_checkpoints(midagma_batch* h, int64_t b, midagma_ckpt* out, int64_t cap);

/* The PST trek regularizer in a batch (additive, ABI 11; d <= 32): its value and gradient are
 * computed inside each problem's workgroup (csrc/pst_blk.h), so a problem's result does not depend
 * on the rest of the batch; it agrees with midagma_set_trek's launch chain on a midagma_solver to
 * rounding, not bit for bit.  Errors as the batch entries' (midagma_batch_last_error).
 * set: seq 0 exp | 1 inv, agg and mode as midagma_set_trek; weight holds B values (one per
 *   problem), pairs m (i, j) int64 shared by the problems (repeats count, (i, j) and (j, i)
 *   differ, (i, i) is allowed).  mode 0 or m = 0 switches the regularizer off again.
 *   MIDAGMA_E_ARG: d > 32, seq log or binom, a pair index outside [0, d), a non-finite weight.
 * value: trek_value_grad of B given matrices (W is B x d x d host), no Adam step: value holds B
 *   values, grad (nullable) B x d x d; zeros without a regularizer. */
int midagma_btrek_set(midagma_batch* h, int seq, int agg, int mode, const double* weight, double eps_inv,
                      const int64_t* pairs, int64_t m);
int midagma_btrek_value(midagma_batch* h, const double* W, double* value, double* grad);

/* The logistic loss in a batch (additive, ABI 11; d <= 64, float64 W): the reference's
 * DagmaLinear("logistic") loop for B problems at once.  The loss has no covariance to fold n into,
 * so each problem's workgroup streams its X through the score phase of every slot in row blocks
 * (X^T expit(X W) on the FP64 matrix cores, csrc/small.hip), with fixed-order sums: a problem's W,
 * result and checkpoint records do not depend on B, on the other problems, on whether X is shared,
 * or on how the slots are split over launches, bit for bit.  They agree with a data-mode logistic
 * midagma_solver, which runs the large-tile launch chain, to rounding.  Errors as the batch entries'.
 * Not run here (MIDAGMA_E_ARG): a trek regularizer set with midagma_btrek_set, a float32 W, a
 * different n per problem.
 * set_data: host X, n x d row-major (shared = 1: one X for all B problems, stored once on the
 *   device) or B x n x d (shared = 0), copied and zero-padded to the device layout.  MIDAGMA_E_ARG:
 *   a null pointer, n < 1, n >= 2^31, inf/nan in X, or padded slabs that exceed the device's free
 *   memory (checked before allocating).
 * minimize: midagma_batch_minimize's arguments and semantics (per-problem mu, s, lr, lambda1;
 *   active; results; checkpoints through midagma_batch_checkpoints, whose score is the logistic
 *   loss / n).  Needs midagma_batch_set_cov with the uncentred X^T X / n of each problem (the
 *   reference's cov, linear.py:428) and set_data first, else MIDAGMA_E_ARG.  Masks apply as for l2.
 * score: the reference's _score for all B problems at given W (B x d x d host), no Adam step:
 *   loss holds B values, sum(logaddexp(0, X W) - X o (X W)) / n; G (nullable, B x d x d) is
 *   X^T expit(X W) / n - cov and needs set_cov. */
int midagma_blogit_set_data(midagma_batch* h, const double* X, int64_t n, int shared);
int midagma_blogit_minimize(midagma_batch* h, double* W, const double* mu, const double* s_dom, const double* lr,
                            const double* lambda1, int64_t max_iter, double tol, double beta1, double beta2,
                            int64_t checkpoint, const uint8_t* active, midagma_result* res);
int midagma_blogit_score(midagma_batch* h, const double* W, double* loss, double* G);

/* Bootstrap covariances for a batch, formed on the device from one X (additive, ABI 11).
 * Replicate b of `seed` draws n row indices with replacement:
 *   o = Philox4x32-10(counter (j, b, 0, 0), key (seed & 0xffffffff, seed >> 32)),
 *   r = (o0 << 32) | o1,  idx[j] = (r * n) >> 64  (the high 64 bits of the 128-bit product),
 * and its covariance is that of the resample, Xb = X[idx]; Xb -= Xb.mean(0); Xb^T Xb / n, computed
 * as (S - t t^T / n) / n over the rows of X weighted by how often each is drawn, X centred once by
 * its global column mean.  The result for replicate b depends on (X, seed, b) alone and is exactly
 * symmetric.
 * boot_cov: cov of replicates first .. first+B-1 of (seed) from X (n x d, leading dimension ldx,
 *   host or device memory per on_device) into the batch's B problems; afterwards the batch is as
 *   after midagma_batch_set_cov.  X is not written.  Replicates are processed in chunks whose
 *   scratch (n int32 counts and the Gram partials per replicate) stays within budget_bytes
 *   (<= 0: 1 GiB; at least one replicate per chunk); results do not depend on the chunking.  A
 *   device X must be complete before the call (the batch runs on its own stream).
 *   MIDAGMA_E_ARG before any device work: a null handle or X, n < 1, n >= 2^31, ldx < d,
 *   first < 0 or first + B > 2^32; MIDAGMA_E_ARG with set_cov's message: X holds inf/nan (the
 *   batch's cov is then left as it was).
 * boot_get_cov: the batch's current covariances, B x d x d, to the host (diagnostics and tests).
 * boot_profile: device-event times in ms of the last boot_cov, summed over its chunks: [0] copy
 *   and centring of X, [1] counts, [2] weighted Gram, [3] finish. */
int midagma_boot_cov(midagma_batch* h, const void* X, int64_t n, int64_t ldx, int on_device, uint64_t seed,
                     int64_t first, int64_t budget_bytes);
int midagma_boot_get_cov(midagma_batch* h, double* out);
int midagma_boot_profile(const midagma_batch* h, double* ms_out);

/* Pearson and Spearman on the device (notreks/mi_tests.py: pearson_stat_pvalue / spearman_stat_pvalue
 * over all pairs at once; the analytic p-values stay host work), csrc/corr.hip.  Purely additive:
 * MIDAGMA_ABI_VERSION stays 11.  X_dev is n x d row-major device memory of the current device with
 * row stride ldx and is never written; the work is enqueued on `stream` (a hipStream_t, NULL: the
 * null stream) behind X's producer, and each entry returns after its result is written.  Every
 * entry checks its arguments before it touches a device: MIDAGMA_E_ARG for a null pointer,
 * n outside [2, 2^31), d outside [1, 65535], ldx < d or an output leading dimension < d (message:
 * midagma_last_error(NULL)).  MIDAGMA_E_ARG too when X holds inf or nan (found on the device; the
 * output is then unspecified).
 * colrank: R[r, c] (ldr) = the 1-based average rank of X[r, c] within column c
 *   (scipy.stats.rankdata(method="average"); -0.0 ties with +0.0), an exact half-integer.  A
 *   stable LSD radix sort of (64-bit key, row) per column, the columns in chunks whose scratch
 *   stays within budget_bytes (<= 0: 2 GiB; at least one column); the ranks do not depend on it.
 * corr: Rho (d x d, ldrho) = the Pearson correlation matrix of X's columns: G_ij / sqrt(G_ii G_jj)
 *   clamped to [-1, 1] for the Gram G of the columns minus their means (midagma_gram's FP64 MFMA
 *   GEMM over a centred staging copy in row chunks within budget_bytes, <= 0: 2 GiB, chunk sums in a
 *   fixed order), 1 on the diagonal.  const_col[c] = 1 when column c's max equals its min (scipy's
 *   constant-input rule, on the raw values), else 0; such a column's row and column of Rho are NaN.
 *   Spearman's rho is corr of colrank's R.
 * corr_workspace: the bytes of device scratch the larger of the two entries allocates for these
 *   arguments; 0 for n or d out of range. */
int midagma_colrank(const double* X_dev, int64_t n, int64_t d, int64_t ldx, double* R_dev, int64_t ldr,
                    int64_t budget_bytes, void* stream);
int midagma_corr(const double* X_dev, int64_t n, int64_t d, int64_t ldx, double* Rho_dev, int64_t ldrho,
                 int32_t* const_col_dev, int64_t budget_bytes, void* stream);
int64_t midagma_corr_workspace(int64_t n, int64_t d, int64_t budget_bytes);

/* colargsort (additive, ABI 11; csrc/corr.hip): order[c n + i] (int32, column-major d x n) = the
 * row at position i of the stable argsort of column c of X (-0.0 equal to +0.0): the row payload
 * colrank's radix sort carries, with its passes, key map, chunking (budget_bytes as colrank) and
 * determinism.  Arguments, errors and the stream rule as colrank's. */
int midagma_colargsort(const double* X_dev, int64_t n, int64_t d, int64_t ldx, int32_t* order_dev,
                       int64_t budget_bytes, void* stream);

/* dCor permutation tests of pairs of columns without an n x n sum (additive, ABI 11; csrc/dcor.hip):
 * the dCor statistic of midagma_indep_run and its bias-corrected form, exact in O(n m) work an
 * evaluation for a block edge m near sqrt(n) (a sort, block sums and K x K cell tables, K =
 * ceil(n / m)), for 2 <= n < 2^31.  Not the midagma_indep_ prefix: that handle keeps the transposed X
 * of an O(n^2) kernel, caps n at 16384 and packs a < 2^14 into its permutation keys; this one
 * keeps per-column sorts and row sums, has another permutation rule and no HSIC, and none of the
 * indep entries applies to it.  Errors: midagma_dcor_last_error(handle) (or (NULL)).  One host
 * thread drives a handle at a time.
 * create: no device call; the device is opened by the first set_data*.
 * set_data: host X (n x d row-major), copied.  set_data_dev: device X of the handle's device, row
 *   stride ld, never written, read on hip_stream behind its producer; the entry synchronises
 *   hip_stream before it returns (midagma_indep_set_data_dev's ordering rule), so the caller
 *   synchronises nothing.  Both run the per-column pre-pass (stable argsort through colargsort
 *   within budget_bytes, centred values, row sums, a.., dvar^2 in both forms, the zero-range mark
 *   max == min on the raw values).  MIDAGMA_E_ARG before any device call: a null pointer, n outside
 *   [2, 2^31), d outside [1, 65535], ld < d; MIDAGMA_E_ARG too for inf / nan in X (found on the
 *   device); the handle then holds no data.
 * run: for each of the m pairs (int64 m x 2) stat[q], ge[q] = #{p < P : value_p >= value_0} and
 *   null_out (nullable, m x P) as midagma_indep_run's dcor: unbiased = 0 counts by dcov^2 and returns
 *   sqrt(max(dcov^2, 0)) / sqrt(sqrt(dvar_x^2 dvar_y^2)) (0 when a variance is <= 0); unbiased = 1
 *   counts by the U-centred dcov^2_U and returns R_U = dcov^2_U / sqrt(dvar_U,x dvar_U,y) (0 when a
 *   variance is <= 0; needs n >= 4).  A pair with a zero-range column gives 0, ge = P.
 *   perms: m x P x n int32 host array, every row a permutation of [0, n) (checked on the host), or
 *   NULL for device permutations: pi for (pair q of the call, permutation p) is the stable argsort
 *   over a of the 64-bit word (o0 << 32) | o1, o = Philox4x32-10(counter (q, p, a, 0), key (seed low
 *   word, seed high word)).  block: the block edge m, 0 for the rule (the power of two in
 *   [64, 1024] with m^2 >= n, else 1024; midagma_dcor_block) or a value in [4, 1024] (tests); the
 *   result depends on it by rounding only.  Evaluations ((pair, permutation), the identity
 *   included) run in chunks whose scratch (cell tables, permutations and inverses, the sort's
 *   buffers, partials) stays within budget_bytes (<= 0: 2 GiB; at least one evaluation; at most
 *   16383); results do not depend on it.  MIDAGMA_E_ARG before any device call: null pointers,
 *   P outside [0, 65535], a pair index outside [0, d), a block that is neither 0 nor in [4, 1024],
 *   no data.
 * perms (tests, diagnostics): the P device permutations of pair q of a call with this seed
 *   (perms_out P x n) and their inverses (inverse_out, nullable). */
typedef struct midagma_dcor midagma_dcor;
int midagma_dcor_create(midagma_dcor** out, int device);
void midagma_dcor_destroy(midagma_dcor* h);
const char* midagma_dcor_last_error(const midagma_dcor* h);
int midagma_dcor_set_data(midagma_dcor* h, const double* X, int64_t n, int64_t d, int64_t budget_bytes);
int midagma_dcor_set_data_dev(midagma_dcor* h, const double* X_dev, int64_t n, int64_t d, int64_t ld,
                              int64_t budget_bytes, void* hip_stream);
int midagma_dcor_run(midagma_dcor* h, const int64_t* pairs, int64_t m, int64_t P, const int32_t* perms,
                     uint64_t seed, int unbiased, int block, int64_t budget_bytes, double* stat, int64_t* ge,
                     double* null_out);
int midagma_dcor_perms(midagma_dcor* h, int64_t q, int64_t P, uint64_t seed, int32_t* perms_out,
                       int32_t* inverse_out);
int midagma_dcor_block(int64_t n);

/* HSIC permutation tests of pairs of columns from low-rank factors of the RBF Gram matrices
 * (additive, ABI 11; csrc/hsic.hip): midagma_indep_run's hsic statistic to within 4 eta (1 + eta)
 * plus rounding, for 2 <= n < 2^31.  A column's Gram matrix K is replaced by F F^T, F (n x r) its
 * pivoted incomplete Cholesky factor stopped when the largest residual diagonal entry is <= eta =
 * tol, so max |K - F F^T| <= eta; with Fc, Gc the column-centred factors of the pair's columns,
 * HSIC(x, y[pi]) = || Fc^T Gc[pi, :] ||_F^2 / n^2, an FP64 MFMA GEMM over the rows in which a
 * permutation gathers rows of Gc.  Not the midagma_indep_ prefix: none of that handle's entries
 * applies to this one.  Errors: midagma_hsic_last_error(handle) (or (NULL)).  One host thread
 * drives a handle at a time.  Results are the same bits run to run and do not depend on
 * budget_bytes.
 * create: no device call; the device is opened by the first set_data*.
 * set_data / set_data_dev: as midagma_dcor_set_data / _dev (arguments, checks, the stream-ordering
 *   rule; X is never written).  The handle keeps the columns by row and sorted (16 bytes a value).
 *   Bandwidths and factors are dropped.
 * set_bandwidths / median_bandwidths: as the midagma_indep_ entries; the medians are numpy's bit for
 *   bit at any n (the sorted column in global memory, one launch a bisection round, the decision on
 *   the device).  Factors are dropped.
 * factor: factors the ncols listed columns at tol (1e-14 <= tol <= 1e-3) and keeps the factors on
 *   the handle; rank_out / resid_out (nullable, ncols each): the rank and the largest residual
 *   diagonal entry reached.  Pivot: the largest residual diagonal entry, ties to the smallest row;
 *   stops at max d <= tol or rank n.  The rank cap is 256: a column that needs more fails with
 *   MIDAGMA_E_ARG and a message that names the column, its rank and its residual.  A zero-range
 *   column has rank 1 and a centred factor that is exactly 0.
 * get_factor (tests, diagnostics): the centred factor of a column that factor factored, n x r_pad
 *   row-major (r_pad = the rank rounded up to a multiple of 16, zero padded), and the r_pad column
 *   means that were subtracted (nullable).
 * run: stat[q], ge[q] = #{p < P : value_p >= value_0} and null_out (nullable, m x P) of the m pairs as
 *   midagma_indep_run's hsic (a pair with a zero-range column: 0, ge = P).  perms: m x P x n int32 host
 *   array, every row a permutation of [0, n) (checked on the device before any row is gathered), or
 *   NULL for midagma_dcor_run's device permutations (the same keys, q the pair's index in the call).
 *   chunk: rows per partial product, 0 for the rule (2048) or a multiple of 16 in [16, 2^20] (tests);
 *   the result depends on it by rounding only.  budget_bytes (<= 0: 2 GiB): half bounds the factors
 *   held at once (pairs are taken in consecutive groups whose columns' factors fit, at least one
 *   pair; a column is refactored when it returns), half the scratch of a batch of evaluations
 *   (partials, permutations, the sort's buffers; at least 4 evaluations).  Columns that were not
 *   factored at this tol are factored first.  MIDAGMA_E_ARG before any device call: null pointers,
 *   P outside [0, 65535], tol or chunk out of range, a pair index outside [0, d), no data, no
 *   bandwidths.
 * perms (tests, diagnostics): the P device permutations of pair q of a call with this seed.
 * profile (diagnostics): ms_out holds 4 doubles: the last median_bandwidths' time, and of the last
 *   run (or factor) the factorisation (host clock, synchronised), the permutations and the
 *   evaluation kernels (device events, summed over the batches).
 * all_pairs (additive, ABI 11): the chi-square test's statistic of every pair of the listed columns
 *   (cols NULL: all d, ncols ignored) from one evaluation a pair, no permutations.  With D = 1 - K
 *   off the diagonal (hyppo's Hsic convention) and A~, B~ the U-centred D of two columns,
 *   cov_u_out (ncols x ncols, required) receives cov_U = <A~, B~> / (n (n - 3)), the variances on
 *   the diagonal; the caller forms R_U = cov_U(x, y) / sqrt(cov_U(x, x) cov_U(y, y)) and
 *   p = chi2.sf(n R_U + 1, 1).  biased_out (nullable, ncols x ncols) receives run's statistic
 *   || Fc_i^T Fc_j ||_F^2 / n^2.  Both are symmetric; a pair with a zero-range column is 0 in both.
 *   Computed from the centred factors and O(n) vectors a column as
 *   <A~_x, A~_y> = || Fc_x^T Fc_y ||_F^2 + 2 n v~_x.v~_y + n^2 c_x c_y - a_x.a_y: the block norms by a
 *   tiled FP64 MFMA pass over the factors side by side (128 x 128 tiles on and above the diagonal,
 *   row slabs staged in LDS, rows in chunks as run's), the two vector Grams by the same pass.  Within
 *   (n - 1) / (n - 3) c_n^2 tol (2 + tol), c_n = (4 n - 4) / (n - 2), plus rounding, of the n^2
 *   definition.  No floating-point atomics: the same bits run to run, whatever budget_bytes, the
 *   column list around a pair and the launch geometry.  budget_bytes (<= 0: 2 GiB): half bounds the
 *   factors and vectors held (all listed columns at once if they fit, else column groups of a
 *   quarter each, two held at a time, refactored when they return), half the chunk partials of a
 *   batch of tiles (at least one tile).  MIDAGMA_E_ARG before any device call: null handle or
 *   output, ncols < 0, tol or chunk out of range, no data, n < 4, no bandwidths, a column outside
 *   [0, d).
 * all_pairs_profile (diagnostics): ms_out holds 3 doubles of the last all_pairs: the factorisation
 *   (host clock), the tiled pass over the factors, and the vectors with their Grams (device
 *   events).  A call of its own: profile's 4 doubles stay 4 for the callers that sized a buffer. */
typedef struct midagma_hsic midagma_hsic;
int midagma_hsic_create(midagma_hsic** out, int device);
void midagma_hsic_destroy(midagma_hsic* h);
const char* midagma_hsic_last_error(const midagma_hsic* h);
int midagma_hsic_set_data(midagma_hsic* h, const double* X, int64_t n, int64_t d, int64_t budget_bytes);
int midagma_hsic_set_data_dev(midagma_hsic* h, const double* X_dev, int64_t n, int64_t d, int64_t ld,
                              int64_t budget_bytes, void* hip_stream);
int midagma_hsic_set_bandwidths(midagma_hsic* h, const double* sigma2, int64_t d);
int midagma_hsic_median_bandwidths(midagma_hsic* h, const int64_t* cols, int64_t ncols, double* sigma2_out);
int midagma_hsic_factor(midagma_hsic* h, const int64_t* cols, int64_t ncols, double tol, int32_t* rank_out,
                        double* resid_out);
int midagma_hsic_get_factor(midagma_hsic* h, int64_t col, double* fc_out, double* mean_out);
int midagma_hsic_run(midagma_hsic* h, const int64_t* pairs, int64_t m, int64_t P, const int32_t* perms,
                     uint64_t seed, double tol, int64_t chunk, int64_t budget_bytes, double* stat, int64_t* ge,
                     double* null_out);
int midagma_hsic_perms(midagma_hsic* h, int64_t q, int64_t P, uint64_t seed, int32_t* perms_out);
int midagma_hsic_profile(const midagma_hsic* h, double* ms_out);
int midagma_hsic_all_pairs(midagma_hsic* h, const int64_t* cols, int64_t ncols, double tol, int64_t chunk,
                           int64_t budget_bytes, double* cov_u_out, double* biased_out);
int midagma_hsic_all_pairs_profile(const midagma_hsic* h, double* ms_out);
#ifdef __cplusplus
}
#endif

#endif /* MIDAGMA_HIP_H_ */
