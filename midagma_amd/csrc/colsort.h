// The segmented stable LSD radix sort of corr.hip, for the other files that sort on the device
// (dcor.hip and hsic.hip: the columns' argsort; coltest.h: the Philox keys of their permutations).
//
// nseg segments of n (64-bit key, 32-bit payload) records each, segment c at offset c n of every
// buffer.  The records start in K0 / I0; a pass that moves a segment writes it to the other side,
// and a pass in which all keys of a segment share the digit is skipped for that segment (key_or /
// key_and: the OR and AND of the segment's keys; ~0 / 0 make every pass live).  The sort is stable,
// uses no atomics on its outputs and gives the same bits run to run.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace midagma {

struct SegSort {
  uint64_t *K0, *K1;                   // nseg n keys each
  uint32_t *I0, *I1;                   // nseg n payloads each
  unsigned long long *key_or, *key_and;  // nseg each
  uint32_t* hist;                      // nseg * segsort_hist_per_segment(n)
};

// histogram words per segment
int64_t segsort_hist_per_segment(int64_t n);
// the eight passes (nseg <= 65535)
void launch_segsort(const SegSort& s, int64_t n, int64_t nseg, hipStream_t stream);
// order[c n + i] = the payload at sorted position i of segment c; inverse (nullable):
// inverse[c n + payload] = i.  Payloads must be < n.
void launch_segsort_payload(const SegSort& s, int64_t n, int64_t nseg, int32_t* order, int32_t* inverse,
                            hipStream_t stream);
// order[c n + i] (int32, column-major d x n) = the row at position i of the stable argsort of column
// c of X (n x d row-major, ldx), -0.0 equal to +0.0: midagma_colargsort's body.  Throws
// std::invalid_argument when X holds inf or nan.  Synchronises `stream` before it returns.
void colargsort_run(const double* X_dev, int64_t n, int64_t d, int64_t ldx, int32_t* order_dev, int64_t budget_bytes,
                    hipStream_t stream);

}  // namespace midagma
