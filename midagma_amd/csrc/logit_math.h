// The logistic loss's two scalar functions, shared by its device paths (gemm.hip's sigmoid
// epilogues on the large-tile launch chain, logit_blk.h's row-block score phase in the batch) so
// that both use the same arithmetic.
#pragma once

#include <hip/hip_runtime.h>

namespace midagma {

// numpy.logaddexp(0, x) (npy_math: log1p/exp split on the sign of the difference)
__device__ __forceinline__ double logaddexp0(double x) {
  if (x == 0.0) return 0.69314718055994530942;
  const double t = -x;
  if (t > 0) return log1p(exp(-t));
  return x + log1p(exp(t));
}

// scipy.special.expit as the reference's sigmoid evaluates it (linear.py:91)
__device__ __forceinline__ double expit(double x) { return 1.0 / (1.0 + exp(-x)); }

}  // namespace midagma
