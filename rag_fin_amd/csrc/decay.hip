// Decay ranker: the row weights of a time-decayed search (include/ragfin.h, "decayed search"; DESIGN
// 4.4q).  One lane per row: w = 1 within `offset` of `origin`, `decay` at distance offset + scale,
// along a bell curve, an exponential or a straight line; bit for bit
// rag_fin_amd/ranker.py:decay_weights_reference.  Every step is one IEEE fp64 operation, rounded on
// its own, and 2^-t is its own arithmetic, not a libm's: the same bytes on the host and on the
// device, whatever order the workgroups run in.
#include "rf_internal.h"

#define DECAY_THREADS 256

// No contraction anywhere below: a multiplication followed by an addition stays two roundings.  (The
// __dmul_rn / __dadd_rn of the HIP headers are the plain operators and fuse into an fma once inlined
// next to each other; the operators written under this pragma carry no licence to.)
#pragma clang fp contract(off)

// 2^-t for t >= 0: 0 unless t < 1100 (a NaN and +inf included); else n = floor(t + 0.5), f = t - n
// (exact), x = -(f ln2), the degree-13 Taylor polynomial of e^x in Horner form and the scaling by
// 2^-n.  p lies in [0.70, 1.42], so p 2^-min(n, 1000) is exact and the second factor, 2^-(n - 1000)
// for n > 1000, rounds once, into the subnormals: what ldexp(p, -n) gives.
__device__ __forceinline__ double exp2_neg(double t) {
  if (!(t < 1100.0)) return 0.0;
  const double n = floor(t + 0.5);
  const double f = t - n;
  const double x = -(f * 0.6931471805599453);
  constexpr double C[14] = {1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0,
                            1.0 / 362880.0,     1.0 / 40320.0,     1.0 / 5040.0,     1.0 / 720.0,
                            1.0 / 120.0,        1.0 / 24.0,        1.0 / 6.0,        1.0 / 2.0,
                            1.0,                1.0};
  double p = C[0];
#pragma unroll
  for (int i = 1; i < 14; ++i) p = p * x + C[i];
  const int ni = (int)n;                       // 0 .. 1100
  const int n1 = ni < 1000 ? ni : 1000;
  const double s1 = __builtin_bit_cast(double, (uint64_t)(1023 - n1) << 52);          // 2^-n1
  const double s2 = __builtin_bit_cast(double, (uint64_t)(1023 - (ni - n1)) << 52);   // 2^-(n - n1), >= 2^-100
  return (p * s1) * s2;
}

// INT: the column holds int64 (rounded to the nearest double), else fp64.
template <bool INT>
__global__ void __launch_bounds__(DECAY_THREADS) k_decay_weights(const void* __restrict__ col, int64_t n_rows,
                                                                 int function, double origin, double scale,
                                                                 double offset, double shape,
                                                                 double* __restrict__ w64, float* __restrict__ w32) {
  const int64_t row = (int64_t)blockIdx.x * DECAY_THREADS + threadIdx.x;
  if (row >= n_rows) return;
  const double v = INT ? (double)((const int64_t*)col)[row] : ((const double*)col)[row];
  const double e = fabs(v - origin) - offset;
  const double d = e > 0.0 ? e : 0.0;
  double w;
  if (function == RF_DECAY_LINEAR) {
    const double u = (shape - d) / shape;
    w = u > 0.0 ? u : 0.0;
  } else {
    const double r = d / scale;
    w = exp2_neg(shape * (function == RF_DECAY_GAUSS ? r * r : r));
  }
  if (v != v) w = 0.0;
  w64[row] = w;
  w32[row] = (float)w;   // round to nearest even
}

extern "C" int rf_decay_weights(const void* column_dev, int column_is_int64, int64_t n_rows, int function,
                                double origin, double scale, double offset, double shape, double* w64_dev,
                                float* w32_dev, void* stream) {
  if (!column_dev || !w64_dev || !w32_dev) {
    rf_set_error("rf_decay_weights: null argument");
    return RF_ERR_INVALID;
  }
  if (n_rows < 0 || n_rows > (int64_t)0xFFFFFFFFll - 32) {
    rf_set_error("rf_decay_weights: n_rows = %lld out of range", (long long)n_rows);
    return RF_ERR_INVALID;
  }
  if (function != RF_DECAY_GAUSS && function != RF_DECAY_EXP && function != RF_DECAY_LINEAR) {
    rf_set_error("rf_decay_weights: unknown function code %d", function);
    return RF_ERR_INVALID;
  }
  const double fmax = 1.79769313486231570e308;
  // (each comparison is false for a NaN)
  if (!(origin >= -fmax && origin <= fmax) || !(scale > 0.0 && scale <= fmax) || !(offset >= 0.0 && offset <= fmax) ||
      !(shape > 0.0 && shape <= fmax)) {
    rf_set_error("rf_decay_weights: need a finite origin, finite scale > 0, offset >= 0 and shape > 0 (got %g, %g, %g, %g)",
                 origin, scale, offset, shape);
    return RF_ERR_INVALID;
  }
  if ((((uintptr_t)column_dev) & 7) || (((uintptr_t)w64_dev) & 7) || (((uintptr_t)w32_dev) & 3)) {
    rf_set_error("rf_decay_weights: misaligned column or output");
    return RF_ERR_INVALID;
  }
  if (n_rows == 0) return RF_OK;
  const dim3 grid((uint32_t)((n_rows + DECAY_THREADS - 1) / DECAY_THREADS));
  if (column_is_int64)
    hipLaunchKernelGGL(k_decay_weights<true>, grid, dim3(DECAY_THREADS), 0, (hipStream_t)stream, column_dev, n_rows,
                       function, origin, scale, offset, shape, w64_dev, w32_dev);
  else
    hipLaunchKernelGGL(k_decay_weights<false>, grid, dim3(DECAY_THREADS), 0, (hipStream_t)stream, column_dev, n_rows,
                       function, origin, scale, offset, shape, w64_dev, w32_dev);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
