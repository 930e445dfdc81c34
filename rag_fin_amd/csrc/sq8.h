// SQ8 error bound, shared by k_threshold (merge.hip) and the debug dump (sq8.hip).
//
// For query q and row c: a = q.c, q~ = t_q q^, c~ = s_r c^_r, a~ = fl(fl(t_q s_r) D) with the
// exact integer D = q^.c^_r.  Then
//   |a - a~| <= n_q e_r + f_q ||c~|| + rounding,   n_q >= ||q||, f_q >= ||q - q~||, e_r >= ||c - c~||,
// and ||c~|| <= N'.  The slack covers the two fp32 roundings of a~, the fp32 evaluation of the emit
// test, the fp32 cut of the merge and the fp64 ranking chain; it is 2^-18 of the magnitude scale
// (n_q + f_q) N' + n_q E that all of them are relative to.
#pragma once
#include <hip/hip_runtime.h>

#define RF_SQ8_SLACK 3.814697265625e-06  // 2^-18

__device__ __forceinline__ double rf_sq8_slack(double nq, double fq, double Np, double E) {
  return RF_SQ8_SLACK * ((nq + fq) * Np + nq * E);
}
// delta_q = n_q E + f_q N' + slack, rounded up: bounds |a - a~| for every row of the corpus
__device__ __forceinline__ float rf_sq8_delta(float nq, float fq, float Np, float E) {
  const double d = (double)nq * E + (double)fq * Np + rf_sq8_slack(nq, fq, Np, E);
  return __double2float_ru(d);
}
// beta_r = n_q e_r + f_q N' + slack, rounded up: bounds |a - a~| for the row whose residual norm is
// e_r (e_r <= E, so beta_r <= delta_q); what the refine stage prunes by
__device__ __forceinline__ float rf_sq8_beta(float nq, float er, float fq, float Np, float E) {
  const double d = (double)nq * er + (double)fq * Np + rf_sq8_slack(nq, fq, Np, E);
  return __double2float_ru(d);
}
// emit threshold thr_q = m_k - eps - f_q N' - slack, rounded down; a row is emitted when
// a~ + n_q e_r >= thr_q
__device__ __forceinline__ float rf_sq8_thr(float mk, float eps, float nq, float fq, float Np, float E) {
  const double t = (double)mk - (double)eps - (double)fq * Np - rf_sq8_slack(nq, fq, Np, E);
  return __double2float_rd(t);
}
// sqrt of an fp64 sum of squares, rounded up into fp32 (the 2^-40 pad covers the fp64 sum's rounding)
__device__ __forceinline__ float rf_sqrt_up(double s2) {
  return __double2float_ru(sqrt(s2 * (1.0 + 0x1p-40)));
}
// position of row r (0..31) of a block in the per-block metadata arrays: accumulator order, so the
// lane half h finds the 16 values of its registers i (row (i & 3) + 8 (i >> 2) + 4 h) contiguous
__host__ __device__ __forceinline__ int rf_sq8_slot(int r) { return ((r >> 2) & 1) * 16 + (r & 3) + 4 * (r >> 3); }
