// Shared by lexical_update.hip and lexical_build.hip: the workgroup shape of the kernels that walk
// chunks of RF_LEX_CHUNK elements, and the workgroup-wide exclusive scan their prefix sums are made of.
#pragma once
#include "rf_internal.h"

#define LEX_THREADS 256
#define LEX_WAVES (LEX_THREADS / 64)
#define LEX_PER_THREAD (RF_LEX_CHUNK / LEX_THREADS)

static_assert(RF_LEX_CHUNK % LEX_THREADS == 0, "a thread owns whole strided slots of a chunk");

__device__ __forceinline__ int64_t lex_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- the prefix sum: reduce per chunk, scan the chunk sums, scan inside the chunks -------------------
// Exclusive scan of (a, b) over the workgroup in thread order; (ta, tb) = the workgroup's totals.
__device__ __forceinline__ void lex_block_scan2(int64_t& a, int64_t& b, int64_t& ta, int64_t& tb, int64_t (*s_w)[2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  long long ia = a, ib = b;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long va = __shfl_up(ia, o), vb = __shfl_up(ib, o);
    if (lane >= o) {
      ia += va;
      ib += vb;
    }
  }
  if (lane == 63) {
    s_w[w][0] = ia;
    s_w[w][1] = ib;
  }
  __syncthreads();
  int64_t oa = 0, ob = 0;
  ta = 0;
  tb = 0;
#pragma unroll
  for (int i = 0; i < LEX_WAVES; ++i) {
    if (i < w) {
      oa += s_w[i][0];
      ob += s_w[i][1];
    }
    ta += s_w[i][0];
    tb += s_w[i][1];
  }
  __syncthreads();   // s_w is free for the next round
  a = oa + (int64_t)ia - a;
  b = ob + (int64_t)ib - b;
}
