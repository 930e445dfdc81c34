// The span order and the per-start search shared by the reader's two decoders: k_qa_spans (reader.hip, one pair
// in one workgroup) and the stitched decode over sliding windows (reader_windows.hip, one 512-start tile of a
// context per workgroup).
#pragma once
#include "rf_internal.h"

#define RD_THREADS 512            // one thread per position of the pair (T <= 512) and per candidate start
#define RD_WAVES (RD_THREADS / 64)
#define RD_NONE 0x7fffffff        // key of "no candidate": loses against every candidate

// (z desc, key asc) with key = (start << 6) | (end - start): the order of the output, (z desc, i asc, j asc).
// Keys of distinct candidates differ, so this is a strict total order: the maximum of a set is one element,
// whatever the order in which a reduction meets its members.
__device__ __forceinline__ bool rd_better(float za, int ka, float zb, int kb) {
  return za > zb || (za == zb && ka < kb);
}

// The best candidate of start i that comes strictly AFTER (zp, jp) in the start's own order (z desc, j asc);
// (+inf, -1) = the best of all.  j ascends and only a strictly greater z replaces the held one, so among equal
// z the smallest j is kept.  -> key, or RD_NONE.
__device__ __forceinline__ int rd_next(const float* __restrict__ e, float si, int i, int jmax, float zp, int jp,
                                       float* zout) {
  float bz = -INFINITY;
  int bj = -1;
  // (unrolled: the LDS reads of eight ends are in flight together.  In a selection round ONE lane runs this
  // loop while the workgroup waits at the barrier; taken read by read, a round cost 4.4 us: DESIGN.md 5.0o)
#pragma unroll 8
  for (int j = i; j <= jmax; ++j) {
    const float z = si + e[j];
    const bool after = z < zp || (z == zp && j > jp);
    if (after && (bj < 0 || z > bz)) {
      bz = z;
      bj = j;
    }
  }
  *zout = bz;
  return bj < 0 ? RD_NONE : ((i << 6) | (bj - i));
}
