// Device helpers shared by the candidate merges, k_merge (merge.hip) and k_merge_grouped
// (grouped.hip), and by the MMR stage k_mmr (mmr.hip).  The candidate order, the contract dot and
// the rescoring stage are the exactness contract (mirrored by oracle/search.py): all
// three take them from here.
#pragma once
#include "rf_internal.h"

#define MERGE_THREADS 256     // one workgroup per query
#define MERGE_STAGE_ROWS 32   // rows of R staged in LDS at a time: 8 lanes per row

// Wave-wide reductions on the DPP network (row_shr 1/2/4/8, row_bcast 15/31):
// six VALU-rate steps instead of six LDS-crossbar shuffles.  The full result
// lands in lane 63 and is broadcast with readlane.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_keep(uint32_t v) {
  // lanes without a valid source (or in a masked row) keep their own value
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#define RF_STEP(ctrl, rm)                                                           \
  {                                                                                 \
    const uint32_t lo = dpp_keep<ctrl, rm>((uint32_t)v);                            \
    const uint32_t hi = dpp_keep<ctrl, rm>((uint32_t)(v >> 32));                    \
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;               \
    v = w > v ? w : v;                                                              \
  }
  RF_STEP(0x111, 0xF) RF_STEP(0x112, 0xF) RF_STEP(0x114, 0xF) RF_STEP(0x118, 0xF)
  RF_STEP(0x142, 0xA) RF_STEP(0x143, 0xC)
#undef RF_STEP
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

// larger key <=> (higher MFMA score, then lower row)
__device__ __forceinline__ unsigned long long cand_key(uint2 e) {
  return ((unsigned long long)rf_f2ord(__builtin_bit_cast(float, e.y)) << 32) |
         (unsigned long long)(0xFFFFFFFFu - e.x);
}
__device__ __forceinline__ float key_score(unsigned long long key) {
  return rf_ord2f((uint32_t)(key >> 32));
}
__device__ __forceinline__ uint32_t key_row(unsigned long long key) {
  return 0xFFFFFFFFu - (uint32_t)key;
}

// (score desc, row asc): is (s1, r1) ranked strictly before (s2, r2)?  Row: uint32_t for the rows
// of one index, int64_t for the global ids of the exhaustive and cross-shard paths.
template <class Row>
__device__ __forceinline__ bool ranks_before(double s1, Row r1, double s2, Row r2) {
  return (s1 > s2) || (s1 == s2 && r1 < r2);
}

// The candidate lists of one query: RF_CAND_SHARDS lists of up to `cap` entries; candidate
// g -> (list s, entry g - off[s]).
struct CandLists {
  const uint2* lists;
  uint32_t cap;
  uint32_t off[RF_CAND_SHARDS + 1];
  uint32_t c;   // candidates the merge takes: at most RF_CAND_CAP
};
// Returns RF_FLAG_CAND_OVERFLOW if a list ran past its capacity or the lists hold more than
// RF_CAND_CAP together, 0 otherwise.
__device__ __forceinline__ uint32_t cand_lists(CandLists& L, const uint32_t* __restrict__ cand_cnt,
                                               const uint2* __restrict__ cand, uint32_t cap, int qi) {
  uint32_t fl = 0u;
  L.off[0] = 0u;
#pragma unroll
  for (int s = 0; s < RF_CAND_SHARDS; ++s) {
    const uint32_t n = cand_cnt[qi * RF_CAND_SHARDS + s];
    if (n > cap) fl = RF_FLAG_CAND_OVERFLOW;
    L.off[s + 1] = L.off[s] + (n < cap ? n : cap);
  }
  const uint32_t total = L.off[RF_CAND_SHARDS];
  if (total > RF_CAND_CAP) fl = RF_FLAG_CAND_OVERFLOW;
  L.c = total < RF_CAND_CAP ? total : RF_CAND_CAP;
  L.lists = cand + (size_t)qi * RF_CAND_SHARDS * cap;
  L.cap = cap;
  return fl;
}
// Candidate g.  A row id past the corpus cannot come from the sweep (k_threshold /
// k_group_threshold zero the counters of every search); should one appear (a caller sharing one
// workspace between concurrent searches), never let it reach a row gather -- make it the worst
// candidate and report it (the merge then flags the query).
__device__ __forceinline__ uint2 cand_at(const CandLists& L, uint32_t g, uint32_t n_rows, bool& bad_row) {
  uint32_t s = 0u, first = 0u;   // list s starts at candidate first = off[s] (off ascends)
#pragma unroll
  for (int t = 1; t < RF_CAND_SHARDS; ++t)
    if (g >= L.off[t]) {
      s = (uint32_t)t;
      first = L.off[t];
    }
  uint2 e = L.lists[(size_t)s * L.cap + (g - first)];
  if (e.x >= n_rows) {
    e.x = 0u;
    e.y = 0xFF800000u;  // -inf
    bad_row = true;
  }
  return e;
}

// The contract dot product of two fp16 rows of `chunks` 16-byte chunks in LDS, by 8 adjacent
// lanes (an aligned group of 8; every lane of the wave calls it): lane j owns chain j of the
// contract (dims j, j + 8, ... ascending, one fma per step; the product of two fp16 values is
// exact in fp64, so the result does not depend on which row is `a`), combined by the xor tree
// 1, 2, 4 = ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)).  Every lane of the group returns the dot.
__device__ __forceinline__ double contract_dot8(const _Float16* a, const _Float16* b, int chunks, int j) {
  double acc = 0.0;
#pragma unroll 8
  for (int ch = 0; ch < chunks; ++ch)
    acc = fma((double)a[8 * ch + j], (double)b[8 * ch + j], acc);
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  acc += __shfl_xor(acc, 4);
  return acc;
}

// The fp64 ranking scores of the rows r_row[0..R) into r_exact, by all MERGE_THREADS threads:
// the rows pass through LDS MERGE_STAGE_ROWS at a time (srows: [32][2 KS + 1] uint4; one HBM
// latency per stage instead of one per 16-byte chunk), then 8 lanes per row run contract_dot8
// against the query.  qh: the query row as fp16 in LDS.
__device__ __forceinline__ void rescore_rows(const uint32_t* r_row, uint32_t R, const uint4* __restrict__ tiles,
                                             int KS, const _Float16* qh, uint4* srows, double* r_exact) {
  const int tid = threadIdx.x;
  const int chunks = 2 * KS;
  const int srow_stride = 2 * KS + 1;
  for (uint32_t base = 0; base < R; base += MERGE_STAGE_ROWS) {
    const uint32_t nb = (R - base) < MERGE_STAGE_ROWS ? (R - base) : MERGE_STAGE_ROWS;
    for (uint32_t idx = tid; idx < nb * (uint32_t)chunks; idx += MERGE_THREADS) {
      const uint32_t r = idx / chunks, ch = idx % chunks;
      srows[r * srow_stride + ch] = tiles[rf_chunk_index((int64_t)r_row[base + r], (int)ch, KS)];
    }
    __syncthreads();
    {
      const uint32_t r = (uint32_t)tid >> 3;   // 32 rows x 8 lanes = 256 threads
      const int j = tid & 7;
      const _Float16* row = (const _Float16*)(srows + (r < nb ? r : 0) * srow_stride);
      const double acc = contract_dot8(qh, row, chunks, j);
      if (j == 0 && r < nb) r_exact[base + r] = acc;
    }
    __syncthreads();
  }
}
