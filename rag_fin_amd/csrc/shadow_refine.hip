// Prune + refine: the stage between the int8 emit sweep (sq8.hip) and the merge (merge.hip) of an
// SQ8 sweep.  The emit nominates {row, a~} with a~ from the int8 shadow; per row
// |a - a~| <= beta_r = n_q e_r + f_q N' + slack (§4.4b).  One workgroup per query:
//   1. L = the k-th largest lower bound a~ - beta_r of the query's candidates (fewer than k: no cut,
//      no step 2).  The k rows behind those bounds -- the winners -- have a >= L;
//   2. the winners' contract scores (the fp64 chain of merge_common.h, from the fp16 tiles) come
//      first: L2 = the smallest of them.  They are k distinct rows with a >= L2, so the k-th best
//      exact score is >= max(L, L2);
//   3. a candidate that is no winner and has a~ + beta_r < max(L, L2) cannot be a top-k row and is
//      dropped.  Every rounding of the bounds is directed so that it can only keep more (bounds
//      widen, L sinks); the comparison is in fp64 and keeps a tie;
//   4. the other survivors' contract scores follow, and all of them are rounded once to fp32 and
//      written back, compacted and with the winners first, as the query's candidate lists.
// The merge then sees what a FLAT emit would have given it -- a list that contains the top-k, with
// scores within the FLAT eps (k_threshold leaves it in ws.eps) -- and runs unchanged.
// A query the stage cannot serve (a list of the emit overflowed, k_threshold gave the query up, a row
// id past the corpus, more survivors than REFINE_CAP) leaves with its shard-0 counter past the
// capacity: the merge flags it RF_FLAG_CAND_OVERFLOW and the caller answers it through the fp16 chain.
#include "rf_internal.h"
#include "merge_common.h"
#include "sq8.h"

#define REFINE_CAP 2048        // survivors per query the rescoring stage holds (one candidate list)
#define REFINE_RANK_MAX 1024   // candidates up to which a thread holds 4 of them, otherwise 32

struct RefineParams {
  const _Float16* q;     // row-major [B, dim]
  int dim, KS;
  const uint4* tiles;    // fp16 tiles
  const float* err;      // e_r, [blocks][32] in accumulator order
  const uint32_t* mx;    // {N', E} bits
  const float* nq;       // [64]
  const float* fq;       // [64]
  int k;
  uint32_t* cand_cnt;    // [64][RF_CAND_SHARDS]
  uint2* cand;           // [64][RF_CAND_SHARDS][cap]
  uint32_t cap;
  uint32_t n_rows;
  uint32_t stage;        // survivors staged in LDS at a time (refine_stage_rows)
};

// Rows of the rescoring stage: 64 where a row is at most 1 KiB (dim <= 512), else MERGE_STAGE_ROWS, so
// that the workgroup stays under 96 KiB of LDS (77 632 B at dim 384).  The intent is that it fits a CU
// beside emit workgroups of other batches in flight; that co-residency is reasoned from the LDS sizes
// only and has not been measured (no occupancy counters, no clock stamps).
static uint32_t refine_stage_rows(int dim) { return dim <= 512 ? 2 * MERGE_STAGE_ROWS : MERGE_STAGE_ROWS; }
static size_t refine_lds_bytes(int dim) {
  return (size_t)(MERGE_THREADS / 64) * RF_MAX_K * 8 + (size_t)REFINE_CAP * 12 + 64 + (size_t)dim * 2 +
         (size_t)refine_stage_rows(dim) * (dim * 2 + 16);
}

// rescore_rows of merge_common.h -- the same contract_dot8 over rows staged in LDS -- with a stage of
// `stage` rows (a multiple of MERGE_STAGE_ROWS) and a gather without divisions: wave w takes rows w,
// w + 4, ... of the stage, lane l the chunks l and l + 64 of its row, eight rows in flight per wave
// (a row's 16-byte chunks lie 512 B apart in the tiles: every load is a memory request of its own).
__device__ __forceinline__ void refine_rescore(const uint32_t* r_row, uint32_t R, const uint4* __restrict__ tiles,
                                               int KS, const _Float16* qh, uint4* srows, double* r_exact,
                                               uint32_t stage) {
  constexpr int U = 8;
  constexpr uint32_t WAVES = MERGE_THREADS / 64;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const uint32_t wave = (uint32_t)tid >> 6;
  const int chunks = 2 * KS;   // <= 128
  const int srow_stride = 2 * KS + 1;
  for (uint32_t base = 0; base < R; base += stage) {
    const uint32_t nb = (R - base) < stage ? (R - base) : stage;
    for (uint32_t r = wave; r < nb; r += WAVES * U) {
      uint4 v[U][2];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint32_t rr = r + (uint32_t)u * WAVES;
          const int ch = lane + 64 * h;
          v[u][h] = make_uint4(0u, 0u, 0u, 0u);
          if (rr < nb && ch < chunks) v[u][h] = tiles[rf_chunk_index((int64_t)r_row[base + rr], ch, KS)];
        }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint32_t rr = r + (uint32_t)u * WAVES;
          const int ch = lane + 64 * h;
          if (rr < nb && ch < chunks) srows[rr * srow_stride + ch] = v[u][h];
        }
    }
    __syncthreads();
    for (uint32_t r0 = 0; r0 < nb; r0 += MERGE_STAGE_ROWS) {   // 32 rows x 8 lanes = 256 threads
      const uint32_t r = r0 + ((uint32_t)tid >> 3);
      const int j = tid & 7;
      const _Float16* row = (const _Float16*)(srows + (r < nb ? r : 0) * srow_stride);
      const double acc = contract_dot8(qh, row, chunks, j);
      if (j == 0 && r < nb) r_exact[base + r] = acc;
    }
    __syncthreads();
  }
}

// A fp64 sum of two floats into a float that is certainly not below / not above the true sum: one
// step of 2^-52 past the sum's own rounding, then the directed conversion.
__device__ __forceinline__ float bound_up(double x) { return __double2float_ru(x + fabs(x) * 0x1p-52); }
__device__ __forceinline__ float bound_down(double x) { return __double2float_rd(x - fabs(x) * 0x1p-52); }

// Candidate idx of the query: its row, its upper bound and its key.  Larger key <=> larger lower
// bound; the candidate number makes the keys distinct, and no key is 0 (0: no candidate).
__device__ __forceinline__ void refine_bounds(const CandLists& L, const RefineParams& p, float nq, float fq,
                                              float Np, float E, uint32_t idx, bool& bad_row, uint32_t& row,
                                              float& hi, unsigned long long& key) {
  const uint2 e = cand_at(L, idx, p.n_rows, bad_row);
  const float a = __builtin_bit_cast(float, e.y);
  const float er = p.err[(size_t)(e.x >> 5) * 32 + rf_sq8_slot((int)(e.x & 31u))];
  const float beta = rf_sq8_beta(nq, er, fq, Np, E);
  row = e.x;
  hi = bound_up((double)a + (double)beta);
  key = ((unsigned long long)rf_f2ord(bound_down((double)a - (double)beta)) << 32) |
        (unsigned long long)(0xFFFFFFFFu - idx);
}

// Steps 1 to 3 with PER candidates per thread in registers: the rows that survive go to r_row, the
// winners in slots 0..k-1 with their contract scores already in r_exact, and their number to *r_cnt
// (it may pass REFINE_CAP; only the first REFINE_CAP are stored).  Returns the number of rows at the
// head of r_row that are rescored: k where there was a cut, 0 where all stay.  Every thread of the
// workgroup calls it (it has barriers); misc: [0] survivors, [1] the k-th key's high word = the
// bits of L, [2] its low word, [4] winners placed.
template <int PER>
__device__ __forceinline__ uint32_t refine_prune(const CandLists& L, const RefineParams& p, float nq, float fq,
                                                 unsigned long long* wtop, uint32_t* r_row, double* r_exact,
                                                 uint32_t* misc, const _Float16* qh, uint4* srows,
                                                 bool& bad_row) {
  static_assert(PER <= 32, "one bit of `taken` per candidate of a thread");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const uint32_t c = L.c;
  const int k = p.k;
  const float Np = __builtin_bit_cast(float, p.mx[0]);
  const float E = __builtin_bit_cast(float, p.mx[1]);
  uint32_t* r_cnt = misc;
  unsigned long long key[PER];
  uint32_t row[PER];
  float hi[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const uint32_t idx = (uint32_t)tid + MERGE_THREADS * i;
    key[i] = 0ull;
    row[i] = 0u;
    hi[i] = -INFINITY;
    if (idx < c) refine_bounds(L, p, nq, fq, Np, E, idx, bad_row, row[i], hi[i], key[i]);
  }
  if ((uint32_t)k > c) {  // fewer than k candidates: all stay (uniform over the workgroup)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const uint32_t idx = (uint32_t)tid + MERGE_THREADS * i;
      if (idx < c) {
        const uint32_t slot = atomicAdd(r_cnt, 1u);
        if (slot < REFINE_CAP) r_row[slot] = row[i];
      }
    }
    return 0u;
  }
  // extraction rounds, per wave and then across the waves, as in k_merge's pass 1b; a round marks
  // what it took in `taken` and leaves the keys as they are: they tell the winners below
  uint32_t taken = 0u;
  for (int r = 0; r < k; ++r) {
    unsigned long long m = 0ull;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const unsigned long long v = ((taken >> i) & 1u) ? 0ull : key[i];
      m = v > m ? v : m;
    }
    const unsigned long long wm = wave_max_u64(m);
    if (lane == 0) wtop[wave * RF_MAX_K + r] = wm;
    if (wm != 0ull && m == wm) {
#pragma unroll
      for (int i = 0; i < PER; ++i)
        if (key[i] == wm) taken |= 1u << i;
    }
  }
  __syncthreads();
  if (wave == 0) {
    constexpr int NV = (MERGE_THREADS / 64 * RF_MAX_K + 63) / 64;
    unsigned long long v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j = lane + 64 * i;  // j -> (wave j / k, slot j % k)
      v[i] = j < (MERGE_THREADS / 64) * k ? wtop[(j / k) * RF_MAX_K + (j % k)] : 0ull;
    }
    unsigned long long kth = 0ull;
    for (int r = 0; r < k; ++r) {
      unsigned long long m = v[0];
#pragma unroll
      for (int i = 1; i < NV; ++i) m = v[i] > m ? v[i] : m;
      const unsigned long long wm = wave_max_u64(m);
      kth = wm;
      if (wm != 0ull && m == wm) {
#pragma unroll
        for (int i = 0; i < NV; ++i)
          if (v[i] == wm) v[i] = 0ull;
      }
    }
    if (lane == 0) {
      misc[1] = (uint32_t)(kth >> 32);
      misc[2] = (uint32_t)kth;
      misc[0] = (uint32_t)k;   // the winners' slots; the others are counted on from here
    }
  }
  __syncthreads();
  // the keys are distinct and k <= c of them are not 0: exactly k are >= the k-th
  const unsigned long long kth = ((unsigned long long)misc[1] << 32) | (unsigned long long)misc[2];
#pragma unroll
  for (int i = 0; i < PER; ++i)
    if (key[i] >= kth) {
      const uint32_t slot = atomicAdd(misc + 4, 1u);
      if (slot < (uint32_t)k) r_row[slot] = row[i];
    }
  // a row id past the corpus: the query is given up, nothing more is gathered for it (the barrier
  // also puts the winners' rows in place)
  if (__syncthreads_or(bad_row ? 1 : 0) != 0) {
    bad_row = true;
    return 0u;
  }
  refine_rescore(r_row, (uint32_t)k, p.tiles, p.KS, qh, srows, r_exact, p.stage);
  // L2: the winners are k distinct rows with a >= L2.  (A score that is no number gives no bound.)
  double l2 = INFINITY;
  bool nan = false;
  for (int r = 0; r < k; ++r) {
    const double x = r_exact[r];
    nan = nan || x != x;
    l2 = x < l2 ? x : l2;
  }
  if (nan) l2 = -INFINITY;
  const double l1 = (double)rf_ord2f(misc[1]);
  const double cut = l2 > l1 ? l2 : l1;
  // 4 candidates a thread stay in registers across the winners' gather; 32 would cost the kernel a
  // wave of occupancy, so that path (more than REFINE_RANK_MAX candidates) forms its bounds again
  constexpr bool KEEP = PER <= 4;
  if constexpr (KEEP) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const uint32_t idx = (uint32_t)tid + MERGE_THREADS * i;
      if (idx < c && key[i] < kth && (double)hi[i] >= cut) {   // (a winner is in its slot already)
        const uint32_t slot = atomicAdd(r_cnt, 1u);
        if (slot < REFINE_CAP) r_row[slot] = row[i];
      }
    }
  } else {
#pragma unroll 4
    for (uint32_t idx = (uint32_t)tid; idx < c; idx += MERGE_THREADS) {
      uint32_t rw;
      float h;
      unsigned long long ky;
      refine_bounds(L, p, nq, fq, Np, E, idx, bad_row, rw, h, ky);
      if (ky < kth && (double)h >= cut) {
        const uint32_t slot = atomicAdd(r_cnt, 1u);
        if (slot < REFINE_CAP) r_row[slot] = rw;
      }
    }
  }
  return (uint32_t)k;
}

__global__ void __launch_bounds__(MERGE_THREADS) k_shadow_refine(RefineParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned long long* wtop = (unsigned long long*)lds;                      // [4][RF_MAX_K]
  double* r_exact = (double*)(wtop + (MERGE_THREADS / 64) * RF_MAX_K);      // [REFINE_CAP]
  uint32_t* r_row = (uint32_t*)(r_exact + REFINE_CAP);                      // [REFINE_CAP]
  uint32_t* misc = r_row + REFINE_CAP;                                      // 16 words: see refine_prune
  _Float16* qh = (_Float16*)(misc + 16);                                    // [dim]
  uint4* srows = (uint4*)(qh + p.dim);                                      // [p.stage][2 KS + 1]

  const int qi = blockIdx.x;
  const int tid = threadIdx.x;
  bool bad_row = false;
  CandLists L;
  const uint32_t over = cand_lists(L, p.cand_cnt, p.cand, p.cap, qi);
  if (tid == 0) {
    misc[0] = 0u;
    misc[4] = 0u;
  }
  for (int d = tid; d < p.dim; d += MERGE_THREADS) qh[d] = p.q[(size_t)qi * p.dim + d];
  __syncthreads();
  uint32_t done = 0u;   // rows at the head of r_row that refine_prune rescored: the winners
  if (!over) {  // (uniform over the workgroup)
    const float nq = p.nq[qi], fq = p.fq[qi];
    if (L.c <= REFINE_RANK_MAX)
      done = refine_prune<REFINE_RANK_MAX / MERGE_THREADS>(L, p, nq, fq, wtop, r_row, r_exact, misc, qh, srows,
                                                           bad_row);
    else
      done = refine_prune<RF_CAND_CAP / MERGE_THREADS>(L, p, nq, fq, wtop, r_row, r_exact, misc, qh, srows,
                                                       bad_row);
  }
  const bool bad = __syncthreads_or(bad_row ? 1 : 0) != 0;   // (also the barrier behind the compaction)
  const uint32_t R = misc[0];
  const bool give_up = over != 0u || bad || R > REFINE_CAP;
  if (!give_up) {
    refine_rescore(r_row + done, R - done, p.tiles, p.KS, qh, srows, r_exact + done, p.stage);
    // the lists of a query are contiguous: survivor i is entry i % cap of list i / cap
    uint2* out = p.cand + (size_t)qi * RF_CAND_SHARDS * p.cap;
    for (uint32_t i = tid; i < R; i += MERGE_THREADS)
      out[i] = make_uint2(r_row[i], __builtin_bit_cast(uint32_t, (float)r_exact[i]));
  }
  // (every thread read the counters in cand_lists, before the barriers above)
  if (tid < RF_CAND_SHARDS) {
    const uint32_t first = (uint32_t)tid * p.cap;
    uint32_t n = R > first ? R - first : 0u;
    if (n > p.cap) n = p.cap;
    if (give_up) n = tid == 0 ? p.cap + 1u : 0u;
    p.cand_cnt[qi * RF_CAND_SHARDS + tid] = n;
  }
}

int rf_launch_shadow_refine(const rf_index* ix, const void* q, int B, int k, const rf_workspace& ws,
                            const rf_sq8_ws& sw, hipStream_t st) {
  static_assert(REFINE_CAP <= RF_SHARD_CAP * RF_CAND_SHARDS, "the survivors must fit the candidate lists");
  RefineParams p{};
  p.q = (const _Float16*)q;
  p.dim = ix->dim;
  p.KS = ix->KS;
  p.tiles = ix->tiles;
  p.err = ix->sq8_err;
  p.mx = ix->sq8_max;
  p.nq = sw.nq;
  p.fq = sw.fq;
  p.k = k;
  p.cand_cnt = ws.cand_cnt;
  p.cand = ws.cand;
  p.cap = RF_SHARD_CAP;
  p.n_rows = (uint32_t)ix->size;
  p.stage = refine_stage_rows(ix->dim);
  const size_t lds = refine_lds_bytes(ix->dim);
  static rf_lds_attr lds_attr;
  RF_HIP(rf_ensure_lds(lds_attr, (const void*)k_shadow_refine, lds));
  hipLaunchKernelGGL(k_shadow_refine, dim3(B), dim3(MERGE_THREADS), lds, st, p);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
