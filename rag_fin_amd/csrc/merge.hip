// Threshold selection, candidate merge + exact rescoring, exhaustive fallback
// and cross-shard merge.  Together with scan.hip this is the GPU restatement of
// what Milvus returns for Collection.search(..., COSINE, top_k)
// (vector_rag_mcp/main.py:51-70): the k best rows by descending score.
//
// Ranking contract (mirrored by oracle/search.py): the score of (query, row)
// is the fp64 value p = ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)) where chain
// p_j = sum over d = j, j+8, j+16, ... (ascending) of q[d]*c[d], one fused
// multiply-add per step (products of two fp16 values are exact in fp64); rows
// are ranked by (score descending, row id ascending).
// The MFMA scan only nominates candidates; every returned score comes from the
// fp64 chain, so ids and ranks are bit-reproducible on the CPU.
#include "rf_internal.h"
#include "merge_common.h"
#include "sq8.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// (dpp_keep and wave_max_u64: merge_common.h)
__device__ __forceinline__ float wave_max_f(float v) {
#define RF_STEP(ctrl, rm) \
  v = fmaxf(v, __builtin_bit_cast(float, dpp_keep<ctrl, rm>(__builtin_bit_cast(uint32_t, v))));
  RF_STEP(0x111, 0xF) RF_STEP(0x112, 0xF) RF_STEP(0x114, 0xF) RF_STEP(0x118, 0xF)
  RF_STEP(0x142, 0xA) RF_STEP(0x143, 0xC)
#undef RF_STEP
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float wave_sum_f(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// fp64 ranking score of the contract: eight interleaved chains (chain j takes
// dims d = j mod 8, ascending, one fma per step) combined by a pairwise tree.
__device__ __forceinline__ double tree8(const double (&p)[8]) {
  return ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
}
__device__ __forceinline__ double exact_dot(const _Float16* __restrict__ qrow,
                                            const uint4* __restrict__ tiles, int64_t row, int KS) {
  double p[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = 0.0;
  for (int c = 0; c < 2 * KS; ++c) {
    const uint4 cv = tiles[rf_chunk_index(row, c, KS)];
    const uint4 qv = *(const uint4*)(qrow + 8 * c);
    const half8 ch = __builtin_bit_cast(half8, cv);
    const half8 qh = __builtin_bit_cast(half8, qv);
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = fma((double)qh[j], (double)ch[j], p[j]);
  }
  return tree8(p);
}

// ---- emit threshold -------------------------------------------------------------
// One wave per query.  eps bounds |MFMA fp32 score - exact score|:
// dim * 2^-23 * ||q|| * max||c||  (fp16 products are exact in fp32; the bound
// covers dim roundings of the fp32 accumulator at one ulp each).  The scan
// keeps every row whose MFMA score is >= kth - 2*eps, which provably contains
// every row of the exact top-k ("why the result is exact").
//
// Sample fold (fold != nullptr, scan.hip): then the wave also walks its query's kept lists, one
// per sample wave.  A list whose second best score is below thr holds every row of its wave with
// a score >= thr (at most its best): that row is appended here, with the same {row, score bits}
// the emit would have appended.  Otherwise the query's bit is set in the sample wave's rescan
// mask and nothing of that wave is appended; the first query to mark a wave lists the wave's
// blocks for the emit sweep.  The counters start at what was appended (no atomics: the wave owns
// its query's lists until the emit runs).  The lists are loaded before the k-th maximum is
// selected: their HBM round trip runs under the extraction rounds.
struct ThrFold {
  const uint4* lists;         // nullptr: no fold (the counters start at zero)
  unsigned long long* rmask;
  uint32_t* rlist;
  uint32_t* rcnt;
  uint2* cand;
  uint32_t cap;
  uint32_t n_samp, bstride, W;
  int force;                  // every list counts as incomplete (diagnostics)
};
// SQ8 (rf_search_sq8; mx == nullptr: FLAT).  The k-th partition maximum m_k of the fp16 sample
// then becomes the int8 emit threshold thr_q = m_k - eps - f_q N' - slack; eps_out
// receives the FLAT eps as ever, for the merge behind the refine stage (shadow_refine.hip).
struct ThrSq8 {
  const float* nq;
  const float* fq;
  const uint32_t* mx;         // {N', E} bits
};
// eps of query qi (the bound above), the same value in every lane of the wave
__device__ __forceinline__ float query_eps(const _Float16* __restrict__ q, int qi, int B, int dim, int lane,
                                           const uint32_t* __restrict__ max_norm2) {
  float s = 0.f;
  if (qi < B)
    for (int d = lane; d < dim; d += 64) {
      const float x = (float)q[(size_t)qi * dim + d];
      s = fmaf(x, x, s);
    }
  s = wave_sum_f(s);
  const float cmax2 = __builtin_bit_cast(float, *max_norm2);
  return 1.25f * (float)dim * 1.1920929e-7f * sqrtf(s) * sqrtf(cmax2);
}

// Range search: the sample pass of a band sweep clips by eps before k_threshold has run, so this
// one-wave-per-query kernel writes it first (k_threshold writes the same value again).
__global__ void __launch_bounds__(64) k_band_eps(const _Float16* __restrict__ q, int B, int dim,
                                                 const uint32_t* __restrict__ max_norm2,
                                                 float* __restrict__ eps_out) {
  const float eps = query_eps(q, blockIdx.x, B, dim, threadIdx.x, max_norm2);
  if (threadIdx.x == 0) eps_out[blockIdx.x] = eps;
}

// BAND (range search, rf_band {lo, hi}): pmax holds the partition maxima over the rows with
// score <= hi - eps (scan.hip), and thr = max(m_k - 2 eps, lo - eps): with fewer than k such
// maxima, or a k-th below the floor of the band, every row that can have a > lo is emitted
// (DESIGN 4.4c).  No fold and no SQ8 in this form.
template <bool BAND>
__global__ void __launch_bounds__(64) k_threshold(const _Float16* __restrict__ q, int B, int dim,
                                                  int k, const float* __restrict__ pmax, int P,
                                                  const uint32_t* __restrict__ max_norm2,
                                                  float* __restrict__ thr, float* __restrict__ eps_out,
                                                  uint32_t* __restrict__ cand_cnt, ThrFold fd, ThrSq8 sq,
                                                  rf_band bd) {
  const int qi = blockIdx.x;
  const int lane = threadIdx.x;
  // kept lists per lane and chunk: the first chunk (1024 sample waves, all of a 4-wave sample
  // pass) is in flight during the extraction rounds; an 8-wave pass has a second
  constexpr int FI = 16;
  const bool folding = fd.lists && qi < B;  // wave-uniform
  uint32_t f_best[FI], f_row[FI], f_second[FI];
  auto load_lists = [&](uint32_t base) {
#pragma unroll
    for (int i = 0; i < FI; ++i) {
      const uint32_t sw = base + (uint32_t)(lane + 64 * i);
      f_best[i] = f_second[i] = 0xFF800000u;  // -inf: nothing to append, complete
      f_row[i] = 0u;
      if (folding && sw < fd.W) {
        const uint4 e = fd.lists[(size_t)qi * RF_FOLD_WAVES + sw];  // a query's lists are contiguous
        f_best[i] = e.x;
        f_row[i] = e.y;
        f_second[i] = e.z;
      }
    }
  };
  load_lists(0u);
  const float eps = query_eps(q, qi, B, dim, lane, max_norm2);

  float t;
  bool give_up = false;  // SQ8 only: the query is left to FLAT (see below)
  if (qi >= B) {
    t = INFINITY;
  } else if (P <= 0) {
    t = -INFINITY;
  } else {
    float v[RF_SAMPLE_WGS / 64];
#pragma unroll
    for (int i = 0; i < RF_SAMPLE_WGS / 64; ++i) {
      const int j = lane + 64 * i;
      v[i] = (j < P) ? pmax[(size_t)qi * P + j] : -INFINITY;
    }
    float kth = -INFINITY;
    for (int r = 0; r < k; ++r) {
      float m = v[0];
#pragma unroll
      for (int i = 1; i < RF_SAMPLE_WGS / 64; ++i) m = fmaxf(m, v[i]);
      const float wm = wave_max_f(m);
      kth = wm;
      if (wm == -INFINITY) break;
      const unsigned long long who = __ballot(m == wm);
      const int winner = __ffsll((long long)who) - 1;
      if (lane == winner) {
        bool done = false;
#pragma unroll
        for (int i = 0; i < RF_SAMPLE_WGS / 64; ++i)
          if (!done && v[i] == wm) {
            v[i] = -INFINITY;
            done = true;
          }
      }
    }
    t = (kth == -INFINITY) ? -INFINITY : kth - 2.f * eps;
    if (sq.mx && kth != -INFINITY) {
      t = rf_sq8_thr(kth, eps, sq.nq[qi], sq.fq[qi], __builtin_bit_cast(float, sq.mx[0]),
                     __builtin_bit_cast(float, sq.mx[1]));
      // Give-up rule: when more than 3/4 of the sample partitions left after the k largest hold a
      // row that clears thr_q, the int8 sweep would emit a large share of the corpus (a bound too
      // loose for this query, e.g. a dominant channel) and overflow anyway.  The query then emits
      // nothing and its shard-0 counter is set past the capacity, so the merge flags it and the
      // caller answers it through FLAT: only the speed depends on this rule, never the answer.
      // Applied with at least 64 partitions left (k near P says nothing about the density).
      const uint32_t rest = (uint32_t)(P > k ? P - k : 0);
      uint32_t above = 0u;
#pragma unroll
      for (int i = 0; i < RF_SAMPLE_WGS / 64; ++i) above += (uint32_t)__popcll(__ballot(v[i] >= t));
      if (rest >= 64u && above * 4u > rest * 3u) {
        give_up = true;
        t = INFINITY;
      }
    }
  }
  if (BAND && qi < B) t = fmaxf(t, rf_band_floor(bd.lo - (double)eps));
  if (lane == 0) {
    thr[qi] = t;
    eps_out[qi] = eps;   // SQ8 too: the merge runs behind the refine stage, on fp16-accurate scores (§4.4n)
  }
  uint32_t appended = 0u;  // wave-uniform; entry g goes to shard g % RF_CAND_SHARDS
  if (folding) {
    uint2* lists = fd.cand + (size_t)qi * RF_CAND_SHARDS * fd.cap;
    for (uint32_t base = 0; base < fd.W; base += 64u * FI) {
      if (base) load_lists(base);
      uint32_t incomplete = 0u;  // bit i: the list of sample wave base + lane + 64 i
#pragma unroll
      for (int i = 0; i < FI; ++i) {
        const uint32_t sw = base + (uint32_t)(lane + 64 * i);
        const bool valid = sw < fd.W;
        const bool complete = !fd.force && __builtin_bit_cast(float, f_second[i]) < t;
        incomplete |= (valid && !complete) ? (1u << i) : 0u;
        const bool app = valid && complete && __builtin_bit_cast(float, f_best[i]) >= t;
        const unsigned long long m = __ballot(app);
        if (app) {
          const uint32_t g = appended + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
          const uint32_t slot = g / RF_CAND_SHARDS;
          if (slot < fd.cap) lists[(size_t)(g % RF_CAND_SHARDS) * fd.cap + slot] = make_uint2(f_row[i], f_best[i]);
        }
        appended += (uint32_t)__popcll(m);
      }
      // rare: mark the query in the waves it cannot take from the lists
      while (incomplete) {
        const uint32_t sw = base + (uint32_t)lane + 64u * (uint32_t)(__ffs((int)incomplete) - 1);
        incomplete &= incomplete - 1u;
        const unsigned long long old = atomicOr(&fd.rmask[sw], 1ull << qi);
        if (old == 0ull && sw < fd.n_samp) {
          const uint32_t nb = (fd.n_samp - sw + fd.W - 1u) / fd.W;
          const uint32_t at = atomicAdd(fd.rcnt, nb);
          for (uint32_t j = 0; j < nb; ++j)
            if (at + j < (uint32_t)RF_FOLD_BLOCKS) fd.rlist[at + j] = (sw + j * fd.W) * fd.bstride;
        }
      }
    }
  }
  if (lane < RF_CAND_SHARDS)
    cand_cnt[qi * RF_CAND_SHARDS + lane] = (give_up && lane == 0) ? (uint32_t)RF_SHARD_CAP + 1u
                                                                 : (appended + RF_CAND_SHARDS - 1u - lane) / RF_CAND_SHARDS;
}

// The threshold of a sweep with per-row weights: pmax holds maxima of w32[row] * score,
// which lie within eps_w = 2 eps of the fp64 decayed scores, so thr = m_k - 2 eps_w, and eps_w goes to
// eps_out for the merge.  k_threshold's selection of the k-th partition maximum, without a fold, SQ8
// or a band (a kernel of its own, so that k_threshold stays what it is).
__global__ void __launch_bounds__(64) k_threshold_weighted(const _Float16* __restrict__ q, int B, int dim,
                                                           int k, const float* __restrict__ pmax, int P,
                                                           const uint32_t* __restrict__ max_norm2,
                                                           float* __restrict__ thr, float* __restrict__ eps_out,
                                                           uint32_t* __restrict__ cand_cnt) {
  const int qi = blockIdx.x;
  const int lane = threadIdx.x;
  const float eps_w = 2.f * query_eps(q, qi, B, dim, lane, max_norm2);
  float t;
  if (qi >= B) {
    t = INFINITY;
  } else if (P <= 0) {
    t = -INFINITY;
  } else {
    float v[RF_SAMPLE_WGS / 64];
#pragma unroll
    for (int i = 0; i < RF_SAMPLE_WGS / 64; ++i) {
      const int j = lane + 64 * i;
      v[i] = (j < P) ? pmax[(size_t)qi * P + j] : -INFINITY;
    }
    float kth = -INFINITY;
    for (int r = 0; r < k; ++r) {
      float m = v[0];
#pragma unroll
      for (int i = 1; i < RF_SAMPLE_WGS / 64; ++i) m = fmaxf(m, v[i]);
      const float wm = wave_max_f(m);
      kth = wm;
      if (wm == -INFINITY) break;
      const int winner = __ffsll((long long)__ballot(m == wm)) - 1;
      if (lane == winner) {
        bool done = false;
#pragma unroll
        for (int i = 0; i < RF_SAMPLE_WGS / 64; ++i)
          if (!done && v[i] == wm) {
            v[i] = -INFINITY;
            done = true;
          }
      }
    }
    t = (kth == -INFINITY) ? -INFINITY : kth - 2.f * eps_w;
  }
  if (lane == 0) {
    thr[qi] = t;
    eps_out[qi] = eps_w;
  }
  if (lane < RF_CAND_SHARDS) cand_cnt[qi * RF_CAND_SHARDS + lane] = 0u;
}

// ---- candidate merge + exact rescoring --------------------------------------------
// One workgroup per query:
//   1. find the k-th largest candidate by (MFMA score, row): rank counting over
//      LDS-broadcast keys when there are <= 1024 candidates (the usual ~150-300),
//      extraction rounds otherwise (small corpora, where every row is a candidate);
//   2. compact the rescoring set R = {MFMA score >= kth - 2 eps} (k + a few rows);
//   3. stage the rows of R in LDS with all 256 threads (one HBM latency instead
//      of one per 16-byte chunk), then one thread per row runs the fp64 chain;
//   4. rank R by (exact desc, row asc) and write the top-k.
#define MERGE_PER_THREAD (RF_CAND_CAP / MERGE_THREADS)
#define MERGE_RANK_MAX 1024

static size_t merge_lds_bytes(int dim) {
  return (size_t)MERGE_RANK_MAX * 8 + (MERGE_THREADS / 64) * RF_MAX_K * 8 + RF_RESCORE_CAP * 8 +
         RF_RESCORE_CAP * 4 + 64 + (size_t)dim * 8 + (size_t)MERGE_STAGE_ROWS * (dim * 2 + 16);
}

// BAND (range search): the candidates reach up to hi + eps.  The k-th largest is taken among
// those with score <= hi - eps only (rows that are certainly not above the band; fewer than k of
// them: no cut), R keeps everything at or above the cut -- the fringe (hi - eps, hi + eps]
// included --, and after the fp64 chains every row of R with a > hi or a <= lo is dropped before
// the ranking.
// AFTER (search-after, always with BAND): the ceiling of the k-th selection is the
// strict per-query one (rf_after_ceiling: a key at or below it is eligible whatever its row), and a
// row of R also leaves unless it ranks strictly after the bound (after_s[qi], after_r[qi]) by the
// fp64 (score, id) rule.
// WEIGHTED (per-row weights, never with BAND): the candidates' score bits are those of
// w32[row] * score and eps_in holds eps_w, so R is the near-tie set of the weighted order.  After the
// fp64 chains decayed = w64[row] * s is formed as ONE multiplication and R is ranked by (decayed
// desc, s desc, row asc); `exact` receives decayed and base_out s.
template <bool BAND, bool AFTER, bool WEIGHTED = false>
__device__ __forceinline__ void merge_body(
    unsigned char* lds, const _Float16* __restrict__ q, int dim, int KS, const uint4* __restrict__ tiles, int k,
    int64_t id_base, const uint32_t* __restrict__ cand_cnt, const uint2* __restrict__ cand,
    uint32_t cap, const float* __restrict__ eps_in, float* __restrict__ scores,
    int64_t* __restrict__ ids, double* __restrict__ exact, uint32_t* __restrict__ flags,
    uint32_t* __restrict__ cand_cnt_rw, uint32_t n_rows, int keep_cnt, rf_band bd,
    const double* __restrict__ after_s, const int64_t* __restrict__ after_r,
    const double* __restrict__ w64 = nullptr, double* __restrict__ base_out = nullptr) {
  static_assert(!AFTER || BAND, "a search-after merge is a band merge");
  static_assert(!WEIGHTED || !BAND, "the weighted merge has no band form");
  unsigned long long* skeys = (unsigned long long*)lds;                       // [1024]
  unsigned long long* wtop = skeys + MERGE_RANK_MAX;                          // [4][RF_MAX_K]
  double* r_exact = (double*)(wtop + (MERGE_THREADS / 64) * RF_MAX_K);        // [RESCORE_CAP]
  uint32_t* r_row = (uint32_t*)(r_exact + RF_RESCORE_CAP);                    // [RESCORE_CAP]
  uint32_t* r_cnt = r_row + RF_RESCORE_CAP;                                   // misc: 16 words
  float* t_cut = (float*)(r_cnt + 1);
  uint32_t* n_elig = r_cnt + 2;                                               // BAND: candidates <= hi - eps
  uint32_t* n_band = r_cnt + 3;                                               // BAND: rows of R inside the band
  double* qd = (double*)(r_cnt + 16);                                         // [dim]
  uint4* srows = (uint4*)(qd + dim);                                          // [32][2 KS + 1]

  const int qi = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  bool bad_row = false;
  CandLists L;
  uint32_t fl = cand_lists(L, cand_cnt, cand, cap, qi);
  const uint32_t c = L.c;
  const int kk = (uint32_t)k < c ? k : (int)c;
  bool have_cut = kk > 0 && (uint32_t)k <= c;  // fewer than k candidates: rescore all
  const float eps2 = 2.f * eps_in[qi];
  // BAND: a key takes part in the k-th selection only if its score is <= hs
  const double bound_s = AFTER ? after_s[qi] : 0.0;
  const int64_t bound_r = AFTER ? after_r[qi] - id_base : 0;
  const float hs = AFTER  ? rf_band_floor(rf_after_ceiling(bd.hi, bound_s, true) - (double)eps_in[qi])
                   : BAND ? rf_band_floor(bd.hi - (double)eps_in[qi])
                          : INFINITY;
  if (tid == 0) {
    *r_cnt = 0u;
    *t_cut = -INFINITY;
    if (BAND) *n_elig = *n_band = 0u;
  }
  if (BAND) __syncthreads();
  // counts the eligible keys of the block; every thread calls it once
  auto count_eligible = [&](uint32_t mine) -> uint32_t {
    if (mine) atomicAdd(n_elig, mine);
    __syncthreads();
    return *n_elig;
  };
  for (int d = tid; d < dim; d += MERGE_THREADS) ((_Float16*)qd)[d] = q[(size_t)qi * dim + d];

  if (c <= MERGE_RANK_MAX) {
    // ---- pass 1a: rank counting ------------------------------------------------
    unsigned long long key[MERGE_RANK_MAX / MERGE_THREADS];
#pragma unroll
    for (int i = 0; i < MERGE_RANK_MAX / MERGE_THREADS; ++i) {
      const uint32_t idx = (uint32_t)tid + MERGE_THREADS * i;
      key[i] = idx < c ? cand_key(cand_at(L, idx, n_rows, bad_row)) : 0ull;
      skeys[idx] = (BAND && !(key_score(key[i]) <= hs)) ? 0ull : key[i];  // zero padding never outranks a real key
    }
    if (BAND) {
      uint32_t mine = 0u;
#pragma unroll
      for (int i = 0; i < MERGE_RANK_MAX / MERGE_THREADS; ++i)
        mine += (key[i] != 0ull && key_score(key[i]) <= hs) ? 1u : 0u;
      have_cut = count_eligible(mine) >= (uint32_t)k;
    }
    __syncthreads();
    if (have_cut) {
      uint32_t rank[MERGE_RANK_MAX / MERGE_THREADS];
#pragma unroll
      for (int i = 0; i < MERGE_RANK_MAX / MERGE_THREADS; ++i) rank[i] = 0;
      for (uint32_t j = 0; j < c; j += 8) {
        unsigned long long o[8];  // same addresses in every lane: LDS broadcast, 8 in flight
#pragma unroll
        for (int u = 0; u < 8; ++u) o[u] = skeys[j + u];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int i = 0; i < MERGE_RANK_MAX / MERGE_THREADS; ++i) rank[i] += o[u] > key[i] ? 1u : 0u;
      }
#pragma unroll
      for (int i = 0; i < MERGE_RANK_MAX / MERGE_THREADS; ++i)
        if (key[i] != 0ull && rank[i] == (uint32_t)(kk - 1) && (!BAND || key_score(key[i]) <= hs))
          *t_cut = key_score(key[i]) - eps2;
    }
    __syncthreads();
    // ---- pass 2a: compact R from the LDS keys -----------------------------------
    const float cut = *t_cut;
#pragma unroll
    for (int i = 0; i < MERGE_RANK_MAX / MERGE_THREADS; ++i) {
      if (key[i] != 0ull && key_score(key[i]) >= cut) {
        const uint32_t slot = atomicAdd(r_cnt, 1u);
        if (slot < RF_RESCORE_CAP) r_row[slot] = key_row(key[i]);
      }
    }
  } else {
    // ---- pass 1b: extraction rounds (per wave, then across waves) ---------------
    unsigned long long key[MERGE_PER_THREAD];
#pragma unroll
    for (int i = 0; i < MERGE_PER_THREAD; ++i) {
      const uint32_t idx = (uint32_t)tid + MERGE_THREADS * i;
      key[i] = idx < c ? cand_key(cand_at(L, idx, n_rows, bad_row)) : 0ull;
      if (BAND && !(key_score(key[i]) <= hs)) key[i] = 0ull;
    }
    if (BAND) {
      uint32_t mine = 0u;
#pragma unroll
      for (int i = 0; i < MERGE_PER_THREAD; ++i) mine += key[i] != 0ull ? 1u : 0u;
      have_cut = count_eligible(mine) >= (uint32_t)k;
    }
    for (int r = 0; r < kk; ++r) {
      unsigned long long m = key[0];
#pragma unroll
      for (int i = 1; i < MERGE_PER_THREAD; ++i) m = key[i] > m ? key[i] : m;
      const unsigned long long wm = wave_max_u64(m);
      if (lane == 0) wtop[wave * RF_MAX_K + r] = wm;
      if (wm != 0ull && m == wm) {
#pragma unroll
        for (int i = 0; i < MERGE_PER_THREAD; ++i)
          if (key[i] == wm) key[i] = 0ull;
      }
    }
    __syncthreads();
    if (wave == 0) {
      constexpr int NV = (MERGE_THREADS / 64 * RF_MAX_K + 63) / 64;
      unsigned long long v[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int j = lane + 64 * i;  // j -> (wave j / kk, slot j % kk)
        v[i] = (kk > 0 && j < (MERGE_THREADS / 64) * kk) ? wtop[(j / kk) * RF_MAX_K + (j % kk)] : 0ull;
      }
      unsigned long long kth = 0ull;
      for (int r = 0; r < kk; ++r) {
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
      if (lane == 0 && have_cut) *t_cut = key_score(kth) - eps2;
    }
    __syncthreads();
    // ---- pass 2b: compact R from global ------------------------------------------
    const float cut = *t_cut;
    for (uint32_t idx = tid; idx < c; idx += MERGE_THREADS) {
      const uint2 e = cand_at(L, idx, n_rows, bad_row);
      if (__builtin_bit_cast(float, e.y) >= cut) {
        const uint32_t slot = atomicAdd(r_cnt, 1u);
        if (slot < RF_RESCORE_CAP) r_row[slot] = e.x;
      }
    }
  }
  __syncthreads();
  uint32_t R = *r_cnt;
  if (R > RF_RESCORE_CAP) {
    fl |= RF_FLAG_TIE_OVERFLOW;
    R = RF_RESCORE_CAP;
  }

  // ---- pass 3: exact fp64 scores, rows staged through LDS ---------------------------
  rescore_rows(r_row, R, tiles, KS, (const _Float16*)qd, srows, r_exact);   // (qd: the query row as fp16)

  // ---- pass 4: rank by (exact desc, row asc) and write --------------------------------
  uint32_t n_in = R;
  if (BAND) {
    // rows outside the band leave R: they rank after every row inside it (-inf < lo < a) and
    // are never written
    uint32_t mine = 0u;
    for (uint32_t i = tid; i < R; i += MERGE_THREADS) {
      const double s = r_exact[i];
      if (s > bd.lo && s <= bd.hi && (!AFTER || ranks_before(bound_s, bound_r, s, (int64_t)r_row[i]))) ++mine;
      else r_exact[i] = -INFINITY;
    }
    if (mine) atomicAdd(n_band, mine);
    __syncthreads();
    n_in = *n_band;
  }
  if constexpr (WEIGHTED) {
    // the key area of passes 1 and 2 is free from here on: the decayed scores of R
    double* r_dec = (double*)skeys;   // [RF_RESCORE_CAP] <= MERGE_RANK_MAX entries
    for (uint32_t i = tid; i < R; i += MERGE_THREADS) r_dec[i] = __dmul_rn(w64[r_row[i]], r_exact[i]);
    __syncthreads();
    for (uint32_t i = tid; i < R; i += MERGE_THREADS) {
      const double d = r_dec[i], s = r_exact[i];
      const uint32_t row = r_row[i];
      uint32_t rank = 0;
      for (uint32_t j = 0; j < R; ++j) {
        const double od = r_dec[j];
        rank += (od > d || (od == d && ranks_before(r_exact[j], r_row[j], s, row))) ? 1u : 0u;
      }
      if (rank < (uint32_t)k) {
        const size_t o = (size_t)qi * k + rank;
        scores[o] = (float)d;
        ids[o] = (int64_t)row + id_base;
        if (exact) exact[o] = d;
        if (base_out) base_out[o] = s;
      }
    }
  } else {
    for (uint32_t i = tid; i < R; i += MERGE_THREADS) {
      const double s = r_exact[i];
      const uint32_t row = r_row[i];
      if (BAND && s == -INFINITY) continue;
      uint32_t rank = 0;
      for (uint32_t j = 0; j < R; ++j) rank += ranks_before(r_exact[j], r_row[j], s, row) ? 1u : 0u;
      if (rank < (uint32_t)k) {
        const size_t o = (size_t)qi * k + rank;
        scores[o] = (float)s;
        ids[o] = (int64_t)row + id_base;
        if (exact) exact[o] = s;
      }
    }
  }
  const uint32_t filled = n_in < (uint32_t)k ? n_in : (uint32_t)k;
  for (uint32_t j = filled + tid; j < (uint32_t)k; j += MERGE_THREADS) {
    const size_t o = (size_t)qi * k + j;
    scores[o] = -INFINITY;
    ids[o] = -1;
    if (exact) exact[o] = -INFINITY;
    if (WEIGHTED && base_out) base_out[o] = -INFINITY;
  }
  if (flags && __syncthreads_or(bad_row ? 1 : 0)) fl |= RF_FLAG_CAND_OVERFLOW;
  if (tid == 0 && flags) flags[qi] = fl;
  // leave the counters zero (every thread of this workgroup read them before the barriers
  // above); k_threshold zeroes them again at the start of every search, so a search never
  // depends on what an earlier one -- or an error return mid-pipeline -- left behind
  if (tid < RF_CAND_SHARDS && !keep_cnt) cand_cnt_rw[qi * RF_CAND_SHARDS + tid] = 0u;
}

template <bool BAND>
__global__ void __launch_bounds__(MERGE_THREADS) k_merge(
    const _Float16* __restrict__ q, int dim, int KS, const uint4* __restrict__ tiles, int k,
    int64_t id_base, const uint32_t* __restrict__ cand_cnt, const uint2* __restrict__ cand,
    uint32_t cap, const float* __restrict__ eps_in, float* __restrict__ scores,
    int64_t* __restrict__ ids, double* __restrict__ exact, uint32_t* __restrict__ flags,
    uint32_t* __restrict__ cand_cnt_rw, uint32_t n_rows, int keep_cnt, rf_band bd) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  merge_body<BAND, false>(lds, q, dim, KS, tiles, k, id_base, cand_cnt, cand, cap, eps_in, scores, ids, exact, flags,
                          cand_cnt_rw, n_rows, keep_cnt, bd, nullptr, nullptr);
}

// (a kernel of its own, so that the arguments of the other two stay what they are)
__global__ void __launch_bounds__(MERGE_THREADS) k_merge_after(
    const _Float16* __restrict__ q, int dim, int KS, const uint4* __restrict__ tiles, int k,
    int64_t id_base, const uint32_t* __restrict__ cand_cnt, const uint2* __restrict__ cand,
    uint32_t cap, const float* __restrict__ eps_in, float* __restrict__ scores,
    int64_t* __restrict__ ids, double* __restrict__ exact, uint32_t* __restrict__ flags,
    uint32_t* __restrict__ cand_cnt_rw, uint32_t n_rows, rf_band bd,
    const double* __restrict__ after_s, const int64_t* __restrict__ after_r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  merge_body<true, true>(lds, q, dim, KS, tiles, k, id_base, cand_cnt, cand, cap, eps_in, scores, ids, exact, flags,
                         cand_cnt_rw, n_rows, 0, bd, after_s, after_r);
}
// (a kernel of its own, so that the names and arguments of the others stay what they are)
__global__ void __launch_bounds__(MERGE_THREADS) k_merge_weighted(
    const _Float16* __restrict__ q, int dim, int KS, const uint4* __restrict__ tiles, int k,
    int64_t id_base, const uint32_t* __restrict__ cand_cnt, const uint2* __restrict__ cand,
    uint32_t cap, const float* __restrict__ eps_in, float* __restrict__ scores,
    int64_t* __restrict__ ids, double* __restrict__ decayed, double* __restrict__ base,
    uint32_t* __restrict__ flags, uint32_t* __restrict__ cand_cnt_rw, uint32_t n_rows,
    const double* __restrict__ w64) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  merge_body<false, false, true>(lds, q, dim, KS, tiles, k, id_base, cand_cnt, cand, cap, eps_in, scores, ids, decayed,
                                 flags, cand_cnt_rw, n_rows, 0, rf_band{}, nullptr, nullptr, w64, base);
}

// ---- exhaustive exact path ----------------------------------------------------------
// Workgroup-level running top-k list (sorted, in LDS) updated 256 entries at a
// time by rank counting.  Used for queries the fused path could not prove
// (flags != 0) and as an on-device cross-check in the tests.
#define EX_THREADS 256
struct ExList {
  double s[RF_MAX_K];
  int64_t r[RF_MAX_K];
  int n;
};

__device__ void exlist_update(ExList* L, double* t_s, int64_t* t_r, int* t_n, int k, double s,
                              int64_t row, bool valid, int tid) {
  // does my entry beat the current k-th?
  bool pass = valid;
  if (valid && L->n >= k) pass = ranks_before(s, row, L->s[k - 1], L->r[k - 1]);
  if (__syncthreads_or(pass ? 1 : 0) == 0) return;
  if (tid == 0) *t_n = L->n;
  __syncthreads();
  if (tid < L->n) {
    t_s[tid] = L->s[tid];
    t_r[tid] = L->r[tid];
  }
  if (pass) {
    const int slot = atomicAdd(t_n, 1);
    t_s[slot] = s;
    t_r[slot] = row;
  }
  __syncthreads();
  const int m = *t_n;
  for (int i = tid; i < m; i += EX_THREADS) {
    const double si = t_s[i];
    const int64_t ri = t_r[i];
    int rank = 0;
    for (int j = 0; j < m; ++j) rank += ranks_before(t_s[j], t_r[j], si, ri) ? 1 : 0;
    if (rank < k) {
      L->s[rank] = si;
      L->r[rank] = ri;
    }
  }
  if (tid == 0) L->n = m < k ? m : k;
  __syncthreads();
}

__global__ void __launch_bounds__(EX_THREADS) k_exhaustive_scan(
    const _Float16* __restrict__ q, int dim, int KS, const uint4* __restrict__ tiles, int64_t n_rows,
    int k, double* __restrict__ out_s, int64_t* __restrict__ out_r,
    const double* __restrict__ after_s, const int64_t* __restrict__ after_r, int64_t id_base) {
  __shared__ ExList L;
  __shared__ double t_s[RF_MAX_K + EX_THREADS];
  __shared__ int64_t t_r[RF_MAX_K + EX_THREADS];
  __shared__ int t_n;
  const int tid = threadIdx.x;
  const int qi = blockIdx.y;
  if (tid == 0) L.n = 0;
  __syncthreads();
  const _Float16* qrow = q + (size_t)qi * dim;
  // paging: only rows ranked strictly AFTER (after_s, after_r) are eligible
  const bool paged = after_s != nullptr;
  const double bs = paged ? after_s[qi] : 0.0;
  const int64_t br = paged ? after_r[qi] - id_base : 0;
  const int64_t step = (int64_t)gridDim.x * EX_THREADS;
  for (int64_t base = (int64_t)blockIdx.x * EX_THREADS; base < n_rows; base += step) {
    const int64_t row = base + tid;
    bool valid = row < n_rows;
    const double s = valid ? exact_dot(qrow, tiles, row, KS) : 0.0;
    if (paged) valid = valid && ranks_before(bs, br, s, row);
    exlist_update(&L, t_s, t_r, &t_n, k, s, row, valid, tid);
  }
  const size_t o = ((size_t)qi * gridDim.x + blockIdx.x) * RF_MAX_K;
  if (tid < RF_MAX_K) {
    out_s[o + tid] = tid < L.n ? L.s[tid] : -INFINITY;
    out_r[o + tid] = tid < L.n ? L.r[tid] : -1;
  }
}

// k_exhaustive_scan for filtered search: a row whose filter bit is clear is not eligible.
// (A separate kernel rather than a nullable argument, so the unfiltered kernel's code is unchanged.)
__global__ void __launch_bounds__(EX_THREADS) k_exhaustive_scan_masked(
    const _Float16* __restrict__ q, int dim, int KS, const uint4* __restrict__ tiles, int64_t n_rows,
    int k, double* __restrict__ out_s, int64_t* __restrict__ out_r,
    const double* __restrict__ after_s, const int64_t* __restrict__ after_r, int64_t id_base,
    const uint32_t* __restrict__ mask) {
  __shared__ ExList L;
  __shared__ double t_s[RF_MAX_K + EX_THREADS];
  __shared__ int64_t t_r[RF_MAX_K + EX_THREADS];
  __shared__ int t_n;
  const int tid = threadIdx.x;
  const int qi = blockIdx.y;
  if (tid == 0) L.n = 0;
  __syncthreads();
  const _Float16* qrow = q + (size_t)qi * dim;
  // paging: only rows ranked strictly AFTER (after_s, after_r) are eligible
  const bool paged = after_s != nullptr;
  const double bs = paged ? after_s[qi] : 0.0;
  const int64_t br = paged ? after_r[qi] - id_base : 0;
  const int64_t step = (int64_t)gridDim.x * EX_THREADS;
  for (int64_t base = (int64_t)blockIdx.x * EX_THREADS; base < n_rows; base += step) {
    const int64_t row = base + tid;
    bool valid = row < n_rows && ((mask[row >> 5] >> (row & 31)) & 1u) != 0u;
    const double s = valid ? exact_dot(qrow, tiles, row, KS) : 0.0;
    if (paged) valid = valid && ranks_before(bs, br, s, row);
    exlist_update(&L, t_s, t_r, &t_n, k, s, row, valid, tid);
  }
  const size_t o = ((size_t)qi * gridDim.x + blockIdx.x) * RF_MAX_K;
  if (tid < RF_MAX_K) {
    out_s[o + tid] = tid < L.n ? L.s[tid] : -INFINITY;
    out_r[o + tid] = tid < L.n ? L.r[tid] : -1;
  }
}

// The exhaustive scan of range search: a row is eligible only if lo < a <= hi on its fp64 score
// (and, MASKED, if its filter bit is set), beside the paging bound.  Kernels of their own for the
// same reason as above.
template <bool MASKED>
__global__ void __launch_bounds__(EX_THREADS) k_exhaustive_scan_band(
    const _Float16* __restrict__ q, int dim, int KS, const uint4* __restrict__ tiles, int64_t n_rows,
    int k, double* __restrict__ out_s, int64_t* __restrict__ out_r,
    const double* __restrict__ after_s, const int64_t* __restrict__ after_r, int64_t id_base,
    const uint32_t* __restrict__ mask, rf_band bd) {
  __shared__ ExList L;
  __shared__ double t_s[RF_MAX_K + EX_THREADS];
  __shared__ int64_t t_r[RF_MAX_K + EX_THREADS];
  __shared__ int t_n;
  const int tid = threadIdx.x;
  const int qi = blockIdx.y;
  if (tid == 0) L.n = 0;
  __syncthreads();
  const _Float16* qrow = q + (size_t)qi * dim;
  const bool paged = after_s != nullptr;
  const double bs = paged ? after_s[qi] : 0.0;
  const int64_t br = paged ? after_r[qi] - id_base : 0;
  const int64_t step = (int64_t)gridDim.x * EX_THREADS;
  for (int64_t base = (int64_t)blockIdx.x * EX_THREADS; base < n_rows; base += step) {
    const int64_t row = base + tid;
    bool valid = row < n_rows;
    if (MASKED) valid = valid && ((mask[row >> 5] >> (row & 31)) & 1u) != 0u;
    const double s = valid ? exact_dot(qrow, tiles, row, KS) : 0.0;
    valid = valid && s > bd.lo && s <= bd.hi;
    if (paged) valid = valid && ranks_before(bs, br, s, row);
    exlist_update(&L, t_s, t_r, &t_n, k, s, row, valid, tid);
  }
  const size_t o = ((size_t)qi * gridDim.x + blockIdx.x) * RF_MAX_K;
  if (tid < RF_MAX_K) {
    out_s[o + tid] = tid < L.n ? L.s[tid] : -INFINITY;
    out_r[o + tid] = tid < L.n ? L.r[tid] : -1;
  }
}

__global__ void __launch_bounds__(EX_THREADS) k_exhaustive_final(
    const double* __restrict__ in_s, const int64_t* __restrict__ in_r, int lists, int k,
    int64_t id_base, float* __restrict__ scores, int64_t* __restrict__ ids,
    double* __restrict__ exact) {
  __shared__ ExList L;
  __shared__ double t_s[RF_MAX_K + EX_THREADS];
  __shared__ int64_t t_r[RF_MAX_K + EX_THREADS];
  __shared__ int t_n;
  const int tid = threadIdx.x;
  const int qi = blockIdx.x;
  if (tid == 0) L.n = 0;
  __syncthreads();
  const size_t base = (size_t)qi * lists * RF_MAX_K;
  const int total = lists * RF_MAX_K;
  for (int b = 0; b < total; b += EX_THREADS) {
    const int i = b + tid;
    const bool valid = i < total && in_r[base + i] >= 0;
    const double s = valid ? in_s[base + i] : 0.0;
    const int64_t row = valid ? in_r[base + i] : 0;
    exlist_update(&L, t_s, t_r, &t_n, k, s, row, valid, tid);
  }
  for (int j = tid; j < k; j += EX_THREADS) {
    const size_t o = (size_t)qi * k + j;
    if (j < L.n) {
      scores[o] = (float)L.s[j];
      ids[o] = L.r[j] + id_base;
      if (exact) exact[o] = L.s[j];
    } else {
      scores[o] = -INFINITY;
      ids[o] = -1;
      if (exact) exact[o] = -INFINITY;
    }
  }
}

// ---- exhaustive path with per-row weights ------------------------------------
// The running top-k list of above with one more key: entries rank by (decayed desc, s desc, row
// asc), decayed = w64[row] * s as one fp64 multiplication.
struct ExListW {
  double d[RF_MAX_K];
  double s[RF_MAX_K];
  int64_t r[RF_MAX_K];
  int n;
};
__device__ __forceinline__ bool ranks_before_w(double d1, double s1, int64_t r1, double d2, double s2, int64_t r2) {
  return d1 > d2 || (d1 == d2 && ranks_before(s1, r1, s2, r2));
}

__device__ void exlist_update_w(ExListW* L, double* t_d, double* t_s, int64_t* t_r, int* t_n, int k, double d,
                                double s, int64_t row, bool valid, int tid) {
  bool pass = valid;
  if (valid && L->n >= k) pass = ranks_before_w(d, s, row, L->d[k - 1], L->s[k - 1], L->r[k - 1]);
  if (__syncthreads_or(pass ? 1 : 0) == 0) return;
  if (tid == 0) *t_n = L->n;
  __syncthreads();
  if (tid < L->n) {
    t_d[tid] = L->d[tid];
    t_s[tid] = L->s[tid];
    t_r[tid] = L->r[tid];
  }
  if (pass) {
    const int slot = atomicAdd(t_n, 1);   // < RF_MAX_K + EX_THREADS: the list and one entry per thread
    t_d[slot] = d;
    t_s[slot] = s;
    t_r[slot] = row;
  }
  __syncthreads();
  const int m = *t_n;
  for (int i = tid; i < m; i += EX_THREADS) {
    const double di = t_d[i], si = t_s[i];
    const int64_t ri = t_r[i];
    int rank = 0;
    for (int j = 0; j < m; ++j) rank += ranks_before_w(t_d[j], t_s[j], t_r[j], di, si, ri) ? 1 : 0;
    if (rank < k) {
      L->d[rank] = di;
      L->s[rank] = si;
      L->r[rank] = ri;
    }
  }
  if (tid == 0) L->n = m < k ? m : k;
  __syncthreads();
}

// mask: nullptr = every row
__global__ void __launch_bounds__(EX_THREADS) k_exhaustive_scan_weighted(
    const _Float16* __restrict__ q, int dim, int KS, const uint4* __restrict__ tiles, int64_t n_rows,
    int k, double* __restrict__ out_d, double* __restrict__ out_s, int64_t* __restrict__ out_r,
    const uint32_t* __restrict__ mask, const double* __restrict__ w64) {
  __shared__ ExListW L;
  __shared__ double t_d[RF_MAX_K + EX_THREADS];
  __shared__ double t_s[RF_MAX_K + EX_THREADS];
  __shared__ int64_t t_r[RF_MAX_K + EX_THREADS];
  __shared__ int t_n;
  const int tid = threadIdx.x;
  const int qi = blockIdx.y;
  if (tid == 0) L.n = 0;
  __syncthreads();
  const _Float16* qrow = q + (size_t)qi * dim;
  const int64_t step = (int64_t)gridDim.x * EX_THREADS;
  for (int64_t base = (int64_t)blockIdx.x * EX_THREADS; base < n_rows; base += step) {
    const int64_t row = base + tid;
    const bool valid = row < n_rows && (!mask || ((mask[row >> 5] >> (row & 31)) & 1u) != 0u);
    const double s = valid ? exact_dot(qrow, tiles, row, KS) : 0.0;
    const double d = valid ? __dmul_rn(w64[row], s) : 0.0;
    exlist_update_w(&L, t_d, t_s, t_r, &t_n, k, d, s, row, valid, tid);
  }
  const size_t o = ((size_t)qi * gridDim.x + blockIdx.x) * RF_MAX_K;
  if (tid < RF_MAX_K) {
    out_d[o + tid] = tid < L.n ? L.d[tid] : -INFINITY;
    out_s[o + tid] = tid < L.n ? L.s[tid] : -INFINITY;
    out_r[o + tid] = tid < L.n ? L.r[tid] : -1;
  }
}

__global__ void __launch_bounds__(EX_THREADS) k_exhaustive_final_weighted(
    const double* __restrict__ in_d, const double* __restrict__ in_s, const int64_t* __restrict__ in_r, int lists,
    int k, int64_t id_base, float* __restrict__ scores, int64_t* __restrict__ ids, double* __restrict__ decayed,
    double* __restrict__ base_out) {
  __shared__ ExListW L;
  __shared__ double t_d[RF_MAX_K + EX_THREADS];
  __shared__ double t_s[RF_MAX_K + EX_THREADS];
  __shared__ int64_t t_r[RF_MAX_K + EX_THREADS];
  __shared__ int t_n;
  const int tid = threadIdx.x;
  const int qi = blockIdx.x;
  if (tid == 0) L.n = 0;
  __syncthreads();
  const size_t base = (size_t)qi * lists * RF_MAX_K;
  const int total = lists * RF_MAX_K;
  for (int b = 0; b < total; b += EX_THREADS) {
    const int i = b + tid;
    const bool valid = i < total && in_r[base + i] >= 0;
    exlist_update_w(&L, t_d, t_s, t_r, &t_n, k, valid ? in_d[base + i] : 0.0, valid ? in_s[base + i] : 0.0,
                    valid ? in_r[base + i] : 0, valid, tid);
  }
  for (int j = tid; j < k; j += EX_THREADS) {
    const size_t o = (size_t)qi * k + j;
    const bool have = j < L.n;
    scores[o] = have ? (float)L.d[j] : -INFINITY;
    ids[o] = have ? L.r[j] + id_base : -1;
    if (decayed) decayed[o] = have ? L.d[j] : -INFINITY;
    if (base_out) base_out[o] = have ? L.s[j] : -INFINITY;
  }
}

// ---- cross-shard merge ---------------------------------------------------------------
// in [W][B][k] (exact fp64, global id) -> out [B][k].  Ids are global and unique,
// so ranking by (score desc, id asc) reproduces the single-device order bit for bit.
__global__ void __launch_bounds__(EX_THREADS) k_merge_shards(
    const double* __restrict__ in_s, const int64_t* __restrict__ in_r, size_t sstride,
    int W, int B, int k, float* __restrict__ scores, int64_t* __restrict__ ids,
    const uint32_t* __restrict__ flags_in, size_t fstride, uint32_t* __restrict__ flags_out) {
  // entry (shard w, query qi, rank j) sits at w * sstride + qi * k + j in both arrays; shard w's
  // per-query exactness flags (optional) at flags_in[w * fstride + qi]: the merged answer of a
  // query is proven exact only if EVERY shard's local answer was, so the output flag is their OR
  const int qi = blockIdx.x;
  const int tid = threadIdx.x;
  const int m = W * k;
  const size_t qoff = (size_t)qi * k;
  const size_t ooff = (size_t)qi * k;
  if (flags_out && tid == 0) {
    uint32_t f = 0u;
    if (flags_in)
      for (int w = 0; w < W; ++w) f |= flags_in[(size_t)w * fstride + qi];
    flags_out[qi] = f;
  }
  for (int i = tid; i < m; i += EX_THREADS) {
    const int w = i / k, j = i % k;
    const size_t src = (size_t)w * sstride + qoff + j;
    const int64_t ri = in_r[src];
    if (ri < 0) continue;
    const double si = in_s[src];
    int rank = 0;
    for (int i2 = 0; i2 < m; ++i2) {
      const size_t s2 = (size_t)(i2 / k) * sstride + qoff + (i2 % k);
      const int64_t r2 = in_r[s2];
      if (r2 >= 0 && ranks_before(in_s[s2], r2, si, ri)) ++rank;
    }
    if (rank < k) {
      scores[ooff + rank] = (float)si;
      ids[ooff + rank] = ri;
    }
  }
  // number of valid entries decides how many tail slots stay empty
  __shared__ int n_valid;
  if (tid == 0) n_valid = 0;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < m; i += EX_THREADS)
    mine += in_r[(size_t)(i / k) * sstride + qoff + (i % k)] >= 0 ? 1 : 0;
  if (mine) atomicAdd(&n_valid, mine);
  __syncthreads();
  for (int j = n_valid + tid; j < k; j += EX_THREADS) {
    scores[ooff + j] = -INFINITY;
    ids[ooff + j] = -1;
  }
}

// ---- host side --------------------------------------------------------------------------
int rf_launch_threshold(const rf_index* ix, const void* q, int B, int k, int P,
                        const rf_workspace& ws, hipStream_t st, const rf_fold* fold,
                        const rf_sq8_ws* sq8, const rf_band* band) {
  ThrFold fd{};
  ThrSq8 sq{};
  if (sq8) {
    sq.nq = sq8->nq;
    sq.fq = sq8->fq;
    sq.mx = ix->sq8_max;
  }
  if (fold && fold->n_samp > 0u && P > 0 && B <= RF_QCHUNK) {
    fd.lists = ws.fold;
    fd.rmask = ws.rmask;
    fd.rlist = ws.rlist;
    fd.rcnt = ws.rcnt;
    fd.cand = ws.cand;
    fd.cap = RF_SHARD_CAP;
    fd.n_samp = fold->n_samp;
    fd.bstride = fold->bstride;
    fd.W = fold->W;
    fd.force = rf_knob_fold_dbg & 1;
  }
  // one wave per query slot of the sweep (64, or up to RF_QWIDE for a wide sweep)
  const dim3 grid(B > RF_QCHUNK ? RF_QWIDE : RF_QCHUNK);
  if (band)
    hipLaunchKernelGGL(k_threshold<true>, grid, dim3(64), 0, st, (const _Float16*)q, B, ix->dim, k, ws.pmax, P,
                       ix->max_norm2, ws.thr, ws.eps, ws.cand_cnt, fd, sq, *band);
  else
    hipLaunchKernelGGL(k_threshold<false>, grid, dim3(64), 0, st, (const _Float16*)q, B, ix->dim, k, ws.pmax, P,
                       ix->max_norm2, ws.thr, ws.eps, ws.cand_cnt, fd, sq, rf_band{});
  RF_HIP(hipGetLastError());
  return RF_OK;
}

int rf_launch_threshold_weighted(const rf_index* ix, const void* q, int B, int k, int P, const rf_workspace& ws,
                                 hipStream_t st) {
  hipLaunchKernelGGL(k_threshold_weighted, dim3(RF_QCHUNK), dim3(64), 0, st, (const _Float16*)q, B, ix->dim, k, ws.pmax,
                     P, ix->max_norm2, ws.thr, ws.eps, ws.cand_cnt);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

int rf_launch_merge_weighted(const rf_index* ix, const void* q, int B, int k, int64_t id_base, const rf_workspace& ws,
                             const double* w64, float* scores, int64_t* ids, double* decayed, double* base,
                             uint32_t* flags, hipStream_t st) {
  const size_t lds = merge_lds_bytes(ix->dim);
  static rf_lds_attr lds_attr;
  RF_HIP(rf_ensure_lds(lds_attr, (const void*)k_merge_weighted, lds));
  hipLaunchKernelGGL(k_merge_weighted, dim3(B), dim3(MERGE_THREADS), lds, st, (const _Float16*)q, ix->dim, ix->KS,
                     ix->tiles, k, id_base, ws.cand_cnt, ws.cand, (uint32_t)RF_SHARD_CAP, ws.eps, scores, ids, decayed,
                     base, flags, ws.cand_cnt, (uint32_t)ix->size, w64);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

int rf_launch_exhaustive_weighted(const rf_index* ix, const void* q, int B, int k, int64_t id_base,
                                  const rf_workspace& ws, const double* w64, float* scores, int64_t* ids,
                                  double* decayed, double* base, hipStream_t st, const uint32_t* mask) {
  const int64_t need = (ix->size + EX_THREADS - 1) / EX_THREADS;
  const int lists = (int)(need < RF_EX_WGS ? (need < 1 ? 1 : need) : RF_EX_WGS);
  // the third list array, the plain scores: the candidate area, which this path does not use otherwise
  // (RF_QCHUNK * RF_EX_WGS * RF_MAX_K doubles = 8 MiB of its 32)
  static_assert((size_t)RF_QCHUNK * RF_EX_WGS * RF_MAX_K * sizeof(double) <=
                    (size_t)RF_QWIDE * RF_CAND_SHARDS * RF_SHARD_CAP * sizeof(uint2),
                "the plain scores of the weighted exhaustive lists fit the candidate area");
  double* ex_base = (double*)ws.cand;
  hipLaunchKernelGGL(k_exhaustive_scan_weighted, dim3(lists, B), dim3(EX_THREADS), 0, st, (const _Float16*)q, ix->dim,
                     ix->KS, ix->tiles, ix->size, k, ws.ex_score, ex_base, ws.ex_row, mask, w64);
  hipLaunchKernelGGL(k_exhaustive_final_weighted, dim3(B), dim3(EX_THREADS), 0, st, ws.ex_score, ex_base, ws.ex_row,
                     lists, k, id_base, scores, ids, decayed, base);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

int rf_launch_band_eps(const rf_index* ix, const void* q, int B, const rf_workspace& ws, hipStream_t st) {
  // every query slot of the 64-query sweep: the sample pass reads the eps of all 64 lanes
  hipLaunchKernelGGL(k_band_eps, dim3(RF_QCHUNK), dim3(64), 0, st, (const _Float16*)q, B, ix->dim, ix->max_norm2,
                     ws.eps);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

int rf_launch_merge(const rf_index* ix, const void* q, int B, int k, int64_t id_base,
                    const rf_workspace& ws, float* scores, int64_t* ids, double* exact,
                    uint32_t* flags, hipStream_t st, const rf_band* band, const rf_after* after) {
  const size_t lds = merge_lds_bytes(ix->dim);
  static rf_lds_attr lds_attr, lds_attr_band, lds_attr_after;
  if (band && after) {
    RF_HIP(rf_ensure_lds(lds_attr_after, (const void*)k_merge_after, lds));
    hipLaunchKernelGGL(k_merge_after, dim3(B), dim3(MERGE_THREADS), lds, st, (const _Float16*)q, ix->dim,
                       ix->KS, ix->tiles, k, id_base, ws.cand_cnt, ws.cand, (uint32_t)RF_SHARD_CAP,
                       ws.eps, scores, ids, exact, flags, ws.cand_cnt, (uint32_t)ix->size, *band,
                       after->score, after->id);
  } else if (band) {
    RF_HIP(rf_ensure_lds(lds_attr_band, (const void*)k_merge<true>, lds));
    hipLaunchKernelGGL(k_merge<true>, dim3(B), dim3(MERGE_THREADS), lds, st, (const _Float16*)q, ix->dim,
                       ix->KS, ix->tiles, k, id_base, ws.cand_cnt, ws.cand, (uint32_t)RF_SHARD_CAP,
                       ws.eps, scores, ids, exact, flags, ws.cand_cnt, (uint32_t)ix->size, 0, *band);
  } else {
    RF_HIP(rf_ensure_lds(lds_attr, (const void*)k_merge<false>, lds));
    hipLaunchKernelGGL(k_merge<false>, dim3(B), dim3(MERGE_THREADS), lds, st, (const _Float16*)q, ix->dim,
                       ix->KS, ix->tiles, k, id_base, ws.cand_cnt, ws.cand, (uint32_t)RF_SHARD_CAP,
                       ws.eps, scores, ids, exact, flags, ws.cand_cnt, (uint32_t)ix->size,
                       (rf_knob_fold_dbg & 2) ? 1 : 0, rf_band{});
  }
  RF_HIP(hipGetLastError());
  return RF_OK;
}

int rf_launch_exhaustive(const rf_index* ix, const void* q, int B, int k, int64_t id_base,
                         const rf_workspace& ws, float* scores, int64_t* ids, double* exact,
                         const double* after_s, const int64_t* after_r, hipStream_t st,
                         const uint32_t* mask, const rf_band* band) {
  int64_t need = (ix->size + EX_THREADS - 1) / EX_THREADS;
  int lists = (int)(need < RF_EX_WGS ? (need < 1 ? 1 : need) : RF_EX_WGS);
  if (band && mask)
    hipLaunchKernelGGL(k_exhaustive_scan_band<true>, dim3(lists, B), dim3(EX_THREADS), 0, st,
                       (const _Float16*)q, ix->dim, ix->KS, ix->tiles, ix->size, k, ws.ex_score,
                       ws.ex_row, after_s, after_r, id_base, mask, *band);
  else if (band)
    hipLaunchKernelGGL(k_exhaustive_scan_band<false>, dim3(lists, B), dim3(EX_THREADS), 0, st,
                       (const _Float16*)q, ix->dim, ix->KS, ix->tiles, ix->size, k, ws.ex_score,
                       ws.ex_row, after_s, after_r, id_base, (const uint32_t*)nullptr, *band);
  else if (mask)
    hipLaunchKernelGGL(k_exhaustive_scan_masked, dim3(lists, B), dim3(EX_THREADS), 0, st,
                       (const _Float16*)q, ix->dim, ix->KS, ix->tiles, ix->size, k, ws.ex_score,
                       ws.ex_row, after_s, after_r, id_base, mask);
  else
    hipLaunchKernelGGL(k_exhaustive_scan, dim3(lists, B), dim3(EX_THREADS), 0, st,
                       (const _Float16*)q, ix->dim, ix->KS, ix->tiles, ix->size, k, ws.ex_score,
                       ws.ex_row, after_s, after_r, id_base);
  hipLaunchKernelGGL(k_exhaustive_final, dim3(B), dim3(EX_THREADS), 0, st, ws.ex_score, ws.ex_row,
                     lists, k, id_base, scores, ids, exact);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

int rf_launch_merge_shards(const double* exact, const int64_t* ids, size_t shard_stride, int W, int B, int k,
                           float* scores_out, int64_t* ids_out, const uint32_t* flags_in, size_t flag_stride,
                           uint32_t* flags_out, hipStream_t st) {
  hipLaunchKernelGGL(k_merge_shards, dim3(B), dim3(EX_THREADS), 0, st, exact, ids, shard_stride, W, B, k,
                     scores_out, ids_out, flags_in, flag_stride, flags_out);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
