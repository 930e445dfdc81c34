// Device helpers shared by the sweeps: scan.hip, scan_wide.hip, sq8.hip and grouped.hip.
#pragma once
#include "rf_internal.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// MODE_FOLD: the sample pass that also keeps, per lane, its query's best score with its row and
// its second best score (scan.hip, "sample fold")
enum { MODE_SAMPLE = 0, MODE_EMIT = 1, MODE_FOLD = 2 };

#define SCAP 64  // per-wave LDS staging entries (>= 64: one ballot round can add 64)

struct ScanParams {
  const uint4* corpus;   // tiled
  const _Float16* q;     // row-major [B, dim]
  int B;
  uint32_t n_rows;
  uint32_t n_work;       // work items (blocks) for this launch
  uint32_t bstride;      // corpus block index = work index * bstride
  const float* thr;      // [64]
  uint32_t* cand_cnt;    // [64][RF_CAND_SHARDS]
  uint2* cand;           // [64][RF_CAND_SHARDS][cap]
  uint32_t cap;
  float* pmax;           // [64][P]
  int P;
  // sample fold (rf_fold; the 64-query sweep without a filter).  MODE_FOLD writes `fold` and
  // zeroes rmask / rcnt; MODE_EMIT with s_n > 0 sweeps the n_work - s_n blocks the sample did not
  // read, then the rcnt blocks of rlist, each for the queries of its sample wave's rmask only
  uint4* fold;                   // [64][RF_FOLD_WAVES]
  unsigned long long* rmask;     // [sample waves]
  uint32_t* rlist;
  uint32_t* rcnt;
  uint32_t s_n, s_bs, s_W;       // sampled blocks, their stride, sample waves
  // range search (the BAND instantiations only): the ceiling of the band and the per-query eps.
  // MODE_SAMPLE keeps a row out of the maximum unless score <= hi - eps (then a <= hi for
  // certain), MODE_EMIT appends a row only if score <= hi + eps (any row with a <= hi)
  const float* eps;              // [64]
  double band_hi;
};

// The masked sweep (filtered search): work item w is block blocks[w * bstride] of the filter's
// ascending pass list instead of block w * bstride, and a row is a candidate only if its mask bit
// is set.  The work count comes from the filter header on the device; the host sizes the grid
// from the index's total block count.
struct ScanParamsF : ScanParams {
  const uint32_t* hdr;     // filter header {n_rows, n_pass_rows, n_pass_blocks, n_tiles}
  const uint32_t* mask;    // [nblk] row bits
  const uint32_t* blocks;  // ascending pass blocks
  uint32_t n_blocks;       // blocks of the index (clamp of the device count)
  uint32_t work_lo, work_hi;  // sample pass: bounds of the sampled block count (n_work is unused)
};

// Per-query filters (k_scan_filtered<..., MULTI = true>): hdr / blocks are those of the union of
// the batch's filters (`mask` is not read), and the row bits a lane tests are its own query's:
// word masks_t[b * gp + qfilter[query of the lane]] of block b.  A type of its own, so that the
// arguments of the other sweeps stay what they are.
struct ScanParamsM : ScanParamsF {
  const uint32_t* masks_t;   // [nblk][gp] the filters' mask words, block-major
  const int32_t* qfilter;    // [B] filter number per query
  uint32_t gp;               // words per block: a power of two >= the number of filters
};

// Per-row weights (k_scan_weighted; decayed search): the masked sweep over
// w32[row] * score.  hdr == nullptr: no filter -- the work items are the blocks of the index and the
// mask word of a block has the bits of its existing rows (mask / blocks are not read then).  A type
// of its own, so that the arguments of the other sweeps stay what they are.
struct ScanParamsW : ScanParamsF {
  const float* w32;   // [n_rows], 16-byte aligned, every weight in [0, 1]
};

// Search-after (k_scan_after / k_scan_filtered_after, always the band form): the fp64 score of each
// query's bound.  The ceiling of query b is rf_after_ceiling(band_hi, after_s[b], ...) instead of
// band_hi: min(hi, bound) in the emit, the strict one in the sample pass.  Types of
// their own, so that the arguments of the other sweeps stay what they are.
struct ScanParamsA : ScanParams {
  const double* after_s;   // [B]
};
struct ScanParamsFA : ScanParamsF {
  const double* after_s;   // [B]
};

#ifndef RF_RING24
#define RF_RING24 24
#endif
template <int KS>
struct RingOf {
  static constexpr int R = (KS == 24) ? RF_RING24 : ((KS < 24) ? KS : 16);  // must divide KS
};

__device__ __forceinline__ u32x4 ld_frag(const uint4* p) {
  return __builtin_nontemporal_load((const u32x4*)p);
}

__device__ __forceinline__ float max16(const f32x16& a) {
  float m0 = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
  float m1 = fmaxf(fmaxf(a[4], a[5]), fmaxf(a[6], a[7]));
  float m2 = fmaxf(fmaxf(a[8], a[9]), fmaxf(a[10], a[11]));
  float m3 = fmaxf(fmaxf(a[12], a[13]), fmaxf(a[14], a[15]));
  return fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
}

// row of accumulator register i within the 32-row block (lane half h)
__device__ __forceinline__ uint32_t acc_row(int i, int h) {
  return (uint32_t)((i & 3) + 8 * (i >> 2) + 4 * h);
}

// (a maximum is exact in any order; the wave sums stay with their kernels: their order is their bits)
__device__ __forceinline__ float wave_max_xor(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// The MFMA chain of one 32-row block against the JB query groups in LDS: acc = scores, and the
// register ring re-armed for the next block (fragment t + R is requested right after fragment t
// has been consumed; LAST: nothing follows).
template <int KS, int R, int JB, bool LAST>
__device__ __forceinline__ void mfma_block(u32x4 (&ring)[R], const uint4* cur, const uint4* nxt,
                                           const u32x4* smemQ, int lane, f32x16 (&acc)[JB]) {
  static_assert(KS % R == 0, "ring must divide the block");
  // keep the query-fragment LDS reads inside the block: hoisted out of the
  // block loop they would pin JB*KS*4 registers and spill
  asm volatile("" ::: "memory");
#pragma unroll
  for (int jb = 0; jb < JB; ++jb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[jb][i] = 0.f;
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    const half8 a = __builtin_bit_cast(half8, ring[kk % R]);
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) {
      const half8 b = __builtin_bit_cast(half8, smemQ[(jb * KS + kk) * 64 + lane]);
      acc[jb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[jb], 0, 0, 0);
    }
    // re-arm this ring slot with the fragment R steps ahead
    if (kk + R < KS) {
      ring[kk % R] = ld_frag(cur + (kk + R) * 64);
    } else if (!LAST) {
      ring[kk % R] = ld_frag(nxt + (kk + R - KS) * 64);
    }
  }
}

// The queries of a sweep into LDS in B-fragment order: a row is KF fragments' worth of 32 bytes
// (fp16: KF = KS, 16 dims; int8: KF = KS8, 32 dims), and lane (j = l & 31, h = l >> 5) of fragment
// (jb, kk) holds the 16 bytes at 32 kk + 16 h of query 32 jb + j.  Query slots past B read as zero.
template <int KF, int JB, int WAVES>
__device__ __forceinline__ void stage_queries(u32x4* smemQ, const void* q_bytes, int B) {
  for (int idx = threadIdx.x; idx < JB * KF * 64; idx += WAVES * 64) {
    const int l = idx & 63;
    const int kk = (idx >> 6) % KF;
    const int jb = idx / (64 * KF);
    const int qi = jb * 32 + (l & 31);
    u32x4 v = {0u, 0u, 0u, 0u};
    if (qi < B) v = *(const u32x4*)((const unsigned char*)q_bytes + (size_t)qi * (KF * 32) + kk * 32 + (l >> 5) * 16);
    smemQ[idx] = v;
  }
}

// Work items of a masked sweep: the pass blocks of the filter, zero if its header was built for
// another row count, clamped to the blocks of the index.
__device__ __forceinline__ uint32_t filter_pass_blocks(const uint32_t* hdr, uint32_t n_rows, uint32_t n_blocks) {
  const uint32_t npb = hdr[0] == n_rows ? hdr[2] : 0u;
  return npb < n_blocks ? npb : n_blocks;
}

struct EmitState {
  uint32_t* s_row;     // [entries] per wave (LDS)
  float* s_score;      // [entries]
  uint32_t* s_q;       // [entries]
  uint32_t cnt;        // wave-uniform
  uint32_t q_base;     // query index of this wave's column 0 (wide sweep: 32 * wave)
};

// The staging area of a workgroup is three arrays [waves][entries]: rows, scores, queries.
__device__ __forceinline__ EmitState emit_state(uint32_t* stage, int wave, int waves, int entries) {
  EmitState es;
  es.s_row = stage + wave * entries;
  es.s_score = (float*)(stage + waves * entries) + wave * entries;
  es.s_q = stage + 2 * waves * entries + wave * entries;
  es.cnt = 0;
  es.q_base = 0;
  return es;
}

struct EmitListFull {   // emit_flush: nothing to do for a query whose list is full
  __device__ __forceinline__ void operator()(uint32_t) const {}
};

// on_full(q): called for every entry that found the list of its query q full (the merge flags
// such a query whatever else is appended).
template <class P, class F = EmitListFull>
__device__ __forceinline__ void emit_flush(EmitState& es, const P& p, int lane, F on_full = F()) {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  for (uint32_t i = lane; i < es.cnt; i += 64) {
    const uint32_t q = es.s_q[i];
    // RF_CAND_SHARDS counters per query: same-address atomics serialise (~12 ns
    // each), and most waves flush together at the end of the scan
    const uint32_t list = q * RF_CAND_SHARDS + (blockIdx.x & (RF_CAND_SHARDS - 1));
    const uint32_t slot = atomicAdd(&p.cand_cnt[list], 1u);
    if (slot < p.cap)
      p.cand[(size_t)list * p.cap + slot] =
          make_uint2(es.s_row[i], __builtin_bit_cast(uint32_t, es.s_score[i]));
    else
      on_full(q);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  es.cnt = 0;
}

// The append loop over a per-lane hit mask the caller built (bit jb*16+i: register i of query
// group jb; `sc` holds the scores that are appended).  The wave retires each lane's lowest set
// bit per iteration and ballot-compacts the hits into the staging area; flush() empties it when
// the round would not fit.
template <int JB, class F>
__device__ __forceinline__ void emit_append(const f32x16 (&sc)[JB], uint32_t bits, uint32_t row0, int lane,
                                            EmitState& es, F flush) {
  const int h = lane >> 5;
  unsigned long long mask;
  while ((mask = __ballot(bits != 0u)) != 0ull) {
    const bool pass = bits != 0u;
    const int b = __ffs((int)bits) - 1;  // -1 when !pass (unused then)
    float s = 0.f;
#pragma unroll
    for (int jb = 0; jb < JB; ++jb)
#pragma unroll
      for (int i = 0; i < 16; ++i) s = (b == jb * 16 + i) ? sc[jb][i] : s;
    const uint32_t n = (uint32_t)__popcll(mask);
    if (es.cnt + n > SCAP) flush();
    if (pass) {
      const uint32_t slot = es.cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      es.s_row[slot] = row0 + acc_row(b & 15, h);
      es.s_score[slot] = s;
      es.s_q[slot] = es.q_base + (uint32_t)((b >> 4) * 32 + (lane & 31));
    }
    es.cnt += n;
    bits &= bits - 1u;
  }
}

// Slow path of the filter (some lane holds a score >= its query's threshold).
// Branch-free build of a per-lane 32-bit hit mask, then emit_append: the usual case (one or two
// hits in the whole wave) costs one iteration instead of 32 ballot+branch rounds.
// FILTER: `mword` is the block's filter word; a row whose bit is clear is never a candidate,
// whatever its score (an explicit test: the threshold may be -inf, so masking by writing -inf
// into the accumulators would not keep rejected rows out).
// BAND: `tc` is the per-lane ceiling of the emit (hi + eps); a row above it is no candidate.
// MULTI (per-query filters, with FILTER): the word is the lane's own per query group, `mwl[jb]`,
// instead of the wave's `mword`; the test stays explicit for the same reason.
template <int JB, class P, bool FILTER = false, bool BAND = false, bool MULTI = false>
__device__ __forceinline__ void emit_slow(const f32x16 (&acc)[JB], const float (&th)[JB],
                                          uint32_t row0, int lane, EmitState& es, const P& p,
                                          uint32_t mword = 0u, const float* tc = nullptr,
                                          const uint32_t* mwl = nullptr) {
  const int h = lane >> 5;
  const uint32_t lim = p.n_rows - row0;  // rows of this block that exist (>= 32 except the last block)
  uint32_t bits = 0u;
#pragma unroll
  for (int jb = 0; jb < JB; ++jb)
#pragma unroll
    for (int i = 0; i < 16; ++i)
      bits |= ((acc[jb][i] >= th[jb]) && (acc_row(i, h) < lim) &&
               (!FILTER || (((MULTI ? mwl[jb] : mword) >> acc_row(i, h)) & 1u) != 0u) &&
               (!BAND || acc[jb][i] <= tc[jb])) ? (1u << (jb * 16 + i)) : 0u;
  emit_append<JB>(acc, bits, row0, lane, es, [&] { emit_flush(es, p, lane); });
}

// Slow path, second form (wide sweep): one ballot per accumulator register instead of a
// per-lane bit mask and a 32-way select chain.  A hit is rare (~0.3 per wave and block at the
// default sample size) and almost always a single (query, row) pair, so the cost that matters
// is the scan for it: per register one compare whose SGPR-pair result IS the ballot, one scalar
// test, and the append only behind a taken branch.  `jb_hit` (wave-uniform) says which of the
// query blocks needs scanning at all.
// The staging area holds CAP entries and is flushed by the CALLER at one place per phase (an
// inlined flush per append, or even per query block, multiplies the code and made hipcc spill
// in the MFMA loop).  An append that does not fit -- more hits within one phase than the room
// left at its start: duplicate-heavy or otherwise adversarial data -- is not stored; instead its query's candidate counter is pushed past the
// list capacity, which the merge reports as RF_FLAG_CAND_OVERFLOW, and the caller answers that
// query through the exhaustive path.
template <int JB, int CAP, class P>
__device__ __forceinline__ void emit_scan(const f32x16 (&acc)[JB], const float (&th)[JB],
                                          const unsigned long long (&jb_hit)[JB], uint32_t row0,
                                          int lane, EmitState& es, const P& p) {
  const int h = lane >> 5;
  const uint32_t lim = p.n_rows - row0;  // rows of this block that exist (0 for a block past the end)
#pragma unroll
  for (int jb = 0; jb < JB; ++jb) {
    if (jb_hit[jb] == 0ull) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool ok = (acc[jb][i] >= th[jb]) && (acc_row(i, h) < lim);
      const unsigned long long mask = __ballot(ok);
      if (mask != 0ull) {
        const uint32_t n = (uint32_t)__popcll(mask);
        const uint32_t q = es.q_base + (uint32_t)(jb * 32 + (lane & 31));
        if (es.cnt + n <= (uint32_t)CAP) {
          if (ok) {
            const uint32_t slot = es.cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            es.s_row[slot] = row0 + acc_row(i, h);
            es.s_score[slot] = acc[jb][i];
            es.s_q[slot] = q;
          }
          es.cnt += n;
        } else if (ok) {
          atomicAdd(&p.cand_cnt[q * RF_CAND_SHARDS + (blockIdx.x & (RF_CAND_SHARDS - 1))], p.cap + 1u);
        }
      }
    }
  }
}
