// Streaming query x corpus scan on the matrix cores with a fused top-k filter.
// This is the arithmetic Milvus performs for the reference's
// Collection.search(..., {"metric_type": "COSINE"}, top_k)
// (vector_rag_mcp/main.py:51-57, retrieve.py:28-34), restated for gfx950:
//
//   * the corpus lives in HBM as 32-row blocks of KS = dim/16 MFMA A-fragments
//     (rf_internal.h); a wave streams a block with KS 1-KiB loads that land
//     directly in the operand registers of v_mfma_f32_32x32x16_f16 -- no LDS
//     round trip, no bank conflicts, every byte read exactly once;
//   * the (<= 64) queries of the sweep sit in LDS in B-fragment order and are
//     re-read per k-step (48 KB at dim 384);
//   * each lane owns ONE query column of the 32x32 result, so the top-k filter
//     is a lane-local compare against that query's threshold;
//   * the loads form a register ring: fragment t+R is requested right after
//     fragment t has been consumed, so every wave keeps R KiB (24 KiB at dim
//     384) in flight across block boundaries and filter work.
//
// Two filters share the loop:
//   MODE_SAMPLE  running max per lane over a strided sample of blocks ->
//                one partition maximum per workgroup and query.  The k-th
//                largest of those maxima is a lower bound of the final k-th
//                best score (merge.hip turns it into the emit threshold).
//   MODE_EMIT    every score >= threshold is appended to that query's
//                candidate list (wave-level ballot compaction into LDS,
//                flushed with one global atomic per entry).
//
// Sample fold (64-query sweep without a filter): the sample pass
// (MODE_FOLD) also keeps, per lane, the best score of its query over the lane's rows
// with that row, and the second best score.  k_threshold (merge.hip) appends the best
// row wherever the second best is below the threshold -- then no other row of that lane
// can be a candidate -- and otherwise marks the query in its sample wave's rescan mask.
// The emit sweep then reads only the blocks the sample did not read, plus the blocks of
// the marked sample waves, filtered to the marked queries: every corpus byte is read
// once per batch instead of the sampled 1/16 twice.
#include "rf_internal.h"
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#include "scan_common.h"

// MODE_FOLD: the best of the 16 scores of a lane with its row (the first on ties), and the second
// best, folded into the lane's running (m1, r1, m2).  m1 is selected, never computed, so it is
// the bit pattern the emit would append for row r1; a NaN is never selected (m1 is the maximum
// of the other scores, as max16 is, and serves as the partition maximum pm).  fminf / fmaxf drop
// a NaN: it can only raise m2, which makes a list incomplete, never wrongly complete.
__device__ __forceinline__ void fold_top2(const f32x16& a, uint32_t rbase, float& m1, uint32_t& r1,
                                          float& m2) {
  float b1 = -INFINITY, b2 = -INFINITY;
  uint32_t bi = acc_row(0, 0);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float x = a[i];
    const bool c = x > b1;
    b2 = fmaxf(b2, fminf(b1, x));
    bi = c ? acc_row(i, 0) : bi;
    b1 = c ? x : b1;
  }
  m2 = fmaxf(fmaxf(m2, b2), fminf(m1, b1));
  const bool c = b1 > m1;
  r1 = c ? rbase + bi : r1;
  m1 = c ? b1 : m1;
}

// BAND (range search): tc is the lane's ceiling -- hi - eps in the sample pass (rows above it
// leave the maximum, like rows a filter rejects), hi + eps in the emit (rows above it are no
// candidates; the block prefilter tests thr <= score <= ceiling per row -- two compares whose
// lane masks combine on the scalar unit, no clipped copy of the accumulators -- so a block whose
// only rows >= thr lie above the ceiling never reaches emit_slow).
// MULTI (per-query filters, always with FILTER and without BAND): the filter word is per lane and
// query group, `mwl[jb]` -- the word of the lane's own query's filter for this block -- instead of
// the wave's `mword`.  A block of the union in which the lane's query has no row has word 0 there.
// WEIGHTED (per-row weights, always with FILTER, without BAND and MULTI): every score is multiplied
// by the weight of its row, w32[row] in [0, 1], before anything looks at it -- the sample maxima,
// the threshold test and the appended score bits are those of the weighted score.  Multiply first,
// mask afterwards: a rejected row is set to -inf, and -inf * 0 would be a NaN.  The 16 weights of a
// lane (four runs of four rows) are requested ahead of the MFMA chain; rows past the end weigh 0.
template <int KS, int R, int JB, int MODE, bool LAST, bool FILTER = false, bool BAND = false, bool MULTI = false,
          bool WEIGHTED = false>
__device__ __forceinline__ void block_step(u32x4 (&ring)[R], const uint4* cur,
                                           const uint4* nxt, const u32x4* smemQ, int lane,
                                           uint32_t row0, const float (&th)[JB], float (&pm)[JB],
                                           float (&m1)[JB], uint32_t (&r1)[JB], float (&m2)[JB],
                                           EmitState& es, const ScanParams& p,
                                           uint32_t mword = 0u, const float* tc = nullptr,
                                           const uint32_t* mwl = nullptr, const float* w32 = nullptr) {
  static_assert(!MULTI || (FILTER && !BAND && MODE != MODE_FOLD), "per-query filters: the plain masked sweep only");
  static_assert(!WEIGHTED || (FILTER && !BAND && !MULTI && MODE != MODE_FOLD), "per-row weights: the plain masked sweep only");
  f32x16 acc[JB];
  float wv[WEIGHTED ? 16 : 1];
  if constexpr (WEIGHTED) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const uint32_t r0 = row0 + 8u * (uint32_t)g + 4u * (uint32_t)(lane >> 5);   // rows of registers 4 g .. 4 g + 3
      if (r0 + 4u <= p.n_rows) {
        const float4 v = *(const float4*)(w32 + r0);
        wv[4 * g + 0] = v.x;
        wv[4 * g + 1] = v.y;
        wv[4 * g + 2] = v.z;
        wv[4 * g + 3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) wv[4 * g + j] = r0 + (uint32_t)j < p.n_rows ? w32[r0 + (uint32_t)j] : 0.f;
      }
    }
  }
  mfma_block<KS, R, JB, LAST>(ring, cur, nxt, smemQ, lane, acc);
  if constexpr (WEIGHTED) {
#pragma unroll
    for (int jb = 0; jb < JB; ++jb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[jb][i] *= wv[i];
  }

  if (MODE != MODE_EMIT) {
    if (MULTI) {
      // rows the lane's own filter rejects leave the lane's maximum: every partition maximum of
      // query q is taken over rows of S_q only
      bool part = false;
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) part |= mwl[jb] != 0xFFFFFFFFu;
      if (__ballot(part) != 0ull) {
        const int h = lane >> 5;
#pragma unroll
        for (int jb = 0; jb < JB; ++jb)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (((mwl[jb] >> acc_row(i, h)) & 1u) == 0u) acc[jb][i] = -INFINITY;
      }
    } else if (FILTER) {
      // rows the filter rejects (and rows past the end: their bits are zero) leave the maximum
      if (mword != 0xFFFFFFFFu) {  // wave-uniform
        const int h = lane >> 5;
#pragma unroll
        for (int jb = 0; jb < JB; ++jb)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (((mword >> acc_row(i, h)) & 1u) == 0u) acc[jb][i] = -INFINITY;
      }
    } else if (row0 + 32u > p.n_rows) {  // wave-uniform: only the corpus' last block
      const int h = lane >> 5;
#pragma unroll
      for (int jb = 0; jb < JB; ++jb)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (row0 + acc_row(i, h) >= p.n_rows) acc[jb][i] = -INFINITY;
    }
    if (BAND) {
#pragma unroll
      for (int jb = 0; jb < JB; ++jb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[jb][i] = acc[jb][i] <= tc[jb] ? acc[jb][i] : -INFINITY;
    }
    if (MODE == MODE_FOLD) {
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) fold_top2(acc[jb], row0 + 4u * (uint32_t)(lane >> 5), m1[jb], r1[jb], m2[jb]);
    } else {
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) pm[jb] = fmaxf(pm[jb], max16(acc[jb]));
    }
  } else {
    bool hit = false;
    if (BAND) {
#pragma unroll
      for (int jb = 0; jb < JB; ++jb)
#pragma unroll
        for (int i = 0; i < 16; ++i) hit |= (acc[jb][i] >= th[jb]) & (acc[jb][i] <= tc[jb]);
    } else {
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) hit |= (max16(acc[jb]) >= th[jb]);
    }
    if (__ballot(hit) != 0ull)
      emit_slow<JB, ScanParams, FILTER, BAND, MULTI>(acc, th, row0, lane, es, p, mword, tc, mwl);
  }
}

// FILTER (filtered search, p is a ScanParamsF): the work items are the filter's pass blocks
// (sample pass: every bstride-th of them), counted on the device; see scan_common.h.
// AFTER (search-after, always with BAND): the ceiling is per query, from the bound's score in
// device memory (rf_after_ceiling); everything after the set-up of tc is the band sweep.
template <int KS, int R, int JB, int WAVES, int MODE, bool FILTER, bool BAND, bool AFTER, class PT>
__device__ __forceinline__ void scan_body(PT p, unsigned char* smem_raw) {
  static_assert(!BAND || MODE != MODE_FOLD, "the band sweep has no sample fold");
  static_assert(!AFTER || BAND, "a search-after sweep is a band sweep");
  // MULTI (p is a ScanParamsM): the work items are the pass blocks of the union of the batch's
  // filters, the row bits per lane those of its own query's filter
  constexpr bool MULTI = std::is_same<PT, ScanParamsM>::value;
  static_assert(!MULTI || (FILTER && !BAND), "per-query filters: the plain masked sweep only");
  // WEIGHTED (p is a ScanParamsW): the masked sweep over w32[row] * score; without a filter
  // (hdr == nullptr) the pass list is every block and the mask word the rows that exist
  constexpr bool WEIGHTED = std::is_same<PT, ScanParamsW>::value;
  static_assert(!WEIGHTED || (FILTER && !BAND), "per-row weights: the plain masked sweep only");
  u32x4* smemQ = (u32x4*)smem_raw;                                  // JB*KS*64 uint4
  unsigned char* tail = smem_raw + (size_t)JB * KS * RF_FRAG_BYTES;  // per-mode scratch

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  float th[JB];
  float pm[JB];
  float m1[JB];     // MODE_FOLD: best score (the partition maximum), its row, second best score
  uint32_t r1[JB];
  float m2[JB];
  float tc[JB];     // BAND: the lane's ceiling (block_step)
#pragma unroll
  for (int jb = 0; jb < JB; ++jb) {
    if (BAND) {
      const int ql = jb * 32 + (lane & 31);
      const double e = (double)p.eps[ql];
      double hi = p.band_hi;
      if constexpr (AFTER) {
        if (ql < p.B) hi = rf_after_ceiling(hi, p.after_s[ql], MODE != MODE_EMIT);  // (slots past B have no bound)
      }
      tc[jb] = (MODE == MODE_EMIT) ? rf_band_ceil(hi + e) : rf_band_floor(hi - e);
    } else {
      tc[jb] = INFINITY;
    }
    pm[jb] = -INFINITY;
    m1[jb] = -INFINITY;
    r1[jb] = 0xFFFFFFFFu;
    m2[jb] = -INFINITY;
    th[jb] = (MODE == MODE_EMIT) ? p.thr[jb * 32 + (lane & 31)] : 0.f;
  }
  EmitState es = emit_state((uint32_t*)tail, wave, WAVES, SCAP);  // (touched by MODE_EMIT only)

  // work items w = gw, gw + W, ...  (one item = one 32-row block)
  const uint32_t W = gridDim.x * WAVES;
  // MULTI sample pass: the waves of a workgroup take items a whole grid apart instead of
  // neighbours, so that a partition (= workgroup) reads blocks from all over the union.  A filter
  // that is one contiguous 1/G of the corpus then has rows in about min(P, sampled blocks / G)
  // partitions instead of P / G, and the k-th partition maximum of its queries exists.
  const uint32_t gw = (MULTI && MODE == MODE_SAMPLE) ? wave * gridDim.x + blockIdx.x : blockIdx.x * WAVES + wave;
  if constexpr (FILTER) {
    uint32_t npb;
    if constexpr (WEIGHTED) npb = p.hdr ? filter_pass_blocks(p.hdr, p.n_rows, p.n_blocks) : p.n_blocks;
    else npb = filter_pass_blocks(p.hdr, p.n_rows, p.n_blocks);
    if (MODE == MODE_SAMPLE) {  // ~1/16 of the pass blocks, spread evenly (rf_launch_sample)
      uint32_t n = npb / 16;
      n = n < p.work_lo ? p.work_lo : n;
      n = n > p.work_hi ? p.work_hi : n;
      n = n > npb ? npb : n;
      p.n_work = n;
      p.bstride = n ? npb / n : 1u;
    } else {
      p.n_work = npb;
      p.bstride = 1u;
    }
  }
  // Emit sweep with a sample fold (s_n > 0): item i < M is the i-th block the sample did not read
  // (L of them inside the sample's stride groups, then the tail past the last group), item M + j
  // is rlist[j].  Dense items keep every wave busy: skipping the sampled blocks inside the plain
  // round-robin would idle the waves whose blocks are the sample's (W is a multiple of s_bs).
  // With s_n = 0 item i is block i.
  // (a band sweep never folds: its emit is the plain walk over every block)
  const bool folded = !FILTER && !BAND && MODE == MODE_EMIT && p.s_n > 0u;  // wave-uniform
  const uint32_t M = folded ? p.n_work - p.s_n : p.n_work;
  const uint32_t L = folded ? p.s_n * (p.s_bs - 1u) : 0u;
  uint32_t n_res = 0u;
  if (folded) {  // (consumed after the query staging)
    n_res = *p.rcnt;
    n_res = n_res < p.s_n ? n_res : p.s_n;  // rlist holds each sampled block at most once
  }
  auto block_of = [&](uint32_t i) -> uint32_t {
    if (i < L) {
      const uint32_t g = i / (p.s_bs - 1u);
      return g * p.s_bs + 1u + (i - g * (p.s_bs - 1u));
    }
    if (i < M) return i + (folded ? p.s_n : 0u);
    const uint32_t r = p.rlist[i - M];
    return r < p.n_work ? r : 0u;  // (k_threshold lists sampled blocks only: never past the corpus)
  };

  // Entry of the pass list that work item w of a masked sweep reads.  MULTI sample pass: item w
  // steps through its stride group (entry w * bstride + w mod bstride, still below (w + 1) * bstride
  // <= the list's length), so that the sampled blocks do not all share one residue modulo the
  // stride: with filters interleaved row by row (row r in filter r mod G) the blocks at a fixed
  // even stride hold rows of half the filters only, and the other half would get no threshold.
  auto fitem = [&](uint32_t w) -> uint32_t {
    if constexpr (FILTER) {
      if constexpr (MULTI && MODE == MODE_SAMPLE) return w * p.bstride + w % p.bstride;
      else return w * p.bstride;
    } else {
      return w;
    }
  };
  (void)fitem;
  // WEIGHTED: entry i of the pass list and the mask word of block b, with or without a filter
  auto wblock = [&](uint32_t i) -> uint32_t {
    if constexpr (WEIGHTED) return p.hdr ? p.blocks[i] : i;
    else return i;
  };
  auto wmask = [&](uint32_t b) -> uint32_t {
    if constexpr (WEIGHTED) {
      if (p.hdr) return p.mask[b];
      const uint32_t rows = p.n_rows - b * 32u;   // > 0: b is a block of the index
      return rows < 32u ? (1u << rows) - 1u : 0xFFFFFFFFu;
    } else {
      return 0u;
    }
  };
  (void)wblock;
  (void)wmask;

  u32x4 ring[R];
  if (FILTER ? gw < p.n_work : gw < M) {
    const uint4* src;
    if constexpr (WEIGHTED) src = p.corpus + (size_t)wblock(fitem(gw)) * (KS * 64) + lane;
    else if constexpr (FILTER) src = p.corpus + (size_t)p.blocks[fitem(gw)] * (KS * 64) + lane;
    else if constexpr (MODE == MODE_EMIT && !BAND) src = p.corpus + (size_t)block_of(gw) * (KS * 64) + lane;
    else src = p.corpus + (size_t)gw * p.bstride * (KS * 64) + lane;
#pragma unroll
    for (int s = 0; s < R; ++s) ring[s] = ld_frag(src + s * 64);
  }
  // (the corpus stream starts BEFORE the queries are staged: the first HBM round trip runs
  // under the staging loop and its barrier instead of after them)
  stage_queries<KS, JB, WAVES>(smemQ, p.q, p.B);
  __syncthreads();
  const uint32_t n_items = M + n_res;
  const uint32_t cnt = (n_items > gw) ? (n_items - gw + W - 1) / W : 0u;
  if (!FILTER && !BAND && cnt > 0 && gw >= M) {  // the wave's first item is a rescan (a corpus of few blocks)
    const uint4* src = p.corpus + (size_t)block_of(gw) * (KS * 64) + lane;
#pragma unroll
    for (int s = 0; s < R; ++s) ring[s] = ld_frag(src + s * 64);
  }
  if (cnt > 0) {

    uint32_t w = gw;
    if constexpr (MULTI) {
      // the column of the lane's query's filter in masks_t (a number past the filters lands in a
      // padding column or wraps onto a filter: never past the row of the block)
      uint32_t gcol[JB];
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) {
        const int ql = jb * 32 + (lane & 31);
        gcol[jb] = ql < p.B ? ((uint32_t)p.qfilter[ql] & (p.gp - 1u)) : 0u;
      }
      uint32_t b = p.blocks[fitem(w)];
      for (uint32_t i = 0; i + 1 < cnt; ++i, w += W) {
        // as below, with one vector load per query group for the lane's own mask word: issued
        // ahead of the ring's loads of this step, consumed after the MFMA chain
        const uint32_t bn = p.blocks[fitem(w + W)];
        uint32_t mwl[JB];
#pragma unroll
        for (int jb = 0; jb < JB; ++jb) mwl[jb] = p.masks_t[(size_t)b * p.gp + gcol[jb]];
        const uint4* cur = p.corpus + (size_t)b * (KS * 64) + lane;
        const uint4* nxt = p.corpus + (size_t)bn * (KS * 64) + lane;
        block_step<KS, R, JB, MODE, false, true, false, true>(ring, cur, nxt, smemQ, lane, b * 32u, th, pm, m1, r1, m2, es, p, 0u, tc, mwl);
        b = bn;
      }
      {
        uint32_t mwl[JB];
#pragma unroll
        for (int jb = 0; jb < JB; ++jb) mwl[jb] = p.masks_t[(size_t)b * p.gp + gcol[jb]];
        const uint4* cur = p.corpus + (size_t)b * (KS * 64) + lane;
        block_step<KS, R, JB, MODE, true, true, false, true>(ring, cur, cur, smemQ, lane, b * 32u, th, pm, m1, r1, m2, es, p, 0u, tc, mwl);
      }
    } else if constexpr (WEIGHTED) {
      // the masked sweep below, over the weighted scores
      uint32_t b = wblock(w * p.bstride);
      for (uint32_t i = 0; i + 1 < cnt; ++i, w += W) {
        const uint32_t bn = wblock((w + W) * p.bstride);
        const uint32_t mw = wmask(b);
        const uint4* cur = p.corpus + (size_t)b * (KS * 64) + lane;
        const uint4* nxt = p.corpus + (size_t)bn * (KS * 64) + lane;
        block_step<KS, R, JB, MODE, false, true, false, false, true>(ring, cur, nxt, smemQ, lane, b * 32u, th, pm, m1, r1, m2, es, p, mw, tc, nullptr, p.w32);
        b = bn;
      }
      {
        const uint32_t mw = wmask(b);
        const uint4* cur = p.corpus + (size_t)b * (KS * 64) + lane;
        block_step<KS, R, JB, MODE, true, true, false, false, true>(ring, cur, cur, smemQ, lane, b * 32u, th, pm, m1, r1, m2, es, p, mw, tc, nullptr, p.w32);
      }
    } else if constexpr (FILTER) {
      uint32_t b = p.blocks[w * p.bstride];
      for (uint32_t i = 0; i + 1 < cnt; ++i, w += W) {
        // scalar loads at the top of the step: the next block's index is needed only when the
        // ring re-arms across the boundary, the mask word only after the MFMA chain
        const uint32_t bn = p.blocks[(w + W) * p.bstride];
        const uint32_t mw = p.mask[b];
        const uint4* cur = p.corpus + (size_t)b * (KS * 64) + lane;
        const uint4* nxt = p.corpus + (size_t)bn * (KS * 64) + lane;
        block_step<KS, R, JB, MODE, false, true, BAND>(ring, cur, nxt, smemQ, lane, b * 32u, th, pm, m1, r1, m2, es, p, mw, tc);
        b = bn;
      }
      {
        const uint32_t mw = p.mask[b];
        const uint4* cur = p.corpus + (size_t)b * (KS * 64) + lane;
        block_step<KS, R, JB, MODE, true, true, BAND>(ring, cur, cur, smemQ, lane, b * 32u, th, pm, m1, r1, m2, es, p, mw, tc);
      }
    } else if constexpr (MODE == MODE_EMIT && !BAND) {
      // a rescanned block (item >= M) appends only for the queries its sample wave marked:
      // the others' rows of it came from k_threshold (an MFMA score is finite, never >= +inf)
      auto item_th = [&](uint32_t i, uint32_t b, float (&te)[JB]) {
        if (i < M) {
#pragma unroll
          for (int jb = 0; jb < JB; ++jb) te[jb] = th[jb];
        } else {
          const unsigned long long qm = p.rmask[(b / p.s_bs) % p.s_W];
#pragma unroll
          for (int jb = 0; jb < JB; ++jb)
            te[jb] = ((qm >> (jb * 32 + (lane & 31))) & 1ull) ? th[jb] : INFINITY;
        }
      };
      uint32_t b = block_of(w);
      for (uint32_t i = 0; i + 1 < cnt; ++i, w += W) {
        const uint32_t bn = block_of(w + W);
        const uint4* cur = p.corpus + (size_t)b * (KS * 64) + lane;
        const uint4* nxt = p.corpus + (size_t)bn * (KS * 64) + lane;
        float te[JB];
        item_th(w, b, te);
        block_step<KS, R, JB, MODE, false, false, BAND>(ring, cur, nxt, smemQ, lane, b * 32u, te, pm, m1, r1, m2, es, p, 0u, tc);
        b = bn;
      }
      {
        const uint4* cur = p.corpus + (size_t)b * (KS * 64) + lane;
        float te[JB];
        item_th(w, b, te);
        block_step<KS, R, JB, MODE, true, false, BAND>(ring, cur, cur, smemQ, lane, b * 32u, te, pm, m1, r1, m2, es, p, 0u, tc);
      }
    } else {
      for (uint32_t i = 0; i + 1 < cnt; ++i, w += W) {
        const uint32_t b = w * p.bstride;
        const uint4* cur = p.corpus + (size_t)b * (KS * 64) + lane;
        const uint4* nxt = p.corpus + (size_t)(b + W * p.bstride) * (KS * 64) + lane;
        block_step<KS, R, JB, MODE, false, false, BAND>(ring, cur, nxt, smemQ, lane, b * 32u, th, pm, m1, r1, m2, es, p, 0u, tc);
      }
      {
        const uint32_t b = w * p.bstride;
        const uint4* cur = p.corpus + (size_t)b * (KS * 64) + lane;
        block_step<KS, R, JB, MODE, true, false, BAND>(ring, cur, cur, smemQ, lane, b * 32u, th, pm, m1, r1, m2, es, p, 0u, tc);
      }
    }
  }

  if (MODE == MODE_EMIT) {
    if (es.cnt > 0) emit_flush(es, p, lane);
  } else {
    if (MODE == MODE_FOLD) {
      // this wave's kept list per query: the two lane halves' lists merged into the best score
      // with its row and the second best score over all the wave's rows of that query (a wave
      // without blocks writes -inf: complete, nothing to append); its rescan mask and the rescan
      // count start at zero for k_threshold
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) {
        const float o1 = __shfl_xor(m1[jb], 32);
        const uint32_t orow = (uint32_t)__shfl_xor((int)r1[jb], 32);
        const float o2 = __shfl_xor(m2[jb], 32);
        if (lane < 32) {
          const bool mine = !(o1 > m1[jb]);
          const float s2 = fmaxf(fmaxf(m2[jb], o2), fminf(m1[jb], o1));
          p.fold[(size_t)(jb * 32 + lane) * RF_FOLD_WAVES + gw] =
              make_uint4(__builtin_bit_cast(uint32_t, mine ? m1[jb] : o1), mine ? r1[jb] : orow,
                         __builtin_bit_cast(uint32_t, s2), 0u);
        }
      }
      if (lane == 0) p.rmask[gw] = 0ull;
      if (gw == 0 && lane == 0) *p.rcnt = 0u;
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) pm[jb] = m1[jb];
    }
    // workgroup partition maximum per query: max over waves and lane halves
    float* red = (float*)tail;  // [WAVES*2][JB*32]
#pragma unroll
    for (int jb = 0; jb < JB; ++jb)
      red[(wave * 2 + (lane >> 5)) * (JB * 32) + jb * 32 + (lane & 31)] = pm[jb];
    __syncthreads();
    if (tid < JB * 32) {
      float m = -INFINITY;
      for (int s = 0; s < WAVES * 2; ++s) m = fmaxf(m, red[s * (JB * 32) + tid]);
      p.pmax[(size_t)tid * p.P + blockIdx.x] = m;
    }
  }
}

template <int KS, int R, int JB, int WAVES, int MODE, bool BAND = false>
__global__ void __launch_bounds__(WAVES * 64, 2) k_scan(ScanParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  scan_body<KS, R, JB, WAVES, MODE, false, BAND, false>(p, smem_raw);
}

// MULTI: per-query filters (p is a ScanParamsM: the union's block list, per-lane mask words).
template <int KS, int R, int JB, int WAVES, int MODE, bool BAND = false, bool MULTI = false>
__global__ void __launch_bounds__(WAVES * 64, 2)
k_scan_filtered(typename std::conditional<MULTI, ScanParamsM, ScanParamsF>::type p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  scan_body<KS, R, JB, WAVES, MODE, true, BAND, false>(p, smem_raw);
}

// Per-row weights: the masked sweep over w32[row] * score (a kernel of its own, so that the names
// and arguments of the others stay what they are).
template <int KS, int R, int JB, int WAVES, int MODE>
__global__ void __launch_bounds__(WAVES * 64, 2) k_scan_weighted(ScanParamsW p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  scan_body<KS, R, JB, WAVES, MODE, true, false, false>(p, smem_raw);
}

// The search-after sweeps: the band sweeps above with the per-query ceiling.
template <int KS, int R, int JB, int WAVES, int MODE>
__global__ void __launch_bounds__(WAVES * 64, 2) k_scan_after(ScanParamsA p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  scan_body<KS, R, JB, WAVES, MODE, false, true, true>(p, smem_raw);
}

template <int KS, int R, int JB, int WAVES, int MODE>
__global__ void __launch_bounds__(WAVES * 64, 2) k_scan_filtered_after(ScanParamsFA p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  scan_body<KS, R, JB, WAVES, MODE, true, true, true>(p, smem_raw);
}

// ---- raw score dump (test hook) ---------------------------------------------
template <int KS>
__global__ void __launch_bounds__(64) k_debug_scores(const uint4* corpus, const _Float16* q, int B,
                                                      uint32_t n, float* out) {
  // one wave per (block, 32-query group); plain loads, no ring
  const int lane = threadIdx.x;
  const uint32_t b = blockIdx.x;
  const int jb = blockIdx.y;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int qi = jb * 32 + (lane & 31);
  for (int kk = 0; kk < KS; ++kk) {
    const uint4 av = corpus[((size_t)b * KS + kk) * 64 + lane];
    uint4 bv = make_uint4(0, 0, 0, 0);
    if (qi < B) bv = *(const uint4*)(q + (size_t)qi * (KS * 16) + kk * 16 + (lane >> 5) * 8);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, av),
                                                 __builtin_bit_cast(half8, bv), acc, 0, 0, 0);
  }
  if (qi < B) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t row = b * 32u + acc_row(i, lane >> 5);
      if (row < n) out[(size_t)qi * n + row] = acc[i];
    }
  }
}

// ---- host side ----------------------------------------------------------------
template <int KS, int R, int JB, int WAVES, int MODE, bool BAND, class PT>
static int launch_scan(const PT& p, int grid, hipStream_t st) {
  size_t lds = (size_t)JB * KS * RF_FRAG_BYTES;
  if (MODE == MODE_EMIT) lds += (size_t)3 * WAVES * SCAP * 4;
  else lds += (size_t)WAVES * 2 * JB * 32 * 4;
  auto kern = [] {
    if constexpr (std::is_same<PT, ScanParamsF>::value) return k_scan_filtered<KS, R, JB, WAVES, MODE, BAND>;
    else if constexpr (std::is_same<PT, ScanParamsM>::value) return k_scan_filtered<KS, R, JB, WAVES, MODE, BAND, true>;
    else if constexpr (std::is_same<PT, ScanParamsW>::value) return k_scan_weighted<KS, R, JB, WAVES, MODE>;
    else if constexpr (std::is_same<PT, ScanParamsFA>::value) return k_scan_filtered_after<KS, R, JB, WAVES, MODE>;
    else if constexpr (std::is_same<PT, ScanParamsA>::value) return k_scan_after<KS, R, JB, WAVES, MODE>;
    else return k_scan<KS, R, JB, WAVES, MODE, BAND>;
  }();
  static rf_lds_attr attr;  // per instantiation, per device
  RF_HIP(rf_ensure_lds(attr, (const void*)kern, lds));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVES * 64), lds, st, p);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

// The JB = 1 / JB = 2 pair of one (KS, ring depth, waves) shape.
template <int KS, int R, int WAVES, int MODE, bool BAND, class PT>
static int launch_scan_jb(int JB, const PT& p, int grid, hipStream_t st) {
  return JB == 1 ? launch_scan<KS, R, 1, WAVES, MODE, BAND>(p, grid, st)
                 : launch_scan<KS, R, 2, WAVES, MODE, BAND>(p, grid, st);
}

#define RF_CASE(ks, r, waves, grid) \
  case ks:                          \
    return launch_scan_jb<ks, r, waves, MODE, BAND>(JB, p, grid, st);

// (PT = ScanParamsA / ScanParamsFA: the search-after kernels, BAND = true)
template <int MODE, bool BAND = false, class PT>
static int dispatch_scan(int KS, int JB, const PT& p, int grid4, int grid8,
                         hipStream_t st) {
  // dim 384: the emit sweep runs best with a SHALLOW ring (8 fragments = 8 KiB per
  // wave in flight: 119 us vs 124 us at 24 -- deeper queues only add latency once
  // HBM is saturated), the short sample pass with the full-block ring (16 vs 21 us:
  // it has two blocks per wave and must prefetch the second during the first).
  if (KS == 24 && MODE == MODE_EMIT) {
    // short sweeps (a few blocks per wave: shards of a strong-scaled job, BASELINE configs[1]) are
    // latency-bound like the sample pass and prefer the full-block ring too: 21.7 vs 23.3 us at 100 k rows
    const int ring = (p.n_work < 6u * 4u * (uint32_t)grid4) ? 24 : rf_knob_ring24;
    switch (ring) {
      case 8:
        return launch_scan_jb<24, 8, 4, MODE, BAND>(JB, p, grid4, st);
#ifdef RF_EXPERIMENTS
      case 6:
        return launch_scan_jb<24, 6, 4, MODE, BAND>(JB, p, grid4, st);
      case 12:
        return launch_scan_jb<24, 12, 4, MODE, BAND>(JB, p, grid4, st);
#endif
      default:   // 24: the table's entry
        break;
    }
  }
  switch (KS) {
    RF_CASE(4, 4, 4, grid4)
    RF_CASE(8, 8, 4, grid4)
    RF_CASE(16, 16, 4, grid4)
    RF_CASE(24, 24, 4, grid4)
    RF_CASE(32, 16, 4, grid4)
    RF_CASE(48, 16, 8, grid8)
    RF_CASE(64, 16, 8, grid8)
    default:
      break;
  }
  rf_set_error("no scan kernel for dim %d", KS * 16);
  return RF_ERR_UNSUPPORTED;
}
#undef RF_CASE

int rf_scan_supported_dim(int dim) {
  switch (dim) {
    case 64: case 128: case 256: case 384: case 512: case 768: case 1024:
      return 1;
    default:
      return 0;
  }
}

// Per-query filters: the masked sweep's arguments (over the union: filt) with the per-lane words.
static ScanParamsM multi_params(const ScanParamsF& f, const rf_multi& multi) {
  ScanParamsM m{};
  static_cast<ScanParamsF&>(m) = f;
  m.masks_t = multi.masks_t;
  m.qfilter = multi.qfilter;
  m.gp = multi.gp;
  return m;
}

// Per-row weights: the masked sweep's arguments (filt: the filter's, or none of them) with the weights.
static ScanParamsW weighted_params(const ScanParamsF& f, const float* w32) {
  ScanParamsW w{};
  static_cast<ScanParamsF&>(w) = f;
  w.w32 = w32;
  return w;
}

int rf_launch_sample(const rf_index* ix, const void* q, int B, int JB, const rf_workspace& ws,
                     int* P_out, hipStream_t st, const rf_filter_view* filt, rf_fold* fold,
                     const rf_band* band, const rf_after* after, const rf_multi* multi, const float* w32) {
  const int KS = ix->KS;
  const uint32_t nblk = (uint32_t)((ix->size + 31) / 32);
  const int WAVES = rf_waves_per_wg(KS);
  // Sample ~1/16 of the corpus, spread evenly: candidates per query ~ k * N / n_sample
  // stay ~16 k whatever N is, and a small corpus does not pay a sample pass as long as
  // its scan.  At least 64 workgroups (partitions) so the k-th largest exists for
  // k <= 64, at most RF_SAMPLE_WGS workgroups x SAMPLE_BPW blocks per wave.
  const int SAMPLE_BPW = rf_knob_sample_bpw;
  uint32_t n_work = nblk / 16;
  const uint32_t lo = 64u * WAVES, hi = (uint32_t)RF_SAMPLE_WGS * WAVES * SAMPLE_BPW;
  if (n_work < lo) n_work = lo;
  if (n_work > hi) n_work = hi;
  if (n_work > nblk) n_work = nblk;
  // as many workgroups as there are waves' worth of blocks, capped at one per partition
  // slot; waves take blocks round-robin, so the load is balanced for any n_work
  int grid = (int)((n_work + WAVES - 1) / WAVES);
  if (grid > RF_SAMPLE_WGS) grid = RF_SAMPLE_WGS;
  if (grid < 1) grid = 1;
  const uint32_t bstride = nblk / n_work;  // >= 1
  ScanParams p{};
  p.corpus = ix->tiles;
  p.q = (const _Float16*)q;
  p.B = B;
  p.n_rows = (uint32_t)ix->size;
  p.n_work = n_work;
  p.bstride = bstride;
  p.pmax = ws.pmax;
  p.P = grid;
  *P_out = grid;
  if (fold) *fold = rf_fold{0u, 1u, 1u};
  if (band) {  // the clip reads the eps rf_launch_band_eps wrote; no fold in this form
    p.eps = ws.eps;
    p.band_hi = band->hi;
  }
  if (filt || w32) {
    // the grid (= partitions) is sized from the whole corpus; the kernel derives the sampled
    // count and stride from the filter's device count of pass blocks, within the same bounds
    ScanParamsF f{};
    static_cast<ScanParams&>(f) = p;
    if (filt) {
      f.hdr = filt->hdr;
      f.mask = filt->mask;
      f.blocks = filt->blocks;
    }
    f.n_blocks = nblk;
    f.work_lo = lo;
    f.work_hi = hi;
    if (w32) return dispatch_scan<MODE_SAMPLE>(KS, JB, weighted_params(f, w32), grid, grid, st);
    if (multi) return dispatch_scan<MODE_SAMPLE>(KS, JB, multi_params(f, *multi), grid, grid, st);
    if (band && after) {
      ScanParamsFA fa{};
      static_cast<ScanParamsF&>(fa) = f;
      fa.after_s = after->score;
      return dispatch_scan<MODE_SAMPLE, true>(KS, JB, fa, grid, grid, st);
    }
    return band ? dispatch_scan<MODE_SAMPLE, true>(KS, JB, f, grid, grid, st)
                : dispatch_scan<MODE_SAMPLE>(KS, JB, f, grid, grid, st);
  }
  if (band && after) {
    ScanParamsA pa{};
    static_cast<ScanParams&>(pa) = p;
    pa.after_s = after->score;
    return dispatch_scan<MODE_SAMPLE, true>(KS, JB, pa, grid, grid, st);
  }
  if (band) return dispatch_scan<MODE_SAMPLE, true>(KS, JB, p, grid, grid, st);
  if (fold && rf_knob_sample_fold && B <= RF_QCHUNK && n_work <= (uint32_t)RF_FOLD_BLOCKS &&
      (uint32_t)grid * WAVES <= (uint32_t)RF_FOLD_WAVES) {
    p.fold = ws.fold;
    p.rmask = ws.rmask;
    p.rcnt = ws.rcnt;
    *fold = rf_fold{n_work, bstride, (uint32_t)grid * WAVES};
    return dispatch_scan<MODE_FOLD>(KS, JB, p, grid, grid, st);
  }
  return dispatch_scan<MODE_SAMPLE>(KS, JB, p, grid, grid, st);
}

int rf_launch_emit(const rf_index* ix, const void* q, int B, int JB, const rf_workspace& ws,
                   hipStream_t st, const rf_filter_view* filt, const rf_fold* fold, const rf_band* band,
                   const rf_after* after, const rf_multi* multi, const float* w32) {
  const int KS = ix->KS;
  const uint32_t nblk = (uint32_t)((ix->size + 31) / 32);
  const int grid = rf_emit_grid(ix, rf_knob_emit_wgs_per_cu);
  ScanParams p{};
  p.corpus = ix->tiles;
  p.q = (const _Float16*)q;
  p.B = B;
  p.n_rows = (uint32_t)ix->size;
  p.n_work = nblk;
  p.bstride = 1;
  p.thr = ws.thr;
  p.cand_cnt = ws.cand_cnt;
  p.cand = ws.cand;
  p.cap = RF_SHARD_CAP;
  if (band) {  // eps: what k_threshold wrote
    p.eps = ws.eps;
    p.band_hi = band->hi;
  }
  if (fold && fold->n_samp > 0u && !filt && !band) {
    // the sweep skips the sampled blocks (scan_body): the grid and the ring depth stay those of
    // the whole corpus
    p.rmask = ws.rmask;
    p.rlist = ws.rlist;
    p.rcnt = ws.rcnt;
    p.s_n = fold->n_samp;
    p.s_bs = fold->bstride;
    p.s_W = fold->W;
  }
  if (filt || w32) {
    // grid and ring depth as for the whole corpus; waves past the device count exit
    ScanParamsF f{};
    static_cast<ScanParams&>(f) = p;
    if (filt) {
      f.hdr = filt->hdr;
      f.mask = filt->mask;
      f.blocks = filt->blocks;
    }
    f.n_blocks = nblk;
    if (w32) return dispatch_scan<MODE_EMIT>(KS, JB, weighted_params(f, w32), grid, grid, st);
    if (multi) return dispatch_scan<MODE_EMIT>(KS, JB, multi_params(f, *multi), grid, grid, st);
    if (band && after) {
      ScanParamsFA fa{};
      static_cast<ScanParamsF&>(fa) = f;
      fa.after_s = after->score;
      return dispatch_scan<MODE_EMIT, true>(KS, JB, fa, grid, grid, st);
    }
    return band ? dispatch_scan<MODE_EMIT, true>(KS, JB, f, grid, grid, st)
                : dispatch_scan<MODE_EMIT>(KS, JB, f, grid, grid, st);
  }
  if (band && after) {
    ScanParamsA pa{};
    static_cast<ScanParams&>(pa) = p;
    pa.after_s = after->score;
    return dispatch_scan<MODE_EMIT, true>(KS, JB, pa, grid, grid, st);
  }
  return band ? dispatch_scan<MODE_EMIT, true>(KS, JB, p, grid, grid, st)
              : dispatch_scan<MODE_EMIT>(KS, JB, p, grid, grid, st);
}

int rf_launch_debug_scores(const rf_index* ix, const void* q, int B, int64_t n, float* out,
                           hipStream_t st) {
  const uint32_t nblk = (uint32_t)((n + 31) / 32);
  const dim3 grid(nblk, (B + 31) / 32);
#define RF_DBG(ks)                                                                         \
  case ks:                                                                                 \
    hipLaunchKernelGGL(k_debug_scores<ks>, grid, dim3(64), 0, st, ix->tiles,               \
                       (const _Float16*)q, B, (uint32_t)n, out);                           \
    break;
  switch (ix->KS) {
    RF_DBG(4) RF_DBG(8) RF_DBG(16) RF_DBG(24) RF_DBG(32) RF_DBG(48) RF_DBG(64)
    default:
      rf_set_error("no debug kernel for dim %d", ix->dim);
      return RF_ERR_UNSUPPORTED;
  }
#undef RF_DBG
  RF_HIP(hipGetLastError());
  return RF_OK;
}
