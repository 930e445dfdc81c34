// Entity tagging: the labels of a BertForTokenClassification of the MiniLM-L{6,12}-H384 family over single-segment
// rows, and their BIO grouping into entities.  The layers and the embedding launch are the embedder's
// (encoder.hip); a tag forward closes with one launch of this file (rf_tags_end, encoder_internal.h):
//   k_tag_logits       l[t][c] = cls_w[c] . x_t + cls_b[c] on every final hidden row: thread = token, the
//                      classifier's rows in LDS, the row's 384 features read once
// The decode is a launch of its own (rf_group_entities), so that it also runs on logits no forward produced:
//   k_group_entities   one workgroup per row, thread = position: label and score per token, unit starts, group
//                      starts and surviving groups as three 512-bit masks in LDS, one lane per group for its sum
#include <math.h>

#include "encoder_internal.h"

// ---- the classifier ---------------------------------------------------------------------------------------------
// Every logit is a function of its token's hidden row alone:
//   l[t][c]  fma chain over k = 0 .. 383 ascending from 0.f of cls_w[c][k] * x_t[k], then + cls_b[c] (one fp32 add)
// so a row gives the same bits at any place of any batch.  NC = ceil(L / 8) picks the instantiation: 8 NC
// accumulators per thread, the rows L .. 8 NC - 1 of the LDS image are zero and never written out.
#define TL_THREADS 128
template <int NC>
__global__ void __launch_bounds__(TL_THREADS) k_tag_logits(const _Float16* __restrict__ x,
                                                           const int32_t* __restrict__ tok_off, int T,
                                                           const _Float16* __restrict__ cls_w,
                                                           const _Float16* __restrict__ cls_b, int L,
                                                           float* __restrict__ logits) {
  __shared__ __attribute__((aligned(16))) _Float16 wl[8 * NC][HID];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, t0 = blockIdx.x * TL_THREADS;
  const int tok0 = tok_off[b];
  const int len = min(tok_off[b + 1] - tok0, T);
  if (t0 >= len) return;                                            // workgroup-uniform
  for (int i = tid; i < 8 * NC * (HID / 8); i += TL_THREADS) {
    const int c = i / (HID / 8), k8 = i % (HID / 8);
    half8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.f;
    if (c < L) v = *(const half8*)(cls_w + (size_t)c * HID + 8 * k8);
    *(half8*)&wl[c][8 * k8] = v;
  }
  __syncthreads();
  const int t = t0 + tid;
  if (t >= len) return;
  float acc[8 * NC];
#pragma unroll
  for (int c = 0; c < 8 * NC; ++c) acc[c] = 0.f;
#pragma unroll 2
  for (int k8 = 0; k8 < HID / 8; ++k8) {
    const half8 v = *(const half8*)(x + toff(tok0 + t, 8 * k8, HID / 16));
    float xv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) xv[j] = (float)v[j];
#pragma unroll
    for (int c = 0; c < 8 * NC; ++c) {
      const half8 w = *(const half8*)&wl[c][8 * k8];               // one address per wave: a broadcast
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[c] = fmaf((float)w[j], xv[j], acc[c]);
    }
  }
  float* out = logits + ((size_t)b * T + t) * L;
#pragma unroll
  for (int c = 0; c < 8 * NC; ++c)
    if (c < L) out[c] = acc[c] + (float)cls_b[c];
}

template <int NC>
static void tag_logits_launch(const _Float16* x, const int32_t* tok_off, int B, int T, const rf_tags_end& e,
                              hipStream_t st) {
  hipLaunchKernelGGL(k_tag_logits<NC>, dim3((T + TL_THREADS - 1) / TL_THREADS, B), dim3(TL_THREADS), 0, st, x, tok_off,
                     T, (const _Float16*)e.head->cls_w, (const _Float16*)e.head->cls_b, e.head->num_labels, e.logits);
}

void rf_launch_tags_head(const _Float16* x, const int32_t* tok_off, int B, int T, const rf_tags_end& e, hipStream_t st) {
  switch ((e.head->num_labels + 7) / 8) {
    case 1: tag_logits_launch<1>(x, tok_off, B, T, e, st); break;
    case 2: tag_logits_launch<2>(x, tok_off, B, T, e, st); break;
    case 3: tag_logits_launch<3>(x, tok_off, B, T, e, st); break;
    case 4: tag_logits_launch<4>(x, tok_off, B, T, e, st); break;
    case 5: tag_logits_launch<5>(x, tok_off, B, T, e, st); break;
    case 6: tag_logits_launch<6>(x, tok_off, B, T, e, st); break;
    case 7: tag_logits_launch<7>(x, tok_off, B, T, e, st); break;
    default: tag_logits_launch<8>(x, tok_off, B, T, e, st); break;
  }
}

extern "C" int rf_tag_logits(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev, int B, int T,
                             const rf_tag_head* head, float* logits_dev, void* workspace_dev, size_t workspace_bytes,
                             void* stream) {
  if (!enc || !ids_dev || !lens_dev || !head || !logits_dev || !workspace_dev || !head->cls_w || !head->cls_b) {
    rf_set_error("rf_tag_logits: null argument");
    return RF_ERR_INVALID;
  }
  if (((uintptr_t)head->cls_w & 15) || ((uintptr_t)head->cls_b & 1) ||
      (((uintptr_t)ids_dev | (uintptr_t)lens_dev | (uintptr_t)logits_dev) & 3)) {
    rf_set_error("rf_tag_logits: misaligned pointer (cls_w: 16 bytes; ids, lens, logits: 4)");
    return RF_ERR_INVALID;
  }
  if (B < 1 || T < 1 || (int64_t)B * T > INT32_MAX) {
    rf_set_error("rf_tag_logits: B=%d T=%d out of range", B, T);
    return RF_ERR_INVALID;
  }
  if (head->num_labels < 1 || head->num_labels > RF_TAGGER_MAX_LABELS) {
    rf_set_error("rf_tag_logits: num_labels=%d is outside 1..%d", head->num_labels, RF_TAGGER_MAX_LABELS);
    return RF_ERR_UNSUPPORTED;
  }
  if (T > 512) {
    rf_set_error("rf_tag_logits: T=%d exceeds the 512 positions rf_group_entities holds", T);
    return RF_ERR_UNSUPPORTED;
  }
  rf_tags_end te{head, logits_dev};
  rf_pair_ends ends{};
  ends.tags = &te;
  return rf_encode_pairs(enc, ids_dev, lens_dev, B, T, ends, workspace_dev, workspace_bytes, (hipStream_t)stream,
                         "rf_tag_logits");
}

// ---- the grouping -------------------------------------------------------------------------------------------------
// Thread t owns position t of the row.  Three masks of TG_THREADS bits (one ballot word per wave) carry the
// structure: U = unit starts, G = group starts, S = group starts that survive ignore_tag.  Everything a thread
// needs from its neighbourhood is a bit search in them:
//   the unit before a unit start      the highest bit of U below t
//   the last token of a group         (the lowest bit of G above t) - 1, or the last context position
//   the output slot of a group        the number of bits of S below t
// and the group's score is summed by the thread of its first token, walking U's bits in ascending position.
// Nothing depends on which thread arrives first: integers, and fp64 sums in one written order.
#define TG_THREADS 512
#define TG_WAVES (TG_THREADS / 64)

__device__ __forceinline__ int tg_prev_bit(const uint64_t* m, int t) {          // highest set position < t, or -1
  int w = t >> 6;
  uint64_t v = m[w] & ((1ull << (t & 63)) - 1ull);
  for (;;) {
    if (v) return w * 64 + 63 - __clzll((long long)v);
    if (--w < 0) return -1;
    v = m[w];
  }
}

__device__ __forceinline__ int tg_next_bit(const uint64_t* m, int t) {          // lowest set position > t, or -1
  int w = t >> 6;
  const int l = t & 63;
  uint64_t v = l == 63 ? 0ull : (m[w] & (~0ull << (l + 1)));
  for (;;) {
    if (v) return w * 64 + __ffsll((long long)v) - 1;
    if (++w >= TG_WAVES) return -1;
    v = m[w];
  }
}

__device__ __forceinline__ int tg_rank(const uint64_t* m, int t) {              // set positions < t
  int n = 0;
  for (int w = 0; w < (t >> 6); ++w) n += __popcll(m[w]);
  return n + __popcll(m[t >> 6] & ((1ull << (t & 63)) - 1ull));
}

__global__ void __launch_bounds__(TG_THREADS) k_group_entities(
    const float* __restrict__ logits, const int32_t* __restrict__ lens, const uint8_t* __restrict__ word_start, int T,
    int L, const int32_t* __restrict__ label_tag, const uint8_t* __restrict__ label_begin, int strategy, int ignore_tag,
    int max_entities, int32_t* __restrict__ tok_label, float* __restrict__ tok_score, rf_entity* __restrict__ ent,
    int32_t* __restrict__ count) {
  __shared__ int lab[TG_THREADS];
  __shared__ float sc[TG_THREADS];
  __shared__ int ltag[RF_TAGGER_MAX_LABELS];
  __shared__ int lbeg[RF_TAGGER_MAX_LABELS];
  __shared__ uint64_t um[TG_WAVES], gm[TG_WAVES], sm[TG_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int len = min(max(lens[b], 0), T);                         // (the host refuses T > TG_THREADS)
  const int hi = len - 2;                                          // the last context position
  if (tid < RF_TAGGER_MAX_LABELS) {
    const int c = min(tid, L - 1);
    ltag[tid] = label_tag[c];
    lbeg[tid] = label_begin[c] != 0;
  }

  // ---- label and score of position t = tid ----
  const bool ctx = tid >= 1 && tid <= hi;
  int my_lab = 0;
  float my_sc = 0.f;
  if (ctx) {
    const float* row = logits + ((size_t)b * T + tid) * L;
    float best = row[0];
    for (int c = 1; c < L; ++c) {
      const float v = row[c];
      if (v > best) {                                              // strictly: the smallest c among equals stays
        best = v;
        my_lab = c;
      }
    }
    double s = 0.0;
    for (int c = 0; c < L; ++c) s += exp((double)row[c] - (double)best);
    my_sc = (float)(1.0 / s);
    if (tok_label) tok_label[(size_t)b * T + tid] = my_lab;
    if (tok_score) tok_score[(size_t)b * T + tid] = my_sc;
  }
  lab[tid] = my_lab;
  sc[tid] = my_sc;
  const bool ustart = ctx && (strategy == RF_TAG_SIMPLE || tid == 1 || word_start[(size_t)b * T + tid] != 0);
  const uint64_t ub = __ballot(ustart);
  if (lane == 0) um[wave] = ub;
  __syncthreads();

  // ---- group starts, survivors ----
  bool gstart = false;
  int tag = -1;
  if (ustart) {
    const int p = tg_prev_bit(um, tid);
    tag = ltag[my_lab];
    gstart = p < 0 || tag != ltag[lab[p]] || lbeg[my_lab] != 0;
  }
  const bool keep = gstart && (ignore_tag == -1 || tag != ignore_tag);
  const uint64_t gb = __ballot(gstart), sb = __ballot(keep);
  if (lane == 0) {
    gm[wave] = gb;
    sm[wave] = sb;
  }
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int w = 0; w < TG_WAVES; ++w) total += __popcll(sm[w]);
  rf_entity* out = ent + (size_t)b * max_entities;

  // ---- one lane per surviving group ----
  if (keep) {
    const int slot = tg_rank(sm, tid);
    if (slot < max_entities) {
      const int nx = tg_next_bit(gm, tid);
      const int last = nx < 0 ? hi : nx - 1;
      double s = 0.0;
      int n = 0;
      for (int w = tid >> 6; w <= (last >> 6); ++w) {
        uint64_t v = um[w];
        if (w == (tid >> 6)) v &= ~0ull << (tid & 63);
        if (w == (last >> 6) && (last & 63) != 63) v &= (1ull << ((last & 63) + 1)) - 1ull;
        while (v) {
          s += (double)sc[w * 64 + __ffsll((long long)v) - 1];
          ++n;
          v &= v - 1ull;
        }
      }
      out[slot] = rf_entity{tid, last, tag, (float)(s / (double)n)};
    }
  }
  if (tid == 0) count[b] = total;
  for (int slot = min(total, max_entities) + tid; slot < max_entities; slot += TG_THREADS)
    out[slot] = rf_entity{-1, -1, -1, -INFINITY};
}

extern "C" int rf_group_entities(const float* logits_dev, const int32_t* lens_dev, const uint8_t* word_start_dev, int B,
                                 int T, int L, const int32_t* label_tag_dev, const uint8_t* label_begin_dev, int strategy,
                                 int ignore_tag, int max_entities, int32_t* tok_label_dev, float* tok_score_dev,
                                 rf_entity* ent_dev, int32_t* count_dev, void* stream) {
  if (strategy != RF_TAG_SIMPLE && strategy != RF_TAG_FIRST) {
    rf_set_error("rf_group_entities: strategy=%d is neither RF_TAG_SIMPLE nor RF_TAG_FIRST", strategy);
    return RF_ERR_INVALID;
  }
  if (!logits_dev || !lens_dev || !label_tag_dev || !label_begin_dev || !ent_dev || !count_dev ||
      (strategy == RF_TAG_FIRST && !word_start_dev)) {
    rf_set_error("rf_group_entities: null argument");
    return RF_ERR_INVALID;
  }
  if (B < 1 || T < 1 || T > TG_THREADS || L < 1 || L > RF_TAGGER_MAX_LABELS) {
    rf_set_error("rf_group_entities: B=%d, T=%d (1..%d) or L=%d (1..%d) out of range", B, T, TG_THREADS, L,
                 RF_TAGGER_MAX_LABELS);
    return RF_ERR_INVALID;
  }
  if (max_entities < 1 || max_entities > RF_TAGGER_MAX_ENTITIES) {
    rf_set_error("rf_group_entities: max_entities=%d is outside 1..%d", max_entities, RF_TAGGER_MAX_ENTITIES);
    return RF_ERR_INVALID;
  }
  if ((((uintptr_t)logits_dev | (uintptr_t)lens_dev | (uintptr_t)label_tag_dev | (uintptr_t)tok_label_dev |
        (uintptr_t)tok_score_dev | (uintptr_t)ent_dev | (uintptr_t)count_dev) & 3)) {
    rf_set_error("rf_group_entities: misaligned pointer");
    return RF_ERR_INVALID;
  }
  hipLaunchKernelGGL(k_group_entities, dim3(B), dim3(TG_THREADS), 0, (hipStream_t)stream, logits_dev, lens_dev,
                     word_start_dev, T, L, label_tag_dev, label_begin_dev, strategy, ignore_tag, max_entities,
                     tok_label_dev, tok_score_dev, ent_dev, count_dev);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
