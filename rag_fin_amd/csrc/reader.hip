// Extractive reader: answer spans of (question, chunk) pairs with a BertForQuestionAnswering of the
// MiniLM-L{6,12}-H384 family (e.g. deepset/minilm-uncased-squad2).  The layers and the pair embedding launch are
// the cross-encoder's (rerank.hip); the forward closes with one launch, one workgroup per pair:
//   k_qa_spans   s[t], e[t] = qa_w[0] . x_t + qa_b[0], qa_w[1] . x_t + qa_b[1] on every final hidden row of the pair,
//                the two log-sum-exps over [CLS] + context, and the best n_best spans (i, j) by s[i] + e[j]
// One launch instead of "logits over the packed tokens, then a span search": the logits never leave the CU (LDS),
// no scratch beyond the encoder's workspace is needed, and a pair's 2 x 384-term dots are one coalesced pass over
// its rows (lane = token: the 16-byte slots of consecutive tokens are consecutive in the tiled activations).
#include "encoder_internal.h"
#include "reader_internal.h"   // RD_THREADS, RD_NONE, rd_better, rd_next: shared with reader_windows.hip

// Every number below is a function of the pair's own rows, seg and length alone:
//   s[t], e[t]  fma chain over k = 0 .. 383 ascending from 0.f of w[k] * x_t[k], then + bias (one fp32 add)
//   z           s[i] + e[j], one fp32 add
//   lse         max m over the set (exact), then sum of exp(v - m) in fp64: lane-local term, the xor-shuffle tree
//               32, 16, 8, 4, 2, 1 of a wave, the 8 wave sums ascending; m + log(sum) in fp64, rounded to fp32 once
// so the same pair gives the same bits at any place of any batch.  No atomics; the n_best rounds pick the maximum
// of a strict total order, which does not depend on the tree that finds it.
__global__ void __launch_bounds__(RD_THREADS) k_qa_spans(
    const _Float16* __restrict__ x, const int32_t* __restrict__ tok_off, const int32_t* __restrict__ seg, int T,
    const _Float16* __restrict__ qa_w, const _Float16* __restrict__ qa_b, int max_len, int n_best,
    rf_span* __restrict__ spans, float* __restrict__ norm, float* __restrict__ logits) {
  __shared__ __attribute__((aligned(16))) float wf[2][HID];
  __shared__ float sl[RD_THREADS], el[RD_THREADS];
  __shared__ float red_f[2][2][RD_WAVES];
  __shared__ double red_d[2][RD_WAVES];
  __shared__ int red_k[2][RD_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int tok0 = tok_off[b];
  const int len = min(tok_off[b + 1] - tok0, RD_THREADS);   // (the host refuses T > RD_THREADS)
  rf_span* out = spans + (size_t)b * n_best;
  if (len < 1) {   // no [CLS] row (workgroup-uniform): nothing is read
    if (tid < n_best) out[tid] = rf_span{-1, -1, -INFINITY};
    if (tid < 3) norm[(size_t)b * 3 + tid] = -INFINITY;
    return;
  }
  for (int i = tid; i < 2 * HID; i += RD_THREADS) (&wf[0][0])[i] = (float)qa_w[i];
  __syncthreads();

  // ---- the logits of position t = tid ----
  float sv = -INFINITY, ev = -INFINITY;
  if (tid < len) {
    const int tok = tok0 + tid;
    float as = 0.f, ae = 0.f;
#pragma unroll 8
    for (int c = 0; c < HID / 8; ++c) {
      const half8 v = *(const half8*)(x + toff(tok, 8 * c, HID / 16));
      const float4 s0 = *(const float4*)&wf[0][8 * c], s1 = *(const float4*)&wf[0][8 * c + 4];
      const float4 e0 = *(const float4*)&wf[1][8 * c], e1 = *(const float4*)&wf[1][8 * c + 4];
      const float ws[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
      const float we[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xv = (float)v[j];
        as = fmaf(ws[j], xv, as);
        ae = fmaf(we[j], xv, ae);
      }
    }
    sv = as + (float)qa_b[0];
    ev = ae + (float)qa_b[1];
    if (logits) {
      float* l = logits + ((size_t)b * T + tid) * 2;
      l[0] = sv;
      l[1] = ev;
    }
  }
  sl[tid] = sv;
  el[tid] = ev;

  // ---- the normalisers over {0} u [lo, hi] ----
  const int lo = max(seg[b], 0), hi = len - 2;
  const bool in_set = tid < len && (tid == 0 || (tid >= lo && tid <= hi));
  float ms = in_set ? sv : -INFINITY, me = in_set ? ev : -INFINITY;
  for (int o = 32; o > 0; o >>= 1) {
    ms = fmaxf(ms, __shfl_xor(ms, o));
    me = fmaxf(me, __shfl_xor(me, o));
  }
  if (lane == 0) {
    red_f[0][0][wave] = ms;
    red_f[0][1][wave] = me;
  }
  __syncthreads();   // (also: sl / el are complete)
  ms = red_f[0][0][0];
  me = red_f[0][1][0];
#pragma unroll
  for (int w = 1; w < RD_WAVES; ++w) {
    ms = fmaxf(ms, red_f[0][0][w]);
    me = fmaxf(me, red_f[0][1][w]);
  }
  double ds = in_set ? exp((double)sv - (double)ms) : 0.0;
  double de = in_set ? exp((double)ev - (double)me) : 0.0;
  for (int o = 32; o > 0; o >>= 1) {
    ds += __shfl_xor(ds, o);
    de += __shfl_xor(de, o);
  }
  if (lane == 0) {
    red_d[0][wave] = ds;
    red_d[1][wave] = de;
  }
  __syncthreads();
  if (tid == 0) {
    double ts = red_d[0][0], te = red_d[1][0];
#pragma unroll
    for (int w = 1; w < RD_WAVES; ++w) {
      ts += red_d[0][w];
      te += red_d[1][w];
    }
    norm[(size_t)b * 3 + 0] = sl[0] + el[0];
    norm[(size_t)b * 3 + 1] = (float)((double)ms + log(ts));
    norm[(size_t)b * 3 + 2] = (float)((double)me + log(te));
  }

  // ---- the best n_best spans: thread = candidate start lo + tid, holding the best span it has not given yet ----
  const int i = lo + tid;
  const bool starts = i <= hi;
  const int jmax = min(i + max_len - 1, hi);
  const float si = starts ? sl[i] : 0.f;
  float bz = -INFINITY;
  int bk = starts ? rd_next(el, si, i, jmax, INFINITY, -1, &bz) : RD_NONE;
  int r = 0;
  for (; r < n_best; ++r) {
    float z = bz;
    int k = bk;
    for (int o = 32; o > 0; o >>= 1) {
      const float zo = __shfl_xor(z, o);
      const int ko = __shfl_xor(k, o);
      if (rd_better(zo, ko, z, k)) {
        z = zo;
        k = ko;
      }
    }
    // two buffers by the round's parity: a round's writes cannot meet the reads of the round before last,
    // which every thread left before the barrier of the round between
    if (lane == 0) {
      red_f[1][r & 1][wave] = z;
      red_k[r & 1][wave] = k;
    }
    __syncthreads();
    z = red_f[1][r & 1][0];
    k = red_k[r & 1][0];
#pragma unroll
    for (int w = 1; w < RD_WAVES; ++w) {
      const float zo = red_f[1][r & 1][w];
      const int ko = red_k[r & 1][w];
      if (rd_better(zo, ko, z, k)) {
        z = zo;
        k = ko;
      }
    }
    if (k == RD_NONE) break;   // workgroup-uniform: every thread read the same eight entries
    const int wi = k >> 6, wj = wi + (k & 63);
    if (tid == 0) out[r] = rf_span{wi, wj, z};
    if (starts && wi == i) bk = rd_next(el, si, i, jmax, z, wj, &bz);   // the winner's owner moves on
  }
  if (tid >= r && tid < n_best) out[tid] = rf_span{-1, -1, -INFINITY};
}

void rf_launch_qa_spans(const _Float16* x, const int32_t* tok_off, int B, int T, const rf_pair_ends& ends,
                        hipStream_t st) {
  hipLaunchKernelGGL(k_qa_spans, dim3(B), dim3(RD_THREADS), 0, st, x, tok_off, ends.seg, T,
                     (const _Float16*)ends.qa->qa_w, (const _Float16*)ends.qa->qa_b, ends.max_answer_len, ends.n_best,
                     ends.spans, ends.norm, ends.qa_logits);
}

extern "C" int rf_answer_spans(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev,
                               const int32_t* seg_dev, int B, int T, const rf_qa_head* head, int max_answer_len,
                               int n_best, rf_span* spans_dev, float* norm_dev, float* logits_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!enc || !ids_dev || !lens_dev || !seg_dev || !head || !spans_dev || !norm_dev || !workspace_dev) {
    rf_set_error("rf_answer_spans: null argument");
    return RF_ERR_INVALID;
  }
  if (n_best < 1 || n_best > RF_READER_MAX_BEST || max_answer_len < 1 || max_answer_len > RF_READER_MAX_SPAN) {
    rf_set_error("rf_answer_spans: n_best=%d (1..%d) or max_answer_len=%d (1..%d) out of range", n_best,
                 RF_READER_MAX_BEST, max_answer_len, RF_READER_MAX_SPAN);
    return RF_ERR_INVALID;
  }
  if (!head->qa_w || ((uintptr_t)head->qa_w & 15) || !head->qa_b || ((uintptr_t)head->qa_b & 1)) {
    rf_set_error("rf_answer_spans: head pointer null or misaligned (qa_w: 16 bytes)");
    return RF_ERR_INVALID;
  }
  if (T > RD_THREADS) {
    rf_set_error("rf_answer_spans: T=%d exceeds the %d positions the span stage holds", T, RD_THREADS);
    return RF_ERR_UNSUPPORTED;
  }
  rf_pair_ends ends{};
  ends.seg = seg_dev;
  ends.qa = head;
  ends.max_answer_len = max_answer_len;
  ends.n_best = n_best;
  ends.spans = spans_dev;
  ends.norm = norm_dev;
  ends.qa_logits = logits_dev;
  return rf_encode_pairs(enc, ids_dev, lens_dev, B, T, ends, workspace_dev, workspace_bytes, (hipStream_t)stream,
                         "rf_answer_spans");
}
