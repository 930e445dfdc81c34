// Cross-encoder reranking: score (query, chunk) pairs with a BertForSequenceClassification of the
// MiniLM-L{6,12}-H384 family (cross-encoder/ms-marco-MiniLM-L-6-v2 and -L-12-v2).  The six or twelve layers
// are the sentence embedder's (encoder.hip, encoder_post.hip), unchanged; a pair forward differs in the launch
// that opens it and the launch that closes it (rf_pair_ends, encoder_internal.h):
//   k_embed_pair_ln  k_embed_ln with the token-type row chosen per position: row 1 from seg[b] on
//   k_cls_head       logit = wc . tanh(Wp x + bp) + bc on the final hidden row x of the [CLS] token
#include "encoder_internal.h"

__global__ void __launch_bounds__(256) k_embed_pair_ln(
    const int32_t* __restrict__ ids, const int32_t* __restrict__ lens, const int32_t* __restrict__ seg,
    int32_t* __restrict__ tok_off, int B, int T, int vocab, const _Float16* __restrict__ word,
    const _Float16* __restrict__ pos, const _Float16* __restrict__ type, const _Float16* __restrict__ g,
    const _Float16* __restrict__ b, float eps, _Float16* __restrict__ out) {
  embed_ln_rows<true>(ids, lens, seg, tok_off, B, T, vocab, word, pos, type, g, b, eps, out);
}

// CH_SEQ sequences per workgroup, so the 288 KB pooler matrix is streamed once per CH_SEQ sequences (from L2
// after the first workgroup); thread j owns pooler output j of every sequence of the group.
//   x      the [CLS] rows as fp32 in LDS (a wave reads them as broadcasts)
//   y[j]   = fma chain over k = 0 .. 383 ascending from 0.f of Wp[j][k] * x[k], then + bp[j]; t[j] = tanhf(y[j])
//   logit  = lane l of one wave: fma chain over j = l, l + 64, .. l + 320 ascending from 0.f of wc[j] * t[j];
//            the 64 lanes meet in the xor-shuffle tree 32, 16, 8, 4, 2, 1; then + bc
// None of it depends on the sequence's slot in the group or its place in the batch: the same pair gives the
// same bits wherever it sits.  A sequence without tokens has no [CLS] row: its logit is -inf and no row is read.
#define CH_SEQ 16
#define CH_THREADS HID
__global__ void __launch_bounds__(CH_THREADS) k_cls_head(
    const _Float16* __restrict__ x, const int32_t* __restrict__ tok_off, int B,
    const _Float16* __restrict__ pool_w, const _Float16* __restrict__ pool_b,
    const _Float16* __restrict__ cls_w, const _Float16* __restrict__ cls_b, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float xs[CH_SEQ][HID];   // the [CLS] rows, then the tanh outputs
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * CH_SEQ;
  // 48 16-byte slots per row: slot c = features 8 c .. 8 c + 7 of the tiled activations
  for (int i = tid; i < CH_SEQ * (HID / 8); i += CH_THREADS) {
    const int s = i / (HID / 8), c = i % (HID / 8);
    const int b = b0 + s;
    half8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.f;
    if (b < B) {
      const int tok = tok_off[b];
      if (tok_off[b + 1] - tok >= 1) v = *(const half8*)(x + toff(tok, 8 * c, HID / 16));
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) xs[s][8 * c + j] = (float)v[j];
  }
  __syncthreads();
  float acc[CH_SEQ];
#pragma unroll
  for (int s = 0; s < CH_SEQ; ++s) acc[s] = 0.f;
  const _Float16* wrow = pool_w + (size_t)tid * HID;
#pragma unroll 2
  for (int k = 0; k < HID; k += 8) {
    const half8 w = *(const half8*)(wrow + k);
#pragma unroll
    for (int s = 0; s < CH_SEQ; ++s) {
      const float4 x0 = *(const float4*)&xs[s][k];
      const float4 x1 = *(const float4*)&xs[s][k + 4];
      acc[s] = fmaf((float)w[0], x0.x, acc[s]);
      acc[s] = fmaf((float)w[1], x0.y, acc[s]);
      acc[s] = fmaf((float)w[2], x0.z, acc[s]);
      acc[s] = fmaf((float)w[3], x0.w, acc[s]);
      acc[s] = fmaf((float)w[4], x1.x, acc[s]);
      acc[s] = fmaf((float)w[5], x1.y, acc[s]);
      acc[s] = fmaf((float)w[6], x1.z, acc[s]);
      acc[s] = fmaf((float)w[7], x1.w, acc[s]);
    }
  }
  const float bp = (float)pool_b[tid];
  __syncthreads();   // every thread has read the rows: the buffer now takes the tanh outputs
#pragma unroll
  for (int s = 0; s < CH_SEQ; ++s) xs[s][tid] = tanhf(acc[s] + bp);
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  float wc[HID / 64];
#pragma unroll
  for (int i = 0; i < HID / 64; ++i) wc[i] = (float)cls_w[lane + 64 * i];
  const float bc = (float)cls_b[0];
  for (int s = wave; s < CH_SEQ; s += CH_THREADS / 64) {   // wave-uniform
    const int b = b0 + s;
    if (b >= B) break;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < HID / 64; ++i) v = fmaf(wc[i], xs[s][lane + 64 * i], v);
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) out[b] = (tok_off[b + 1] - tok_off[b] >= 1) ? v + bc : -INFINITY;
  }
}

void rf_launch_embed_pair(const int32_t* ids, const int32_t* lens, const int32_t* seg, int32_t* tok_off, int B, int T,
                          const rf_encoder_config& c, const rf_encoder_weights& w, _Float16* out, hipStream_t st) {
  const int chunks = B * ((T + 31) / 32);   // one workgroup per 32 positions of a row
  hipLaunchKernelGGL(k_embed_pair_ln, dim3(chunks), dim3(256), 0, st, ids, lens, seg, tok_off, B, T, c.vocab_size,
                     (const _Float16*)w.word_emb, (const _Float16*)w.pos_emb, (const _Float16*)w.type_emb,
                     (const _Float16*)w.emb_ln_g, (const _Float16*)w.emb_ln_b, c.ln_eps, out);
}

void rf_launch_cls_head(const _Float16* x, const int32_t* tok_off, int B, const rf_pair_head& head, float* logits,
                        hipStream_t st) {
  hipLaunchKernelGGL(k_cls_head, dim3((B + CH_SEQ - 1) / CH_SEQ), dim3(CH_THREADS), 0, st, x, tok_off, B,
                     (const _Float16*)head.pool_w, (const _Float16*)head.pool_b, (const _Float16*)head.cls_w,
                     (const _Float16*)head.cls_b, logits);
}

extern "C" int rf_score_pairs(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev,
                              const int32_t* seg_dev, int B, int T, const rf_pair_head* head, float* logits_dev,
                              void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!enc || !ids_dev || !lens_dev || !seg_dev || !head || !logits_dev || !workspace_dev) {
    rf_set_error("rf_score_pairs: null argument");
    return RF_ERR_INVALID;
  }
  if (head->num_labels != 1) {
    rf_set_error("rf_score_pairs: num_labels=%d (one relevance logit per pair is supported)", head->num_labels);
    return RF_ERR_UNSUPPORTED;
  }
  const void* const ptrs[4] = {head->pool_w, head->pool_b, head->cls_w, head->cls_b};
  for (int i = 0; i < 4; ++i)
    if (!ptrs[i] || ((uintptr_t)ptrs[i] & (i == 0 ? 15 : 1))) {
      rf_set_error("rf_score_pairs: head pointer %d null or misaligned (pool_w: 16 bytes)", i);
      return RF_ERR_INVALID;
    }
  return rf_encode_pairs(enc, ids_dev, lens_dev, B, T, rf_pair_ends{seg_dev, head, logits_dev}, workspace_dev,
                         workspace_bytes, (hipStream_t)stream);
}
