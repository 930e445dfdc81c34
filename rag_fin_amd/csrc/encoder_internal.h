// Declarations shared by the encoder's translation units (encoder.hip, encoder_post.hip).
#pragma once
#include "rf_internal.h"
#include "lds_ring.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define HID 384
#define HEAD_DIM 32

// Activations live in the same fragment tiling as the corpus and the weights:
// [token block of 32][k-step = feature/16][lane = 32*((feature/8)&1) + token%32][8 halfs].
// A 32-token x 16-feature fragment is 1 KiB contiguous, so the GEMMs read their B
// operands with one coalesced wave load, and an epilogue's 4-consecutive-feature
// stores of a wave fill 512 contiguous bytes.  (Row-major activations made every
// B-fragment load touch 32 different cache lines: the GEMMs were TA-bound at ~17 %
// of the matrix peak.)  toff() = offset in halfs of (token t, feature f); KSf = width/16.
__device__ __forceinline__ size_t toff(int t, int f, int KSf) {
  return (((size_t)(t >> 5) * KSf + (f >> 4)) * 64 + (size_t)(((f >> 3) & 1) * 32 + (t & 31))) * 8 + (f & 7);
}

// ---- the embedding launch that opens a forward (k_embed_ln in encoder.hip, k_embed_pair_ln in rerank.hip) ----
// One workgroup per 32 consecutive positions of one sequence, lane = (position c, feature half h); its four
// waves take six of the 24 16-feature groups each.  The wave's stores are runs of whole 16-byte slots of the
// tiled activations (a token's slot of fragment f is next to its neighbour's: 512 contiguous bytes per half,
// split at most once by a token-block boundary) instead of 48 slots 1 KiB apart per token; every load of a
// wave (18 x 16 bytes per lane) is in flight at once and its 48 sums stay in registers; the LayerNorm sums are
// lane-local plus one xor-32 exchange and one trip through LDS between the four waves.  The per-sequence
// scalars (length, packed offset) are wave-uniform scalar loads.  (Round-2 history: one wave per token, four
// tokens per wave in a row, each a chain of three dependent vector loads: 49 us per 64 k-token batch; one wave
// per 32 positions with two sweeps over the rows: 56 us -- 8 waves per CU cannot hide the latency.)
template <bool PAIR>   // PAIR: seg[b] = index of the first segment-1 position of sequence b (>= its length: none)
__device__ __forceinline__ void embed_ln_rows(
    const int32_t* __restrict__ ids, const int32_t* __restrict__ lens, const int32_t* __restrict__ seg,
    int32_t* __restrict__ tok_off, int B, int T, int vocab, const _Float16* __restrict__ word,
    const _Float16* __restrict__ pos, const _Float16* __restrict__ type, const _Float16* __restrict__ g,
    const _Float16* __restrict__ b, float eps, _Float16* __restrict__ out) {
  __shared__ float red[2][4][32];
  constexpr int FW = HID / 16 / 4;                             // feature groups per wave (6)
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int cpr = (T + 31) >> 5;                               // 32-position chunks per sequence row
  const int bi = blockIdx.x / cpr, p0 = (blockIdx.x % cpr) * 32;
  const int len = min(max(lens[bi], 0), T);
  // ONE sequence (a query): the packed offsets are {0, len} -- written here, so that the launch of k_tok_offsets
  // (a dependent kernel boundary, ~4.5 us of the query's latency) is not needed
  if (B == 1 && blockIdx.x == 0 && threadIdx.x == 0) {
    tok_off[0] = 0;
    tok_off[1] = len;
  }
  if (p0 >= len) return;                                       // workgroup-uniform
  const int p = p0 + c;
  const bool live = p < len;
  int id = live ? ids[(size_t)bi * T + p] : 0;
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const int f0 = 16 * FW * wave + 8 * h;                       // the lane's first feature
  const _Float16* wrow = word + (size_t)id * HID + f0;
  const _Float16* prow = pos + (size_t)(live ? p : 0) * HID + f0;
  // PAIR: positions from seg[bi] on belong to the second segment and take type row 1 (a per-lane choice
  // between two rows; the arithmetic below is the same)
  const _Float16* trow = type + f0;
  if constexpr (PAIR) trow += (p >= seg[bi]) ? HID : 0;
  half8 a[FW], cc[FW], d[FW];
#pragma unroll
  for (int f = 0; f < FW; ++f) {
    a[f] = *(const half8*)(wrow + 16 * f);
    cc[f] = *(const half8*)(prow + 16 * f);
    d[f] = *(const half8*)(trow + 16 * f);
  }
  float v[FW][8];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int f = 0; f < FW; ++f)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[f][j] = (float)a[f][j] + (float)cc[f][j] + (float)d[f][j];
      s1 += v[f][j];
      s2 = fmaf(v[f][j], v[f][j], s2);
    }
  s1 += __shfl_xor(s1, 32);
  s2 += __shfl_xor(s2, 32);
  if (h == 0) {
    red[0][wave][c] = s1;
    red[1][wave][c] = s2;
  }
  // the scale and shift are not needed before the statistics: their round trip sits under the exchange
  half8 gg[FW], bb[FW];
#pragma unroll
  for (int f = 0; f < FW; ++f) {
    gg[f] = *(const half8*)(g + f0 + 16 * f);
    bb[f] = *(const half8*)(b + f0 + 16 * f);
  }
  __syncthreads();
  const float t1 = (red[0][0][c] + red[0][1][c]) + (red[0][2][c] + red[0][3][c]);
  const float t2 = (red[1][0][c] + red[1][1][c]) + (red[1][2][c] + red[1][3][c]);
  const float mu = t1 * (1.f / HID);
  // E[v^2] - mu^2 in fp32 over 384 values of order 1 with |mu| << 1: the cancellation is ~1e-6 relative
  const float rstd = rsqrtf(fmaxf(t2 * (1.f / HID) - mu * mu, 0.f) + eps);
  const int token = (B == 1 ? 0 : tok_off[bi]) + p;
  _Float16* orow = out + ((size_t)(token >> 5) * (HID / 16) * 64 + (size_t)h * 32 + (token & 31)) * 8 + (size_t)(FW * wave) * 512;
#pragma unroll
  for (int f = 0; f < FW; ++f) {
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (_Float16)((v[f][j] - mu) * rstd * (float)gg[f][j] + (float)bb[f][j]);
    if (live) *(half8*)(orow + (size_t)f * 512) = o;
  }
}


// (the attribute means something in the device pass only; the host pass of the same source would warn)
#ifdef __HIP_DEVICE_COMPILE__
#define RF_NO_PACKED_FP32 __attribute__((target("no-packed-fp32-ops")))
#else
#define RF_NO_PACKED_FP32
#endif

// ---- encoder_post.hip: the layer's post-attention half in one launch ---------------------
// out-projection + residual + LayerNorm, FFN1 + GELU, FFN2 + residual + LayerNorm for 128 tokens per
// workgroup; the activations between the three GEMMs never leave the registers.
#define PB_STEPS_A 6    // ring steps of the out-projection: 12 feature blocks, two per step
#define PB_STEPS_B 50   // ring steps of the MLP part: 48 intermediate blocks + 2 of pipeline drain
#define PB_FRAGS 48     // 1-KiB fragments per ring step
#define PB_PARAM_FRAGS 15   // fp32 parameter block: b1 [1536], bo, g1, be1, b2, g2, be2 [384 each] = 15 KiB
#define PB_STEPS_C 18   // ring steps of the NEXT layer's QKV projection: 36 feature blocks, two per step
#define PB_QB_FRAGS 8   // the next layer's QKV bias as fp32 [1152] (4.5 KiB), padded
// per-layer pack the kernel reads: [parameters, padded to 16 fragments][out-projection 288][MLP stream 2400]
// [QKV of the next layer 864][its bias 8]
#define PB_RING_FRAGS ((PB_STEPS_A + PB_STEPS_B + PB_STEPS_C) * PB_FRAGS)
#define PB_PACK_FRAGS (16 + PB_RING_FRAGS + PB_QB_FRAGS)
static inline size_t rf_post_pack_elems(void) { return (size_t)PB_PACK_FRAGS * 512; }   // halfs per layer
// row-major weights / biases of all L layers -> pack [L][PB_PACK_FRAGS][64 lanes][16 B]
void rf_launch_post_pack_build(const rf_encoder_weights* w, void* pack, int L, hipStream_t st);
struct rf_post_args {
  const _Float16* ctx;      // [Mpad, 384] tiled: attention output
  const _Float16* res;      // [Mpad, 384] tiled: the layer's input (residual of the first LayerNorm)
  _Float16* out;            // [Mpad, 384] tiled: the layer's output
  _Float16* qkv_out;        // [Mpad, 1152] tiled: Q | K | V of the NEXT layer (its weights are in this layer's pack), or nullptr
  const uint4* pack;        // this layer's pack (rf_launch_post_pack_build)
  float eps;
  const int32_t* m_ptr;     // packed token count
  float* dbg;               // clock stamps (experiments build), or nullptr
  int abl;                  // ablation bits (experiments build; results wrong): see k_post_block
};
int rf_launch_post_block(const rf_post_args& a, int token_slots, hipStream_t st);

// ---- rerank.hip: a cross-encoder forward = the same layers between two other launches -----------------
// encode_enqueue's option: which embedding launch opens the forward and which launch closes it.  nullptr is
// the sentence embedder (k_embed_ln ... k_pool_norm); with it the forward opens with k_embed_pair_ln (segment
// ids) and closes with k_cls_head (pooler + classifier on the [CLS] row) instead.  The layer loop is the same.
// A second pair of ends (reader.hip): with `qa` set the forward closes with k_qa_spans (QA head + span search on
// every row of the pair) instead of k_cls_head; `head` and `logits` are then unused.
struct rf_pair_ends {
  const int32_t* seg;         // [B] first segment-1 position per sequence
  const rf_pair_head* head;   // device pointers of the classification head
  float* logits;              // [B]
  const rf_qa_head* qa;       // device pointers of the span head, or nullptr: the classification head closes
  int max_answer_len, n_best;
  rf_span* spans;             // [B, n_best]
  float* norm;                // [B, 3]
  float* qa_logits;           // [B, T, 2] or nullptr
  const struct rf_terms_end* terms;   // a third pair of ends (splade.hip), or nullptr: see below
  const struct rf_tokens_end* tokens; // a fourth pair of ends (late_interaction.hip), or nullptr: see below
  const struct rf_tags_end* tags;     // a fifth pair of ends (tagger.hip), or nullptr: see below
  const struct rf_sentence_end* sentence;   // a sixth pair of ends (sentence_head.hip), or nullptr: see below
};
void rf_launch_embed_pair(const int32_t* ids, const int32_t* lens, const int32_t* seg, int32_t* tok_off, int B, int T,
                          const rf_encoder_config& c, const rf_encoder_weights& w, _Float16* out, hipStream_t st);
void rf_launch_cls_head(const _Float16* x, const int32_t* tok_off, int B, const rf_pair_head& head, float* logits,
                        hipStream_t st);
void rf_launch_qa_spans(const _Float16* x, const int32_t* tok_off, int B, int T, const rf_pair_ends& ends,
                        hipStream_t st);
// ---- splade.hip: a term forward = the same layers between the embedder's embedding launch and an MLM head ---------
// With `terms` set in rf_pair_ends the forward opens with k_embed_ln (token types 0: `seg` is not read and the
// encoder needs no second token-type row) and closes with k_mlm_transform + k_mlm_decode_max; the other fields
// are unused.
struct rf_terms_end {
  const rf_mlm_head* head;    // device pointers of the masked-language-model head
  float* weights;             // [B, vocab]
  _Float16* g;                // [ceil32(B * T), 384] tiled: the transformed tokens (workspace)
};
void rf_launch_terms_head(const _Float16* x, const int32_t* tok_off, int B, int T, const rf_terms_end& e, float eps,
                          hipStream_t st);
// ---- late_interaction.hip: a token forward = the same layers between the embedder's embedding launch and a projection --
// With `tokens` set in rf_pair_ends the forward opens with k_embed_ln (token types 0, as for `terms`) and closes
// with k_token_offsets + k_token_project; the other fields are unused.
struct rf_tokens_end {
  const rf_token_head* head;  // device pointers of the projection and the skip bitmap
  int32_t* out_off;           // [B + 1]
  _Float16* out_vec;          // [<= B * T, dim]
};
void rf_launch_tokens_head(const _Float16* x, const int32_t* tok_off, const int32_t* ids, const int32_t* lens, int B,
                           int T, const rf_tokens_end& e, hipStream_t st);
// ---- tagger.hip: a tag forward = the same layers between the embedder's embedding launch and a token classifier ------
// With `tags` set in rf_pair_ends the forward opens with k_embed_ln (token types 0, as for `terms`) and closes
// with k_tag_logits; the other fields are unused.
struct rf_tags_end {
  const rf_tag_head* head;    // device pointers of the classifier
  float* logits;              // [B, T, num_labels]
};
void rf_launch_tags_head(const _Float16* x, const int32_t* tok_off, int B, int T, const rf_tags_end& e, hipStream_t st);
// ---- sentence_head.hip: a sentence forward = rf_encode's launches with another pooling launch at the end ------------
// With `sentence` set in rf_pair_ends the forward opens with k_embed_ln (token types 0, as for `terms`), runs the
// layer loop exactly as rf_encode does (the single-query launch included) and closes with k_sentence_head where
// k_pool_norm is launched otherwise; the other fields are unused.
struct rf_sentence_end {
  rf_sentence_head head;      // pooling mode and whether to normalise (host values)
  const int32_t* skip;        // [B] leading tokens left out of the pooled set, or nullptr: none
  _Float16* out16;            // [B, 384] or nullptr
  float* out32;               // [B, 384] or nullptr
};
void rf_launch_sentence_head(const _Float16* x, const int32_t* tok_off, const int32_t* skip, int B, int T,
                             const rf_sentence_head& head, _Float16* out16, float* out32, hipStream_t st);
const rf_encoder_config& rf_encoder_cfg(const rf_encoder_t* enc);   // encoder.hip
// encoder.hip: argument checks of rf_encode + the plain launch sequence with `ends` (never a cached hipGraph);
// `who` names the public entry in the error text
int rf_encode_pairs(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev, int B, int T,
                    const rf_pair_ends& ends, void* workspace_dev, size_t workspace_bytes, hipStream_t st,
                    const char* who = "rf_score_pairs");
