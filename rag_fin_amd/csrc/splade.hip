// Learned sparse vectors (SPLADE): a BertForMaskedLM head over the sentence embedder's layers, max-pooled over
// the tokens of a row, and the exact selection that cuts a row to its heaviest terms.
//   weights[b, v] = log1p(relu(max_{t < lens[b]} (dec_w[v] . g_t + dec_b[v]))),  g_t = LayerNorm(gelu(tr_w x_t + tr_b))
// The layers are rf_encode's (encoder.hip, encoder_post.hip), unchanged; a term forward opens with the embedder's
// own embedding launch (token types 0) and closes with the two launches of this file (rf_terms_end,
// encoder_internal.h):
//   k_mlm_transform    g_t for every packed token, fp16, in the tiled fragment layout of toff()
//   k_mlm_decode_max   the [tokens, H] x [H, V] decoder GEMM whose logits never leave the registers: a wave keeps
//                      64 vocabulary rows of dec_w as MFMA operands, streams the token blocks of one row after
//                      the other and keeps one running max per (row, term) -- the [tokens, V] logits (1 GB for a
//                      64 x 128 batch) are never formed.  log1p(relu(.)) is monotone, and so is "+ dec_b[v]" in
//                      fp32, so both are applied once per (b, v) after the max instead of once per token.
// rf_sparsify_terms: three launches (count, offsets, select) that turn dense [B, V] weights into packed CSR.
#include <float.h>

#include "encoder_internal.h"

// ---- g_t = LayerNorm(gelu(tr_w x_t + tr_b)) ----------------------------------------------------------------------
// MT_TOK packed tokens per workgroup, thread j owns transform output j of every token of the group (k_cls_head's
// scheme: the 288 KB matrix is streamed once per MT_TOK tokens, the rows sit in LDS as fp32 and are read as
// broadcasts).
//   y[j]   = fma chain over k = 0 .. 383 ascending from 0.f of tr_w[j][k] * x[k], then + tr_b[j]
//   a[j]   = 0.5 y (1 + erf(y / sqrt 2))
//   mean, variance: a wave per token, lane l sums a[l], a[l + 64], .. a[l + 320] ascending, the 64 lanes meet in
//            the xor-shuffle tree 32 .. 1; the variance is the second pass sum (a - mean)^2 in the same order
//   g[j]   = fp16((a[j] - mean) * rstd * gamma[j] + beta[j])
// None of it depends on the token's slot in the group: the same token gives the same bits wherever it is packed.
#define MT_TOK 16
#define MT_THREADS HID
__global__ void __launch_bounds__(MT_THREADS) k_mlm_transform(
    const _Float16* __restrict__ x, const int32_t* __restrict__ m_ptr, const _Float16* __restrict__ tr_w,
    const _Float16* __restrict__ tr_b, const _Float16* __restrict__ ln_g, const _Float16* __restrict__ ln_b,
    float eps, _Float16* __restrict__ g) {
  __shared__ __attribute__((aligned(16))) float xs[MT_TOK][HID];   // the hidden rows, then a, then g
  const int tid = threadIdx.x;
  const int M = *m_ptr;                                            // packed token count
  const int t0 = blockIdx.x * MT_TOK;
  if (t0 >= M) return;                                             // workgroup-uniform
  for (int i = tid; i < MT_TOK * (HID / 8); i += MT_THREADS) {
    const int s = i / (HID / 8), c = i % (HID / 8);
    half8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.f;
    if (t0 + s < M) v = *(const half8*)(x + toff(t0 + s, 8 * c, HID / 16));
#pragma unroll
    for (int j = 0; j < 8; ++j) xs[s][8 * c + j] = (float)v[j];
  }
  __syncthreads();
  float acc[MT_TOK];
#pragma unroll
  for (int s = 0; s < MT_TOK; ++s) acc[s] = 0.f;
  const _Float16* wrow = tr_w + (size_t)tid * HID;
#pragma unroll 2
  for (int k = 0; k < HID; k += 8) {
    const half8 w = *(const half8*)(wrow + k);
#pragma unroll
    for (int s = 0; s < MT_TOK; ++s) {
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
  const float bt = (float)tr_b[tid];
  __syncthreads();   // every thread has read the rows: the buffer now takes the activations
#pragma unroll
  for (int s = 0; s < MT_TOK; ++s) {
    const float y = acc[s] + bt;
    xs[s][tid] = 0.5f * y * (1.f + erff(y * 0.70710678118654752f));
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  float gam[HID / 64], bet[HID / 64];
#pragma unroll
  for (int i = 0; i < HID / 64; ++i) {
    gam[i] = (float)ln_g[lane + 64 * i];
    bet[i] = (float)ln_b[lane + 64 * i];
  }
  for (int s = wave; s < MT_TOK; s += MT_THREADS / 64) {   // wave-uniform; a wave owns its tokens' rows from here on
    float a[HID / 64];
    float s1 = 0.f;
#pragma unroll
    for (int i = 0; i < HID / 64; ++i) {
      a[i] = xs[s][lane + 64 * i];
      s1 += a[i];
    }
    for (int o = 32; o > 0; o >>= 1) s1 += __shfl_xor(s1, o);
    const float mu = s1 * (1.f / HID);
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < HID / 64; ++i) s2 = fmaf(a[i] - mu, a[i] - mu, s2);
    for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
    const float rstd = rsqrtf(s2 * (1.f / HID) + eps);
#pragma unroll
    for (int i = 0; i < HID / 64; ++i) xs[s][lane + 64 * i] = (a[i] - mu) * rstd * gam[i] + bet[i];
  }
  __syncthreads();
  for (int i = tid; i < MT_TOK * (HID / 8); i += MT_THREADS) {
    const int s = i / (HID / 8), c = i % (HID / 8);
    if (t0 + s >= M) continue;
    half8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (_Float16)xs[s][8 * c + j];
    *(half8*)(g + toff(t0 + s, 8 * c, HID / 16)) = v;
  }
}

// ---- weights[b, v] = log1p(relu(max_t dec_w[v] . g_t + dec_b[v])) -------------------------------------------------
// Grid (vocabulary tiles of DM_VOCAB terms, groups of DM_ROWS rows).  A wave holds DM_TILES x 32 vocabulary rows
// of dec_w for its whole life as the B operands of v_mfma_f32_32x32x16_f16 (lane l: term l % 32, features
// 16 ks + 8 (l / 32) .. + 7 -- sixteen bytes of the row-major [V, H] matrix as it is, no repacking); the A
// operand is a 1-KiB fragment of the tiled activations (32 packed tokens x 16 features, one coalesced wave load).
// The 32 x 32 fp32 result has the term on the lane and the tokens in the 16 registers (token 32 tb + (i & 3) +
// 8 (i >> 2) + 4 (l / 32)), so the max over tokens is 16 fmaxf per lane and ONE xor-32 exchange per row; tokens
// of a neighbouring row that share the first or the last 32-token block, and the slots behind the last packed
// token, are left out by index (a select, never arithmetic: what those slots hold does not matter).
// A term's dot product with a token is the same MFMA chain over ks = 0 .. 23 wherever the token sits in its
// block and wherever the row sits in the batch, and max is exact: the same row gives the same bits anywhere.
// No atomics.  Terms past V in the last tile read row V - 1 and write nothing.
// Two waves per SIMD (the second launch bound: 246 VGPRs, 192 of them the resident dec_w rows, no spill): the
// other wave's MFMAs cover a wave's wait for its next 1-KiB fragment of g.
#define DM_TILES 2
#define DM_WAVES 4
#define DM_VOCAB (32 * DM_TILES * DM_WAVES)
#define DM_ROWS 8
__global__ void __launch_bounds__(64 * DM_WAVES, 2) k_mlm_decode_max(
    const _Float16* __restrict__ g, const int32_t* __restrict__ tok_off, int B, int V,
    const _Float16* __restrict__ dec_w, const _Float16* __restrict__ dec_b, float* __restrict__ out) {
  constexpr int KS = HID / 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int v0 = blockIdx.x * DM_VOCAB + wave * (32 * DM_TILES);
  if (v0 >= V) return;                                             // wave-uniform; the kernel has no barrier
  half8 wf[DM_TILES][KS];
  float bias[DM_TILES];
#pragma unroll
  for (int t = 0; t < DM_TILES; ++t) {
    const int v = min(v0 + 32 * t + r, V - 1);
    const _Float16* wrow = dec_w + (size_t)v * HID + 8 * h;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wf[t][ks] = *(const half8*)(wrow + 16 * ks);
    bias[t] = (float)dec_b[v];
  }
  const int b_end = min(B, (int)(blockIdx.y + 1) * DM_ROWS);
  for (int b = blockIdx.y * DM_ROWS; b < b_end; ++b) {
    const int t0 = tok_off[b], t1 = tok_off[b + 1];                // wave-uniform
    float mx[DM_TILES];
#pragma unroll
    for (int t = 0; t < DM_TILES; ++t) mx[t] = -INFINITY;
    if (t1 > t0) {
      for (int tb = t0 >> 5; tb * 32 < t1; ++tb) {
        const half8* xp = (const half8*)g + (size_t)tb * KS * 64 + lane;
        f32x16 acc[DM_TILES];
#pragma unroll
        for (int t = 0; t < DM_TILES; ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const half8 xa = xp[ks * 64];
#pragma unroll
          for (int t = 0; t < DM_TILES; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa, wf[t][ks], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int tok = tb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
          const bool in_row = tok >= t0 && tok < t1;
#pragma unroll
          for (int t = 0; t < DM_TILES; ++t) mx[t] = in_row ? fmaxf(mx[t], acc[t][i]) : mx[t];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < DM_TILES; ++t) {
      const float m = fmaxf(mx[t], __shfl_xor(mx[t], 32));
      const int v = v0 + 32 * t + r;
      if (h == 0 && v < V) {
        const float z = m + bias[t];                               // -inf for a row without tokens
        float w = z > 0.f ? log1pf(z) : 0.f;
        if (!(w >= FLT_MIN)) w = 0.f;                              // +0.0f or a normal positive float
        out[(size_t)b * V + v] = w;
      }
    }
  }
}

void rf_launch_terms_head(const _Float16* x, const int32_t* tok_off, int B, int T, const rf_terms_end& e, float eps,
                          hipStream_t st) {
  const rf_mlm_head& hd = *e.head;
  const int slots = B * T;   // upper bound of the packed token count; workgroups past it return at once
  hipLaunchKernelGGL(k_mlm_transform, dim3((slots + MT_TOK - 1) / MT_TOK), dim3(MT_THREADS), 0, st, x, tok_off + B,
                     (const _Float16*)hd.tr_w, (const _Float16*)hd.tr_b, (const _Float16*)hd.tr_ln_g,
                     (const _Float16*)hd.tr_ln_b, eps, e.g);
  hipLaunchKernelGGL(k_mlm_decode_max, dim3((hd.vocab + DM_VOCAB - 1) / DM_VOCAB, (B + DM_ROWS - 1) / DM_ROWS),
                     dim3(64 * DM_WAVES), 0, st, e.g, tok_off, B, hd.vocab, (const _Float16*)hd.dec_w,
                     (const _Float16*)hd.dec_b, e.weights);
}

static size_t terms_g_bytes(int B, int T) { return (((size_t)B * T + 31) / 32 * 32) * HID * 2; }
static size_t align256(size_t n) { return (n + 255) / 256 * 256; }

extern "C" size_t rf_encode_terms_workspace_bytes(const rf_encoder_t* enc, int B, int T) {
  const size_t base = rf_encode_workspace_bytes(enc, B, T);
  if (!base) return 0;
  return align256(base) + terms_g_bytes(B, T);
}

extern "C" int rf_encode_terms(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev, int B, int T,
                               const rf_mlm_head* head, float* weights_dev, void* workspace_dev,
                               size_t workspace_bytes, void* stream) {
  if (!enc || !ids_dev || !lens_dev || !head || !weights_dev || !workspace_dev) {
    rf_set_error("rf_encode_terms: null argument");
    return RF_ERR_INVALID;
  }
  const void* const ptrs[6] = {head->tr_w, head->dec_w, head->tr_b, head->tr_ln_g, head->tr_ln_b, head->dec_b};
  for (int i = 0; i < 6; ++i)
    if (!ptrs[i] || ((uintptr_t)ptrs[i] & (i < 2 ? 15 : 1))) {
      rf_set_error("rf_encode_terms: head pointer %d null or misaligned (tr_w, dec_w: 16 bytes)", i);
      return RF_ERR_INVALID;
    }
  if (((uintptr_t)weights_dev & 3) || ((uintptr_t)ids_dev & 3) || ((uintptr_t)lens_dev & 3)) {
    rf_set_error("rf_encode_terms: misaligned ids, lens or weights");
    return RF_ERR_INVALID;
  }
  if (B <= 0 || T <= 0) {
    rf_set_error("rf_encode_terms: B=%d T=%d out of range", B, T);
    return RF_ERR_INVALID;
  }
  const rf_encoder_config& c = rf_encoder_cfg(enc);
  if (head->vocab != c.vocab_size) {
    rf_set_error("rf_encode_terms: the head has %d terms, the encoder's vocabulary %d", head->vocab, c.vocab_size);
    return RF_ERR_UNSUPPORTED;
  }
  if (T > c.max_position) {
    rf_set_error("rf_encode_terms: T=%d exceeds max_position %d", T, c.max_position);
    return RF_ERR_UNSUPPORTED;
  }
  const size_t base = align256(rf_encode_workspace_bytes(enc, B, T));
  if (workspace_bytes < base + terms_g_bytes(B, T) || ((uintptr_t)workspace_dev & 15)) {
    rf_set_error("rf_encode_terms: workspace too small or misaligned");
    return RF_ERR_CAPACITY;
  }
  rf_terms_end te{head, weights_dev, (_Float16*)((unsigned char*)workspace_dev + base)};
  rf_pair_ends ends{};
  ends.terms = &te;
  return rf_encode_pairs(enc, ids_dev, lens_dev, B, T, ends, workspace_dev, workspace_bytes, (hipStream_t)stream,
                         "rf_encode_terms");
}

// ---- dense [B, V] weights -> packed CSR of the heaviest terms ------------------------------------------------------
// Entries > 0 are kept; of more than max_terms the best max_terms by (value descending, term id ascending).
// A positive float's bit pattern orders as the float does, so the selection is integer work on keys (0 = not
// kept):
//   k_terms_count    off[b + 1] = min(positives of row b, max_terms)
//   k_terms_offsets  one workgroup: the running sum in place, off[0] = 0
//   k_terms_select   a row with fewer than max_terms entries keeps every key > 0.  Otherwise four 8-bit radix
//                    passes (a 256-bin LDS histogram each) find the key `thr` of the max_terms-th entry and how
//                    many entries equal to it are still needed; a last sweep over the row in ascending term id
//                    keeps key > thr and the first `need` of key == thr, at slot (kept before it) found by
//                    ballot counts -- so the CSR comes out in ascending term id and packed.
// The LDS atomics only count: their arrival order shows nowhere.  No global atomics, no allocation, no sync.
#define ST_THREADS 1024
__device__ __forceinline__ uint32_t term_key(float w) { return w > 0.f ? __float_as_uint(w) : 0u; }

__global__ void __launch_bounds__(ST_THREADS) k_terms_count(const float* __restrict__ w, int V, int max_terms,
                                                            int32_t* __restrict__ off) {
  __shared__ int32_t part[ST_THREADS / 64];
  const float* row = w + (size_t)blockIdx.x * V;
  int32_t c = 0;
  for (int v = threadIdx.x; v < V; v += ST_THREADS) c += term_key(row[v]) != 0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t s = 0;
    for (int i = 0; i < ST_THREADS / 64; ++i) s += part[i];
    off[blockIdx.x + 1] = min(s, max_terms);
  }
}

__global__ void __launch_bounds__(256) k_terms_offsets(int32_t* __restrict__ off, int B) {
  __shared__ int32_t part[256];
  const int tid = threadIdx.x;
  const int per = (B + 255) / 256;
  const int lo = min(B, tid * per), hi = min(B, lo + per);
  int32_t s = 0;
  for (int i = lo; i < hi; ++i) s += off[i + 1];
  part[tid] = s;
  __syncthreads();
  int32_t run = 0;
  for (int j = 0; j < tid; ++j) run += part[j];
  for (int i = lo; i < hi; ++i) {   // a thread reads and writes its own entries only
    run += off[i + 1];
    off[i + 1] = run;
  }
  if (tid == 0) off[0] = 0;
}

__global__ void __launch_bounds__(ST_THREADS) k_terms_select(const float* __restrict__ w, int V, int max_terms,
                                                             const int32_t* __restrict__ off,
                                                             int32_t* __restrict__ term, float* __restrict__ val) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sel[2];                       // thr, need
  __shared__ int32_t wtot[2][2][ST_THREADS / 64];   // [chunk parity][gt | eq][wave]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = w + (size_t)blockIdx.x * V;
  const int base = off[blockIdx.x];
  const int kept = off[blockIdx.x + 1] - base;
  if (kept <= 0) return;                            // workgroup-uniform
  uint32_t thr = 0, need = 0;
  if (kept >= max_terms) {                          // (== : at least max_terms positives)
    uint32_t prefix = 0, remaining = (uint32_t)max_terms;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int v = tid; v < V; v += ST_THREADS) {
        const uint32_t key = term_key(row[v]);
        const bool same = shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8));
        if (key && same) atomicAdd(&hist[(key >> shift) & 255], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        uint32_t above = 0;
        int bin = 255;
        for (; bin > 0; --bin) {
          if (above + hist[bin] >= remaining) break;
          above += hist[bin];
        }
        sel[0] = prefix | ((uint32_t)bin << shift);
        sel[1] = remaining - above;
      }
      __syncthreads();
      prefix = sel[0];
      remaining = sel[1];
    }
    thr = prefix;
    need = remaining;
  }
  int n_gt = 0, n_eq = 0;                           // entries of either kind before this chunk
  int parity = 0;
  for (int v0 = 0; v0 < V; v0 += ST_THREADS, parity ^= 1) {
    const int v = v0 + tid;
    const float x = v < V ? row[v] : 0.f;
    const uint32_t key = term_key(x);
    const bool gt = key > thr, eq = thr != 0 && key == thr;
    const uint64_t bg = __ballot(gt), be = __ballot(eq);
    if (lane == 0) {
      wtot[parity][0][wave] = __popcll(bg);
      wtot[parity][1][wave] = __popcll(be);
    }
    __syncthreads();   // one barrier per chunk: the next chunk writes the other half of wtot
    int gt_before = n_gt, eq_before = n_eq, gt_all = 0, eq_all = 0;
#pragma unroll
    for (int j = 0; j < ST_THREADS / 64; ++j) {
      const int a = wtot[parity][0][j], c = wtot[parity][1][j];
      gt_before += j < wave ? a : 0;
      eq_before += j < wave ? c : 0;
      gt_all += a;
      eq_all += c;
    }
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    gt_before += __popcll(bg & below);
    eq_before += __popcll(be & below);
    if (gt || (eq && (uint32_t)eq_before < need)) {
      const int slot = gt_before + min(eq_before, (int)need);
      if (slot < kept) {                            // (always: a guard against an out-of-range store)
        term[base + slot] = v;
        val[base + slot] = x;
      }
    }
    n_gt += gt_all;
    n_eq += eq_all;
  }
}

extern "C" int rf_sparsify_terms(const float* weights_dev, int B, int V, int max_terms, int32_t* off_dev,
                                 int32_t* term_dev, float* val_dev, void* stream) {
  if (!weights_dev || !off_dev || !term_dev || !val_dev) {
    rf_set_error("rf_sparsify_terms: null argument");
    return RF_ERR_INVALID;
  }
  if (B < 1 || V < 1 || max_terms < 1 || max_terms > RF_TERMS_MAX || (int64_t)B * max_terms > INT32_MAX) {
    rf_set_error("rf_sparsify_terms: B=%d V=%d max_terms=%d out of range (max_terms 1..%d)", B, V, max_terms,
                 RF_TERMS_MAX);
    return RF_ERR_INVALID;
  }
  if (((uintptr_t)weights_dev | (uintptr_t)off_dev | (uintptr_t)term_dev | (uintptr_t)val_dev) & 3) {
    rf_set_error("rf_sparsify_terms: misaligned pointer");
    return RF_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_terms_count, dim3(B), dim3(ST_THREADS), 0, st, weights_dev, V, max_terms, off_dev);
  hipLaunchKernelGGL(k_terms_offsets, dim3(1), dim3(256), 0, st, off_dev, B);
  hipLaunchKernelGGL(k_terms_select, dim3(B), dim3(ST_THREADS), 0, st, weights_dev, V, max_terms, off_dev, term_dev,
                     val_dev);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
