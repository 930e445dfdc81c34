// Late interaction (ColBERT): one unit vector per kept token of a row, MaxSim of a bag of query vectors against
// the bags of a token field, and the exact selection of the best rows.
//   token vector    v_t = normalize(proj_w x_t),  x_t = last hidden state of token t of the row
//   score(q, r)     = sum_{i < q_len} max_{j in row r} (q_i . d_j)
// The layers are rf_encode's (encoder.hip, encoder_post.hip), unchanged; a token forward opens with the embedder's
// own embedding launch (token types 0) and closes with the two launches of this file (rf_tokens_end,
// encoder_internal.h):
//   k_token_offsets   kept tokens per row and their exclusive scan over the rows (integers, a fixed order)
//   k_token_project   the [D, H] projection of every packed token, its fp32 norm, one rounding to fp16, written at
//                     out_off[row] + (rank of the token among the row's kept tokens)
// rf_maxsim: k_maxsim_pairs (candidate mode: a wave per (query, row) pair) and k_maxsim_rows (all-rows mode: a
// workgroup per run of rows, looping over the queries) share one scoring routine, so a pair has one score.
// rf_maxsim_topk: k_maxsim_topk, one workgroup per query.
#include <math.h>

#include "encoder_internal.h"

// ---- kept tokens per row, exclusive scan over the rows -------------------------------------------------------------
// One workgroup; thread i owns the rows [i * per, (i + 1) * per) from the count to the scan, so it reads only what
// it wrote itself.  A token is kept when t < min(max(lens[b], 0), T) and bit id of `skip` is clear (ids are
// clamped into the vocabulary as the embedding launch clamps them).
__device__ __forceinline__ bool token_kept(const int32_t* __restrict__ ids, size_t at, const uint32_t* __restrict__ skip,
                                           int vocab) {
  if (!skip) return true;
  int id = ids[at];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  return ((skip[id >> 5] >> (id & 31)) & 1u) == 0u;
}

__global__ void __launch_bounds__(256) k_token_offsets(const int32_t* __restrict__ ids, const int32_t* __restrict__ lens,
                                                       int B, int T, const uint32_t* __restrict__ skip, int vocab,
                                                       int32_t* __restrict__ off) {
  __shared__ int32_t part[256];
  const int tid = threadIdx.x;
  const int per = (B + 255) / 256;
  const int lo = min(B, tid * per), hi = min(B, lo + per);
  int32_t s = 0;
  for (int b = lo; b < hi; ++b) {
    const int len = min(max(lens[b], 0), T);
    int32_t c = 0;
    for (int t = 0; t < len; ++t) c += token_kept(ids, (size_t)b * T + t, skip, vocab) ? 1 : 0;
    off[b + 1] = c;
    s += c;
  }
  part[tid] = s;
  __syncthreads();
  int32_t run = 0;
  for (int j = 0; j < tid; ++j) run += part[j];
  for (int b = lo; b < hi; ++b) {
    run += off[b + 1];
    off[b + 1] = run;
  }
  if (tid == 0) off[0] = 0;
}

// ---- v = proj_w x_t, v / max(|v|, 1e-12), fp16 ------------------------------------------------------------------------
// TP_TOK packed tokens per workgroup, thread j < D owns component j of every token of the group (k_cls_head's
// scheme: the hidden rows sit in LDS as fp32 and are read as broadcasts).
//   v[j]  = fma chain over k = 0 .. 383 ascending from 0.f of proj_w[j][k] * x[k]
//   |v|^2 : a wave per token, lane l sums v[l]^2 and v[l + 64]^2 (absent components are 0) in that order, the 64
//           lanes meet in the xor-shuffle tree 32 .. 1
//   out   = fp16(v[j] / max(sqrt(|v|^2), 1e-12))
// The token's row and position come from a binary search in the packed offsets, its rank from ballots over the
// row's ids before it.  None of it depends on the token's slot in the group or the row's place in the batch.
#define TP_TOK 16
#define TP_THREADS RF_MAXSIM_DIM
__global__ void __launch_bounds__(TP_THREADS) k_token_project(
    const _Float16* __restrict__ x, const int32_t* __restrict__ tok_off, const int32_t* __restrict__ ids, int B, int T,
    const _Float16* __restrict__ proj_w, int D, const uint32_t* __restrict__ skip, int vocab,
    const int32_t* __restrict__ out_off, _Float16* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float xs[TP_TOK][HID];   // the hidden rows
  __shared__ float vs[TP_TOK][RF_MAXSIM_DIM];                       // the projected rows
  __shared__ int32_t dst[TP_TOK];                                   // output slot of each token, -1: dropped
  __shared__ float inv[TP_TOK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = tok_off[B];                                         // packed token count
  const int t0 = blockIdx.x * TP_TOK;
  if (t0 >= M) return;                                              // workgroup-uniform
  for (int i = tid; i < TP_TOK * (HID / 8); i += TP_THREADS) {
    const int s = i / (HID / 8), c = i % (HID / 8);
    half8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.f;
    if (t0 + s < M) v = *(const half8*)(x + toff(t0 + s, 8 * c, HID / 16));
#pragma unroll
    for (int j = 0; j < 8; ++j) xs[s][8 * c + j] = (float)v[j];
  }
  for (int s = wave; s < TP_TOK; s += TP_THREADS / 64) {            // wave-uniform
    const int p = t0 + s;
    int slot = -1;
    if (p < M) {
      int lo = 0, hi = B - 1;                                       // the last row b with tok_off[b] <= p
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tok_off[mid] <= p) lo = mid; else hi = mid - 1;
      }
      const int b = lo, t = p - tok_off[b];
      int rank = 0;
      for (int u0 = 0; u0 < t; u0 += 64) {
        const int u = u0 + lane;
        const bool k = u < t && token_kept(ids, (size_t)b * T + u, skip, vocab);
        rank += __popcll(__ballot(k));
      }
      if (token_kept(ids, (size_t)b * T + t, skip, vocab)) slot = out_off[b] + rank;
    }
    if (lane == 0) dst[s] = slot;
  }
  __syncthreads();
  if (tid < D) {
    float acc[TP_TOK];
#pragma unroll
    for (int s = 0; s < TP_TOK; ++s) acc[s] = 0.f;
    const _Float16* wrow = proj_w + (size_t)tid * HID;
#pragma unroll 2
    for (int k = 0; k < HID; k += 8) {
      const half8 w = *(const half8*)(wrow + k);
#pragma unroll
      for (int s = 0; s < TP_TOK; ++s) {
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
#pragma unroll
    for (int s = 0; s < TP_TOK; ++s) vs[s][tid] = acc[s];
  } else {
#pragma unroll
    for (int s = 0; s < TP_TOK; ++s) vs[s][tid] = 0.f;
  }
  __syncthreads();
  for (int s = wave; s < TP_TOK; s += TP_THREADS / 64) {
    const float a = vs[s][lane], c = vs[s][lane + 64];
    float ss = a * a;
    ss = fmaf(c, c, ss);
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    if (lane == 0) inv[s] = fmaxf(sqrtf(ss), 1e-12f);
  }
  __syncthreads();
  if (tid < D) {
#pragma unroll
    for (int s = 0; s < TP_TOK; ++s) {
      const int slot = dst[s];
      if (slot >= 0) out[(size_t)slot * D + tid] = (_Float16)(vs[s][tid] / inv[s]);
    }
  }
}

void rf_launch_tokens_head(const _Float16* x, const int32_t* tok_off, const int32_t* ids, const int32_t* lens, int B,
                           int T, const rf_tokens_end& e, hipStream_t st) {
  const rf_token_head& hd = *e.head;
  hipLaunchKernelGGL(k_token_offsets, dim3(1), dim3(256), 0, st, ids, lens, B, T, hd.skip, hd.vocab, e.out_off);
  const int slots = B * T;   // upper bound of the packed token count; workgroups past it return at once
  hipLaunchKernelGGL(k_token_project, dim3((slots + TP_TOK - 1) / TP_TOK), dim3(TP_THREADS), 0, st, x, tok_off, ids, B,
                     T, (const _Float16*)hd.proj_w, hd.dim, hd.skip, hd.vocab, e.out_off, e.out_vec);
}

static bool maxsim_dim_ok(int d) { return d >= 16 && d <= RF_MAXSIM_DIM && d % 16 == 0; }

extern "C" size_t rf_encode_tokens_workspace_bytes(const rf_encoder_t* enc, int B, int T) {
  if (!enc || B < 1 || T < 1) return 0;
  return rf_encode_workspace_bytes(enc, B, T);
}

extern "C" int rf_encode_tokens(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev, int B, int T,
                                const rf_token_head* head, int32_t* out_off_dev, void* out_vec_dev,
                                void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!enc || !ids_dev || !lens_dev || !head || !out_off_dev || !out_vec_dev || !workspace_dev || !head->proj_w) {
    rf_set_error("rf_encode_tokens: null argument");
    return RF_ERR_INVALID;
  }
  if (((uintptr_t)head->proj_w & 15) || ((uintptr_t)out_vec_dev & 15) || ((uintptr_t)head->skip & 3) ||
      (((uintptr_t)ids_dev | (uintptr_t)lens_dev | (uintptr_t)out_off_dev) & 3)) {
    rf_set_error("rf_encode_tokens: misaligned pointer (proj_w, out_vec: 16 bytes; ids, lens, out_off, skip: 4)");
    return RF_ERR_INVALID;
  }
  if (B < 1 || T < 1) {
    rf_set_error("rf_encode_tokens: B=%d T=%d out of range", B, T);
    return RF_ERR_INVALID;
  }
  if (!maxsim_dim_ok(head->dim)) {
    rf_set_error("rf_encode_tokens: dim=%d is not a multiple of 16 in 16..%d", head->dim, RF_MAXSIM_DIM);
    return RF_ERR_UNSUPPORTED;
  }
  const rf_encoder_config& c = rf_encoder_cfg(enc);
  if (head->vocab != c.vocab_size) {
    rf_set_error("rf_encode_tokens: the head's vocabulary is %d, the encoder's %d", head->vocab, c.vocab_size);
    return RF_ERR_UNSUPPORTED;
  }
  if (T > c.max_position) {
    rf_set_error("rf_encode_tokens: T=%d exceeds max_position %d", T, c.max_position);
    return RF_ERR_UNSUPPORTED;
  }
  if ((int64_t)B * T > INT32_MAX) {
    rf_set_error("rf_encode_tokens: B=%d T=%d out of range", B, T);
    return RF_ERR_INVALID;
  }
  rf_tokens_end te{head, out_off_dev, (_Float16*)out_vec_dev};
  rf_pair_ends ends{};
  ends.tokens = &te;
  return rf_encode_pairs(enc, ids_dev, lens_dev, B, T, ends, workspace_dev, workspace_bytes, (hipStream_t)stream,
                         "rf_encode_tokens");
}

// ---- MaxSim -----------------------------------------------------------------------------------------------------------
// v_mfma_f32_32x32x16_f16 with the document's tokens on the A rows and the query's tokens on the B columns: lane l
// (r = l % 32, h = l / 32) holds features 16 ks + 8 h .. + 7 of document token r of a 32-token tile and of query
// token r -- sixteen bytes of the row-major matrices as they are.  The 32 x 32 fp32 result has the query token on
// the lane and the tile's document tokens in the 16 registers (token (i & 3) + 8 (i >> 2) + 4 h), so the max over
// a document is 16 fmaxf per lane and tile into ONE running register, and one xor-32 exchange per (query, row).
// Document tokens behind the row's end are left out by index (a select: they enter as -inf, never as 0; their
// lanes re-read the row's last token, so nothing outside the row is touched); query slots >= q_len are never
// loaded (their lanes hold zeros) and never summed.  A dot product is the MFMA chain ks = 0 .. D/16 - 1 from 0.f,
// the same wherever the token sits in its tile; max is exact; the sum over the query's tokens is
//   s = 0.f; for i = 0 .. q_len - 1: s = s + m_i
// on every lane alike.  So a (query, row) pair has one score, whichever kernel, workgroup or wave computes it.
// A wave keeps MS_TILES tiles of a row as A operands (MS_TILES * D/16 * 4 VGPRs); in all-rows mode they stay
// there while the wave walks over the queries, so a row of up to 32 MS_TILES tokens is read once per call.
#define MS_TILES 4
#define MS_WAVES 4
#define MS_RUN 64      // rows of one workgroup in all-rows mode
#define MS_QCHUNK 64   // queries whose scores one workgroup gathers in LDS before writing them out

struct MaxsimArgs {
  const _Float16* vec;
  const int64_t* off;
  int64_t n_rows;
  int D;
  const _Float16* q;
  const int32_t* q_len;
  int B;
  const int64_t* cand_off;
  const int64_t* cand_row;
  const uint32_t* filt;
  float* scores;
};

template <int KS>
__device__ __forceinline__ void ms_load_query(half8 (&qf)[KS], const _Float16* __restrict__ q, int q_len, int lane) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    half8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.f;
    if (r < q_len) v = *(const half8*)(q + (size_t)r * (16 * KS) + 16 * ks + 8 * h);
    qf[ks] = v;
  }
}

// tiles [tg, tg + MS_TILES) of the row whose tokens are [t0, t1), t1 > t0
template <int KS>
__device__ __forceinline__ void ms_load_docs(half8 (&a)[MS_TILES][KS], const _Float16* __restrict__ vec, int64_t tg,
                                             int64_t t1, int lane) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int g = 0; g < MS_TILES; ++g) {
    if (tg + 32 * g < t1) {                                          // wave-uniform
      const int64_t tok = min(tg + 32 * g + r, t1 - 1);
      const _Float16* row = vec + (size_t)tok * (16 * KS) + 8 * h;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) a[g][ks] = *(const half8*)(row + 16 * ks);
    }
  }
}

template <int KS>
__device__ __forceinline__ float ms_tiles_max(float mx, const half8 (&a)[MS_TILES][KS], const half8 (&qf)[KS],
                                              int64_t tg, int64_t t1, int lane) {
  const int h = lane >> 5;
#pragma unroll
  for (int g = 0; g < MS_TILES; ++g) {
    if (tg + 32 * g < t1) {                                          // wave-uniform
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[g][ks], qf[ks], acc, 0, 0, 0);
      const int n = (int)min((int64_t)32, t1 - (tg + 32 * g));       // the tile's tokens that belong to the row
      if (n >= 32) {                                                 // wave-uniform: a whole tile needs no select
#pragma unroll
        for (int i = 0; i < 16; ++i) mx = fmaxf(mx, acc[i]);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) mx = ((i & 3) + 8 * (i >> 2) + 4 * h) < n ? fmaxf(mx, acc[i]) : mx;
      }
    }
  }
  return mx;
}

// the per-token maxima (lane r and r + 32 hold halves of query token r's) -> the score, on every lane: the lanes'
// values are read one after the other into the scalar unit and added in token order (a token past q_len leaves
// the sum as it is: a select, not an addition of zero)
__device__ __forceinline__ float ms_finish(float mx, int q_len) {
  const float m = fmaxf(mx, __shfl_xor(mx, 32));
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < RF_MAXSIM_QTOK; ++i) {
    const float mi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, m), i));
    s = i < q_len ? s + mi : s;
  }
  return s;
}

// a row's token range, or t1 = t0 when the row is no hit: outside [0, n_rows), failing the filter, or empty
__device__ __forceinline__ void ms_row_range(const MaxsimArgs& P, int64_t row, int64_t& t0, int64_t& t1) {
  t0 = t1 = 0;
  if (row < 0 || row >= P.n_rows) return;
  if (P.filt) {
    if ((int64_t)P.filt[0] != P.n_rows) return;                     // a header for another row count passes no row
    if (((P.filt[RF_FILTER_HDR_WORDS + (row >> 5)] >> (row & 31)) & 1u) == 0u) return;
  }
  t0 = P.off[row];
  t1 = max(P.off[row + 1], t0);
}

// candidate mode: waves stride over the pairs; a pair's query is found by a binary search in cand_off
template <int KS>
__global__ void __launch_bounds__(64 * MS_WAVES) k_maxsim_pairs(const MaxsimArgs P) {
  const int lane = threadIdx.x & 63;
  const int64_t n_pairs = P.cand_off[P.B];
  const int64_t stride = (int64_t)gridDim.x * MS_WAVES;
  for (int64_t p = (int64_t)blockIdx.x * MS_WAVES + (threadIdx.x >> 6); p < n_pairs; p += stride) {   // wave-uniform
    int lo = 0, hi = P.B - 1;                                       // the last query b with cand_off[b] <= p
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (P.cand_off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int ql = min(max(P.q_len[lo], 0), RF_MAXSIM_QTOK);
    int64_t t0, t1;
    ms_row_range(P, P.cand_row[p], t0, t1);
    float score = -INFINITY;
    if (ql > 0 && t1 > t0) {
      half8 qf[KS];
      ms_load_query<KS>(qf, P.q + (size_t)lo * RF_MAXSIM_QTOK * (16 * KS), ql, lane);
      float mx = -INFINITY;
      for (int64_t tg = t0; tg < t1; tg += 32 * MS_TILES) {
        half8 a[MS_TILES][KS];
        ms_load_docs<KS>(a, P.vec, tg, t1, lane);
        mx = ms_tiles_max<KS>(mx, a, qf, tg, t1, lane);
      }
      score = ms_finish(mx, ql);
    }
    if (lane == 0) P.scores[p] = score;
  }
}

// all-rows mode: a workgroup takes MS_RUN consecutive rows, a wave every MS_WAVES-th of them; the wave holds a row
// of up to 32 MS_TILES tokens as A operands while it walks over the queries (a longer row is re-read per query,
// from the caches, through the same registers).  The scores of MS_QCHUNK queries x MS_RUN rows are gathered in
// LDS and written as runs of consecutive rows.  Two waves per SIMD (the second launch bound): the other wave's
// MFMAs cover a wave's wait for its next query.
template <int KS>
__global__ void __launch_bounds__(64 * MS_WAVES, 2) k_maxsim_rows(const MaxsimArgs P) {
  __shared__ float sc[MS_QCHUNK][MS_RUN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * MS_RUN;
  const int rows_here = (int)min((int64_t)MS_RUN, P.n_rows - row0);
  for (int b0 = 0; b0 < P.B; b0 += MS_QCHUNK) {
    const int nb = min(MS_QCHUNK, P.B - b0);
    for (int rl = wave; rl < rows_here; rl += MS_WAVES) {           // wave-uniform
      int64_t t0, t1;
      ms_row_range(P, row0 + rl, t0, t1);
      if (t1 <= t0) {
        for (int j = lane; j < nb; j += 64) sc[j][rl] = -INFINITY;
        continue;
      }
      const bool long_row = t1 - t0 > 32 * MS_TILES;                  // wave-uniform
      half8 a[MS_TILES][KS];
      if (!long_row) ms_load_docs<KS>(a, P.vec, t0, t1, lane);
      // the next query's operands are loaded while this one's MFMAs run
      half8 qf[KS], qn[KS];
      int ql = min(max(P.q_len[b0], 0), RF_MAXSIM_QTOK), qln = 0;
      ms_load_query<KS>(qf, P.q + (size_t)b0 * RF_MAXSIM_QTOK * (16 * KS), ql, lane);
      for (int j = 0; j < nb; ++j, ql = qln) {
        if (j > 0) {
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) qf[ks] = qn[ks];
        }
        if (j + 1 < nb) {
          qln = min(max(P.q_len[b0 + j + 1], 0), RF_MAXSIM_QTOK);
          ms_load_query<KS>(qn, P.q + (size_t)(b0 + j + 1) * RF_MAXSIM_QTOK * (16 * KS), qln, lane);
        }
        float score = -INFINITY;
        if (ql > 0) {
          float mx = -INFINITY;
          if (!long_row) {
            mx = ms_tiles_max<KS>(mx, a, qf, t0, t1, lane);
          } else {
            for (int64_t tg = t0; tg < t1; tg += 32 * MS_TILES) {
              ms_load_docs<KS>(a, P.vec, tg, t1, lane);
              mx = ms_tiles_max<KS>(mx, a, qf, tg, t1, lane);
            }
          }
          score = ms_finish(mx, ql);
        }
        if (lane == 0) sc[j][rl] = score;
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb * MS_RUN; i += 64 * MS_WAVES) {
      const int j = i / MS_RUN, rl = i % MS_RUN;
      if (rl < rows_here) P.scores[(size_t)(b0 + j) * P.n_rows + row0 + rl] = sc[j][rl];
    }
    __syncthreads();
  }
}

template <int KS>
static void maxsim_launch(const MaxsimArgs& P, hipStream_t st) {
  if (P.cand_off) {
    // the pair count lives on the device: a fixed grid strides over it (waves past it leave at once)
    hipLaunchKernelGGL(k_maxsim_pairs<KS>, dim3(2048), dim3(64 * MS_WAVES), 0, st, P);
  } else {
    hipLaunchKernelGGL(k_maxsim_rows<KS>, dim3((unsigned)((P.n_rows + MS_RUN - 1) / MS_RUN)), dim3(64 * MS_WAVES), 0,
                       st, P);
  }
}

extern "C" int rf_maxsim(const rf_token_field* docs, const void* q_vec_dev, const int32_t* q_len_dev, int B,
                         const int64_t* cand_off_dev, const int64_t* cand_row_dev, const void* filter_dev,
                         float* scores_dev, void* stream) {
  if (!docs || !q_vec_dev || !q_len_dev || !scores_dev || !docs->off || (cand_off_dev && !cand_row_dev)) {
    rf_set_error("rf_maxsim: null argument");
    return RF_ERR_INVALID;
  }
  if (!maxsim_dim_ok(docs->dim)) {
    rf_set_error("rf_maxsim: dim=%d is not a multiple of 16 in 16..%d", docs->dim, RF_MAXSIM_DIM);
    return RF_ERR_UNSUPPORTED;
  }
  if (B < 1 || docs->n_rows < 0 || docs->n_rows > (int64_t)0x7fffffff * MS_RUN) {
    rf_set_error("rf_maxsim: B=%d n_rows=%lld out of range", B, (long long)docs->n_rows);
    return RF_ERR_INVALID;
  }
  if (!docs->vec && docs->n_rows > 0) {
    rf_set_error("rf_maxsim: null argument");
    return RF_ERR_INVALID;
  }
  if (((uintptr_t)docs->vec & 15) || ((uintptr_t)q_vec_dev & 15) || ((uintptr_t)filter_dev & 15) ||
      (((uintptr_t)docs->off | (uintptr_t)cand_off_dev | (uintptr_t)cand_row_dev) & 7) ||
      (((uintptr_t)q_len_dev | (uintptr_t)scores_dev) & 3)) {
    rf_set_error("rf_maxsim: misaligned pointer (vectors and filter: 16 bytes; offsets and rows: 8; q_len, scores: 4)");
    return RF_ERR_INVALID;
  }
  if (!cand_off_dev && docs->n_rows == 0) return RF_OK;             // [B, 0] scores
  MaxsimArgs P;
  P.vec = (const _Float16*)docs->vec;
  P.off = docs->off;
  P.n_rows = docs->n_rows;
  P.D = docs->dim;
  P.q = (const _Float16*)q_vec_dev;
  P.q_len = q_len_dev;
  P.B = B;
  P.cand_off = cand_off_dev;
  P.cand_row = cand_row_dev;
  P.filt = (const uint32_t*)filter_dev;
  P.scores = scores_dev;
  hipStream_t st = (hipStream_t)stream;
  switch (docs->dim / 16) {
    case 1: maxsim_launch<1>(P, st); break;
    case 2: maxsim_launch<2>(P, st); break;
    case 3: maxsim_launch<3>(P, st); break;
    case 4: maxsim_launch<4>(P, st); break;
    case 5: maxsim_launch<5>(P, st); break;
    case 6: maxsim_launch<6>(P, st); break;
    case 7: maxsim_launch<7>(P, st); break;
    default: maxsim_launch<8>(P, st); break;
  }
  RF_HIP(hipGetLastError());
  return RF_OK;
}

// ---- the best k of a segment of scores ----------------------------------------------------------------------------------
// One workgroup per query over scores[seg_off[b] .. seg_off[b + 1]).  A float's bit pattern, sign-folded, orders as
// the float does, so the selection is integer work on keys (0 = no hit: -inf or NaN):
//   four 8-bit radix passes (a 256-bin LDS histogram each) find the key `thr` of the k-th best entry and how many
//   entries equal to it are still needed; a sweep in ascending position keeps key > thr and the first `need` of
//   key == thr, at slot (kept before it) found by ballot counts; the <= k kept entries are then ranked among
//   themselves by (key descending, position ascending) and written in that order, the tail padded with -inf / -1.
// The LDS atomics only count: their arrival order shows nowhere.  No global atomics, no allocation, no sync.
#define TK_THREADS 1024
__device__ __forceinline__ uint32_t score_key(float s) {
  if (!(s > -INFINITY)) return 0u;
  const uint32_t u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(TK_THREADS) k_maxsim_topk(const float* __restrict__ scores,
                                                            const int64_t* __restrict__ seg_off,
                                                            const int64_t* __restrict__ rows, int k, int64_t id_base,
                                                            float* __restrict__ scores_out, int64_t* __restrict__ ids_out,
                                                            double* __restrict__ exact_out) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sel[2];                       // thr, need
  __shared__ int32_t wtot[2][2][TK_THREADS / 64];   // [chunk parity][gt | eq][wave]
  __shared__ uint32_t kept_key[RF_MAX_K];
  __shared__ int64_t kept_pos[RF_MAX_K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t s0 = seg_off[blockIdx.x];
  const int64_t n = max(seg_off[blockIdx.x + 1] - s0, (int64_t)0);
  const float* seg = scores + s0;
  uint32_t prefix = 0, remaining = (uint32_t)k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int64_t v = tid; v < n; v += TK_THREADS) {
      const uint32_t key = score_key(seg[v]);
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
  // (fewer than k hits: every pass ends in bin 0, thr = 0 and every hit has key > thr)
  const uint32_t thr = prefix, need = remaining;
  int n_gt = 0, n_eq = 0;                           // entries of either kind before this chunk
  int parity = 0;
  for (int64_t v0 = 0; v0 < n; v0 += TK_THREADS, parity ^= 1) {
    const int64_t v = v0 + tid;
    const uint32_t key = v < n ? score_key(seg[v]) : 0u;
    const bool gt = key > thr, eq = thr != 0 && key == thr;
    const uint64_t bg = __ballot(gt), be = __ballot(eq);
    if (lane == 0) {
      wtot[parity][0][wave] = __popcll(bg);
      wtot[parity][1][wave] = __popcll(be);
    }
    __syncthreads();   // one barrier per chunk: the next chunk writes the other half of wtot
    int gt_before = n_gt, eq_before = n_eq, gt_all = 0, eq_all = 0;
#pragma unroll
    for (int j = 0; j < TK_THREADS / 64; ++j) {
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
      if (slot < k) {                               // (always: a guard against an out-of-range store)
        kept_key[slot] = key;
        kept_pos[slot] = v;
      }
    }
    n_gt += gt_all;
    n_eq += eq_all;
  }
  __syncthreads();
  const int m = min(n_gt + min(n_eq, (int)need), k);
  const size_t out0 = (size_t)blockIdx.x * k;
  if (tid < k) {
    if (tid < m) {
      const uint32_t key = kept_key[tid];
      int rank = 0;                                 // slots ascend with the position
      for (int j = 0; j < m; ++j) rank += (kept_key[j] > key || (kept_key[j] == key && j < tid)) ? 1 : 0;
      const int64_t pos = kept_pos[tid];
      const float s = seg[pos];
      scores_out[out0 + rank] = s;
      ids_out[out0 + rank] = rows ? rows[s0 + pos] : id_base + pos;
      if (exact_out) exact_out[out0 + rank] = (double)s;
    } else {
      scores_out[out0 + tid] = -INFINITY;
      ids_out[out0 + tid] = -1;
      if (exact_out) exact_out[out0 + tid] = -INFINITY;
    }
  }
}

extern "C" int rf_maxsim_topk(const float* scores_dev, const int64_t* seg_off_dev, const int64_t* rows_dev, int B, int k,
                              int64_t id_base, float* scores_out, int64_t* ids_out, double* exact_out, void* stream) {
  if (!scores_dev || !seg_off_dev || !scores_out || !ids_out) {
    rf_set_error("rf_maxsim_topk: null argument");
    return RF_ERR_INVALID;
  }
  if (B < 1 || k < 1 || k > RF_MAX_K) {
    rf_set_error("rf_maxsim_topk: need B >= 1 and 1 <= k <= %d (got B = %d, k = %d)", RF_MAX_K, B, k);
    return RF_ERR_INVALID;
  }
  if ((((uintptr_t)scores_dev | (uintptr_t)scores_out) & 3) ||
      (((uintptr_t)seg_off_dev | (uintptr_t)rows_dev | (uintptr_t)ids_out | (uintptr_t)exact_out) & 7)) {
    rf_set_error("rf_maxsim_topk: misaligned pointer");
    return RF_ERR_INVALID;
  }
  hipLaunchKernelGGL(k_maxsim_topk, dim3(B), dim3(TK_THREADS), 0, (hipStream_t)stream, scores_dev, seg_off_dev,
                     rows_dev, k, id_base, scores_out, ids_out, exact_out);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
