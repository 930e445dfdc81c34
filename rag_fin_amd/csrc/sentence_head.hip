// Sentence-embedder families: the Pooling and Normalize modules of a sentence-transformers directory as the launch
// that closes a sentence forward (rf_sentence_end, encoder_internal.h).  The layers and the embedding launch are
// the embedder's (encoder.hip); where rf_encode closes with k_pool_norm, rf_encode_sentences closes with
//   k_sentence_head<MODE>   one 4-wave workgroup per sequence: pool the tokens skip <= t < len (mean, max,
//                           mean / sqrt(len)) or take token 0 (CLS), then optionally x / max(||x||, 1e-12)
// MEAN with skip == 0 and normalize == 1 is k_pool_norm's arithmetic, addition by addition: the loop below is its
// loop with one more term in the lanes' load predicate, so the two entries give the same bits.
#include <math.h>

#include "encoder_internal.h"

static __device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// The activations are fragment-tiled (32 tokens x 16 features = 1 KiB contiguous), so a wave reads whole
// fragments: wave w takes the feature steps kk = w, w + 4, ... of every token block the sequence touches, lane
// (t = l & 31, h = l >> 5) folds the 8 features 16 kk + 8 h .. of the sequence's tokens t, t + 32, t + 64 ...
// (SEQUENCE-relative: a row's bits do not depend on where it sits in the packed stream), eight tokens per lane and
// trip with every load issued before the first add, and the 32 token lanes meet in a 5-step shuffle tree.
//   MEAN / MEAN_SQRT_LEN  `skip` is a mask on the lane's token index (rel >= skip), not a shifted start: the
//                         tokens keep their lanes and their trips, so the additions that remain happen in
//                         k_pool_norm's order
//   MAX                   a running fmaxf per lane from -inf, the same tree with fmaxf; fp16 -> fp32 is exact, so
//                         the result is the exact maximum of the hidden values
//   CLS                   one token: 192 lanes load two features each of token 0; `skip` is not read
// An empty set (skip >= len, or len == 0) gives the zero vector in every mode.
template <int MODE>
__global__ void __launch_bounds__(256) k_sentence_head(const _Float16* __restrict__ x,
                                                       const int32_t* __restrict__ tok_off,
                                                       const int32_t* __restrict__ skip, int normalize,
                                                       _Float16* __restrict__ out16, float* __restrict__ out32) {
  __shared__ float pooled[HID];
  __shared__ float red[4];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int t = lane & 31, h = lane >> 5;
  const int r0 = tok_off[b];
  const int n = tok_off[b + 1] - r0;
  if constexpr (MODE == RF_POOL_CLS) {
    if (tid < HID / 2) {
      half2v v;
      v[0] = v[1] = (_Float16)0.f;
      if (n > 0) v = *(const half2v*)(x + toff(r0, 2 * tid, HID / 16));   // features 2 tid, 2 tid + 1 share a slot
      pooled[2 * tid] = (float)v[0];
      pooled[2 * tid + 1] = (float)v[1];
    }
  } else {
    const int s = skip ? min(max(skip[b], 0), n) : 0;
    const int cnt = n - s;
    const float inv_cnt = 1.f / fmaxf((float)cnt, 1e-9f);
    const float root = sqrtf((float)max(cnt, 1));   // (an empty set sums to 0: 0 / 1)
    constexpr float ID = (MODE == RF_POOL_MAX) ? -INFINITY : 0.f;   // the fold's identity
    for (int kk = wave; kk < HID / 16; kk += 4) {
      float a[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = ID;
      for (int i0 = 0; i0 < n; i0 += 256) {
        half8 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int rel = i0 + 32 * u + t;
          const int tok = r0 + rel;
#pragma unroll
          for (int j = 0; j < 8; ++j) v[u][j] = (_Float16)ID;
          if (rel < n && rel >= s) v[u] = *(const half8*)(x + (((size_t)(tok >> 5) * (HID / 16) + kk) * 64 + h * 32 + (tok & 31)) * 8);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if constexpr (MODE == RF_POOL_MAX) a[j] = fmaxf(a[j], (float)v[u][j]);
            else a[j] += (float)v[u][j];
          }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = a[j];
        if constexpr (MODE == RF_POOL_MAX) {
          v = fmaxf(v, __shfl_xor(v, 1));
          v = fmaxf(v, __shfl_xor(v, 2));
          v = fmaxf(v, __shfl_xor(v, 4));
          v = fmaxf(v, __shfl_xor(v, 8));
          v = fmaxf(v, __shfl_xor(v, 16));
          v = cnt > 0 ? v : 0.f;
        } else {
          v += __shfl_xor(v, 1);
          v += __shfl_xor(v, 2);
          v += __shfl_xor(v, 4);
          v += __shfl_xor(v, 8);
          v += __shfl_xor(v, 16);
          if constexpr (MODE == RF_POOL_MEAN) v = v * inv_cnt;
          else v = v / root;
        }
        if (t == 0) pooled[16 * kk + 8 * h + j] = v;
      }
    }
  }
  __syncthreads();
  float a0 = 0.f, a1 = 0.f;
  if (tid < HID / 2) {
    a0 = pooled[tid * 2];
    a1 = pooled[tid * 2 + 1];
  }
  if (normalize) {   // a kernel argument: the barrier below is workgroup-uniform
    const float s = wave_sum(a0 * a0 + a1 * a1);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float nrm = fmaxf(sqrtf((red[0] + red[1]) + (red[2] + red[3])), 1e-12f);
    a0 /= nrm;
    a1 /= nrm;
  }
  if (tid < HID / 2) {
    if (out16) {
      out16[(size_t)b * HID + tid * 2] = (_Float16)a0;
      out16[(size_t)b * HID + tid * 2 + 1] = (_Float16)a1;
    }
    if (out32) {
      out32[(size_t)b * HID + tid * 2] = a0;
      out32[(size_t)b * HID + tid * 2 + 1] = a1;
    }
  }
}

template <int MODE>
static void sentence_head_launch(const _Float16* x, const int32_t* tok_off, const int32_t* skip, int B,
                                 const rf_sentence_head& head, _Float16* out16, float* out32, hipStream_t st) {
  hipLaunchKernelGGL(k_sentence_head<MODE>, dim3(B), dim3(256), 0, st, x, tok_off, skip, (int)(head.normalize != 0),
                     out16, out32);
}

void rf_launch_sentence_head(const _Float16* x, const int32_t* tok_off, const int32_t* skip, int B, int T,
                             const rf_sentence_head& head, _Float16* out16, float* out32, hipStream_t st) {
  (void)T;   // the packed offsets already hold lengths clamped to it
  switch (head.pooling) {   // (validated by rf_encode_sentences)
    case RF_POOL_CLS: sentence_head_launch<RF_POOL_CLS>(x, tok_off, skip, B, head, out16, out32, st); break;
    case RF_POOL_MAX: sentence_head_launch<RF_POOL_MAX>(x, tok_off, skip, B, head, out16, out32, st); break;
    case RF_POOL_MEAN_SQRT_LEN: sentence_head_launch<RF_POOL_MEAN_SQRT_LEN>(x, tok_off, skip, B, head, out16, out32, st); break;
    default: sentence_head_launch<RF_POOL_MEAN>(x, tok_off, skip, B, head, out16, out32, st); break;
  }
}
