// Diversified search: maximal-marginal-relevance selection over the candidates of a search
// (include/ragfin.h, "diversified search").  A post-stage on a [B, fetch_k] answer
// of any search form: it reads the candidates' fp16 rows once and touches no sweep.
//
// Per query, candidates c_0 .. c_{F-1} in the order of the search (fp64 score s_i descending, row
// ascending), g(i, j) = the contract dot of the rows of c_i and c_j, mu = 1 - lambda:
//   round t:  v_i = (lambda s_i) - pen_i over the unselected i, pen_i = 0.0 in round 0 and
//             mu m_i afterwards; each product and the subtraction rounded to fp64 on its own;
//             pick = the largest v_i, the smallest i on a tie; slot t = (float(s), id, s) of the pick;
//             m_i = max(m_i, g(i, pick)), m_i = -inf before the first pick.
// min(k, F) rounds; the other slots are -inf / -1.  Mirrored in numpy by tests/test_mmr_search_gpu.py.
#include "rf_internal.h"
#include "merge_common.h"

#define MMR_NONE 0xFFFFFFFFu

// Bookkeeping ahead of the staged rows: s[64], m[64] fp64, row[64], {pick, F, 2 spare} uint32.
#define MMR_HDR_BYTES (RF_MAX_K * 8 + RF_MAX_K * 8 + RF_MAX_K * 4 + 16)

// The staged rows use the padded stride of rescore_rows' srows: 2 KS + 1 uint4 per row.  Largest
// case, dim 1024 (KS 64) and fetch_k 64: 64 x 129 x 16 B = 132 096 B + 1 296 B of bookkeeping, of
// the 160 KiB of a CU: every supported dim fits in one piece.
static size_t mmr_lds_bytes(int KS, int fetch_k) {
  return (size_t)MMR_HDR_BYTES + (size_t)fetch_k * (2 * KS + 1) * 16;
}

// v = (lam s) - pen with two roundings: no contraction into an fma in this function.
__device__ __forceinline__ double mmr_value(double lam, double s, double pen) {
#pragma clang fp contract(off)
  const double rel = lam * s;
  return rel - pen;
}
__device__ __forceinline__ double mmr_penalty(double mu, double m) {
#pragma clang fp contract(off)
  return mu * m;
}

__global__ void __launch_bounds__(MERGE_THREADS) k_mmr(
    const uint4* __restrict__ tiles, int KS, uint32_t n_rows, int fetch_k, int k, double lam, double mu,
    int64_t id_base, const double* __restrict__ cand_exact, const int64_t* __restrict__ cand_ids,
    float* __restrict__ scores, int64_t* __restrict__ ids, double* __restrict__ exact) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  double* s_s = (double*)lds;                        // [64] relevance score of candidate i
  double* s_m = s_s + RF_MAX_K;                      // [64] max similarity to the picks so far
  uint32_t* s_row = (uint32_t*)(s_m + RF_MAX_K);     // [64] row, MMR_NONE = absent
  uint32_t* s_pick = s_row + RF_MAX_K;               // the pick of the round
  uint32_t* s_F = s_pick + 1;                        // real candidates
  uint4* srows = (uint4*)(lds + MMR_HDR_BYTES);      // [fetch_k][2 KS + 1]

  const int qi = blockIdx.x;
  const int tid = threadIdx.x;
  const int chunks = 2 * KS;
  const int stride = 2 * KS + 1;
  const size_t in0 = (size_t)qi * fetch_k;
  const size_t out0 = (size_t)qi * k;

  // ---- the candidates: wave 0, lane i owns candidate i -------------------------------------------
  // An id of -1 (padding) or one whose row is not in the index is absent: never gathered, never picked.
  bool avail = false;
  double s_mine = -INFINITY;
  int64_t id_mine = -1;
  if (tid < 64) {
    if (tid < fetch_k) {
      id_mine = cand_ids[in0 + tid];
      const int64_t row = id_mine - id_base;
      avail = id_mine >= 0 && row >= 0 && row < (int64_t)n_rows;
      if (avail) s_mine = cand_exact[in0 + tid];
      s_row[tid] = avail ? (uint32_t)row : MMR_NONE;
      s_s[tid] = s_mine;
      s_m[tid] = -INFINITY;
    }
    const uint32_t F = (uint32_t)__popcll(__ballot(avail));
    if (tid == 0) *s_F = F;
  }
  __syncthreads();
  const uint32_t F = *s_F;
  const uint32_t rounds = F < (uint32_t)k ? F : (uint32_t)k;

  // ---- stage the rows once ------------------------------------------------------------------------
  if (rounds > 1u) {
    for (uint32_t idx = tid; idx < (uint32_t)fetch_k * (uint32_t)chunks; idx += MERGE_THREADS) {
      const uint32_t r = idx / chunks, ch = idx % chunks;
      const uint32_t row = s_row[r];
      srows[r * stride + ch] = row != MMR_NONE ? tiles[rf_chunk_index((int64_t)row, (int)ch, KS)]
                                               : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  __syncthreads();

  // ---- the rounds -----------------------------------------------------------------------------------
  for (uint32_t t = 0; t < rounds; ++t) {
    if (tid < 64) {
      // argmax on (v descending, i ascending) over the unselected candidates: one butterfly
      const double pen = t == 0u ? 0.0 : mmr_penalty(mu, s_m[tid < fetch_k ? tid : 0]);
      double v = mmr_value(lam, s_mine, pen);
      uint32_t bi = avail ? (uint32_t)tid : MMR_NONE;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, o);
        const bool take = oi != MMR_NONE && (bi == MMR_NONE || ov > v || (ov == v && oi < bi));
        if (take) {
          v = ov;
          bi = oi;
        }
      }
      const uint32_t pick = (uint32_t)__shfl((int)bi, 0);   // one answer for the wave
      if ((uint32_t)tid == pick) {
        avail = false;
        scores[out0 + t] = (float)s_mine;
        ids[out0 + t] = id_mine;
        if (exact) exact[out0 + t] = s_mine;
      }
      if (tid == 0) *s_pick = pick;
    }
    if (t + 1u == rounds) break;
    __syncthreads();
    const uint32_t pick = *s_pick;
    if (pick >= (uint32_t)fetch_k) break;   // (cannot happen: rounds <= F; keeps the row read in bounds)
    // the column g(., pick): 8 lanes per row, 32 rows per pass, from LDS only
    const _Float16* prow = (const _Float16*)(srows + pick * stride);
    const int j = tid & 7;
    for (uint32_t base = 0; base < (uint32_t)fetch_k; base += MERGE_STAGE_ROWS) {
      const uint32_t r = base + ((uint32_t)tid >> 3);
      const _Float16* row = (const _Float16*)(srows + (r < (uint32_t)fetch_k ? r : 0u) * stride);
      const double g = contract_dot8(row, prow, chunks, j);
      if (j == 0 && r < (uint32_t)fetch_k) {
        const double m = s_m[r];
        s_m[r] = g > m ? g : m;
      }
    }
    __syncthreads();
  }

  // ---- the slots no round filled ------------------------------------------------------------------
  for (uint32_t o = rounds + tid; o < (uint32_t)k; o += MERGE_THREADS) {
    scores[out0 + o] = -INFINITY;
    ids[out0 + o] = -1;
    if (exact) exact[out0 + o] = -INFINITY;
  }
}

int rf_launch_mmr(const rf_index* ix, int B, int fetch_k, int k, double lambda, int64_t id_base,
                  const double* cand_exact, const int64_t* cand_ids, float* scores, int64_t* ids,
                  double* exact, hipStream_t st) {
  const size_t lds = mmr_lds_bytes(ix->KS, fetch_k);
  static rf_lds_attr lds_attr;
  RF_HIP(rf_ensure_lds(lds_attr, (const void*)k_mmr, lds));
  const double mu = 1.0 - lambda;
  hipLaunchKernelGGL(k_mmr, dim3(B), dim3(MERGE_THREADS), lds, st, ix->tiles, ix->KS, (uint32_t)ix->size, fetch_k, k,
                     lambda, mu, id_base, cand_exact, cand_ids, scores, ids, exact);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
