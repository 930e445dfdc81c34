// Lexical search: exact BM25 top-k over posting lists, and weighted reciprocal-rank fusion of the
// answers of several searches (include/ragfin.h, "lexical search").
//
// Postings (built on the host, rag_fin_amd/lexical.py): term t owns post_row / post_imp
// [post_off[t], post_off[t + 1]), rows ascending; imp = float32(idf * tf-saturation), > 0.
// Query: its distinct known terms t_1 < .. < t_m with weights w_i = float32(count in the query).
// Score of row r:  acc = 0.0f; for i = 1..m, if t_i in r: acc = acc + (w_i * imp[t_i, r]) -- the
// product and the sum each rounded to fp32 on its own, in ascending term order.  A row is a hit iff
// acc > 0 and its filter bit is set; ranking (score desc, row asc).  The summation order is fixed by
// a barrier between terms and rows within a term are distinct, so no two lanes meet on an
// accumulator: no atomics, and the same bits on every run and for every batch size.
// Mirrored in numpy by rag_fin_amd/lexical.py (bm25_reference, rrf_reference).
#include "rf_internal.h"

#define SPARSE_THREADS 256
#define SPARSE_WAVES (SPARSE_THREADS / 64)
#define SPARSE_PER_THREAD (RF_SPARSE_TILE_ROWS / SPARSE_THREADS)
#define FUSE_THREADS 256   // = the most candidates of a fusion: RF_FUSE_MAX_ARMS * RF_MAX_K

static_assert(RF_SPARSE_TILE_ROWS % SPARSE_THREADS == 0, "a thread owns whole strided slots of the tile");
static_assert(RF_SPARSE_MAX_TERMS <= SPARSE_THREADS, "one lane per query term in the slice search");
static_assert(RF_FUSE_MAX_ARMS * RF_MAX_K <= FUSE_THREADS, "one lane per fusion candidate");

// A hit as one word: larger key <=> (higher score, then lower row).  Scores of hits are positive
// floats, whose bit patterns order as unsigned integers; 0 is "no hit".
__device__ __forceinline__ unsigned long long sparse_key(float score, uint32_t row) {
  return ((unsigned long long)__builtin_bit_cast(uint32_t, score) << 32) | (unsigned long long)(0xFFFFFFFFu - row);
}

// acc + (w * imp) with two roundings.  (__fadd_rn(acc, __fmul_rn(w, imp)) is plain `acc + w * imp` to the
// compiler, which contracted it into v_fmac_f32 -- invisible while the weights were the small term counts of
// BM25 queries, whose products are exact, and 1-2 ulp off the definition with the real-valued weights of
// learned sparse vectors.  The pragma keeps the product and the sum apart.)
__device__ __forceinline__ float sparse_add(float acc, float w, float imp) {
#pragma clang fp contract(off)
  const float prod = w * imp;
  return acc + prod;
}

// first p in [lo, hi) with rows[p] >= row (rows ascending), hi if none
__device__ __forceinline__ int64_t sparse_lower_bound(const uint32_t* __restrict__ rows, int64_t lo, int64_t hi,
                                                      uint32_t row) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (rows[mid] < row) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The largest key of the workgroup, known to every thread after ONE barrier: wave butterflies, then
// the wave maxima through `wmax` -- the caller alternates between two such arrays from round to
// round, so a fast wave's next write never lands under a slow wave's read.
__device__ __forceinline__ unsigned long long sparse_block_max(unsigned long long key, unsigned long long* wmax) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = key;
  __syncthreads();
  unsigned long long best = wmax[0];
#pragma unroll
  for (int w = 1; w < SPARSE_WAVES; ++w) best = wmax[w] > best ? wmax[w] : best;
  return best;
}

struct SparseScan {
  const int64_t* post_off;
  const uint32_t* post_row;
  const float* post_imp;
  const uint32_t* filt;      // the filter buffer (header + mask), or nullptr
  const int32_t* q_off;
  const int32_t* q_term;
  const float* q_weight;
  unsigned long long* lists;  // [B][n_tiles][k] keys, best first, 0 past the end
  int64_t n_terms, nnz;
  uint32_t n_rows, n_tiles;
  int k;
};

// Grid (tiles, B).  The workgroup accumulates rows [tile * TILE, (tile + 1) * TILE) in LDS.
__global__ void __launch_bounds__(SPARSE_THREADS) k_sparse_scan(SparseScan P) {
  __shared__ float s_acc[RF_SPARSE_TILE_ROWS];
  __shared__ int64_t s_beg[RF_SPARSE_MAX_TERMS], s_end[RF_SPARSE_MAX_TERMS];
  __shared__ float s_w[RF_SPARSE_MAX_TERMS];
  __shared__ unsigned long long s_wmax[2][SPARSE_WAVES];

  const uint32_t tid = threadIdx.x;
  const uint32_t tile = blockIdx.x;
  const uint32_t b = blockIdx.y;
  const uint32_t row0 = tile * (uint32_t)RF_SPARSE_TILE_ROWS;
  const uint32_t left = P.n_rows - row0;   // (tile < n_tiles: row0 < n_rows)
  const uint32_t rows_here = left < (uint32_t)RF_SPARSE_TILE_ROWS ? left : (uint32_t)RF_SPARSE_TILE_ROWS;

  const int32_t q0 = P.q_off[b];
  int32_t m = P.q_off[b + 1] - q0;
  m = m < 0 ? 0 : (m > RF_SPARSE_MAX_TERMS ? RF_SPARSE_MAX_TERMS : m);

  for (uint32_t i = tid; i < (uint32_t)RF_SPARSE_TILE_ROWS; i += SPARSE_THREADS) s_acc[i] = 0.0f;
  // lane i: the slice of term i's postings that falls into this tile
  if (tid < (uint32_t)m) {
    const int64_t t = (int64_t)P.q_term[q0 + (int32_t)tid];
    int64_t lo = 0, hi = 0;
    if (t >= 0 && t < P.n_terms) {
      lo = P.post_off[t];
      hi = P.post_off[t + 1];
      lo = lo < 0 ? 0 : (lo > P.nnz ? P.nnz : lo);
      hi = hi < lo ? lo : (hi > P.nnz ? P.nnz : hi);
    }
    const int64_t beg = sparse_lower_bound(P.post_row, lo, hi, row0);
    s_beg[tid] = beg;
    s_end[tid] = sparse_lower_bound(P.post_row, beg, hi, row0 + rows_here);   // (row0 + rows_here <= n_rows < 2^31)
    s_w[tid] = P.q_weight[q0 + (int32_t)tid];
  }
  __syncthreads();

  // term after term: the barrier makes the summation order the definition's
  for (int32_t i = 0; i < m; ++i) {
    const int64_t end = s_end[i];
    const float w = s_w[i];
    for (int64_t p = s_beg[i] + tid; p < end; p += SPARSE_THREADS) {
      const uint32_t local = P.post_row[p] - row0;
      if (local < rows_here) s_acc[local] = sparse_add(s_acc[local], w, P.post_imp[p]);   // (unsigned: a row below row0 wraps past rows_here)
    }
    __syncthreads();
  }

  // hits: acc > 0 and the filter bit.  Thread tid owns slots tid + j * THREADS; a slot that is no
  // hit is zeroed, so "the largest remaining value" is all the selection needs to know.
  const bool filt_ok = P.filt == nullptr || P.filt[0] == P.n_rows;   // a header for another row count passes no row
  const uint32_t* mask = P.filt ? P.filt + RF_FILTER_HDR_WORDS : nullptr;
  unsigned long long mine = 0ull;
  for (uint32_t j = 0; j < (uint32_t)SPARSE_PER_THREAD; ++j) {
    const uint32_t local = j * SPARSE_THREADS + tid;
    const float a = s_acc[local];
    bool hit = local < rows_here && a > 0.0f && filt_ok;
    if (hit && mask) {
      const uint32_t row = row0 + local;
      hit = ((mask[row >> 5] >> (row & 31u)) & 1u) != 0u;
    }
    if (!hit) s_acc[local] = 0.0f;
    else {
      const unsigned long long key = sparse_key(a, row0 + local);
      mine = key > mine ? key : mine;
    }
  }

  // the tile's top k: one workgroup-wide maximum per slot; the owner retires its slot and looks for
  // its next best (its own slots only: no barrier for that)
  unsigned long long* out = P.lists + ((size_t)b * P.n_tiles + tile) * (size_t)P.k;
  int t = 0;
  for (; t < P.k; ++t) {
    const unsigned long long best = sparse_block_max(mine, s_wmax[t & 1]);
    if (best == 0ull) break;
    if (mine == best) {
      out[t] = best;
      s_acc[(0xFFFFFFFFu - (uint32_t)best) - row0] = 0.0f;
      mine = 0ull;
      for (uint32_t j = 0; j < (uint32_t)SPARSE_PER_THREAD; ++j) {
        const uint32_t local = j * SPARSE_THREADS + tid;
        const float a = s_acc[local];
        if (a > 0.0f) {
          const unsigned long long key = sparse_key(a, row0 + local);
          mine = key > mine ? key : mine;
        }
      }
    }
  }
  for (int o = t + (int)tid; o < P.k; o += SPARSE_THREADS) out[o] = 0ull;
}

// One workgroup per query: the n_tiles sorted lists merged by (score desc, row asc).  Thread tid
// owns lists tid + j * THREADS and a cursor into each; a round takes the largest head.
__global__ void __launch_bounds__(SPARSE_THREADS) k_sparse_merge(
    const unsigned long long* __restrict__ lists, uint32_t n_tiles, int k, int64_t id_base,
    float* __restrict__ scores, int64_t* __restrict__ ids, double* __restrict__ exact) {
  __shared__ unsigned long long s_wmax[2][SPARSE_WAVES];
  const uint32_t tid = threadIdx.x;
  const unsigned long long* mine_lists = lists + (size_t)blockIdx.x * n_tiles * (size_t)k;
  const size_t out0 = (size_t)blockIdx.x * k;

  // the head of the best list among this thread's (a list's keys descend, so its head is its best)
  unsigned long long mine = 0ull;
  uint32_t mine_list = 0u;
  int mine_pos = 0;
  for (uint32_t l = tid; l < n_tiles; l += SPARSE_THREADS) {
    const unsigned long long key = mine_lists[(size_t)l * k];
    if (key > mine) {
      mine = key;
      mine_list = l;
    }
  }
  int t = 0;
  if (n_tiles <= (uint32_t)SPARSE_THREADS) {
    // at most one list per thread: a cursor is all the state
    for (; t < k; ++t) {
      const unsigned long long best = sparse_block_max(mine, s_wmax[t & 1]);
      if (best == 0ull) break;
      if (mine == best) {
        const float s = __builtin_bit_cast(float, (uint32_t)(best >> 32));
        scores[out0 + t] = s;
        ids[out0 + t] = (int64_t)(0xFFFFFFFFu - (uint32_t)best) + id_base;
        if (exact) exact[out0 + t] = (double)s;
        ++mine_pos;
        mine = mine_pos < k ? mine_lists[(size_t)mine_list * k + mine_pos] : 0ull;
      }
    }
  } else {
    // several lists per thread: a taken key is the bound, the next head is the largest key below it
    // (keys are unique: one per row)
    unsigned long long bound = ~0ull;
    for (; t < k; ++t) {
      const unsigned long long best = sparse_block_max(mine, s_wmax[t & 1]);
      if (best == 0ull) break;
      if (tid == 0) {
        const float s = __builtin_bit_cast(float, (uint32_t)(best >> 32));
        scores[out0 + t] = s;
        ids[out0 + t] = (int64_t)(0xFFFFFFFFu - (uint32_t)best) + id_base;
        if (exact) exact[out0 + t] = (double)s;
      }
      bound = best;
      if (mine == best) {
        mine = 0ull;
        for (uint32_t l = tid; l < n_tiles; l += SPARSE_THREADS) {
          for (int p = 0; p < k; ++p) {
            const unsigned long long key = mine_lists[(size_t)l * k + p];
            if (key < bound) {
              mine = key > mine ? key : mine;
              break;
            }
          }
        }
      }
    }
  }
  for (int o = t + (int)tid; o < k; o += SPARSE_THREADS) {
    scores[out0 + o] = -INFINITY;
    ids[out0 + o] = -1;
    if (exact) exact[out0 + o] = -INFINITY;
  }
}

// ---- reciprocal-rank fusion --------------------------------------------------------------------------
struct FuseArgs {
  double w[RF_FUSE_MAX_ARMS];
  double rrf_k;
  int A, F, B, k;
};

// w / (rrf_k + rank): the sum and the division each rounded on their own
__device__ __forceinline__ double rrf_term(double w, double rrf_k, int rank) {
#pragma clang fp contract(off)
  const double den = rrf_k + (double)rank;
  return w / den;
}

// One workgroup per query; lane c = a F + j is candidate j of arm a.
__global__ void __launch_bounds__(FUSE_THREADS) k_fuse_rrf(FuseArgs P, const int64_t* __restrict__ arms,
                                                           float* __restrict__ scores, int64_t* __restrict__ ids,
                                                           double* __restrict__ exact) {
  __shared__ int64_t s_id[FUSE_THREADS];    // the candidates as the arms gave them
  __shared__ int64_t s_rep[FUSE_THREADS];   // ... and with every repeat of an id struck out (-1)
  __shared__ double s_fused[FUSE_THREADS];
  const int c = threadIdx.x;
  const int b = blockIdx.x;
  const int n = P.A * P.F;
  int64_t id = -1;
  if (c < n) {
    const int a = c / P.F, j = c % P.F;
    id = arms[((size_t)a * P.B + b) * P.F + j];
    if (id < 0) id = -1;
  }
  s_id[c] = id;
  __syncthreads();
  // the first occurrence of an id represents it
  bool rep = id >= 0;
  for (int e = 0; e < c && rep; ++e) rep = s_id[e] != id;
  double fused = -INFINITY;
  if (rep) {
    fused = 0.0;
    for (int a = 0; a < P.A; ++a) {
      for (int j = 0; j < P.F; ++j) {
        if (s_id[a * P.F + j] == id) {
          fused = fused + rrf_term(P.w[a], P.rrf_k, j + 1);
          break;
        }
      }
    }
  }
  s_fused[c] = fused;
  s_rep[c] = rep ? id : -1;   // (not into s_id: other waves are still summing over it)
  __syncthreads();
  // rank = the representatives ranked before this one by (fused desc, id asc); every lane counts them all
  int rank = 0, reps = 0;
  for (int e = 0; e < n; ++e) {
    const int64_t oid = s_rep[e];
    if (oid < 0) continue;
    const double of = s_fused[e];
    ++reps;
    rank += (of > fused || (of == fused && oid < id)) ? 1 : 0;
  }
  if (rep) {
    if (rank < P.k) {
      const size_t o = (size_t)b * P.k + rank;
      scores[o] = (float)fused;
      ids[o] = id;
      if (exact) exact[o] = fused;
    }
  }
  for (int o = reps + c; o < P.k; o += FUSE_THREADS) {
    const size_t at = (size_t)b * P.k + o;
    scores[at] = -INFINITY;
    ids[at] = -1;
    if (exact) exact[at] = -INFINITY;
  }
}

// ---- entry points ------------------------------------------------------------------------------------
static bool misaligned(const void* p) { return (((uintptr_t)p) & 15) != 0; }

extern "C" int rf_sparse_create(rf_sparse_t** out, int64_t n_rows, int64_t n_terms, int64_t nnz,
                                const int64_t* post_off_dev, const uint32_t* post_row_dev,
                                const float* post_imp_dev, int device) {
  if (out) *out = nullptr;
  if (!out || !post_off_dev || !post_row_dev || !post_imp_dev) {
    rf_set_error("rf_sparse_create: null argument");
    return RF_ERR_INVALID;
  }
  if (n_rows < 1 || n_rows >= ((int64_t)1 << 31) || n_terms < 1 || nnz < 1 || device < 0) {
    rf_set_error("rf_sparse_create: need 1 <= n_rows < 2^31, n_terms >= 1, nnz >= 1, device >= 0 (got %lld, %lld, "
                 "%lld, %d)", (long long)n_rows, (long long)n_terms, (long long)nnz, device);
    return RF_ERR_INVALID;
  }
  if (misaligned(post_off_dev) || misaligned(post_row_dev) || misaligned(post_imp_dev)) {
    rf_set_error("rf_sparse_create: the posting arrays must be 16-byte aligned");
    return RF_ERR_INVALID;
  }
  rf_sparse* sp = new (std::nothrow) rf_sparse();
  if (!sp) {
    rf_set_error("out of host memory");
    return RF_ERR_INVALID;
  }
  sp->n_rows = n_rows;
  sp->n_terms = n_terms;
  sp->nnz = nnz;
  sp->post_off = post_off_dev;
  sp->post_row = post_row_dev;
  sp->post_imp = post_imp_dev;
  sp->device = device;
  *out = sp;
  return RF_OK;
}

extern "C" int rf_sparse_destroy(rf_sparse_t* sp) {
  delete sp;
  return RF_OK;
}

static uint32_t sparse_tiles(const rf_sparse* sp) {
  return (uint32_t)((sp->n_rows + RF_SPARSE_TILE_ROWS - 1) / RF_SPARSE_TILE_ROWS);
}

extern "C" size_t rf_sparse_search_workspace_bytes(const rf_sparse_t* sp, int B, int k) {
  if (!sp || B < 1 || B > 65535 || k < 1 || k > RF_MAX_K) return 0;
  return (size_t)B * sparse_tiles(sp) * (size_t)k * sizeof(unsigned long long);
}

extern "C" int rf_sparse_search(const rf_sparse_t* sp, const void* filter_dev, const int32_t* q_off_dev,
                                const int32_t* q_term_dev, const float* q_weight_dev, int B, int k, int64_t id_base,
                                float* scores_dev, int64_t* ids_dev, double* exact_dev, void* workspace_dev,
                                size_t workspace_bytes, void* stream) {
  if (!sp || !q_off_dev || !q_term_dev || !q_weight_dev || !scores_dev || !ids_dev || !workspace_dev) {
    rf_set_error("rf_sparse_search: null argument");
    return RF_ERR_INVALID;
  }
  if (B < 1 || B > 65535 || k < 1 || k > RF_MAX_K) {
    rf_set_error("rf_sparse_search: need 1 <= B <= 65535 and 1 <= k <= %d (got B = %d, k = %d)", RF_MAX_K, B, k);
    return RF_ERR_INVALID;
  }
  if (misaligned(workspace_dev) || (filter_dev && misaligned(filter_dev))) {
    rf_set_error("rf_sparse_search: workspace and filter buffer must be 16-byte aligned");
    return RF_ERR_INVALID;
  }
  const size_t need = rf_sparse_search_workspace_bytes(sp, B, k);
  if (workspace_bytes < need) {
    rf_set_error("rf_sparse_search: workspace %zu B < required %zu B", workspace_bytes, need);
    return RF_ERR_CAPACITY;
  }
  hipStream_t st = (hipStream_t)stream;
  SparseScan P;
  P.post_off = sp->post_off;
  P.post_row = sp->post_row;
  P.post_imp = sp->post_imp;
  P.filt = (const uint32_t*)filter_dev;
  P.q_off = q_off_dev;
  P.q_term = q_term_dev;
  P.q_weight = q_weight_dev;
  P.lists = (unsigned long long*)workspace_dev;
  P.n_terms = sp->n_terms;
  P.nnz = sp->nnz;
  P.n_rows = (uint32_t)sp->n_rows;
  P.n_tiles = sparse_tiles(sp);
  P.k = k;
  hipLaunchKernelGGL(k_sparse_scan, dim3(P.n_tiles, (uint32_t)B), dim3(SPARSE_THREADS), 0, st, P);
  RF_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_sparse_merge, dim3((uint32_t)B), dim3(SPARSE_THREADS), 0, st, P.lists, P.n_tiles, k, id_base,
                     scores_dev, ids_dev, exact_dev);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

extern "C" int rf_fuse_rrf(int A, const int64_t* ids_dev, int F, const double* weights_host, double rrf_k, int B,
                           int k, float* scores_dev, int64_t* ids_dev_out, double* exact_dev, void* stream) {
  if (!ids_dev || !scores_dev || !ids_dev_out) {
    rf_set_error("rf_fuse_rrf: null argument");
    return RF_ERR_INVALID;
  }
  if (A < 1 || A > RF_FUSE_MAX_ARMS || F < 1 || F > RF_MAX_K || B < 1 || k < 1 || k > RF_MAX_K) {
    rf_set_error("rf_fuse_rrf: need 1 <= A <= %d, 1 <= F <= %d, B >= 1, 1 <= k <= %d (got A = %d, F = %d, B = %d, "
                 "k = %d)", RF_FUSE_MAX_ARMS, RF_MAX_K, RF_MAX_K, A, F, B, k);
    return RF_ERR_INVALID;
  }
  if (!(rrf_k > 0.0) || rrf_k > 1.0e300) {   // also catches a NaN and +inf
    rf_set_error("rf_fuse_rrf: rrf_k = %g must be finite and > 0", rrf_k);
    return RF_ERR_INVALID;
  }
  FuseArgs P;
  for (int a = 0; a < RF_FUSE_MAX_ARMS; ++a) {
    const double w = (weights_host && a < A) ? weights_host[a] : 1.0;
    if (!(w >= 0.0) || w > 1.0e300) {
      rf_set_error("rf_fuse_rrf: weight %d = %g must be finite and >= 0", a, w);
      return RF_ERR_INVALID;
    }
    P.w[a] = w;
  }
  P.rrf_k = rrf_k;
  P.A = A;
  P.F = F;
  P.B = B;
  P.k = k;
  hipLaunchKernelGGL(k_fuse_rrf, dim3((uint32_t)B), dim3(FUSE_THREADS), 0, (hipStream_t)stream, P, ids_dev, scores_dev,
                     ids_dev_out, exact_dev);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
