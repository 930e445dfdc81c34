// Lexical index build: a token stream -> post_off / post_row / post_tf / pos_off / pos, on the device
// (include/ragfin.h, "lexical index build").
//
// The tokens of a corpus arrive as term ids in (row, position) order.  A STABLE sort by term id alone
// puts them in (term, row, position) order, which is the order of the `pos` array:
//   rf_sparse_count_plan    the sort (least-significant-digit radix sort, 8-bit digits, the token index
//                           as payload), the row of every sorted token (binary search in row_start), the
//                           posting heads ((term, row) differs from the predecessor's) and their exclusive
//                           scan, and post_off[t] = the scan at term t's first token
//   rf_sparse_count_apply   a head at sorted index i is posting q = scan[i]: post_row[q], its first
//                           position index i (pos_off[q]), and tf[q] = the distance to the next head;
//                           pos[i] = the token's index minus its row's start
// One pass of the sort: a digit histogram per tile of RF_LEX_SORT_TILE tokens, laid out [digit][tile];
// the exclusive scan of that array is where every (digit, tile) group goes; then each tile scatters its
// tokens in rounds of one token per thread -- the lanes of a wave that hold the same digit find each
// other with eight __ballot calls (rank = popcount of the peers below), the per-wave digit counts of a
// round sit in LDS and are summed over the earlier waves, and a per-digit running base carries the
// earlier rounds.  Round, wave, lane is token order, so the scatter is stable.
// Integers only, LDS counters, no global atomics: the same bits on every run.
// Mirrored in numpy by rag_fin_amd/lexical.py (counts_from_tokens).
#include "lexical_common.h"

#define SORT_ROUNDS (RF_LEX_SORT_TILE / LEX_THREADS)

static_assert(RF_LEX_SORT_TILE % LEX_THREADS == 0, "a tile is whole rounds of one token per thread");
static_assert(LEX_THREADS == 256, "thread d of a workgroup owns digit d");

// ---- a generic in-place exclusive scan of int64 v[0 .. n), reduce-then-scan over chunks ----------------
struct LexScan {
  int64_t* v;
  int64_t n;
  int64_t* part;    // [chunks]
  int64_t chunks;
};

__global__ void __launch_bounds__(LEX_THREADS) k_lexb_scan_reduce(LexScan P) {
  __shared__ int64_t s_w[LEX_WAVES][2];
  const int64_t p0 = (int64_t)blockIdx.x * RF_LEX_CHUNK;
  int64_t a = 0, b = 0;
#pragma unroll
  for (int j = 0; j < LEX_PER_THREAD; ++j) {
    const int64_t p = p0 + j * LEX_THREADS + threadIdx.x;
    if (p < P.n) a += P.v[p];
  }
  int64_t ta, tb;
  lex_block_scan2(a, b, ta, tb, s_w);
  if (threadIdx.x == 0) P.part[blockIdx.x] = ta;
}

// one workgroup: the chunk sums become their exclusive scan, tile after tile with a running carry
__global__ void __launch_bounds__(LEX_THREADS) k_lexb_scan_parts(LexScan P) {
  __shared__ int64_t s_w[LEX_WAVES][2];
  int64_t ca = 0;
  for (int64_t c0 = 0; c0 < P.chunks; c0 += RF_LEX_CHUNK) {
    int64_t va[LEX_PER_THREAD];
    int64_t a = 0, b = 0;
#pragma unroll
    for (int j = 0; j < LEX_PER_THREAD; ++j) {   // a thread owns LEX_PER_THREAD consecutive sums
      const int64_t c = c0 + (int64_t)threadIdx.x * LEX_PER_THREAD + j;
      va[j] = c < P.chunks ? P.part[c] : 0;
      a += va[j];
    }
    int64_t ta, tb;
    lex_block_scan2(a, b, ta, tb, s_w);
    a += ca;
#pragma unroll
    for (int j = 0; j < LEX_PER_THREAD; ++j) {
      const int64_t c = c0 + (int64_t)threadIdx.x * LEX_PER_THREAD + j;
      if (c < P.chunks) P.part[c] = a;
      a += va[j];
    }
    ca += ta;
  }
}

__global__ void __launch_bounds__(LEX_THREADS) k_lexb_scan_chunks(LexScan P) {
  __shared__ int64_t s_w[LEX_WAVES][2];
  const int64_t p0 = (int64_t)blockIdx.x * RF_LEX_CHUNK;
  int64_t ca = P.part[blockIdx.x];
#pragma unroll
  for (int j = 0; j < LEX_PER_THREAD; ++j) {   // (no early exit: every thread meets the barriers)
    const int64_t p = p0 + j * LEX_THREADS + threadIdx.x;
    int64_t a = p < P.n ? P.v[p] : 0, b = 0;
    int64_t ta, tb;
    lex_block_scan2(a, b, ta, tb, s_w);
    if (p < P.n) P.v[p] = ca + a;
    ca += ta;
  }
}

static int64_t lexb_chunks(int64_t n) { return (n + RF_LEX_CHUNK - 1) / RF_LEX_CHUNK; }

static int lexb_scan(int64_t* v, int64_t n, int64_t* part, hipStream_t st) {
  LexScan P;
  P.v = v;
  P.n = n;
  P.part = part;
  P.chunks = lexb_chunks(n);
  hipLaunchKernelGGL(k_lexb_scan_reduce, dim3((uint32_t)P.chunks), dim3(LEX_THREADS), 0, st, P);
  RF_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_lexb_scan_parts, dim3(1), dim3(LEX_THREADS), 0, st, P);
  RF_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_lexb_scan_chunks, dim3((uint32_t)P.chunks), dim3(LEX_THREADS), 0, st, P);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

// ---- the sort ---------------------------------------------------------------------------------------------
struct LexSort {
  const int32_t* key_in;   // [n]: the term ids (first pass: the caller's stream, clamped on read)
  const int32_t* idx_in;   // [n] or nullptr in the first pass: the payload is the token's own index
  int32_t* key_out;
  int32_t* idx_out;
  int64_t* hist;           // [256][tiles]: the counts, then (scanned in place) the destinations
  int64_t n, tiles;
  int32_t max_key;         // n_terms - 1
  int shift;
};

__device__ __forceinline__ int32_t lexb_key(const LexSort& P, int64_t i) {
  const int32_t k = P.key_in[i];
  return k < 0 ? 0 : (k > P.max_key ? P.max_key : k);
}

__global__ void __launch_bounds__(LEX_THREADS) k_lexb_hist(LexSort P) {
  __shared__ uint32_t s_cnt[256];
  s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * RF_LEX_SORT_TILE;
#pragma unroll 4
  for (int j = 0; j < SORT_ROUNDS; ++j) {
    const int64_t i = i0 + j * LEX_THREADS + threadIdx.x;
    if (i < P.n) atomicAdd(&s_cnt[(lexb_key(P, i) >> P.shift) & 255], 1u);   // an LDS integer counter
  }
  __syncthreads();
  P.hist[(int64_t)threadIdx.x * P.tiles + blockIdx.x] = (int64_t)s_cnt[threadIdx.x];
}

__global__ void __launch_bounds__(LEX_THREADS) k_lexb_scatter(LexSort P) {
  __shared__ int64_t s_base[256];            // where the next token of digit d of this tile goes
  __shared__ uint32_t s_cnt[LEX_WAVES][256];  // the round's tokens of digit d per wave
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  s_base[threadIdx.x] = P.hist[(int64_t)threadIdx.x * P.tiles + blockIdx.x];
#pragma unroll
  for (int v = 0; v < LEX_WAVES; ++v) s_cnt[v][threadIdx.x] = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * RF_LEX_SORT_TILE;
  for (int j = 0; j < SORT_ROUNDS; ++j) {   // (no early exit: every thread meets the barriers)
    const int64_t i = i0 + j * LEX_THREADS + threadIdx.x;
    const bool valid = i < P.n;
    int32_t key = 0, idx = 0;
    if (valid) {
      key = lexb_key(P, i);
      idx = P.idx_in ? P.idx_in[i] : (int32_t)i;
    }
    const int d = (key >> P.shift) & 255;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (d >> bit) & 1;
      const unsigned long long m = __ballot(one);
      peers &= one ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rank == 0) s_cnt[w][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      int64_t dst = s_base[d] + rank;
#pragma unroll
      for (int v = 0; v < LEX_WAVES; ++v)
        if (v < w) dst += s_cnt[v][d];
      if (dst >= 0 && dst < P.n) {   // (always, for a histogram of these very keys)
        P.key_out[dst] = key;
        P.idx_out[dst] = idx;
      }
    }
    __syncthreads();
    uint32_t tot = 0;
#pragma unroll
    for (int v = 0; v < LEX_WAVES; ++v) {
      tot += s_cnt[v][threadIdx.x];
      s_cnt[v][threadIdx.x] = 0;
    }
    s_base[threadIdx.x] += tot;
    __syncthreads();
  }
}

// ---- rows, heads, term offsets ------------------------------------------------------------------------------
struct LexCount {
  const int32_t* key;        // [n] sorted term ids
  const int32_t* idx;        // [n] the token index of every sorted token
  const int64_t* row_start;  // [n_rows + 1]
  uint32_t* row;             // [n]
  int64_t* heads;            // [n + 1]: the head flags, then their exclusive scan closed by nnz
  int64_t* start;            // [n + 1]: first sorted index of every posting (pos_off when positions are wanted)
  int64_t* post_off;         // [n_terms + 1]
  int64_t* totals;           // [2]: nnz, n_pos
  int64_t n, n_rows, n_terms;
};

// the last r in [0, n_rows - 1] with row_start[r] <= i (0 if none)
__device__ __forceinline__ int64_t lexb_row_of(const int64_t* __restrict__ row_start, int64_t n_rows, int64_t i) {
  int64_t lo = 0, hi = n_rows - 1;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo + 1) >> 1);
    if (row_start[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(LEX_THREADS) k_lexb_rows(LexCount P) {
  const int64_t i = (int64_t)blockIdx.x * LEX_THREADS + threadIdx.x;
  if (i < P.n) P.row[i] = (uint32_t)lexb_row_of(P.row_start, P.n_rows, lex_clamp(P.idx[i], 0, P.n - 1));
}

__global__ void __launch_bounds__(LEX_THREADS) k_lexb_heads(LexCount P) {
  const int64_t i = (int64_t)blockIdx.x * LEX_THREADS + threadIdx.x;
  if (i < P.n) P.heads[i] = (i == 0 || P.key[i] != P.key[i - 1] || P.row[i] != P.row[i - 1]) ? 1 : 0;
  else if (i == P.n) P.heads[i] = 0;
}

// post_off[t] = the scan at the first sorted token whose term is >= t; t = n_terms closes with nnz
__global__ void __launch_bounds__(LEX_THREADS) k_lexb_terms(LexCount P) {
  const int64_t t = (int64_t)blockIdx.x * LEX_THREADS + threadIdx.x;
  if (t > P.n_terms) return;
  int64_t lo = 0, hi = P.n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)P.key[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  P.post_off[t] = P.heads[lo];
  if (t == 0) {
    P.totals[0] = P.heads[P.n];
    P.totals[1] = P.n;
  }
}

struct LexCountOut {
  uint32_t* post_row;
  uint32_t* post_tf;
  uint32_t* pos;   // or nullptr
  int64_t nnz, n_pos;
};

__global__ void __launch_bounds__(LEX_THREADS) k_lexb_apply_heads(LexCount P, LexCountOut O) {
  const int64_t i = (int64_t)blockIdx.x * LEX_THREADS + threadIdx.x;
  if (i > P.n) return;
  const int64_t q = P.heads[i];
  if (i == P.n) {   // the closing offset
    if (q >= 0 && q <= O.nnz) P.start[q] = P.n;
    return;
  }
  const uint32_t row = P.row[i];
  if (P.heads[i + 1] != q && q >= 0 && q < O.nnz) {   // a head
    O.post_row[q] = row;
    P.start[q] = i;
  }
  if (O.pos && i < O.n_pos) {
    const int64_t at = (int64_t)P.idx[i] - P.row_start[row];
    O.pos[i] = (uint32_t)lex_clamp(at, 0, 0xffffffffll);
  }
}

__global__ void __launch_bounds__(LEX_THREADS) k_lexb_apply_tf(const int64_t* __restrict__ start, LexCountOut O, int64_t n) {
  const int64_t q = (int64_t)blockIdx.x * LEX_THREADS + threadIdx.x;
  if (q < O.nnz) O.post_tf[q] = (uint32_t)lex_clamp(start[q + 1] - start[q], 0, n);
}

// ---- entry points ---------------------------------------------------------------------------------------
static bool misaligned(const void* p) { return (((uintptr_t)p) & 15) != 0; }
static size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

static int lexb_passes(int64_t n_terms) {
  int bits = 1;
  while (bits < 32 && ((int64_t)1 << bits) < n_terms) ++bits;   // bits of the largest id, n_terms - 1
  return (bits + 7) / 8;
}

// the workspace: two (key, idx) buffers the passes alternate between, then the arrays of the count
struct LexBuildWs {
  int32_t* key[2];
  int32_t* idx[2];
  uint32_t* row;
  int64_t* heads;
  int64_t* start;
  int64_t* hist;
  int64_t* part;
  int64_t tiles;
  size_t bytes;
};

static bool lexb_in_range(int64_t n_tokens, int64_t n_terms) {
  return n_tokens >= 1 && n_tokens < ((int64_t)1 << 31) && n_terms >= 1 && n_terms < ((int64_t)1 << 31);
}

static LexBuildWs lexb_carve(void* base, int64_t n) {
  LexBuildWs W;
  W.tiles = (n + RF_LEX_SORT_TILE - 1) / RF_LEX_SORT_TILE;
  const int64_t scan_n = 256 * W.tiles > n + 1 ? 256 * W.tiles : n + 1;
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t b) {
    char* at = p + off;
    off += up16(b);
    return (void*)at;
  };
  for (int k = 0; k < 2; ++k) W.key[k] = (int32_t*)take((size_t)n * sizeof(int32_t));
  for (int k = 0; k < 2; ++k) W.idx[k] = (int32_t*)take((size_t)n * sizeof(int32_t));
  W.row = (uint32_t*)take((size_t)n * sizeof(uint32_t));
  W.heads = (int64_t*)take((size_t)(n + 1) * sizeof(int64_t));
  W.start = (int64_t*)take((size_t)(n + 1) * sizeof(int64_t));
  W.hist = (int64_t*)take((size_t)(256 * W.tiles) * sizeof(int64_t));
  W.part = (int64_t*)take((size_t)lexb_chunks(scan_n) * sizeof(int64_t));
  W.bytes = off;
  return W;
}

extern "C" size_t rf_sparse_count_workspace_bytes(int64_t n_tokens, int64_t n_terms) {
  if (!lexb_in_range(n_tokens, n_terms)) return 0;
  return lexb_carve(nullptr, n_tokens).bytes;
}

static bool lexb_args_ok(const char* fn, const int64_t* row_start_dev, int64_t n_tokens, int64_t n_rows, int64_t n_terms,
                         void* workspace_dev, size_t workspace_bytes) {
  if (!row_start_dev || !workspace_dev) {
    rf_set_error("%s: null argument", fn);
    return false;
  }
  if (!lexb_in_range(n_tokens, n_terms) || n_rows < 1 || n_rows >= ((int64_t)1 << 31)) {
    rf_set_error("%s: need 1 <= n_tokens < 2^31, 1 <= n_rows < 2^31, 1 <= n_terms < 2^31 (got %lld, %lld, %lld)", fn,
                 (long long)n_tokens, (long long)n_rows, (long long)n_terms);
    return false;
  }
  if (misaligned(row_start_dev) || misaligned(workspace_dev)) {
    rf_set_error("%s: every array must be 16-byte aligned", fn);
    return false;
  }
  const size_t need = rf_sparse_count_workspace_bytes(n_tokens, n_terms);
  if (workspace_bytes < need) {
    rf_set_error("%s: workspace %zu B < required %zu B", fn, workspace_bytes, need);
    return false;
  }
  return true;
}

static LexCount lexb_count(const LexBuildWs& W, const int64_t* row_start_dev, int64_t n_tokens, int64_t n_rows,
                           int64_t n_terms) {
  const int last = (lexb_passes(n_terms) - 1) & 1;   // pass p writes buffer p & 1
  LexCount C;
  C.key = W.key[last];
  C.idx = W.idx[last];
  C.row_start = row_start_dev;
  C.row = W.row;
  C.heads = W.heads;
  C.start = W.start;
  C.post_off = nullptr;
  C.totals = nullptr;
  C.n = n_tokens;
  C.n_rows = n_rows;
  C.n_terms = n_terms;
  return C;
}

extern "C" int rf_sparse_count_plan(const int32_t* tok_dev, const int64_t* row_start_dev, int64_t n_tokens, int64_t n_rows,
                                    int64_t n_terms, int64_t* post_off_dev, int64_t* totals_dev, void* workspace_dev,
                                    size_t workspace_bytes, void* stream) {
  const char* fn = "rf_sparse_count_plan";
  if (!tok_dev || !post_off_dev || !totals_dev) {
    rf_set_error("%s: null argument", fn);
    return RF_ERR_INVALID;
  }
  if (!lexb_args_ok(fn, row_start_dev, n_tokens, n_rows, n_terms, workspace_dev, workspace_bytes)) return RF_ERR_INVALID;
  if (misaligned(tok_dev) || misaligned(post_off_dev) || (((uintptr_t)totals_dev) & 7) != 0) {
    rf_set_error("%s: tok_dev and post_off_dev must be 16-byte aligned, totals_dev 8-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const LexBuildWs W = lexb_carve(workspace_dev, n_tokens);
  const int passes = lexb_passes(n_terms);
  for (int p = 0; p < passes; ++p) {
    LexSort S;
    S.key_in = p == 0 ? tok_dev : W.key[(p - 1) & 1];
    S.idx_in = p == 0 ? nullptr : W.idx[(p - 1) & 1];
    S.key_out = W.key[p & 1];
    S.idx_out = W.idx[p & 1];
    S.hist = W.hist;
    S.n = n_tokens;
    S.tiles = W.tiles;
    S.max_key = (int32_t)(n_terms - 1);
    S.shift = 8 * p;
    hipLaunchKernelGGL(k_lexb_hist, dim3((uint32_t)W.tiles), dim3(LEX_THREADS), 0, st, S);
    RF_HIP(hipGetLastError());
    const int rc = lexb_scan(W.hist, 256 * W.tiles, W.part, st);
    if (rc != RF_OK) return rc;
    hipLaunchKernelGGL(k_lexb_scatter, dim3((uint32_t)W.tiles), dim3(LEX_THREADS), 0, st, S);
    RF_HIP(hipGetLastError());
  }
  LexCount C = lexb_count(W, row_start_dev, n_tokens, n_rows, n_terms);
  C.post_off = post_off_dev;
  C.totals = totals_dev;
  const uint32_t grid = (uint32_t)((n_tokens + 1 + LEX_THREADS - 1) / LEX_THREADS);
  hipLaunchKernelGGL(k_lexb_rows, dim3(grid), dim3(LEX_THREADS), 0, st, C);
  RF_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_lexb_heads, dim3(grid), dim3(LEX_THREADS), 0, st, C);
  RF_HIP(hipGetLastError());
  const int rc = lexb_scan(W.heads, n_tokens + 1, W.part, st);
  if (rc != RF_OK) return rc;
  hipLaunchKernelGGL(k_lexb_terms, dim3((uint32_t)((n_terms + 1 + LEX_THREADS - 1) / LEX_THREADS)), dim3(LEX_THREADS), 0, st,
                     C);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

extern "C" int rf_sparse_count_apply(const int64_t* row_start_dev, int64_t n_tokens, int64_t n_rows, int64_t n_terms,
                                     void* workspace_dev, size_t workspace_bytes, const rf_postings* out, int want_positions,
                                     void* stream) {
  const char* fn = "rf_sparse_count_apply";
  if (!out) {
    rf_set_error("%s: out is NULL", fn);
    return RF_ERR_INVALID;
  }
  if (!lexb_args_ok(fn, row_start_dev, n_tokens, n_rows, n_terms, workspace_dev, workspace_bytes)) return RF_ERR_INVALID;
  const bool pos = want_positions != 0;
  if (out->nnz < 1 || out->nnz > n_tokens || out->n_pos < 0 || !out->post_row || !out->post_tf ||
      (pos && (!out->pos_off || !out->pos || out->n_pos < 1))) {
    rf_set_error("%s: out needs 1 <= nnz <= n_tokens, post_row and post_tf, and with positions pos_off, pos and n_pos >= 1",
                 fn);
    return RF_ERR_INVALID;
  }
  if (misaligned(out->post_row) || misaligned(out->post_tf) || (pos && (misaligned(out->pos_off) || misaligned(out->pos)))) {
    rf_set_error("%s: the arrays of out must be 16-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const LexBuildWs W = lexb_carve(workspace_dev, n_tokens);
  LexCount C = lexb_count(W, row_start_dev, n_tokens, n_rows, n_terms);
  if (pos) C.start = out->pos_off;   // [nnz + 1]: a head's sorted index is its first position
  LexCountOut O;
  O.post_row = out->post_row;
  O.post_tf = out->post_tf;
  O.pos = pos ? out->pos : nullptr;
  O.nnz = out->nnz;
  O.n_pos = pos ? out->n_pos : 0;
  hipLaunchKernelGGL(k_lexb_apply_heads, dim3((uint32_t)((n_tokens + 1 + LEX_THREADS - 1) / LEX_THREADS)), dim3(LEX_THREADS),
                     0, st, C, O);
  RF_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_lexb_apply_tf, dim3((uint32_t)((O.nnz + LEX_THREADS - 1) / LEX_THREADS)), dim3(LEX_THREADS), 0, st,
                     (const int64_t*)C.start, O, n_tokens);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
