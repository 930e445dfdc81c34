// Lexical index maintenance: the posting arrays after an append or a delete, on the device
// (include/ragfin.h, "lexical index maintenance").
//
// With the term frequencies kept beside the postings every BM25 impact is re-derivable, so a write
// never needs the texts of the surviving rows:
//   rf_sparse_impacts        imp = float32(idf * ((tf (k1 + 1)) / (tf + k1 ((1 - b) + b (dl / avgdl))))), fp64,
//                            one rounding per operation (contraction off), idf from the host
//   rf_sparse_append         per merged term: the old segment, then the delta segment (rows + n_old)
//   rf_sparse_compact_plan   exclusive scans of the kept-posting flags and kept position counts
//   rf_sparse_compact_apply  scatter of the kept postings, rows renumbered through the row map
// Every kernel works on chunks of RF_LEX_CHUNK postings: lane-strided (coalesced) reads of the
// posting arrays, the chunk's term range found once by two binary searches and a posting's term inside
// that range.  Integers only apart from the impacts, no atomics: the same bits on every run.
// Mirrored in numpy by rag_fin_amd/lexical.py (append_reference, compact_reference, impacts).
#include "lexical_common.h"

// the device view of one rf_postings (n_pos, pos_off, pos: 0 / nullptr without positions)
struct LexSide {
  const int64_t* post_off;
  const uint32_t* post_row;
  const uint32_t* post_tf;
  const int64_t* pos_off;
  const uint32_t* pos;
  int64_t n_rows, n_terms, nnz, n_pos;
};
struct LexOut {
  uint32_t* post_row;
  uint32_t* post_tf;
  int64_t* pos_off;
  uint32_t* pos;
  int64_t nnz, n_pos;
};

// the last t in [lo, hi] with off[t] <= p (lo if none): the term that owns posting p
__device__ __forceinline__ int64_t lex_term_of(const int64_t* __restrict__ off, int64_t lo, int64_t hi, int64_t p) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo + 1) >> 1);
    if (off[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The terms of the chunk that starts at p0, [s_t[0], s_t[1]], inside [0, n_terms - 1]: known to every
// thread after the barrier.
__device__ __forceinline__ void lex_chunk_terms(const int64_t* __restrict__ off, int64_t n_terms, int64_t nnz, int64_t p0,
                                                int64_t* s_t) {
  if (threadIdx.x < 2) {
    const int64_t last = p0 + RF_LEX_CHUNK - 1 < nnz - 1 ? p0 + RF_LEX_CHUNK - 1 : nnz - 1;
    s_t[threadIdx.x] = lex_term_of(off, 0, n_terms - 1, threadIdx.x == 0 ? p0 : last);
  }
  __syncthreads();
}

// the positions of posting p: `lo` inside [0, n_pos], `cnt` >= 0 with lo + cnt <= n_pos
__device__ __forceinline__ void lex_pos_range(const int64_t* __restrict__ pos_off, int64_t p, int64_t n_pos, int64_t& lo,
                                              int64_t& cnt) {
  lo = lex_clamp(pos_off[p], 0, n_pos);
  const int64_t hi = lex_clamp(pos_off[p + 1], lo, n_pos);
  cnt = hi - lo;
}

// ---- impacts ------------------------------------------------------------------------------------------
struct LexImpacts {
  const int64_t* post_off;
  const uint32_t* post_row;
  const uint32_t* post_tf;
  const double* idf;
  const int32_t* dl;
  float* post_imp;
  int64_t n_rows, n_terms, nnz;
  double avgdl, k1, k1p1, omb, b;   // k1p1 = k1 + 1, omb = 1 - b: formed once, in fp64, on the host
};

__device__ __forceinline__ float lex_impact(double idf, double tf, double dl, const LexImpacts& P) {
#pragma clang fp contract(off)
  const double ratio = dl / P.avgdl;
  const double scaled = P.b * ratio;
  const double norm = P.omb + scaled;
  const double knorm = P.k1 * norm;
  const double den = tf + knorm;
  const double num = tf * P.k1p1;
  const double frac = num / den;
  const double imp = idf * frac;
  return (float)imp;
}

__global__ void __launch_bounds__(LEX_THREADS) k_lex_impacts(LexImpacts P) {
  __shared__ int64_t s_t[2];
  const int64_t p0 = (int64_t)blockIdx.x * RF_LEX_CHUNK;
  lex_chunk_terms(P.post_off, P.n_terms, P.nnz, p0, s_t);
  const int64_t t_lo = s_t[0], t_hi = s_t[1];
#pragma unroll
  for (int j = 0; j < LEX_PER_THREAD; ++j) {
    const int64_t p = p0 + j * LEX_THREADS + threadIdx.x;
    if (p >= P.nnz) break;
    const int64_t t = lex_term_of(P.post_off, t_lo, t_hi, p);
    const uint32_t row = P.post_row[p];
    float imp = 0.0f;   // a row outside the index: skipped, as rf_sparse_search skips it
    if ((int64_t)row < P.n_rows) imp = lex_impact(P.idf[t], (double)P.post_tf[p], (double)P.dl[row], P);
    P.post_imp[p] = imp;
  }
}

// ---- the compaction plan (the prefix sum helpers: lexical_common.h) ------------------------------------
struct LexPlan {
  LexSide S;
  const int32_t* row_map;   // [n_rows]: the new row number, or < 0
  int64_t* dst_post;        // [nnz + 1]
  int64_t* dst_pos;         // [nnz + 1] or nullptr
  int64_t* term_dst;        // [n_terms + 2]
  int64_t* part_post;       // [chunks]
  int64_t* part_pos;        // [chunks]
  int64_t chunks;
};

// (kept flag, kept position count) of posting p
__device__ __forceinline__ void lex_kept(const LexPlan& P, int64_t p, int64_t& flag, int64_t& npos) {
  const uint32_t row = P.S.post_row[p];
  flag = ((int64_t)row < P.S.n_rows && P.row_map[row] >= 0) ? 1 : 0;
  npos = 0;
  if (flag && P.dst_pos) {
    int64_t lo;
    lex_pos_range(P.S.pos_off, p, P.S.n_pos, lo, npos);
  }
}

__global__ void __launch_bounds__(LEX_THREADS) k_lex_plan_reduce(LexPlan P) {
  __shared__ int64_t s_w[LEX_WAVES][2];
  const int64_t p0 = (int64_t)blockIdx.x * RF_LEX_CHUNK;
  int64_t a = 0, b = 0;
#pragma unroll
  for (int j = 0; j < LEX_PER_THREAD; ++j) {
    const int64_t p = p0 + j * LEX_THREADS + threadIdx.x;
    if (p < P.S.nnz) {
      int64_t f, n;
      lex_kept(P, p, f, n);
      a += f;
      b += n;
    }
  }
  int64_t ta, tb;
  lex_block_scan2(a, b, ta, tb, s_w);
  if (threadIdx.x == 0) {
    P.part_post[blockIdx.x] = ta;
    P.part_pos[blockIdx.x] = tb;
  }
}

// One workgroup: the chunk sums become their exclusive scan, tile after tile of RF_LEX_CHUNK sums with a
// running carry; the totals close dst_post / dst_pos.
__global__ void __launch_bounds__(LEX_THREADS) k_lex_plan_scan_parts(LexPlan P) {
  __shared__ int64_t s_w[LEX_WAVES][2];
  int64_t ca = 0, cb = 0;
  for (int64_t c0 = 0; c0 < P.chunks; c0 += RF_LEX_CHUNK) {
    int64_t va[LEX_PER_THREAD], vb[LEX_PER_THREAD];
    int64_t a = 0, b = 0;
#pragma unroll
    for (int j = 0; j < LEX_PER_THREAD; ++j) {   // a thread owns LEX_PER_THREAD consecutive sums
      const int64_t c = c0 + (int64_t)threadIdx.x * LEX_PER_THREAD + j;
      va[j] = c < P.chunks ? P.part_post[c] : 0;
      vb[j] = c < P.chunks ? P.part_pos[c] : 0;
      a += va[j];
      b += vb[j];
    }
    int64_t ta, tb;
    lex_block_scan2(a, b, ta, tb, s_w);
    a += ca;
    b += cb;
#pragma unroll
    for (int j = 0; j < LEX_PER_THREAD; ++j) {
      const int64_t c = c0 + (int64_t)threadIdx.x * LEX_PER_THREAD + j;
      if (c < P.chunks) {
        P.part_post[c] = a;
        P.part_pos[c] = b;
      }
      a += va[j];
      b += vb[j];
    }
    ca += ta;
    cb += tb;
  }
  if (threadIdx.x == 0) {
    P.dst_post[P.S.nnz] = ca;
    if (P.dst_pos) P.dst_pos[P.S.nnz] = cb;
  }
}

__global__ void __launch_bounds__(LEX_THREADS) k_lex_plan_scan_chunks(LexPlan P) {
  __shared__ int64_t s_w[LEX_WAVES][2];
  const int64_t p0 = (int64_t)blockIdx.x * RF_LEX_CHUNK;
  int64_t ca = P.part_post[blockIdx.x], cb = P.part_pos[blockIdx.x];
#pragma unroll
  for (int j = 0; j < LEX_PER_THREAD; ++j) {   // (no early exit: every thread meets the barriers)
    const int64_t p = p0 + j * LEX_THREADS + threadIdx.x;
    int64_t a = 0, b = 0;
    if (p < P.S.nnz) lex_kept(P, p, a, b);
    int64_t ta, tb;
    lex_block_scan2(a, b, ta, tb, s_w);
    if (p < P.S.nnz) {
      P.dst_post[p] = ca + a;
      if (P.dst_pos) P.dst_pos[p] = cb + b;
    }
    ca += ta;
    cb += tb;
  }
}

// term_dst[t] = dst_post[post_off[t]] for t = 0 .. n_terms; term_dst[n_terms + 1] = the kept positions
__global__ void __launch_bounds__(LEX_THREADS) k_lex_plan_terms(LexPlan P) {
  const int64_t t = (int64_t)blockIdx.x * LEX_THREADS + threadIdx.x;
  if (t <= P.S.n_terms) P.term_dst[t] = P.dst_post[lex_clamp(P.S.post_off[t], 0, P.S.nnz)];
  else if (t == P.S.n_terms + 1) P.term_dst[t] = P.dst_pos ? P.dst_pos[P.S.nnz] : 0;
}

// ---- scatter --------------------------------------------------------------------------------------------
// posting p of S goes to slot q of O with row `row`; its positions to O.pos[d ..)
__device__ __forceinline__ void lex_put(const LexSide& S, const LexOut& O, int64_t p, int64_t q, uint32_t row, int64_t d) {
  if (q < 0 || q >= O.nnz) return;
  O.post_row[q] = row;
  O.post_tf[q] = S.post_tf[p];
  if (O.pos_off) {
    int64_t lo, cnt;
    lex_pos_range(S.pos_off, p, S.n_pos, lo, cnt);
    d = lex_clamp(d, 0, O.n_pos);
    O.pos_off[q] = d;
    if (cnt > O.n_pos - d) cnt = O.n_pos - d;
    for (int64_t j = 0; j < cnt; ++j) O.pos[d + j] = S.pos[lo + j];
  }
}

struct LexApply {
  LexSide S;
  LexOut O;
  const int32_t* row_map;
  const int64_t* dst_post;
  const int64_t* dst_pos;
};

__global__ void __launch_bounds__(LEX_THREADS) k_lex_compact_apply(LexApply P) {
  const int64_t p0 = (int64_t)blockIdx.x * RF_LEX_CHUNK;
#pragma unroll
  for (int j = 0; j < LEX_PER_THREAD; ++j) {
    const int64_t p = p0 + j * LEX_THREADS + threadIdx.x;
    if (p >= P.S.nnz) break;
    const uint32_t row = P.S.post_row[p];
    if ((int64_t)row < P.S.n_rows) {
      const int32_t to = P.row_map[row];
      if (to >= 0) lex_put(P.S, P.O, p, P.dst_post[p], (uint32_t)to, P.O.pos_off ? P.dst_pos[p] : 0);
    }
    if (p == P.S.nnz - 1 && P.O.pos_off) {   // the closing offset
      const int64_t q = P.dst_post[P.S.nnz];
      if (q >= 0 && q <= P.O.nnz) P.O.pos_off[q] = lex_clamp(P.dst_pos[P.S.nnz], 0, P.O.n_pos);
    }
  }
}

struct LexAppend {
  LexSide A, D;              // the old postings and the delta
  LexOut O;                  // the merged postings
  const int64_t* map_old;    // [A.n_terms] merged id of an old term
  const int64_t* map_delta;  // [D.n_terms] merged id of a delta term
  const int64_t* post_off;   // [n_terms + 1] of the merged postings
  int64_t n_terms;
  int64_t* base_old;         // [A.n_terms] slot of an old posting p = p + base_old[t]
  int64_t* shift_old;        // [A.n_terms] its positions start at pos_off[p] + shift_old[t]
  int64_t* base_delta;       // [D.n_terms]
  int64_t* shift_delta;      // [D.n_terms]
};

// entries of the ascending map[0 .. n) below m (strict) or at most m
__device__ __forceinline__ int64_t lex_count_below(const int64_t* __restrict__ map, int64_t n, int64_t m, bool strict) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (strict ? map[mid] < m : map[mid] <= m) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Per term of either side: where its postings and their positions go.  A merged term's list is its old
// segment, then its delta segment; the positions are laid out in the same order, so an old posting's
// positions move up by the delta positions of every smaller merged term, and a delta posting's by the old
// positions of every merged term up to its own.
__global__ void __launch_bounds__(LEX_THREADS) k_lex_append_tables(LexAppend P) {
  const int64_t i = (int64_t)blockIdx.x * LEX_THREADS + threadIdx.x;
  const bool pos = P.O.pos_off != nullptr;
  if (i < P.A.n_terms) {
    const int64_t m = lex_clamp(P.map_old[i], 0, P.n_terms - 1);
    P.base_old[i] = P.post_off[m] - P.A.post_off[i];
    const int64_t before = lex_count_below(P.map_delta, P.D.n_terms, m, true);
    P.shift_old[i] = pos ? P.D.pos_off[lex_clamp(P.D.post_off[before], 0, P.D.nnz)] : 0;
  } else if (i < P.A.n_terms + P.D.n_terms) {
    const int64_t d = i - P.A.n_terms;
    const int64_t m = lex_clamp(P.map_delta[d], 0, P.n_terms - 1);
    P.base_delta[d] = P.post_off[m + 1] - P.D.post_off[d + 1];
    const int64_t upto = lex_count_below(P.map_old, P.A.n_terms, m, false);
    P.shift_delta[d] = pos ? P.A.pos_off[lex_clamp(P.A.post_off[upto], 0, P.A.nnz)] : 0;
  }
  if (i == 0 && pos) P.O.pos_off[P.O.nnz] = P.O.n_pos;
}

// one side of the append: S's postings to their slots, rows + row_add
__global__ void __launch_bounds__(LEX_THREADS) k_lex_append_move(LexSide S, LexOut O, const int64_t* __restrict__ base,
                                                                 const int64_t* __restrict__ shift, uint32_t row_add) {
  __shared__ int64_t s_t[2];
  const int64_t p0 = (int64_t)blockIdx.x * RF_LEX_CHUNK;
  lex_chunk_terms(S.post_off, S.n_terms, S.nnz, p0, s_t);
  const int64_t t_lo = s_t[0], t_hi = s_t[1];
#pragma unroll
  for (int j = 0; j < LEX_PER_THREAD; ++j) {
    const int64_t p = p0 + j * LEX_THREADS + threadIdx.x;
    if (p >= S.nnz) break;
    const int64_t t = lex_term_of(S.post_off, t_lo, t_hi, p);
    int64_t d = 0;
    if (O.pos_off) d = lex_clamp(S.pos_off[p], 0, S.n_pos) + shift[t];
    lex_put(S, O, p, p + base[t], S.post_row[p] + row_add, d);
  }
}

// ---- entry points ---------------------------------------------------------------------------------------
static bool misaligned(const void* p) { return (((uintptr_t)p) & 15) != 0; }

static int64_t lex_chunks(int64_t nnz) { return (nnz + RF_LEX_CHUNK - 1) / RF_LEX_CHUNK; }

// the host-side checks of one rf_postings; need_post_off: an input side or the merged output
static bool lex_side_ok(const char* fn, const char* what, const rf_postings* a, bool need_post_off, int64_t min_nnz) {
  if (!a) {
    rf_set_error("%s: %s is NULL", fn, what);
    return false;
  }
  if (a->n_rows < 0 || a->n_rows >= ((int64_t)1 << 31) || a->n_terms < 0 || a->nnz < min_nnz || a->n_pos < 0 ||
      lex_chunks(a->nnz) >= ((int64_t)1 << 31)) {
    rf_set_error("%s: %s needs 0 <= n_rows < 2^31, n_terms >= 0, nnz >= %lld, n_pos >= 0 (got %lld, %lld, %lld, %lld)", fn,
                 what, (long long)min_nnz, (long long)a->n_rows, (long long)a->n_terms, (long long)a->nnz,
                 (long long)a->n_pos);
    return false;
  }
  if (!a->post_row || !a->post_tf || (need_post_off && !a->post_off) || ((a->pos_off == nullptr) != (a->pos == nullptr))) {
    rf_set_error("%s: %s has a NULL array (pos_off and pos are given together or not at all)", fn, what);
    return false;
  }
  if (misaligned(a->post_off) || misaligned(a->post_row) || misaligned(a->post_tf) || misaligned(a->pos_off) ||
      misaligned(a->pos)) {
    rf_set_error("%s: the arrays of %s must be 16-byte aligned", fn, what);
    return false;
  }
  return true;
}

static LexSide lex_side(const rf_postings* a) {
  LexSide S;
  S.post_off = a->post_off;
  S.post_row = a->post_row;
  S.post_tf = a->post_tf;
  S.pos_off = a->pos_off;
  S.pos = a->pos;
  S.n_rows = a->n_rows;
  S.n_terms = a->n_terms;
  S.nnz = a->nnz;
  S.n_pos = a->pos_off ? a->n_pos : 0;
  return S;
}

static LexOut lex_out(const rf_postings* a) {
  LexOut O;
  O.post_row = a->post_row;
  O.post_tf = a->post_tf;
  O.pos_off = a->pos_off;
  O.pos = a->pos;
  O.nnz = a->nnz;
  O.n_pos = a->pos_off ? a->n_pos : 0;
  return O;
}

extern "C" int rf_sparse_impacts(const int64_t* post_off_dev, const uint32_t* post_row_dev, const uint32_t* post_tf_dev,
                                 const double* idf_dev, const int32_t* dl_dev, int64_t n_rows, int64_t n_terms, int64_t nnz,
                                 double avgdl, double k1, double b, float* post_imp_dev, void* stream) {
  if (!post_off_dev || !post_row_dev || !post_tf_dev || !idf_dev || !dl_dev || !post_imp_dev) {
    rf_set_error("rf_sparse_impacts: null argument");
    return RF_ERR_INVALID;
  }
  if (n_rows < 1 || n_rows >= ((int64_t)1 << 31) || n_terms < 1 || nnz < 1 || lex_chunks(nnz) >= ((int64_t)1 << 31)) {
    rf_set_error("rf_sparse_impacts: need 1 <= n_rows < 2^31, n_terms >= 1, nnz >= 1 (got %lld, %lld, %lld)",
                 (long long)n_rows, (long long)n_terms, (long long)nnz);
    return RF_ERR_INVALID;
  }
  if (!(avgdl > 0.0) || avgdl > 1.0e300 || !(k1 >= 0.0) || k1 > 1.0e300 || !(b >= 0.0) || !(b <= 1.0)) {
    rf_set_error("rf_sparse_impacts: need avgdl > 0, k1 >= 0, 0 <= b <= 1, all finite (got %g, %g, %g)", avgdl, k1, b);
    return RF_ERR_INVALID;
  }
  if (misaligned(post_off_dev) || misaligned(post_row_dev) || misaligned(post_tf_dev) || misaligned(idf_dev) ||
      misaligned(dl_dev) || misaligned(post_imp_dev)) {
    rf_set_error("rf_sparse_impacts: every array must be 16-byte aligned");
    return RF_ERR_INVALID;
  }
  LexImpacts P;
  P.post_off = post_off_dev;
  P.post_row = post_row_dev;
  P.post_tf = post_tf_dev;
  P.idf = idf_dev;
  P.dl = dl_dev;
  P.post_imp = post_imp_dev;
  P.n_rows = n_rows;
  P.n_terms = n_terms;
  P.nnz = nnz;
  P.avgdl = avgdl;
  P.k1 = k1;
  P.k1p1 = k1 + 1.0;
  P.omb = 1.0 - b;
  P.b = b;
  hipLaunchKernelGGL(k_lex_impacts, dim3((uint32_t)lex_chunks(nnz)), dim3(LEX_THREADS), 0, (hipStream_t)stream, P);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

extern "C" size_t rf_sparse_append_workspace_bytes(int64_t n_terms_old, int64_t n_terms_delta) {
  if (n_terms_old < 0 || n_terms_delta < 0) return 0;
  return (size_t)(n_terms_old + n_terms_delta + 1) * 2 * sizeof(int64_t);
}

extern "C" int rf_sparse_append(const rf_postings* old_p, const rf_postings* delta, const int64_t* map_old_dev,
                                const int64_t* map_delta_dev, const rf_postings* merged, void* workspace_dev,
                                size_t workspace_bytes, void* stream) {
  const char* fn = "rf_sparse_append";
  if (!lex_side_ok(fn, "old", old_p, true, 1) || !lex_side_ok(fn, "delta", delta, true, 0) ||
      !lex_side_ok(fn, "merged", merged, true, 1))
    return RF_ERR_INVALID;
  if (!map_old_dev || !map_delta_dev || !workspace_dev) {
    rf_set_error("rf_sparse_append: null argument");
    return RF_ERR_INVALID;
  }
  if (misaligned(map_old_dev) || misaligned(map_delta_dev) || misaligned(workspace_dev)) {
    rf_set_error("rf_sparse_append: the term maps and the workspace must be 16-byte aligned");
    return RF_ERR_INVALID;
  }
  const bool pos = merged->pos_off != nullptr;
  if (old_p->n_terms < 1 || merged->n_terms < old_p->n_terms || merged->n_terms > old_p->n_terms + delta->n_terms ||
      merged->nnz != old_p->nnz + delta->nnz || merged->n_rows != old_p->n_rows + delta->n_rows ||
      (old_p->pos_off != nullptr) != pos || (delta->pos_off != nullptr) != pos ||
      (pos && merged->n_pos != old_p->n_pos + delta->n_pos)) {
    rf_set_error("rf_sparse_append: the merged postings must hold the rows, postings and positions of both sides, and "
                 "between n_terms(old) and n_terms(old) + n_terms(delta) terms; positions on all three or on none");
    return RF_ERR_INVALID;
  }
  const size_t need = rf_sparse_append_workspace_bytes(old_p->n_terms, delta->n_terms);
  if (workspace_bytes < need) {
    rf_set_error("rf_sparse_append: workspace %zu B < required %zu B", workspace_bytes, need);
    return RF_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  LexAppend P;
  P.A = lex_side(old_p);
  P.D = lex_side(delta);
  P.O = lex_out(merged);
  P.map_old = map_old_dev;
  P.map_delta = map_delta_dev;
  P.post_off = merged->post_off;
  P.n_terms = merged->n_terms;
  P.base_old = (int64_t*)workspace_dev;
  P.shift_old = P.base_old + P.A.n_terms;
  P.base_delta = P.shift_old + P.A.n_terms;
  P.shift_delta = P.base_delta + P.D.n_terms;
  const int64_t terms = P.A.n_terms + P.D.n_terms;
  hipLaunchKernelGGL(k_lex_append_tables, dim3((uint32_t)((terms + LEX_THREADS - 1) / LEX_THREADS)), dim3(LEX_THREADS), 0,
                     st, P);
  RF_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_lex_append_move, dim3((uint32_t)lex_chunks(P.A.nnz)), dim3(LEX_THREADS), 0, st, P.A, P.O,
                     (const int64_t*)P.base_old, (const int64_t*)P.shift_old, 0u);
  RF_HIP(hipGetLastError());
  if (P.D.nnz > 0 && P.D.n_terms > 0) {
    hipLaunchKernelGGL(k_lex_append_move, dim3((uint32_t)lex_chunks(P.D.nnz)), dim3(LEX_THREADS), 0, st, P.D, P.O,
                       (const int64_t*)P.base_delta, (const int64_t*)P.shift_delta, (uint32_t)old_p->n_rows);
    RF_HIP(hipGetLastError());
  }
  return RF_OK;
}

extern "C" size_t rf_sparse_compact_workspace_bytes(int64_t nnz) {
  if (nnz < 1 || lex_chunks(nnz) >= ((int64_t)1 << 31)) return 0;
  return (size_t)lex_chunks(nnz) * 2 * sizeof(int64_t);
}

extern "C" int rf_sparse_compact_plan(const rf_postings* old_p, const int32_t* row_map_dev, int64_t* dst_post_dev,
                                      int64_t* dst_pos_dev, int64_t* term_dst_dev, void* workspace_dev,
                                      size_t workspace_bytes, void* stream) {
  if (!lex_side_ok("rf_sparse_compact_plan", "old", old_p, true, 1)) return RF_ERR_INVALID;
  if (!row_map_dev || !dst_post_dev || !term_dst_dev || !workspace_dev || old_p->n_rows < 1 || old_p->n_terms < 1) {
    rf_set_error("rf_sparse_compact_plan: null argument, or no row or no term");
    return RF_ERR_INVALID;
  }
  if ((dst_pos_dev != nullptr) != (old_p->pos_off != nullptr)) {
    rf_set_error("rf_sparse_compact_plan: dst_pos_dev goes with the positions of the postings: both or neither");
    return RF_ERR_INVALID;
  }
  if (misaligned(row_map_dev) || misaligned(dst_post_dev) || misaligned(dst_pos_dev) || misaligned(term_dst_dev) ||
      misaligned(workspace_dev)) {
    rf_set_error("rf_sparse_compact_plan: every array must be 16-byte aligned");
    return RF_ERR_INVALID;
  }
  const size_t need = rf_sparse_compact_workspace_bytes(old_p->nnz);
  if (workspace_bytes < need) {
    rf_set_error("rf_sparse_compact_plan: workspace %zu B < required %zu B", workspace_bytes, need);
    return RF_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  LexPlan P;
  P.S = lex_side(old_p);
  P.row_map = row_map_dev;
  P.dst_post = dst_post_dev;
  P.dst_pos = dst_pos_dev;
  P.term_dst = term_dst_dev;
  P.chunks = lex_chunks(P.S.nnz);
  P.part_post = (int64_t*)workspace_dev;
  P.part_pos = P.part_post + P.chunks;
  hipLaunchKernelGGL(k_lex_plan_reduce, dim3((uint32_t)P.chunks), dim3(LEX_THREADS), 0, st, P);
  RF_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_lex_plan_scan_parts, dim3(1), dim3(LEX_THREADS), 0, st, P);
  RF_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_lex_plan_scan_chunks, dim3((uint32_t)P.chunks), dim3(LEX_THREADS), 0, st, P);
  RF_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_lex_plan_terms, dim3((uint32_t)((P.S.n_terms + 2 + LEX_THREADS - 1) / LEX_THREADS)),
                     dim3(LEX_THREADS), 0, st, P);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

extern "C" int rf_sparse_compact_apply(const rf_postings* old_p, const int32_t* row_map_dev, const int64_t* dst_post_dev,
                                       const int64_t* dst_pos_dev, const rf_postings* out, void* stream) {
  const char* fn = "rf_sparse_compact_apply";
  if (!lex_side_ok(fn, "old", old_p, false, 1) || !lex_side_ok(fn, "out", out, false, 1)) return RF_ERR_INVALID;
  if (!row_map_dev || !dst_post_dev || old_p->n_rows < 1) {
    rf_set_error("rf_sparse_compact_apply: null argument, or no row");
    return RF_ERR_INVALID;
  }
  const bool pos = out->pos_off != nullptr;
  if ((dst_pos_dev != nullptr) != pos || (old_p->pos_off != nullptr) != pos || out->nnz > old_p->nnz ||
      out->n_rows > old_p->n_rows) {
    rf_set_error("rf_sparse_compact_apply: positions on both sides and dst_pos_dev, or on neither; the output holds at "
                 "most the rows and postings of the input");
    return RF_ERR_INVALID;
  }
  if (misaligned(row_map_dev) || misaligned(dst_post_dev) || misaligned(dst_pos_dev)) {
    rf_set_error("rf_sparse_compact_apply: every array must be 16-byte aligned");
    return RF_ERR_INVALID;
  }
  LexApply P;
  P.S = lex_side(old_p);
  P.O = lex_out(out);
  P.row_map = row_map_dev;
  P.dst_post = dst_post_dev;
  P.dst_pos = dst_pos_dev;
  hipLaunchKernelGGL(k_lex_compact_apply, dim3((uint32_t)lex_chunks(P.S.nnz)), dim3(LEX_THREADS), 0, (hipStream_t)stream,
                     P);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
