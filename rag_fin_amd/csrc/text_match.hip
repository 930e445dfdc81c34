// Keyword filters: the posting lists of the lexical index turned into one row bitmap per
// TEXT_MATCH / PHRASE_MATCH leaf of a filter expression (include/ragfin.h, "keyword filters";
// DESIGN 4.4h).  rf_filter_eval_bitmaps (filter.hip) reads the bitmaps through RF_FOP_BITMAP leaves.
//
//   k_text_terms  one wave per leaf: every term's posting range, clamped, and whether the term
//                 repeats an earlier one of the leaf (a phrase may) -> the workspace
//   k_text_match  grid (row tiles, leaves): per tile row one counter in LDS = the leaf's distinct
//                 terms that hold the row, added term after term with a barrier in between (rows
//                 within a term are distinct: plain read-modify-writes).  MATCH: count >= min_match.
//                 PHRASE: the rows that hold every term are compacted and one lane per row checks
//                 adjacency in the position lists.  Each wave ballots 64 rows into two words.
// Integers only, and no result depends on the order in which lanes, waves or workgroups run (the
// compaction's order does, the bits it leads to do not): the same bitmap on every run.
// Mirrored in numpy by rag_fin_amd/lexical.py (text_match_reference).
#include "rf_internal.h"

#define TEXT_THREADS 256
#define TEXT_WAVES (TEXT_THREADS / 64)
#define TEXT_TILE_WORDS (RF_SPARSE_TILE_ROWS / 32)

static_assert(RF_SPARSE_MAX_TERMS == 64, "k_text_terms gives a leaf one wave: one lane per term");
static_assert(RF_SPARSE_MAX_TERMS <= TEXT_THREADS, "one lane per term in the slice search");
static_assert(RF_SPARSE_TILE_ROWS % 64 == 0 && RF_SPARSE_TILE_ROWS <= 65536, "64-row ballots; candidates as uint16");

// a leaf's term in the workspace: its postings are [lo, hi) (empty for an id outside the dictionary)
struct TextTerm {
  int64_t lo, hi;
  int32_t repeat;   // 1: the same id stands earlier in the leaf
  int32_t pad[3];
};
static_assert(sizeof(TextTerm) == 32, "workspace layout");

struct TextArgs {
  rf_text_leaf leaves[RF_TEXT_MAX_LEAVES];
  const int64_t* post_off;
  const uint32_t* post_row;
  const int64_t* pos_off;
  const uint32_t* pos;
  const int32_t* terms;
  TextTerm* table;       // [n_leaves][RF_SPARSE_MAX_TERMS]
  uint32_t* bitmaps;
  int64_t n_terms, nnz, n_pos, words_per_leaf;
  uint32_t n_rows, n_tiles;
};

// first p in [lo, hi) with a[p] >= x (a ascending), hi if none
__device__ __forceinline__ int64_t text_lower_bound(const uint32_t* __restrict__ a, int64_t lo, int64_t hi, uint32_t x) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t text_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Grid (leaves), one wave: lane i owns term i of the leaf.
__global__ void __launch_bounds__(64) k_text_terms(TextArgs P) {
  __shared__ int32_t s_term[RF_SPARSE_MAX_TERMS];
  const rf_text_leaf& L = P.leaves[blockIdx.x];
  const int i = threadIdx.x;
  const int m = L.n_terms;   // (1..RF_SPARSE_MAX_TERMS, inside terms_dev: checked on the host)
  int32_t t = -1;
  if (i < m) t = P.terms[L.term_off + i];
  s_term[i] = t;
  __syncthreads();
  if (i < m) {
    TextTerm e;
    e.lo = e.hi = 0;
    if (t >= 0 && (int64_t)t < P.n_terms) {
      e.lo = text_clamp(P.post_off[t], 0, P.nnz);
      e.hi = text_clamp(P.post_off[t + 1], e.lo, P.nnz);
    }
    e.repeat = 0;
    for (int j = 0; j < i; ++j) e.repeat |= s_term[j] == t ? 1 : 0;
    e.pad[0] = e.pad[1] = e.pad[2] = 0;
    P.table[(size_t)blockIdx.x * RF_SPARSE_MAX_TERMS + i] = e;
  }
}

// Does `row` hold the phrase?  Term i's postings inside the tile are [s_beg[i], s_end[i]).  The start
// positions (those of term 0) are taken 64 at a time as a bit set; term after term strikes the starts
// whose position + i it does not hold.
__device__ bool text_phrase_row(const TextArgs& P, int m, const int64_t* s_beg, const int64_t* s_end, uint32_t row) {
  const int64_t q0 = text_lower_bound(P.post_row, s_beg[0], s_end[0], row);
  if (q0 >= s_end[0] || P.post_row[q0] != row) return false;
  const int64_t a0 = text_clamp(P.pos_off[q0], 0, P.n_pos);
  const int64_t a1 = text_clamp(P.pos_off[q0 + 1], a0, P.n_pos);
  for (int64_t base = a0; base < a1; base += 64) {
    const int n = (int)(a1 - base < 64 ? a1 - base : 64);
    unsigned long long alive = n == 64 ? ~0ull : ((1ull << n) - 1ull);
    for (int i = 1; i < m && alive; ++i) {
      const int64_t q = text_lower_bound(P.post_row, s_beg[i], s_end[i], row);
      if (q >= s_end[i] || P.post_row[q] != row) return false;   // the row does not hold term i at all
      const int64_t b0 = text_clamp(P.pos_off[q], 0, P.n_pos);
      const int64_t b1 = text_clamp(P.pos_off[q + 1], b0, P.n_pos);
      for (int j = 0; j < n; ++j) {
        if (!((alive >> j) & 1ull)) continue;
        const uint32_t want = P.pos[base + j] + (uint32_t)i;
        const int64_t at = text_lower_bound(P.pos, b0, b1, want);
        if (at >= b1 || P.pos[at] != want) alive &= ~(1ull << j);
      }
    }
    if (alive) return true;
  }
  return false;
}

// Grid (tiles, leaves).  The workgroup owns rows [tile * TILE, (tile + 1) * TILE) and the TILE / 32
// words of the leaf's bitmap that hold them.  Every barrier is reached by every thread.
__global__ void __launch_bounds__(TEXT_THREADS) k_text_match(TextArgs P) {
  __shared__ uint32_t s_cnt[RF_SPARSE_TILE_ROWS];
  __shared__ uint16_t s_cand[RF_SPARSE_TILE_ROWS];
  __shared__ int64_t s_beg[RF_SPARSE_MAX_TERMS], s_end[RF_SPARSE_MAX_TERMS];
  __shared__ int32_t s_repeat[RF_SPARSE_MAX_TERMS];
  __shared__ uint32_t s_ncand;

  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t tile = blockIdx.x;
  const rf_text_leaf& L = P.leaves[blockIdx.y];
  const int m = L.n_terms;
  const bool phrase = L.kind == RF_TEXT_PHRASE;
  const uint32_t row0 = tile * (uint32_t)RF_SPARSE_TILE_ROWS;
  const uint32_t left = P.n_rows - row0;   // (tile < n_tiles: row0 < n_rows)
  const uint32_t rows_here = left < (uint32_t)RF_SPARSE_TILE_ROWS ? left : (uint32_t)RF_SPARSE_TILE_ROWS;

  for (uint32_t i = tid; i < (uint32_t)RF_SPARSE_TILE_ROWS; i += TEXT_THREADS) s_cnt[i] = 0u;
  if (tid == 0) s_ncand = 0u;
  // lane i: the slice of term i's postings that falls into this tile
  if (tid < (uint32_t)m) {
    const TextTerm e = P.table[(size_t)blockIdx.y * RF_SPARSE_MAX_TERMS + tid];
    const int64_t beg = text_lower_bound(P.post_row, e.lo, e.hi, row0);
    s_beg[tid] = beg;
    s_end[tid] = text_lower_bound(P.post_row, beg, e.hi, row0 + rows_here);   // (row0 + rows_here <= n_rows < 2^31)
    s_repeat[tid] = e.repeat;
  }
  __syncthreads();

  // count the distinct terms that hold each row: term after term, a barrier in between
  uint32_t distinct = 0u;
  for (int i = 0; i < m; ++i) {
    if (!s_repeat[i]) {   // (uniform over the workgroup)
      ++distinct;
      const int64_t end = s_end[i];
      for (int64_t p = s_beg[i] + tid; p < end; p += TEXT_THREADS) {
        const uint32_t local = P.post_row[p] - row0;
        if (local < rows_here) s_cnt[local] += 1u;   // (unsigned: a row below row0 wraps past rows_here)
      }
    }
    __syncthreads();
  }

  // PHRASE: the rows that hold every term become candidates; their counter becomes the verdict
  if (phrase) {
    for (uint32_t c = wave; c < (uint32_t)(RF_SPARSE_TILE_ROWS / 64); c += TEXT_WAVES) {
      const uint32_t local = c * 64u + lane;
      const bool cand = local < rows_here && s_cnt[local] == distinct;
      s_cnt[local] = 0u;
      const unsigned long long b = __ballot(cand);
      if (b == 0ull) continue;   // (wave-uniform)
      uint32_t base = 0u;
      if (lane == 0) base = atomicAdd(&s_ncand, (uint32_t)__popcll(b));
      base = __shfl(base, 0);
      if (cand) s_cand[base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = (uint16_t)local;
    }
  }
  __syncthreads();
  if (phrase) {
    const uint32_t n = s_ncand;   // (<= rows_here)
    for (uint32_t c = tid; c < n; c += TEXT_THREADS) {
      const uint32_t local = s_cand[c];
      if (text_phrase_row(P, m, s_beg, s_end, row0 + local)) s_cnt[local] = 1u;
    }
  }
  __syncthreads();

  // 64 rows per wave and step -> two words; the words past the rows (up to words_per_leaf) are zero
  const uint32_t need = phrase ? 1u : (uint32_t)L.min_match;
  uint32_t* out = P.bitmaps + (size_t)blockIdx.y * (size_t)P.words_per_leaf;
  const int64_t w0 = (int64_t)tile * TEXT_TILE_WORDS;
  for (uint32_t c = wave; c < (uint32_t)(RF_SPARSE_TILE_ROWS / 64); c += TEXT_WAVES) {
    const uint32_t local = c * 64u + lane;
    const bool pass = local < rows_here && s_cnt[local] >= need;
    const unsigned long long b = __ballot(pass);
    const int64_t w = w0 + 2 * (int64_t)c + (int64_t)lane;
    if (lane < 2u && w < P.words_per_leaf) out[w] = lane == 0 ? (uint32_t)b : (uint32_t)(b >> 32);
  }
  if (tile + 1u == P.n_tiles) {
    for (int64_t w = (int64_t)P.n_tiles * TEXT_TILE_WORDS + tid; w < P.words_per_leaf; w += TEXT_THREADS) out[w] = 0u;
  }
}

// ---- entry points ------------------------------------------------------------------------------------
static bool misaligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) != 0; }

extern "C" int rf_sparse_attach_positions(rf_sparse_t* sp, const int64_t* pos_off_dev, const uint32_t* pos_dev,
                                          int64_t n_pos) {
  if (!sp || !pos_off_dev || !pos_dev) {
    rf_set_error("rf_sparse_attach_positions: null argument");
    return RF_ERR_INVALID;
  }
  if (misaligned(pos_off_dev, 16) || misaligned(pos_dev, 16)) {
    rf_set_error("rf_sparse_attach_positions: the position arrays must be 16-byte aligned");
    return RF_ERR_INVALID;
  }
  if (n_pos < sp->nnz) {   // every posting holds at least one position
    rf_set_error("rf_sparse_attach_positions: n_pos = %lld < nnz = %lld", (long long)n_pos, (long long)sp->nnz);
    return RF_ERR_INVALID;
  }
  sp->pos_off = pos_off_dev;
  sp->pos = pos_dev;
  sp->n_pos = n_pos;
  return RF_OK;
}

extern "C" size_t rf_text_match_workspace_bytes(const rf_sparse_t* sp, int n_leaves) {
  if (!sp || n_leaves < 1 || n_leaves > RF_TEXT_MAX_LEAVES) return 0;
  return (size_t)n_leaves * RF_SPARSE_MAX_TERMS * sizeof(TextTerm);
}

extern "C" int rf_text_match(const rf_sparse_t* sp, const rf_text_leaf* leaves_host, int n_leaves,
                             const int32_t* terms_dev, int64_t n_terms_total, uint32_t* bitmaps_dev,
                             int64_t words_per_leaf, void* workspace_dev, size_t workspace_bytes, void* stream) {
  static const char* fn = "rf_text_match";
  if (!sp || !leaves_host || !terms_dev || !bitmaps_dev || !workspace_dev) {
    rf_set_error("%s: null argument", fn);
    return RF_ERR_INVALID;
  }
  if (n_leaves < 1 || n_leaves > RF_TEXT_MAX_LEAVES) {
    rf_set_error("%s: n_leaves = %d outside 1..%d", fn, n_leaves, RF_TEXT_MAX_LEAVES);
    return RF_ERR_INVALID;
  }
  if (misaligned(bitmaps_dev, 16) || misaligned(workspace_dev, 16) || misaligned(terms_dev, 4)) {
    rf_set_error("%s: bitmaps and workspace must be 16-byte aligned, terms 4-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  const int64_t words = (sp->n_rows + 31) / 32;
  if (words_per_leaf < words || words_per_leaf > (int64_t)0x7FFFFFFF / RF_TEXT_MAX_LEAVES) {
    rf_set_error("%s: words_per_leaf = %lld, need >= %lld (and leaf offsets that fit int32)", fn,
                 (long long)words_per_leaf, (long long)words);
    return RF_ERR_INVALID;
  }
  TextArgs P{};
  for (int l = 0; l < n_leaves; ++l) {
    const rf_text_leaf& L = leaves_host[l];
    if (L.kind != RF_TEXT_MATCH && L.kind != RF_TEXT_PHRASE) {
      rf_set_error("%s: leaf %d: unknown kind %d", fn, l, L.kind);
      return RF_ERR_INVALID;
    }
    if (L.n_terms < 1 || L.n_terms > RF_SPARSE_MAX_TERMS || L.term_off < 0 ||
        (int64_t)L.term_off + L.n_terms > n_terms_total) {
      rf_set_error("%s: leaf %d: terms [%d, %d + %d) must be 1..%d entries inside the %lld given", fn, l, L.term_off,
                   L.term_off, L.n_terms, RF_SPARSE_MAX_TERMS, (long long)n_terms_total);
      return RF_ERR_INVALID;
    }
    if (L.min_match < 1) {
      rf_set_error("%s: leaf %d: min_match = %d < 1", fn, l, L.min_match);
      return RF_ERR_INVALID;
    }
    if (L.kind == RF_TEXT_PHRASE && (!sp->pos_off || !sp->pos)) {
      rf_set_error("%s: leaf %d is a phrase, the handle has no positions (rf_sparse_attach_positions)", fn, l);
      return RF_ERR_INVALID;
    }
    P.leaves[l] = L;
  }
  const size_t need = rf_text_match_workspace_bytes(sp, n_leaves);
  if (workspace_bytes < need) {
    rf_set_error("%s: workspace %zu B < required %zu B", fn, workspace_bytes, need);
    return RF_ERR_INVALID;
  }
  P.post_off = sp->post_off;
  P.post_row = sp->post_row;
  P.pos_off = sp->pos_off;
  P.pos = sp->pos;
  P.terms = terms_dev;
  P.table = (TextTerm*)workspace_dev;
  P.bitmaps = bitmaps_dev;
  P.n_terms = sp->n_terms;
  P.nnz = sp->nnz;
  P.n_pos = sp->n_pos;
  P.words_per_leaf = words_per_leaf;
  P.n_rows = (uint32_t)sp->n_rows;
  P.n_tiles = (uint32_t)((sp->n_rows + RF_SPARSE_TILE_ROWS - 1) / RF_SPARSE_TILE_ROWS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_text_terms, dim3((uint32_t)n_leaves), dim3(64), 0, st, P);
  RF_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_text_match, dim3(P.n_tiles, (uint32_t)n_leaves), dim3(TEXT_THREADS), 0, st, P);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
