// Row filter of filtered search: the compiled predicate of Collection.search(..., expr=...)
// evaluated on the device into a row mask, and the mask compacted into the ascending list of
// 32-row blocks that hold a passing row (include/ragfin.h, "filtered search").
//
//   k_filter_eval     one thread per row runs the postfix program on a bool stack held in the
//                     bits of one register; a wave64 ballot gives two mask words; each workgroup
//                     counts its tile's non-empty blocks and passing rows
//   k_filter_copy     (rf_filter_from_mask) the caller's mask instead of a program, same counts
//   k_filter_compact  each tile adds up the counts of the tiles before it (a scan), then writes
//                     the indices of its non-empty blocks in ascending order; the last tile
//                     writes the header
// No output depends on the order in which atomics or workgroups run: the same mask gives the
// same buffer, bit for bit.
#include "rf_internal.h"

// ---- buffer layout ---------------------------------------------------------------------------
static inline size_t align16(size_t x) { return (x + 15) / 16 * 16; }

static inline int64_t filter_blocks(int64_t n_rows) { return (n_rows + 31) / 32; }

static inline bool filter_rows_ok(int64_t n_rows) {
  return n_rows >= 0 && n_rows <= (int64_t)0xFFFFFFFFll - 32;   // row and block numbers fit uint32
}

size_t rf_filter_layout(int64_t n_rows, size_t* mask_off, size_t* blocks_off, size_t* tiles_off) {
  const size_t words = align16((size_t)filter_blocks(n_rows) * 4);
  const size_t m = RF_FILTER_HDR_WORDS * 4;
  if (mask_off) *mask_off = m;
  if (blocks_off) *blocks_off = m + words;
  if (tiles_off) *tiles_off = m + 2 * words;
  return m + 2 * words + (size_t)2 * RF_FILTER_MAX_TILES * 4;
}

rf_filter_view rf_filter_carve(const void* filter, int64_t n_rows) {
  size_t mo, bo;
  rf_filter_layout(n_rows, &mo, &bo, nullptr);
  const unsigned char* base = (const unsigned char*)filter;
  rf_filter_view v;
  v.hdr = (const uint32_t*)base;
  v.mask = (const uint32_t*)(base + mo);
  v.blocks = (const uint32_t*)(base + bo);
  return v;
}

extern "C" size_t rf_filter_bytes(int64_t n_rows) {
  if (!filter_rows_ok(n_rows)) return 0;
  return rf_filter_layout(n_rows, nullptr, nullptr, nullptr);
}

// Compaction tiles: at most RF_FILTER_MAX_TILES, each a multiple of 32 mask words (one
// k_filter_eval iteration of a 16-wave workgroup), so that the scan over the tile counts stays short.
struct TilePlan {
  uint32_t nblk, tile_words, n_tiles;
};
static TilePlan plan_tiles(int64_t n_rows) {
  TilePlan t;
  t.nblk = (uint32_t)filter_blocks(n_rows);
  const uint32_t per = 32u * RF_FILTER_MAX_TILES;
  t.tile_words = 32u * ((t.nblk + per - 1) / per > 0 ? (t.nblk + per - 1) / per : 1u);
  t.n_tiles = (t.nblk + t.tile_words - 1) / t.tile_words;
  return t;
}

// ---- kernels -----------------------------------------------------------------------------------
#define FILTER_EVAL_THREADS 1024
#define FILTER_COMPACT_THREADS 256

struct FilterProg {
  rf_filter_op ops[RF_FILTER_MAX_OPS];
  const int32_t* codes[3];     // period, chunk_type, statement_type
  const double* value;         // primary_value
  const uint32_t* code_sets;
  const uint32_t* row_lists;
  const uint32_t* bitmaps;
  uint32_t* mask;
  uint32_t* tile_cnt;          // [n_tiles][2] {non-empty blocks, passing rows}
  uint32_t n_rows, nblk, tile_words, n_ops;
};

__device__ __forceinline__ bool eval_row(const FilterProg& P, uint32_t row) {
  uint32_t st = 0u;   // bool stack: bit 0 is the top
  for (uint32_t i = 0; i < P.n_ops; ++i) {
    const rf_filter_op& o = P.ops[i];   // wave-uniform: scalar loads from the kernel arguments
    const int op = o.op;
    if (op == RF_FOP_AND || op == RF_FOP_OR) {
      const uint32_t a = st & 1u;
      st >>= 1;
      const uint32_t b = st & 1u;
      st = (st & ~1u) | (op == RF_FOP_AND ? (a & b) : (a | b));
      continue;
    }
    if (op == RF_FOP_NOT) {
      st ^= 1u;
      continue;
    }
    bool v = false;
    if (op == RF_FOP_CODESET) {
      const uint32_t c = (uint32_t)P.codes[o.column][row];
      v = c < 32u * (uint32_t)o.len && ((P.code_sets[o.off + (c >> 5)] >> (c & 31u)) & 1u) != 0u;
    } else if (op == RF_FOP_RANGE) {
      const double x = P.value[row];
      const bool a = (o.flags & RF_FRANGE_LO_INCL) ? x >= o.lo : x > o.lo;
      const bool b = (o.flags & RF_FRANGE_HI_INCL) ? x <= o.hi : x < o.hi;
      v = a && b;   // NaN fails both
    } else if (op == RF_FOP_ROWLIST) {
      // lower bound of `row` in the sorted list
      const uint32_t* L = P.row_lists + o.off;
      uint32_t lo = 0u, n = (uint32_t)o.len;
      while (n > 0u) {
        const uint32_t half = n >> 1;
        if (L[lo + half] < row) {
          lo += half + 1u;
          n -= half + 1u;
        } else {
          n = half;
        }
      }
      v = lo < (uint32_t)o.len && L[lo] == row;
    } else if (op == RF_FOP_BITMAP) {
      const uint32_t w = row >> 5;
      v = w < (uint32_t)o.len && ((P.bitmaps[(uint32_t)o.off + w] >> (row & 31u)) & 1u) != 0u;
    } else {
      v = op == RF_FOP_TRUE;
    }
    st = (st << 1) | (v ? 1u : 0u);
  }
  return (st & 1u) != 0u;
}

__device__ __forceinline__ uint32_t wave_sum_u(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// one workgroup per tile; a wave evaluates 64 rows (two mask words) per iteration
__global__ void __launch_bounds__(FILTER_EVAL_THREADS) k_filter_eval(FilterProg P) {
  __shared__ uint32_t red[2][FILTER_EVAL_THREADS / 64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const uint32_t w0 = blockIdx.x * P.tile_words;
  const uint32_t w1 = min(w0 + P.tile_words, P.nblk);
  uint32_t nz = 0u, pc = 0u;   // wave-uniform
  for (uint32_t w = w0 + 2u * wave; w < w1; w += 2u * (FILTER_EVAL_THREADS / 64)) {
    const uint32_t row = w * 32u + (uint32_t)lane;
    const bool pass = row < P.n_rows && eval_row(P, row);
    const unsigned long long m = __ballot(pass);   // bits past n_rows are zero
    const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
    if (lane == 0) P.mask[w] = lo;
    if (lane == 1 && w + 1u < w1) P.mask[w + 1u] = hi;
    nz += (lo != 0u) + (hi != 0u);
    pc += (uint32_t)__popcll(m);
  }
  if (lane == 0) {
    red[0][wave] = nz;
    red[1][wave] = pc;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    uint32_t s = 0u;
    for (int i = 0; i < FILTER_EVAL_THREADS / 64; ++i) s += red[threadIdx.x][i];
    P.tile_cnt[2 * blockIdx.x + threadIdx.x] = s;
  }
}

// rf_filter_from_mask: copy the caller's words (bits past n_rows cleared) and count them
__global__ void __launch_bounds__(FILTER_EVAL_THREADS) k_filter_copy(const uint32_t* __restrict__ src,
                                                                    uint32_t* __restrict__ mask,
                                                                    uint32_t* __restrict__ tile_cnt,
                                                                    uint32_t n_rows, uint32_t nblk,
                                                                    uint32_t tile_words) {
  __shared__ uint32_t red[2][FILTER_EVAL_THREADS / 64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const uint32_t w0 = blockIdx.x * tile_words;
  const uint32_t w1 = min(w0 + tile_words, nblk);
  uint32_t nz = 0u, pc = 0u;
  for (uint32_t w = w0 + threadIdx.x; w < w1; w += FILTER_EVAL_THREADS) {
    uint32_t v = src[w];
    const uint32_t rows = n_rows - w * 32u;   // > 0
    if (rows < 32u) v &= (1u << rows) - 1u;
    mask[w] = v;
    nz += v != 0u;
    pc += (uint32_t)__popc(v);
  }
  nz = wave_sum_u(nz);
  pc = wave_sum_u(pc);
  if (lane == 0) {
    red[0][wave] = nz;
    red[1][wave] = pc;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    uint32_t s = 0u;
    for (int i = 0; i < FILTER_EVAL_THREADS / 64; ++i) s += red[threadIdx.x][i];
    tile_cnt[2 * blockIdx.x + threadIdx.x] = s;
  }
}

// one workgroup per tile (at least one: the last writes the header)
__global__ void __launch_bounds__(FILTER_COMPACT_THREADS) k_filter_compact(
    const uint32_t* __restrict__ mask, const uint32_t* __restrict__ tile_cnt, uint32_t* __restrict__ blocks,
    uint32_t* __restrict__ hdr, uint32_t n_rows, uint32_t nblk, uint32_t tile_words, uint32_t n_tiles) {
  constexpr int NW = FILTER_COMPACT_THREADS / 64;
  __shared__ uint32_t red[2][NW];
  __shared__ uint32_t wcnt[NW];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const uint32_t t = blockIdx.x;
  // exclusive prefix of the counts of the tiles before this one (fixed summation order)
  uint32_t pb = 0u, pr = 0u;
  for (uint32_t i = tid; i < t && i < n_tiles; i += FILTER_COMPACT_THREADS) {
    pb += tile_cnt[2 * i];
    pr += tile_cnt[2 * i + 1];
  }
  pb = wave_sum_u(pb);
  pr = wave_sum_u(pr);
  if (lane == 0) {
    red[0][wave] = pb;
    red[1][wave] = pr;
  }
  __syncthreads();
  uint32_t base_b = 0u, base_r = 0u;
  for (int i = 0; i < NW; ++i) {
    base_b += red[0][i];
    base_r += red[1][i];
  }
  if (t + 1u == gridDim.x && tid == 0) {
    const uint32_t own_b = t < n_tiles ? tile_cnt[2 * t] : 0u;
    const uint32_t own_r = t < n_tiles ? tile_cnt[2 * t + 1] : 0u;
    hdr[0] = n_rows;
    hdr[1] = base_r + own_r;
    hdr[2] = base_b + own_b;
    hdr[3] = n_tiles;
  }
  if (t >= n_tiles) return;
  const uint32_t w0 = t * tile_words;
  const uint32_t w1 = min(w0 + tile_words, nblk);
  uint32_t out = base_b;
  for (uint32_t j0 = w0; j0 < w1; j0 += FILTER_COMPACT_THREADS) {
    const uint32_t j = j0 + (uint32_t)tid;
    const bool nz = j < w1 && mask[j] != 0u;
    const unsigned long long b = __ballot(nz);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0u, all = 0u;
    for (int i = 0; i < NW; ++i) {
      before += i < wave ? wcnt[i] : 0u;
      all += wcnt[i];
    }
    if (nz) blocks[out + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = j;
    out += all;
    __syncthreads();   // wcnt is rewritten by the next chunk
  }
}

// ---- host side ---------------------------------------------------------------------------------
static int launch_compact(void* filter_dev, int64_t n_rows, const TilePlan& tp, hipStream_t st) {
  size_t mo, bo, to;
  rf_filter_layout(n_rows, &mo, &bo, &to);
  unsigned char* base = (unsigned char*)filter_dev;
  const uint32_t grid = tp.n_tiles > 0 ? tp.n_tiles : 1u;
  hipLaunchKernelGGL(k_filter_compact, dim3(grid), dim3(FILTER_COMPACT_THREADS), 0, st,
                     (const uint32_t*)(base + mo), (const uint32_t*)(base + to), (uint32_t*)(base + bo),
                     (uint32_t*)base, (uint32_t)n_rows, tp.nblk, tp.tile_words, tp.n_tiles);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

static int check_filter_buffer(const char* fn, int64_t n_rows, const void* filter_dev) {
  if (!filter_dev) {
    rf_set_error("%s: null filter buffer", fn);
    return RF_ERR_INVALID;
  }
  if (((uintptr_t)filter_dev) & 15) {
    rf_set_error("%s: filter buffer must be 16-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  if (!filter_rows_ok(n_rows)) {
    rf_set_error("%s: n_rows = %lld out of range", fn, (long long)n_rows);
    return RF_ERR_INVALID;
  }
  return RF_OK;
}

static int filter_eval(const char* fn, const rf_filter_op* ops, int n_ops, const uint32_t* code_sets_dev,
                       const uint32_t* row_lists_dev, const uint32_t* bitmaps_dev, const void* const* columns,
                       int64_t n_rows, void* filter_dev, void* stream) {
  if (!ops || !columns) {
    rf_set_error("%s: null program or column table", fn);
    return RF_ERR_INVALID;
  }
  if (n_ops < 1 || n_ops > RF_FILTER_MAX_OPS) {
    rf_set_error("%s: n_ops = %d outside 1..%d", fn, n_ops, RF_FILTER_MAX_OPS);
    return RF_ERR_INVALID;
  }
  int rc = check_filter_buffer(fn, n_rows, filter_dev);
  if (rc != RF_OK) return rc;
  FilterProg P{};
  int depth = 0;
  for (int i = 0; i < n_ops; ++i) {
    const rf_filter_op& o = ops[i];
    switch (o.op) {
      case RF_FOP_CODESET:
        if (o.column < 0 || o.column > 2 || !columns[o.column] || o.off < 0 || o.len < 0 ||
            (o.len > 0 && !code_sets_dev)) {
          rf_set_error("%s: op %d: bad code-set leaf (column %d, off %d, len %d)", fn, i, o.column, o.off, o.len);
          return RF_ERR_INVALID;
        }
        ++depth;
        break;
      case RF_FOP_RANGE:
        if (o.column != 3 || !columns[3]) {
          rf_set_error("%s: op %d: a range leaf reads column 3 (fp64), which must be given", fn, i);
          return RF_ERR_INVALID;
        }
        ++depth;
        break;
      case RF_FOP_ROWLIST:
        if (o.off < 0 || o.len < 0 || (o.len > 0 && !row_lists_dev)) {
          rf_set_error("%s: op %d: bad row-list leaf (off %d, len %d)", fn, i, o.off, o.len);
          return RF_ERR_INVALID;
        }
        ++depth;
        break;
      case RF_FOP_BITMAP:
        if (o.off < 0 || o.len < 0 || !bitmaps_dev) {
          rf_set_error("%s: op %d: bad bitmap leaf (off %d, len %d%s)", fn, i, o.off, o.len,
                       bitmaps_dev ? "" : ", no bitmaps given");
          return RF_ERR_INVALID;
        }
        ++depth;
        break;
      case RF_FOP_TRUE:
      case RF_FOP_FALSE:
        ++depth;
        break;
      case RF_FOP_AND:
      case RF_FOP_OR:
        if (depth < 2) {
          rf_set_error("%s: op %d: AND / OR needs two operands, the stack holds %d", fn, i, depth);
          return RF_ERR_INVALID;
        }
        --depth;
        break;
      case RF_FOP_NOT:
        if (depth < 1) {
          rf_set_error("%s: op %d: NOT on an empty stack", fn, i);
          return RF_ERR_INVALID;
        }
        break;
      default:
        rf_set_error("%s: op %d: unknown opcode %d", fn, i, o.op);
        return RF_ERR_INVALID;
    }
    if (depth > RF_FILTER_MAX_DEPTH) {
      rf_set_error("%s: op %d: stack depth %d exceeds %d", fn, i, depth, RF_FILTER_MAX_DEPTH);
      return RF_ERR_INVALID;
    }
    P.ops[i] = o;
  }
  if (depth != 1) {
    rf_set_error("%s: the program leaves %d values on the stack (must be 1)", fn, depth);
    return RF_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const TilePlan tp = plan_tiles(n_rows);
  size_t mo, bo, to;
  rf_filter_layout(n_rows, &mo, &bo, &to);
  unsigned char* base = (unsigned char*)filter_dev;
  for (int c = 0; c < 3; ++c) P.codes[c] = (const int32_t*)columns[c];
  P.value = (const double*)columns[3];
  P.code_sets = code_sets_dev;
  P.row_lists = row_lists_dev;
  P.bitmaps = bitmaps_dev;
  P.mask = (uint32_t*)(base + mo);
  P.tile_cnt = (uint32_t*)(base + to);
  P.n_rows = (uint32_t)n_rows;
  P.nblk = tp.nblk;
  P.tile_words = tp.tile_words;
  P.n_ops = (uint32_t)n_ops;
  if (tp.n_tiles > 0) {
    hipLaunchKernelGGL(k_filter_eval, dim3(tp.n_tiles), dim3(FILTER_EVAL_THREADS), 0, st, P);
    RF_HIP(hipGetLastError());
  }
  return launch_compact(filter_dev, n_rows, tp, st);
}

extern "C" int rf_filter_eval(const rf_filter_op* ops, int n_ops, const uint32_t* code_sets_dev,
                              const uint32_t* row_lists_dev, const void* const* columns, int64_t n_rows,
                              void* filter_dev, void* stream) {
  return filter_eval("rf_filter_eval", ops, n_ops, code_sets_dev, row_lists_dev, nullptr, columns, n_rows, filter_dev,
                     stream);
}

extern "C" int rf_filter_eval_bitmaps(const rf_filter_op* ops, int n_ops, const uint32_t* code_sets_dev,
                                      const uint32_t* row_lists_dev, const uint32_t* bitmaps_dev,
                                      const void* const* columns, int64_t n_rows, void* filter_dev, void* stream) {
  return filter_eval("rf_filter_eval_bitmaps", ops, n_ops, code_sets_dev, row_lists_dev, bitmaps_dev, columns, n_rows,
                     filter_dev, stream);
}

extern "C" int rf_filter_from_mask(const uint32_t* mask_dev, int64_t n_rows, void* filter_dev, void* stream) {
  int rc = check_filter_buffer("rf_filter_from_mask", n_rows, filter_dev);
  if (rc != RF_OK) return rc;
  if (!mask_dev && n_rows > 0) {
    rf_set_error("rf_filter_from_mask: null mask");
    return RF_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const TilePlan tp = plan_tiles(n_rows);
  size_t mo, bo, to;
  rf_filter_layout(n_rows, &mo, &bo, &to);
  unsigned char* base = (unsigned char*)filter_dev;
  if (tp.n_tiles > 0) {
    hipLaunchKernelGGL(k_filter_copy, dim3(tp.n_tiles), dim3(FILTER_EVAL_THREADS), 0, st, mask_dev,
                       (uint32_t*)(base + mo), (uint32_t*)(base + to), (uint32_t)n_rows, tp.nblk, tp.tile_words);
    RF_HIP(hipGetLastError());
  }
  return launch_compact(filter_dev, n_rows, tp, st);
}

// ---- per-query filters (include/ragfin.h, "per-query filters") ----------------------------------
uint32_t rf_multi_columns(int n_filters) {
  uint32_t gp = 1u;
  while (gp < (uint32_t)n_filters) gp <<= 1;
  return gp;
}

size_t rf_multi_layout(int64_t n_rows, int n_filters, size_t* masks_off) {
  const size_t m = (rf_filter_layout(n_rows, nullptr, nullptr, nullptr) + 255) / 256 * 256;
  if (masks_off) *masks_off = m;
  return m + (size_t)filter_blocks(n_rows) * rf_multi_columns(n_filters) * 4;
}

static bool multi_count_ok(int n_filters) { return n_filters >= 1 && n_filters <= RF_MULTI_MAX_FILTERS; }

extern "C" size_t rf_multi_filter_bytes(int64_t n_rows, int n_filters) {
  if (!filter_rows_ok(n_rows) || !multi_count_ok(n_filters)) return 0;
  return rf_multi_layout(n_rows, n_filters, nullptr);
}

struct MultiSrc {
  const uint32_t* hdr[RF_MULTI_MAX_FILTERS];
  const uint32_t* mask[RF_MULTI_MAX_FILTERS];
};

// k_filter_copy with the OR of G masks as the source, which also writes the G words of every
// block side by side (block-major).  A filter whose header was built for another row count
// passes no row, as in the masked sweep (filter_pass_blocks).  One thread per mask word: no
// atomics, the same filters give the same buffer bit for bit.
__global__ void __launch_bounds__(FILTER_EVAL_THREADS) k_multi_union(MultiSrc src, uint32_t G, uint32_t gp,
                                                                    uint32_t* __restrict__ mask,
                                                                    uint32_t* __restrict__ masks_t,
                                                                    uint32_t* __restrict__ tile_cnt,
                                                                    uint32_t n_rows, uint32_t nblk,
                                                                    uint32_t tile_words) {
  __shared__ uint32_t red[2][FILTER_EVAL_THREADS / 64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const uint32_t w0 = blockIdx.x * tile_words;
  const uint32_t w1 = min(w0 + tile_words, nblk);
  uint32_t nz = 0u, pc = 0u;
  for (uint32_t w = w0 + threadIdx.x; w < w1; w += FILTER_EVAL_THREADS) {
    const uint32_t rows = n_rows - w * 32u;   // > 0
    const uint32_t keep = rows < 32u ? (1u << rows) - 1u : 0xFFFFFFFFu;
    uint32_t u = 0u;
    for (uint32_t g = 0; g < gp; ++g) {   // (g, G, gp: wave-uniform)
      uint32_t v = 0u;
      if (g < G && src.hdr[g][0] == n_rows) v = src.mask[g][w] & keep;
      masks_t[(size_t)w * gp + g] = v;
      u |= v;
    }
    mask[w] = u;
    nz += u != 0u;
    pc += (uint32_t)__popc(u);
  }
  nz = wave_sum_u(nz);
  pc = wave_sum_u(pc);
  if (lane == 0) {
    red[0][wave] = nz;
    red[1][wave] = pc;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    uint32_t s = 0u;
    for (int i = 0; i < FILTER_EVAL_THREADS / 64; ++i) s += red[threadIdx.x][i];
    tile_cnt[2 * blockIdx.x + threadIdx.x] = s;
  }
}

extern "C" int rf_multi_filter_build(const void* const* filters, int n_filters, int64_t n_rows, void* multi_dev,
                                     void* stream) {
  if (!filters || !multi_count_ok(n_filters)) {
    rf_set_error("rf_multi_filter_build: null filter array, or n_filters = %d outside 1..%d", n_filters,
                 RF_MULTI_MAX_FILTERS);
    return RF_ERR_INVALID;
  }
  int rc = check_filter_buffer("rf_multi_filter_build", n_rows, multi_dev);
  if (rc != RF_OK) return rc;
  MultiSrc src{};
  for (int g = 0; g < n_filters; ++g) {
    if (!filters[g] || (((uintptr_t)filters[g]) & 15)) {
      rf_set_error("rf_multi_filter_build: filter %d null or not 16-byte aligned", g);
      return RF_ERR_INVALID;
    }
    const rf_filter_view v = rf_filter_carve(filters[g], n_rows);
    src.hdr[g] = v.hdr;
    src.mask[g] = v.mask;
  }
  hipStream_t st = (hipStream_t)stream;
  const TilePlan tp = plan_tiles(n_rows);
  size_t mo, bo, to, so;
  rf_filter_layout(n_rows, &mo, &bo, &to);
  rf_multi_layout(n_rows, n_filters, &so);
  unsigned char* base = (unsigned char*)multi_dev;
  // every byte of the buffer is defined: what the kernels below do not write (the block list past
  // the count, unused scratch, alignment gaps) is zero, so equal filters give equal buffers
  RF_HIP(hipMemsetAsync(multi_dev, 0, rf_multi_layout(n_rows, n_filters, nullptr), st));
  if (tp.n_tiles > 0) {
    hipLaunchKernelGGL(k_multi_union, dim3(tp.n_tiles), dim3(FILTER_EVAL_THREADS), 0, st, src, (uint32_t)n_filters,
                       rf_multi_columns(n_filters), (uint32_t*)(base + mo), (uint32_t*)(base + so),
                       (uint32_t*)(base + to), (uint32_t)n_rows, tp.nblk, tp.tile_words);
    RF_HIP(hipGetLastError());
  }
  return launch_compact(multi_dev, n_rows, tp, st);
}
