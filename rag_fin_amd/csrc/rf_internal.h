// Internal declarations shared by the HIP translation units of libragfin_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <atomic>
#include <mutex>
#include <vector>
#include "../../include/ragfin.h"

// ---- tiled corpus layout ---------------------------------------------------
// The corpus is stored as 32-row blocks.  Block b holds KS = dim/16 "fragments"
// of 1 KiB; fragment kk is exactly the A operand of one
// v_mfma_f32_32x32x16_f16: lane l (r = l & 31, h = l >> 5) owns the 16 bytes
// row[32 b + r][16 kk + 8 h .. +8).  One wave-wide 16-byte load therefore reads
// 1 KiB of contiguous HBM straight into MFMA operand registers.
#define RF_BLOCK_ROWS 32
#define RF_FRAG_BYTES 1024

__host__ __device__ inline size_t rf_chunk_index(int64_t row, int chunk, int KS) {
  // index (in uint4 units) of 16-byte chunk `chunk` (dims 8*chunk..+8) of `row`
  const int64_t b = row >> 5;
  const int r = (int)(row & 31);
  return ((size_t)b * KS + (chunk >> 1)) * 64 + (size_t)((chunk & 1) * 32 + r);
}

struct rf_index {
  int dim;
  int KS;              // dim / 16
  int device;
  int64_t capacity;    // rows
  int64_t size;        // rows (host-side counter; adds are stream-ordered)
  uint4* tiles;        // device: capacity_blocks * KS * 64 uint4
  uint32_t* max_norm2; // device: bits of max squared row norm (float >= 0)
  size_t storage_bytes;
  int num_cus;         // compute units of `device`
  // SQ8 shadow (sq8.hip): a caller-owned int8 copy of the rows, nullptr while none is attached
  uint4* sq8_tiles;    // device: capacity_blocks * KS8 * 64 uint4 (KS8 = dim / 32)
  float* sq8_scale;    // device: [capacity_blocks][32] s_r, in accumulator order (rf_sq8_slot)
  float* sq8_err;      // device: [capacity_blocks][32] e_r, same order
  uint32_t* sq8_max;   // device: {bits of N' = max ||s_r c^_r||, bits of E = max e_r}
  // rf_index_set_shadow_first: rf_search sweeps the shadow first from this many rows on (0: never)
  int64_t shadow_min_rows;
};
// An index is immutable during searches (no mutable host state: any number of threads may
// search one index concurrently, each with its own workspace and stream); rf_index_add_f16 /
// rf_index_reset / rf_index_compact must not run concurrently with a search (include/ragfin.h,
// "Threading").

// ---- tuning knobs ------------------------------------------------------------------------
// The shipped library has NO run-time tuning surface: every knob below is a compile-time
// constant.  Built with -DRF_EXPERIMENTS (python -m rag_fin_amd.build --experiments ->
// libragfin_hip_exp.so, used by tools/ only) the same names are process-wide ints set through
// rf_set_tuning (api.hip), for A/B runs in one process.  ONE list: X(name, default, low, high)
// gives the constant rf_knob_<name> here, and the variable and the rf_set_tuning key "<name>"
// with its range in api.hip.
#define RF_KNOBS(X)                                                                                                  \
  X(ring24, 8, 6, 24)            /* register-ring depth (fragments) of the dim-384 emit sweep: 6 | 8 | 12 | 24 */    \
  X(emit_wgs_per_cu, 0, 0, 4)    /* emit grid = CUs x this (0 = default for the dim) */                              \
  X(sample_bpw, 2, 1, 8)         /* sample blocks per wave */                                                        \
  X(sq8_ring12, 6, 4, 12)        /* register-ring depth (fragments) of the dim-384 int8 emit: 12 | 6 | 4 (A/B only: the product ships 6) */ \
  X(sample_fold, 1, 0, 1)        /* 64-query sweep: the emit skips the sampled blocks (k_threshold appends what the sample kept) */ \
  X(fold_dbg, 0, 0, 3)           /* sample fold diagnostics: 1 = every kept list counts as incomplete (all rescanned), 2 = k_merge leaves the candidate counters */ \
  X(wide_sample_pairs, 4, 1, 8)  /* wide sample pass: block pairs per workgroup, at most */                          \
  X(wide_dbg, 0, 0, 63)          /* wide sweep diagnostic bits (clock stamps, ablations: scan_wide.hip, dispatch_w16) */ \
  X(wide_ne, 0, 0, 112)          /* wide sweep: LDS-DMA pieces per phase of waves 0-3 (0 = the product's split) */   \
  X(linear_dma, 1, 0, 3)         /* encoder: layer 0's QKV GEMM through the LDS-DMA ring at >= 8192 token slots (0 off, 1 auto, 2 always 256-token, 3 never 256-token) */ \
  X(linear_small, 1, 0, 1)       /* encoder: feature-split GEMMs + separate LayerNorm at <= 1024 token slots */      \
  X(encode_graph, 1, 0, 1)       /* encoder: query-sized forwards replay a cached hipGraph */                        \
  X(linear_dbg, 0, 0, 63)        /* encoder: k_linear_dma ablation bits (results wrong) */                           \
  X(debug_epi, 0, 0, 5)          /* encoder: which kernel writes clock stamps (0 QKV k_linear_dma, 2 attention, 5 post block; 1, 3, 4 stamped kernels that are gone and select none) */ \
  X(one_query, 1, 0, 1)          /* encoder: a single sequence of <= 32 tokens takes the fused QKV + attention launch */ \
  X(post_block, 1, 0, 1)         /* encoder: out-projection + MLP of a layer as one launch at >= 8192 token slots (encoder_post.hip) */ \
  X(post_qkv, 1, 0, 1)           /* encoder: k_post_block also computes the next layer's QKV projection */           \
  X(post_dbg, 0, 0, 511)         /* encoder: k_post_block ablation bits (results wrong) */
#ifdef RF_EXPERIMENTS
#define RF_KNOB_DECL(name, dflt, lo, hi) extern int rf_knob_##name;
#else
#define RF_KNOB_DECL(name, dflt, lo, hi) static constexpr int rf_knob_##name = dflt;
#endif
RF_KNOBS(RF_KNOB_DECL)
#undef RF_KNOB_DECL
#ifdef RF_EXPERIMENTS
extern int rf_tuning_generation;   // bumped by rf_set_tuning: cached encode graphs of older settings are not replayed
extern void* rf_debug_buffer;      // rf_debug_set_buffer: clock stamps of the diagnostic runs
#else
static constexpr int rf_tuning_generation = 0;
static constexpr void* rf_debug_buffer = nullptr;
#endif

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device: cache what has
// been set per device, not per process (a second index / encoder on another GPU of the same
// process must get the attribute too).  Racing first calls both set it: idempotent.
#define RF_MAX_DEVICES 64
struct rf_lds_attr {
  std::atomic<uint32_t> bytes[RF_MAX_DEVICES];
};
static inline hipError_t rf_ensure_lds(rf_lds_attr& a, const void* fn, size_t lds) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= RF_MAX_DEVICES) return hipErrorInvalidDevice;
  if (a.bytes[dev].load(std::memory_order_relaxed) >= lds) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) a.bytes[dev].store((uint32_t)lds, std::memory_order_relaxed);
  return e;
}

// queries per wide sweep (scan_wide.hip); every per-query workspace array is sized for it
#define RF_QWIDE 256
// per-query candidate capacity of the fused scan: RF_CAND_SHARDS lists (picked by
// workgroup id) of RF_SHARD_CAP entries; the merge handles RF_CAND_CAP in total
#define RF_CAND_CAP 8192
#define RF_CAND_SHARDS 8
#define RF_SHARD_CAP 2048
// rows below which the sample pass is skipped (every row becomes a candidate)
#define RF_SMALL_ROWS 8192
// partition maxima per query produced by the sample pass (one per workgroup)
#define RF_SAMPLE_WGS 256
// rescoring-set capacity per query
#define RF_RESCORE_CAP 256
// sample fold: waves of a sample pass (RF_SAMPLE_WGS workgroups of at most 8 waves) and the
// most blocks it reads (at most 8 per wave: rf_knob_sample_bpw)
#define RF_FOLD_WAVES (RF_SAMPLE_WGS * 8)
#define RF_FOLD_BLOCKS (RF_FOLD_WAVES * 8)

struct rf_workspace {
  float* thr;          // [64]
  float* eps;          // [64]
  uint32_t* cand_cnt;  // [64][RF_CAND_SHARDS]
  float* pmax;         // [64][RF_SAMPLE_WGS]
  uint2* cand;         // [64][RF_CAND_SHARDS][RF_SHARD_CAP]  {row, score bits}
  // sample fold (scan.hip, k_threshold): what the sample pass saw, per sample wave
  uint4* fold;         // [64 queries][RF_FOLD_WAVES] {best score bits, its row, second best score bits, 0}
  unsigned long long* rmask;  // [RF_FOLD_WAVES] queries whose kept list of that wave is incomplete
  uint32_t* rlist;     // [RF_FOLD_BLOCKS] sampled blocks the emit sweeps again (of waves with rmask != 0)
  uint32_t* rcnt;      // [1] entries of rlist
  // exhaustive path
  double* ex_score;    // [RF_EX_LISTS][RF_MAX_K]
  int64_t* ex_row;     // [RF_EX_LISTS][RF_MAX_K]
};
#define RF_EX_WGS 256

void rf_set_error(const char* fmt, ...);
#define RF_HIP(call)                                                              \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) {                                                       \
      rf_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                   __LINE__);                                                     \
      return RF_ERR_HIP;                                                          \
    }                                                                             \
  } while (0)

// index.hip: row-major fp16 [n, 16*KS] -> fragment-tiled (also used for encoder weights)
void rf_launch_tile_rows(const void* rows, uint4* tiles, int64_t first_row, int64_t n, int KS,
                         hipStream_t st);
// filter.hip: views into a caller's filter buffer (include/ragfin.h, "filtered search")
#define RF_FILTER_HDR_WORDS 4
#define RF_FILTER_MAX_TILES 1024   // compaction tiles; a tile is 32 * rows_per_thread mask words
struct rf_filter_view {
  const uint32_t* hdr;     // {n_rows, n_pass_rows, n_pass_blocks, n_tiles}
  const uint32_t* mask;    // [nblk]
  const uint32_t* blocks;  // [nblk], the first hdr[2] entries valid
};
size_t rf_filter_layout(int64_t n_rows, size_t* mask_off, size_t* blocks_off, size_t* tiles_off);
rf_filter_view rf_filter_carve(const void* filter, int64_t n_rows);
// Per-query filters (include/ragfin.h, "per-query filters"): the multi-filter buffer is the filter
// buffer of the union of G filters (rf_filter_carve reads it as such), then, 256-byte aligned, the
// G masks block-major: word [b * gp + g] is mask word b of filter g, gp = G rounded up to a power
// of two (words of the padding columns are zero).
struct rf_multi {
  const uint32_t* masks_t;   // [nblk][gp]
  const int32_t* qfilter;    // [B] filter number per query, device
  uint32_t gp;
};
uint32_t rf_multi_columns(int n_filters);
size_t rf_multi_layout(int64_t n_rows, int n_filters, size_t* masks_off);

// Sample fold: the geometry of a sample pass that kept its lists (n_samp = 0: none kept; the
// threshold appends nothing and the emit sweeps every block).  Sample wave s read blocks
// (s + j W) * bstride for s + j W < n_samp.
struct rf_fold {
  uint32_t n_samp;   // sampled blocks
  uint32_t bstride;  // block stride of the sample
  uint32_t W;        // waves of the sample pass
};
// Range search (include/ragfin.h, "range search"): the band radius < a <= range_filter on the
// contract score a, both bounds as fp64 (lo = -inf / hi = +inf: open on that side).  The sweep
// tests MFMA scores against float bounds derived from them and the query's eps; the derivation is
// shared by every kernel (rf_band_floor / rf_band_ceil below).
struct rf_band {
  double lo, hi;
};
// Search-after (include/ragfin.h, "paged search"): per query of the batch, the (fp64 score, id) of
// the hit the page follows, in device memory.  A sweep with a bound is a band sweep (rf_band, both
// sides open without a band of the caller's) whose ceiling is per query: rf_after_ceiling below.
struct rf_after {
  const double* score;   // [B]
  const int64_t* id;     // [B], with the id base
};
// scan.hip (filt: nullptr = every row; otherwise the masked sweep over the filter's blocks)
// band: nullptr = no band; otherwise the band form of the sweep (never with a fold)
// after: nullptr = no bound; otherwise the search-after form (always with a band)
// fold: rf_launch_sample fills it (the fold is off for a filtered sweep and with the knob off);
// rf_launch_threshold and rf_launch_emit take what it filled, nullptr = no fold
// multi: nullptr = one filter for the batch; otherwise per-query filters -- filt is the union of
// the batch's filters and each query's row bits are its own filter's (never with band / after)
// w32: nullptr = plain scores; otherwise per-row weights -- the sweep runs on w32[row] * score, over
// the filter's rows or, without filt, over every row (never with fold / band / after / multi)
int rf_launch_sample(const rf_index* ix, const void* q, int B, int JB, const rf_workspace& ws,
                     int* P_out, hipStream_t st, const rf_filter_view* filt = nullptr,
                     rf_fold* fold = nullptr, const rf_band* band = nullptr, const rf_after* after = nullptr,
                     const rf_multi* multi = nullptr, const float* w32 = nullptr);
int rf_launch_emit(const rf_index* ix, const void* q, int B, int JB, const rf_workspace& ws,
                   hipStream_t st, const rf_filter_view* filt = nullptr, const rf_fold* fold = nullptr,
                   const rf_band* band = nullptr, const rf_after* after = nullptr,
                   const rf_multi* multi = nullptr, const float* w32 = nullptr);
// Shape of the 64-query sweeps (scan.hip, grouped.hip): waves per workgroup by dim, and the emit
// grid = CUs x workgroups per CU (0 = the default of the dim), at most one wave per 32-row block.
static inline int rf_waves_per_wg(int KS) { return KS >= 48 ? 8 : 4; }
static inline int rf_emit_grid(const rf_index* ix, int wgs_per_cu) {
  const int WAVES = rf_waves_per_wg(ix->KS);
  const uint32_t nblk = (uint32_t)((ix->size + 31) / 32);
  int grid = ix->num_cus * (wgs_per_cu > 0 ? wgs_per_cu : (ix->KS >= 48 ? 1 : 2));
  const uint32_t need = (nblk + WAVES - 1) / WAVES;
  if ((uint32_t)grid > need) grid = (int)need;
  return grid < 1 ? 1 : grid;
}
int rf_launch_debug_scores(const rf_index* ix, const void* q, int B, int64_t n, float* out,
                           hipStream_t st);
int rf_scan_supported_dim(int dim);
// scan_wide.hip
int rf_wide_supported(const rf_index* ix);
int rf_launch_wide_sample(const rf_index* ix, const void* q, int B, const rf_workspace& ws, int* P_out,
                          hipStream_t st);
int rf_launch_wide_emit(const rf_index* ix, const void* q, int B, const rf_workspace& ws, hipStream_t st);
// sq8.hip: the SQ8 shadow (include/ragfin.h, "SQ8 index").  Per-query quantization of a sweep,
// written by rf_launch_sq8_queries into the workspace area after the FLAT carve.
struct rf_sq8_ws {
  int8_t* q8;          // [64][dim] q^
  float* tq;           // [64] query scale t_q
  float* nq;           // [64] ||q||, rounded up
  float* fq;           // [64] ||q - t_q q^||, rounded up
};
// quantize rows [row0, 32 * ceil(row1 / 32)) of the fp16 tiles into the shadow (pad rows give 0)
int rf_sq8_quantize_rows(rf_index* ix, int64_t row0, int64_t row1, hipStream_t st);
int rf_launch_sq8_queries(const rf_index* ix, const void* q, int B, const rf_sq8_ws& sw, hipStream_t st);
int rf_launch_sq8_emit(const rf_index* ix, int B, int JB, const rf_workspace& ws, const rf_sq8_ws& sw,
                       hipStream_t st);
int rf_launch_sq8_debug(const rf_index* ix, int B, int64_t n, const rf_sq8_ws& sw, float* out, float* delta,
                        hipStream_t st);
// shadow_refine.hip: behind rf_launch_sq8_emit -- prune each query's candidates by the per-row bound
// and replace them by {row, fp16-accurate score} of the survivors
int rf_launch_shadow_refine(const rf_index* ix, const void* q, int B, int k, const rf_workspace& ws,
                            const rf_sq8_ws& sw, hipStream_t st);
// merge.hip
int rf_launch_threshold(const rf_index* ix, const void* q, int B, int k, int P,
                        const rf_workspace& ws, hipStream_t st, const rf_fold* fold = nullptr,
                        const rf_sq8_ws* sq8 = nullptr, const rf_band* band = nullptr);
// the per-query eps of k_threshold into ws.eps, ahead of a band sample pass (which clips by it)
int rf_launch_band_eps(const rf_index* ix, const void* q, int B, const rf_workspace& ws, hipStream_t st);
int rf_launch_merge(const rf_index* ix, const void* q, int B, int k, int64_t id_base,
                    const rf_workspace& ws, float* scores, int64_t* ids, double* exact,
                    uint32_t* flags, hipStream_t st, const rf_band* band = nullptr,
                    const rf_after* after = nullptr);
int rf_launch_exhaustive(const rf_index* ix, const void* q, int B, int k, int64_t id_base,
                         const rf_workspace& ws, float* scores, int64_t* ids, double* exact,
                         const double* after_s, const int64_t* after_r, hipStream_t st,
                         const uint32_t* mask = nullptr, const rf_band* band = nullptr);
// Per-row weights (include/ragfin.h, "decayed search"): w32 / w64 [n_rows] on the device, every weight
// in [0, 1].  The sweeps run on w32[row] * score; threshold and merge take eps_w = 2 eps for eps
// (DESIGN 4.4q), and the merge ranks by (w64[row] * s desc, s desc, row asc).
struct rf_weights {
  const float* w32;
  const double* w64;
};
int rf_launch_threshold_weighted(const rf_index* ix, const void* q, int B, int k, int P, const rf_workspace& ws,
                                 hipStream_t st);
int rf_launch_merge_weighted(const rf_index* ix, const void* q, int B, int k, int64_t id_base, const rf_workspace& ws,
                             const double* w64, float* scores, int64_t* ids, double* decayed, double* base,
                             uint32_t* flags, hipStream_t st);
// (uses ws.cand as the third list array beside ws.ex_score / ws.ex_row)
int rf_launch_exhaustive_weighted(const rf_index* ix, const void* q, int B, int k, int64_t id_base,
                                  const rf_workspace& ws, const double* w64, float* scores, int64_t* ids,
                                  double* decayed, double* base, hipStream_t st, const uint32_t* mask);
// grouped.hip (include/ragfin.h, "grouping search"): one code per row, the best n_groups groups by
// their best group_size rows.  The sweeps write one partition of group maxima per workgroup.
#define RF_GROUP_PARTS 512   // partitions (workgroups) of the group-maximum sweep, at most
struct rf_group {
  const int32_t* codes;  // device [n_rows]; a code outside [0, n_codes) = a row without a group
  int n_codes;           // <= RF_GROUP_MAX_CODES
  int n_groups;          // groups returned per query
  int group_size;        // rows returned per group
};
struct rf_grouped_ws {
  float* gpmax;          // [RF_GROUP_PARTS][64][n_codes] partition maxima per (query, code)
  float* gthr;           // [64][RF_GROUP_MAX_CODES] emit threshold per (query, code)
};
// (eps: rf_launch_band_eps writes it ahead of the chain)
int rf_launch_group_max(const rf_index* ix, const void* q, int B, int JB, const rf_group& g,
                        const rf_workspace& ws, const rf_grouped_ws& gws, int* P_out, hipStream_t st,
                        const rf_filter_view* filt);
int rf_launch_group_threshold(int B, const rf_group& g, int P, const rf_workspace& ws,
                              const rf_grouped_ws& gws, hipStream_t st);
int rf_launch_group_emit(const rf_index* ix, const void* q, int B, int JB, const rf_group& g,
                         const rf_workspace& ws, const rf_grouped_ws& gws, hipStream_t st,
                         const rf_filter_view* filt);
int rf_launch_merge_grouped(const rf_index* ix, const void* q, int B, const rf_group& g, int64_t id_base,
                            const rf_workspace& ws, float* scores, int64_t* ids, double* exact,
                            uint32_t* flags, hipStream_t st);
int rf_launch_merge_shards(const double* exact, const int64_t* ids, size_t shard_stride, int W, int B, int k,
                           float* scores_out, int64_t* ids_out, const uint32_t* flags_in, size_t flag_stride,
                           uint32_t* flags_out, hipStream_t st);
// mmr.hip (include/ragfin.h, "diversified search"): MMR selection of k of the fetch_k candidates
// per query, one workgroup per query; the arguments are checked by the caller
int rf_launch_mmr(const rf_index* ix, int B, int fetch_k, int k, double lambda, int64_t id_base,
                  const double* cand_exact, const int64_t* cand_ids, float* scores, int64_t* ids,
                  double* exact, hipStream_t st);

// sparse.hip, text_match.hip: the handle over the caller's posting arrays (include/ragfin.h, "lexical
// search"), and the token positions of every posting once rf_sparse_attach_positions gave them
struct rf_sparse {
  int64_t n_rows, n_terms, nnz;
  const int64_t* post_off;
  const uint32_t* post_row;
  const float* post_imp;
  int device;
  const int64_t* pos_off;   // [nnz + 1], nullptr while no positions are attached
  const uint32_t* pos;      // [n_pos]
  int64_t n_pos;
};

// order-preserving map float -> uint32 (larger float <=> larger uint)
__host__ __device__ inline uint32_t rf_f2ord(float f) {
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float rf_ord2f(uint32_t o) {
  uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __builtin_bit_cast(float, u);
}

// Range search: the float at or just below / at or just above a double (never on the wrong side
// of it; +-inf pass through), by one step in the ordered encoding.
__host__ __device__ inline float rf_band_floor(double x) {
  const float f = (float)x;
  return (double)f > x ? rf_ord2f(rf_f2ord(f) - 1u) : f;
}
__host__ __device__ inline float rf_band_ceil(double x) {
  const float f = (float)x;
  return (double)f < x ? rf_ord2f(rf_f2ord(f) + 1u) : f;
}

// Search-after: the largest double below x (+-inf and a NaN pass through).
__host__ __device__ inline double rf_next_below(double x) {
  if (!(x > -INFINITY && x < INFINITY)) return x;
  uint64_t u = __builtin_bit_cast(uint64_t, x);
  if (x > 0.0) u -= 1u;
  else if (x == 0.0) u = 0x8000000000000001ull;   // below +-0: the negative subnormal
  else u += 1u;
  return __builtin_bit_cast(double, u);
}
// The fp64 ceiling of a query whose page follows a hit of score `after` inside a band up to hi.
// Plain: min(hi, after) -- no eligible row scores above it.  strict: a row at or below it is
// eligible whatever its id, i.e. it scores strictly below the bound when the bound is the tighter
// (or an equal) side.  A NaN bound leaves hi (the merge's (score, id) rule then drops every row).
__host__ __device__ inline double rf_after_ceiling(double hi, double after, bool strict) {
  if (!(after <= hi)) return hi;
  return strict ? rf_next_below(after) : after;
}
