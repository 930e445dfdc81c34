// Boosted search: a ranker that multiplies the score of the rows a filter selects (include/ragfin.h,
// "boosted search").  m boost filters split the rows into 2^m classes by which filters
// a row passes; every class has one weight, so inside a class the boosted ranking is the plain one
// and the boosted top-k of the corpus is the merge of the classes' plain filtered top-k lists.
//
//   k_boost_classes  one thread per mask word: the 2^m class words of that word from the m filter
//                    masks (and the base filter's), and the exact row count of every class
//   k_merge_boosted  one workgroup per query: the classes' candidates in LDS, boosted = W * s as one
//                    fp64 multiplication, ranked by counting under (boosted desc, s desc, id asc)
// The class masks depend on their inputs alone and the counts are integer sums: the same filters
// give the same bytes whatever order the workgroups and atomics run in.
#include "rf_internal.h"

#define BOOST_CLASSES (1 << RF_BOOST_MAX)   // 8: classes of a search, and the most a merge takes
#define BOOST_THREADS 256
#define BOOST_MERGE_THREADS (BOOST_CLASSES * RF_MAX_K)   // one lane per candidate of a query
static_assert(BOOST_MERGE_THREADS <= 1024, "one workgroup holds every candidate of a query");

static inline bool boost_rows_ok(int64_t n_rows) {
  return n_rows >= 1 && n_rows <= (int64_t)0xFFFFFFFFll - 32;   // the range of a filter buffer, without 0
}

extern "C" size_t rf_boost_class_stride_words(int64_t n_rows) {
  if (!boost_rows_ok(n_rows)) return 0;
  return (size_t)((n_rows + 31) / 32 + 3) / 4 * 4;
}

// ---- class masks -------------------------------------------------------------------------------------
struct BoostSrc {
  const uint32_t* hdr[RF_BOOST_MAX + 1];    // [0..m) the boost filters, [RF_BOOST_MAX] the base filter or nullptr
  const uint32_t* mask[RF_BOOST_MAX + 1];
};

__global__ void __launch_bounds__(BOOST_THREADS) k_boost_classes(BoostSrc src, uint32_t m, uint32_t n_rows,
                                                                 uint32_t nblk, uint32_t stride,
                                                                 uint32_t* __restrict__ class_masks,
                                                                 unsigned long long* __restrict__ class_counts) {
  __shared__ uint32_t red[BOOST_CLASSES][BOOST_THREADS / 64];
  const uint32_t C = 1u << m;   // (m, C: workgroup-uniform)
  const uint32_t w = blockIdx.x * BOOST_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  uint32_t base = 0u;
  uint32_t f[RF_BOOST_MAX] = {0u, 0u, 0u};
  if (w < nblk) {
    // the rows of this word: the complemented terms below would set the bits past n_rows
    const uint32_t rows = n_rows - w * 32u;   // > 0
    base = rows < 32u ? (1u << rows) - 1u : 0xFFFFFFFFu;
    if (src.hdr[RF_BOOST_MAX]) base &= src.hdr[RF_BOOST_MAX][0] == n_rows ? src.mask[RF_BOOST_MAX][w] : 0u;
    for (uint32_t i = 0; i < m; ++i) f[i] = src.hdr[i][0] == n_rows ? src.mask[i][w] : 0u;   // another row count: no row
  }
#pragma unroll
  for (uint32_t c = 0; c < (uint32_t)BOOST_CLASSES; ++c) {
    if (c >= C) break;
    uint32_t v = base;   // 0 in the padding words [nblk, stride)
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)RF_BOOST_MAX; ++i)
      if (i < m) v &= ((c >> i) & 1u) ? f[i] : ~f[i];
    if (w < stride) class_masks[(size_t)c * stride + w] = v;
    uint32_t pc = (uint32_t)__popc(v);
    for (int o = 32; o > 0; o >>= 1) pc += __shfl_xor(pc, o);
    if (lane == 0) red[c][wave] = pc;
  }
  __syncthreads();
  if (threadIdx.x < C) {
    uint32_t s = 0u;
    for (int i = 0; i < BOOST_THREADS / 64; ++i) s += red[threadIdx.x][i];
    if (s) atomicAdd(&class_counts[threadIdx.x], (unsigned long long)s);   // integer sum: any order, one value
  }
}

extern "C" int rf_boost_classes(const void* base_filter_dev, const void* const* boost_filters, int m, int64_t n_rows,
                                uint32_t* class_masks_dev, int64_t* class_counts_dev, void* stream) {
  if (!boost_filters || !class_masks_dev || !class_counts_dev) {
    rf_set_error("rf_boost_classes: null argument");
    return RF_ERR_INVALID;
  }
  if (m < 1 || m > RF_BOOST_MAX) {
    rf_set_error("rf_boost_classes: m = %d outside 1..%d", m, RF_BOOST_MAX);
    return RF_ERR_INVALID;
  }
  if (!boost_rows_ok(n_rows)) {
    rf_set_error("rf_boost_classes: n_rows = %lld out of range", (long long)n_rows);
    return RF_ERR_INVALID;
  }
  if ((((uintptr_t)class_masks_dev) & 15) || (((uintptr_t)class_counts_dev) & 7)) {
    rf_set_error("rf_boost_classes: the class masks must be 16-byte and the counts 8-byte aligned");
    return RF_ERR_INVALID;
  }
  if (base_filter_dev && (((uintptr_t)base_filter_dev) & 15)) {
    rf_set_error("rf_boost_classes: the base filter buffer must be 16-byte aligned");
    return RF_ERR_INVALID;
  }
  BoostSrc src{};
  for (int i = 0; i < m; ++i) {
    if (!boost_filters[i] || (((uintptr_t)boost_filters[i]) & 15)) {
      rf_set_error("rf_boost_classes: boost filter %d null or not 16-byte aligned", i);
      return RF_ERR_INVALID;
    }
    const rf_filter_view v = rf_filter_carve(boost_filters[i], n_rows);
    src.hdr[i] = v.hdr;
    src.mask[i] = v.mask;
  }
  if (base_filter_dev) {
    const rf_filter_view v = rf_filter_carve(base_filter_dev, n_rows);
    src.hdr[RF_BOOST_MAX] = v.hdr;
    src.mask[RF_BOOST_MAX] = v.mask;
  }
  hipStream_t st = (hipStream_t)stream;
  const uint32_t nblk = (uint32_t)((n_rows + 31) / 32);
  const uint32_t stride = (uint32_t)rf_boost_class_stride_words(n_rows);
  RF_HIP(hipMemsetAsync(class_counts_dev, 0, sizeof(int64_t) << m, st));
  hipLaunchKernelGGL(k_boost_classes, dim3((stride + BOOST_THREADS - 1) / BOOST_THREADS), dim3(BOOST_THREADS), 0, st, src,
                     (uint32_t)m, (uint32_t)n_rows, nblk, stride, class_masks_dev,
                     (unsigned long long*)class_counts_dev);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

// ---- merge of the class answers ------------------------------------------------------------------------
struct BoostMerge {
  double w[BOOST_CLASSES];
  int B, C, k_in, k;
};

// One workgroup per query; lane t = c k_in + j is candidate j of class c.
__global__ void __launch_bounds__(BOOST_MERGE_THREADS) k_merge_boosted(BoostMerge P, const double* __restrict__ exact,
                                                                       const int64_t* __restrict__ cand,
                                                                       float* __restrict__ scores,
                                                                       int64_t* __restrict__ ids,
                                                                       double* __restrict__ boosted_out,
                                                                       double* __restrict__ base_out) {
  __shared__ int64_t s_id[BOOST_MERGE_THREADS];
  __shared__ double s_base[BOOST_MERGE_THREADS];
  __shared__ double s_boost[BOOST_MERGE_THREADS];
  const int t = threadIdx.x;
  const int b = blockIdx.x;
  const int n = P.C * P.k_in;   // <= BOOST_MERGE_THREADS (checked by the caller)
  int64_t id = -1;
  double s = -INFINITY, bs = -INFINITY;
  if (t < n) {
    const size_t at = (size_t)b * n + t;
    id = cand[at];
    if (id < 0) {
      id = -1;
    } else {
      s = exact[at];
      bs = __dmul_rn(P.w[t / P.k_in], s);   // one multiplication, rounded once: never contracted
    }
  }
  s_id[t] = id;
  s_base[t] = s;
  s_boost[t] = bs;
  __syncthreads();
  // rank = the candidates before this one under (boosted desc, s desc, id asc); ids are distinct (the
  // classes are disjoint), a repeated id would rank by its position
  int rank = 0, live = 0;
  for (int e = 0; e < n; ++e) {
    const int64_t oid = s_id[e];
    if (oid < 0) continue;
    ++live;
    const double ob = s_boost[e], os = s_base[e];
    const bool before = ob > bs || (ob == bs && (os > s || (os == s && (oid < id || (oid == id && e < t)))));
    rank += before ? 1 : 0;
  }
  if (id >= 0 && rank < P.k) {
    const size_t o = (size_t)b * P.k + rank;
    scores[o] = (float)bs;
    ids[o] = id;
    if (boosted_out) boosted_out[o] = bs;
    if (base_out) base_out[o] = s;
  }
  for (int o = live + t; o < P.k; o += BOOST_MERGE_THREADS) {
    const size_t at = (size_t)b * P.k + o;
    scores[at] = -INFINITY;
    ids[at] = -1;
    if (boosted_out) boosted_out[at] = -INFINITY;
    if (base_out) base_out[at] = -INFINITY;
  }
}

extern "C" int rf_merge_boosted(const double* exact_dev, const int64_t* ids_dev, int B, int C, int k_in,
                                const double* class_weight_host, int k, float* scores_dev, int64_t* ids_out_dev,
                                double* boosted_dev, double* base_dev, void* stream) {
  if (!exact_dev || !ids_dev || !class_weight_host || !scores_dev || !ids_out_dev) {
    rf_set_error("rf_merge_boosted: null argument");
    return RF_ERR_INVALID;
  }
  if (B < 1 || C < 1 || C > BOOST_CLASSES || k_in < 1 || k_in > RF_MAX_K || k < 1 || k > RF_MAX_K) {
    rf_set_error("rf_merge_boosted: need B >= 1, 1 <= C <= %d, 1 <= k_in <= %d, 1 <= k <= %d (got B = %d, C = %d, "
                 "k_in = %d, k = %d)", BOOST_CLASSES, RF_MAX_K, RF_MAX_K, B, C, k_in, k);
    return RF_ERR_INVALID;
  }
  BoostMerge P{};
  for (int c = 0; c < C; ++c) {
    const double w = class_weight_host[c];
    if (!(w > 0.0) || w > 1.79769313486231570e308) {   // also catches a NaN and +inf
      rf_set_error("rf_merge_boosted: class weight %d = %g must be finite and > 0", c, w);
      return RF_ERR_INVALID;
    }
    P.w[c] = w;
  }
  P.B = B;
  P.C = C;
  P.k_in = k_in;
  P.k = k;
  hipLaunchKernelGGL(k_merge_boosted, dim3((uint32_t)B), dim3(BOOST_MERGE_THREADS), 0, (hipStream_t)stream, P, exact_dev,
                     ids_dev, scores_dev, ids_out_dev, boosted_dev, base_dev);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
