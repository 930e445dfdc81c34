// Metric aggregations: the exact sum, count, min and max of numeric columns per selected facet bucket and
// over all passing rows (include/ragfin.h, "metric aggregations").
//
//   k_stats_slots   rf_facet_select's device output -> per field an int32 table slot_of[bin]: the position
//                   of the bin among the selected buckets, -1 for a bin that was not selected
//   k_facet_stats   grid (workgroups, fields + 1); column f < fields walks field f's units exactly as
//                   k_facet_counts does (facet_walk.h), the last column takes every passing row as a unit
//                   of its one slot.  A unit maps bin -> slot, skips -1, and adds each metric's value into
//                   the record (slot, metric): three 32-bit pieces of the value's fixed-point image into
//                   int64 limbs (exact_sum.h), the count, and min / max through order-preserving keys.
//                   64-bit integer atomics only: into a workgroup-private LDS copy of the field's records
//                   when slots x metrics <= RF_STATS_LDS_RECORDS, flushed with one global add per non-zero
//                   word; straight into global memory beyond that.
//   k_stats_finish  a lane per record: carries, one rounding to the nearest double, the inf / NaN rule
// Integer adds and max commute: the same inputs give the same bits on every run, whatever the grid.
#include "facet_walk.h"
#include "exact_sum.h"

#define STATS_LDS_WORDS (RF_STATS_LDS_RECORDS * RF_STATS_WORDS)

struct StatsArgs {
  rf_facet_field f[RF_FACET_MAX_FIELDS];
  rf_stats_metric m[RF_STATS_MAX_METRICS];
  int64_t rec_off[RF_FACET_MAX_FIELDS + 1];   // the first record of each field; [n_fields]: the all-rows group
  int32_t n_slots[RF_FACET_MAX_FIELDS + 1];   // min(limit, n_bins) per field; 1 for the all-rows group
  FilterWalk W;
  const int32_t* slot_of;
  unsigned long long* acc;
  int32_t n_fields, n_metrics;
};

// a workgroup per field (slot_of is -1 everywhere when it starts)
__global__ void __launch_bounds__(FACET_THREADS) k_stats_slots(StatsArgs P, const long long* __restrict__ sel,
                                                               uint32_t limit, int32_t* __restrict__ slot_of) {
  const rf_facet_field& F = P.f[blockIdx.x];
  const uint32_t n_bins = (uint32_t)F.n_codes + (F.kind == RF_FACET_DYNAMIC ? 2u : 0u);
  const long long* out = sel + (size_t)blockIdx.x * (RF_FACET_SCALARS + 2u * limit);
  const long long selected = out[0];
  for (uint32_t s = threadIdx.x; s < limit; s += FACET_THREADS) {
    const long long bin = out[RF_FACET_SCALARS + limit + s];
    if ((long long)s < selected && bin >= 0 && bin < (long long)n_bins && s < (uint32_t)P.n_slots[blockIdx.x])
      slot_of[F.counter_off + bin] = (int32_t)s;
  }
}

__global__ void __launch_bounds__(FACET_THREADS) k_facet_stats(StatsArgs P) {
  __shared__ unsigned long long s_acc[STATS_LDS_WORDS];
  const uint32_t fi = blockIdx.y;
  const bool all = fi == (uint32_t)P.n_fields;   // (uniform) the all-rows group: no field, one slot
  const rf_facet_field& F = P.f[all ? 0u : fi];   // (not read for the all-rows group)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t n_codes = all ? 0u : (uint32_t)F.n_codes;
  const uint32_t n_bins = n_codes + (!all && F.kind == RF_FACET_DYNAMIC ? 2u : 0u);
  const uint32_t M = (uint32_t)P.n_metrics;
  const uint32_t n_slots = (uint32_t)P.n_slots[fi];
  const uint32_t n_rec = n_slots * M;
  const bool lds = n_rec <= (uint32_t)RF_STATS_LDS_RECORDS;
  const uint32_t npass = walk_count(P.W);
  const uint32_t per = (!all && F.kind == RF_FACET_ARRAY) ? 1u : 2u;   // blocks a wave takes per step
  const uint32_t n_items = (npass + per - 1u) / per;
  if (n_slots == 0u || blockIdx.x * FACET_WAVES >= n_items) return;   // (uniform over the workgroup)
  unsigned long long* G = P.acc + (size_t)P.rec_off[fi] * RF_STATS_WORDS;
  const int32_t* slot_of = all ? nullptr : P.slot_of + F.counter_off;
  const uint32_t n_words = n_rec * RF_STATS_WORDS;
  if (lds) {
    for (uint32_t i = threadIdx.x; i < n_words; i += FACET_THREADS) s_acc[i] = 0ull;
    __syncthreads();
  }
  unsigned long long* A = lds ? s_acc : G;
  // one unit: its slot's record of every metric takes the row's value
  auto unit = [&](bool act, uint32_t bin, uint32_t row) {
    int32_t slot = -1;
    if (act) slot = all ? 0 : (bin < n_bins ? slot_of[bin] : -1);   // (bin == n_bins is `missing`: no bucket)
    if (slot < 0 || (uint32_t)slot >= n_slots) return;
    for (uint32_t m = 0u; m < M; ++m) {   // (uniform)
      unsigned long long* R = A + ((size_t)slot * M + m) * RF_STATS_WORDS;
      auto add = [&](int word, int64_t delta) { atomicAdd(&R[word], (unsigned long long)delta); };
      auto mx = [&](int word, uint64_t key) { atomicMax(&R[word], (unsigned long long)key); };
      const long long v = ((const long long*)P.m[m].column_dev)[row];
      if (P.m[m].is_f64) es_accumulate_f64((uint64_t)v, add, mx);
      else es_accumulate_i64((int64_t)v, add, mx);
    }
  };
  for (uint32_t it = blockIdx.x * FACET_WAVES + wave; it < n_items; it += gridDim.x * FACET_WAVES) {   // (per wave)
    if (all) {
      const uint32_t j = it * 2u + (lane >> 5);
      bool act = false;
      uint32_t row = 0u;
      if (j < npass) {
        const uint32_t b = walk_block(P.W, j);
        act = ((walk_mask(P.W, b) >> (lane & 31u)) & 1u) != 0u;
        row = b * 32u + (lane & 31u);
      }
      unit(act, 0u, row);
    } else {
      facet_units(F, P.W, it, npass, lane, n_codes, n_bins, unit);
    }
  }
  if (lds) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_words; i += FACET_THREADS) {
      const unsigned long long v = s_acc[i];
      if (!v) continue;
      const uint32_t word = i % RF_STATS_WORDS;
      if (word == ES_MIN || word == ES_MAX) atomicMax(&G[i], v);
      else atomicAdd(&G[i], v);
    }
  }
}

__global__ void __launch_bounds__(FACET_THREADS) k_stats_finish(long long* __restrict__ acc, StatsArgs P, int64_t n_records,
                                                                long long* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * FACET_THREADS + threadIdx.x;
  if (r >= n_records) return;
  es_finish((int64_t*)acc + r * RF_STATS_WORDS, P.m[r % P.n_metrics].is_f64, (int64_t*)out + r * RF_STATS_OUT);
}

// ---- the entry points --------------------------------------------------------------------------------
static int check_metrics(const char* fn, const rf_stats_metric* metrics_host, int n_metrics, bool need_columns) {
  if (!metrics_host || n_metrics < 1 || n_metrics > RF_STATS_MAX_METRICS) {
    rf_set_error("%s: null metrics, or n_metrics = %d outside 1..%d", fn, n_metrics, RF_STATS_MAX_METRICS);
    return RF_ERR_INVALID;
  }
  for (int m = 0; m < n_metrics; ++m)
    if (need_columns && (!metrics_host[m].column_dev || (((uintptr_t)metrics_host[m].column_dev) & 7))) {
      rf_set_error("%s: metric %d: the column is null or not 8-byte aligned", fn, m);
      return RF_ERR_INVALID;
    }
  return RF_OK;
}

// the record layout of a call: fields (n_fields may be 0), then the all-rows group; -> records in all
static int64_t stats_layout(StatsArgs& P, const rf_facet_field* fields_host, int n_fields, int n_metrics, int limit) {
  int64_t at = 0;
  for (int i = 0; i < n_fields; ++i) {
    P.f[i] = fields_host[i];
    const int64_t bins = (int64_t)facet_bins(fields_host[i]);
    P.rec_off[i] = at;
    P.n_slots[i] = (int32_t)(bins < limit ? bins : limit);
    at += (int64_t)P.n_slots[i] * n_metrics;
  }
  P.rec_off[n_fields] = at;
  P.n_slots[n_fields] = 1;
  P.n_fields = n_fields;
  P.n_metrics = n_metrics;
  return at + n_metrics;
}

extern "C" int64_t rf_facet_stats_records(const rf_facet_field* fields_host, int n_fields, int n_metrics, int limit) {
  if (n_fields < 0 || n_fields > RF_FACET_MAX_FIELDS || (n_fields > 0 && !fields_host) || n_metrics < 1 ||
      n_metrics > RF_STATS_MAX_METRICS || limit < 1 || limit > RF_FACET_MAX_LIMIT)
    return -1;
  StatsArgs P{};
  return stats_layout(P, fields_host, n_fields, n_metrics, limit);
}

extern "C" int rf_facet_stats_slots(const rf_facet_field* fields_host, int n_fields, const int64_t* select_dev, int limit,
                                    int32_t* slot_of_dev, int64_t n_counters, void* stream) {
  static const char* fn = "rf_facet_stats_slots";
  if (!select_dev || (((uintptr_t)select_dev) & 7) || !slot_of_dev || (((uintptr_t)slot_of_dev) & 3) || n_counters < 1) {
    rf_set_error("%s: select_dev or slot_of_dev is null or misaligned, or n_counters < 1", fn);
    return RF_ERR_INVALID;
  }
  if (limit < 1 || limit > RF_FACET_MAX_LIMIT) {
    rf_set_error("%s: limit = %d outside 1..%d", fn, limit, RF_FACET_MAX_LIMIT);
    return RF_ERR_INVALID;
  }
  int rc = check_fields(fn, fields_host, n_fields, n_counters, false, false);
  if (rc != RF_OK) return rc;
  StatsArgs P{};
  stats_layout(P, fields_host, n_fields, 1, limit);
  hipStream_t st = (hipStream_t)stream;
  RF_HIP(hipMemsetAsync(slot_of_dev, 0xFF, (size_t)n_counters * 4, st));   // -1: not selected
  hipLaunchKernelGGL(k_stats_slots, dim3((uint32_t)n_fields), dim3(FACET_THREADS), 0, st, P,
                     (const long long*)select_dev, (uint32_t)limit, slot_of_dev);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

extern "C" int rf_facet_stats(const void* filter_dev, const rf_facet_field* fields_host, int n_fields,
                              const rf_stats_metric* metrics_host, int n_metrics, const int32_t* slot_of_dev,
                              int64_t n_counters, int limit, int64_t n_rows, int64_t* acc_dev, int64_t n_records, int grid,
                              void* stream) {
  static const char* fn = "rf_facet_stats";
  if (!acc_dev || (((uintptr_t)acc_dev) & 7)) {
    rf_set_error("%s: acc_dev is null or not 8-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  if (n_fields < 0 || limit < 1 || limit > RF_FACET_MAX_LIMIT || grid < 0) {
    rf_set_error("%s: n_fields = %d < 0, limit = %d outside 1..%d, or grid = %d < 0", fn, n_fields, limit,
                 RF_FACET_MAX_LIMIT, grid);
    return RF_ERR_INVALID;
  }
  if (n_rows > (int64_t)0x7FFFFFFFll) {   // a limb takes fewer than 2^31 pieces (exact_sum.h)
    rf_set_error("%s: n_rows = %lld exceeds 2^31 - 1, the bound of the limbs", fn, (long long)n_rows);
    return RF_ERR_INVALID;
  }
  int rc = check_rows(fn, n_rows, filter_dev);
  if (rc != RF_OK) return rc;
  rc = check_metrics(fn, metrics_host, n_metrics, n_rows > 0);
  if (rc != RF_OK) return rc;
  if (n_fields > 0) {
    rc = check_fields(fn, fields_host, n_fields, n_counters, true, false);
    if (rc != RF_OK) return rc;
    if (!slot_of_dev || (((uintptr_t)slot_of_dev) & 3)) {
      rf_set_error("%s: slot_of_dev is null or not 4-byte aligned", fn);
      return RF_ERR_INVALID;
    }
  }
  StatsArgs P{};
  const int64_t need = stats_layout(P, fields_host, n_fields, n_metrics, limit);
  if (n_records != need) {
    rf_set_error("%s: n_records = %lld, the call has %lld (rf_facet_stats_records)", fn, (long long)n_records,
                 (long long)need);
    return RF_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  RF_HIP(hipMemsetAsync(acc_dev, 0, (size_t)n_records * RF_STATS_WORDS * 8, st));
  if (n_rows == 0) return RF_OK;
  for (int m = 0; m < n_metrics; ++m) P.m[m] = metrics_host[m];
  P.W = make_walk(filter_dev, n_rows);
  P.slot_of = slot_of_dev;
  P.acc = (unsigned long long*)acc_dev;
  uint32_t gx = facet_grid(n_rows, FACET_WAVES);
  if (grid > 0) gx = (uint32_t)(grid > FACET_MAX_GRID ? FACET_MAX_GRID : grid);
  hipLaunchKernelGGL(k_facet_stats, dim3(gx, (uint32_t)n_fields + 1u), dim3(FACET_THREADS), 0, st, P);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

extern "C" int rf_facet_stats_finish(int64_t* acc_dev, const rf_stats_metric* metrics_host, int n_metrics,
                                     int64_t n_records, int64_t* out_dev, void* stream) {
  static const char* fn = "rf_facet_stats_finish";
  if (!acc_dev || (((uintptr_t)acc_dev) & 7) || !out_dev || (((uintptr_t)out_dev) & 7)) {
    rf_set_error("%s: acc_dev or out_dev is null or not 8-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  int rc = check_metrics(fn, metrics_host, n_metrics, false);
  if (rc != RF_OK) return rc;
  if (n_records < 1 || n_records % n_metrics != 0 ||
      n_records > (int64_t)(RF_FACET_MAX_FIELDS * RF_FACET_MAX_LIMIT + 1) * RF_STATS_MAX_METRICS) {
    rf_set_error("%s: n_records = %lld is no multiple of n_metrics = %d, or out of range", fn, (long long)n_records,
                 n_metrics);
    return RF_ERR_INVALID;
  }
  StatsArgs P{};
  for (int m = 0; m < n_metrics; ++m) P.m[m] = metrics_host[m];
  P.n_metrics = n_metrics;
  const uint32_t g = (uint32_t)((n_records + FACET_THREADS - 1) / FACET_THREADS);
  hipLaunchKernelGGL(k_stats_finish, dim3(g), dim3(FACET_THREADS), 0, (hipStream_t)stream, (long long*)acc_dev, P,
                     n_records, (long long*)out_dev);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
