// Faceted counts: how many of the rows a filter passes hold each value of a dictionary-coded column, the
// best bins of each field, and range counts over a numeric column (include/ragfin.h, "faceted counts";
// DESIGN 4.4t).
//
//   k_facet_counts      grid (workgroups, fields).  The filter's ascending list of passing 32-row blocks is
//                       the work list (no filter: every block).  CODES / DYNAMIC: a wave takes two blocks, a
//                       lane one row.  ARRAY: a wave takes one block, keeps its 33 offsets in registers and
//                       strides over the block's contiguous element span; an element counts when its
//                       first-occurrence byte is set and its row passes (the row by a 5-step search over the
//                       offsets through shuffles).  Lanes that hit the same bin are merged by ballot first;
//                       then an LDS histogram (n_codes <= RF_FACET_LDS_CODES) flushed with one global add per
//                       non-zero bin, or global integer atomics.
//   k_first_occurrence  a wave per row: element e is flagged when no earlier element of its row equals it
//   k_facet_select      a workgroup per field: radix select of the limit-th best (count, rank) key, gather,
//                       bitonic sort in LDS
//   k_facet_ranges      range counts by ballot, LDS partials, integer adds; min / max through an
//                       order-preserving key
// Integer adds, min and max commute: the same inputs give the same bits on every run.
#include "facet_walk.h"

#define FACET_LDS_BINS (RF_FACET_LDS_CODES + 3)   // the codes, False / True of a dynamic key, `missing`
#define SELECT_THREADS 1024

// hist[bin] += 1 for every active lane.  Called by all 64 lanes of a wave together: up to four distinct
// bins are merged by ballot (one add each of the lane count), the lanes left over add on their own.
template <typename T>
__device__ __forceinline__ void wave_add(T* hist, bool active, uint32_t bin, uint32_t lane) {
  for (int round = 0; round < 4; ++round) {
    const unsigned long long act = __ballot(active);
    if (act == 0ull) return;   // (wave-uniform)
    const int leader = __ffsll((long long)act) - 1;
    const uint32_t lb = (uint32_t)__shfl((int)bin, leader);
    const bool same = active && bin == lb;
    const unsigned long long m = __ballot(same);
    if ((int)lane == leader) atomicAdd(&hist[lb], (T)__popcll(m));
    active = active && !same;
  }
  if (active) atomicAdd(&hist[bin], (T)1);
}

// ---- rf_facet_counts -------------------------------------------------------------------------------
struct FacetArgs {
  rf_facet_field f[RF_FACET_MAX_FIELDS];
  FilterWalk W;
  unsigned long long* counters;
};

__global__ void __launch_bounds__(FACET_THREADS) k_facet_counts(FacetArgs P) {
  __shared__ uint32_t s_hist[FACET_LDS_BINS];
  const rf_facet_field& F = P.f[blockIdx.y];   // (uniform: from the kernel arguments)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t n_codes = (uint32_t)F.n_codes;
  const uint32_t n_bins = n_codes + (F.kind == RF_FACET_DYNAMIC ? 2u : 0u);   // bin n_bins: `missing`
  const bool lds = n_codes <= (uint32_t)RF_FACET_LDS_CODES;
  const uint32_t npass = walk_count(P.W);
  const uint32_t per = F.kind == RF_FACET_ARRAY ? 1u : 2u;   // blocks a wave takes per step
  const uint32_t n_items = (npass + per - 1u) / per;
  if (blockIdx.x * FACET_WAVES >= n_items) return;   // (uniform over the workgroup) nothing to count
  unsigned long long* G = P.counters + F.counter_off;
  if (lds) {
    for (uint32_t i = threadIdx.x; i <= n_bins; i += FACET_THREADS) s_hist[i] = 0u;
    __syncthreads();
  }
  for (uint32_t it = blockIdx.x * FACET_WAVES + wave; it < n_items; it += gridDim.x * FACET_WAVES) {   // (per wave)
    // (the CODES / ARRAY / DYNAMIC unit rules: facet_walk.h)
    facet_units(F, P.W, it, npass, lane, n_codes, n_bins, [&](bool act, uint32_t bin, uint32_t) {
      if (lds) wave_add(s_hist, act, bin, lane); else wave_add(G, act, bin, lane);
    });
  }
  if (lds) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= n_bins; i += FACET_THREADS) {
      const uint32_t v = s_hist[i];
      if (v) atomicAdd(&G[i], (unsigned long long)v);
    }
  }
}

extern "C" int rf_facet_counts(const void* filter_dev, const rf_facet_field* fields_host, int n_fields, int64_t n_rows,
                               int64_t* counters_dev, int64_t n_counters, void* stream) {
  static const char* fn = "rf_facet_counts";
  if (!counters_dev || (((uintptr_t)counters_dev) & 7) || n_counters < 1) {
    rf_set_error("%s: counters_dev is null or not 8-byte aligned, or n_counters < 1", fn);
    return RF_ERR_INVALID;
  }
  int rc = check_rows(fn, n_rows, filter_dev);
  if (rc != RF_OK) return rc;
  rc = check_fields(fn, fields_host, n_fields, n_counters, true, false);
  if (rc != RF_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  RF_HIP(hipMemsetAsync(counters_dev, 0, (size_t)n_counters * 8, st));
  if (n_rows == 0) return RF_OK;
  FacetArgs P{};
  for (int i = 0; i < n_fields; ++i) P.f[i] = fields_host[i];
  P.W = make_walk(filter_dev, n_rows);
  P.counters = (unsigned long long*)counters_dev;
  // (a workgroup's four waves take four ARRAY blocks, or eight blocks of a scalar field, per step)
  hipLaunchKernelGGL(k_facet_counts, dim3(facet_grid(n_rows, FACET_WAVES), (uint32_t)n_fields), dim3(FACET_THREADS), 0,
                     st, P);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

// ---- rf_array_first_occurrence -----------------------------------------------------------------------
__global__ void __launch_bounds__(FACET_THREADS) k_first_occurrence(const int64_t* __restrict__ off,
                                                                   const int32_t* __restrict__ vals, int64_t row_lo,
                                                                   int64_t row_hi, uint8_t* __restrict__ flags) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = threadIdx.x >> 6;
  for (int64_t r = row_lo + (int64_t)blockIdx.x * FACET_WAVES + wave; r < row_hi;
       r += (int64_t)gridDim.x * FACET_WAVES) {   // (per wave)
    const int64_t s = off[r], t = off[r + 1];
    for (int64_t eb = s; eb < t; eb += 64) {
      const int64_t e = eb + (int64_t)lane;
      const bool valid = e < t;
      const int32_t x = valid ? vals[e] : 0;
      bool dup = false;
      const int64_t jmax = (eb + 63 < t - 1) ? eb + 63 : t - 1;   // the last element of this trip: j stays below it
      for (int64_t j = s; j < jmax; ++j) {   // (uniform: one broadcast load per step)
        const int32_t y = vals[j];
        dup = dup || (valid && j < e && y == x);
        if (__ballot(valid && !dup && j + 1 < e) == 0ull) break;   // every lane has its answer
      }
      if (valid) flags[e] = dup ? (uint8_t)0 : (uint8_t)1;
    }
  }
}

extern "C" int rf_array_first_occurrence(const int64_t* offsets_dev, const int32_t* values_dev, int64_t row_lo,
                                         int64_t row_hi, uint8_t* flags_dev, void* stream) {
  static const char* fn = "rf_array_first_occurrence";
  if (row_lo < 0 || row_hi < row_lo || row_hi > (int64_t)0xFFFFFFFFll - 32) {
    rf_set_error("%s: rows [%lld, %lld) out of range", fn, (long long)row_lo, (long long)row_hi);
    return RF_ERR_INVALID;
  }
  if (!offsets_dev || (((uintptr_t)offsets_dev) & 7) || !values_dev || (((uintptr_t)values_dev) & 3) || !flags_dev) {
    rf_set_error("%s: a null array, offsets not 8-byte or values not 4-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  if (row_hi == row_lo) return RF_OK;
  const int64_t g = (row_hi - row_lo + FACET_WAVES - 1) / FACET_WAVES;
  hipLaunchKernelGGL(k_first_occurrence, dim3((uint32_t)(g > 4096 ? 4096 : g)), dim3(FACET_THREADS), 0,
                     (hipStream_t)stream, offsets_dev, values_dev, row_lo, row_hi, flags_dev);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

// ---- rf_facet_select ---------------------------------------------------------------------------------
struct SelectArgs {
  rf_facet_field f[RF_FACET_MAX_FIELDS];
  const unsigned long long* counters;
  long long* out;
  unsigned long long min_count;
  uint32_t limit;
};

__device__ __forceinline__ unsigned long long wave_sum_ull(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// one workgroup per field
__global__ void __launch_bounds__(SELECT_THREADS) k_facet_select(SelectArgs P) {
  constexpr int NW = SELECT_THREADS / 64;
  __shared__ uint32_t s_hist[256];
  __shared__ unsigned long long s_key[SELECT_THREADS];
  __shared__ uint32_t s_bin[SELECT_THREADS];
  __shared__ unsigned long long s_red[3][NW];
  __shared__ unsigned long long s_prefix;
  __shared__ uint32_t s_remaining, s_n;
  const rf_facet_field& F = P.f[blockIdx.x];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n_bins = (uint32_t)F.n_codes + (F.kind == RF_FACET_DYNAMIC ? 2u : 0u);
  const unsigned long long* C = P.counters + F.counter_off;
  const int32_t* rank = F.rank_dev;
  const uint32_t limit = P.limit;
  long long* out = P.out + (size_t)blockIdx.x * (RF_FACET_SCALARS + 2u * limit);
  // bins with a count, the sum of all bins, bins that may be selected
  unsigned long long d = 0ull, tot = 0ull, el = 0ull;
  for (uint32_t i = tid; i < n_bins; i += SELECT_THREADS) {
    const unsigned long long c = C[i];
    d += c > 0ull;
    tot += c;
    el += c >= P.min_count;
  }
  d = wave_sum_ull(d);
  tot = wave_sum_ull(tot);
  el = wave_sum_ull(el);
  if (lane == 0u) {
    s_red[0][wave] = d;
    s_red[1][wave] = tot;
    s_red[2][wave] = el;
  }
  __syncthreads();
  d = tot = el = 0ull;
  for (int i = 0; i < NW; ++i) {
    d += s_red[0][i];
    tot += s_red[1][i];
    el += s_red[2][i];
  }
  const uint32_t want = (uint32_t)(el < (unsigned long long)limit ? el : (unsigned long long)limit);
  // the key of a bin: count, then the complement of the rank, so that the largest key is the best bin;
  // 0 for a bin that may not be selected (min_count >= 1: a selectable key is at least 2^32)
  auto key_of = [&](uint32_t i) -> unsigned long long {
    const unsigned long long c = C[i];
    return c >= P.min_count ? (c << 32) | (unsigned long long)(~(uint32_t)rank[i]) : 0ull;
  };
  if (tid == 0u) {
    s_prefix = 0ull;
    s_remaining = want;
    s_n = 0u;
  }
  s_key[tid] = 0ull;
  s_bin[tid] = 0xFFFFFFFFu;
  __syncthreads();
  if (want > 0u) {   // (uniform)
    // radix select, the top byte first: afterwards s_prefix is the want-th largest key (keys are distinct)
    for (int pass = 7; pass >= 0; --pass) {
      if (tid < 256u) s_hist[tid] = 0u;
      __syncthreads();
      const unsigned long long prefix = s_prefix;
      for (uint32_t i0 = 0u; i0 < n_bins; i0 += SELECT_THREADS) {   // (uniform: wave_add takes whole waves)
        const uint32_t i = i0 + tid;
        const unsigned long long k = i < n_bins ? key_of(i) : 0ull;
        const bool in = k != 0ull && (pass == 7 || (k >> (8 * (pass + 1))) == (prefix >> (8 * (pass + 1))));
        wave_add(s_hist, in, (uint32_t)(k >> (8 * pass)) & 255u, lane);
      }
      __syncthreads();
      if (tid == 0u) {
        uint32_t cum = 0u;
        const uint32_t rem = s_remaining;
        for (int b = 255; b >= 0; --b) {
          if (cum + s_hist[b] >= rem) {
            s_prefix = prefix | ((unsigned long long)b << (8 * pass));
            s_remaining = rem - cum;
            break;
          }
          cum += s_hist[b];
        }
      }
      __syncthreads();
    }
    const unsigned long long cut = s_prefix;
    for (uint32_t i = tid; i < n_bins; i += SELECT_THREADS) {
      const unsigned long long k = key_of(i);
      if (k != 0ull && k >= cut) {
        const uint32_t p = atomicAdd(&s_n, 1u);   // (arrival order: the sort below removes it)
        if (p < SELECT_THREADS) {
          s_key[p] = k;
          s_bin[p] = i;
        }
      }
    }
    __syncthreads();
    // bitonic sort of the 1024 slots by key, descending (empty slots hold 0 and sink to the end)
    for (uint32_t k = 2u; k <= SELECT_THREADS; k <<= 1) {
      for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
        const uint32_t o = tid ^ j;
        if (o > tid) {
          const unsigned long long a = s_key[tid], b = s_key[o];
          if (((tid & k) == 0u) ? a < b : a > b) {
            s_key[tid] = b;
            s_key[o] = a;
            const uint32_t t = s_bin[tid];
            s_bin[tid] = s_bin[o];
            s_bin[o] = t;
          }
        }
        __syncthreads();
      }
    }
  }
  if (tid < limit) {
    out[RF_FACET_SCALARS + tid] = tid < want ? (long long)(s_key[tid] >> 32) : 0ll;
    out[RF_FACET_SCALARS + limit + tid] = tid < want ? (long long)s_bin[tid] : -1ll;
  }
  if (tid == 0u) {
    unsigned long long sel = 0ull;
    for (uint32_t i = 0u; i < want; ++i) sel += s_key[i] >> 32;
    out[0] = (long long)want;
    out[1] = (long long)d;
    out[2] = (long long)sel;
    out[3] = (long long)C[n_bins];
    out[4] = (long long)tot;
    out[5] = out[6] = out[7] = 0ll;
  }
}

extern "C" int rf_facet_select(const rf_facet_field* fields_host, int n_fields, const int64_t* counters_dev,
                               int64_t n_counters, int limit, int64_t min_count, int64_t* out_dev, void* stream) {
  static const char* fn = "rf_facet_select";
  if (!counters_dev || (((uintptr_t)counters_dev) & 7) || !out_dev || (((uintptr_t)out_dev) & 7)) {
    rf_set_error("%s: counters_dev or out_dev is null or not 8-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  if (limit < 1 || limit > RF_FACET_MAX_LIMIT || min_count < 1) {
    rf_set_error("%s: limit = %d outside 1..%d, or min_count = %lld < 1", fn, limit, RF_FACET_MAX_LIMIT,
                 (long long)min_count);
    return RF_ERR_INVALID;
  }
  int rc = check_fields(fn, fields_host, n_fields, n_counters, false, true);
  if (rc != RF_OK) return rc;
  SelectArgs P{};
  for (int i = 0; i < n_fields; ++i) P.f[i] = fields_host[i];
  P.counters = (const unsigned long long*)counters_dev;
  P.out = (long long*)out_dev;
  P.min_count = (unsigned long long)min_count;
  P.limit = (uint32_t)limit;
  hipLaunchKernelGGL(k_facet_select, dim3((uint32_t)n_fields), dim3(SELECT_THREADS), 0, (hipStream_t)stream, P);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

// ---- rf_facet_ranges ---------------------------------------------------------------------------------
struct RangeArgs {
  rf_facet_range r[RF_FACET_MAX_RANGES];
  FilterWalk W;
  const void* column;
  unsigned long long* out;
  int n_ranges, is_f64;
};

// order-preserving keys: a < b as values  <=>  key(a) < key(b) as unsigned (fp64: no NaN comes here)
__device__ __forceinline__ unsigned long long key_of_i64(long long x) { return (unsigned long long)x ^ (1ull << 63); }
__device__ __forceinline__ unsigned long long key_of_f64(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : b | (1ull << 63);
}

#define RANGE_NAN RF_FACET_MAX_RANGES
#define RANGE_VALID (RF_FACET_MAX_RANGES + 1)
#define RANGE_MIN (RF_FACET_MAX_RANGES + 2)   // while the workgroups add: the largest complement of a key
#define RANGE_MAX (RF_FACET_MAX_RANGES + 3)

__global__ void __launch_bounds__(FACET_THREADS) k_facet_ranges(RangeArgs P) {
  __shared__ unsigned long long s_cnt[RF_FACET_MAX_RANGES + 4];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t npass = walk_count(P.W);
  const uint32_t n_items = (npass + 1u) / 2u;
  if (blockIdx.x * FACET_WAVES >= n_items) return;   // (uniform over the workgroup)
  if (threadIdx.x < RF_FACET_MAX_RANGES + 4) s_cnt[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned long long mine = 0ull;          // lane r: the wave's count of range r
  unsigned long long nan = 0ull, nv = 0ull;   // (wave-uniform)
  unsigned long long kmin_c = 0ull, kmax = 0ull;   // the largest ~key and the largest key this lane saw
  for (uint32_t it = blockIdx.x * FACET_WAVES + wave; it < n_items; it += gridDim.x * FACET_WAVES) {   // (per wave)
    const uint32_t j = it * 2u + (lane >> 5);
    bool pass = false;
    uint32_t row = 0u;
    if (j < npass) {
      const uint32_t b = walk_block(P.W, j);
      pass = ((walk_mask(P.W, b) >> (lane & 31u)) & 1u) != 0u;
      row = b * 32u + (lane & 31u);
    }
    long long xi = 0ll;
    double xf = 0.0;
    bool ok = pass;
    unsigned long long key = 0ull;
    if (pass) {
      if (P.is_f64) {
        xf = ((const double*)P.column)[row];
        ok = xf == xf;
        key = key_of_f64(xf);
      } else {
        xi = ((const long long*)P.column)[row];
        key = key_of_i64(xi);
      }
    }
    nan += (unsigned long long)__popcll(__ballot(pass && !ok));
    nv += (unsigned long long)__popcll(__ballot(ok));
    if (ok) {
      kmin_c = max(kmin_c, ~key);
      kmax = max(kmax, key);
    }
    for (int r = 0; r < P.n_ranges; ++r) {   // (uniform)
      const rf_facet_range& R = P.r[r];
      bool in = ok && !(R.flags & RF_FRANGE_EMPTY);
      if (P.is_f64)
        in = in && ((R.flags & RF_FRANGE_NO_LO) || xf >= R.flo) && ((R.flags & RF_FRANGE_NO_HI) || xf < R.fhi);
      else
        in = in && ((R.flags & RF_FRANGE_NO_LO) || xi >= R.ilo) && ((R.flags & RF_FRANGE_NO_HI) || xi < R.ihi);
      const unsigned long long c = (unsigned long long)__popcll(__ballot(in));
      if ((int)lane == r) mine += c;
    }
  }
  if (mine) atomicAdd(&s_cnt[lane], mine);   // (lane < n_ranges <= 64)
  for (int o = 32; o > 0; o >>= 1) {
    kmin_c = max(kmin_c, (unsigned long long)__shfl_xor(kmin_c, o));
    kmax = max(kmax, (unsigned long long)__shfl_xor(kmax, o));
  }
  if (lane == 0u) {
    if (nan) atomicAdd(&s_cnt[RANGE_NAN], nan);
    if (nv) {
      atomicAdd(&s_cnt[RANGE_VALID], nv);
      atomicMax(&s_cnt[RANGE_MIN], kmin_c);
      atomicMax(&s_cnt[RANGE_MAX], kmax);
    }
  }
  __syncthreads();
  if (threadIdx.x < RF_FACET_MAX_RANGES + 2) {
    const unsigned long long v = s_cnt[threadIdx.x];
    if (v) atomicAdd(&P.out[threadIdx.x], v);
  } else if (threadIdx.x < RF_FACET_MAX_RANGES + 4 && s_cnt[RANGE_VALID]) {
    atomicMax(&P.out[threadIdx.x], s_cnt[threadIdx.x]);
  }
}

// keys back to the values' own bits
__global__ void k_facet_ranges_finish(unsigned long long* out, int is_f64) {
  if (threadIdx.x != 0 || out[RANGE_VALID] == 0ull) return;
  const unsigned long long kmin = ~out[RANGE_MIN], kmax = out[RANGE_MAX];
  if (is_f64) {
    out[RANGE_MIN] = (kmin >> 63) ? kmin ^ (1ull << 63) : ~kmin;
    out[RANGE_MAX] = (kmax >> 63) ? kmax ^ (1ull << 63) : ~kmax;
  } else {
    out[RANGE_MIN] = kmin ^ (1ull << 63);
    out[RANGE_MAX] = kmax ^ (1ull << 63);
  }
}

extern "C" int rf_facet_ranges(const void* filter_dev, const void* column_dev, int is_f64,
                               const rf_facet_range* ranges_host, int n_ranges, int64_t n_rows, int64_t* out_dev,
                               void* stream) {
  static const char* fn = "rf_facet_ranges";
  if (!ranges_host || n_ranges < 1 || n_ranges > RF_FACET_MAX_RANGES) {
    rf_set_error("%s: null ranges, or n_ranges = %d outside 1..%d", fn, n_ranges, RF_FACET_MAX_RANGES);
    return RF_ERR_INVALID;
  }
  if (!out_dev || (((uintptr_t)out_dev) & 7) || (((uintptr_t)column_dev) & 7) || (!column_dev && n_rows > 0)) {
    rf_set_error("%s: out_dev or the column is null or not 8-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  int rc = check_rows(fn, n_rows, filter_dev);
  if (rc != RF_OK) return rc;
  RangeArgs P{};
  for (int r = 0; r < n_ranges; ++r) {
    if (ranges_host[r].flags & ~(RF_FRANGE_NO_LO | RF_FRANGE_NO_HI | RF_FRANGE_EMPTY)) {
      rf_set_error("%s: range %d: unknown flags %d", fn, r, ranges_host[r].flags);
      return RF_ERR_INVALID;
    }
    P.r[r] = ranges_host[r];
  }
  hipStream_t st = (hipStream_t)stream;
  RF_HIP(hipMemsetAsync(out_dev, 0, (size_t)(RF_FACET_MAX_RANGES + 4) * 8, st));
  if (n_rows == 0) return RF_OK;
  P.W = make_walk(filter_dev, n_rows);
  P.column = column_dev;
  P.out = (unsigned long long*)out_dev;
  P.n_ranges = n_ranges;
  P.is_f64 = is_f64 ? 1 : 0;
  hipLaunchKernelGGL(k_facet_ranges, dim3(facet_grid(n_rows, 2 * FACET_WAVES)), dim3(FACET_THREADS), 0, st, P);
  RF_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_facet_ranges_finish, dim3(1), dim3(64), 0, st, (unsigned long long*)out_dev, P.is_f64);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
