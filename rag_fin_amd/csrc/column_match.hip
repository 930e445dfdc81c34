// User-defined scalar fields: the leaves of a filter expression over a collection's extra columns,
// evaluated into one row bitmap per leaf (include/ragfin.h, "user-defined scalar fields").
// rf_filter_eval_bitmaps (filter.hip) reads the bitmaps through RF_FOP_BITMAP leaves, as it reads
// rf_text_match's.
//
//   k_column_match  grid (row chunks, leaves): a lane owns one row of a 256-row chunk, loads its 4- or
//                   8-byte column value (coalesced) and tests it; a wave ballots its 64 predicates into
//                   two mask words.  A workgroup strides over the chunks, so a large collection costs a
//                   bounded number of workgroups per leaf.
// Integers and IEEE comparisons only, every word written exactly once: the same bitmap on every run.
#include "rf_internal.h"

#define COLUMN_THREADS 256
#define COLUMN_MAX_GRID 1024   // workgroups per leaf; the rest of the chunks are strided over

struct ColumnArgs {
  rf_column_leaf leaves[RF_COLUMN_MAX_LEAVES];
  const uint32_t* code_sets;
  const int64_t* value_sets;
  uint32_t* bitmaps;
  int64_t n_rows, nwords, n_chunks;
};

__device__ __forceinline__ bool column_pass(const ColumnArgs& P, const rf_column_leaf& L, int64_t row) {
  switch (L.kind) {   // (wave-uniform: the leaf comes from the kernel arguments)
    case RF_CLEAF_CODESET: {
      const uint32_t c = (uint32_t)((const int32_t*)L.column_dev)[row];   // (a negative code wraps past 32 len)
      return (uint64_t)c < 32ull * (uint64_t)L.len && ((P.code_sets[L.off + (c >> 5)] >> (c & 31u)) & 1u) != 0u;
    }
    case RF_CLEAF_I64_RANGE: {
      const int64_t x = ((const int64_t*)L.column_dev)[row];
      return x >= L.ilo && x <= L.ihi;
    }
    case RF_CLEAF_I64_SET: {
      const int64_t x = ((const int64_t*)L.column_dev)[row];
      const int64_t* S = P.value_sets + L.off;
      int64_t lo = 0, n = L.len;   // lower bound of x in the sorted slice
      while (n > 0) {
        const int64_t half = n >> 1;
        if (S[lo + half] < x) {
          lo += half + 1;
          n -= half + 1;
        } else {
          n = half;
        }
      }
      return lo < L.len && S[lo] == x;
    }
    default: {   // RF_CLEAF_F64_RANGE
      const double x = ((const double*)L.column_dev)[row];
      const bool a = (L.flags & RF_FRANGE_LO_INCL) ? x >= L.flo : x > L.flo;
      const bool b = (L.flags & RF_FRANGE_HI_INCL) ? x <= L.fhi : x < L.fhi;
      return a && b;   // NaN fails both
    }
  }
}

__global__ void __launch_bounds__(COLUMN_THREADS) k_column_match(ColumnArgs P) {
  const rf_column_leaf& L = P.leaves[blockIdx.y];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t* out = P.bitmaps + (size_t)blockIdx.y * (size_t)P.nwords;
  for (int64_t chunk = blockIdx.x; chunk < P.n_chunks; chunk += gridDim.x) {   // (uniform over the workgroup)
    const int64_t row = chunk * COLUMN_THREADS + (int64_t)threadIdx.x;
    const bool pass = row < P.n_rows && column_pass(P, L, row);
    const unsigned long long b = __ballot(pass);   // bits past n_rows are zero
    const int64_t w = ((row - (int64_t)lane) >> 5) + (int64_t)lane;   // lanes 0 and 1: the wave's two words
    if (lane < 2u && w < P.nwords) out[w] = lane == 0u ? (uint32_t)b : (uint32_t)(b >> 32);
  }
}

extern "C" int rf_column_match(const rf_column_leaf* leaves_host, int n_leaves, const uint32_t* code_sets_dev,
                               const int64_t* value_sets_dev, int64_t n_rows, uint32_t* bitmaps_dev, void* stream) {
  static const char* fn = "rf_column_match";
  if (!leaves_host || !bitmaps_dev) {
    rf_set_error("%s: null argument", fn);
    return RF_ERR_INVALID;
  }
  if (n_leaves < 1 || n_leaves > RF_COLUMN_MAX_LEAVES) {
    rf_set_error("%s: n_leaves = %d outside 1..%d", fn, n_leaves, RF_COLUMN_MAX_LEAVES);
    return RF_ERR_INVALID;
  }
  if (n_rows < 0 || n_rows > (int64_t)0xFFFFFFFFll - 32) {   // the row range of a filter buffer
    rf_set_error("%s: n_rows = %lld out of range", fn, (long long)n_rows);
    return RF_ERR_INVALID;
  }
  if ((((uintptr_t)bitmaps_dev) & 3) || (((uintptr_t)code_sets_dev) & 3) || (((uintptr_t)value_sets_dev) & 7)) {
    rf_set_error("%s: bitmaps and code sets must be 4-byte aligned, value sets 8-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  ColumnArgs P{};
  for (int l = 0; l < n_leaves; ++l) {
    const rf_column_leaf& L = leaves_host[l];
    uintptr_t align = 7;
    switch (L.kind) {
      case RF_CLEAF_CODESET:
        // (a row reads word off + (code >> 5) only for a code below 32 len: inside [off, off + len))
        if (L.off < 0 || L.len < 0 || L.len > (int64_t)1 << 26 || (L.len > 0 && !code_sets_dev)) {
          rf_set_error("%s: leaf %d: bad code-set leaf (off %lld, len %lld)", fn, l, (long long)L.off, (long long)L.len);
          return RF_ERR_INVALID;
        }
        align = 3;
        break;
      case RF_CLEAF_I64_SET:
        if (L.off < 0 || L.len < 0 || L.len > RF_COLUMN_MAX_SET || (L.len > 0 && !value_sets_dev)) {
          rf_set_error("%s: leaf %d: bad value-set leaf (off %lld, len %lld, at most %d values)", fn, l,
                       (long long)L.off, (long long)L.len, RF_COLUMN_MAX_SET);
          return RF_ERR_INVALID;
        }
        break;
      case RF_CLEAF_I64_RANGE:
        break;
      case RF_CLEAF_F64_RANGE:
        if (L.flags & ~(RF_FRANGE_LO_INCL | RF_FRANGE_HI_INCL)) {
          rf_set_error("%s: leaf %d: unknown range flags %d", fn, l, L.flags);
          return RF_ERR_INVALID;
        }
        break;
      default:
        rf_set_error("%s: leaf %d: unknown kind %d", fn, l, L.kind);
        return RF_ERR_INVALID;
    }
    if (n_rows > 0 && (!L.column_dev || (((uintptr_t)L.column_dev) & align))) {
      rf_set_error("%s: leaf %d: the column is null or not aligned to its element size", fn, l);
      return RF_ERR_INVALID;
    }
    P.leaves[l] = L;
  }
  if (n_rows == 0) return RF_OK;   // no word to write
  P.code_sets = code_sets_dev;
  P.value_sets = value_sets_dev;
  P.bitmaps = bitmaps_dev;
  P.n_rows = n_rows;
  P.nwords = (n_rows + 31) / 32;
  P.n_chunks = (n_rows + COLUMN_THREADS - 1) / COLUMN_THREADS;
  const uint32_t grid = (uint32_t)(P.n_chunks < COLUMN_MAX_GRID ? P.n_chunks : COLUMN_MAX_GRID);
  hipLaunchKernelGGL(k_column_match, dim3(grid, (uint32_t)n_leaves), dim3(COLUMN_THREADS), 0, (hipStream_t)stream, P);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
