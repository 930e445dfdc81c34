// Dynamic fields: the leaves of a filter expression over schemaless metadata, evaluated into one row bitmap
// per leaf (include/ragfin.h, "dynamic fields").  A key's device mirror is a tagged column: a
// uint8 tag per row (absent | bool | int | double | string) and 8 bytes of payload.  rf_filter_eval_bitmaps
// (filter.hip) reads the bitmaps through RF_FOP_BITMAP leaves, as it reads rf_text_match's and
// rf_column_match's.
//
//   k_dynamic_match  grid (row chunks, leaves): a lane owns one row of a 256-row chunk, loads its tag byte
//                    (64 consecutive bytes per wave) and, where the leaf's kind names that tag, its 8-byte
//                    payload; a wave ballots its 64 predicates into two mask words.  A workgroup strides over
//                    the chunks, so a large collection costs a bounded number of workgroups per leaf.
// Integers and IEEE comparisons only, every word written exactly once: the same bitmap on every run.
#include "rf_internal.h"

#define DYNAMIC_THREADS 256
#define DYNAMIC_MAX_GRID 1024   // workgroups per leaf; the rest of the chunks are strided over

struct DynamicArgs {
  rf_dynamic_leaf leaves[RF_DYNAMIC_MAX_LEAVES];
  const uint32_t* code_sets;
  const int64_t* int_sets;
  const double* f64_sets;
  uint32_t* bitmaps;
  int64_t n_rows, nwords, n_chunks;
};

// x is in the sorted slice S[0 .. n): lower bound, then one equality test (never reads outside the slice)
template <typename T>
__device__ __forceinline__ bool sorted_has(const T* S, int64_t len, T x) {
  int64_t lo = 0, n = len;
  while (n > 0) {
    const int64_t half = n >> 1;
    if (S[lo + half] < x) {   // (a NaN x: never true, lo stays 0 and the equality fails)
      lo += half + 1;
      n -= half + 1;
    } else {
      n = half;
    }
  }
  return lo < len && S[lo] == x;
}

__device__ __forceinline__ bool dynamic_pass(const DynamicArgs& P, const rf_dynamic_leaf& L, int64_t row) {
  const uint32_t tag = L.tags_dev[row];
  switch (L.kind) {   // (wave-uniform: the leaf comes from the kernel arguments)
    case RF_DLEAF_TAGS:
      return tag < 8u && (((uint32_t)L.flags >> tag) & 1u) != 0u;
    case RF_DLEAF_STR_CODESET: {
      if (tag != RF_DTAG_STRING) return false;
      const uint64_t c = ((const uint64_t*)L.payload_dev)[row];   // (a negative code wraps past 32 len)
      return c < 32ull * (uint64_t)L.len && ((P.code_sets[L.off + (int64_t)(c >> 5)] >> (uint32_t)(c & 31ull)) & 1u) != 0u;
    }
    case RF_DLEAF_BOOL: {
      if (tag != RF_DTAG_BOOL) return false;
      const uint64_t v = ((const uint64_t*)L.payload_dev)[row];
      return v < 2ull && (((uint32_t)L.flags >> (uint32_t)v) & 1u) != 0u;
    }
    case RF_DLEAF_NUM_RANGE: {
      if (tag == RF_DTAG_INT) {
        const int64_t x = ((const int64_t*)L.payload_dev)[row];
        return x >= L.ilo && x <= L.ihi;
      }
      if (tag != RF_DTAG_DOUBLE) return false;
      const double x = ((const double*)L.payload_dev)[row];
      const bool a = (L.flags & RF_FRANGE_LO_INCL) ? x >= L.flo : x > L.flo;
      const bool b = (L.flags & RF_FRANGE_HI_INCL) ? x <= L.fhi : x < L.fhi;
      return a && b;   // NaN fails both
    }
    default: {   // RF_DLEAF_NUM_SET
      if (tag == RF_DTAG_INT) return sorted_has(P.int_sets + L.off, L.len, ((const int64_t*)L.payload_dev)[row]);
      if (tag != RF_DTAG_DOUBLE) return false;
      return sorted_has(P.f64_sets + L.foff, L.flen, ((const double*)L.payload_dev)[row]);
    }
  }
}

__global__ void __launch_bounds__(DYNAMIC_THREADS) k_dynamic_match(DynamicArgs P) {
  const rf_dynamic_leaf& L = P.leaves[blockIdx.y];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t* out = P.bitmaps + (size_t)blockIdx.y * (size_t)P.nwords;
  for (int64_t chunk = blockIdx.x; chunk < P.n_chunks; chunk += gridDim.x) {   // (uniform over the workgroup)
    const int64_t row = chunk * DYNAMIC_THREADS + (int64_t)threadIdx.x;
    const bool pass = row < P.n_rows && dynamic_pass(P, L, row);
    const unsigned long long b = __ballot(pass);   // bits past n_rows are zero
    const int64_t w = ((row - (int64_t)lane) >> 5) + (int64_t)lane;   // lanes 0 and 1: the wave's two words
    if (lane < 2u && w < P.nwords) out[w] = lane == 0u ? (uint32_t)b : (uint32_t)(b >> 32);
  }
}

static bool bad_slice(int64_t off, int64_t len, int64_t max_len) {
  return off < 0 || len < 0 || len > max_len;
}

extern "C" int rf_dynamic_match(const rf_dynamic_leaf* leaves_host, int n_leaves, const uint32_t* code_sets_dev,
                                const int64_t* int_sets_dev, const double* f64_sets_dev, int64_t n_rows,
                                uint32_t* bitmaps_dev, void* stream) {
  static const char* fn = "rf_dynamic_match";
  if (!leaves_host || !bitmaps_dev) {
    rf_set_error("%s: null argument", fn);
    return RF_ERR_INVALID;
  }
  if (n_leaves < 1 || n_leaves > RF_DYNAMIC_MAX_LEAVES) {
    rf_set_error("%s: n_leaves = %d outside 1..%d", fn, n_leaves, RF_DYNAMIC_MAX_LEAVES);
    return RF_ERR_INVALID;
  }
  if (n_rows < 0 || n_rows > (int64_t)0xFFFFFFFFll - 32) {   // the row range of a filter buffer
    rf_set_error("%s: n_rows = %lld out of range", fn, (long long)n_rows);
    return RF_ERR_INVALID;
  }
  if ((((uintptr_t)bitmaps_dev) & 3) || (((uintptr_t)code_sets_dev) & 3) || (((uintptr_t)int_sets_dev) & 7) ||
      (((uintptr_t)f64_sets_dev) & 7)) {
    rf_set_error("%s: bitmaps and code sets must be 4-byte aligned, value sets 8-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  DynamicArgs P{};
  for (int l = 0; l < n_leaves; ++l) {
    const rf_dynamic_leaf& L = leaves_host[l];
    int flag_bits = 0;
    switch (L.kind) {
      case RF_DLEAF_TAGS:
        flag_bits = 0xFF;
        break;
      case RF_DLEAF_STR_CODESET:
        // (a row reads word off + (code >> 5) only for a code below 32 len: inside [off, off + len))
        if (bad_slice(L.off, L.len, (int64_t)1 << 26) || (L.len > 0 && !code_sets_dev)) {
          rf_set_error("%s: leaf %d: bad code-set leaf (off %lld, len %lld)", fn, l, (long long)L.off, (long long)L.len);
          return RF_ERR_INVALID;
        }
        break;
      case RF_DLEAF_BOOL:
        flag_bits = 3;
        break;
      case RF_DLEAF_NUM_RANGE:
        flag_bits = RF_FRANGE_LO_INCL | RF_FRANGE_HI_INCL;
        break;
      case RF_DLEAF_NUM_SET:
        if (bad_slice(L.off, L.len, RF_COLUMN_MAX_SET) || bad_slice(L.foff, L.flen, RF_COLUMN_MAX_SET) ||
            (L.len > 0 && !int_sets_dev) || (L.flen > 0 && !f64_sets_dev)) {
          rf_set_error("%s: leaf %d: bad value-set leaf (off %lld, len %lld, foff %lld, flen %lld, at most %d values)", fn,
                       l, (long long)L.off, (long long)L.len, (long long)L.foff, (long long)L.flen, RF_COLUMN_MAX_SET);
          return RF_ERR_INVALID;
        }
        break;
      default:
        rf_set_error("%s: leaf %d: unknown kind %d", fn, l, L.kind);
        return RF_ERR_INVALID;
    }
    if (L.flags & ~flag_bits) {
      rf_set_error("%s: leaf %d: flags %d outside the bits of kind %d", fn, l, L.flags, L.kind);
      return RF_ERR_INVALID;
    }
    if (n_rows > 0 && (!L.tags_dev || (L.kind != RF_DLEAF_TAGS && !L.payload_dev) || (((uintptr_t)L.payload_dev) & 7))) {
      rf_set_error("%s: leaf %d: the tags or the payload are null, or the payload is not 8-byte aligned", fn, l);
      return RF_ERR_INVALID;
    }
    P.leaves[l] = L;
  }
  if (n_rows == 0) return RF_OK;   // no word to write
  P.code_sets = code_sets_dev;
  P.int_sets = int_sets_dev;
  P.f64_sets = f64_sets_dev;
  P.bitmaps = bitmaps_dev;
  P.n_rows = n_rows;
  P.nwords = (n_rows + 31) / 32;
  P.n_chunks = (n_rows + DYNAMIC_THREADS - 1) / DYNAMIC_THREADS;
  const uint32_t grid = (uint32_t)(P.n_chunks < DYNAMIC_MAX_GRID ? P.n_chunks : DYNAMIC_MAX_GRID);
  hipLaunchKernelGGL(k_dynamic_match, dim3(grid, (uint32_t)n_leaves), dim3(DYNAMIC_THREADS), 0, (hipStream_t)stream, P);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
