// ARRAY fields: the leaves of a filter expression over a collection's multi-valued columns, evaluated
// into one row bitmap per leaf (include/ragfin.h, "ARRAY fields").  rf_filter_eval_bitmaps
// (filter.hip) reads the bitmaps through RF_FOP_BITMAP leaves, as it reads rf_column_match's.
//
// A field is CSR on the device: offsets int64 [n_rows + 1], values back to back.
//   k_array_match  grid (row chunks, leaves), 4 waves of 64 rows per 256-row chunk.
//     LENGTH, ELEM  a lane owns one row: two offset loads, at most one element load, a scalar test.
//     MATCH         a wave owns 64 consecutive rows: the lanes stage the 65 offsets in the wave's slice of
//                   LDS, stride over the rows' one contiguous element span (coalesced), look each element
//                   up in the sorted needle slice and, on a hit only, find the owning row by binary search
//                   over the staged offsets and OR the needle's bit into the row's 64-bit LDS slot.  One
//                   4096-element row is 64 trips of the whole wave, not 4096 of one lane.
// The LDS OR is commutative and idempotent, every output word is written exactly once, and there is no
// global atomic: the same bitmap on every run.
#include "rf_internal.h"

#define ARRAY_THREADS 256
#define ARRAY_WAVES (ARRAY_THREADS / 64)
#define ARRAY_MAX_GRID 1024   // workgroups per leaf; the rest of the chunks are strided over

struct ArrayArgs {
  rf_array_leaf leaves[RF_ARRAY_MAX_LEAVES];
  const uint32_t* code_sets;
  const int64_t* value_sets;
  const double* f64_sets;
  uint32_t* bitmaps;
  int64_t n_rows, nwords, n_chunks;
};

// the position of x in the sorted slice S[0 .. n), or -1: lower bound by `<`, then `==` (a NaN x is below
// nothing and equals nothing)
template <typename T>
__device__ __forceinline__ int64_t needle_position(const T* S, int64_t len, T x) {
  int64_t lo = 0, n = len;
  while (n > 0) {
    const int64_t half = n >> 1;
    if (S[lo + half] < x) {
      lo += half + 1;
      n -= half + 1;
    } else {
      n = half;
    }
  }
  return (lo < len && S[lo] == x) ? lo : -1;
}

// the scalar tests of rf_column_match (column_match.hip, column_pass), on element e of the values
__device__ __forceinline__ bool elem_pass(const ArrayArgs& P, const rf_array_leaf& L, int64_t e) {
  switch (L.elem) {   // (wave-uniform: the leaf comes from the kernel arguments)
    case RF_CLEAF_CODESET: {
      const uint32_t c = (uint32_t)((const int32_t*)L.values_dev)[e];   // (a negative code wraps past 32 len)
      return (uint64_t)c < 32ull * (uint64_t)L.len && ((P.code_sets[L.off + (c >> 5)] >> (c & 31u)) & 1u) != 0u;
    }
    case RF_CLEAF_I64_RANGE: {
      const int64_t x = ((const int64_t*)L.values_dev)[e];
      return x >= L.ilo && x <= L.ihi;
    }
    case RF_CLEAF_I64_SET:
      return needle_position(P.value_sets + L.off, L.len, ((const int64_t*)L.values_dev)[e]) >= 0;
    default: {   // RF_CLEAF_F64_RANGE
      const double x = ((const double*)L.values_dev)[e];
      const bool a = (L.flags & RF_FRANGE_LO_INCL) ? x >= L.flo : x > L.flo;
      const bool b = (L.flags & RF_FRANGE_HI_INCL) ? x <= L.fhi : x < L.fhi;
      return a && b;   // NaN fails both
    }
  }
}

__global__ void __launch_bounds__(ARRAY_THREADS) k_array_match(ArrayArgs P) {
  __shared__ int64_t s_off[ARRAY_WAVES][65];              // the wave's 64 rows' offsets, and the end of the last
  __shared__ unsigned long long s_slot[ARRAY_WAVES][64];  // per row: the needles seen so far, one bit each
  const rf_array_leaf& L = P.leaves[blockIdx.y];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = threadIdx.x >> 6;
  const int64_t* off = L.offsets_dev;
  uint32_t* out = P.bitmaps + (size_t)blockIdx.y * (size_t)P.nwords;
  for (int64_t chunk = blockIdx.x; chunk < P.n_chunks; chunk += gridDim.x) {   // (uniform over the workgroup)
    const int64_t r0 = chunk * ARRAY_THREADS + (int64_t)wave * 64;
    const int64_t row = r0 + (int64_t)lane;
    bool pass = false;
    if (L.kind == RF_ALEAF_MATCH) {   // (uniform over the grid row: the barriers below are legal)
      // rows past n_rows read offsets[n_rows]: they are empty, and no index leaves [0, n_rows]
      s_off[wave][lane] = off[row < P.n_rows ? row : P.n_rows];
      if (lane == 0u) s_off[wave][64] = off[r0 + 64 < P.n_rows ? r0 + 64 : P.n_rows];
      s_slot[wave][lane] = 0ull;
      __syncthreads();
      const int64_t e1 = s_off[wave][64];
      for (int64_t e = s_off[wave][0] + (int64_t)lane; e < e1; e += 64) {   // (trip count per wave: no barrier inside)
        int64_t pos;
        if (L.elem == RF_AELEM_F64)
          pos = needle_position(P.f64_sets + L.off, L.len, ((const double*)L.values_dev)[e]);
        else if (L.elem == RF_AELEM_I64)
          pos = needle_position(P.value_sets + L.off, L.len, ((const int64_t*)L.values_dev)[e]);
        else
          pos = needle_position(P.value_sets + L.off, L.len, (int64_t)((const int32_t*)L.values_dev)[e]);
        if (pos >= 0) {
          // the owner: the largest r with off[r] <= e.  s_off[0] <= e < s_off[64], and a run of empty rows
          // before the owner shares its offset, so the upper bound minus one lands on the non-empty row
          int lo = 0, n = 64;   // first index in [0, 64) whose offset is above e (64: none)
          while (n > 0) {
            const int half = n >> 1;
            if (s_off[wave][lo + half] <= e) {
              lo += half + 1;
              n -= half + 1;
            } else {
              n = half;
            }
          }
          atomicOr(&s_slot[wave][lo > 0 ? lo - 1 : 0], L.need == 1 ? 1ull : 1ull << pos);   // (need > 1: len <= 64, pos < 64)
        }
      }
      __syncthreads();
      pass = row < P.n_rows && __popcll(s_slot[wave][lane]) >= L.need;
    } else if (row < P.n_rows) {
      const int64_t o0 = off[row], len = off[row + 1] - o0;
      if (L.kind == RF_ALEAF_LENGTH)
        pass = len >= L.ilo && len <= L.ihi;
      else
        pass = L.index < len && elem_pass(P, L, o0 + L.index);
    }
    const unsigned long long b = __ballot(pass);   // bits past n_rows are zero
    const int64_t w = (r0 >> 5) + (int64_t)lane;   // lanes 0 and 1: the wave's two words
    if (lane < 2u && w < P.nwords) out[w] = lane == 0u ? (uint32_t)b : (uint32_t)(b >> 32);
  }
}

extern "C" int rf_array_match(const rf_array_leaf* leaves_host, int n_leaves, const uint32_t* code_sets_dev,
                              const int64_t* value_sets_dev, const double* f64_sets_dev, int64_t n_rows,
                              uint32_t* bitmaps_dev, void* stream) {
  static const char* fn = "rf_array_match";
  if (!leaves_host || !bitmaps_dev) {
    rf_set_error("%s: null argument", fn);
    return RF_ERR_INVALID;
  }
  if (n_leaves < 1 || n_leaves > RF_ARRAY_MAX_LEAVES) {
    rf_set_error("%s: n_leaves = %d outside 1..%d", fn, n_leaves, RF_ARRAY_MAX_LEAVES);
    return RF_ERR_INVALID;
  }
  if (n_rows < 0 || n_rows > (int64_t)0xFFFFFFFFll - 32) {   // the row range of a filter buffer
    rf_set_error("%s: n_rows = %lld out of range", fn, (long long)n_rows);
    return RF_ERR_INVALID;
  }
  if ((((uintptr_t)bitmaps_dev) & 3) || (((uintptr_t)code_sets_dev) & 3) || (((uintptr_t)value_sets_dev) & 7) ||
      (((uintptr_t)f64_sets_dev) & 7)) {
    rf_set_error("%s: bitmaps and code sets must be 4-byte aligned, value sets 8-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  ArrayArgs P{};
  for (int l = 0; l < n_leaves; ++l) {
    const rf_array_leaf& L = leaves_host[l];
    uintptr_t align = 7;
    if (L.off < 0 || L.len < 0 || L.index < 0) {
      rf_set_error("%s: leaf %d: negative off, len or index (%lld, %lld, %lld)", fn, l, (long long)L.off,
                   (long long)L.len, (long long)L.index);
      return RF_ERR_INVALID;
    }
    switch (L.kind) {
      case RF_ALEAF_LENGTH:
        break;
      case RF_ALEAF_ELEM:
        switch (L.elem) {
          case RF_CLEAF_CODESET:
            // (an element reads word off + (code >> 5) only for a code below 32 len: inside [off, off + len))
            if (L.len > (int64_t)1 << 26 || (L.len > 0 && !code_sets_dev)) {
              rf_set_error("%s: leaf %d: bad code-set leaf (off %lld, len %lld)", fn, l, (long long)L.off, (long long)L.len);
              return RF_ERR_INVALID;
            }
            align = 3;
            break;
          case RF_CLEAF_I64_SET:
            if (L.len > RF_COLUMN_MAX_SET || (L.len > 0 && !value_sets_dev)) {
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
            rf_set_error("%s: leaf %d: unknown element test %d", fn, l, L.elem);
            return RF_ERR_INVALID;
        }
        break;
      case RF_ALEAF_MATCH:
        if (L.elem != RF_AELEM_CODE && L.elem != RF_AELEM_I64 && L.elem != RF_AELEM_F64) {
          rf_set_error("%s: leaf %d: unknown element type %d", fn, l, L.elem);
          return RF_ERR_INVALID;
        }
        if (L.len > RF_COLUMN_MAX_SET || (L.need != 1 && (int64_t)L.need != L.len) || L.need < 0 || L.need > 64) {
          rf_set_error("%s: leaf %d: bad needle slice (len %lld, at most %d; need %d must be 1 or len, at most 64)", fn,
                       l, (long long)L.len, RF_COLUMN_MAX_SET, L.need);
          return RF_ERR_INVALID;
        }
        if (L.len > 0 && !(L.elem == RF_AELEM_F64 ? (const void*)f64_sets_dev : (const void*)value_sets_dev)) {
          rf_set_error("%s: leaf %d: the needle set is null", fn, l);
          return RF_ERR_INVALID;
        }
        if (L.elem == RF_AELEM_CODE) align = 3;
        break;
      default:
        rf_set_error("%s: leaf %d: unknown kind %d", fn, l, L.kind);
        return RF_ERR_INVALID;
    }
    if (!L.offsets_dev || (((uintptr_t)L.offsets_dev) & 7)) {
      rf_set_error("%s: leaf %d: the offsets are null or not 8-byte aligned", fn, l);
      return RF_ERR_INVALID;
    }
    if (L.kind != RF_ALEAF_LENGTH && (!L.values_dev || (((uintptr_t)L.values_dev) & align))) {
      rf_set_error("%s: leaf %d: the values are null or not aligned to their element size", fn, l);
      return RF_ERR_INVALID;
    }
    P.leaves[l] = L;
  }
  if (n_rows == 0) return RF_OK;   // no word to write
  P.code_sets = code_sets_dev;
  P.value_sets = value_sets_dev;
  P.f64_sets = f64_sets_dev;
  P.bitmaps = bitmaps_dev;
  P.n_rows = n_rows;
  P.nwords = (n_rows + 31) / 32;
  P.n_chunks = (n_rows + ARRAY_THREADS - 1) / ARRAY_THREADS;
  const uint32_t grid = (uint32_t)(P.n_chunks < ARRAY_MAX_GRID ? P.n_chunks : ARRAY_MAX_GRID);
  hipLaunchKernelGGL(k_array_match, dim3(grid, (uint32_t)n_leaves), dim3(ARRAY_THREADS), 0, (hipStream_t)stream, P);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
