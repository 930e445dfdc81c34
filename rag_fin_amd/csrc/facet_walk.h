// What the facet kernels share (facets.hip, facet_stats.hip): the walk over the 32-row blocks a filter
// passes, and the units of a value field -- which (row, bin) pairs a passing block contributes, by the
// CODES / ARRAY / DYNAMIC rules of include/ragfin.h, "faceted counts".
#pragma once
#include "rf_internal.h"

#define FACET_THREADS 256
#define FACET_WAVES (FACET_THREADS / 64)
#define FACET_MAX_GRID 512

// ---- the rows a filter passes, block by block ----------------------------------------------------
struct FilterWalk {
  const uint32_t* hdr;      // null: no filter, every row passes
  const uint32_t* mask;
  const uint32_t* blocks;
  uint32_t n_rows, nblk;
};

static inline FilterWalk make_walk(const void* filter_dev, int64_t n_rows) {
  FilterWalk W{};
  if (filter_dev) {
    const rf_filter_view v = rf_filter_carve(filter_dev, n_rows);
    W.hdr = v.hdr;
    W.mask = v.mask;
    W.blocks = v.blocks;
  }
  W.n_rows = (uint32_t)n_rows;
  W.nblk = (uint32_t)((n_rows + 31) / 32);
  return W;
}

// passing blocks (a filter built for another row count passes nothing)
__device__ __forceinline__ uint32_t walk_count(const FilterWalk& W) {
  if (!W.hdr) return W.nblk;
  return W.hdr[0] == W.n_rows ? min(W.hdr[2], W.nblk) : 0u;
}

__device__ __forceinline__ uint32_t walk_block(const FilterWalk& W, uint32_t j) { return W.hdr ? W.blocks[j] : j; }

// the passing rows of block b, bits past n_rows zero; a block number outside the rows passes nothing
__device__ __forceinline__ uint32_t walk_mask(const FilterWalk& W, uint32_t b) {
  if (b >= W.nblk) return 0u;
  uint32_t m = W.hdr ? W.mask[b] : 0xFFFFFFFFu;
  const uint32_t rows = W.n_rows - b * 32u;   // > 0
  if (rows < 32u) m &= (1u << rows) - 1u;
  return m;
}

static inline uint32_t facet_grid(int64_t n_rows, uint32_t blocks_per_wg) {
  const int64_t nblk = (n_rows + 31) / 32;
  const int64_t g = (nblk + blocks_per_wg - 1) / blocks_per_wg;
  return (uint32_t)(g < 1 ? 1 : g > FACET_MAX_GRID ? FACET_MAX_GRID : g);
}

// ---- the host-side checks of the entry points ------------------------------------------------------
static inline uint32_t facet_bins(const rf_facet_field& F) {
  return (uint32_t)F.n_codes + (F.kind == RF_FACET_DYNAMIC ? 2u : 0u);
}

static inline int check_fields(const char* fn, const rf_facet_field* fields_host, int n_fields, int64_t n_counters,
                        bool need_columns, bool need_rank) {
  if (!fields_host || n_fields < 1 || n_fields > RF_FACET_MAX_FIELDS) {
    rf_set_error("%s: null fields, or n_fields = %d outside 1..%d", fn, n_fields, RF_FACET_MAX_FIELDS);
    return RF_ERR_INVALID;
  }
  for (int i = 0; i < n_fields; ++i) {
    const rf_facet_field& F = fields_host[i];
    if (F.kind != RF_FACET_CODES && F.kind != RF_FACET_ARRAY && F.kind != RF_FACET_DYNAMIC) {
      rf_set_error("%s: field %d: unknown kind %d", fn, i, F.kind);
      return RF_ERR_INVALID;
    }
    if (F.n_codes < 0 || F.n_codes > 0x7FFFFFF0) {
      rf_set_error("%s: field %d: n_codes = %d out of range", fn, i, F.n_codes);
      return RF_ERR_INVALID;
    }
    const int64_t bins = (int64_t)facet_bins(F) + 1;
    if (F.counter_off < 0 || F.counter_off > n_counters || bins > n_counters - F.counter_off) {
      rf_set_error("%s: field %d: counters [%lld, %lld) lie outside the %lld given", fn, i, (long long)F.counter_off,
                   (long long)(F.counter_off + bins), (long long)n_counters);
      return RF_ERR_INVALID;
    }
    if (need_columns) {
      const uintptr_t a_align = F.kind == RF_FACET_CODES ? 3 : F.kind == RF_FACET_ARRAY ? 7 : 0;
      const uintptr_t b_align = F.kind == RF_FACET_ARRAY ? 3 : 7;
      if (!F.a_dev || (((uintptr_t)F.a_dev) & a_align) ||
          (F.kind != RF_FACET_CODES && (!F.b_dev || (((uintptr_t)F.b_dev) & b_align))) ||
          (F.kind == RF_FACET_ARRAY && !F.c_dev)) {
        rf_set_error("%s: field %d: a column is null or not aligned to its element size", fn, i);
        return RF_ERR_INVALID;
      }
    }
    if (need_rank && facet_bins(F) > 0 && (!F.rank_dev || (((uintptr_t)F.rank_dev) & 3))) {
      rf_set_error("%s: field %d: rank_dev is null or not 4-byte aligned", fn, i);
      return RF_ERR_INVALID;
    }
  }
  return RF_OK;
}

static inline int check_rows(const char* fn, int64_t n_rows, const void* filter_dev) {
  if (n_rows < 0 || n_rows > (int64_t)0xFFFFFFFFll - 32) {   // the row range of a filter buffer
    rf_set_error("%s: n_rows = %lld out of range", fn, (long long)n_rows);
    return RF_ERR_INVALID;
  }
  if (((uintptr_t)filter_dev) & 15) {
    rf_set_error("%s: filter buffer must be 16-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  return RF_OK;
}

// ---- the units of a value field ------------------------------------------------------------------------
// The units of step `it` of field F's work list (a wave takes one passing block of an ARRAY field per step,
// two of a scalar one).  Called by all 64 lanes of a wave together; emit(active,
// bin, row) is called by all of them together too, once for a scalar field and once per 64 elements (and
// once for the rows without elements) of an ARRAY field.  bin == n_bins is `missing`; an active lane's bin
// is in [0, n_bins] and its row passes the filter.
template <typename Emit>
__device__ __forceinline__ void facet_units(const rf_facet_field& F, const FilterWalk& W, uint32_t it, uint32_t npass,
                                            uint32_t lane, uint32_t n_codes, uint32_t n_bins, Emit emit) {
  if (F.kind == RF_FACET_ARRAY) {
    const int64_t* off = (const int64_t*)F.a_dev;
    const int32_t* vals = (const int32_t*)F.b_dev;
    const uint8_t* first = (const uint8_t*)F.c_dev;
    const uint32_t b = walk_block(W, it);
    const uint32_t m = walk_mask(W, b);   // (0 for a block outside the rows: nothing below reads then)
    const int64_t r0 = (int64_t)b * 32;
    // lane l <= 32 holds offsets[r0 + l] (rows past n_rows: offsets[n_rows], they are empty)
    int64_t at = r0 + (int64_t)min(lane, 32u);
    if (at > (int64_t)W.n_rows) at = (int64_t)W.n_rows;
    const long long ro = m ? off[at] : 0ll;
    const long long e0 = __shfl(ro, 0), e1 = __shfl(ro, 32);
    const long long next = __shfl(ro, (int)min(lane + 1u, 32u));
    const bool miss = lane < 32u && ((m >> lane) & 1u) != 0u && next == ro;   // a passing row without elements
    emit(miss, n_bins, (uint32_t)r0 + (lane & 31u));
    for (long long eb = e0; eb < e1; eb += 64) {   // (trip count per wave; every lane runs every shuffle)
      const long long e = eb + (long long)lane;
      const bool valid = e < e1;
      int pos = 0;   // the owner: the largest r in [0, 32) with offsets[r0 + r] <= e
      for (int step = 16; step > 0; step >>= 1) {
        const long long v = __shfl(ro, pos + step);
        if (v <= e) pos += step;
      }
      bool act = valid && ((m >> pos) & 1u) != 0u && first[e] != 0;
      uint32_t bin = 0u;
      if (act) {
        bin = (uint32_t)vals[e];
        act = bin < n_codes;
      }
      emit(act, bin, (uint32_t)r0 + (uint32_t)pos);
    }
  } else {
    const uint32_t j = it * 2u + (lane >> 5);
    bool act = false;
    uint32_t row = 0u;
    if (j < npass) {
      const uint32_t b = walk_block(W, j);
      act = ((walk_mask(W, b) >> (lane & 31u)) & 1u) != 0u;
      row = b * 32u + (lane & 31u);
    }
    uint32_t bin = n_bins;
    if (act) {
      if (F.kind == RF_FACET_CODES) {
        bin = (uint32_t)((const int32_t*)F.a_dev)[row];
        act = bin < n_codes;
      } else {
        const uint8_t tag = ((const uint8_t*)F.a_dev)[row];
        if (tag == RF_DTAG_STRING) {
          const unsigned long long c = (unsigned long long)((const int64_t*)F.b_dev)[row];
          act = c < (unsigned long long)n_codes;
          bin = (uint32_t)c;
        } else if (tag == RF_DTAG_BOOL) {
          bin = n_codes + (((const int64_t*)F.b_dev)[row] != 0 ? 1u : 0u);
        }
      }
    }
    emit(act, bin, row);
  }
}
