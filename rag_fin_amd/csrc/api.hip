// extern "C" search entry points: orchestration of the scan / merge launches.
// Reference call site replaced: Collection.search(query_embedding, "embedding",
// {"metric_type": "COSINE"}, top_k, ...) -- vector_rag_mcp/main.py:51-57.
#include "rf_internal.h"
#include <stdlib.h>
#include <string.h>

// ---- workspace layout ---------------------------------------------------------------------------
// Arrays carved off a caller's buffer in order, each 256-byte aligned (base == nullptr: sizes only).
struct rf_arena {
  unsigned char* base;
  size_t off;
  template <class T>
  T* take(size_t count) {
    T* p = base ? (T*)(base + off) : nullptr;
    off = (off + count * sizeof(T) + 255) / 256 * 256;
    return p;
  }
};

static rf_workspace carve(rf_arena& a) {
  rf_workspace ws;
  ws.thr = a.take<float>(RF_QWIDE);
  ws.eps = a.take<float>(RF_QWIDE);
  ws.cand_cnt = a.take<uint32_t>((size_t)RF_QWIDE * RF_CAND_SHARDS);
  ws.pmax = a.take<float>((size_t)RF_QWIDE * RF_SAMPLE_WGS);
  ws.cand = a.take<uint2>((size_t)RF_QWIDE * RF_CAND_SHARDS * RF_SHARD_CAP);
  ws.fold = a.take<uint4>((size_t)RF_FOLD_WAVES * RF_QCHUNK);
  ws.rmask = a.take<unsigned long long>(RF_FOLD_WAVES);
  ws.rlist = a.take<uint32_t>(RF_FOLD_BLOCKS);
  ws.rcnt = a.take<uint32_t>(1);
  ws.ex_score = a.take<double>((size_t)RF_QCHUNK * RF_EX_WGS * RF_MAX_K);
  ws.ex_row = a.take<int64_t>((size_t)RF_QCHUNK * RF_EX_WGS * RF_MAX_K);
  return ws;
}

// The SQ8 workspace is the FLAT one followed by the per-sweep query quantization (q^ for 64 queries
// of up to 1024 dims, then t_q, n_q, f_q).
static rf_sq8_ws carve_sq8(rf_arena& a, rf_workspace* ws) {
  const rf_workspace flat = carve(a);
  if (ws) *ws = flat;
  rf_sq8_ws sw;
  sw.q8 = a.take<int8_t>((size_t)RF_QCHUNK * 1024);
  sw.tq = a.take<float>(RF_QCHUNK);
  sw.nq = a.take<float>(RF_QCHUNK);
  sw.fq = a.take<float>(RF_QCHUNK);
  return sw;
}

// The grouped workspace is the SQ8 one followed by the partition maxima and the thresholds per
// (query, code) of a sweep.
static rf_grouped_ws carve_grouped(rf_arena& a, rf_workspace* ws) {
  carve_sq8(a, ws);
  rf_grouped_ws gw;
  gw.gpmax = a.take<float>((size_t)RF_GROUP_PARTS * RF_QCHUNK * RF_GROUP_MAX_CODES);
  gw.gthr = a.take<float>((size_t)RF_QCHUNK * RF_GROUP_MAX_CODES);
  return gw;
}

#ifdef RF_EXPERIMENTS
// Diagnostic hook: byte offset of a named workspace array ("pmax", "cand", "thr", "eps", "cand_cnt",
// "rmask", "rcnt").
extern "C" size_t rf_debug_workspace_offset(const char* field) {
  rf_arena a{(unsigned char*)(uintptr_t)4096, 0};   // never dereferenced
  const rf_workspace ws = carve(a);
  const struct { const char* name; const void* at; } fields[] = {
      {"pmax", ws.pmax}, {"cand", ws.cand},   {"thr", ws.thr},  {"eps", ws.eps},
      {"cand_cnt", ws.cand_cnt}, {"rmask", ws.rmask}, {"rcnt", ws.rcnt}};
  for (const auto& f : fields)
    if (field && !strcmp(field, f.name)) return (size_t)((const unsigned char*)f.at - a.base);
  return (size_t)-1;
}

// The tuning knobs (rf_internal.h, RF_KNOBS) as process-wide ints behind rf_set_tuning.
#define RF_KNOB_DEF(name, dflt, lo, hi) int rf_knob_##name = dflt;
RF_KNOBS(RF_KNOB_DEF)
#undef RF_KNOB_DEF
int rf_tuning_generation = 0;
void* rf_debug_buffer = nullptr;
extern "C" int rf_debug_set_buffer(void* dev_ptr) {
  rf_debug_buffer = dev_ptr;
  return RF_OK;
}
extern "C" int rf_set_tuning(const char* key, int value) {
  if (!key) return RF_ERR_INVALID;
  ++rf_tuning_generation;   // cached encode graphs were captured under the old settings
  const struct { const char* name; int* var; int lo, hi; } keys[] = {
#define RF_KNOB_KEY(name, dflt, lo, hi) {#name, &rf_knob_##name, lo, hi},
      RF_KNOBS(RF_KNOB_KEY)
#undef RF_KNOB_KEY
  };
  for (const auto& k : keys)
    if (!strcmp(key, k.name) && value >= k.lo && value <= k.hi) {
      if (k.var == &rf_knob_ring24 && value != 6 && value != 8 && value != 12 && value != 24) break;
      if (k.var == &rf_knob_sq8_ring12 && value != 4 && value != 6 && value != 12) break;
      *k.var = value;
      return RF_OK;
    }
  rf_set_error("rf_set_tuning: unknown key or bad value (%s = %d)", key, value);
  return RF_ERR_INVALID;
}
#endif

// rf_search sweeps the shadow first (rf_index_set_shadow_first) when one is attached and the index has
// the rows for it; the sweep itself also needs a plain batch of at most 64 queries (shadow_sweep).
static bool shadow_first(const rf_index_t* ix) { return ix && ix->shadow_min_rows > 0 && ix->sq8_tiles; }

// (with shadow-first set the rf_search workspace holds the SQ8 query area too)
extern "C" size_t rf_search_workspace_bytes(const rf_index_t* ix) {
  rf_arena a{nullptr, 0};
  if (shadow_first(ix)) carve_sq8(a, nullptr);
  else carve(a);
  return a.off;
}

extern "C" size_t rf_search_sq8_workspace_bytes(const rf_index_t* ix) {
  (void)ix;
  rf_arena a{nullptr, 0};
  carve_sq8(a, nullptr);
  return a.off;
}

// ---- argument checks ----------------------------------------------------------------------------
static int check_search_args(const char* fn, const rf_index_t* ix, const void* q, int B, int k,
                             const void* scores, const void* ids, const void* ws, size_t ws_bytes) {
  if (!ix || !q || !scores || !ids || !ws) {
    rf_set_error("%s: null argument", fn);
    return RF_ERR_INVALID;
  }
  if (B <= 0) {
    rf_set_error("%s: B = %d", fn, B);
    return RF_ERR_INVALID;
  }
  if (k <= 0 || k > RF_MAX_K) {
    rf_set_error("%s: k = %d outside 1..%d", fn, k, RF_MAX_K);
    return RF_ERR_UNSUPPORTED;
  }
  if ((((uintptr_t)q) & 15) || (((uintptr_t)ws) & 15)) {
    rf_set_error("%s: q / workspace must be 16-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  // (the FLAT size, which every form needs; the index itself is not read here)
  if (ws_bytes < rf_search_workspace_bytes(nullptr)) {
    rf_set_error("%s: workspace %zu B < required %zu B", fn, ws_bytes,
                 rf_search_workspace_bytes(nullptr));
    return RF_ERR_CAPACITY;
  }
  return RF_OK;
}

static int check_sq8(const char* fn, const rf_index_t* ix, size_t ws_bytes) {
  if (!ix->sq8_tiles) {
    rf_set_error("%s: no SQ8 shadow attached (rf_index_attach_sq8)", fn);
    return RF_ERR_INVALID;
  }
  if (ws_bytes < rf_search_sq8_workspace_bytes(ix)) {
    rf_set_error("%s: workspace %zu B < required %zu B", fn, ws_bytes, rf_search_sq8_workspace_bytes(ix));
    return RF_ERR_CAPACITY;
  }
  return RF_OK;
}

static int check_filter_arg(const char* fn, const void* filter_dev) {
  if (!filter_dev || (((uintptr_t)filter_dev) & 15)) {
    rf_set_error("%s: filter buffer null or not 16-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  return RF_OK;
}

__global__ void k_fill_empty(int n, int B, float* scores, int64_t* ids, double* exact,
                             uint32_t* flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    scores[i] = -INFINITY;
    ids[i] = -1;
    if (exact) exact[i] = -INFINITY;
  }
  if (flags && i < B) flags[i] = 0u;
}

// ---- the chunk walk -----------------------------------------------------------------------------
// Per-query outputs of a batch, [B, k] each (flags: [B]); any of them may be absent.
struct rf_out {
  float* scores;
  int64_t* ids;
  double* exact;     // (a weighted search: the decayed scores)
  uint32_t* flags;
  double* base;      // a weighted search only: the plain fp64 scores
};

static int fill_empty(int B, int k, const rf_out& o, hipStream_t st) {
  const int n = B * k;
  hipLaunchKernelGGL(k_fill_empty, dim3((n + 255) / 256), dim3(256), 0, st, n, B, o.scores, o.ids,
                     o.exact, o.flags);
  if (o.base)   // (a weighted search: its second fp64 output, through the same kernel)
    hipLaunchKernelGGL(k_fill_empty, dim3((n + 255) / 256), dim3(256), 0, st, n, 0, o.scores, o.ids, o.base,
                       (uint32_t*)nullptr);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

// More than one 64-query sweep left and dim 384: one wide sweep of up to 256 queries.
// Small corpora -- every row a candidate -- stay on the 64-query kernel (its inline flushes take
// any hit density, the wide kernel's bounded staging would flag every query), and so do large k
// (the k-th of ~64 partition maxima is a weak threshold) and k-dense searches of mid-sized
// corpora (expected hits per wave and phase ~ 2^15 k / N against room for 96).
static bool take_wide(const rf_index_t* ix, int left, int k) {
  return rf_wide_supported(ix) && left > RF_QCHUNK && ix->size > RF_SMALL_ROWS && k <= 16 &&
         ix->size >= (int64_t)k * 1024;
}

// Queries of the next sweep when `left` remain; widen: the caller's chain has a wide form.
static int chunk_width(const rf_index_t* ix, int left, int k, bool widen, bool* wide) {
  *wide = widen && take_wide(ix, left, k);
  const int cap = *wide ? RF_QWIDE : RF_QCHUNK;
  return left < cap ? left : cap;
}

template <class T>
static T* at(T* p, size_t off) { return p ? p + off : nullptr; }

// Walks a batch in sweeps: body(q0, nb, wide, q of the chunk, outputs of the chunk), with `row`
// output elements per query.  Anything else a body offsets (bounds, deltas) it offsets by q0.
template <class F>
static int for_chunks(const rf_index_t* ix, const void* q_dev, int B, int k, size_t row, bool widen,
                      const rf_out& o, F&& body) {
  for (int q0 = 0; q0 < B;) {
    bool wide;
    const int nb = chunk_width(ix, B - q0, k, widen, &wide);
    const size_t r0 = (size_t)q0 * row;
    const int rc = body(q0, nb, wide, (const _Float16*)q_dev + (size_t)q0 * ix->dim,
                        rf_out{at(o.scores, r0), at(o.ids, r0), at(o.exact, r0), at(o.flags, (size_t)q0), at(o.base, r0)});
    if (rc != RF_OK) return rc;
    q0 += nb;
  }
  return RF_OK;
}

// ---- the search chain ---------------------------------------------------------------------------
// Which form of the chain a sweep runs.  filt: the masked sweep of filtered search (never wide:
// B > 64 runs as 64-query sweeps).  sq8: the int8 emit over the shadow, after quantizing the
// queries into *sq8 (64-query sweeps only, no filtered form).  wide: the 256-query kernels.
// band: range search (with or without filt; never SQ8, never wide, no sample fold): the sample
// pass clips at the ceiling by the eps a pre-kernel writes, the threshold has the floor of the
// band under it, the emit clips at the ceiling and the merge drops what the fp64 scores put
// outside the band.
// after: search-after (always with band, both sides open when the caller gave none): the band
// chain with the ceiling of each query read from its bound in device memory; the merge also drops
// what the fp64 (score, id) rule puts at or before the bound.
// multi: per-query filters (always with filt, which is then the union of the batch's filters;
// never with sq8, wide, band or after): both sweeps walk the union's blocks and test each query's
// rows against its own filter's words; threshold and merge are per query as ever.
// weights: per-row weights (with or without filt; never with sq8, wide, band, after or multi, and no
// sample fold): both sweeps run on w32[row] * score, threshold and merge take eps_w = 2 eps, and the
// merge ranks by (w64[row] * s desc, s desc, row asc) -- DESIGN 4.4q.
struct rf_variant {
  const rf_filter_view* filt;
  const rf_sq8_ws* sq8;
  bool wide;
  const rf_band* band;
  const rf_after* after;
  const rf_multi* multi;
  bool coarse;   // SQ8 timed as the four FLAT stages: sample | threshold | quantize + emit + refine | merge
  const rf_weights* weights;
};

static int mark(hipEvent_t* ev, int* n, hipStream_t st) {
  if (ev) RF_HIP(hipEventRecord(ev[(*n)++], st));
  return RF_OK;
}

// Time the stages of one sweep: run(ev) records `marks` events, one before the first stage and one
// after each; the marks - 1 stage times in ms go to stage_ms.
template <class F>
static int time_stages(int marks, float* stage_ms, F run) {
  hipEvent_t ev[7];
  for (int i = 0; i < marks; ++i) RF_HIP(hipEventCreate(&ev[i]));
  const int rc = run(ev);
  if (rc == RF_OK) {
    RF_HIP(hipEventSynchronize(ev[marks - 1]));
    for (int i = 0; i + 1 < marks; ++i) RF_HIP(hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]));
  }
  for (int i = 0; i < marks; ++i) (void)hipEventDestroy(ev[i]);
  return rc;
}

// One sweep of nb <= RF_QWIDE queries: (SQ8: quantize the queries ->) sample -> threshold -> emit ->
// (SQ8: prune + refine ->) merge.  ev: nullable; one event before the first stage and one after each
// (5; SQ8: 7, or 6 with v.coarse, which times emit + refine as one).
static int sweep(const rf_index_t* ix, const rf_variant& v, const _Float16* qc, int nb, int k, int64_t id_base,
                 const rf_workspace& ws, const rf_out& o, hipStream_t st, hipEvent_t* ev) {
  const int JB = nb <= 32 ? 1 : 2;
  int P = 0, n_ev = 0;
  // the unfiltered 64-query FLAT sweep folds the sample into the emit; n_samp stays 0 unless the
  // sample pass keeps its lists
  rf_fold kept{};
  rf_fold* fold = (v.wide || v.sq8 || v.filt || v.band || v.weights) ? nullptr : &kept;
  const float* w32 = v.weights ? v.weights->w32 : nullptr;
  int rc = mark(ev, &n_ev, st);
  if (v.sq8) {
    if (rc == RF_OK) rc = rf_launch_sq8_queries(ix, qc, nb, *v.sq8, st);
    if (rc == RF_OK) rc = mark(ev, &n_ev, st);
  }
  if (rc == RF_OK && ix->size > RF_SMALL_ROWS && v.band) rc = rf_launch_band_eps(ix, qc, nb, ws, st);
  if (rc == RF_OK && ix->size > RF_SMALL_ROWS)
    rc = v.wide ? rf_launch_wide_sample(ix, qc, nb, ws, &P, st)
                : rf_launch_sample(ix, qc, nb, JB, ws, &P, st, v.filt, fold, v.band, v.after, v.multi, w32);
  if (rc == RF_OK) rc = mark(ev, &n_ev, st);
  if (rc == RF_OK)
    rc = v.weights ? rf_launch_threshold_weighted(ix, qc, nb, k, P, ws, st)
                   : rf_launch_threshold(ix, qc, nb, k, P, ws, st, fold, v.sq8, v.band);
  if (rc == RF_OK) rc = mark(ev, &n_ev, st);
  if (rc == RF_OK)
    rc = v.wide  ? rf_launch_wide_emit(ix, qc, nb, ws, st)
         : v.sq8 ? rf_launch_sq8_emit(ix, nb, JB, ws, *v.sq8, st)
                 : rf_launch_emit(ix, qc, nb, JB, ws, st, v.filt, fold, v.band, v.after, v.multi, w32);
  if (v.sq8) {
    if (rc == RF_OK && !v.coarse) rc = mark(ev, &n_ev, st);
    if (rc == RF_OK) rc = rf_launch_shadow_refine(ix, qc, nb, k, ws, *v.sq8, st);
  }
  if (rc == RF_OK) rc = mark(ev, &n_ev, st);
  if (rc == RF_OK)
    rc = v.weights ? rf_launch_merge_weighted(ix, qc, nb, k, id_base, ws, v.weights->w64, o.scores, o.ids, o.exact, o.base,
                                              o.flags, st)
                   : rf_launch_merge(ix, qc, nb, k, id_base, ws, o.scores, o.ids, o.exact, o.flags, st, v.band, v.after);
  if (rc == RF_OK) rc = mark(ev, &n_ev, st);
  return rc;
}

// Every search entry point below: the whole batch (stage_ms == nullptr), or its first sweep alone
// with HIP events around the stages, whose times in ms go to stage_ms (4 floats, RF_SQ8 6).
// sq8 on a small corpus runs the FLAT chain: every row is a candidate there anyway (no sample pass
// to gain from).
enum { RF_FP16 = 0, RF_SQ8 = 1, RF_SHADOW = 2 };   // RF_SHADOW: the SQ8 chain, timed as the four FLAT stages
static int search_enqueue(const rf_index_t* ix, const void* q_dev, int B, int k, int64_t id_base, const rf_out& o,
                          void* workspace_dev, hipStream_t st, const rf_filter_view* filt, int sq8,
                          float* stage_ms = nullptr, const rf_band* band = nullptr,
                          const rf_after* after = nullptr, const rf_multi* multi = nullptr,
                          const rf_weights* weights = nullptr) {
  if (ix->size == 0) return fill_empty(B, k, o, st);
  rf_arena a{(unsigned char*)workspace_dev, 0};
  rf_workspace ws;
  const rf_sq8_ws sw = carve_sq8(a, &ws);   // (the SQ8 area is only touched by an SQ8 sweep)
  const rf_sq8_ws* sq = sq8 != RF_FP16 && ix->size > RF_SMALL_ROWS ? &sw : nullptr;
  const bool coarse = sq8 == RF_SHADOW;
  const bool widen = !filt && !sq && !band && !weights;
  if (!stage_ms)
    return for_chunks(ix, q_dev, B, k, (size_t)k, widen, o,
                      [&](int q0, int nb, bool wide, const _Float16* qc, const rf_out& oc) {
                        const rf_after ac{after ? after->score + q0 : nullptr, after ? after->id + q0 : nullptr};
                        const rf_multi mc{multi ? multi->masks_t : nullptr, multi ? multi->qfilter + q0 : nullptr,
                                          multi ? multi->gp : 0u};
                        return sweep(ix, rf_variant{filt, sq, wide, band, after ? &ac : nullptr, multi ? &mc : nullptr, coarse,
                                                    weights},
                                     qc, nb, k, id_base, ws, oc, st, nullptr);
                      });
  bool wide;
  const int nb = chunk_width(ix, B, k, widen, &wide);   // the first sweep the batch would run
  // The four coarse stages of the shadow chain: `sample` and `threshold` are the kernels the fp16 chain
  // runs under those names, `emit` is everything that stands in the fp16 emit's place -- the query
  // quantization (only the int8 sweep reads q^), the int8 sweep and the prune + refine.
  float t[6];
  const bool fold4 = sq && coarse;
  const int rc = time_stages(sq ? (coarse ? 6 : 7) : 5, fold4 ? t : stage_ms, [&](hipEvent_t* ev) {
    return sweep(ix, rf_variant{filt, sq, wide, band, after, multi, coarse, weights}, (const _Float16*)q_dev, nb, k,
                 id_base, ws, o, st, ev);
  });
  if (rc == RF_OK && fold4) {
    stage_ms[0] = t[1];
    stage_ms[1] = t[2];
    stage_ms[2] = t[0] + t[3];
    stage_ms[3] = t[4];
  }
  return rc;
}

// The chain of a plain search of B queries: the shadow first (rf_index_set_shadow_first) when the index
// carries one, has the rows for it and the batch is one 64-query sweep; otherwise fp16 (wide sweeps
// and the 64-query chunks of a larger batch included).
static int plain_chain(const rf_index_t* ix, int B) {
  return shadow_first(ix) && ix->size >= ix->shadow_min_rows && ix->size > RF_SMALL_ROWS && B <= RF_QCHUNK ? RF_SHADOW
                                                                                                          : RF_FP16;
}

extern "C" int rf_index_set_shadow_first(rf_index_t* ix, int64_t min_rows) {
  if (!ix) {
    rf_set_error("rf_index_set_shadow_first: null index");
    return RF_ERR_INVALID;
  }
  ix->shadow_min_rows = min_rows > 0 ? min_rows : 0;
  return RF_OK;
}

extern "C" int rf_search(const rf_index_t* ix, const void* q_dev, int B, int k, int64_t id_base,
                         float* scores_dev, int64_t* ids_dev, double* exact_dev,
                         uint32_t* flags_dev, void* workspace_dev, size_t workspace_bytes,
                         void* stream) {
  int rc = check_search_args("rf_search", ix, q_dev, B, k, scores_dev, ids_dev, workspace_dev,
                             workspace_bytes);
  if (rc == RF_OK && plain_chain(ix, B) == RF_SHADOW) rc = check_sq8("rf_search", ix, workspace_bytes);
  if (rc != RF_OK) return rc;
  return search_enqueue(ix, q_dev, B, k, id_base, rf_out{scores_dev, ids_dev, exact_dev, flags_dev}, workspace_dev,
                        (hipStream_t)stream, nullptr, plain_chain(ix, B));
}

// The fp16 chain whatever is attached: the FLAT tier of the flagged-query ladder.
extern "C" int rf_search_fp16(const rf_index_t* ix, const void* q_dev, int B, int k, int64_t id_base,
                              float* scores_dev, int64_t* ids_dev, double* exact_dev,
                              uint32_t* flags_dev, void* workspace_dev, size_t workspace_bytes,
                              void* stream) {
  int rc = check_search_args("rf_search_fp16", ix, q_dev, B, k, scores_dev, ids_dev, workspace_dev,
                             workspace_bytes);
  if (rc != RF_OK) return rc;
  return search_enqueue(ix, q_dev, B, k, id_base, rf_out{scores_dev, ids_dev, exact_dev, flags_dev}, workspace_dev,
                        (hipStream_t)stream, nullptr, RF_FP16);
}

extern "C" int rf_search_profile(const rf_index_t* ix, const void* q_dev, int B, int k,
                                 int64_t id_base, float* scores_dev, int64_t* ids_dev,
                                 double* exact_dev, uint32_t* flags_dev, void* workspace_dev,
                                 size_t workspace_bytes, void* stream, float* stage_ms_host) {
  int rc = check_search_args("rf_search_profile", ix, q_dev, B, k, scores_dev, ids_dev,
                             workspace_dev, workspace_bytes);
  if (rc == RF_OK && plain_chain(ix, B) == RF_SHADOW) rc = check_sq8("rf_search_profile", ix, workspace_bytes);
  if (rc != RF_OK) return rc;
  if (!stage_ms_host || ix->size == 0) {
    rf_set_error("rf_search_profile: null stage buffer or empty index");
    return RF_ERR_INVALID;
  }
  return search_enqueue(ix, q_dev, B, k, id_base, rf_out{scores_dev, ids_dev, exact_dev, flags_dev}, workspace_dev,
                        (hipStream_t)stream, nullptr, plain_chain(ix, B), stage_ms_host);
}

// ---- SQ8 (include/ragfin.h, "SQ8 index") ------------------------------------------------------------
extern "C" int rf_search_sq8(const rf_index_t* ix, const void* q_dev, int B, int k, int64_t id_base,
                             float* scores_dev, int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream) {
  int rc = check_search_args("rf_search_sq8", ix, q_dev, B, k, scores_dev, ids_dev, workspace_dev,
                             workspace_bytes);
  if (rc != RF_OK) return rc;
  rc = check_sq8("rf_search_sq8", ix, workspace_bytes);
  if (rc != RF_OK) return rc;
  return search_enqueue(ix, q_dev, B, k, id_base, rf_out{scores_dev, ids_dev, exact_dev, flags_dev}, workspace_dev,
                        (hipStream_t)stream, nullptr, RF_SQ8);
}

extern "C" int rf_search_sq8_profile(const rf_index_t* ix, const void* q_dev, int B, int k, int64_t id_base,
                                     float* scores_dev, int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev,
                                     void* workspace_dev, size_t workspace_bytes, void* stream,
                                     float* stage_ms_host) {
  int rc = check_search_args("rf_search_sq8_profile", ix, q_dev, B, k, scores_dev, ids_dev, workspace_dev,
                             workspace_bytes);
  if (rc != RF_OK) return rc;
  rc = check_sq8("rf_search_sq8_profile", ix, workspace_bytes);
  if (rc != RF_OK) return rc;
  if (!stage_ms_host || ix->size <= RF_SMALL_ROWS) {
    rf_set_error("rf_search_sq8_profile: null stage buffer or a corpus of <= %d rows", RF_SMALL_ROWS);
    return RF_ERR_INVALID;
  }
  return search_enqueue(ix, q_dev, B, k, id_base, rf_out{scores_dev, ids_dev, exact_dev, flags_dev}, workspace_dev,
                        (hipStream_t)stream, nullptr, RF_SQ8, stage_ms_host);
}

extern "C" int rf_debug_scores_sq8(const rf_index_t* ix, const void* q_dev, int B, int64_t n, float* out_dev,
                                   float* delta_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!ix || !q_dev || !out_dev || !workspace_dev || B <= 0 || n <= 0 || n > ix->size) {
    rf_set_error("rf_debug_scores_sq8: bad argument");
    return RF_ERR_INVALID;
  }
  int rc = check_sq8("rf_debug_scores_sq8", ix, workspace_bytes);
  if (rc != RF_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  rf_arena a{(unsigned char*)workspace_dev, 0};
  const rf_sq8_ws sw = carve_sq8(a, nullptr);
  // (n scores per query: the walk offsets out_dev as a [B, n] output)
  return for_chunks(ix, q_dev, B, 0, (size_t)n, false, rf_out{out_dev, nullptr, nullptr, nullptr},
                    [&](int q0, int nb, bool, const _Float16* qc, const rf_out& oc) {
                      const int rc = rf_launch_sq8_queries(ix, qc, nb, sw, st);
                      return rc != RF_OK ? rc : rf_launch_sq8_debug(ix, nb, n, sw, oc.scores, at(delta_dev, (size_t)q0), st);
                    });
}

static int exhaustive_impl(const char* fn, const rf_index_t* ix, const void* q_dev, int B, int k,
                           int64_t id_base, float* scores_dev, int64_t* ids_dev, double* exact_dev,
                           const double* after_s, const int64_t* after_r, void* workspace_dev,
                           size_t workspace_bytes, void* stream, const uint32_t* mask = nullptr,
                           const rf_band* band = nullptr) {
  int rc = check_search_args(fn, ix, q_dev, B, k, scores_dev, ids_dev, workspace_dev, workspace_bytes);
  if (rc != RF_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const rf_out o{scores_dev, ids_dev, exact_dev, nullptr};
  if (ix->size == 0) return fill_empty(B, k, o, st);
  rf_arena a{(unsigned char*)workspace_dev, 0};
  const rf_workspace ws = carve(a);
  return for_chunks(ix, q_dev, B, k, (size_t)k, false, o,
                    [&](int q0, int nb, bool, const _Float16* qc, const rf_out& oc) {
                      return rf_launch_exhaustive(ix, qc, nb, k, id_base, ws, oc.scores, oc.ids, oc.exact,
                                                  at(after_s, (size_t)q0), at(after_r, (size_t)q0), st, mask, band);
                    });
}

extern "C" int rf_search_exhaustive(const rf_index_t* ix, const void* q_dev, int B, int k,
                                    int64_t id_base, float* scores_dev, int64_t* ids_dev,
                                    double* exact_dev, void* workspace_dev, size_t workspace_bytes,
                                    void* stream) {
  return exhaustive_impl("rf_search_exhaustive", ix, q_dev, B, k, id_base, scores_dev, ids_dev,
                         exact_dev, nullptr, nullptr, workspace_dev, workspace_bytes, stream);
}

extern "C" int rf_search_exhaustive_after(const rf_index_t* ix, const void* q_dev, int B, int k,
                                          int64_t id_base, const double* after_score_dev,
                                          const int64_t* after_id_dev, float* scores_dev,
                                          int64_t* ids_dev, double* exact_dev, void* workspace_dev,
                                          size_t workspace_bytes, void* stream) {
  if (!after_score_dev || !after_id_dev) {
    rf_set_error("rf_search_exhaustive_after: null bound arrays");
    return RF_ERR_INVALID;
  }
  return exhaustive_impl("rf_search_exhaustive_after", ix, q_dev, B, k, id_base, scores_dev, ids_dev,
                         exact_dev, after_score_dev, after_id_dev, workspace_dev, workspace_bytes, stream);
}

// ---- filtered search (include/ragfin.h, "filtered search") ---------------------------------------
extern "C" int rf_search_filtered(const rf_index_t* ix, const void* filter_dev, const void* q_dev, int B, int k,
                                  int64_t id_base, float* scores_dev, int64_t* ids_dev, double* exact_dev,
                                  uint32_t* flags_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  int rc = check_search_args("rf_search_filtered", ix, q_dev, B, k, scores_dev, ids_dev, workspace_dev,
                             workspace_bytes);
  if (rc != RF_OK) return rc;
  rc = check_filter_arg("rf_search_filtered", filter_dev);
  if (rc != RF_OK) return rc;
  const rf_filter_view f = rf_filter_carve(filter_dev, ix->size);
  return search_enqueue(ix, q_dev, B, k, id_base, rf_out{scores_dev, ids_dev, exact_dev, flags_dev}, workspace_dev,
                        (hipStream_t)stream, &f, RF_FP16);
}

extern "C" int rf_search_exhaustive_filtered(const rf_index_t* ix, const void* filter_dev, const void* q_dev,
                                             int B, int k, int64_t id_base, const double* after_score_dev,
                                             const int64_t* after_id_dev, float* scores_dev, int64_t* ids_dev,
                                             double* exact_dev, void* workspace_dev, size_t workspace_bytes,
                                             void* stream) {
  int rc = check_filter_arg("rf_search_exhaustive_filtered", filter_dev);
  if (rc != RF_OK) return rc;
  if ((after_score_dev == nullptr) != (after_id_dev == nullptr)) {
    rf_set_error("rf_search_exhaustive_filtered: give both bound arrays or neither");
    return RF_ERR_INVALID;
  }
  // (the masked exhaustive kernel checks no header: the mask of a buffer built for this index
  // covers exactly ix->size rows)
  const rf_filter_view f = rf_filter_carve(filter_dev, ix ? ix->size : 0);
  return exhaustive_impl("rf_search_exhaustive_filtered", ix, q_dev, B, k, id_base, scores_dev, ids_dev,
                         exact_dev, after_score_dev, after_id_dev, workspace_dev, workspace_bytes, stream, f.mask);
}

// ---- per-query filters (include/ragfin.h, "per-query filters") -----------------------------------
extern "C" int rf_search_multi_filtered(const rf_index_t* ix, const void* multi_dev, int n_filters,
                                        const int32_t* qfilter_dev, const void* q_dev, int B, int k, int64_t id_base,
                                        float* scores_dev, int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev,
                                        void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!qfilter_dev || n_filters < 1 || n_filters > RF_MULTI_MAX_FILTERS) {
    rf_set_error("rf_search_multi_filtered: null qfilter, or n_filters = %d outside 1..%d", n_filters,
                 RF_MULTI_MAX_FILTERS);
    return RF_ERR_INVALID;
  }
  int rc = check_filter_arg("rf_search_multi_filtered", multi_dev);
  if (rc != RF_OK) return rc;
  rc = check_search_args("rf_search_multi_filtered", ix, q_dev, B, k, scores_dev, ids_dev, workspace_dev,
                         workspace_bytes);
  if (rc != RF_OK) return rc;
  // the buffer starts with the union in the filter buffer format: the sweeps' work list
  const rf_filter_view f = rf_filter_carve(multi_dev, ix->size);
  size_t so;
  rf_multi_layout(ix->size, n_filters, &so);
  const rf_multi m{(const uint32_t*)((const unsigned char*)multi_dev + so), qfilter_dev, rf_multi_columns(n_filters)};
  return search_enqueue(ix, q_dev, B, k, id_base, rf_out{scores_dev, ids_dev, exact_dev, flags_dev}, workspace_dev,
                        (hipStream_t)stream, &f, RF_FP16, nullptr, nullptr, nullptr, &m);
}

// ---- decayed search (include/ragfin.h, "decayed search") ------------------------------------------
static int check_weights(const char* fn, const rf_index_t* ix, const void* filter_dev, const float* w32_dev,
                         const double* w64_dev) {
  if (!w32_dev || !w64_dev || (((uintptr_t)w32_dev) & 15) || (((uintptr_t)w64_dev) & 7)) {
    rf_set_error("%s: weights null, or w32 not 16-byte / w64 not 8-byte aligned", fn);
    return RF_ERR_INVALID;
  }
  if (ix && ix->size > (int64_t)0xFFFFFFFFll - 32) {
    rf_set_error("%s: %lld rows out of range", fn, (long long)ix->size);
    return RF_ERR_INVALID;
  }
  return filter_dev ? check_filter_arg(fn, filter_dev) : RF_OK;
}

extern "C" int rf_search_weighted(const rf_index_t* ix, const void* filter_dev, const float* w32_dev,
                                  const double* w64_dev, const void* q_dev, int B, int k, int64_t id_base,
                                  float* scores_dev, int64_t* ids_dev, double* decayed_dev, double* base_dev,
                                  uint32_t* flags_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  int rc = check_search_args("rf_search_weighted", ix, q_dev, B, k, scores_dev, ids_dev, workspace_dev,
                             workspace_bytes);
  if (rc == RF_OK) rc = check_weights("rf_search_weighted", ix, filter_dev, w32_dev, w64_dev);
  if (rc != RF_OK) return rc;
  const rf_filter_view f = filter_dev ? rf_filter_carve(filter_dev, ix->size) : rf_filter_view{};
  const rf_weights w{w32_dev, w64_dev};
  return search_enqueue(ix, q_dev, B, k, id_base, rf_out{scores_dev, ids_dev, decayed_dev, flags_dev, base_dev},
                        workspace_dev, (hipStream_t)stream, filter_dev ? &f : nullptr, RF_FP16, nullptr, nullptr, nullptr,
                        nullptr, &w);
}

extern "C" int rf_search_exhaustive_weighted(const rf_index_t* ix, const void* filter_dev, const float* w32_dev,
                                             const double* w64_dev, const void* q_dev, int B, int k, int64_t id_base,
                                             float* scores_dev, int64_t* ids_dev, double* decayed_dev,
                                             double* base_dev, void* workspace_dev, size_t workspace_bytes,
                                             void* stream) {
  int rc = check_search_args("rf_search_exhaustive_weighted", ix, q_dev, B, k, scores_dev, ids_dev, workspace_dev,
                             workspace_bytes);
  if (rc == RF_OK) rc = check_weights("rf_search_exhaustive_weighted", ix, filter_dev, w32_dev, w64_dev);
  if (rc != RF_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const rf_out o{scores_dev, ids_dev, decayed_dev, nullptr, base_dev};
  if (ix->size == 0) return fill_empty(B, k, o, st);
  rf_arena a{(unsigned char*)workspace_dev, 0};
  const rf_workspace ws = carve(a);
  // (as in rf_search_exhaustive_filtered, the mask of a buffer built for this index covers its rows)
  const uint32_t* mask = filter_dev ? rf_filter_carve(filter_dev, ix->size).mask : nullptr;
  return for_chunks(ix, q_dev, B, k, (size_t)k, false, o,
                    [&](int, int nb, bool, const _Float16* qc, const rf_out& oc) {
                      return rf_launch_exhaustive_weighted(ix, qc, nb, k, id_base, ws, w64_dev, oc.scores, oc.ids, oc.exact,
                                                           oc.base, st, mask);
                    });
}

// ---- range search (include/ragfin.h, "range search") ----------------------------------------------
static int check_band(const char* fn, double radius, double range_filter) {
  if (!(radius < range_filter)) {   // also catches a NaN on either side
    rf_set_error("%s: need radius < range_filter (got %g, %g)", fn, radius, range_filter);
    return RF_ERR_INVALID;
  }
  return RF_OK;
}

extern "C" int rf_search_range(const rf_index_t* ix, const void* filter_dev, const void* q_dev, int B, int k,
                               int64_t id_base, double radius, double range_filter, float* scores_dev,
                               int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev, void* workspace_dev,
                               size_t workspace_bytes, void* stream) {
  int rc = check_search_args("rf_search_range", ix, q_dev, B, k, scores_dev, ids_dev, workspace_dev,
                             workspace_bytes);
  if (rc == RF_OK) rc = check_band("rf_search_range", radius, range_filter);
  if (rc == RF_OK && filter_dev) rc = check_filter_arg("rf_search_range", filter_dev);
  if (rc != RF_OK) return rc;
  const rf_band band{radius, range_filter};
  const rf_filter_view f = filter_dev ? rf_filter_carve(filter_dev, ix->size) : rf_filter_view{};
  return search_enqueue(ix, q_dev, B, k, id_base, rf_out{scores_dev, ids_dev, exact_dev, flags_dev}, workspace_dev,
                        (hipStream_t)stream, filter_dev ? &f : nullptr, RF_FP16, nullptr, &band);
}

extern "C" int rf_search_exhaustive_range(const rf_index_t* ix, const void* filter_dev, const void* q_dev, int B,
                                          int k, int64_t id_base, double radius, double range_filter,
                                          const double* after_score_dev, const int64_t* after_id_dev,
                                          float* scores_dev, int64_t* ids_dev, double* exact_dev,
                                          void* workspace_dev, size_t workspace_bytes, void* stream) {
  int rc = check_band("rf_search_exhaustive_range", radius, range_filter);
  if (rc == RF_OK && filter_dev) rc = check_filter_arg("rf_search_exhaustive_range", filter_dev);
  if (rc != RF_OK) return rc;
  if ((after_score_dev == nullptr) != (after_id_dev == nullptr)) {
    rf_set_error("rf_search_exhaustive_range: give both bound arrays or neither");
    return RF_ERR_INVALID;
  }
  const rf_band band{radius, range_filter};
  const rf_filter_view f = filter_dev ? rf_filter_carve(filter_dev, ix ? ix->size : 0) : rf_filter_view{};
  return exhaustive_impl("rf_search_exhaustive_range", ix, q_dev, B, k, id_base, scores_dev, ids_dev, exact_dev,
                         after_score_dev, after_id_dev, workspace_dev, workspace_bytes, stream,
                         filter_dev ? f.mask : nullptr, &band);
}

// ---- paged search (include/ragfin.h, "paged search") ----------------------------------------------
static int search_after_impl(const char* fn, const rf_index_t* ix, const void* filter_dev, const void* q_dev, int B,
                             int k, int64_t id_base, double radius, double range_filter,
                             const double* after_score_dev, const int64_t* after_id_dev, const rf_out& o,
                             void* workspace_dev, size_t workspace_bytes, void* stream, float* stage_ms) {
  if (!after_score_dev || !after_id_dev) {
    rf_set_error("%s: null bound arrays", fn);
    return RF_ERR_INVALID;
  }
  if (k > RF_MAX_K) {   // (no larger sweep exists to be "unsupported" here: a page is at most RF_MAX_K hits)
    rf_set_error("%s: k = %d outside 1..%d", fn, k, RF_MAX_K);
    return RF_ERR_INVALID;
  }
  int rc = check_search_args(fn, ix, q_dev, B, k, o.scores, o.ids, workspace_dev, workspace_bytes);
  if (rc == RF_OK) rc = check_band(fn, radius, range_filter);
  if (rc == RF_OK && filter_dev) rc = check_filter_arg(fn, filter_dev);
  if (rc != RF_OK) return rc;
  const rf_band band{radius, range_filter};
  const rf_after after{after_score_dev, after_id_dev};
  const rf_filter_view f = filter_dev ? rf_filter_carve(filter_dev, ix->size) : rf_filter_view{};
  return search_enqueue(ix, q_dev, B, k, id_base, o, workspace_dev, (hipStream_t)stream, filter_dev ? &f : nullptr,
                        RF_FP16, stage_ms, &band, &after);
}

extern "C" int rf_search_after(const rf_index_t* ix, const void* filter_dev, const void* q_dev, int B, int k,
                               int64_t id_base, double radius, double range_filter, const double* after_score_dev,
                               const int64_t* after_id_dev, float* scores_dev, int64_t* ids_dev, double* exact_dev,
                               uint32_t* flags_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return search_after_impl("rf_search_after", ix, filter_dev, q_dev, B, k, id_base, radius, range_filter,
                           after_score_dev, after_id_dev, rf_out{scores_dev, ids_dev, exact_dev, flags_dev},
                           workspace_dev, workspace_bytes, stream, nullptr);
}

extern "C" int rf_search_after_profile(const rf_index_t* ix, const void* filter_dev, const void* q_dev, int B, int k,
                                       int64_t id_base, double radius, double range_filter,
                                       const double* after_score_dev, const int64_t* after_id_dev, float* scores_dev,
                                       int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev, void* workspace_dev,
                                       size_t workspace_bytes, void* stream, float* stage_ms_host) {
  if (!stage_ms_host || !ix || ix->size == 0) {
    rf_set_error("rf_search_after_profile: null stage buffer, null or empty index");
    return RF_ERR_INVALID;
  }
  return search_after_impl("rf_search_after_profile", ix, filter_dev, q_dev, B, k, id_base, radius, range_filter,
                           after_score_dev, after_id_dev, rf_out{scores_dev, ids_dev, exact_dev, flags_dev},
                           workspace_dev, workspace_bytes, stream, stage_ms_host);
}

// ---- grouping search (include/ragfin.h, "grouping search") ----------------------------------------
extern "C" size_t rf_search_grouped_workspace_bytes(const rf_index_t* ix) {
  (void)ix;
  rf_arena a{nullptr, 0};
  carve_grouped(a, nullptr);
  return a.off;
}

extern "C" size_t rf_debug_grouped_counters_offset(void) {
  rf_arena a{(unsigned char*)(uintptr_t)4096, 0};   // never dereferenced
  const rf_workspace ws = carve(a);
  return (size_t)((const unsigned char*)ws.cand_cnt - a.base);
}

// One grouped sweep of nb <= 64 queries: eps -> group-maximum sweep -> thresholds -> emit -> merge.
// ev: nullable, 5 events.
static int sweep_grouped(const rf_index_t* ix, const rf_filter_view* filt, const rf_group& g, const _Float16* qc,
                         int nb, int64_t id_base, const rf_workspace& ws, const rf_grouped_ws& gws,
                         const rf_out& o, hipStream_t st, hipEvent_t* ev) {
  const int JB = nb <= 32 ? 1 : 2;
  int P = 0, n_ev = 0;
  int rc = rf_launch_band_eps(ix, qc, nb, ws, st);
  if (rc == RF_OK) rc = mark(ev, &n_ev, st);
  if (rc == RF_OK) rc = rf_launch_group_max(ix, qc, nb, JB, g, ws, gws, &P, st, filt);
  if (rc == RF_OK) rc = mark(ev, &n_ev, st);
  if (rc == RF_OK) rc = rf_launch_group_threshold(nb, g, P, ws, gws, st);
  if (rc == RF_OK) rc = mark(ev, &n_ev, st);
  if (rc == RF_OK) rc = rf_launch_group_emit(ix, qc, nb, JB, g, ws, gws, st, filt);
  if (rc == RF_OK) rc = mark(ev, &n_ev, st);
  if (rc == RF_OK) rc = rf_launch_merge_grouped(ix, qc, nb, g, id_base, ws, o.scores, o.ids, o.exact, o.flags, st);
  if (rc == RF_OK) rc = mark(ev, &n_ev, st);
  return rc;
}

static int grouped_impl(const char* fn, const rf_index_t* ix, const void* filter_dev, const int32_t* codes,
                        int n_codes, const void* q_dev, int B, int n_groups, int group_size, int64_t id_base,
                        const rf_out& o, void* workspace_dev, size_t workspace_bytes, hipStream_t st,
                        float* stage_ms) {
  if (!codes || n_groups < 1 || group_size < 1 || n_codes < 1 ||
      (int64_t)n_groups * group_size > RF_MAX_K) {
    rf_set_error("%s: null codes, or n_codes / n_groups / group_size < 1, or n_groups * group_size > %d", fn,
                 RF_MAX_K);
    return RF_ERR_INVALID;
  }
  if (n_codes > RF_GROUP_MAX_CODES) {
    rf_set_error("%s: n_codes = %d above the fused path's %d", fn, n_codes, RF_GROUP_MAX_CODES);
    return RF_ERR_UNSUPPORTED;
  }
  const int k = n_groups * group_size;
  int rc = check_search_args(fn, ix, q_dev, B, k, o.scores, o.ids, workspace_dev, workspace_bytes);
  if (rc == RF_OK && filter_dev) rc = check_filter_arg(fn, filter_dev);
  if (rc != RF_OK) return rc;
  if (workspace_bytes < rf_search_grouped_workspace_bytes(ix)) {
    rf_set_error("%s: workspace %zu B < required %zu B", fn, workspace_bytes, rf_search_grouped_workspace_bytes(ix));
    return RF_ERR_CAPACITY;
  }
  if (ix->size == 0) {
    if (stage_ms) {
      rf_set_error("%s: empty index", fn);
      return RF_ERR_INVALID;
    }
    return fill_empty(B, k, o, st);
  }
  rf_arena a{(unsigned char*)workspace_dev, 0};
  rf_workspace ws;
  const rf_grouped_ws gws = carve_grouped(a, &ws);
  const rf_filter_view f = filter_dev ? rf_filter_carve(filter_dev, ix->size) : rf_filter_view{};
  const rf_filter_view* filt = filter_dev ? &f : nullptr;
  const rf_group g{codes, n_codes, n_groups, group_size};
  if (!stage_ms)
    return for_chunks(ix, q_dev, B, k, (size_t)k, false, o,
                      [&](int, int nb, bool, const _Float16* qc, const rf_out& oc) {
                        return sweep_grouped(ix, filt, g, qc, nb, id_base, ws, gws, oc, st, nullptr);
                      });
  return time_stages(5, stage_ms, [&](hipEvent_t* ev) {
    return sweep_grouped(ix, filt, g, (const _Float16*)q_dev, B < RF_QCHUNK ? B : RF_QCHUNK, id_base, ws, gws, o, st, ev);
  });
}

extern "C" int rf_search_grouped(const rf_index_t* ix, const void* filter_dev, const int32_t* group_codes_dev,
                                 int n_codes, const void* q_dev, int B, int n_groups, int group_size,
                                 int64_t id_base, float* scores_dev, int64_t* ids_dev, double* exact_dev,
                                 uint32_t* flags_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return grouped_impl("rf_search_grouped", ix, filter_dev, group_codes_dev, n_codes, q_dev, B, n_groups, group_size,
                      id_base, rf_out{scores_dev, ids_dev, exact_dev, flags_dev}, workspace_dev, workspace_bytes,
                      (hipStream_t)stream, nullptr);
}

extern "C" int rf_search_grouped_profile(const rf_index_t* ix, const void* filter_dev,
                                         const int32_t* group_codes_dev, int n_codes, const void* q_dev, int B,
                                         int n_groups, int group_size, int64_t id_base, float* scores_dev,
                                         int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev,
                                         void* workspace_dev, size_t workspace_bytes, void* stream,
                                         float* stage_ms_host) {
  if (!stage_ms_host) {
    rf_set_error("rf_search_grouped_profile: null stage buffer");
    return RF_ERR_INVALID;
  }
  return grouped_impl("rf_search_grouped_profile", ix, filter_dev, group_codes_dev, n_codes, q_dev, B, n_groups,
                      group_size, id_base, rf_out{scores_dev, ids_dev, exact_dev, flags_dev}, workspace_dev,
                      workspace_bytes, (hipStream_t)stream, stage_ms_host);
}

// ---- diversified search (include/ragfin.h, "diversified search") ----------------------------------
extern "C" int rf_mmr_select(const rf_index_t* ix, int B, int fetch_k, int k, double lambda, int64_t id_base,
                             const double* cand_exact_dev, const int64_t* cand_ids_dev, float* scores_dev,
                             int64_t* ids_dev, double* exact_dev, void* stream) {
  if (!ix || !cand_exact_dev || !cand_ids_dev || !scores_dev || !ids_dev) {
    rf_set_error("rf_mmr_select: null argument");
    return RF_ERR_INVALID;
  }
  if (B < 1 || k < 1 || k > fetch_k || fetch_k > RF_MAX_K) {
    rf_set_error("rf_mmr_select: need B >= 1 and 1 <= k <= fetch_k <= %d (got B = %d, k = %d, fetch_k = %d)",
                 RF_MAX_K, B, k, fetch_k);
    return RF_ERR_INVALID;
  }
  if (!(lambda >= 0.0 && lambda <= 1.0)) {   // also catches a NaN
    rf_set_error("rf_mmr_select: lambda = %g outside [0, 1]", lambda);
    return RF_ERR_INVALID;
  }
  return rf_launch_mmr(ix, B, fetch_k, k, lambda, id_base, cand_exact_dev, cand_ids_dev, scores_dev, ids_dev,
                       exact_dev, (hipStream_t)stream);
}

extern "C" int rf_merge_shards(const double* exact_dev, const int64_t* ids_dev, int W, int B, int k,
                               float* scores_out_dev, int64_t* ids_out_dev, void* stream) {
  if (!exact_dev || !ids_dev || !scores_out_dev || !ids_out_dev || W <= 0 || B <= 0 || k <= 0) {
    rf_set_error("rf_merge_shards: bad argument");
    return RF_ERR_INVALID;
  }
  return rf_launch_merge_shards(exact_dev, ids_dev, (size_t)B * k, W, B, k, scores_out_dev, ids_out_dev, nullptr, 0,
                                nullptr, (hipStream_t)stream);
}

extern "C" size_t rf_packed_shard_words(int B, int k) {
  if (B <= 0 || k <= 0) return 0;
  return (size_t)2 * B * k + ((size_t)B + 1) / 2;
}

extern "C" int rf_merge_shards_packed(const int64_t* packed_dev, int W, int B, int k,
                                      float* scores_out_dev, int64_t* ids_out_dev,
                                      uint32_t* flags_out_dev, void* stream) {
  if (!packed_dev || !scores_out_dev || !ids_out_dev || W <= 0 || B <= 0 || k <= 0) {
    rf_set_error("rf_merge_shards_packed: bad argument");
    return RF_ERR_INVALID;
  }
  // shard w = { fp64 score bits [B, k], int64 ids [B, k], uint32 flags [B] (padded to a whole word) }
  const size_t words = rf_packed_shard_words(B, k);
  return rf_launch_merge_shards((const double*)packed_dev, packed_dev + (size_t)B * k, words, W, B, k, scores_out_dev,
                                ids_out_dev, (const uint32_t*)(packed_dev + (size_t)2 * B * k), words * 2, flags_out_dev,
                                (hipStream_t)stream);
}

// local row numbers -> global ids through a table, in place (-1 = "no hit" stays -1)
__global__ void __launch_bounds__(256) k_map_ids(int64_t* __restrict__ ids, int64_t n, const int64_t* __restrict__ id_map,
                                                 int64_t n_map) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t v = ids[i];
  if (v >= 0) ids[i] = v < n_map ? id_map[v] : (int64_t)-1;
}

extern "C" int rf_map_ids(int64_t* ids_dev, int64_t n, const int64_t* id_map_dev, int64_t n_map, void* stream) {
  if (!ids_dev || n < 0 || n_map < 0 || (n_map > 0 && !id_map_dev)) {
    rf_set_error("rf_map_ids: bad argument");
    return RF_ERR_INVALID;
  }
  if (n == 0) return RF_OK;
  hipLaunchKernelGGL(k_map_ids, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ids_dev, n,
                     id_map_dev, n_map);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

extern "C" int rf_debug_scores(const rf_index_t* ix, const void* q_dev, int B, int64_t n,
                               float* out_dev, void* stream) {
  if (!ix || !q_dev || !out_dev || B <= 0 || n <= 0 || n > ix->size) {
    rf_set_error("rf_debug_scores: bad argument");
    return RF_ERR_INVALID;
  }
  return rf_launch_debug_scores(ix, q_dev, B, n, out_dev, (hipStream_t)stream);
}
