/*
 * ragfin.h -- C ABI of libragfin_hip.so: the MI355X (gfx950) engine behind the
 * vector-retrieval hot path of rag-fin.
 *
 * Every entry point replaces a call the reference makes into one of its two
 * un-vendored dependencies (sentence-transformers, pymilvus -> Milvus server);
 * the reference call site each one stands in for is cited as
 * <file>:<line> relative to the reference tree.
 *
 * Conventions
 *   - plain C: pointers, sizes, opaque handles; no C++/torch types cross the ABI.
 *   - every function returns an int status (RF_OK == 0, negative on error);
 *     rf_last_error() gives the message for the calling thread.
 *   - the CALLER owns all device memory (corpus storage, workspaces, inputs,
 *     outputs); the library owns only small host-side handles.  Nothing here
 *     calls hipMalloc/hipFree, and nothing synchronises the host with the
 *     stream: work is enqueued on `stream` (a hipStream_t passed as void*) in
 *     order, so a caller may capture it into a hipGraph.
 *   - device pointers must be 16-byte aligned.
 *   - threading: an rf_index_t / rf_encoder_t may be used by any number of host threads at
 *     once as long as each concurrent call has its OWN workspace (and normally its own
 *     stream); the handles hold no per-call state.  rf_index_add_f16 / rf_index_reset /
 *     rf_index_compact / rf_index_attach_sq8 / rf_index_detach_sq8 must not run concurrently with a
 *     search on the same index.  A process may hold indexes and
 *     encoders on several devices; the calling thread's current HIP device must be the
 *     handle's device (hipSetDevice / torch.cuda.device).
 */
#ifndef RAGFIN_H
#define RAGFIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_OK 0
#define RF_ERR_INVALID (-1)    /* bad argument (null, misaligned, out of range) */
#define RF_ERR_UNSUPPORTED (-2) /* dim / k / device not supported by the kernels */
#define RF_ERR_CAPACITY (-3)   /* index full, or workspace/storage too small */
#define RF_ERR_HIP (-4)        /* a HIP runtime call failed */
#define RF_ERR_DEVICE (-5)     /* no gfx950 device */

/* per-query flag bits written by rf_search into flags_dev */
#define RF_FLAG_CAND_OVERFLOW 1u /* candidate buffer overflowed: result not proven exact */
#define RF_FLAG_TIE_OVERFLOW 2u  /* more near-ties than the rescoring set holds */

#define RF_MAX_K 64      /* largest top-k the fused scan path serves */
#define RF_QCHUNK 64     /* queries per corpus sweep */

typedef struct rf_index rf_index_t;
typedef struct rf_encoder rf_encoder_t;
typedef struct rf_comm rf_comm_t;      /* one rank's membership of a sharded search job (RCCL communicator) */

/* ---- library ---------------------------------------------------------- */
int rf_version(void);
/* Hex digest of the sources this binary was compiled from (every .hip / .h / .cpp under csrc/ and
 * this header), stamped at build time; rag_fin_amd/_lib.py compares it with the sources on disk and
 * rebuilds (hipcc present) or refuses to load (hipcc absent) a stale library. */
const char* rf_build_id(void);
const char* rf_last_error(void);
/* RF_OK when `device` is a gfx950 part the kernels were built for. */
int rf_device_check(int device);

/* ---- corpus index: replaces the Milvus collection -----------------------
 * Reference: schema + index build "chunking_storing (1).py":14-29 (FLOAT_VECTOR
 * dim 384, COSINE); the vectors live here as fp16 in an MFMA-fragment tiled
 * layout.  The scalar fields live host-side in Python; the four that
 * filtered search tests (period, chunk_type, statement_type as dictionary codes,
 * primary_value as fp64) are mirrored on the device by the caller and handed to
 * rf_filter_eval (section "filtered search" below). */
size_t rf_index_storage_bytes(int dim, int64_t capacity_rows);
int rf_index_create(rf_index_t** out, int dim, int64_t capacity_rows,
                    void* storage_dev, size_t storage_bytes, int device);
int rf_index_destroy(rf_index_t* ix);
/* Collection.insert/flush/load -- "chunking_storing (1).py":383-396.
 * rows_dev: fp16 [n, dim] row-major.  Appends n rows (ids size .. size+n-1). */
int rf_index_add_f16(rf_index_t* ix, const void* rows_dev, int64_t n, void* stream);
/* Collection.delete(expr) / upsert: keep rows keep_rows_dev[0..n_keep) (int64, STRICTLY ascending,
 * all < size) in that order and drop the rest; row keep_rows_dev[j] becomes row j.  Afterwards
 * the index is bit-identical to one created empty and given the surviving rows with
 * rf_index_add_f16 in order: same tiles for blocks [0, ceil(n_keep/32)), pad rows of the last
 * block zero, same max_norm2 word (recomputed over the survivors, not kept).  size becomes n_keep
 * (host counter, no sync).  scratch_dev: caller-owned, 16-byte aligned, >= 32 * dim * 2 bytes; the
 * compaction runs in windows of scratch_bytes / (2 * dim) rows (rounded down to a multiple of 32),
 * so a larger scratch means fewer windows.  n_keep == 0 acts as rf_index_reset (keep_rows_dev and
 * scratch_dev may then be null); n_keep == size still rewrites the index.  Ascending order is a
 * precondition the caller checks (it is not verified on the device).  Stream-ordered; like
 * rf_index_add_f16 it must not run concurrently with a search of the same index. */
int rf_index_compact(rf_index_t* ix, const int64_t* keep_rows_dev, int64_t n_keep,
                     void* scratch_dev, size_t scratch_bytes, void* stream);
/* Collection.num_entities -- vector_rag_mcp/main.py:113,120,164 */
int64_t rf_index_size(const rf_index_t* ix);
int rf_index_dim(const rf_index_t* ix);
/* drop + recreate -- "chunking_storing (1).py":25-28 */
int rf_index_reset(rf_index_t* ix, void* stream);
/* Collection.query(expr="id in [...]") vector fetch -- graph_cons.py:308-311.
 * rows_dev: int64 [n] row numbers; out_dev: fp16 [n, dim] row-major. */
int rf_index_get_rows_f16(const rf_index_t* ix, const int64_t* rows_dev, int64_t n,
                          void* out_dev, void* stream);
/* fp32 [n, dim] -> L2-normalised fp16 [n, dim] (what COSINE needs so that the
 * scan can use the inner product).  Reference: the normalise step of
 * SentenceTransformer.encode feeding Collection.insert, same file :380-394. */
int rf_normalize_f32_to_f16(const float* in_dev, int64_t n, int dim, int normalize,
                            void* out_dev, void* stream);

/* ---- search: replaces Collection.search(..., COSINE, top_k) ---------------
 * Reference: vector_rag_mcp/main.py:51-57, retrieve.py:28-34,
 * "chunking_storing (1).py":411-417, graph_cons.py:275-281.
 *
 * q_dev      fp16 [B, dim] row-major queries (L2-normalised by the caller for
 *            COSINE; raw for inner product)
 * scores_dev fp32 [B, k]   score of rank j (descending), -inf past the end
 * ids_dev    int64 [B, k]  row id + id_base, -1 past the end
 * exact_dev  fp64 [B, k]   (nullable) the un-rounded ranking scores, used by
 *            the cross-shard merge
 * flags_dev  uint32 [B]    RF_FLAG_* bits; 0 means the result is proven equal
 *            to the exact ranking by (score desc, id asc)
 * The four output pointers may also be device-visible host memory (pinned,
 * host-coherent): the last kernel then stores the result straight into it
 * and the caller only synchronises the stream -- worthwhile for query-sized
 * results (no copy command between the kernel and the host).
 */
size_t rf_search_workspace_bytes(const rf_index_t* ix);
int rf_search(const rf_index_t* ix, const void* q_dev, int B, int k, int64_t id_base,
              float* scores_dev, int64_t* ids_dev, double* exact_dev,
              uint32_t* flags_dev, void* workspace_dev, size_t workspace_bytes,
              void* stream);
/* Profiling variant of rf_search for the FIRST corpus sweep of the batch (min(B, 64) queries,
 * or min(B, 256) where rf_search would take the wide sweep: dim 384, B > 64): same
 * launches, with HIP events around each stage.  SYNCHRONISES the stream.
 * stage_ms_host (host memory) receives {sample scan, threshold, emit scan, merge}
 * in milliseconds.  Measurement hook for bench.py; no reference counterpart. */
int rf_search_profile(const rf_index_t* ix, const void* q_dev, int B, int k, int64_t id_base,
                      float* scores_dev, int64_t* ids_dev, double* exact_dev,
                      uint32_t* flags_dev, void* workspace_dev, size_t workspace_bytes,
                      void* stream, float* stage_ms_host);
/* Slow, unconditionally exact path (fp64 scores of every row); used for the
 * queries rf_search flagged.  Same outputs. */
int rf_search_exhaustive(const rf_index_t* ix, const void* q_dev, int B, int k,
                         int64_t id_base, float* scores_dev, int64_t* ids_dev,
                         double* exact_dev, void* workspace_dev, size_t workspace_bytes,
                         void* stream);
/* Paging for limits above RF_MAX_K (the reference's hybrid consumer asks for
 * limit=1000, graph_cons.py:275-281): the next k hits ranked strictly AFTER the
 * per-query bound (after_score_dev fp64 [B], after_id_dev int64 [B] = the last hit
 * of the previous page, ids including id_base).  Exhaustive fp64 path. */
int rf_search_exhaustive_after(const rf_index_t* ix, const void* q_dev, int B, int k,
                               int64_t id_base, const double* after_score_dev,
                               const int64_t* after_id_dev, float* scores_dev, int64_t* ids_dev,
                               double* exact_dev, void* workspace_dev, size_t workspace_bytes,
                               void* stream);
/* ---- filtered search: Collection.search(..., expr=...) --------------------------------------
 * Reference: the `expr` argument of pymilvus Collection.search / query (the schema's scalar
 * fields, "chunking_storing (1).py":14-22).  rag_fin_amd/filter_expr.py parses a Milvus
 * boolean-expression subset and compiles it into the postfix program below; the scan then
 * visits only the 32-row blocks that hold a passing row and tests every candidate row's bit.
 *
 * Filter buffer (caller-owned device memory, rf_filter_bytes(n_rows) bytes, 16-byte aligned):
 *   uint32 header[4]   {n_rows, n_pass_rows, n_pass_blocks, n_tiles}
 *   uint32 mask[nblk]  nblk = ceil(n_rows / 32); bit r of word b: row 32 b + r passes;
 *                      bits past n_rows are zero
 *   uint32 blocks[nblk] the ASCENDING list of the n_pass_blocks blocks with a passing row
 *   (then scratch of the compaction: per-tile counts)
 * The header counts are written on the device; the host reads them only if it wants to.
 * Compaction is deterministic (per-tile counts, a scan, then the writes): the same mask always
 * gives the same buffer, bit for bit.
 *
 * Program: n_ops (1..RF_FILTER_MAX_OPS) rf_filter_op in HOST memory (copied into the launch's
 * arguments, so the call captures into a hipGraph), evaluated per row on a bool stack of at
 * most RF_FILTER_MAX_DEPTH entries; the program must leave exactly one value.  Leaves:
 *   RF_FOP_CODESET  column c in 0..2: the row's int32 dictionary code x passes iff
 *                   0 <= x < 32 len and bit x of code_sets_dev[off .. off + len) is set
 *   RF_FOP_RANGE    column 3 (fp64): lo <(=) x <(=) hi, RF_FRANGE_* bits say which ends are
 *                   inclusive; IEEE comparisons, so a NaN value fails
 *   RF_FOP_ROWLIST  the row number is in row_lists_dev[off .. off + len) (sorted ascending,
 *                   binary search)
 *   RF_FOP_BITMAP   (rf_filter_eval_bitmaps only) row r passes iff (r >> 5) < len and bit r & 31 of
 *                   bitmaps_dev[off + (r >> 5)] is set: a row bitmap some earlier call on the same
 *                   stream wrote, such as rf_text_match ("keyword filters" below)
 *   RF_FOP_TRUE / RF_FOP_FALSE
 * and RF_FOP_AND / RF_FOP_OR (two operands) / RF_FOP_NOT (one).
 * columns: HOST array of RF_FILTER_COLUMNS device pointers {int32 period codes [n_rows],
 * int32 chunk_type codes, int32 statement_type codes, fp64 primary_value [n_rows]}; an entry
 * the program does not read may be NULL.  code_sets_dev / row_lists_dev may be NULL when the
 * program has no leaf of that kind.  rf_filter_eval is rf_filter_eval_bitmaps with bitmaps_dev =
 * NULL; a RF_FOP_BITMAP leaf with a NULL bitmaps_dev is RF_ERR_INVALID before any device call.
 * rf_filter_from_mask: the same buffer from a caller's own row mask (mask_dev uint32 [nblk],
 * same bit layout; bits past n_rows are ignored) -- compaction only.
 *
 * rf_search_filtered: rf_search restricted to the rows the filter passes; same outputs and
 * flag contract (flags 0 = proven equal to the exact ranking of the PASSING rows).  Fewer
 * passing rows than k: the tail is padded with -inf / -1 and flags stay 0.  The filter must
 * have been built for n_rows == rf_index_size(ix) (a header for another row count passes no
 * row).  Filtered searches run as 64-query sweeps whatever B is (no wide sweep).
 * rf_search_exhaustive_filtered: the fp64 fallback for flagged queries; after_score_dev /
 * after_id_dev are both NULL, or both set for paging above RF_MAX_K as in
 * rf_search_exhaustive_after.
 * New in this build; the reference calls Milvus without `expr` on this path. */
#define RF_FILTER_MAX_OPS 64
#define RF_FILTER_MAX_DEPTH 32
#define RF_FILTER_COLUMNS 4
#define RF_FOP_CODESET 1
#define RF_FOP_RANGE 2
#define RF_FOP_ROWLIST 3
#define RF_FOP_TRUE 4
#define RF_FOP_FALSE 5
#define RF_FOP_AND 6
#define RF_FOP_OR 7
#define RF_FOP_NOT 8
#define RF_FOP_BITMAP 9      /* row r passes iff (r >> 5) < len and bit (r & 31) of bitmaps_dev[off + (r >> 5)] is set */
#define RF_FRANGE_LO_INCL 1
#define RF_FRANGE_HI_INCL 2
typedef struct rf_filter_op {
  int32_t op;      /* RF_FOP_* */
  int32_t column;  /* CODESET: 0..2; RANGE: 3 */
  int32_t off;     /* CODESET: first word in code_sets_dev; ROWLIST: first entry in row_lists_dev;
                      BITMAP: first word in bitmaps_dev */
  int32_t len;     /* CODESET, BITMAP: words; ROWLIST: entries */
  int32_t flags;   /* RANGE: RF_FRANGE_* bits */
  int32_t pad;
  double lo, hi;   /* RANGE bounds */
} rf_filter_op;
size_t rf_filter_bytes(int64_t n_rows);
int rf_filter_eval(const rf_filter_op* ops, int n_ops, const uint32_t* code_sets_dev,
                   const uint32_t* row_lists_dev, const void* const* columns, int64_t n_rows,
                   void* filter_dev, void* stream);
int rf_filter_eval_bitmaps(const rf_filter_op* ops, int n_ops, const uint32_t* code_sets_dev,
                           const uint32_t* row_lists_dev, const uint32_t* bitmaps_dev,
                           const void* const* columns, int64_t n_rows, void* filter_dev, void* stream);
int rf_filter_from_mask(const uint32_t* mask_dev, int64_t n_rows, void* filter_dev, void* stream);
int rf_search_filtered(const rf_index_t* ix, const void* filter_dev, const void* q_dev, int B, int k,
                       int64_t id_base, float* scores_dev, int64_t* ids_dev, double* exact_dev,
                       uint32_t* flags_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int rf_search_exhaustive_filtered(const rf_index_t* ix, const void* filter_dev, const void* q_dev, int B,
                                  int k, int64_t id_base, const double* after_score_dev,
                                  const int64_t* after_id_dev, float* scores_dev, int64_t* ids_dev,
                                  double* exact_dev, void* workspace_dev, size_t workspace_bytes,
                                  void* stream);
/* ---- per-query filters: one sweep for a batch whose queries differ in expr ---------------------
 * rf_search_filtered takes one filter for the whole batch.  Here every query of the batch has a
 * filter of its own, one of G <= RF_MULTI_MAX_FILTERS filter buffers built for the same n_rows, and
 * the batch still costs one sweep: over the blocks of the UNION of the G filters, each query
 * testing rows against its own filter's bits.  Query b's answer is rf_search_filtered's with filter
 * qfilter[b], bit for bit (ids, fp64 scores, fp32 scores); same flag contract, per query.
 *
 * Multi-filter buffer (caller-owned device memory, rf_multi_filter_bytes(n_rows, G) bytes, 16-byte
 * aligned; 0 for an n_rows or G out of range):
 *   the filter buffer of the union (OR of the G masks): header, mask, ascending block list and
 *   compaction scratch exactly as above, so the buffer can be read, or searched, as that filter
 *   then, from the next 256-byte boundary: uint32 masks[nblk][Gp], Gp = G rounded up to a power
 *   of two -- word [b][g] is mask word b of filter g (block-major: the words a sweep needs for one
 *   block lie side by side); the padding columns are zero
 * rf_multi_filter_build: filters is a HOST array of G device pointers (copied into the launch's
 * arguments: the call captures into a hipGraph).  A filter whose header was built for another row
 * count contributes no row.  Deterministic as the filter buffer is: no output depends on the order
 * of atomics, and every byte of the buffer is defined (what the build has no value for -- the block
 * list past its count, unused scratch, the alignment gap -- is zero), so equal filters give equal
 * buffers byte for byte.  RF_ERR_INVALID before any device call for a NULL array or entry, G outside
 * 1..RF_MULTI_MAX_FILTERS, a misaligned buffer or n_rows out of range.
 *
 * rf_search_multi_filtered: qfilter_dev int32 [B], the filter number of each query in [0, G)
 * (device memory; a number outside that range reads a padding column or another filter's, never
 * outside the buffer).  n_filters is the G the buffer was built with.  Otherwise the conventions
 * of rf_search_filtered: any B, run as 64-query sweeps; k <= RF_MAX_K; stream-ordered, no host sync,
 * captures into a hipGraph; the tail of a query with fewer passing rows than k is -inf / -1 with
 * flags 0; multi_dev must have been built for n_rows == rf_index_size(ix).  A flagged query is
 * re-run by the caller through rf_search_exhaustive_filtered with ITS filter's buffer.  No range,
 * search-after, grouping or SQ8 form.
 * New in this build; the reference calls Milvus one query at a time on this path. */
#define RF_MULTI_MAX_FILTERS 64
size_t rf_multi_filter_bytes(int64_t n_rows, int n_filters);
int rf_multi_filter_build(const void* const* filters, int n_filters, int64_t n_rows, void* multi_dev,
                          void* stream);
int rf_search_multi_filtered(const rf_index_t* ix, const void* multi_dev, int n_filters,
                             const int32_t* qfilter_dev, const void* q_dev, int B, int k, int64_t id_base,
                             float* scores_dev, int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);
/* ---- boosted search: Collection.search(..., ranker=Function(..., params={"reranker": "boost", ...})) ----
 * Milvus' Boost Ranker multiplies the score of the rows a filter selects by a weight.  Here the
 * boosted ranking is the exact top-k of the whole corpus under the boosted score (the
 * definition in numpy: rag_fin_amd/ranker.py, boost_reference).  m <= RF_BOOST_MAX boosts
 * (filter_i, weight_i) split the rows into 2^m CLASSES: bit i of a row's class c is set iff the row
 * passes filter_i, and W[c] is the product of the weights of the set bits.  With s the fp64 contract
 * score, boosted = W[class] * s (one fp64 multiplication) and rows rank by (boosted desc, s desc,
 * row asc).  Inside a class that order is the plain (s desc, row asc) one, so the boosted top-k is
 * the top-k of the union of every class's plain filtered top-k: the caller runs the classes as
 * queries of rf_search_multi_filtered (or rf_search_filtered) and merges their answers.
 *
 * rf_boost_classes: the class masks of m filter buffers built for n_rows (boost_filters: a HOST array
 * of m device pointers, copied into the launch's arguments), within the rows of base_filter_dev when
 * that is not NULL.  class_masks_dev uint32 [2^m][stride], stride = rf_boost_class_stride_words(n_rows)
 * (ceil(n_rows / 32) rounded up to a multiple of 4, so every class mask is 16-byte aligned; 0 for an
 * n_rows outside 1..2^32 - 33): word w of class c = base[w] AND, for each i, F_i[w] when bit i of c is
 * set and NOT F_i[w] otherwise -- the mask format of the filter buffer, ready for rf_filter_from_mask.
 * Bits at positions >= n_rows and the words from ceil(n_rows / 32) to the stride are ZERO in every
 * class.  class_counts_dev int64 [2^m]: the rows of each class (integer sums: independent of the order
 * of the atomics); they add up to the rows the base filter passes.  A filter buffer whose header was
 * built for another row count contributes no row.  Stream-ordered, no allocation, captures into a
 * hipGraph; the same inputs give the same bytes.  RF_ERR_INVALID before any device call: a NULL array,
 * entry or output, m outside 1..RF_BOOST_MAX, a filter or class_masks_dev not 16-byte aligned,
 * class_counts_dev not 8-byte aligned, n_rows out of range.
 *
 * rf_merge_boosted: per query b the C <= 8 class answers exact_dev fp64 / ids_dev int64 [B, C, k_in]
 * (the outputs of the class searches; an id < 0 is padding, ids are distinct within a query) ->
 * the best k candidates by (boosted desc, s desc, id asc), boosted = class_weight[c] * s as ONE fp64
 * multiplication (never contracted), as scores_dev = (float)boosted, ids_out_dev, boosted_dev and
 * base_dev = s ([B, k]; the two fp64 outputs may be NULL); the tail is -inf / -1 / -inf / -inf.
 * class_weight_host: C doubles in HOST memory (they travel in the launch arguments), finite and > 0.
 * One workgroup per query, the C k_in <= 512 candidates ranked by counting in LDS; no workspace,
 * stream-ordered, captures into a hipGraph.  RF_ERR_INVALID before any device call: a NULL argument
 * (but the two nullable ones), B < 1, C outside 1..8, k or k_in outside 1..RF_MAX_K, a weight that is
 * not finite or not > 0.
 * New in this build; the reference calls Milvus without a ranker on this path. */
#define RF_BOOST_MAX 3
size_t rf_boost_class_stride_words(int64_t n_rows);
int rf_boost_classes(const void* base_filter_dev, const void* const* boost_filters, int m, int64_t n_rows,
                     uint32_t* class_masks_dev, int64_t* class_counts_dev, void* stream);
int rf_merge_boosted(const double* exact_dev, const int64_t* ids_dev, int B, int C, int k_in,
                     const double* class_weight_host, int k, float* scores_dev, int64_t* ids_out_dev,
                     double* boosted_dev, double* base_dev, void* stream);
/* ---- decayed search: Collection.search(..., ranker=Function(..., params={"reranker": "decay", ...})) ----
 * Milvus' decay rankers scale a score by how far a numeric field's value lies from an origin.  The
 * weight differs row by row, so the exact decayed top-k is no merge of plain top-k lists: the sweep
 * itself runs on the weighted score (the definitions in numpy: rag_fin_amd/ranker.py,
 * decay_weights_reference and decay_reference).
 *
 * rf_decay_weights: one weight per row of a device column (int64 when column_is_int64, rounded to the
 * nearest double, else fp64).  d = max(0, |v - origin| - offset);
 *   RF_DECAY_GAUSS   w = 2^-(shape (d / scale)^2)      shape = -log2(decay)
 *   RF_DECAY_EXP     w = 2^-(shape (d / scale))        shape = -log2(decay)
 *   RF_DECAY_LINEAR  w = max(0, (shape - d) / shape)   shape = scale / (1 - decay)
 * so w is in [0, 1], 1 within `offset` of the origin and `decay` at distance offset + scale; a NaN value
 * weighs 0.  Every step is one IEEE fp64 operation and 2^-t is defined by its arithmetic (0 unless
 * t < 1100; n = floor(t + 0.5), the degree-13 Taylor polynomial of e^x at x = -(t - n) ln2 in Horner
 * form, scaled by 2^-n as ldexp does), so w64_dev [n_rows] is bit for bit the numpy definition and
 * w32_dev [n_rows] its rounding to nearest.  Stream-ordered, no allocation, captures into a hipGraph.
 * RF_ERR_INVALID before any device call: a NULL or misaligned pointer, n_rows outside 0..2^32 - 33, an
 * unknown function, an origin that is not finite, a scale or shape that is not finite and > 0, an
 * offset that is not finite and >= 0.
 *
 * rf_search_weighted: per query the best k rows (of the rows filter_dev passes; NULL: of all rows)
 * by (decayed desc, s desc, row asc), with s the fp64 contract score and decayed = w64[row] * s as ONE
 * fp64 multiplication; scores_dev = (float)decayed, decayed_dev and base_dev = s may be NULL, the
 * tail is -inf / -1 / -inf / -inf.  PRECONDITION: every weight lies in [0, 1] -- no NaN, nothing above
 * 1 -- and w32[row] is w64[row] rounded to nearest (what rf_decay_weights writes); w32_dev [n_rows]
 * 16-byte, w64_dev [n_rows] 8-byte aligned.  One sweep of the fp16 rows per 64 queries (the masked
 * 64-query chain; an attached SQ8 shadow is not used): sample, threshold, emit and merge all see
 * fl32(w32[row] * MFMA score), which lies within eps_w = 2 eps of decayed, so eps_w stands wherever
 * rf_search uses eps.  A negative score is multiplied like any other: a small weight moves it
 * towards 0, i.e. up.  Flags, workspace (rf_search_workspace_bytes), stream order and capture as for
 * rf_search_filtered; a flagged query is re-run by the caller through
 * rf_search_exhaustive_weighted, the fp64 kernel over the same rows and weights (no flags; it uses
 * the workspace's candidate area for its lists).  No range, search-after, per-query-filter, grouping
 * or SQ8 form.
 * New in this build; the reference calls Milvus without a ranker on this path. */
#define RF_DECAY_GAUSS 0
#define RF_DECAY_EXP 1
#define RF_DECAY_LINEAR 2
int rf_decay_weights(const void* column_dev, int column_is_int64, int64_t n_rows, int function, double origin,
                     double scale, double offset, double shape, double* w64_dev, float* w32_dev, void* stream);
int rf_search_weighted(const rf_index_t* ix, const void* filter_dev, const float* w32_dev, const double* w64_dev,
                       const void* q_dev, int B, int k, int64_t id_base, float* scores_dev, int64_t* ids_dev,
                       double* decayed_dev, double* base_dev, uint32_t* flags_dev, void* workspace_dev,
                       size_t workspace_bytes, void* stream);
int rf_search_exhaustive_weighted(const rf_index_t* ix, const void* filter_dev, const float* w32_dev,
                                  const double* w64_dev, const void* q_dev, int B, int k, int64_t id_base,
                                  float* scores_dev, int64_t* ids_dev, double* decayed_dev, double* base_dev,
                                  void* workspace_dev, size_t workspace_bytes, void* stream);
/* ---- range search: Collection.search(..., param={"params": {"radius": r, "range_filter": f}}) ----
 * The best k hits whose score lies in the band  radius < score <= range_filter  (COSINE / IP:
 * higher is better), i.e. the (score desc, row asc) ranking of rf_search with every row outside
 * the band removed.  Band membership is decided on the contract score -- the fp64 value exact_dev
 * receives -- against the two bounds as fp64: not on the MFMA score and not on the fp32 rounding
 * of the score (so a returned fp32 score may EQUAL (float)radius: its fp64 value is above it).
 * radius may be -INFINITY (a band with only a ceiling) and range_filter +INFINITY (only a floor);
 * radius >= range_filter or a NaN returns RF_ERR_INVALID.  Fewer band rows than k: the tail is
 * -inf / -1 and flags stay 0 (an empty band is a proven answer).
 * filter_dev: NULL, or a filter buffer as for rf_search_filtered -- the band within the passing
 * rows.  Otherwise the conventions of rf_search_filtered: stream-ordered, no host sync, captures
 * into a hipGraph (the bounds travel in the launch arguments), outputs may be pinned host memory,
 * flags 0 = proven equal to the exact ranking of the band, non-zero (RF_FLAG_*) = answer that
 * query through rf_search_exhaustive_range.  Workspace: rf_search_workspace_bytes.
 * What runs: 64-query sweeps whatever B is (no wide band kernel); the sample pass clips at the
 * ceiling, the threshold has the floor of the band under it, the emit appends only rows between
 * the two, and the merge drops what the fp64 scores put outside the band.  No
 * sample fold and no SQ8 form: an index with an SQ8 shadow answers a range search from its fp16
 * rows.  Corpora of <= 8192 rows skip the sample pass as in rf_search (every row at or above
 * the floor and at or below the ceiling is a candidate).
 * rf_search_exhaustive_range: the fp64 kernel with the eligibility test radius < a <=
 * range_filter; after_score_dev / after_id_dev are both NULL, or both set for paging above
 * RF_MAX_K as in rf_search_exhaustive_after.  No flags: its answer is exact by construction.
 * New in this build; the reference calls Milvus without range parameters on this path. */
int rf_search_range(const rf_index_t* ix, const void* filter_dev, const void* q_dev, int B, int k,
                    int64_t id_base, double radius, double range_filter, float* scores_dev,
                    int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev, void* workspace_dev,
                    size_t workspace_bytes, void* stream);
int rf_search_exhaustive_range(const rf_index_t* ix, const void* filter_dev, const void* q_dev, int B,
                               int k, int64_t id_base, double radius, double range_filter,
                               const double* after_score_dev, const int64_t* after_id_dev,
                               float* scores_dev, int64_t* ids_dev, double* exact_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream);
/* ---- paged search: Collection.search(..., offset=o) / Collection.search_iterator(...) -------------
 * "The next k hits after hit X": per query b the best k rows by (fp64 contract score desc, row asc)
 * among the rows that
 *   - pass filter_dev (NULL: every row),
 *   - lie in the band  radius < a <= range_filter  (-INFINITY / +INFINITY leave a side open; both
 *     open: no band), decided on the fp64 score as in rf_search_range, and
 *   - rank strictly AFTER the bound: a < after_score_dev[b], or a == after_score_dev[b] and
 *     row + id_base > after_id_dev[b] -- the rule of rf_search_exhaustive_after.
 * after_score_dev fp64 [B], after_id_dev int64 [B] (ids WITH the id base), device memory, read by
 * the kernels in stream order (the previous page's last hit can feed them without a host sync).
 * A bound score of +inf makes every row eligible (the answer of rf_search_range / rf_search); a
 * bound (-inf, any id) makes none eligible: all padding (-inf / -1), flags 0.  A NaN bound gives
 * an unspecified page (never an out-of-range access).
 * Conventions of rf_search_range: stream-ordered, no host sync, no allocation, outputs may be
 * pinned host memory, workspace rf_search_workspace_bytes, 64-query sweeps whatever B is (no wide
 * sweep, no sample fold, no SQ8 form; for B > 64 each sweep reads its own 64 bounds), flags 0 =
 * proven equal to the exact ranking of the eligible rows, non-zero (RF_FLAG_*) = answer that query
 * through rf_search_exhaustive_range / _filtered / _after with the same filter, band and bound.
 * More than 256 rows tied at the bound's score (within the sweep's error bound) raise
 * RF_FLAG_TIE_OVERFLOW.
 * RF_ERR_INVALID before any device call: a NULL bound array, radius >= range_filter or a NaN, k
 * outside 1..RF_MAX_K, and the argument errors of rf_search.
 * What runs: the band chain of rf_search_range with a per-query ceiling min(range_filter, bound
 * score); the sample pass and the merge's k-th cut count only rows strictly below the bound score,
 * and the merge drops every rescored row at or before the bound by the fp64 (score, id) rule
 * (DESIGN 4.4i).  A page costs one sweep of the corpus whatever its depth.
 * rf_search_after_profile: the first sweep alone with HIP events around its stages (4 floats:
 * sample, threshold, emit, merge; synchronises).
 * New in this build; the reference pages through Milvus (offset / search_iterator). */
int rf_search_after(const rf_index_t* ix, const void* filter_dev, const void* q_dev, int B, int k,
                    int64_t id_base, double radius, double range_filter,
                    const double* after_score_dev, const int64_t* after_id_dev,
                    float* scores_dev, int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);
int rf_search_after_profile(const rf_index_t* ix, const void* filter_dev, const void* q_dev, int B, int k,
                            int64_t id_base, double radius, double range_filter,
                            const double* after_score_dev, const int64_t* after_id_dev,
                            float* scores_dev, int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev,
                            void* workspace_dev, size_t workspace_bytes, void* stream, float* stage_ms_host);
/* ---- grouping search: Collection.search(..., group_by_field=f, group_size=s) -----------------------
 * The best n_groups GROUPS instead of the best k rows: a group is the set of rows that share a
 * code (the caller's int32 dictionary code of the group-by field, one per row), its rows are ranked
 * by (fp64 contract score desc, row asc) as everywhere else and it keeps its first
 * min(group_size, rows of the group); groups are ranked by their best row under the same rule.
 *   group_codes_dev  int32 [rf_index_size(ix)] on the device.  A code outside [0, n_codes) is a row
 *                    without a group: it is never returned.
 *   n_codes          size of the dictionary, 1..RF_GROUP_MAX_CODES for this fused path; above it
 *                    RF_ERR_UNSUPPORTED (the caller answers group by group through
 *                    rf_search_exhaustive_filtered).  The cap comes from the LDS budget of the sweep
 *                    at dim 1024: 128 KiB of query fragments + a 64-code x 64-query fp32 table
 *                    (16 KiB) + 6 KiB of staging, of 160 KiB.
 *   n_groups, group_size   n_groups * group_size <= RF_MAX_K and both >= 1, else RF_ERR_INVALID
 *                    (so is a null group_codes_dev).
 *   filter_dev       NULL, or a filter buffer as for rf_search_filtered: groups are formed among the
 *                    passing rows only (a group without a passing row does not exist).
 * Outputs are [B, n_groups * group_size] (flags: [B]): the group of rank j occupies slots
 * [j * group_size, (j + 1) * group_size), best row first; a short group and missing groups are
 * padded with -inf / -1.  flags 0 = proven equal to the exact grouped ranking; non-zero (RF_FLAG_*)
 * = answer that query group by group through the exhaustive kernel.
 * Otherwise the conventions of rf_search_filtered: stream-ordered, no host sync, captures into a
 * hipGraph, outputs may be pinned host memory, 64-query sweeps whatever B is.
 * What runs per sweep: a sweep of every (passing) block that keeps the maximum MFMA
 * score per (query, code) and workgroup, a threshold per (query, code) -- +inf for a group that
 * cannot be among the first n_groups --, the same sweep again appending every row that reaches
 * the threshold of its own group, and a merge that rescored in fp64.  The corpus is read twice,
 * whatever its size (no small-corpus shortcut, no sample fold, no SQ8 form: an index with an SQ8
 * shadow answers from its fp16 rows).  workspace_bytes >= rf_search_grouped_workspace_bytes
 * (> rf_search_sq8_workspace_bytes; its leading part is the rf_search workspace).
 * rf_search_grouped_profile: the first sweep with HIP events: stage_ms_host (host) receives
 * {group-maximum sweep, threshold, emit sweep, merge} in ms; SYNCHRONISES.
 * rf_debug_grouped_counters_offset: test hook -- byte offset in the workspace of the uint32
 * [64][8] candidate counters, which a grouped search leaves as its last sweep wrote them (list
 * capacity 2048 each).
 * New in this build; the reference calls Milvus without group_by_field on this path. */
#define RF_GROUP_MAX_CODES 64
size_t rf_search_grouped_workspace_bytes(const rf_index_t* ix);
int rf_search_grouped(const rf_index_t* ix, const void* filter_dev, const int32_t* group_codes_dev, int n_codes,
                      const void* q_dev, int B, int n_groups, int group_size, int64_t id_base,
                      float* scores_dev, int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);
int rf_search_grouped_profile(const rf_index_t* ix, const void* filter_dev, const int32_t* group_codes_dev,
                              int n_codes, const void* q_dev, int B, int n_groups, int group_size,
                              int64_t id_base, float* scores_dev, int64_t* ids_dev, double* exact_dev,
                              uint32_t* flags_dev, void* workspace_dev, size_t workspace_bytes, void* stream,
                              float* stage_ms_host);
size_t rf_debug_grouped_counters_offset(void);
/* ---- diversified search: maximal-marginal-relevance re-ranking of a search's answer ----------------
 * What RAG clients do after Collection.search (LangChain's max_marginal_relevance_search: search
 * fetch_k hits, query() their vectors back, a numpy loop), as one stage on the device: it picks k
 * of the fetch_k candidates of a search, trading relevance against similarity to what is already
 * picked.  The candidates are the [B, fetch_k] outputs of ANY search entry point above for
 * k = fetch_k (plain, filtered, range, SQ8, exhaustive): their ids (id_base included, -1 padded)
 * and their fp64 ranking scores (exact_dev), in that search's order.
 * Definition, per query (1 <= k <= fetch_k <= RF_MAX_K, lambda in [0, 1],
 * mu = 1.0 - lambda in fp64): candidate i has the score s_i; g(i, j) is the contract dot product of
 * the fp16 rows of candidates i and j (the cosine for normalised rows); m_i = -inf.  Each round
 * computes v_i = (lambda * s_i) - pen_i for every unselected i, pen_i = 0.0 in the first round and
 * mu * m_i afterwards, the two products and the subtraction each rounded to fp64 on its own (no
 * fma); the pick is the largest v_i, the smallest i on a tie; then m_i = max(m_i, g(i, pick)).
 * min(k, real candidates) rounds.  Output slot t holds the t-th pick: (float(s), id, s) -- the
 * RELEVANCE score, in MMR order; the remaining slots are -inf / -1.  lambda = 1 reproduces the
 * first k candidates; the first pick is always the best hit.  An id that is negative or whose row
 * (id - id_base) is not in the index is treated as absent.  Non-finite candidate scores:
 * unspecified.
 * Conventions of rf_search: stream-ordered, no host sync, no allocation, no workspace, captures
 * into a hipGraph, outputs may be pinned host memory.  RF_ERR_INVALID: a null pointer (exact_dev
 * may be NULL), B < 1, k < 1, k > fetch_k, fetch_k > RF_MAX_K, lambda outside [0, 1] or NaN --
 * checked on the host before any device call.  The flags of the candidate search still decide
 * whether a query's candidates are proven exact: re-run a flagged query, then this stage on it.
 * One workgroup per query; the candidate rows are staged once in LDS (fetch_k x (dim * 2 + 16)
 * bytes, 129 KiB at dim 1024 and fetch_k 64), the rounds read LDS only.
 * New in this build; the reference has no re-ranking stage. */
int rf_mmr_select(const rf_index_t* ix, int B, int fetch_k, int k, double lambda, int64_t id_base,
                  const double* cand_exact_dev, const int64_t* cand_ids_dev, float* scores_dev,
                  int64_t* ids_dev, double* exact_dev, void* stream);
/* ---- lexical search: BM25 over posting lists, and reciprocal-rank fusion of several searches --------
 * What RAG stacks put beside the dense retriever (Milvus: a BM25 sparse field, hybrid_search with
 * RRFRanker; LangChain: EnsembleRetriever).  The caller builds the postings on the host
 * (rag_fin_amd/lexical.py) and owns the device arrays, like the index storage:
 *   post_off  int64  [n_terms + 1]  term t's postings are [post_off[t], post_off[t + 1])
 *   post_row  uint32 [nnz]          rows holding the term, ASCENDING within a term
 *   post_imp  fp32   [nnz]          the BM25 impact of (term, row): idf * tf-saturation, computed in
 *                                   fp64 on the host and rounded to fp32 once; positive and normal
 * A batch of queries is CSR on the device: q_off int32 [B + 1], q_term int32 (a query's distinct term
 * ids, ascending), q_weight fp32 (the count of the term in the query); at most RF_SPARSE_MAX_TERMS
 * terms per query (the kernel reads no more than that of a longer one).
 * Score of row r:  acc = 0.0f; for the query's terms in order, if the term is in r:
 * acc = acc + (w * imp), the product and the sum each rounded to fp32 on its own (no fma).  A row is
 * a hit iff it holds a query term (acc > 0) and its bit is set in the filter, if one is given.
 * Ranking (score desc, row asc); outputs as rf_search: scores_dev fp32 [B, k], ids_dev int64 [B, k]
 * (row + id_base), exact_dev fp64 [B, k] (nullable) = (double)score, padded with -inf / -1.  No flags
 * and no fallback: the summation order is fixed, so the answer is exact by construction and has the
 * same bits on every run and for every B.
 *   rf_sparse_create    host-side handle over the caller's arrays (checked on the host: non-null,
 *                       16-byte aligned, 1 <= n_rows < 2^31, n_terms >= 1, nnz >= 1); no device call
 *   rf_sparse_search    stream-ordered, no host sync, no allocation, captures into a hipGraph,
 *                       1 <= k <= RF_MAX_K, 1 <= B <= 65535; RF_ERR_INVALID before any device call.
 *                       filter_dev: NULL or a filter buffer as for rf_search_filtered (mask bits only;
 *                       a header built for another row count passes no row).
 *                       workspace_bytes >= rf_sparse_search_workspace_bytes(sp, B, k).
 * What runs: grid (row tiles, B); a workgroup owns RF_SPARSE_TILE_ROWS consecutive rows as fp32
 * accumulators in LDS, finds each term's slice of postings inside its tile by binary search, adds
 * term after term with a barrier in between (rows within a term are distinct: plain read-modify-
 * writes, no atomics), and selects its own top k into the workspace; a second launch, one workgroup
 * per query, merges the tiles' lists.  A posting whose row is outside the tile or the index is
 * skipped: malformed postings give wrong scores, never an out-of-range access.
 *
 * rf_fuse_rrf: weighted reciprocal-rank fusion of A <= RF_FUSE_MAX_ARMS answers.  ids_dev int64
 * [A, B, F]: arm a's ids for query b in that search's order (-1 = padding), F <= RF_MAX_K.
 *   fused(d) = sum over the arms a, in arm order, that hold d of  weights[a] / (rrf_k + rank_a(d)),
 * rank_a(d) 1-based (the first occurrence, should an arm repeat an id), each division rounded to fp64
 * on its own, the sum in fp64.  weights_host: A doubles in HOST memory (they travel in the launch
 * arguments), finite and >= 0, NULL = all 1.0; rrf_k finite and > 0.  The best k distinct ids by
 * (fused desc, id asc) go out as (float(fused), id, fused), padded with -inf / -1; 1 <= k <= RF_MAX_K.
 * One workgroup per query, the A F <= 256 candidates deduplicated in LDS; no workspace.
 * New in this build; the reference has no lexical arm and no fusion stage. */
#define RF_SPARSE_MAX_TERMS 64
#define RF_SPARSE_TILE_ROWS 8192
#define RF_FUSE_MAX_ARMS 4
typedef struct rf_sparse rf_sparse_t;
int rf_sparse_create(rf_sparse_t** out, int64_t n_rows, int64_t n_terms, int64_t nnz,
                     const int64_t* post_off_dev, const uint32_t* post_row_dev, const float* post_imp_dev,
                     int device);
int rf_sparse_destroy(rf_sparse_t* sp);
size_t rf_sparse_search_workspace_bytes(const rf_sparse_t* sp, int B, int k);
int rf_sparse_search(const rf_sparse_t* sp, const void* filter_dev, const int32_t* q_off_dev,
                     const int32_t* q_term_dev, const float* q_weight_dev, int B, int k, int64_t id_base,
                     float* scores_dev, int64_t* ids_dev, double* exact_dev, void* workspace_dev,
                     size_t workspace_bytes, void* stream);
int rf_fuse_rrf(int A, const int64_t* ids_dev, int F, const double* weights_host, double rrf_k, int B, int k,
                float* scores_dev, int64_t* ids_dev_out, double* exact_dev, void* stream);
/* ---- keyword filters: TEXT_MATCH / PHRASE_MATCH as leaves of a filter expression ------------------
 * Milvus pairs its BM25 field with TEXT_MATCH(field, 'terms' [, minimum_should_match=N]) and
 * PHRASE_MATCH(field, 'a b c') in `expr`.  rf_text_match turns the posting lists of an rf_sparse_t
 * into one row bitmap per leaf, which a RF_FOP_BITMAP leaf of rf_filter_eval_bitmaps then reads
 * (the definition in numpy: rag_fin_amd/lexical.py, text_match_reference).
 *   RF_TEXT_MATCH   terms: DISTINCT term ids, ascending.  Row r passes iff at least min_match of
 *                   them have a posting for r.
 *   RF_TEXT_PHRASE  terms: the phrase p_0 .. p_{m-1} in order, repeats allowed (min_match is not
 *                   read).  Row r passes iff some position j has term p_i at position j + i of r for
 *                   every i.  Needs the positions: for posting q (in post_row order), the ASCENDING
 *                   token positions pos[pos_off[q] .. pos_off[q + 1]) of that term in that row
 *                   (pos_off int64 [nnz + 1], pos uint32 [n_pos], caller-owned device memory, attached
 *                   once by rf_sparse_attach_positions: host-checked, no device call).
 * A term id outside [0, n_terms) has no postings.  leaves_host: n_leaves (1..RF_TEXT_MAX_LEAVES)
 * leaves in HOST memory (they travel in the launch arguments); leaf l reads terms_dev[term_off ..
 * term_off + n_terms), 1 <= n_terms <= RF_SPARSE_MAX_TERMS, inside [0, n_terms_total), and writes
 * EVERY word of bitmaps_dev[l * words_per_leaf .. (l + 1) * words_per_leaf), words_per_leaf >=
 * ceil(n_rows / 32); bits past n_rows are zero.  Stream-ordered, no host sync, no allocation;
 * workspace_bytes >= rf_text_match_workspace_bytes(sp, n_leaves) (0 = n_leaves out of range).
 * RF_ERR_INVALID before any device call: n_leaves, a leaf's kind, n_terms, term range or min_match
 * (< 1) out of range, a PHRASE leaf on a handle without positions, a workspace that is too small, a
 * NULL pointer, bitmaps_dev / workspace_dev not 16-byte aligned, terms_dev not 4-byte aligned.
 * What runs: one small launch clamps every term's posting range and marks the repeats of a term;
 * then grid (row tiles of RF_SPARSE_TILE_ROWS, leaves): a workgroup counts, per tile row in LDS, the
 * leaf's distinct terms that hold the row (term after term with a barrier in between, rows within
 * a term are distinct: no atomics on a counter), a PHRASE leaf then verifies adjacency for the rows
 * that hold every term (binary searches in the position lists), and each wave ballots 64 rows into
 * two words.  Integers only: the same bits on every run.  Offsets and rows are clamped as in
 * rf_sparse_search: malformed postings give wrong bits, never an out-of-range access.
 * New in this build; the reference filters on no text. */
#define RF_TEXT_MATCH 1
#define RF_TEXT_PHRASE 2
#define RF_TEXT_MAX_LEAVES 16
typedef struct rf_text_leaf {
  int32_t kind;       /* RF_TEXT_MATCH | RF_TEXT_PHRASE */
  int32_t term_off;   /* first entry in terms_dev */
  int32_t n_terms;    /* 1..RF_SPARSE_MAX_TERMS */
  int32_t min_match;  /* MATCH: >= 1; PHRASE: >= 1, not read */
} rf_text_leaf;
int rf_sparse_attach_positions(rf_sparse_t* sp, const int64_t* pos_off_dev, const uint32_t* pos_dev, int64_t n_pos);
size_t rf_text_match_workspace_bytes(const rf_sparse_t* sp, int n_leaves);
int rf_text_match(const rf_sparse_t* sp, const rf_text_leaf* leaves_host, int n_leaves, const int32_t* terms_dev,
                  int64_t n_terms_total, uint32_t* bitmaps_dev, int64_t words_per_leaf, void* workspace_dev,
                  size_t workspace_bytes, void* stream);
/* ---- user-defined scalar fields: the leaves of `expr` over a collection's own columns --------------
 * A pymilvus user declares FieldSchemas of their own next to the reference's seven
 * (rag_fin_amd/schema.py: VARCHAR, INT64, DOUBLE, BOOL).  The filter program above reads four
 * hard-wired columns; a leaf over any other column is evaluated here into a row bitmap, which a
 * RF_FOP_BITMAP leaf of rf_filter_eval_bitmaps then reads -- the door rf_text_match uses.
 * Leaf kinds (column_dev: the leaf's column in device memory, [n_rows], aligned to its element):
 *   RF_CLEAF_CODESET    int32 dictionary codes (VARCHAR, BOOL): row passes iff its code x has
 *                       0 <= x < 32 len and bit x of code_sets_dev[off .. off + len) is set
 *   RF_CLEAF_I64_RANGE  int64 values: ilo <= x <= ihi, both ends inclusive (ilo > ihi passes nothing)
 *   RF_CLEAF_I64_SET    int64 values: x is in value_sets_dev[off .. off + len) (sorted ascending,
 *                       binary search), len <= RF_COLUMN_MAX_SET
 *   RF_CLEAF_F64_RANGE  fp64 values: flo <(=) x <(=) fhi, RF_FRANGE_* bits in flags say which ends
 *                       are inclusive; IEEE comparisons, so a NaN value fails
 * leaves_host: n_leaves (1..RF_COLUMN_MAX_LEAVES) leaves in HOST memory (they travel in the launch
 * arguments, so the call captures into a hipGraph); leaf l writes EVERY word of bitmaps_dev[l * nwords ..
 * (l + 1) * nwords), nwords = ceil(n_rows / 32): bit r & 31 of word r >> 5 = row r passes; bits past
 * n_rows are zero, so the caller need not clear the buffer.  One launch for all leaves, grid (row chunks,
 * leaves): a lane owns one row, a wave's 64 predicates become two words by ballot.  Stream-ordered, no
 * host sync, no allocation, no atomics; integers and IEEE comparisons only: the same bits on every run.
 * RF_ERR_INVALID before any device call: a NULL leaves_host / bitmaps_dev, n_leaves or n_rows out of
 * range, an unknown kind, a negative off or len, a set of more than RF_COLUMN_MAX_SET values, a leaf
 * that needs code_sets_dev / value_sets_dev when that is NULL, unknown flags, a column that is NULL or
 * misaligned.  A code or a search position outside the leaf's [off, off + len) is never dereferenced.
 * n_rows == 0 writes nothing and returns RF_OK.
 * New in this build; the reference's collection carries no field of its own. */
#define RF_COLUMN_MAX_LEAVES 16
#define RF_COLUMN_MAX_SET 65536
#define RF_CLEAF_CODESET 1
#define RF_CLEAF_I64_RANGE 2
#define RF_CLEAF_I64_SET 3
#define RF_CLEAF_F64_RANGE 4
typedef struct rf_column_leaf {
  int32_t kind;            /* RF_CLEAF_* */
  int32_t flags;           /* F64_RANGE: RF_FRANGE_* bits */
  const void* column_dev;  /* int32 codes | int64 | fp64, [n_rows] */
  int64_t off;             /* CODESET: first word in code_sets_dev; I64_SET: first entry in value_sets_dev */
  int64_t len;             /* CODESET: words; I64_SET: entries */
  int64_t ilo, ihi;        /* I64_RANGE bounds, inclusive */
  double flo, fhi;         /* F64_RANGE bounds */
} rf_column_leaf;
int rf_column_match(const rf_column_leaf* leaves_host, int n_leaves, const uint32_t* code_sets_dev,
                    const int64_t* value_sets_dev, int64_t n_rows, uint32_t* bitmaps_dev, void* stream);
/* ---- dynamic fields: the leaves of `expr` over schemaless metadata, typed per row ---------------------
 * pymilvus' enable_dynamic_field: a row may carry keys the schema does not declare, and two rows may hold
 * values of different types under one key, or none.  The device mirror of one key is a tagged column:
 *   tags_dev     uint8 [n_rows]: RF_DTAG_ABSENT (the row lacks the key) | BOOL | INT | DOUBLE | STRING
 *   payload_dev  8 bytes [n_rows], 8-byte aligned: the int64 value, the fp64 bits, a bool as 0 / 1, or the
 *                string's code into the key's append-only dictionary (as an int64 >= 0); unread for ABSENT
 * A leaf is evaluated into a row bitmap that an RF_FOP_BITMAP leaf of rf_filter_eval_bitmaps reads -- the
 * door rf_text_match and rf_column_match use.  Leaf kinds:
 *   RF_DLEAF_TAGS         the row's tag t has bit t of flags set (flags: 8 bits; a tag >= 8 fails)
 *   RF_DLEAF_STR_CODESET  tag STRING and the code x has 0 <= x < 32 len and bit x of
 *                         code_sets_dev[off .. off + len) set
 *   RF_DLEAF_BOOL         tag BOOL and the value v (0 / 1; anything else fails) has bit v of flags set
 *   RF_DLEAF_NUM_RANGE    tag INT: ilo <= x <= ihi, both ends inclusive (ilo > ihi passes no INT row);
 *                         tag DOUBLE: flo <(=) x <(=) fhi, RF_FRANGE_* bits in flags say which ends are
 *                         inclusive, IEEE comparisons, so a NaN value fails
 *   RF_DLEAF_NUM_SET      tag INT: x is in int_sets_dev[off .. off + len); tag DOUBLE: x equals (IEEE ==) an
 *                         entry of f64_sets_dev[foff .. foff + flen); both sorted ascending, binary search,
 *                         at most RF_COLUMN_MAX_SET entries each
 * A row whose tag the kind does not name fails.  Otherwise the contract of rf_column_match: leaves_host is
 * HOST memory, n_leaves in 1..RF_DYNAMIC_MAX_LEAVES (they travel in the launch arguments, so the call
 * captures into a hipGraph); leaf l writes EVERY word of bitmaps_dev[l * nwords .. (l + 1) * nwords),
 * nwords = ceil(n_rows / 32), bits past n_rows zero; one launch, grid (row chunks, leaves), a lane owns a
 * row, a wave's 64 predicates become two words by ballot; stream-ordered, no host sync, no allocation, no
 * atomics; integers and IEEE comparisons only: the same bits on every run.
 * RF_ERR_INVALID before any device call: a NULL leaves_host / bitmaps_dev, n_leaves or n_rows out of range,
 * an unknown kind, flags outside the kind's bits, a negative or too large off / len / foff / flen, a leaf
 * that needs code_sets_dev / int_sets_dev / f64_sets_dev when that is NULL, a misaligned set or bitmap
 * pointer, tags_dev NULL, payload_dev NULL (any kind but TAGS) or not 8-byte aligned.  A set of length 0 is
 * legal and passes nothing; a code or a search position outside the leaf's slice is never dereferenced.
 * n_rows == 0 writes nothing and returns RF_OK.
 * New in this build; the reference's collection has no dynamic field. */
#define RF_DYNAMIC_MAX_LEAVES 16
#define RF_DTAG_ABSENT 0
#define RF_DTAG_BOOL 1
#define RF_DTAG_INT 2
#define RF_DTAG_DOUBLE 3
#define RF_DTAG_STRING 4
#define RF_DLEAF_TAGS 1
#define RF_DLEAF_STR_CODESET 2
#define RF_DLEAF_BOOL 3
#define RF_DLEAF_NUM_RANGE 4
#define RF_DLEAF_NUM_SET 5
typedef struct rf_dynamic_leaf {
  int32_t kind;             /* RF_DLEAF_* */
  int32_t flags;            /* TAGS: tag mask; BOOL: value set (bits 0, 1); NUM_RANGE: RF_FRANGE_* bits; else 0 */
  const uint8_t* tags_dev;  /* [n_rows] */
  const void* payload_dev;  /* 8 bytes [n_rows]; TAGS does not read it */
  int64_t off, len;         /* STR_CODESET: words of code_sets_dev; NUM_SET: entries of int_sets_dev */
  int64_t foff, flen;       /* NUM_SET: entries of f64_sets_dev */
  int64_t ilo, ihi;         /* NUM_RANGE: the INT rows' bounds, inclusive */
  double flo, fhi;          /* NUM_RANGE: the DOUBLE rows' bounds */
} rf_dynamic_leaf;
int rf_dynamic_match(const rf_dynamic_leaf* leaves_host, int n_leaves, const uint32_t* code_sets_dev,
                     const int64_t* int_sets_dev, const double* f64_sets_dev, int64_t n_rows,
                     uint32_t* bitmaps_dev, void* stream);
/* ---- ARRAY fields: the leaves of `expr` over a collection's multi-valued columns ---------------------
 * pymilvus' DataType.ARRAY: a row holds 0 .. max_capacity (<= 4096) elements of one scalar type
 * (rag_fin_amd/schema.py).  The device mirror of one ARRAY field is CSR:
 *   offsets_dev  int64 [n_rows + 1], 8-byte aligned, offsets[0] == 0, non-decreasing: row r holds the
 *                elements [offsets[r], offsets[r + 1])
 *   values_dev   the elements back to back: int32 codes into the field's append-only dictionary (VARCHAR,
 *                BOOL), int64 (INT64) or fp64 (DOUBLE), aligned to the element
 * A leaf is evaluated into a row bitmap that an RF_FOP_BITMAP leaf of rf_filter_eval_bitmaps reads -- the
 * door rf_text_match, rf_column_match and rf_dynamic_match use.  Leaf kinds:
 *   RF_ALEAF_LENGTH  ilo <= offsets[r + 1] - offsets[r] <= ihi, both ends inclusive (ilo > ihi passes
 *                    nothing); values_dev is not read
 *   RF_ALEAF_ELEM    the row holds more than `index` elements and element `index` passes the scalar test
 *                    `elem` names: RF_CLEAF_CODESET (int32 codes), RF_CLEAF_I64_RANGE, RF_CLEAF_I64_SET
 *                    (int64) or RF_CLEAF_F64_RANGE (fp64), with off / len / ilo / ihi / flags / flo / fhi
 *                    as in rf_column_leaf; a shorter row fails
 *   RF_ALEAF_MATCH   `elem` names the element type (RF_AELEM_CODE / I64 / F64); the needles are the slice
 *                    [off, off + len) of value_sets_dev (CODE, I64: int64, a code widened) or of
 *                    f64_sets_dev (F64), sorted ascending and distinct, len <= RF_COLUMN_MAX_SET; the row
 *                    passes iff at least `need` DISTINCT needles occur among its elements (int64 equality,
 *                    IEEE == for fp64: a NaN element matches nothing, -0.0 matches 0.0).  need == 1: ANY /
 *                    CONTAINS; need == len <= 64: ALL (need == len == 0 passes every row)
 * LENGTH and ELEM: a lane owns one row (two offset loads, at most one element load).  MATCH is
 * wave-cooperative: a wave owns 64 consecutive rows, stages their 65 offsets in LDS, strides over the
 * rows' one contiguous element span with coalesced loads, looks each element up in the needle slice by
 * binary search and, on a hit only, locates the owning row (the largest r with offsets[r] <= e) by binary
 * search over the staged offsets and ORs the needle's bit into the row's 64-bit LDS slot; lane r then
 * tests popcount(slot[r]) >= need.  The OR is commutative and idempotent, so the slot does not depend on
 * the order the hits arrive in.
 * Otherwise the contract of rf_column_match: leaves_host is HOST memory, n_leaves in
 * 1..RF_ARRAY_MAX_LEAVES (they travel in the launch arguments); leaf l writes EVERY word of
 * bitmaps_dev[l * nwords .. (l + 1) * nwords), nwords = ceil(n_rows / 32), bits past n_rows zero; one
 * launch, grid (row chunks, leaves), a wave's 64 predicates become two words by ballot; stream-ordered, no
 * host sync, no allocation, no global atomics; integers and IEEE comparisons only: the same bits on every
 * run.
 * RF_ERR_INVALID before any device call: a NULL leaves_host / bitmaps_dev, n_leaves or n_rows out of range,
 * an unknown kind or elem, unknown flags, a negative off / len / index, need outside {1, len} or above 64, a
 * set of more than RF_COLUMN_MAX_SET values (1 << 26 code-set words), a leaf that needs code_sets_dev /
 * value_sets_dev / f64_sets_dev when that is NULL, a misaligned set or bitmap pointer, offsets_dev NULL or
 * not 8-byte aligned, values_dev NULL (any kind but LENGTH) or not aligned to its element.  A column whose
 * rows are all empty may pass any aligned non-NULL values_dev: none of it is read.  The offsets are trusted
 * (the store derives them from the rows' lengths); an element or a search position outside a leaf's slice is
 * never dereferenced.  n_rows == 0 writes nothing and returns RF_OK.
 * New in this build; the reference's collection has no ARRAY field. */
#define RF_ARRAY_MAX_LEAVES 16
#define RF_ALEAF_LENGTH 1
#define RF_ALEAF_ELEM 2
#define RF_ALEAF_MATCH 3
#define RF_AELEM_CODE 1
#define RF_AELEM_I64 2
#define RF_AELEM_F64 3
typedef struct rf_array_leaf {
  int32_t kind;                /* RF_ALEAF_* */
  int32_t elem;                /* ELEM: RF_CLEAF_* (the scalar test); MATCH: RF_AELEM_* (the element type) */
  int32_t flags;               /* ELEM with RF_CLEAF_F64_RANGE: RF_FRANGE_* bits; else 0 */
  int32_t need;                /* MATCH: 1 or len */
  const int64_t* offsets_dev;  /* [n_rows + 1] */
  const void* values_dev;      /* int32 codes | int64 | fp64; LENGTH does not read it */
  int64_t index;               /* ELEM: the element's position in its row, >= 0 */
  int64_t off, len;            /* ELEM: as rf_column_leaf; MATCH: the needle slice */
  int64_t ilo, ihi;            /* LENGTH, ELEM with RF_CLEAF_I64_RANGE: bounds, inclusive */
  double flo, fhi;             /* ELEM with RF_CLEAF_F64_RANGE: bounds */
} rf_array_leaf;
int rf_array_match(const rf_array_leaf* leaves_host, int n_leaves, const uint32_t* code_sets_dev,
                   const int64_t* value_sets_dev, const double* f64_sets_dev, int64_t n_rows,
                   uint32_t* bitmaps_dev, void* stream);
/* ---- lexical index maintenance: the postings after an append or a delete, without the old texts -------
 * A write changes N, avgdl and df, and through them every BM25 impact -- but with the term frequencies
 * kept beside the postings (post_tf uint32 [nnz]) everything is re-derivable: the arrays after a write
 * are bit for bit those of a fresh build of the surviving texts (the definitions in
 * numpy: rag_fin_amd/lexical.py, append_reference / compact_reference / impacts).
 * rf_postings describes one set of posting arrays in caller-owned device memory, inputs and outputs
 * alike: post_off int64 [n_terms + 1], post_row / post_tf uint32 [nnz], and, both or neither, pos_off
 * int64 [nnz + 1] with pos uint32 [n_pos] (the token positions of "keyword filters").  Every offset is
 * int64.  All calls are stream-ordered, allocate nothing and do not synchronise; RF_ERR_INVALID comes
 * from host-side checks before any device call (a NULL or not 16-byte-aligned array, a negative size,
 * n_rows >= 2^31, sizes that do not add up, a workspace that is too small).  As in rf_sparse_search, a
 * row or an offset out of range is clamped or skipped, never dereferenced: malformed postings give
 * wrong arrays, not an out-of-range access.  Integers only apart from the impacts, no atomics: the
 * same bits on every run.  What runs: workgroups over chunks of RF_LEX_CHUNK postings, read lane-
 * strided; a chunk's term range is found by two binary searches in post_off, a posting's term inside
 * that range.
 *   rf_sparse_impacts   post_imp[p] = float32(idf[t] * ((tf * (k1 + 1)) / (tf + k1 * ((1 - b) + b *
 *                       (dl[row] / avgdl))))), every operation in fp64, rounded on its own (no
 *                       contraction); (k1 + 1) and (1 - b) are formed once.  idf fp64 [n_terms] comes
 *                       from the host (log is not correctly rounded: it must be the host's), dl int32
 *                       [n_rows].  avgdl > 0, k1 >= 0, 0 <= b <= 1.  A row >= n_rows gets impact 0.
 *   rf_sparse_append    merged = old followed, per merged term, by delta with rows + old->n_rows.
 *                       delta: the postings of the appended rows alone, over their own dictionary, rows
 *                       from 0 (nnz = 0 and n_terms = 0 are allowed; its arrays stay non-NULL).
 *                       map_old_dev int64 [old->n_terms], map_delta_dev int64 [delta->n_terms]: the
 *                       merged term id of every term, ascending.  merged: post_off is an INPUT (the
 *                       host knows every df), post_row / post_tf and pos_off / pos are written, n_rows,
 *                       nnz and n_pos are the sums of both sides.  Positions on all three or on none.
 *                       workspace_bytes >= rf_sparse_append_workspace_bytes(n_terms old, delta).
 *                       One small launch makes the per-term tables (where a term's postings and their
 *                       positions go), then one launch per side moves it: every posting is read once
 *                       and written once.
 *   rf_sparse_compact_plan   row_map_dev int32 [old->n_rows]: the new number of a row, or < 0 for a row
 *                       that goes.  Writes dst_post_dev int64 [nnz + 1], the exclusive scan of "posting
 *                       p is kept" closed by the total; with positions, dst_pos_dev int64 [nnz + 1],
 *                       the exclusive scan of the kept postings' position counts (else NULL); and
 *                       term_dst_dev int64 [n_terms + 2]: dst_post[post_off[t]] for t = 0 .. n_terms, the
 *                       raw term offsets (a term whose two offsets are equal is gone), then the kept
 *                       positions.  The host reads those back, drops the dead terms and sizes the
 *                       outputs.  workspace_bytes >= rf_sparse_compact_workspace_bytes(nnz) (0 = out of
 *                       range).  The prefix sum is reduce-then-scan over chunks of RF_LEX_CHUNK: a sum
 *                       per chunk, one workgroup scans the sums in tiles of RF_LEX_CHUNK with a carry,
 *                       then every chunk scans itself from its offset.
 *   rf_sparse_compact_apply  kept posting p goes to slot dst_post[p] with row row_map[row] and its tf; its
 *                       positions to pos[dst_pos[p] ..), pos_off closed at slot dst_post[nnz].  out:
 *                       post_row / post_tf / pos_off / pos are written, nnz and n_pos are capacities (a
 *                       slot or a position past them is not written); out->post_off is not read.
 * New in this build; the reference has no lexical index. */
#define RF_LEX_CHUNK 1024
typedef struct rf_postings {
  int64_t n_rows, n_terms, nnz, n_pos;
  int64_t* post_off;   /* [n_terms + 1] */
  uint32_t* post_row;  /* [nnz] */
  uint32_t* post_tf;   /* [nnz] */
  int64_t* pos_off;    /* [nnz + 1] or NULL */
  uint32_t* pos;       /* [n_pos] or NULL */
} rf_postings;
int rf_sparse_impacts(const int64_t* post_off_dev, const uint32_t* post_row_dev, const uint32_t* post_tf_dev,
                      const double* idf_dev, const int32_t* dl_dev, int64_t n_rows, int64_t n_terms, int64_t nnz,
                      double avgdl, double k1, double b, float* post_imp_dev, void* stream);
size_t rf_sparse_append_workspace_bytes(int64_t n_terms_old, int64_t n_terms_delta);
int rf_sparse_append(const rf_postings* old_p, const rf_postings* delta, const int64_t* map_old_dev,
                     const int64_t* map_delta_dev, const rf_postings* merged, void* workspace_dev,
                     size_t workspace_bytes, void* stream);
size_t rf_sparse_compact_workspace_bytes(int64_t nnz);
int rf_sparse_compact_plan(const rf_postings* old_p, const int32_t* row_map_dev, int64_t* dst_post_dev,
                           int64_t* dst_pos_dev, int64_t* term_dst_dev, void* workspace_dev, size_t workspace_bytes,
                           void* stream);
int rf_sparse_compact_apply(const rf_postings* old_p, const int32_t* row_map_dev, const int64_t* dst_post_dev,
                            const int64_t* dst_pos_dev, const rf_postings* out, void* stream);
/* ---- lexical index build: a token stream -> the posting arrays, on the device ------------------------
 * What rag_fin_amd/lexical.py's count_terms computes, from term ids instead of strings (DESIGN 4.4l;
 * the definition in numpy: lexical.counts_from_tokens).  tok_dev int32 [n_tokens]: the term id of
 * every token of the corpus in (row, position) order (rf_analyze's tok); row_start_dev int64
 * [n_rows + 1]: where each row's tokens start, closed by n_tokens (rows may be empty).  A stable sort
 * by term id puts the tokens in (term, row, position) order; a token whose (term, row) differs from
 * its predecessor's heads a posting, the exclusive scan of the heads numbers the postings, a run's
 * length is its tf, a head's sorted index its pos_off, and pos[i] is sorted token i's index minus its
 * row's start.  The sort is a least-significant-digit radix sort with 8-bit digits,
 * ceil(bits(n_terms - 1) / 8) passes over tiles of RF_LEX_SORT_TILE tokens, the token index as
 * payload; the scans are the reduce-then-scan over chunks of RF_LEX_CHUNK of the compaction plan.
 *   rf_sparse_count_workspace_bytes   0 = out of range (n_tokens or n_terms < 1 or >= 2^31)
 *   rf_sparse_count_plan    writes post_off_dev int64 [n_terms + 1] and totals_dev int64 [2] = { nnz,
 *                           n_pos = n_tokens } (8-byte aligned: it may follow post_off in one buffer,
 *                           read back in one copy), and leaves the sorted stream in the workspace
 *   rf_sparse_count_apply   same sizes and the same, untouched workspace.  out: post_row / post_tf
 *                           [nnz] are written, with want_positions also pos_off int64 [nnz + 1] and pos
 *                           uint32 [n_pos]; nnz and n_pos are capacities (a slot past them is not
 *                           written); post_off is not read.
 * Stream-ordered, no allocation, no synchronisation; integers only, LDS counters, no global atomics:
 * the same bits on every run.  RF_ERR_INVALID from host-side checks before any device call, as above.
 * A term id outside [0, n_terms) is clamped into it; a malformed row_start gives wrong rows, never an
 * out-of-range access.  New in this build; the reference has no lexical index. */
#define RF_LEX_SORT_TILE 4096
size_t rf_sparse_count_workspace_bytes(int64_t n_tokens, int64_t n_terms);
int rf_sparse_count_plan(const int32_t* tok_dev, const int64_t* row_start_dev, int64_t n_tokens, int64_t n_rows,
                         int64_t n_terms, int64_t* post_off_dev, int64_t* totals_dev, void* workspace_dev,
                         size_t workspace_bytes, void* stream);
int rf_sparse_count_apply(const int64_t* row_start_dev, int64_t n_tokens, int64_t n_rows, int64_t n_terms,
                          void* workspace_dev, size_t workspace_bytes, const rf_postings* out, int want_positions,
                          void* stream);
/* Cross-shard merge after the RCCL all-gather: in [W, B, k] (exact fp64, id
 * int64) -> out [B, k] by (score desc, id asc).  New in this build (the
 * reference is single-process); see SURVEY.md 8e. */
int rf_merge_shards(const double* exact_dev, const int64_t* ids_dev, int W, int B, int k,
                    float* scores_out_dev, int64_t* ids_out_dev, void* stream);
/* Same merge on the all-gather's own layout.  Each rank's send buffer is
 * rf_packed_shard_words(B, k) int64 words:
 *   [0, B k)        the fp64 ranking scores (bit patterns)   <- rf_search exact_dev
 *   [B k, 2 B k)    the global row ids                       <- rf_search ids_dev
 *   [2 B k, ...)    uint32 flags[B] (RF_FLAG_*), zero-padded <- rf_search flags_dev
 * so rf_search writes its outputs straight into ONE send buffer and no repacking kernel runs
 * between the scan, the collective and the merge.  packed_dev = the gathered [W] buffers.
 * flags_out_dev (nullable) uint32 [B]: OR of the W shards' flags -- identical on every rank, so
 * all ranks agree on which queries to re-run through rf_search_exhaustive (a query whose LOCAL
 * answer was unproven on ANY shard has an unproven merged answer). */
size_t rf_packed_shard_words(int B, int k);
int rf_merge_shards_packed(const int64_t* packed_dev, int W, int B, int k,
                           float* scores_out_dev, int64_t* ids_out_dev,
                           uint32_t* flags_out_dev, void* stream);
/* Shards that are not contiguous in the global row numbering (a store that grows by appending a
 * slice of every insert to every rank): rf_search runs with id_base 0 and this call turns the
 * LOCAL row numbers it wrote into global ids through the shard's table, in place, on `stream`:
 * ids_dev[i] = id_map_dev[ids_dev[i]] for ids >= 0 (-1 = "no hit" stays; a row number past n_map
 * becomes -1).  Between the scan and the all-gather: the N > 1 step is then four enqueues
 * (rf_search_fp16, rf_map_ids, ncclAllGather, rf_merge_shards_packed) and no host library touches
 * the ids.  New in this build; stands beside vector_rag_mcp/main.py:51-57. */
int rf_map_ids(int64_t* ids_dev, int64_t n, const int64_t* id_map_dev, int64_t n_map, void* stream);
/* ---- the sharded step as ONE call (rf_comm_init / rf_search_sharded; 8e) ----------
 * One process per GPU; rank r holds a row shard in its rf_index_t.  The reference has no counterpart
 * (one Milvus server answers vector_rag_mcp/main.py:51-57); this is what stands in for it at N > 1.
 *   rf_comm_unique_id   rank 0 draws the job's 128-byte id (RF_COMM_ID_BYTES, host memory); the HOST
 *                       ships it to the other ranks (MPI, a socket, torch.distributed, a file)
 *   rf_comm_init        every rank: ncclCommInitRank on `device` -- blocks until all `world` ranks arrive
 *   rf_search_sharded   every rank, same B and k, calls in the same order on all ranks: rf_search_fp16 (the
 *                       fp16 chain even on an index with rf_index_set_shadow_first: the step's flag
 *                       resolution has no fp16 tier to put behind a shadow pass) into
 *                       the packed send buffer, rf_map_ids when id_map_dev is given (id_base is then
 *                       ignored), ncclAllGather of rf_packed_shard_words(B, k) words, rf_merge_shards_packed.
 *                       Four enqueues on `stream`, no host synchronisation; scores_dev / ids_dev hold the
 *                       GLOBAL top-k on every rank, flags_dev (nullable) the OR of the shards' RF_FLAG_*
 *                       bits -- a flagged query is re-run through rf_search_exhaustive on every shard and
 *                       merged again by the host, exactly as for one GPU.
 *                       scratch_dev: rf_search_sharded_scratch_words(comm, B, k) int64 words of device
 *                       memory owned by the caller, not shared between steps that may be in flight together.
 * One collective at a time per communicator: the caller serialises rf_search_sharded calls on one rf_comm_t
 * (different streams are fine as long as every rank enqueues them in the same order).
 * RCCL is bound at run time (dlopen of librccl.so, or RAGFIN_RCCL_PATH; a copy the process has already
 * loaded is reused): where it is absent these calls return RF_ERR_UNSUPPORTED and the rest of the
 * library works.  rag_fin_amd/sharded.py runs the same four enqueues from Python (rag_fin_amd/rccl.py
 * binds the same library). */
#define RF_COMM_ID_BYTES 128
int rf_comm_unique_id(void* id_out);
int rf_comm_init(int rank, int world, const void* id, int device, rf_comm_t** out);
int rf_comm_destroy(rf_comm_t* comm);
int rf_comm_rank(const rf_comm_t* comm);
int rf_comm_world(const rf_comm_t* comm);
size_t rf_search_sharded_scratch_words(const rf_comm_t* comm, int B, int k);
int rf_search_sharded(const rf_index_t* ix, rf_comm_t* comm, const void* q_dev, int B, int k,
                      int64_t id_base, const int64_t* id_map_dev, int64_t n_map,
                      float* scores_dev, int64_t* ids_dev, uint32_t* flags_dev,
                      void* workspace_dev, size_t workspace_bytes,
                      int64_t* scratch_dev, size_t scratch_words, void* stream);
/* Test hook: raw MFMA scan scores fp32 [B, n] for the first n rows. */
int rf_debug_scores(const rf_index_t* ix, const void* q_dev, int B, int64_t n,
                    float* out_dev, void* stream);

/* ---- SQ8 index: Collection.create_index("embedding", {"index_type": "SQ8", ...}) -------------------
 * Reference: "chunking_storing (1).py":29 picks the index type.  SQ8 keeps an int8 copy of the corpus
 * (the "shadow") next to the fp16 tiles and sweeps it with v_mfma_i32_32x32x32_i8: dim + 8 bytes per
 * row instead of 2 dim, plus the fp16 sample pass.  The answer
 * stays EXACT: the int8 scores only nominate candidates, each row tested against its own error bound,
 * and the merge rescores them in fp64 from the fp16 tiles.  Ids, ranks, scores and
 * the flag contract are those of rf_search.
 *   rf_sq8_storage_bytes   bytes of the shadow for `capacity_rows` rows (0 unless dim % 32 == 0 and the
 *                          dim has a scan kernel); a SEPARATE caller-owned allocation, 16-byte aligned
 *   rf_index_attach_sq8    quantize every existing row into the shadow (stream-ordered); from then on
 *                          rf_index_add_f16 / rf_index_compact / rf_index_reset keep it current, and
 *                          it is byte-identical to a fresh attach over the same rows.  Other dims:
 *                          RF_ERR_UNSUPPORTED.  Like rf_index_add_f16: never concurrent with a search.
 *   rf_index_detach_sq8    forget the shadow (the caller frees it after the stream has drained)
 *   rf_search_sq8          rf_search's arguments and outputs; 64-query sweeps for any B.  A corpus of
 *                          <= 8192 rows (every row a candidate) runs the FLAT path.  A flagged query
 *                          is re-run through rf_search_fp16 and, only if that flags too, rf_search_exhaustive.
 *                          A query whose bound is too loose for the int8 sweep (most sample partitions
 *                          clear its threshold) is given up before the sweep and flagged.
 *                          workspace_bytes >= rf_search_sq8_workspace_bytes (> rf_search_workspace_bytes)
 *   rf_search_sq8_profile  the first sweep with HIP events: stage_ms_host (host) receives {query
 *                          quantization, sample, threshold, int8 emit, prune + refine, merge} in ms
 *                          (six floats); SYNCHRONISES
 *   rf_debug_scores_sq8    test hook: a~ fp32 [B, n] of the first n rows, delta_dev (nullable) fp32 [B]
 *                          the bound delta_q >= |a - a~| of every row
 *   rf_index_get_rows_sq8  test hook: the un-tiled int8 rows [n, dim], s_r fp32 [n], e_r fp32 [n] */
size_t rf_sq8_storage_bytes(int dim, int64_t capacity_rows);
int rf_index_attach_sq8(rf_index_t* ix, void* storage_dev, size_t storage_bytes, void* stream);
int rf_index_detach_sq8(rf_index_t* ix);
size_t rf_search_sq8_workspace_bytes(const rf_index_t* ix);
int rf_search_sq8(const rf_index_t* ix, const void* q_dev, int B, int k, int64_t id_base,
                  float* scores_dev, int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev,
                  void* workspace_dev, size_t workspace_bytes, void* stream);
int rf_search_sq8_profile(const rf_index_t* ix, const void* q_dev, int B, int k, int64_t id_base,
                          float* scores_dev, int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev,
                          void* workspace_dev, size_t workspace_bytes, void* stream, float* stage_ms_host);
int rf_debug_scores_sq8(const rf_index_t* ix, const void* q_dev, int B, int64_t n, float* out_dev,
                        float* delta_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int rf_index_get_rows_sq8(const rf_index_t* ix, const int64_t* rows_dev, int64_t n, void* out_dev,
                          float* scales_dev, float* err_dev, void* stream);

/* ---- shadow first: rf_search over a large index reads the int8 shadow ------------------------------
 * An SQ8 sweep is: quantize the queries -> fp16 sample -> threshold -> int8 emit -> prune + refine ->
 * merge.  The refine stage drops every candidate whose upper bound a~ + beta_r lies under the k-th
 * largest lower bound a~ - beta_r and gives the survivors their fp16 score, so the merge works on what a
 * FLAT emit would have handed it: about half the bytes of the fp16 sweep per batch.
 *   rf_index_set_shadow_first  min_rows > 0: rf_search and rf_search_profile run that chain when a shadow
 *                          is attached, the index holds >= min_rows rows (and > 8192) and the batch is one
 *                          plain sweep (B <= 64); wider batches and every other search form stay on fp16.
 *                          min_rows <= 0 turns it off (the default); attaching a shadow alone changes
 *                          nothing.  While it is set and a shadow is attached, rf_search_workspace_bytes
 *                          is the SQ8 size: read it after the switch.  Host state of the index: like
 *                          rf_index_add_f16, never concurrent with a search.
 *                          rf_search_profile keeps its four stages: `sample` includes the query
 *                          quantization, `emit` the refine stage.
 *   rf_search_fp16         rf_search's arguments and outputs through the fp16 chain whatever is attached:
 *                          the tier a query flagged by a shadow-first rf_search or by rf_search_sq8 is
 *                          re-run through (rf_search again would sweep the shadow a second time). */
int rf_index_set_shadow_first(rf_index_t* ix, int64_t min_rows);
int rf_search_fp16(const rf_index_t* ix, const void* q_dev, int B, int k, int64_t id_base,
                   float* scores_dev, int64_t* ids_dev, double* exact_dev, uint32_t* flags_dev,
                   void* workspace_dev, size_t workspace_bytes, void* stream);

#ifdef RF_EXPERIMENTS
/* ---- experiments build only (python -m rag_fin_amd.build --experiments ->
 * libragfin_hip_exp.so; used by tools/, never by the product or the tests) -------------------
 * The shipped library has no run-time tuning surface: the knobs are compile-time constants
 * (csrc/rf_internal.h).  In the experiments build they are process-wide ints, NOT thread-safe
 * against concurrent searches.  Keys: "ring24" (6|8|12|24), "emit_wgs_per_cu" (0..4),
 * "sample_bpw" (1..8), "sample_fold" (0|1), "fold_dbg", "wide_sample_pairs" (1..8), "wide_dbg",
 * "wide_ne"; encoder: "linear_dma" (0..3), "linear_small", "encode_graph", "one_query",
 * "post_block", "post_qkv" (0|1), "linear_dbg", "post_dbg", "debug_epi" (0|2|5).  The list with
 * defaults and ranges is RF_KNOBS in csrc/rf_internal.h; any other key is an error. */
int rf_set_tuning(const char* key, int value);
/* byte offset of a named array ("pmax", "cand", "thr", "eps", "cand_cnt", "rmask", "rcnt") inside a
 * search workspace (the same in an SQ8 workspace, whose query area follows the FLAT arrays) */
size_t rf_debug_workspace_offset(const char* field);
/* a device buffer (>= 64 KiB, or NULL to switch off) that instrumented kernels fill with
 * clock stamps (encoder k_linear_dma: 8 floats per wave) */
int rf_debug_set_buffer(void* dev_ptr);
#endif

/* ---- embedder: replaces SentenceTransformer('all-MiniLM-L6-v2').encode ----
 * Reference: vector_rag_mcp/main.py:41,50; retrieve.py:14,27;
 * "chunking_storing (1).py":8,380,408. */
typedef struct rf_encoder_config {
  int32_t vocab_size, hidden, layers, heads, intermediate, max_position, type_vocab;
  float ln_eps;
} rf_encoder_config;

/* All pointers are device fp16 unless noted; per-layer arrays are
 * [layers] x tensor, contiguous.  Linear weights are stored [out, in]
 * (PyTorch nn.Linear layout). */
typedef struct rf_encoder_weights {
  const void* word_emb;   /* [vocab, H] */
  const void* pos_emb;    /* [max_position, H] */
  const void* type_emb;   /* [type_vocab, H] */
  const void* emb_ln_g;   /* [H] */
  const void* emb_ln_b;   /* [H] */
  const void* qkv_w;      /* [L, 3H, H]  (q;k;v stacked on the out axis) */
  const void* qkv_b;      /* [L, 3H] */
  const void* ao_w;       /* [L, H, H] */
  const void* ao_b;       /* [L, H] */
  const void* ln1_g;      /* [L, H] */
  const void* ln1_b;      /* [L, H] */
  const void* ff1_w;      /* [L, I, H] */
  const void* ff1_b;      /* [L, I] */
  const void* ff2_w;      /* [L, H, I] */
  const void* ff2_b;      /* [L, H] */
  const void* ln2_g;      /* [L, H] */
  const void* ln2_b;      /* [L, H] */
} rf_encoder_weights;

/* Bytes of caller-owned device storage the encoder needs for its MFMA-tiled copy
 * of the four Linear weights per layer (0 if cfg is unsupported). */
size_t rf_encoder_storage_bytes(const rf_encoder_config* cfg);
/* Tiles the Linear weights into storage_dev on `stream` and keeps the remaining
 * pointers of `w` (embeddings, biases, LayerNorm) -- the caller keeps those
 * tensors alive for the encoder's lifetime.  Supported: hidden == 384,
 * head_dim == 32, intermediate == 1536 (the all-MiniLM-L{6,12}-H384 family); anything else
 * returns RF_ERR_UNSUPPORTED. */
int rf_encoder_create(rf_encoder_t** out, const rf_encoder_config* cfg,
                      const rf_encoder_weights* w, void* storage_dev, size_t storage_bytes,
                      int device, void* stream);
int rf_encoder_destroy(rf_encoder_t* enc);
size_t rf_encode_workspace_bytes(const rf_encoder_t* enc, int B, int T);
/* Query-sized calls (B * T <= 1024): the launch sequence is captured once per (B, T, buffer
 * pointers) into a hipGraph owned by the encoder handle and replayed on `stream`
 * afterwards; callers that want the replay keep their buffers at fixed addresses
 * (rag_fin_amd.embedder does).
 * ids_dev int32 [B, T] (padded), lens_dev int32 [B] (valid tokens per row).
 * out_f16_dev fp16 [B, H] and/or out_f32_dev fp32 [B, H] (either nullable):
 * masked mean-pool + L2-normalise of the last hidden state.
 * T <= max_position (RF_ERR_INVALID beyond).  T <= 256 -- the reference model's max_seq_length,
 * vector_rag_mcp/main.py:41 -- runs the MFMA attention; 256 < T <= max_position is supported and
 * tested (tests/test_encoder_gpu.py, T = 257, 300, 384, 512 against the fp64 oracle at the same
 * tolerances) but takes a scalar attention kernel: correct, several times slower per token.
 * Batches of >= 8192 token slots take the fused per-layer path (csrc/encoder_post.hip); the cached
 * hipGraphs are an LRU of 32 entries, an evicted one is destroyed after its last launch has finished. */
int rf_encode(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev,
              int B, int T, void* out_f16_dev, float* out_f32_dev,
              void* workspace_dev, size_t workspace_bytes, void* stream);

/* Sentence-embedder families: rf_encode with the Pooling and Normalize modules of a sentence-transformers
 * directory (BGE and arctic-embed pool the [CLS] token, E5 excludes nothing but prepends a prompt, the
 * multi-qa "dot" models have no Normalize module).  The forward is rf_encode's -- the same embedding launch and
 * layers on every path by B and T -- and closes with one launch of csrc/sentence_head.hip where rf_encode pools.
 * ids_dev, lens_dev, outputs and workspace as for rf_encode; skip_dev int32 [B] or NULL (= all 0) is the number
 * of leading tokens of a row left out of the pooled set (a prompt's, with include_prompt false), clamped to
 * 0..lens[b].
 *   set       of row b: the tokens skip[b] <= t < lens[b]
 *   MEAN      sum / max(count, 1e-9)       MEAN_SQRT_LEN  sum / sqrt(count)
 *   MAX       the per-feature maximum over the set: exact, the hidden values are fp16
 *   CLS       token 0, whatever skip says
 *   empty set the zero vector in the three set modes (sentence-transformers' Pooling gives -1e9 for MAX there:
 *             a departure, written down as such; rag_fin_amd.embedder never produces an empty set); a row with
 *             lens < 1 gives zeros in every mode
 *   normalize != 0 divides by max(||x||_2, 1e-12); otherwise the pooled vector is written as it is
 * The sums are fp32 in a fixed, sequence-relative order; skip masks tokens out of that order and does not shift
 * it, so RF_POOL_MEAN with normalize = 1 and no skip equals rf_encode's fp32 and fp16 outputs bit for bit, and a
 * row's bits do not depend on its place in the batch.  Always plain launches: the cached hipGraphs are
 * rf_encode's alone, so a single query pays its launches one by one.
 * RF_ERR_INVALID before any launch: a null enc, ids, lens, head or workspace, both outputs null, pooling outside
 * the enum, B or T < 1.  RF_ERR_UNSUPPORTED: T > max_position.  RF_ERR_CAPACITY: workspace too small or misaligned.
 * New in this build; the reference embeds with all-MiniLM-L6-v2 alone (vector_rag_mcp/main.py:41). */
enum { RF_POOL_MEAN = 0, RF_POOL_CLS = 1, RF_POOL_MAX = 2, RF_POOL_MEAN_SQRT_LEN = 3 };
typedef struct rf_sentence_head {
  int32_t pooling;                   /* RF_POOL_* */
  int32_t normalize;                 /* != 0: L2-normalise the pooled vector */
} rf_sentence_head;
int rf_encode_sentences(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev,
                        const int32_t* skip_dev, int B, int T, const rf_sentence_head* head, void* out_f16_dev,
                        float* out_f32_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Cross-encoder reranking: one relevance logit per (query, chunk) pair from a
 * BertForSequenceClassification checkpoint of the same family (cross-encoder/ms-marco-MiniLM-L-6-v2,
 * -L-12-v2): the encoder handle holds the BertModel weights, `head` the pooler and the classifier
 * (device fp16, row-major as nn.Linear stores them; the caller keeps them alive for the call).
 * Same conventions as rf_encode: stream-ordered, caller-owned buffers, workspace of
 * rf_encode_workspace_bytes(enc, B, T) bytes.
 * ids_dev int32 [B, T]: [CLS] query [SEP] chunk [SEP], padded; lens_dev int32 [B]; seg_dev int32 [B]: the
 * index of the first token of the second segment (token_type_ids = 1 from there on; seg >= len: the row
 * has no second segment).  logits_dev fp32 [B]:
 *   logit = cls_w . tanh(pool_w x + pool_b) + cls_b,  x = the last hidden state of the row's [CLS] token,
 * accumulated in fp32 in a fixed order (csrc/rerank.hip), so a pair's logit has the same bits wherever the
 * pair sits in a batch; a row with lens < 1 has no [CLS] token and gets -inf.  No activation is applied.
 * The layers are rf_encode's (all its paths by B and T); these calls are always plain launches and never
 * touch rf_encode's cached hipGraphs.
 * RF_ERR_UNSUPPORTED: num_labels != 1, an encoder with type_vocab < 2, T > max_position. */
typedef struct rf_pair_head {
  const void* pool_w;   /* [H, H]  bert.pooler.dense.weight (16-byte aligned) */
  const void* pool_b;   /* [H] */
  const void* cls_w;    /* [1, H]  classifier.weight */
  const void* cls_b;    /* [1] */
  int32_t num_labels;
} rf_pair_head;
int rf_score_pairs(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev,
                   const int32_t* seg_dev, int B, int T, const rf_pair_head* head, float* logits_dev,
                   void* workspace_dev, size_t workspace_bytes, void* stream);

/* Extractive reading: the best answer spans of (question, chunk) pairs from a BertForQuestionAnswering
 * checkpoint of the same family (e.g. deepset/minilm-uncased-squad2): the encoder handle holds the BertModel
 * weights, `head` the span head qa_outputs (device fp16, row-major as nn.Linear stores it; kept alive by the
 * caller for the call).  ids_dev, lens_dev, seg_dev, B, T, the workspace and the stream are rf_score_pairs':
 * [CLS] question [SEP] chunk [SEP] rows, seg = index of the chunk's first token.  The layers are rf_encode's;
 * the call is always plain launches and never touches rf_encode's cached hipGraphs.  Per pair b (csrc/reader.hip):
 *   logits      s[t] = qa_w[0] . x_t + qa_b[0], e[t] = qa_w[1] . x_t + qa_b[1] for t < lens[b], x_t the last
 *               hidden state of token t, accumulated in fp32 in one fixed order; written to logits_dev
 *               [B, T, 2] (start, end per position) when it is not NULL, positions >= lens[b] untouched
 *   candidates  the context is lo = seg[b] .. hi = lens[b] - 2 (the closing [SEP] excluded); a candidate is
 *               (i, j) with lo <= i <= j <= hi and j - i + 1 <= max_answer_len, z = s[i] + e[j] (one fp32
 *               add).  spans_dev [B, n_best]: the best n_best by (z descending, i ascending, j ascending),
 *               token positions in the pair; slots beyond the number of candidates are (-1, -1, -inf).
 *               seg >= lens - 1 or lens < 3: no candidates, every slot empty, the call succeeds
 *   norm_dev    [B, 3]: z_null = s[0] + e[0] (the [CLS] slot, SQuAD 2's "no answer"),
 *               lse_start = log sum exp(s[t]) over t in {0} u [lo, hi], lse_end the same over e (maximum
 *               subtracted, summed in fp64 in a fixed order, rounded to fp32 once).  exp(z - lse_start -
 *               lse_end) is the product of the two softmax probabilities; the library returns no probability.
 *               A row with lens < 1 has no [CLS] token: its three values are -inf and its slots empty
 * All of it is a function of the pair alone -- no atomics, no arrival-order reduction: the same pair gives the
 * same bits at any place of any batch.
 * RF_ERR_INVALID: n_best outside 1..RF_READER_MAX_BEST, max_answer_len outside 1..RF_READER_MAX_SPAN, a null or
 * misaligned pointer.  RF_ERR_UNSUPPORTED: an encoder with type_vocab < 2, T > max_position, T > 512 (the
 * positions one workgroup of the span stage holds).  RF_ERR_CAPACITY: workspace too small or misaligned. */
#define RF_READER_MAX_BEST 16
#define RF_READER_MAX_SPAN 64
typedef struct rf_qa_head {
  const void* qa_w;   /* [2, H]  qa_outputs.weight: row 0 = start, row 1 = end (16-byte aligned) */
  const void* qa_b;   /* [2] */
} rf_qa_head;
typedef struct rf_span {
  int32_t start, end;   /* token positions in the pair; -1, -1 = none */
  float z;              /* s[start] + e[end]; -inf = none */
} rf_span;
int rf_answer_spans(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev,
                    const int32_t* seg_dev, int B, int T, const rf_qa_head* head, int max_answer_len, int n_best,
                    rf_span* spans_dev, float* norm_dev, float* logits_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);

/* Sliding windows over a long context: a context of more tokens than a pair row holds is read as W overlapping
 * windows, each a pair row of rf_answer_spans (called with logits_dev), and rf_stitch_spans decodes ONE ranking
 * and ONE pair of normalisers per context from the windows' logits -- not one softmax per window, whose scores
 * are not comparable between windows (a window without the answer puts a probability near 1 on its best wrong
 * span) and which reports a span seen by two windows twice.  csrc/reader_windows.hip; three launches per call.
 *   win_dev      [W] windows; rows ctx_win_dev[c] .. ctx_win_dev[c + 1] (a CSR over the C contexts) are context
 *                c's, in ascending `first`, each with count <= T.  Row w of win_dev describes row w of logits_dev
 *   L            max(first + count) over the context's windows, the context's token count
 *                (<= RF_READER_MAX_CONTEXT; every token lies in one of the windows)
 *   owner        of context token t: the window w holding t with the largest min(t - first_w, first_w + count_w
 *                - 1 - t), ties to the smallest w (BERT's "max context" rule in integers)
 *   S[t], E[t]   logits[owner, seg_owner + t - first_owner, 0 / 1], copied, no arithmetic
 *   null slot    the window with the smallest fp32 s_w[0] + e_w[0] (its [CLS] position), ties to the smallest w
 *                (run_squad's minimum over features); z_null is that sum
 *   candidates   (i, j), 0 <= i <= j < L, j - i + 1 <= max_answer_len, z = S[i] + E[j] (one fp32 add); a span
 *                may cross the seam between two owners.  spans_dev [C, n_best]: the best n_best by (z descending,
 *                i ascending, j ascending), CONTEXT-token indices; slots beyond the candidates are (-1, -1, -inf)
 *   norm_dev     [C, 3]: z_null, lse_start = log sum exp over the null slot's s[0] and S[0 .. L), lse_end the same
 *                over e[0] and E: the exact maximum subtracted, exp summed in fp64 in one fixed order (the null
 *                term, then the 512-token tiles ascending, each by a fixed tree), max + log(sum) rounded to fp32
 *                once
 *   L == 0       no candidates, the normalisers are the null slot's alone; a context without windows: three -inf
 * No atomics and no arrival-order reduction; every selection is the maximum of the strict total order
 * (z, (i << 6) | (j - i)): a context gives the same bits at any place among any other contexts, in every call.
 * Malformed windows (descending `first`, count > T, a token in no window, L beyond the limit) give wrong numbers,
 * never an access out of range: every index is clamped to W, T and L.
 * The workspace is scratch of the call (rf_stitch_workspace_bytes; 16-byte aligned): concurrent calls need one
 * each.  It holds a 512-token tile per window (~4.3 KB), which bounds every context's tokens because count <= T
 * <= 512, so its size follows from W; C and max_context_tokens (the largest L of the call) are checked against
 * their ranges, and 0 is returned for C < 1, W < 0 or a context beyond RF_READER_MAX_CONTEXT.
 * Checked before anything is launched (a refused call writes nothing).  RF_ERR_INVALID: a null pointer, n_best
 * outside 1..RF_READER_MAX_BEST, max_answer_len outside 1..RF_READER_MAX_SPAN, W < 0, C < 1, T < 1.
 * RF_ERR_UNSUPPORTED: T > 512.  RF_ERR_CAPACITY: workspace too small or misaligned. */
typedef struct rf_window {
  int32_t first;   /* context-token index of the window's first context token */
  int32_t count;   /* context tokens in the window (>= 0) */
  int32_t seg;     /* position of that first context token in the window's pair row */
  int32_t pad;
} rf_window;
#define RF_READER_MAX_CONTEXT 65536   /* tokens of one stitched context */
int rf_stitch_spans(const float* logits_dev, int W, int T, const rf_window* win_dev, const int32_t* ctx_win_dev,
                    int C, int max_answer_len, int n_best, rf_span* spans_dev, float* norm_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);
size_t rf_stitch_workspace_bytes(int W, int C, int max_context_tokens);

/* ---- learned sparse vectors (SPLADE): an MLM head over the encoder, max-pooled over a row's tokens ----
 * The model is a BertForMaskedLM of the same family (sentence-transformers' SparseEncoder; a Milvus
 * SPARSE_FLOAT_VECTOR field with metric IP): the encoder handle holds the BertModel weights, `head` the
 * cls.predictions module (device fp16, row-major as nn.Linear stores it; kept alive by the caller for the call).
 * ids_dev int32 [B, T], lens_dev int32 [B] as for rf_encode; token types are 0.  For row b and term v
 * (csrc/splade.hip):
 *   g_t = LayerNorm(gelu(tr_w x_t + tr_b))   x_t = last hidden state of token t < lens[b], [CLS] and [SEP] included
 *   m   = max_t (dec_w[v] . g_t + dec_b[v])
 *   weights[b, v] = log1p(max(m, 0))         applied once per (b, v), after the max: log1p o relu is monotone
 * fp16 operands, fp32 accumulation; g_t is rounded to fp16 before the decoder GEMM.  Every output is exactly
 * +0.0f or a normal positive float (anything below FLT_MIN is flushed to +0.0f; no -0.0, no denormal); a row
 * with lens < 1 is all zeros; padding positions contribute nothing.  A row's values are a function of the row
 * and of (B, T) alone -- no atomics, no arrival-order reduction: the same row gives the same bits at any place
 * of the batch.  The [tokens, V] logits are never stored: the workspace is rf_encode's plus one fp16
 * [tokens, H] matrix.  The layers are rf_encode's (all its paths by B and T); the call is always plain
 * launches and never touches rf_encode's cached hipGraphs.  Stream-ordered, no host sync, no allocation.
 * RF_ERR_UNSUPPORTED: head->vocab != the encoder's vocab_size, T > max_position.  RF_ERR_INVALID: a null or
 * misaligned pointer (tr_w, dec_w: 16 bytes), B or T < 1.  RF_ERR_CAPACITY: workspace too small or misaligned.
 *
 * rf_sparsify_terms: dense fp32 [B, V] weights -> packed CSR of each row's heaviest terms, exact.  The entries
 * > 0 are kept; of more than max_terms (1..RF_TERMS_MAX) the best max_terms by (value descending, term id
 * ascending).  Row b's entries are term_dev / val_dev [off_dev[b] .. off_dev[b + 1]), term ids ascending;
 * off_dev int32 [B + 1], term_dev int32 and val_dev fp32 with room for B * max_terms entries (what lies past
 * off_dev[B] is not written).  One workgroup per row: a radix selection on the bit patterns of the positive
 * floats and a sweep in term order; integers only, LDS counters whose arrival order shows nowhere: the same
 * bits on every run.  Stream-ordered, no allocation, no host sync, no workspace.  RF_ERR_INVALID before any
 * device call: a null or misaligned pointer, B or V < 1, max_terms out of range.
 * New in this build; the reference has no learned sparse arm. */
typedef struct rf_mlm_head {        /* device fp16, nn.Linear layout, 16-byte aligned, caller keeps alive */
  const void *tr_w, *tr_b;          /* [H,H], [H]  cls.predictions.transform.dense */
  const void *tr_ln_g, *tr_ln_b;    /* [H]         cls.predictions.transform.LayerNorm */
  const void *dec_w, *dec_b;        /* [V,H], [V]  cls.predictions.decoder (tied: the word embeddings), cls.predictions.bias */
  int32_t vocab;
} rf_mlm_head;
size_t rf_encode_terms_workspace_bytes(const rf_encoder_t* enc, int B, int T);
int rf_encode_terms(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev, int B, int T,
                    const rf_mlm_head* head, float* weights_dev, void* workspace_dev, size_t workspace_bytes,
                    void* stream);
#define RF_TERMS_MAX 256
int rf_sparsify_terms(const float* weights_dev, int B, int V, int max_terms, int32_t* off_dev, int32_t* term_dev,
                      float* val_dev, void* stream);

/* ---- late interaction (ColBERT): token vectors, MaxSim, the exact best rows (csrc/late_interaction.hip) ----
 * The model is a BertModel of the same family with a bias-free projection to `dim` features (Stanford
 * HF_ColBERT "linear.weight", PyLate "1_Dense"); a Milvus embedding list with metric MAX_SIM_IP.
 *
 * rf_encode_tokens: ids_dev int32 [B, T], lens_dev int32 [B] as for rf_encode; token types are 0.  The forward
 * opens with the embedder's embedding launch, runs rf_encode's layers (all its paths by B and T; always plain
 * launches, never rf_encode's cached hipGraphs) and closes with two launches:
 *   1. the kept tokens per row and their exclusive scan over the rows, integers in a fixed order.  A token is
 *      kept when t < lens[b] (lens clamped to 0..T) and bit `id` of head->skip is clear (skip NULL: none is
 *      dropped; ids clamped into the vocabulary as the embedding clamps them).
 *   2. for every kept token v = proj_w . x_t, an fp32 fma chain over k ascending from 0, then
 *      v / max(|v|, 1e-12) with |v|^2 summed in fp32 in one fixed order, rounded to fp16 once, written at
 *      out_off_dev[b] + (rank of the token among the row's kept tokens).
 * Row b's vectors are out_vec_dev[out_off_dev[b] .. out_off_dev[b + 1]) (units of `dim` halfs), in token
 * order; out_vec_dev has room for B * T vectors and nothing past out_off_dev[B] is written.  A row with
 * lens < 1 has no tokens.  A row's vectors depend on the row and on (B, T) alone -- no atomics, no
 * arrival-order reduction: the same row gives the same bits at any place of the batch and in every call.
 * Stream-ordered, no host sync, no allocation; the workspace is rf_encode's
 * (rf_encode_tokens_workspace_bytes; 0 for a shape that is out of range).
 * Refusals, all before any launch.  RF_ERR_INVALID: a null or misaligned pointer (proj_w, out_vec_dev: 16
 * bytes), B or T < 1.  RF_ERR_UNSUPPORTED: dim not a multiple of 16 in 16..RF_MAXSIM_DIM, head->vocab != the
 * encoder's vocab_size, T > max_position.  RF_ERR_CAPACITY: workspace too small or misaligned.
 *
 * rf_maxsim: score(q, r) = sum over i < q_len of max over the tokens j of row r of (q_i . d_j).
 * v_mfma_f32_32x32x16_f16 with the document's tokens on the A rows and the query's on the B columns: every dot
 * product is one fp32 MFMA chain over the D/16 feature blocks in ascending order from 0 (an order that depends
 * on D alone), the max is exact, and the sum is s = 0.0f; s = s + m_i for i = 0 .. q_len - 1, one fp32 add
 * each.  A row without tokens, a query with q_len == 0, a row whose filter bit is clear and a candidate row
 * outside [0, n_rows) score -inf ("not a hit"; such a row's tokens are not read).  Query slots i >= q_len are
 * never read.  Document lanes past the end of a row enter the max as -inf.  A score depends on the (query, row)
 * pair alone: the same bits in either mode, at any place of any call.  q_len_dev values are clamped to
 * 0..RF_MAXSIM_QTOK.  filter_dev: NULL, or a filter buffer built for docs->n_rows rows (a header for another
 * row count passes no row), as rf_sparse_search takes it.
 *   candidate mode (cand_off_dev given): query b scores the rows cand_row_dev[cand_off_dev[b] ..
 *     cand_off_dev[b + 1]); scores_dev is parallel to cand_row_dev.  A wave per (query, row) pair.
 *   all-rows mode (cand_off_dev NULL): scores_dev is [B, n_rows].  A workgroup takes 64 consecutive rows and
 *     walks over the B queries; a wave keeps up to 128 tokens of its row in registers meanwhile, so the field is
 *     read from memory once per call, not once per query.
 * Stream-ordered, no host sync, no allocation, no workspace, no atomics.  Before any launch -- RF_ERR_INVALID:
 * a null or misaligned pointer (vectors, filter: 16 bytes; offsets, rows: 8), B < 1, n_rows < 0;
 * RF_ERR_UNSUPPORTED: dim not a multiple of 16 in 16..RF_MAXSIM_DIM.  docs->off must ascend and end at the
 * number of vectors: a malformed field gives wrong bits or reads outside docs->vec.
 *
 * rf_maxsim_topk: per query b the best k (1..RF_MAX_K) entries of scores_dev[seg_off_dev[b] .. seg_off_dev[b + 1])
 * by (score descending, position in the segment ascending); -inf and NaN entries are never hits; floats order
 * by their bit patterns (-0.0 below +0.0; rf_maxsim never gives -0.0).  The id of a hit is rows_dev[seg_off_dev[b]
 * + position], or id_base + position when rows_dev is NULL -- (score descending, row ascending) there.  Outputs
 * [B, k], padded with -inf / -1 as rf_sparse_search pads; exact_out (nullable) holds the scores as doubles.  One
 * workgroup per query: a radix selection on the bit patterns and an ordered emit; integers only, LDS counters
 * whose arrival order shows nowhere: the same bits on every run.  Segments of 0 to 2^40 entries.
 * Stream-ordered, no allocation, no host sync, no workspace.  RF_ERR_INVALID before any launch: a null or
 * misaligned pointer (but the two nullable ones), B < 1, k outside 1..RF_MAX_K.
 * New in this build; the reference has no late-interaction stage. */
#define RF_MAXSIM_QTOK 32   /* token slots of one query */
#define RF_MAXSIM_DIM 128   /* largest token vector */
typedef struct rf_token_head {      /* caller keeps alive for the call */
  const void* proj_w;               /* [dim, H] device fp16, nn.Linear layout, no bias, 16-byte aligned */
  int32_t dim;                      /* a multiple of 16, 16..RF_MAXSIM_DIM */
  const uint32_t* skip;             /* NULL, or a device bitmap over the vocabulary (ceil(vocab / 32) words):
                                       tokens whose id is set are dropped */
  int32_t vocab;
} rf_token_head;
typedef struct rf_token_field {
  const void* vec;                  /* device fp16 [n_tok, dim], 16-byte aligned */
  const int64_t* off;               /* device [n_rows + 1], ascending, off[n_rows] = n_tok */
  int64_t n_rows;
  int32_t dim;
} rf_token_field;
size_t rf_encode_tokens_workspace_bytes(const rf_encoder_t* enc, int B, int T);
int rf_encode_tokens(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev, int B, int T,
                     const rf_token_head* head, int32_t* out_off_dev, void* out_vec_dev, void* workspace_dev,
                     size_t workspace_bytes, void* stream);
int rf_maxsim(const rf_token_field* docs, const void* q_vec_dev, const int32_t* q_len_dev, int B,
              const int64_t* cand_off_dev, const int64_t* cand_row_dev, const void* filter_dev, float* scores_dev,
              void* stream);
int rf_maxsim_topk(const float* scores_dev, const int64_t* seg_off_dev, const int64_t* rows_dev, int B, int k,
                   int64_t id_base, float* scores_out, int64_t* ids_out, double* exact_out, void* stream);

/* Entity tagging: a BertForTokenClassification head over the same encoder, and the BIO grouping of its labels
 * into entities (the `transformers` token-classification pipeline's group_entities rule, in integers).
 *
 * rf_tag_logits: ids_dev int32 [B, T], lens_dev int32 [B] as for rf_encode -- single-segment rows [CLS] text
 * [SEP], token types 0.  The layers are rf_encode's; the forward opens with the embedder's embedding launch and
 * closes with one launch (csrc/tagger.hip) on the last hidden states x_t where rf_encode_tokens reads them:
 *   l[t][c] = cls_w[c] . x_t + cls_b[c]   for t < lens[b], c < num_labels
 * an fma chain over k = 0 .. H - 1 ascending from 0.f, then one fp32 add of the bias: a function of the row's own
 * hidden states alone.  logits_dev is float [B, T, num_labels]; positions >= lens[b] are untouched.  The workspace
 * is rf_encode's (rf_encode_workspace_bytes: the hidden states already live there).  Always plain launches; the
 * cached hipGraphs are rf_encode's alone.
 * Before any launch -- RF_ERR_INVALID: a null or misaligned pointer (cls_w: 16 bytes), B or T < 1.
 * RF_ERR_UNSUPPORTED: num_labels outside 1..RF_TAGGER_MAX_LABELS, T > max_position, T > 512.
 * RF_ERR_CAPACITY: workspace too small or misaligned.
 *
 * rf_group_entities: one workgroup per row of logits_dev float [B, T, L] (rf_tag_logits', or any other), no
 * workspace, no forward.  lens_dev [B] is clamped to 0..T; word_start_dev uint8 [B, T] is read under RF_TAG_FIRST
 * only (1 = the token starts a word) and may be NULL under RF_TAG_SIMPLE; label_tag_dev int32 [L] names the tag of
 * each label ("B-ORG" and "I-ORG" share one), label_begin_dev uint8 [L] is 1 for the B- labels.
 *   context   positions 1 .. lens - 2 ([CLS] and the closing [SEP] excluded); lens < 3: no units, count 0
 *   unit      RF_TAG_SIMPLE: every context token.  RF_TAG_FIRST: a run that starts at a context token with
 *             word_start = 1 and takes the tokens with word_start = 0 behind it; the first context token always
 *             starts a unit
 *   label     of a unit: argmax over c of the logits of its FIRST token, the smallest c among equals
 *   score     of a unit: 1 / sum_c exp(l_c - l_max) over that token's logits, summed in fp64 with c ascending,
 *             rounded to fp32 once (the softmax probability of the label)
 *   groups    unit u joins the running group iff label_tag[label_u] == label_tag[label of the unit before it]
 *             and label_begin[label_u] == 0; otherwise it starts a group
 *   rf_entity tag = the tag of the group's first unit; first = the first token of its first unit, last = the last
 *             token of its last unit; score = (its units' fp32 scores summed as fp64 in position order) / (their
 *             number), rounded to fp32 once
 *   output    groups whose tag == ignore_tag are dropped (-1 drops none); the others are written in position
 *             order.  count_dev[b] = how many survive, also beyond max_entities; ent_dev [B, max_entities] holds
 *             the first max_entities of them, the unused slots are (-1, -1, -1, -inf)
 *   tokens    tok_label_dev int32 / tok_score_dev float [B, T] (each nullable): the RF_TAG_SIMPLE label and score
 *             of every context token, whatever the strategy; other positions are untouched
 * Integers and fixed-order sums only: no atomics, no arrival-order reduction, the same bits on every run.  Table
 * indices are clamped: malformed lens give wrong numbers, never an access out of range.  Logits are expected
 * finite.  Stream-ordered, no allocation, no host sync.
 * RF_ERR_INVALID before any launch: a null pointer (but the nullable ones; word_start_dev under RF_TAG_FIRST is
 * not), B < 1, T outside 1..512, L outside 1..RF_TAGGER_MAX_LABELS, strategy outside {0, 1}, max_entities outside
 * 1..RF_TAGGER_MAX_ENTITIES.
 * The pipeline's MAX and AVERAGE strategies compare softmax values across tokens, which is no function of the
 * logits' order alone; they are not offered.
 * New in this build; the reference tags entities with a hosted LLM (FinRag_knowledge_graph/entity/extraction.py). */
#define RF_TAGGER_MAX_LABELS 64
#define RF_TAGGER_MAX_ENTITIES 128   /* groups reported per row */
#define RF_TAG_SIMPLE 0              /* unit = token */
#define RF_TAG_FIRST 1               /* unit = word, labelled by its first token */
typedef struct rf_tag_head {         /* caller keeps alive for the call */
  const void* cls_w;                 /* [num_labels, H] classifier.weight, device fp16, 16-byte aligned */
  const void* cls_b;                 /* [num_labels] */
  int32_t num_labels;
} rf_tag_head;
typedef struct rf_entity {
  int32_t first, last;               /* token positions in the row, inclusive; -1, -1 = none */
  int32_t tag;
  float score;
} rf_entity;
int rf_tag_logits(const rf_encoder_t* enc, const int32_t* ids_dev, const int32_t* lens_dev, int B, int T,
                  const rf_tag_head* head, float* logits_dev, void* workspace_dev, size_t workspace_bytes,
                  void* stream);
int rf_group_entities(const float* logits_dev, const int32_t* lens_dev, const uint8_t* word_start_dev, int B, int T,
                      int L, const int32_t* label_tag_dev, const uint8_t* label_begin_dev, int strategy,
                      int ignore_tag, int max_entities, int32_t* tok_label_dev, float* tok_score_dev,
                      rf_entity* ent_dev, int32_t* count_dev, void* stream);

/* ---- tokenizer: the text -> token-id stage in front of rf_encode ------------------------
 * Reference: the WordPiece tokenizer SentenceTransformer('all-MiniLM-L6-v2') loads by name
 * (vector_rag_mcp/main.py:41,50; "chunking_storing (1).py":8,380).  Host code, multi-threaded.
 * ASCII text is tokenised end to end; text with non-ASCII characters must be pre-normalised by
 * the caller (rag_fin_amd/tokenizer.py does it with Python's unicodedata: clean, NFC, lower,
 * NFD, strip Mn, CJK / non-ASCII punctuation padded with spaces).
 * vocab_utf8: the vocabulary file's bytes, one token per line, line i = id i. */
typedef struct rf_tokenizer rf_tokenizer_t;
int rf_tokenizer_create(rf_tokenizer_t** out, const char* vocab_utf8, size_t vocab_bytes,
                        int do_lower_case, int max_chars_per_word);
int rf_tokenizer_destroy(rf_tokenizer_t* t);
/* Non-ASCII code points to split off as punctuation (Unicode category P*), so that text whose
 * non-ASCII characters are all "simple" (caseless, no decomposition, not a mark / space /
 * control / CJK ideograph) needs no pre-normalisation.  cps: int32 [n], any order. */
int rf_tokenizer_set_punctuation(rf_tokenizer_t* t, const int32_t* cps, int n);
/* ids5 <- { [UNK], [CLS], [SEP], [PAD], [MASK] (-1 if absent) } */
int rf_tokenizer_special_ids(const rf_tokenizer_t* t, int32_t* ids5);
/* char_offsets int64 [n + 1] (ascending, in code points, char_offsets[0] = 0) -> byte_offsets int64 [n + 1]
 * into text_bytes (the n texts' UTF-8 bytes back to back, n_bytes in all): lets a host encode a whole batch
 * with one call of its runtime and hand over per-text CHARACTER counts.  -1 if the counts do not match the
 * blob.  Host helper of rf_tokenize_batch; no reference counterpart. */
int rf_utf8_offsets(const char* text_bytes, int64_t n_bytes, const int64_t* char_offsets, int n,
                    int64_t* byte_offsets);
/* text_bytes: the n texts' UTF-8 bytes back to back, text i = [offsets[i], offsets[i+1]).
 * ids_out int32 [n, max_len] ([CLS] ids [SEP], padded with [PAD]); lens_out int32 [n].
 * n_threads <= 0: one per hardware thread (at most 64). */
int rf_tokenize_batch(const rf_tokenizer_t* t, const char* text_bytes, const int64_t* offsets, int n,
                      int max_len, int32_t* ids_out, int32_t* lens_out, int n_threads);

/* ---- analyzer: texts -> the term-id stream that rf_sparse_count_plan consumes -------------------
 * The basic tokenisation in front of the lexical index, host code, multi-threaded: the
 * ASCII rules rf_tokenize_batch applies before its WordPiece step -- ASCII control characters dropped
 * without splitting on them, " \t\n\r" the whitespace, A-Z lower-cased, every character of the four
 * ASCII punctuation ranges and every code point of punct_cps (int32 [n_punct], any order; NULL with
 * 0) a term of its own, every other byte sequence a word character.  Text with other non-ASCII
 * characters is pre-normalised by the caller (rag_fin_amd/lexical.py, analyze_native).
 * text_bytes / offsets int64 [n + 1]: as in rf_tokenize_batch.  Malformed UTF-8 is memory-safe (a
 * sequence cut short ends with its text) and gives terms that are not UTF-8.
 * The result, behind the handle:
 *   dictionary  the distinct terms in ascending order of their UTF-8 BYTES (= code-point order, the
 *               order of Python's sorted() on str); term id = position.  vocab_blob holds every term
 *               followed by '\n' (no term contains one), vocab_off int64 [n_terms + 1] where each
 *               starts: term t = blob[vocab_off[t], vocab_off[t + 1] - 1).
 *   tok         int32 [n_tokens]: the term id of every token in text order, texts back to back
 *   dl          int64 [n]: the tokens of every text
 * The result does not depend on n_threads (<= 0: one per hardware thread, at most 64; at least 64
 * texts per thread).  rf_analysis_sizes: sizes4 <- { n, n_tokens, n_terms, bytes of vocab_blob }.
 * rf_analysis_read copies into the caller's arrays; a NULL array is skipped.  More than 2^31 - 1
 * distinct terms: RF_ERR_INVALID.  Host memory that ran out, in the call or in one of its threads:
 * RF_ERR_CAPACITY (*out stays NULL, nothing is leaked), so that a caller can tell it from a bad argument.  New in this build; the reference has no lexical index. */
typedef struct rf_analysis rf_analysis_t;
int rf_analyze(const char* text_bytes, const int64_t* offsets, int64_t n, const int32_t* punct_cps, int n_punct,
               int n_threads, rf_analysis_t** out);
int rf_analysis_sizes(const rf_analysis_t* a, int64_t* sizes4);
int rf_analysis_read(const rf_analysis_t* a, char* vocab_blob, int64_t* vocab_off, int32_t* tok, int64_t* dl);
int rf_analysis_destroy(rf_analysis_t* a);

/* ---- faceted counts: how many passing rows hold each value of a field, and range counts ----------
 * Collection.facets(fields, expr, ...): counts per value of dictionary-coded columns among the rows a
 * filter passes (the definition in numpy: rag_fin_amd/facets.py, facets_reference).
 * Everything is an integer and every add commutes, so the same inputs give the same bits on every run;
 * there is no float atomic and no sum of values.  All calls are stream-ordered, allocate nothing and do
 * not synchronise; RF_ERR_INVALID comes from host-side checks before any device call.
 *
 * A field (rf_facet_field, HOST memory, at most RF_FACET_MAX_FIELDS per call: they travel in the launch
 * arguments) is one of
 *   RF_FACET_CODES    a_dev int32 codes [n_rows]: one unit per passing row, bin = the code
 *   RF_FACET_ARRAY    a_dev int64 offsets [n_rows + 1], b_dev int32 element codes [nnz], c_dev uint8 [nnz]
 *                     first-occurrence flags (rf_array_first_occurrence): one unit per passing row and
 *                     DISTINCT code the row holds (the flagged elements); a passing row without elements
 *                     adds one to the `missing` bin
 *   RF_FACET_DYNAMIC  a_dev uint8 tags [n_rows], b_dev int64 payload [n_rows] (the tagged column of
 *                     "dynamic fields"): a string adds to the bin of its code, a bool to bin n_codes +
 *                     payload (False, True); every other passing row (absent, int, double) is `missing`
 * n_codes is the dictionary size; the field has n_bins = n_codes (DYNAMIC: n_codes + 2) value bins and its
 * counters are counters_dev[counter_off .. counter_off + n_bins], the last one `missing`.  A code outside
 * [0, n_codes) is counted nowhere and never dereferenced.
 *
 * rf_facet_counts: ONE launch for all fields, grid (workgroups, fields).  filter_dev is a filter buffer
 * for n_rows rows (rf_filter_eval / rf_filter_from_mask), or NULL for every row -- the same counters as a
 * filter that passes every row.  Only the filter's list of passing 32-row blocks is walked: a filter that
 * passes 1 % of the blocks reads 1 % of the columns.  A wave first merges the lanes that hit the same bin
 * (a ballot per distinct bin, a few rounds), then adds into a workgroup-private LDS histogram when
 * n_codes <= RF_FACET_LDS_CODES, and the workgroup does one global int64 add per non-zero bin; a larger
 * dictionary adds straight into global memory with integer atomics.  ARRAY: a wave owns one passing
 * block, keeps its 33 offsets in registers, strides over the block's contiguous element span and finds
 * each flagged element's row by a binary search over the offsets (shuffles).  The call zeroes
 * counters_dev[0 .. n_counters) first.  A filter built for another row count passes nothing.
 *
 * rf_array_first_occurrence: flags_dev[e] = 1 iff no earlier element of the same row holds values_dev[e],
 * for the elements of rows [row_lo, row_hi); a wave per row, every lane stops at its first duplicate.  The
 * store runs it once per mirrored span and keeps the bytes beside the CSR mirror (appended on sync,
 * gathered on compact: a row's content never changes in place), so no facet call scans a row for
 * duplicates.
 *
 * rf_facet_select: per field the `limit` (1..RF_FACET_MAX_LIMIT) best bins by (count descending, value
 * rank ascending) among the bins with count >= min_count (>= 1); rank_dev int32 [n_bins] is the position
 * of each bin's value in the sorted dictionary (dictionaries are first-seen order: the code is not the
 * rank), distinct per field.  One workgroup per field: an 8-pass radix select over the 64-bit key
 * (count << 32 | ~rank) finds the limit-th best key exactly -- ties at the cut are resolved by rank on the
 * device -- then the keys at or above it are gathered and sorted in LDS.  out_dev int64
 * [n_fields][RF_FACET_SCALARS + 2 * limit]: { selected, distinct (bins with count >= 1), the sum of the
 * selected counts, missing, the sum of all value bins, 0, 0, 0 }, then `limit` counts, then `limit` bin
 * numbers (best first; -1 / 0 past `selected`).  Only that crosses PCIe, whatever the dictionary size.
 * Counts must be below 2^32 (n_rows of a filter buffer is).
 *
 * rf_facet_ranges: one numeric column (is_f64: fp64, else int64) under the same filter; range r counts the
 * passing rows with lo[r] <= x < hi[r] (flags: RF_FRANGE_NO_LO / RF_FRANGE_NO_HI drop a bound,
 * RF_FRANGE_EMPTY counts nothing), n_ranges in 1..RF_FACET_MAX_RANGES, ranges may overlap.  int64 compares
 * as int64 (bounds in ilo / ihi), fp64 by IEEE comparison (flo / fhi): a NaN falls in no range and is
 * counted apart.  Per-wave ballots, per-workgroup LDS partials, then integer adds; min and max go through
 * an order-preserving unsigned 64-bit key and integer atomicMax alone (the minimum is kept as the maximum of the
 * complemented key, so that the zeroed buffer is the identity of both), so they do not depend on the arrival order.  out_dev int64 [RF_FACET_MAX_RANGES + 4]: the range counts, then { NaN rows, non-NaN rows,
 * min, max } -- min / max as the value's own bits (int64, or the fp64's), undefined when no non-NaN row
 * passes.  Which sign a tie between -0.0 and +0.0 returns as min / max is unspecified.
 * New in this build; the reference counts its collection on the host. */
#define RF_FACET_MAX_FIELDS 16
#define RF_FACET_LDS_CODES 4096
#define RF_FACET_MAX_LIMIT 1000
#define RF_FACET_SCALARS 8
#define RF_FACET_MAX_RANGES 64
#define RF_FACET_CODES 1
#define RF_FACET_ARRAY 2
#define RF_FACET_DYNAMIC 3
#define RF_FRANGE_NO_LO 4
#define RF_FRANGE_NO_HI 8
#define RF_FRANGE_EMPTY 16
typedef struct rf_facet_field {
  int32_t kind;             /* RF_FACET_* */
  int32_t n_codes;          /* dictionary size, >= 0 */
  const void* a_dev;        /* CODES: codes; ARRAY: offsets; DYNAMIC: tags */
  const void* b_dev;        /* ARRAY: element codes; DYNAMIC: payload; CODES: unused */
  const void* c_dev;        /* ARRAY: first-occurrence flags; else unused */
  const int32_t* rank_dev;  /* rf_facet_select: [n_bins]; rf_facet_counts does not read it */
  int64_t counter_off;      /* the field's n_bins + 1 counters start here */
} rf_facet_field;
typedef struct rf_facet_range {
  int32_t flags;            /* RF_FRANGE_NO_LO | RF_FRANGE_NO_HI | RF_FRANGE_EMPTY */
  int32_t pad;
  int64_t ilo, ihi;         /* int64 column: ilo <= x < ihi */
  double flo, fhi;          /* fp64 column: flo <= x < fhi */
} rf_facet_range;
int rf_facet_counts(const void* filter_dev, const rf_facet_field* fields_host, int n_fields, int64_t n_rows,
                    int64_t* counters_dev, int64_t n_counters, void* stream);
int rf_array_first_occurrence(const int64_t* offsets_dev, const int32_t* values_dev, int64_t row_lo, int64_t row_hi,
                              uint8_t* flags_dev, void* stream);
int rf_facet_select(const rf_facet_field* fields_host, int n_fields, const int64_t* counters_dev, int64_t n_counters,
                    int limit, int64_t min_count, int64_t* out_dev, void* stream);
int rf_facet_ranges(const void* filter_dev, const void* column_dev, int is_f64, const rf_facet_range* ranges_host,
                    int n_ranges, int64_t n_rows, int64_t* out_dev, void* stream);

/* ---- metric aggregations: exact sum, count, min, max of numeric columns per facet bucket -----------
 * Collection.facets(..., metrics=[...]) and query(expr, ["sum(f)", ...]): for up to RF_STATS_MAX_METRICS
 * numeric columns (rf_stats_metric, HOST memory: column_dev int64 or fp64 [n_rows], is_f64) the count, the
 * NaN count, the EXACT sum, the minimum and the maximum over the units of every bucket rf_facet_select
 * selected, and over all passing rows (the definition: rag_fin_amd/facets.py,
 * stats_reference).  An fp64 sum is the exact sum of the finite values rounded ONCE to the nearest double,
 * ties to even (what math.fsum returns): a finite double is M * 2^(p - 1074) with a 53-bit M, so the value
 * is added, as three pieces below 2^32 of M << (p & 31), into limbs p >> 5, + 1, + 2 of a fixed-point
 * accumulator of 66 limbs (limb j weighs 2^(32 j - 1074)) kept in int64 words; integer adds commute, so the
 * accumulator -- and the result -- has the same bits on every run, whatever the grid, the filter or the
 * arrival order.  An int64 value adds its low 32 bits (unsigned) to limb 0 and its high 32 bits (signed) to
 * limb 1.  There is no float atomic anywhere.  All calls are stream-ordered, allocate nothing and do not
 * synchronise; RF_ERR_INVALID comes from host-side checks before any device call.
 *
 * Records.  One record of RF_STATS_WORDS int64 words per (field, selected bucket, metric): 66 limbs, then
 * { count (non-NaN values), nan, +inf values, -inf values, min, max } -- min as the largest complement of
 * the order-preserving key of rf_facet_ranges, max as the largest key, so that a zeroed record is the
 * identity of both.  Field f has n_slots = min(limit, n_bins) slots; its records start at record
 * n_metrics * (the slots of the fields before it), record (slot, metric) at slot * n_metrics + metric;
 * behind the last field come the n_metrics records of the one-slot group of ALL passing rows.
 * rf_facet_stats_records returns the record count of a call (-1 on a bad argument).
 * Limits: n_rows <= 2^31 - 1 (a limb takes one piece below 2^32 per value, so it stays inside an int64 for
 * fewer than 2^31 values; a larger n_rows is RF_ERR_INVALID), n_metrics in 1..RF_STATS_MAX_METRICS,
 * n_fields in 0..RF_FACET_MAX_FIELDS (0: the all-rows group alone -- no value field, no select),
 * limit in 1..RF_FACET_MAX_LIMIT.
 *
 * rf_facet_stats_slots: select_dev is rf_facet_select's out_dev, still on the device (no host round
 * trip); slot_of_dev int32 [n_counters], laid out as the counters are: slot_of[counter_off + bin] = the
 * position of the bin among the field's selected buckets, -1 for every other bin.
 *
 * rf_facet_stats: ONE launch for all fields and metrics, grid (workgroups, n_fields + 1); the last column
 * is the all-rows group.  It walks the filter's passing 32-row blocks with the code of rf_facet_counts:
 * the same units (a passing row of a CODES / DYNAMIC field; a passing row and DISTINCT element of an ARRAY
 * field, by the first-occurrence flags and the owner search), maps bin -> slot, skips -1 and `missing`,
 * and per metric classifies the row's value as NaN (counted in nan, nothing else), +-inf (counted, min /
 * max, its own counter) or finite (counted, min / max, three limb adds).  64-bit integer atomics only:
 * into a workgroup-private LDS copy of the field's records when n_slots * n_metrics <=
 * RF_STATS_LDS_RECORDS (36 KiB), flushed with one global add / max per non-zero word; straight into
 * acc_dev beyond that.  The call zeroes acc_dev[0 .. n_records * RF_STATS_WORDS) first.  grid: workgroups
 * per column, 0 for the default (tests compare grids: the result does not depend on it).
 *
 * rf_facet_stats_finish: one lane per record.  It propagates the carries through the limbs into sign and
 * magnitude, finds the top bit, takes 53 bits with guard and sticky, rounds to nearest even (below 2^-1022
 * nothing is rounded: every sum is a multiple of 2^-1074), maps overflow to +-inf, and applies the inf
 * rule: NaN when +inf and -inf both occur, that infinity when one does.  An exact zero is +0.0.  The
 * routine is csrc/exact_sum.h, which a host test compiles too.  out_dev int64 [n_records][RF_STATS_OUT]:
 * { count, nan, the sum's bits, 0, min, max, 0, 0 } for an fp64 metric (min / max as the values' bits),
 * { count, 0, limb 0, limb 1, min, max, 0, 0 } for an int64 one: the exact sum is limb 0 + limb 1 * 2^32,
 * formed on the host, since it may exceed 64 bits.  min / max are undefined when count is 0.  The
 * records' limbs are consumed.  Only out_dev is downloaded.
 * New in this build; the reference sums on the host, in row order. */
#define RF_STATS_MAX_METRICS 4
#define RF_STATS_WORDS 72
#define RF_STATS_OUT 8
#define RF_STATS_LDS_RECORDS 64
typedef struct rf_stats_metric {
  const void* column_dev;   /* int64 or fp64 [n_rows] */
  int32_t is_f64;
  int32_t pad;
} rf_stats_metric;
int64_t rf_facet_stats_records(const rf_facet_field* fields_host, int n_fields, int n_metrics, int limit);
int rf_facet_stats_slots(const rf_facet_field* fields_host, int n_fields, const int64_t* select_dev, int limit,
                         int32_t* slot_of_dev, int64_t n_counters, void* stream);
int rf_facet_stats(const void* filter_dev, const rf_facet_field* fields_host, int n_fields,
                   const rf_stats_metric* metrics_host, int n_metrics, const int32_t* slot_of_dev, int64_t n_counters,
                   int limit, int64_t n_rows, int64_t* acc_dev, int64_t n_records, int grid, void* stream);
int rf_facet_stats_finish(int64_t* acc_dev, const rf_stats_metric* metrics_host, int n_metrics, int64_t n_records,
                          int64_t* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RAGFIN_H */
