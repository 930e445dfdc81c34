"""ctypes binding of libragfin_hip.so (include/ragfin.h).

There is no CPU fallback: if the library cannot be loaded, or a call returns a
non-zero status, an exception is raised.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64,
                    c_size_t, c_uint32, c_void_p)

from . import build as _build

RF_OK = 0
RF_MAX_K = 64
RF_QCHUNK = 64
RF_SMALL_ROWS = 8192      # rows up to which every row is a candidate (no sample pass, no shadow chain)
RF_FLAG_CAND_OVERFLOW = 1
RF_FLAG_TIE_OVERFLOW = 2
RF_GROUP_MAX_CODES = 64   # dictionary size the fused grouped path serves (include/ragfin.h)
# lexical search (include/ragfin.h, "lexical search")
RF_SPARSE_MAX_TERMS = 64     # distinct known terms of one query
RF_SPARSE_TILE_ROWS = 8192   # rows a workgroup of the posting scan accumulates in LDS
RF_FUSE_MAX_ARMS = 4         # answers rf_fuse_rrf fuses
# boosted search (include/ragfin.h, "boosted search")
RF_BOOST_MAX = 3             # boosts of one search: 2^3 = 8 row classes, the most rf_merge_boosted takes
# decayed search (include/ragfin.h, "decayed search"): the function codes of rf_decay_weights
RF_DECAY_GAUSS, RF_DECAY_EXP, RF_DECAY_LINEAR = 0, 1, 2
# keyword filters (include/ragfin.h, "keyword filters")
RF_TEXT_MATCH = 1
RF_TEXT_PHRASE = 2
RF_TEXT_MAX_LEAVES = 16      # text leaves one rf_text_match call (one filter expression) holds
# user-defined scalar fields (include/ragfin.h, "user-defined scalar fields")
RF_COLUMN_MAX_LEAVES = 16    # column leaves one rf_column_match call (one filter expression) holds
RF_COLUMN_MAX_SET = 65536    # values of one INT64 `in` list
RF_CLEAF_CODESET, RF_CLEAF_I64_RANGE, RF_CLEAF_I64_SET, RF_CLEAF_F64_RANGE = 1, 2, 3, 4
# dynamic fields (include/ragfin.h, "dynamic fields")
RF_DYNAMIC_MAX_LEAVES = 16   # dynamic leaves one rf_dynamic_match call holds
RF_DTAG_ABSENT, RF_DTAG_BOOL, RF_DTAG_INT, RF_DTAG_DOUBLE, RF_DTAG_STRING = range(5)
RF_DLEAF_TAGS, RF_DLEAF_STR_CODESET, RF_DLEAF_BOOL, RF_DLEAF_NUM_RANGE, RF_DLEAF_NUM_SET = 1, 2, 3, 4, 5
# ARRAY fields (include/ragfin.h, "ARRAY fields")
RF_ARRAY_MAX_LEAVES = 16     # array leaves one rf_array_match call holds
RF_ALEAF_LENGTH, RF_ALEAF_ELEM, RF_ALEAF_MATCH = 1, 2, 3
RF_AELEM_CODE, RF_AELEM_I64, RF_AELEM_F64 = 1, 2, 3
RF_ARRAY_MAX_ALL = 64        # needles of one ARRAY_CONTAINS_ALL: one bit each of a row's 64-bit slot
# faceted counts (include/ragfin.h, "faceted counts")
RF_FACET_MAX_FIELDS = 16     # fields one rf_facet_counts / rf_facet_select call holds
RF_FACET_LDS_CODES = 4096    # dictionary size up to which a workgroup counts in an LDS histogram
RF_FACET_MAX_LIMIT = 1000    # bins rf_facet_select returns per field, at most
RF_FACET_SCALARS = 8         # int64 scalars in front of a field's selected counts and bins
RF_FACET_MAX_RANGES = 64     # ranges of one rf_facet_ranges call
RF_FACET_CODES, RF_FACET_ARRAY, RF_FACET_DYNAMIC = 1, 2, 3
RF_FRANGE_NO_LO, RF_FRANGE_NO_HI, RF_FRANGE_EMPTY = 4, 8, 16
# metric aggregations (include/ragfin.h, "metric aggregations")
RF_STATS_MAX_METRICS = 4     # metric columns of one rf_facet_stats call
RF_STATS_WORDS = 72          # int64 words of an accumulator record: 66 limbs, count, nan, +inf, -inf, min, max
RF_STATS_OUT = 8             # int64 words of a finished record
RF_STATS_LDS_RECORDS = 64    # records of a field up to which a workgroup accumulates in LDS
# lexical index maintenance (include/ragfin.h, "lexical index maintenance")
RF_LEX_CHUNK = 1024          # postings per workgroup, and the tile of the second level of the prefix sum
# lexical index build (include/ragfin.h, "lexical index build")
RF_LEX_SORT_TILE = 4096      # tokens per workgroup of a radix-sort pass


class RagfinError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libragfin_hip error {code}: {msg}")
        self.code = code


class EncoderConfig(Structure):
    _fields_ = [("vocab_size", c_int32), ("hidden", c_int32), ("layers", c_int32),
                ("heads", c_int32), ("intermediate", c_int32), ("max_position", c_int32),
                ("type_vocab", c_int32), ("ln_eps", c_float)]


# filtered search (include/ragfin.h, "filtered search")
RF_FILTER_MAX_OPS = 64
RF_FILTER_MAX_DEPTH = 32
RF_FILTER_COLUMNS = 4
RF_FOP_CODESET, RF_FOP_RANGE, RF_FOP_ROWLIST, RF_FOP_TRUE, RF_FOP_FALSE, RF_FOP_AND, RF_FOP_OR, RF_FOP_NOT = range(1, 9)
RF_FOP_BITMAP = 9
RF_FRANGE_LO_INCL = 1
RF_FRANGE_HI_INCL = 2


class FilterOp(Structure):
    _fields_ = [("op", c_int32), ("column", c_int32), ("off", c_int32), ("len", c_int32),
                ("flags", c_int32), ("pad", c_int32), ("lo", c_double), ("hi", c_double)]


class TextLeaf(Structure):
    _fields_ = [("kind", c_int32), ("term_off", c_int32), ("n_terms", c_int32), ("min_match", c_int32)]


class ColumnLeaf(Structure):
    """rf_column_leaf: one leaf of a filter expression over an extra column."""
    _fields_ = [("kind", c_int32), ("flags", c_int32), ("column_dev", c_void_p), ("off", c_int64), ("len", c_int64),
                ("ilo", c_int64), ("ihi", c_int64), ("flo", c_double), ("fhi", c_double)]


class DynamicLeaf(Structure):
    """rf_dynamic_leaf: one leaf of a filter expression over a dynamic key's tagged column."""
    _fields_ = [("kind", c_int32), ("flags", c_int32), ("tags_dev", c_void_p), ("payload_dev", c_void_p),
                ("off", c_int64), ("len", c_int64), ("foff", c_int64), ("flen", c_int64),
                ("ilo", c_int64), ("ihi", c_int64), ("flo", c_double), ("fhi", c_double)]


class ArrayLeaf(Structure):
    """rf_array_leaf: one leaf of a filter expression over an ARRAY field's CSR mirror."""
    _fields_ = [("kind", c_int32), ("elem", c_int32), ("flags", c_int32), ("need", c_int32),
                ("offsets_dev", c_void_p), ("values_dev", c_void_p), ("index", c_int64),
                ("off", c_int64), ("len", c_int64), ("ilo", c_int64), ("ihi", c_int64),
                ("flo", c_double), ("fhi", c_double)]


class FacetField(Structure):
    """rf_facet_field: one field of a faceted count (a coded column, a CSR array of codes, a dynamic key)."""
    _fields_ = [("kind", c_int32), ("n_codes", c_int32), ("a_dev", c_void_p), ("b_dev", c_void_p), ("c_dev", c_void_p),
                ("rank_dev", c_void_p), ("counter_off", c_int64)]


class StatsMetric(Structure):
    """rf_stats_metric: one numeric column of a metric aggregation."""
    _fields_ = [("column_dev", c_void_p), ("is_f64", c_int32), ("pad", c_int32)]


class FacetRange(Structure):
    """rf_facet_range: one [lo, hi) range of rf_facet_ranges."""
    _fields_ = [("flags", c_int32), ("pad", c_int32), ("ilo", c_int64), ("ihi", c_int64), ("flo", c_double),
                ("fhi", c_double)]


class Postings(Structure):
    """rf_postings: one set of posting arrays in device memory (lexical index maintenance)."""
    _fields_ = [("n_rows", c_int64), ("n_terms", c_int64), ("nnz", c_int64), ("n_pos", c_int64),
                ("post_off", c_void_p), ("post_row", c_void_p), ("post_tf", c_void_p), ("pos_off", c_void_p),
                ("pos", c_void_p)]


ENCODER_WEIGHT_FIELDS = ["word_emb", "pos_emb", "type_emb", "emb_ln_g", "emb_ln_b", "qkv_w",
                         "qkv_b", "ao_w", "ao_b", "ln1_g", "ln1_b", "ff1_w", "ff1_b", "ff2_w",
                         "ff2_b", "ln2_g", "ln2_b"]


class EncoderWeights(Structure):
    _fields_ = [(n, c_void_p) for n in ENCODER_WEIGHT_FIELDS]


class PairHead(Structure):
    """rf_pair_head: the pooler and classifier of a cross-encoder (device fp16 pointers)."""
    _fields_ = [("pool_w", c_void_p), ("pool_b", c_void_p), ("cls_w", c_void_p), ("cls_b", c_void_p),
                ("num_labels", c_int32)]


# extractive reading (include/ragfin.h, rf_answer_spans)
RF_READER_MAX_BEST = 16      # spans per pair one call returns
RF_READER_MAX_SPAN = 64      # tokens of the longest span
RF_READER_MAX_T = 512        # positions of a pair the span stage holds
RF_READER_MAX_CONTEXT = 65536   # tokens of one context stitched from sliding windows (rf_stitch_spans)


class QaHead(Structure):
    """rf_qa_head: qa_outputs of a BertForQuestionAnswering (device fp16 pointers)."""
    _fields_ = [("qa_w", c_void_p), ("qa_b", c_void_p)]


# learned sparse vectors (include/ragfin.h, rf_encode_terms)
RF_TERMS_MAX = 256           # terms rf_sparsify_terms keeps of one row, at most


class MlmHead(Structure):
    """rf_mlm_head: cls.predictions of a BertForMaskedLM (device fp16 pointers)."""
    _fields_ = [("tr_w", c_void_p), ("tr_b", c_void_p), ("tr_ln_g", c_void_p), ("tr_ln_b", c_void_p),
                ("dec_w", c_void_p), ("dec_b", c_void_p), ("vocab", c_int32)]


# late interaction (include/ragfin.h, rf_encode_tokens / rf_maxsim)
RF_MAXSIM_QTOK = 32          # token slots of one query
RF_MAXSIM_DIM = 128          # largest token vector


class TokenHead(Structure):
    """rf_token_head: the projection of a ColBERT model and the skip bitmap (device pointers)."""
    _fields_ = [("proj_w", c_void_p), ("dim", c_int32), ("skip", c_void_p), ("vocab", c_int32)]


class TokenField(Structure):
    """rf_token_field: the token vectors of the rows of a collection as CSR (device pointers)."""
    _fields_ = [("vec", c_void_p), ("off", c_void_p), ("n_rows", c_int64), ("dim", c_int32)]


# entity tagging (include/ragfin.h, rf_tag_logits / rf_group_entities)
RF_TAGGER_MAX_LABELS = 64    # labels of a classifier
RF_TAGGER_MAX_ENTITIES = 128   # groups reported per row
RF_TAGGER_MAX_T = 512        # positions of a row the grouping holds
RF_TAG_SIMPLE, RF_TAG_FIRST = 0, 1


class TagHead(Structure):
    """rf_tag_head: the classifier of a BertForTokenClassification (device fp16 pointers)."""
    _fields_ = [("cls_w", c_void_p), ("cls_b", c_void_p), ("num_labels", c_int32)]


# sentence-embedder families (include/ragfin.h, rf_encode_sentences)
RF_POOL_MEAN, RF_POOL_CLS, RF_POOL_MAX, RF_POOL_MEAN_SQRT_LEN = 0, 1, 2, 3


class SentenceHead(Structure):
    """rf_sentence_head: the Pooling mode and whether a Normalize module follows it."""
    _fields_ = [("pooling", c_int32), ("normalize", c_int32)]


# name -> (restype, argtypes); every symbol include/ragfin.h declares
SIGNATURES = {
    "rf_version": (c_int, []),
    "rf_build_id": (c_char_p, []),
    "rf_last_error": (c_char_p, []),
    "rf_device_check": (c_int, [c_int]),
    "rf_index_storage_bytes": (c_size_t, [c_int, c_int64]),
    "rf_index_create": (c_int, [POINTER(c_void_p), c_int, c_int64, c_void_p, c_size_t, c_int]),
    "rf_index_destroy": (c_int, [c_void_p]),
    "rf_index_add_f16": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "rf_index_size": (c_int64, [c_void_p]),
    "rf_index_dim": (c_int, [c_void_p]),
    "rf_index_reset": (c_int, [c_void_p, c_void_p]),
    "rf_index_compact": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_size_t, c_void_p]),
    "rf_index_get_rows_f16": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "rf_normalize_f32_to_f16": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "rf_search_workspace_bytes": (c_size_t, [c_void_p]),
    "rf_search": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                          c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_search_profile": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
                                  POINTER(c_float)]),
    "rf_search_exhaustive": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_search_exhaustive_after": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_filter_bytes": (c_size_t, [c_int64]),
    "rf_filter_eval": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "rf_filter_eval_bitmaps": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                       c_void_p]),
    "rf_filter_from_mask": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "rf_search_filtered": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_search_exhaustive_filtered": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                              c_void_p]),
    "rf_multi_filter_bytes": (c_size_t, [c_int64, c_int]),
    "rf_multi_filter_build": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "rf_search_multi_filtered": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int64,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_boost_class_stride_words": (c_size_t, [c_int64]),
    "rf_boost_classes": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    "rf_merge_boosted": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_double), c_int, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "rf_decay_weights": (c_int, [c_void_p, c_int, c_int64, c_int, c_double, c_double, c_double, c_double, c_void_p,
                                 c_void_p, c_void_p]),
    "rf_search_weighted": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_search_exhaustive_weighted": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_search_range": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_double, c_double, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_search_exhaustive_range": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_double, c_double,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                           c_void_p]),
    "rf_search_after": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_double, c_double, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_search_after_profile": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_double, c_double,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                        c_void_p, POINTER(c_float)]),
    "rf_search_grouped_workspace_bytes": (c_size_t, [c_void_p]),
    "rf_search_grouped": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int64,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_search_grouped_profile": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int64,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
                                          POINTER(c_float)]),
    "rf_debug_grouped_counters_offset": (c_size_t, []),
    "rf_mmr_select": (c_int, [c_void_p, c_int, c_int, c_int, c_double, c_int64, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p]),
    "rf_sparse_create": (c_int, [POINTER(c_void_p), c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int]),
    "rf_sparse_destroy": (c_int, [c_void_p]),
    "rf_sparse_search_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rf_sparse_search": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_sparse_attach_positions": (c_int, [c_void_p, c_void_p, c_void_p, c_int64]),
    "rf_text_match_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "rf_text_match": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_size_t,
                              c_void_p]),
    "rf_column_match": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "rf_dynamic_match": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "rf_array_match": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "rf_facet_counts": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int64, c_void_p]),
    "rf_array_first_occurrence": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "rf_facet_select": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p]),
    "rf_facet_ranges": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "rf_facet_stats_records": (c_int64, [c_void_p, c_int, c_int, c_int]),
    "rf_facet_stats_slots": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int64, c_void_p]),
    "rf_facet_stats": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int64, c_int, c_int64, c_void_p,
                               c_int64, c_int, c_void_p]),
    "rf_facet_stats_finish": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "rf_sparse_impacts": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_double,
                                  c_double, c_double, c_void_p, c_void_p]),
    "rf_sparse_append_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "rf_sparse_append": (c_int, [POINTER(Postings), POINTER(Postings), c_void_p, c_void_p, POINTER(Postings), c_void_p,
                                 c_size_t, c_void_p]),
    "rf_sparse_compact_workspace_bytes": (c_size_t, [c_int64]),
    "rf_sparse_compact_plan": (c_int, [POINTER(Postings), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                       c_void_p]),
    "rf_sparse_compact_apply": (c_int, [POINTER(Postings), c_void_p, c_void_p, c_void_p, POINTER(Postings), c_void_p]),
    "rf_sparse_count_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "rf_sparse_count_plan": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t,
                                     c_void_p]),
    "rf_sparse_count_apply": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_size_t, POINTER(Postings), c_int,
                                      c_void_p]),
    "rf_fuse_rrf": (c_int, [c_int, c_void_p, c_int, POINTER(c_double), c_double, c_int, c_int, c_void_p, c_void_p,
                            c_void_p, c_void_p]),
    "rf_merge_shards": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                c_void_p]),
    "rf_packed_shard_words": (c_size_t, [c_int, c_int]),
    "rf_merge_shards_packed": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rf_map_ids": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "rf_comm_unique_id": (c_int, [c_void_p]),
    "rf_comm_init": (c_int, [c_int, c_int, c_void_p, c_int, POINTER(c_void_p)]),
    "rf_comm_destroy": (c_int, [c_void_p]),
    "rf_comm_rank": (c_int, [c_void_p]),
    "rf_comm_world": (c_int, [c_void_p]),
    "rf_search_sharded_scratch_words": (c_size_t, [c_void_p, c_int, c_int]),
    "rf_search_sharded": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_int64, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "rf_tokenizer_create": (c_int, [POINTER(c_void_p), c_char_p, c_size_t, c_int, c_int]),
    "rf_tokenizer_destroy": (c_int, [c_void_p]),
    "rf_tokenizer_set_punctuation": (c_int, [c_void_p, c_void_p, c_int]),
    "rf_tokenizer_special_ids": (c_int, [c_void_p, c_void_p]),
    "rf_tokenize_batch": (c_int, [c_void_p, c_char_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int]),
    "rf_utf8_offsets": (c_int, [c_char_p, c_int64, c_void_p, c_int, c_void_p]),
    "rf_analyze": (c_int, [c_char_p, c_void_p, c_int64, c_void_p, c_int, c_int, POINTER(c_void_p)]),
    "rf_analysis_sizes": (c_int, [c_void_p, c_void_p]),
    "rf_analysis_read": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rf_analysis_destroy": (c_int, [c_void_p]),
    "rf_debug_scores": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "rf_sq8_storage_bytes": (c_size_t, [c_int, c_int64]),
    "rf_index_attach_sq8": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_index_detach_sq8": (c_int, [c_void_p]),
    "rf_search_sq8_workspace_bytes": (c_size_t, [c_void_p]),
    "rf_search_sq8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_index_set_shadow_first": (c_int, [c_void_p, c_int64]),
    "rf_search_fp16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_search_sq8_profile": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, POINTER(c_float)]),
    "rf_debug_scores_sq8": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                                    c_size_t, c_void_p]),
    "rf_index_get_rows_sq8": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rf_encoder_storage_bytes": (c_size_t, [POINTER(EncoderConfig)]),
    "rf_encoder_create": (c_int, [POINTER(c_void_p), POINTER(EncoderConfig),
                                  POINTER(EncoderWeights), c_void_p, c_size_t, c_int, c_void_p]),
    "rf_encoder_destroy": (c_int, [c_void_p]),
    "rf_encode_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rf_encode": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                          c_size_t, c_void_p]),
    "rf_score_pairs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(PairHead), c_void_p,
                               c_void_p, c_size_t, c_void_p]),
    "rf_answer_spans": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(QaHead), c_int, c_int,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_stitch_spans": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                c_void_p, c_size_t, c_void_p]),
    "rf_stitch_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "rf_encode_terms_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rf_encode_terms": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(MlmHead), c_void_p, c_void_p,
                                c_size_t, c_void_p]),
    "rf_sparsify_terms": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rf_encode_tokens_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rf_encode_tokens": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(TokenHead), c_void_p, c_void_p,
                                 c_void_p, c_size_t, c_void_p]),
    "rf_maxsim": (c_int, [POINTER(TokenField), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                          c_void_p]),
    "rf_maxsim_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    "rf_tag_logits": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(TagHead), c_void_p, c_void_p,
                              c_size_t, c_void_p]),
    "rf_encode_sentences": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(SentenceHead),
                                    c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rf_group_entities": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int,
                                  c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# present only in the experiments build (libragfin_hip_exp.so, tools/): bound when exported
EXPERIMENT_SIGNATURES = {
    "rf_set_tuning": (c_int, [c_char_p, c_int]),
    "rf_debug_workspace_offset": (c_size_t, [c_char_p]),
    "rf_debug_set_buffer": (c_int, [c_void_p]),
}

_lib = None


def library_path() -> str:
    # RAGFIN_LIB=exp: the experiments build (tools/); any other value: an explicit path
    v = os.environ.get("RAGFIN_LIB")
    if v == "exp":
        return _build.EXP_LIB_PATH
    return v or _build.LIB_PATH


def load_library() -> ctypes.CDLL:
    """Load the library, making sure it was built from the sources on disk: a missing or stale
    .so is rebuilt when hipcc is present and refused when it is not (no silent old kernels)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    in_tree = path in (_build.LIB_PATH, _build.EXP_LIB_PATH)
    exp = path == _build.EXP_LIB_PATH
    if in_tree and (not os.path.exists(path) or _build.built_digest(path) != _build.source_digest(exp)):
        # missing, or built from other sources than those on disk: rebuild where hipcc exists, refuse
        # where it does not -- no fallback.  A current library is loaded as it is: no compiler runs at import.
        if not _build.have_hipcc():
            raise RuntimeError(f"{path} is missing or was built from other sources (build id "
                               f"{_build.built_digest(path) or 'none'}, sources {_build.source_digest(exp)}) and hipcc is "
                               "not available to rebuild it; run `python -m rag_fin_amd.build` where the ROCm toolchain is")
        _build.build_lib(experiments=exp)
    elif not os.path.exists(path):
        raise RuntimeError(f"{path} does not exist")
    # torch ships its own libamdhip64; load it FIRST so that this library binds to the
    # same HIP runtime instance (loaded the other way round, the two runtimes disagree
    # about device visibility: rf_device_check saw "no HIP device" on a GPU box)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in EXPERIMENT_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    if in_tree:
        have = (lib.rf_build_id() or b"").decode()
        want = _build.source_digest(exp)
        if have != want:
            raise RuntimeError(f"{path} was built from other sources (build id {have}, sources {want}) and "
                               "hipcc is not available to rebuild it; run `python -m rag_fin_amd.build` "
                               "where the ROCm toolchain is")
    _lib = lib
    return lib


def check(code: int) -> None:
    if code != RF_OK:
        msg = load_library().rf_last_error()
        raise RagfinError(code, msg.decode() if msg else "")


def current_stream_ptr():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)
