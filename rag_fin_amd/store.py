"""HBM-resident corpus store: the in-process replacement for the reference's Milvus
collection on the vector-RAG path.

Reference surface mirrored (pymilvus `Collection`, as the reference uses it):
  schema          "chunking_storing (1).py":14-22  (id, text, embedding[384], period,
                                                   chunk_type, statement_type, primary_value)
  insert/flush/load                    same file :383-396 (seven parallel columns)
  search(data, "embedding", {"metric_type": "COSINE"}, limit, output_fields=[...])
                                        vector_rag_mcp/main.py:51-57, retrieve.py:28-34
  hit.score / hit.entity.<field>        vector_rag_mcp/main.py:59-70
  num_entities                          vector_rag_mcp/main.py:113,120,164
  query(expr="id in [...]" | "", limit, output_fields)   graph_cons.py:38-42,308-311;
                                        test_vector.py:35-39

Vectors live on the GPU (fp16, MFMA-fragment tiled); the scalar
columns stay in host Python lists, and the four a filter can test are mirrored on the
device on demand (filtered search: `search(..., expr=...)`, `query(expr=...)`,
rag_fin_amd/filter_expr.py).  All arithmetic goes through libragfin_hip.so; there is no
CPU path.

Beyond the reference: a lexical index over the `text` column (create_index("sparse", ...),
search(["query text"], anns_field="sparse", ...): BM25 on the GPU) and `hybrid_search`, which fuses
dense and BM25 arms by reciprocal rank (rag_fin_amd/lexical.py, rag_fin_amd/hybrid.py).
"""
from __future__ import annotations

import contextlib
import itertools
import json
import os
import re
import threading
import time
from typing import Any, Iterable, Sequence

import numpy as np

from . import _lib
from . import filter_expr
from . import schema as schema_
from .schema import DataType, FieldSchema  # noqa: F401
from .hybrid import MAX_ARMS, AnnSearchRequest, RRFRanker

from . import facets as facets_
from .index import (GpuIndex, MultiFilter, SparseIndex, _ptr, array_first_occurrence, array_match, facet_counts, facet_ranges, facet_stats_all, facet_stats_slots, boost_classes, column_match, dynamic_match,  # noqa: F401
                    decay_weights, eval_filter, filter_from_mask, filter_mask_bits, fuse_rrf, grouped_exhaustive, mask_words, merge_boosted,
                    plan_filter_chunks, require_gpu, rerun_flagged, text_words_per_leaf, words_mask)
from .ranker import BoostRanker, DecayRanker, check_rankers, class_weights  # noqa: F401
from .text_fields import LEARNED_FIELD, TOKEN_FIELD, LearnedSparseField, LexicalField, TokenVectorField, is_text  # noqa: F401


SCALAR_FIELDS = ("id", "text", "period", "chunk_type", "statement_type", "primary_value")
FORMAT = "ragfin-corpus-v1"   # columns.json "format"


def _torch():
    import torch
    return torch


class _StageClock:
    """The milliseconds of a call's stages, added into a caller's dict under the key of each lap.
    It synchronises the device at every lap; with no dict it does nothing at all."""

    def __init__(self, timing, device):
        self.timing, self.device = timing, device
        if timing is not None:
            _torch().cuda.synchronize(device)
            self.t = time.perf_counter()

    def lap(self, key: str) -> None:
        if self.timing is None:
            return
        _torch().cuda.synchronize(self.device)
        now = time.perf_counter()
        self.timing[key] = self.timing.get(key, 0.0) + (now - self.t) * 1e3
        self.t = now


def check_band(radius, range_filter=None):
    """Range-search bounds -> the band (radius, range_filter) as two floats, or None when neither is
    given.  A hit has radius < score <= range_filter (higher is better), compared as fp64 on the
    fp64 ranking score.  range_filter without radius, a bound that is no real number (NaN, a string,
    a bool) or radius >= range_filter raises ValueError; range_filter defaults to +inf."""
    import math
    import numbers
    if radius is None and range_filter is None:
        return None
    if radius is None:
        raise ValueError("range search: range_filter needs radius (radius switches range search on)")
    out = []
    for name, v in (("radius", radius), ("range_filter", math.inf if range_filter is None else range_filter)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or math.isnan(float(v)):
            raise ValueError(f"range search: {name} must be a real number, got {v!r}")
        out.append(float(v))
    if not out[0] < out[1]:
        raise ValueError(f"range search: need radius < range_filter, got {out[0]!r} and {out[1]!r}")
    return out[0], out[1]


MMR_MAX_FETCH_K = _lib.RF_MAX_K


MAX_WINDOW = 16384   # Milvus' result window: offset + limit at most this


def check_offset(offset, param, limit) -> int:
    """The offset of a pymilvus-shaped search: the keyword, else param["offset"], else 0.  An int
    >= 0 (no bool), and with an offset the window offset + limit <= MAX_WINDOW; else ValueError."""
    if offset is None and isinstance(param, dict):
        offset = param.get("offset")
    if offset is None:
        return 0
    if isinstance(offset, bool) or not isinstance(offset, (int, np.integer)) or offset < 0:
        raise ValueError(f"offset must be an integer >= 0, got {offset!r}")
    offset = int(offset)
    if offset and (isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or limit < 1
                   or offset + limit > MAX_WINDOW):
        raise ValueError(f"offset + limit must be an integer window of at most {MAX_WINDOW} "
                         f"(got offset = {offset}, limit = {limit!r})")
    return offset


def check_mmr(mmr_lambda, mmr_fetch_k, limit: int):
    """Diversified-search arguments -> (fetch_k, lambda), or None when neither is given.  lambda
    weighs relevance against redundancy (1 = the plain ranking, 0 = diversity only after the best
    hit); fetch_k is the number of best hits the `limit` results are picked from, by default
    min(64, max(20, 4 * limit)).  mmr_fetch_k without mmr_lambda, a lambda that is no real number in
    [0, 1] (NaN, a string, a bool), a fetch_k that is no integer, limit > fetch_k or fetch_k > 64
    raises ValueError."""
    import math
    import numbers
    if mmr_lambda is None:
        if mmr_fetch_k is not None:
            raise ValueError("diversified search: mmr_fetch_k needs mmr_lambda (mmr_lambda switches MMR on)")
        return None
    if isinstance(mmr_lambda, bool) or not isinstance(mmr_lambda, numbers.Real) or math.isnan(float(mmr_lambda)) \
            or not 0.0 <= float(mmr_lambda) <= 1.0:
        raise ValueError(f"diversified search: mmr_lambda must be a real number in [0, 1], got {mmr_lambda!r}")
    if limit < 1:
        raise ValueError("limit must be >= 1")
    if mmr_fetch_k is None:
        mmr_fetch_k = min(MMR_MAX_FETCH_K, max(20, 4 * limit))
    if isinstance(mmr_fetch_k, bool) or not isinstance(mmr_fetch_k, numbers.Integral):
        raise ValueError(f"diversified search: mmr_fetch_k must be an integer, got {mmr_fetch_k!r}")
    if mmr_fetch_k > MMR_MAX_FETCH_K:
        raise ValueError(f"diversified search: mmr_fetch_k = {mmr_fetch_k} > {MMR_MAX_FETCH_K}")
    if limit > mmr_fetch_k:
        raise ValueError(f"diversified search: limit = {limit} > mmr_fetch_k = {mmr_fetch_k}")
    return int(mmr_fetch_k), float(mmr_lambda)


class _DeviceColumns:
    """The device mirror of the four filterable scalar columns: period / chunk_type /
    statement_type as int32 codes into append-only dictionaries, primary_value as fp64.
    Synced lazily from the host lists: rows appended since the last sync are encoded; a
    shorter collection (after drop) is re-encoded from row 0 (the dictionaries stay)."""

    def __init__(self, device):
        torch = _torch()
        self.device = device
        self.dicts = {f: [] for f in filter_expr.VARCHAR_FIELDS}
        self._code = {f: {} for f in filter_expr.VARCHAR_FIELDS}
        self.codes = {f: torch.empty(0, dtype=torch.int32, device=device) for f in filter_expr.VARCHAR_FIELDS}
        self.values = torch.empty(0, dtype=torch.float64, device=device)
        self.n = 0
        # faceted counts: {key: (dictionary length, int32 value ranks on the device)} (CorpusStore._facet_rank).  The
        # dictionaries are append-only, so the same length means the same content and a kept rank stays right.
        self.facet_ranks: dict = {}

    def sync(self, columns: dict, n: int) -> None:
        torch = _torch()
        if n < self.n:
            self.codes = {f: t[:0] for f, t in self.codes.items()}
            self.values = self.values[:0]
            self.n = 0
        if n == self.n:
            return
        lo = self.n
        for f in filter_expr.VARCHAR_FIELDS:
            d, code = self.dicts[f], self._code[f]
            enc = np.empty(n - lo, dtype=np.int32)
            for j, v in enumerate(columns[f][lo:n]):
                c = code.get(v)
                if c is None:
                    c = code[v] = len(d)
                    d.append(v)
                enc[j] = c
            self.codes[f] = torch.cat([self.codes[f], torch.from_numpy(enc).to(self.device)])
        vals = np.asarray(columns["primary_value"][lo:n], dtype=np.float64)
        self.values = torch.cat([self.values, torch.from_numpy(vals).to(self.device)])
        self.n = n

    def compact(self, keep: np.ndarray) -> None:
        """Keep rows `keep` (ascending) of a mirror synced to the whole collection; the
        dictionaries are append-only and stay valid."""
        torch = _torch()
        k = torch.from_numpy(np.ascontiguousarray(keep, dtype=np.int64)).to(self.device)
        self.codes = {f: t.index_select(0, k) for f, t in self.codes.items()}
        self.values = self.values.index_select(0, k)
        self.n = int(keep.size)

    def tensors(self):
        return [self.codes[f] for f in filter_expr.VARCHAR_FIELDS] + [self.values]


class _ExtraColumn:
    """The device mirror of one column of a collection's own fields (schema.py), synced lazily from the host
    list like _DeviceColumns: int64 for INT64, fp64 for DOUBLE, and int32 codes into an append-only dictionary
    (first-seen order) for VARCHAR and BOOL -- and for an INT64 field that is grouped by (coded=True)."""

    def __init__(self, device, dtype, coded: bool = False):
        torch = _torch()
        self.device = device
        self.coded = coded or dtype in (DataType.VARCHAR, DataType.BOOL)
        self.np_dtype = np.int32 if self.coded else (np.int64 if dtype == DataType.INT64 else np.float64)
        self.dict: list = []
        self._code: dict = {}
        self.data = torch.empty(0, dtype=getattr(torch, np.dtype(self.np_dtype).name), device=device)
        self.n = 0
        # faceted counts: {key: (dictionary length, int32 value ranks on the device)} (CorpusStore._facet_rank).  The
        # dictionaries are append-only, so the same length means the same content and a kept rank stays right.
        self.facet_ranks: dict = {}

    def sync(self, values: list, n: int) -> None:
        torch = _torch()
        if n < self.n:   # a shorter collection: re-encode from row 0 (the dictionary stays)
            self.data = self.data[:0]
            self.n = 0
        if n == self.n:
            return
        lo = self.n
        if self.coded:
            d, code = self.dict, self._code
            enc = np.empty(n - lo, dtype=np.int32)
            for j, v in enumerate(values[lo:n]):
                c = code.get(v)
                if c is None:
                    c = code[v] = len(d)
                    d.append(v)
                enc[j] = c
        else:
            enc = np.asarray(values[lo:n], dtype=self.np_dtype)
        self.data = torch.cat([self.data, torch.from_numpy(enc).to(self.device)])
        self.n = n

    def compact(self, k) -> None:
        """Keep rows k (ascending, an int64 device tensor) of a mirror synced to the whole collection."""
        self.data = self.data.index_select(0, k)
        self.n = int(k.numel())


class _ArrayColumn:
    """The device mirror of one ARRAY field, CSR: offsets int64 [n + 1] (offsets[0] == 0) and the rows' elements
    back to back -- int64 for INT64, fp64 for DOUBLE, int32 codes into an append-only dictionary (first-seen
    order) for VARCHAR and BOOL.  Synced lazily and append-only from the host lists, like _ExtraColumn."""

    def __init__(self, device, element_type):
        torch = _torch()
        self.device = device
        self.coded = element_type in (DataType.VARCHAR, DataType.BOOL)
        self.np_dtype = np.int32 if self.coded else (np.int64 if element_type == DataType.INT64 else np.float64)
        self.dict: list = []
        self._code: dict = {}
        self.offsets = torch.zeros(1, dtype=torch.int64, device=device)
        self.values = torch.empty(0, dtype=getattr(torch, np.dtype(self.np_dtype).name), device=device)
        self.n = 0
        self.nnz = 0   # elements mirrored: the last offset, kept on the host
        # faceted counts: one byte per element, 1 where no earlier element of its row holds the same
        # code, for the elements of the first `first_n` rows; None until a facet reads the field
        self.first = None
        self.first_n = 0
        # faceted counts: {key: (dictionary length, int32 value ranks on the device)} (CorpusStore._facet_rank).  The
        # dictionaries are append-only, so the same length means the same content and a kept rank stays right.
        self.facet_ranks: dict = {}

    def first_occurrence(self):
        """The first-occurrence bytes of every mirrored element (coded fields): rf_array_first_occurrence over the
        rows appended since the last call, so a row is scanned for duplicates once, never per facet call."""
        torch = _torch()
        if self.first is None or self.first_n < self.n:
            full = torch.empty(self.nnz, dtype=torch.uint8, device=self.device)
            if self.first is not None:
                full[:self.first.numel()] = self.first
            else:
                self.first_n = 0
            array_first_occurrence(self.device, self.offsets, self.values, self.first_n, self.n, full)
            self.first, self.first_n = full, self.n
        return self.first

    def sync(self, rows: list, n: int) -> None:
        torch = _torch()
        if n < self.n:   # a shorter collection: re-encode from row 0 (the dictionary stays)
            self.offsets, self.values = self.offsets[:1], self.values[:0]
            self.n = self.nnz = 0
            self.first, self.first_n = None, 0
        if n == self.n:
            return
        lens, enc = filter_expr.encode_array(rows[self.n:n], self.np_dtype, self._code if self.coded else None, self.dict)
        ends = self.nnz + np.cumsum(lens)
        self.offsets = torch.cat([self.offsets, torch.from_numpy(ends).to(self.device)])
        self.values = torch.cat([self.values, torch.from_numpy(enc).to(self.device)])
        self.n, self.nnz = n, self.nnz + int(enc.size)

    def compact(self, k) -> None:
        """Keep rows k (ascending, an int64 device tensor) of a mirror synced to the whole collection: the
        surviving rows' elements are gathered in row order and the offsets rebuilt from their lengths."""
        torch = _torch()
        starts = self.offsets[:-1].index_select(0, k)
        lens = self.offsets[1:].index_select(0, k) - starts
        ends = torch.cumsum(lens, 0)
        self.nnz = int(ends[-1]) if k.numel() else 0
        # element j of the new values comes from old position start(row) + (j - new start(row))
        src = torch.repeat_interleave(starts - (ends - lens), lens, output_size=self.nnz) + \
            torch.arange(self.nnz, dtype=torch.int64, device=self.device)
        self.values = self.values.index_select(0, src)
        # (a row's content never changes in place: the bytes of the surviving rows' elements stay valid)
        whole = self.first is not None and self.first_n == self.n
        self.first = self.first.index_select(0, src) if whole else None
        self.offsets = torch.cat([self.offsets[:1], ends])
        self.n = int(k.numel())
        self.first_n = self.n if whole else 0


class _DynamicColumn:
    """The device mirror of one dynamic key: a tag per row (uint8: absent | bool | int | double | string) and 8
    bytes of payload (int64 | fp64 bits | 0 / 1 | the string's code into an append-only dictionary in first-seen
    order) -- 9 bytes per row.  Synced lazily from the host list like _ExtraColumn."""

    def __init__(self, device):
        torch = _torch()
        self.device = device
        self.dict: list = []
        self._code: dict = {}
        self.tags = torch.empty(0, dtype=torch.uint8, device=device)
        self.payload = torch.empty(0, dtype=torch.int64, device=device)
        self.n = 0
        # faceted counts: {key: (dictionary length, int32 value ranks on the device)} (CorpusStore._facet_rank).  The
        # dictionaries are append-only, so the same length means the same content and a kept rank stays right.
        self.facet_ranks: dict = {}

    def sync(self, values: list, n: int) -> None:
        torch = _torch()
        if n < self.n:   # a shorter collection: re-encode from row 0 (the dictionary stays)
            self.tags, self.payload = self.tags[:0], self.payload[:0]
            self.n = 0
        if n == self.n:
            return
        tags, payload = filter_expr.encode_dynamic(values[self.n:n], self._code, self.dict)
        self.tags = torch.cat([self.tags, torch.from_numpy(tags).to(self.device)])
        self.payload = torch.cat([self.payload, torch.from_numpy(payload).to(self.device)])
        self.n = n

    def compact(self, k) -> None:
        """Keep rows k (ascending, an int64 device tensor) of a mirror synced to the whole collection."""
        self.tags = self.tags.index_select(0, k)
        self.payload = self.payload.index_select(0, k)
        self.n = int(k.numel())


class _RWLock:
    """Readers/writer lock of a store: any number of readers (search, query, save) at once, or
    one writer (add, delete, upsert, drop).  Re-entrant per thread: a reader may read again, a
    writer may read or write again; a reader asking to write raises.  A waiting writer holds
    off new readers, so a stream of searches cannot starve an upsert."""

    def __init__(self):
        self._cond = threading.Condition(threading.Lock())
        self._readers = 0
        self._writer = None          # thread ident of the writer
        self._writer_depth = 0
        self._writers_waiting = 0
        self._tls = threading.local()

    @contextlib.contextmanager
    def read(self):
        depth = getattr(self._tls, "depth", 0)
        if depth or self._writer == threading.get_ident():
            self._tls.depth = depth + 1
            try:
                yield
            finally:
                self._tls.depth = depth
            return
        with self._cond:
            while self._writer is not None or self._writers_waiting:
                self._cond.wait()
            self._readers += 1
        self._tls.depth = 1
        try:
            yield
        finally:
            self._tls.depth = 0
            with self._cond:
                self._readers -= 1
                if self._readers == 0:
                    self._cond.notify_all()

    @contextlib.contextmanager
    def write(self):
        me = threading.get_ident()
        if self._writer == me:
            self._writer_depth += 1
            try:
                yield
            finally:
                self._writer_depth -= 1
            return
        if getattr(self._tls, "depth", 0):
            raise RuntimeError("a store mutation was called while this thread holds the store's read lock")
        with self._cond:
            self._writers_waiting += 1
            try:
                while self._writer is not None or self._readers:
                    self._cond.wait()
            finally:
                self._writers_waiting -= 1
            self._writer = me
        try:
            yield
        finally:
            with self._cond:
                self._writer = None
                self._cond.notify_all()


class MutationResult:
    """What delete / upsert return, shaped like pymilvus' MutationResult."""

    def __init__(self, primary_keys=(), insert_count: int = 0, delete_count: int = 0, upsert_count: int = 0):
        self.primary_keys = list(primary_keys)
        self.insert_count = insert_count
        self.delete_count = delete_count
        self.upsert_count = upsert_count

    @property
    def succ_count(self) -> int:
        return max(self.insert_count, self.delete_count, self.upsert_count)

    @property
    def err_count(self) -> int:
        return 0

    def __repr__(self):
        return (f"(insert count: {self.insert_count}, delete count: {self.delete_count}, "
                f"upsert count: {self.upsert_count})")


class _Entity:
    """hit.entity.<field> / hit.entity.get(field) as pymilvus exposes it."""

    def __init__(self, fields: dict):
        self.__dict__.update(fields)
        self._fields = fields

    def get(self, name, default=None):
        return self._fields.get(name, default)

    def to_dict(self):
        return dict(self._fields)


class Hit:
    def __init__(self, row: int, pk: Any, score: float, fields: dict):
        self.row = row
        self.id = pk
        self.score = score
        self.distance = score
        self.entity = _Entity(fields)

    def __repr__(self):
        return f"Hit(id={self.id!r}, score={self.score:.6f})"


class SearchIterator:
    """What CorpusStore.search_iterator returns."""

    def __init__(self, store, data, anns_field, param, batch_size, limit, expr, output_fields):
        torch = _torch()
        if anns_field != "embedding":
            raise ValueError(f"search_iterator: unknown vector field {anns_field!r} (only 'embedding')")
        if store._is_text(data):
            raise ValueError("the embedding field is searched with vectors, not with strings")
        metric = str((param or {}).get("metric_type", store.metric_type)).upper()
        if metric != store.metric_type:
            raise ValueError(f"collection was built for {store.metric_type}, search asked for {metric}")
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or \
                not 1 <= batch_size <= MAX_WINDOW:
            raise ValueError(f"batch_size must be an integer in 1..{MAX_WINDOW}, got {batch_size!r}")
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or (limit < 1 and limit != -1):
            raise ValueError(f"limit must be an integer >= 1, or -1 for no limit, got {limit!r}")
        if check_offset(None, param, 1):
            raise ValueError("search_iterator takes no offset")
        self._fields = store._check_output_fields(output_fields)
        self._store = store
        self._batch = int(batch_size)
        self._left = None if limit == -1 else int(limit)
        self._kw = {}
        with store._rw.read():
            q16 = store._prepare_queries(data)
            if q16.shape[0] != 1:
                raise ValueError(f"search_iterator takes one query vector, got {q16.shape[0]}")
            self._q16 = q16
            if not filter_expr.is_empty(expr):
                self._kw["filt"] = store.build_filter(expr)   # once, for every page
            band = store._band_of(param)
            if band is not None:
                self._kw["band"] = band
            self._gen = store._mutations
            dev = q16.device
            # the bound: (fp64 score, row) of the last hit handed out; +inf = before the first
            self._bound = (torch.full((1,), float("inf"), dtype=torch.float64, device=dev),
                           torch.full((1,), -1, dtype=torch.int64, device=dev))
        self._done = False

    def next(self) -> list:
        torch = _torch()
        if self._done:
            return []
        store = self._store
        with store._rw.read():
            if store._mutations != self._gen:
                raise RuntimeError("search_iterator: the collection changed (insert / delete / upsert / drop) since "
                                   "the iterator was made; its position is a row number and no longer valid")
            want = self._batch if self._left is None else min(self._batch, self._left)
            scores, rows = [], []
            while want > 0 and not self._done and store.num_entities > 0:
                k = min(want, _lib.RF_MAX_K)
                s, i, e = store.index.search_after(self._q16, k, self._bound, want_exact=True, **self._kw)
                last = i[:, -1]
                # (the new bound stays on the device; an exhausted query keeps one nothing can follow)
                self._bound = (torch.where(last >= 0, e[:, -1], torch.full_like(e[:, -1], float("-inf"))).contiguous(),
                               torch.where(last >= 0, last, torch.full_like(last, 2 ** 62)).contiguous())
                packed = torch.stack([i[0], s[0].double().view(torch.int64)]).cpu().numpy()   # the page's download
                r = packed[0]
                n = int((r >= 0).sum())
                rows.append(r[:n])
                scores.append(packed[1].view(np.float64)[:n])
                want -= n
                if n < k:
                    self._done = True
            if store.num_entities == 0:
                self._done = True
            if not rows:
                self._done = True
                return []
            rows, scores = np.concatenate(rows), np.concatenate(scores)
            if self._left is not None:
                self._left -= rows.size
                if self._left <= 0:
                    self._done = True
            return store._hits(rows, scores, self._fields)

    def close(self) -> None:
        self._done = True
        self._kw = {}


_ID_IN = re.compile(r"^\s*id\s+in\s+\[(.*)\]\s*$", re.S)


class CorpusStore:
    """Drop-in for the reference's `Collection("fin_chunks")` on this path."""

    # the collection's own fields (schema.py) and their device mirrors.  Class-level defaults: a subclass
    # whose __init__ does not call this one is a store without extra fields.
    schema: tuple = ()
    _xcols = None        # {(field, coded): _ExtraColumn}, built by the first filter / grouping that reads the field
    _acols = None        # {ARRAY field: _ArrayColumn}, built by the first filter that reads the field
    # dynamic fields (pymilvus' enable_dynamic_field / $meta): {key: column of num_entities values, None where
    # the row lacks the key} for every key some row holds, and the mirrors of the keys an expression has read
    enable_dynamic_field = False
    dynamic: dict = {}
    _dyncols = None      # {key: _DynamicColumn}
    _text_fields: dict = {}   # the fields derived from the text column, by name (a subclass that skips __init__ has none)

    def __init__(self, name: str = "fin_chunks", dim: int = 384, capacity: int = 4096,
                 device=None, metric_type: str = "COSINE", index=None, fields=None, enable_dynamic_field: bool = False):
        """fields: FieldSchema objects (rag_fin_amd.schema) of extra scalar fields next to the reference's
        seven: VARCHAR, INT64, DOUBLE or BOOL, at most 32.  They are inserted (add(extra=), the columns after
        primary_value of insert / upsert), filtered on in expr, grouped by, returned as output fields, and
        saved and loaded like `period`.  A field may also be an ARRAY of one of those types
        (FieldSchema("tags", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=16)): a row holds a
        list; expr reads it through ARRAY_CONTAINS / ARRAY_CONTAINS_ALL / ARRAY_CONTAINS_ANY / ARRAY_LENGTH and
        an index tags[i] (filter_expr's docstring), evaluated on the GPU over a CSR mirror; it is
        returned as an output field, saved and loaded, and cannot be grouped by or decayed over.
        enable_dynamic_field: rows may carry keys that no field declares (pymilvus' $meta; schema.py): a key of
        add(extra=) that is no declared field, or the dict of a trailing column of insert / upsert.  At most 64
        distinct keys; a value is a bool, an int64, a float, a str or None.  Such a key is filtered on in expr
        (bare, or as $meta["key"]; filter_expr's docstring has the semantics) and returned as an output field,
        as is "$meta" (the dict of the keys a row holds)."""
        self.schema = schema_.check_fields(fields)
        self.enable_dynamic_field = bool(enable_dynamic_field)
        self.dynamic = {}
        self._dyncols = None
        self.name = name
        self.dim = dim
        self.metric_type = metric_type.upper()
        if self.metric_type not in ("COSINE", "IP"):
            raise ValueError("metric_type must be COSINE or IP")
        # `index`: an already-built GpuIndex (tests of the sharded store pass a CPU double)
        self.index = index if index is not None else GpuIndex(dim, capacity, device)
        self.columns: dict[str, list] = {f: [] for f in SCALAR_FIELDS + tuple(f.name for f in self.schema)}
        self._pk_row: dict[Any, int] = {}
        self._xcols = None
        self._acols = None
        self._dcols = None                  # _DeviceColumns, built by the first filtered call
        self._filter_lock = threading.Lock()
        # search / query / save read; add / delete / upsert / drop write.  A search hands out row
        # numbers and then reads the host columns at those rows (search_large over several pages):
        # a delete in between would pin another row's entity on a hit.
        self._rw = _RWLock()
        self.index_type = "FLAT"            # create_index: "FLAT" (IVF_FLAT is served as FLAT) or "SQ8"
        self._index_params = None           # what create_index was given (None: no create_index call)
        # the fields derived from the text column (text_fields.py: the lexical index, the learned sparse field, the
        # late-interaction field), each with its declaration and what it built, and the one lock all three build under
        self._sparse_lock = threading.Lock()
        self._text_fields = {f.name: f for f in (LexicalField(self), LearnedSparseField(self), TokenVectorField(self))}
        # bumped by every change of the rows (insert, delete, upsert, drop): a search_iterator's
        # bound is a row number, so it refuses to go on once this has moved
        self._mutations = 0
        self.analyzer = None                # list[str] -> list[list[str]]; None: lexical.analyze

    # -- pymilvus-shaped lifecycle ---------------------------------------------
    def flush(self) -> None:
        _torch().cuda.synchronize(self.index.device)

    def load(self) -> None:
        return None

    def release(self) -> None:
        return None

    def drop(self) -> None:
        """utility.drop_collection + recreate ("chunking_storing (1).py":25-28)."""
        with self._rw.write():
            self._mutations += 1
            self.index.reset()
            for col in self.columns.values():
                col.clear()
            self._pk_row.clear()
            self.dynamic = {}
            self._dcols = None
            self._xcols = None
            self._acols = None
            self._dyncols = None
            for field in self._text_fields.values():
                field.reset()

    LEXICAL_LOG_MAX = 64   # pending mutations the lexical field replays; beyond, it builds whole

    # (the two the store itself turns to: for keyword filters and columns.json; for token_vectors and rerank_tokens)
    _lexical = property(lambda self: self._text_fields[LexicalField.name])
    _late = property(lambda self: self._text_fields[TokenVectorField.name])
    lexical_fallback_reason = property(lambda self: self._lexical.fallback_reason)

    @property
    def num_entities(self) -> int:
        return len(self.columns["id"])

    def _grow(self, need: int) -> None:
        old = self.index
        cap = max(need, old.capacity * 2)
        # (a CPU double of GpuIndex takes no shadow argument)
        new = type(old)(self.dim, cap, old.device, **({"shadow": old.shadow} if hasattr(old, "shadow") else {}))
        n = old.size
        step = 1 << 18
        for s in range(0, n, step):
            new.add(old.get_rows(np.arange(s, min(n, s + step), dtype=np.int64)))
        if self._has_sq8:
            new.enable_sq8()   # re-attach: quantizes the copied rows
        self.index = new

    @property
    def _has_sq8(self) -> bool:
        """The index carries an int8 shadow (a CPU double of GpuIndex has no such attribute)."""
        return getattr(self.index, "sq8", False)

    # -- index type: Collection.create_index / drop_index / has_index --------------------------
    INDEX_TYPES = ("FLAT", "IVF_FLAT", "SQ8")

    def create_index(self, field_name: str, index_params: dict | None = None, **kwargs) -> None:
        """pymilvus-shaped create_index ("chunking_storing (1).py":29).  index_type "FLAT" (the
        default), "IVF_FLAT" (served as FLAT: exact, `params` such as nlist are ignored) or "SQ8"
        (an int8 shadow of the vectors: fewer bytes per search, same exact answers; dim % 32 == 0).
        Any other type, a metric_type other than the collection's or a field other than
        "embedding" / "sparse" raises ValueError.
        field_name "sparse" with {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25",
        "params": {"bm25_k1": 1.2, "bm25_b": 0.75}} declares the lexical index over the `text` column
        and leaves the vector index as it is.  The posting lists are built from the texts by the first
        BM25 search: through the native analyzer and the device build (RAGFIN_LEXICAL_BUILD=
        host|device|auto pins the route), on the host with a custom `analyzer`.  After an add / insert / upsert / delete the first BM25 search or
        keyword filter brings them up to date on the GPU: the mutations since the last build are replayed
        through SparseIndex.appended / .compacted, which analyse only the appended texts and leave the
        arrays bit for bit as a build of the surviving rows would.  They are built whole
        instead after drop(), create_index / drop_index of "sparse", a changed `analyzer`, more than
        LEXICAL_LOG_MAX pending mutations, when no row held a term, or when a replay raised.
        field_name "sparse_embedding" with {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "IP"} and
        encoder=<a SparseEncoder> declares the learned sparse field (Milvus: a SPARSE_FLOAT_VECTOR field
        filled by a function): the store derives each row's term vector from its `text` with the attached
        encoder (encode_document), lazily at the first search of the field; after an add / insert / upsert
        only the new rows are encoded, a delete drops its rows, and the per-row vectors (host CSR) are
        transposed again on the host -- a stable sort by term, rows ascending within a term -- into the
        posting arrays a SparseIndex serves.  They are not saved: a loaded store encodes
        again, as the lexical index is rebuilt.
        field_name "token_embeddings" with {"index_type": "EMB_LIST_FLAT", "metric_type": "MAX_SIM_IP"} and
        encoder=<a ColBERT> declares the late-interaction field (Milvus: an embedding list filled by a
        function): one unit vector per kept token of each row's `text` (encoder.encode(texts, is_query=False)),
        encoded lazily at the first search of the field; after an add / insert / upsert only the new rows are
        encoded and appended to the device CSR, a delete drops its rows from it, so the field always equals
        that of a fresh store.  It is not saved: a loaded store encodes again."""
        params = dict(index_params or {})
        field = self._text_field(field_name)
        if field is not None:
            checked = field.check_params(params, kwargs.get("encoder"))
            with self._rw.write():
                field.declare(checked)
            return
        itype, metric = self._check_index_params(field_name, params)
        with self._rw.write():
            if itype == "SQ8":
                self.index.enable_sq8()
            elif self._has_sq8:
                self.index.disable_sq8()
            self.index_type = "SQ8" if itype == "SQ8" else "FLAT"
            self._index_params = {"index_type": itype, "metric_type": metric, "params": dict(params.get("params") or {})}

    def _check_index_params(self, field_name, params):
        if field_name != "embedding":
            raise ValueError(f"create_index: unknown vector field {field_name!r} (only 'embedding')")
        itype = str(params.get("index_type", "FLAT")).upper()
        if itype not in self.INDEX_TYPES:
            raise ValueError(f"create_index: index_type {itype!r} not supported (one of {', '.join(self.INDEX_TYPES)})")
        metric = str(params.get("metric_type", self.metric_type)).upper()
        if metric != self.metric_type:
            raise ValueError(f"create_index: collection was built for {self.metric_type}, index asked for {metric}")
        p = params.get("params")
        if p is not None and not isinstance(p, dict):
            raise ValueError("create_index: params must be a dict")
        return itype, metric

    def _text_field(self, *names):
        """The field derived from the text column (text_fields.py) that one of `names` names, or None."""
        return next((self._text_fields[n] for n in names if isinstance(n, str) and n in self._text_fields), None)

    def drop_index(self, **kwargs) -> None:
        """Back to FLAT (the shadow of SQ8 is freed).  field_name="sparse" (or index_name="sparse"):
        drop the lexical index instead and leave the vector index alone."""
        field = self._text_field(kwargs.get("field_name"), kwargs.get("index_name"))
        with self._rw.write():
            if field is not None:
                field.declare(None)
                return
            if self._has_sq8:
                self.index.disable_sq8()
            self.index_type = "FLAT"
            self._index_params = None

    def has_index(self, **kwargs) -> bool:
        """field_name="sparse" (or index_name="sparse") asks about the lexical index."""
        field = self._text_field(kwargs.get("field_name"), kwargs.get("index_name"))
        return self._index_params is not None if field is None else field.declared

    def _use_sq8(self, B: int, limit: int, band=None) -> bool:
        # the routing rule: unfiltered, no range parameters, limit <= RF_MAX_K,
        # B <= one 64-query sweep
        return self.index_type == "SQ8" and band is None and limit <= _lib.RF_MAX_K and B <= _lib.RF_QCHUNK

    # -- ingest ------------------------------------------------------------------
    def add(self, ids: Sequence, texts: Sequence[str], embeddings, periods: Sequence[str],
            chunk_types: Sequence[str], statement_types: Sequence[str],
            primary_values: Sequence[float], extra: dict | None = None) -> int:
        """extra: {field name: column} for the collection's own fields (schema.py); a field that is not given
        takes its default, and has to have one.  With enable_dynamic_field a key that is no declared field is a
        dynamic key: its column holds a bool, an int, a float, a str or None (the row lacks the key) per row."""
        cols = (texts, periods, chunk_types, statement_types, primary_values)
        with self._rw.write():
            xcols, dyn = self._check_extra(extra, len(ids), "insert")   # before anything changes
            self._store_vectors(self._check_batch(ids, cols, embeddings, len(ids), "insert"))
            self._append_rows(ids, cols, xcols, dyn)
        return len(ids)

    def _check_extra(self, extra, n: int, what: str):
        """`extra` of an insert / upsert -> (the declared fields' columns in schema order, {dynamic key:
        column}), everything checked and nothing changed."""
        if not self.enable_dynamic_field:
            return schema_.check_columns(self.schema, extra, n, what), {}
        names = {f.name for f in self.schema}
        extra = dict(extra or {})
        own = {k: v for k, v in extra.items() if k in names}
        dyn = schema_.check_dynamic({k: v for k, v in extra.items() if k not in names}, n, self.dynamic, what)
        return schema_.check_columns(self.schema, own, n, what), dyn

    def _check_batch(self, ids, cols, embeddings, n_vec_rows: int, what: str):
        """Everything an insert / upsert (`what`) refuses, checked before anything changes; returns
        the fp16 rows to store.  cols: the five scalar columns after id.  embeddings: n_vec_rows rows
        (the sharded store: this rank's slice); fp16 is embedder output and stays, else to_fp16."""
        torch = _torch()
        n = len(ids)
        if any(len(c) != n for c in cols):
            raise ValueError(f"{what} columns differ in length")
        if what == "insert":   # (an upsert replaces the rows of its existing keys)
            for pk in ids:
                if pk in self._pk_row:
                    raise ValueError(f"duplicate primary key {pk!r}")
        if len(set(ids)) != n:
            raise ValueError(f"duplicate primary keys in {what}")
        emb = self._embedding_rows(embeddings, n_vec_rows)
        if torch.is_tensor(emb) and emb.dtype == torch.float16:
            return emb
        if n_vec_rows == 0:
            return torch.empty((0, self.dim), dtype=torch.float16, device=self.index.device)
        return self.index.to_fp16(emb, normalize=self.metric_type == "COSINE")

    def _embedding_rows(self, embeddings, n_rows: int):
        """embeddings as they came when a tensor, else as an fp32 array; ValueError unless [n_rows, dim]."""
        emb = embeddings if _torch().is_tensor(embeddings) else np.asarray(embeddings, dtype=np.float32)
        if tuple(emb.shape) != (n_rows, self.dim):
            raise ValueError(f"embeddings must be [{n_rows}, {self.dim}], got {tuple(emb.shape)}")
        return emb

    def _store_vectors(self, vec) -> None:
        """Append the checked fp16 rows to the index, growing it first when they do not fit."""
        need = self.index.size + vec.shape[0]
        if need > self.index.capacity:
            self._grow(need)
        self.index.add(vec)

    def _append_rows(self, ids, cols, xcols=(), dyn=None) -> None:
        """The host side of an append: the pk map, the six scalar columns, the checked extra columns
        (schema.check_columns: in schema order) and the checked dynamic columns (schema.check_dynamic)."""
        texts, periods, chunk_types, statement_types, primary_values = cols
        for field in self._text_fields.values():   # each is brought up to date by its next search
            field.rows_appended(texts)
        self._mutations += 1
        base = self.num_entities
        for j, pk in enumerate(ids):
            self._pk_row[pk] = base + j
        self.columns["id"].extend(ids)
        self.columns["text"].extend(texts)
        self.columns["period"].extend(periods)
        self.columns["chunk_type"].extend(chunk_types)
        self.columns["statement_type"].extend(statement_types)
        self.columns["primary_value"].extend(float(v) for v in primary_values)
        for f, col in zip(self.schema, xcols):
            self.columns[f.name].extend(col)
        if self.enable_dynamic_field:
            dyn = dyn or {}
            for key in dyn:
                if key not in self.dynamic:
                    self.dynamic[key] = [None] * base   # the rows so far lack the key
            for key, col in self.dynamic.items():
                col.extend(dyn.get(key) or [None] * len(ids))

    def _split_extra(self, data, what: str):
        """Column-major `data` of 7 + len(schema) columns -> (the reference's seven, {field: column}): the
        collection's own fields follow primary_value in schema order.  With enable_dynamic_field one more column
        may follow them: the rows' $meta, a dict (or None) per row, whose keys join the {field: column}."""
        S = len(self.schema)
        if self.enable_dynamic_field and len(data) == 8 + S:
            extra = schema_.dynamic_columns_of_rows(data[7 + S], len(data[0]), what)
            declared = [f.name for f in self.schema if f.name in extra]
            if declared:
                raise ValueError(f"{what}: $meta holds the declared field {declared[0]!r}; it has a column of its own")
            extra.update({f.name: col for f, col in zip(self.schema, data[7:7 + S])})
            return list(data[:7]), extra
        if not self.schema:
            return data, None
        if len(data) != 7 + S:
            raise ValueError(f"{what} expects {7 + S} columns: id, text, embedding, period, chunk_type, "
                             f"statement_type, primary_value, {', '.join(f.name for f in self.schema)}")
        return list(data[:7]), {f.name: col for f, col in zip(self.schema, data[7:])}

    @staticmethod
    def _split_columns(data, what: str):
        """Column-major `data` in the reference's order -> (ids, the five scalar columns, embeddings)."""
        if len(data) != 7:
            raise ValueError(f"{what} expects 7 columns: id, text, embedding, period, chunk_type, "
                             "statement_type, primary_value")
        ids, texts, emb, periods, ctypes_, stypes, pvals = data
        return ids, (texts, periods, ctypes_, stypes, pvals), emb

    def insert(self, data: Sequence[Sequence]) -> int:
        """Column-major insert in the reference's order
        [id, text, embedding, period, chunk_type, statement_type, primary_value], then the collection's own
        fields in schema order."""
        data, extra = self._split_extra(data, "insert")
        ids, cols, emb = self._split_columns(data, "insert")
        return self.add(ids, cols[0], emb, *cols[1:], **({} if extra is None else {"extra": extra}))

    # -- mutation: Collection.delete(expr) / Collection.upsert(data) -----------------------
    # Deletes compact eagerly: the index, the host columns, the pk map and the device filter
    # mirror are left exactly as a fresh insert of the surviving rows (in their old order) would
    # leave them, so no search path knows about deletes.
    def delete(self, expr: str) -> MutationResult:
        """Remove every row `expr` matches (any expression filtered search accepts, `id in [...]`
        included; the predicate runs on the GPU).  An empty expression raises ValueError, as
        Milvus refuses to delete everything: use drop().  Matching nothing changes nothing."""
        if filter_expr.is_empty(expr):
            raise ValueError("delete needs a non-empty expression (use drop() to remove everything)")
        with self._rw.write():
            return self._delete_mask(self._match_mask(expr))

    def upsert(self, data: Sequence[Sequence]) -> MutationResult:
        """Column-major rows as for insert.  Rows whose primary key exists are deleted, then every
        row is appended in the given order: a replaced row moves to the END of the collection (so
        on an exact score tie -- ranked by score desc, then row asc -- it ranks after older rows).
        Duplicate keys inside one batch raise ValueError, as insert does."""
        data, extra = self._split_extra(data, "upsert")
        ids, cols, emb = self._split_columns(data, "upsert")
        ids = list(ids)
        with self._rw.write():
            xcols, dyn = self._check_extra(extra, len(ids), "upsert")
            vec = self._check_batch(ids, cols, emb, len(ids), "upsert")   # before any row goes
            self._delete_mask(self._pk_mask(ids))
            self._store_vectors(vec)
            self._append_rows(ids, cols, xcols, dyn)
        return MutationResult(ids, insert_count=len(ids), upsert_count=len(ids))

    def _match_mask(self, expr: str) -> np.ndarray:
        """bool [num_entities]: the rows `expr` matches, evaluated on the device."""
        n = self.num_entities
        if n == 0:
            with self._filter_lock:   # still reject a bad expression
                filter_expr.compile_expr(filter_expr.parse(expr, self.analyzer, self.schema, self.enable_dynamic_field),
                                         {f: [] for f in filter_expr.VARCHAR_FIELDS}, {},
                                         {} if self._lexical.declared else None, self.schema, {}, {})
            return np.zeros(0, dtype=bool)
        return filter_mask_bits(self.build_filter(expr), n)

    def _pk_mask(self, keys) -> np.ndarray:
        mask = np.zeros(self.num_entities, dtype=bool)
        rows = [self._pk_row[k] for k in keys if k in self._pk_row]
        mask[rows] = True
        return mask

    def _delete_mask(self, mask: np.ndarray) -> MutationResult:
        """Drop the rows set in `mask` (bool [num_entities]) everywhere.  Caller holds the write lock."""
        gone = np.flatnonzero(mask)
        if gone.size == 0:
            return MutationResult(delete_count=0)
        ids = self.columns["id"]
        pks = [ids[i] for i in gone.tolist()]
        keep_mask = ~mask
        keep = np.flatnonzero(keep_mask)
        n_old = self.num_entities
        for field in self._text_fields.values():
            field.rows_deleted(keep_mask)
        self._mutations += 1
        self._compact_index(keep_mask, keep)
        sel = keep_mask.tolist()
        for f in list(self.columns):
            self.columns[f] = list(itertools.compress(self.columns[f], sel))
        self._pk_row = dict(zip(self.columns["id"], range(keep.size)))
        # (a key that no surviving row holds is gone, as in a fresh store of the surviving rows)
        self.dynamic = {key: col for key, col in ((key, list(itertools.compress(col, sel)))
                                                  for key, col in self.dynamic.items())
                        if any(v is not None for v in col)}
        with self._filter_lock:
            if self._dcols is not None:
                if self._dcols.n == n_old:
                    self._dcols.compact(keep)
                else:   # not synced to the old rows: the next filtered call re-encodes from row 0
                    self._dcols = None
            if self._xcols:
                synced = {key: c for key, c in self._xcols.items() if c.n == n_old}   # the others: as above
                if synced:
                    k = _torch().from_numpy(np.ascontiguousarray(keep, dtype=np.int64)).to(self.index.device)
                    for c in synced.values():
                        c.compact(k)
                self._xcols = synced
            if self._acols:
                synced = {key: c for key, c in self._acols.items() if c.n == n_old}   # the others: as above
                if synced:
                    k = _torch().from_numpy(np.ascontiguousarray(keep, dtype=np.int64)).to(self.index.device)
                    for c in synced.values():
                        c.compact(k)
                self._acols = synced
            if self._dyncols:
                synced = {key: c for key, c in self._dyncols.items() if c.n == n_old and key in self.dynamic}
                if synced:
                    k = _torch().from_numpy(np.ascontiguousarray(keep, dtype=np.int64)).to(self.index.device)
                    for c in synced.values():
                        c.compact(k)
                self._dyncols = synced
        return MutationResult(pks, delete_count=len(pks))

    def _compact_index(self, keep_mask: np.ndarray, keep: np.ndarray) -> None:
        self.index.compact(keep)

    # -- search --------------------------------------------------------------------
    def _prepare_queries(self, data):
        torch = _torch()
        if torch.is_tensor(data) and data.dtype == torch.float16:
            q = data.to(self.index.device)
            return q if q.dim() == 2 else q.unsqueeze(0)
        q = np.asarray(data, dtype=np.float32) if not torch.is_tensor(data) else data.float()
        if q.ndim == 1:
            q = q[None, :]
        return self.index.to_fp16(q, normalize=self.metric_type == "COSINE")

    def search_rows(self, data, limit: int, filt=None, band=None, mmr=None):
        """(scores f32 [B,k'], rows i64 [B,k']) as host numpy, k' = min(limit, N).  filt: a
        filter buffer (build_filter): the top-k of the passing rows, padded with -1 rows.
        band: (radius, range_filter) -- range search: the top-k of the rows with
        radius < fp64 score <= range_filter, padded with -1 rows.
        mmr: (fetch_k, lambda) -- diversified search: `limit` of the best fetch_k such hits by
        maximal marginal relevance, in MMR order (check_mmr)."""
        if limit < 1:
            raise ValueError("limit must be >= 1")
        if band is not None:
            band = check_band(*band)
        if mmr is not None:
            mmr = check_mmr(mmr[1], mmr[0], limit)
        with self._rw.read():
            return self._search_rows(data, limit, filt, band, mmr=mmr)

    GROUP_BY_FIELDS = filter_expr.VARCHAR_FIELDS   # period, chunk_type, statement_type ("id": the plain search)

    def _extra_column(self, field: FieldSchema, coded: bool = False) -> _ExtraColumn:
        """The synced device mirror of one of the collection's own fields.  Caller holds `_filter_lock`."""
        if self._xcols is None:
            self._xcols = {}
        key = (field.name, coded or field.dtype in (DataType.VARCHAR, DataType.BOOL))   # (those are coded anyway)
        col = self._xcols.get(key)
        if col is None:
            col = self._xcols[key] = _ExtraColumn(self.index.device, field.dtype, coded)
        col.sync(self.columns[field.name], self.num_entities)
        return col

    def _array_column(self, field: FieldSchema) -> _ArrayColumn:
        """The synced device mirror of one of the collection's ARRAY fields.  Caller holds `_filter_lock`."""
        if self._acols is None:
            self._acols = {}
        col = self._acols.get(field.name)
        if col is None:
            col = self._acols[field.name] = _ArrayColumn(self.index.device, field.element_type)
        col.sync(self.columns[field.name], self.num_entities)
        return col

    def _dynamic_column(self, key: str) -> _DynamicColumn:
        """The synced device mirror of a dynamic key some row holds.  Caller holds `_filter_lock`."""
        if self._dyncols is None:
            self._dyncols = {}
        col = self._dyncols.get(key)
        if col is None:
            col = self._dyncols[key] = _DynamicColumn(self.index.device)
        col.sync(self.dynamic[key], self.num_entities)
        return col

    def _field(self, name: str):
        """The FieldSchema of one of the collection's own fields, or None."""
        return next((f for f in self.schema if f.name == name), None)

    def _group_codes(self, field: str):
        """(codes int32 [n] on the device, n_codes) of a group-by field, from the device mirror.  An INT64
        field of the collection's own is dictionary-coded on first use."""
        own = self._field(field)
        if own is not None:
            with self._filter_lock:
                col = self._extra_column(own, coded=True)
                return col.data.contiguous(), len(col.dict)
        with self._filter_lock:
            if self._dcols is None:
                self._dcols = _DeviceColumns(self.index.device)
            self._dcols.sync(self.columns, self.num_entities)
            return self._dcols.codes[field].contiguous(), len(self._dcols.dicts[field])

    def _search_rows(self, data, limit: int, filt=None, band=None, group=None, mmr=None):
        q16 = self._prepare_queries(data)
        kw = {} if filt is None else {"filt": filt}   # the index is given a keyword only when it is set
        if group is not None:
            # (field, group_size): the padded [B, limit * group_size] block; never SQ8, never paged
            field, gsize = group
            codes, n_codes = self._group_codes(field)
            return self.index.search_host(q16, limit * gsize, group=(codes, n_codes, limit, gsize), **kw)
        if band is not None:
            kw["band"] = band
        if mmr is not None:
            kw["mmr"] = mmr   # (limit <= fetch_k <= RF_MAX_K: never paged)
        if limit > _lib.RF_MAX_K:
            scores, rows = self.index.search_large(q16, limit, **kw)   # paged, exhaustive beyond 64
            kk = min(limit, self.num_entities)
            return scores[:, :kk].cpu().numpy(), rows[:, :kk].cpu().numpy()
        if filt is None and self._use_sq8(int(q16.shape[0]), limit, band):
            kw["sq8"] = True
        scores, rows = self.index.search_host(q16, limit, **kw)   # one synchronisation for the whole download
        kk = min(limit, self.num_entities)
        return scores[:, :kk], rows[:, :kk]

    def search(self, data, anns_field: str = "embedding", param: dict | None = None,
               limit: int = 3, expr=None, output_fields: Iterable[str] | None = None,
               group_by_field: str | None = None, group_size: int = 1, strict_group_size: bool = False,
               mmr_lambda=None, mmr_fetch_k=None, offset: int | None = None, ranker=None):
        """pymilvus-shaped search: one list of hits per query vector, best first.
        ranker (a BoostRanker, or a list / tuple of 1..3 of them, which multiply): boosted search --
        the rows a boost's filter selects have their score multiplied by its weight (below 1:
        demoted), and the hits are the exact top `limit` of the whole collection (of the rows passing
        expr) by (boosted score desc, plain score desc, row asc); hit.score is float32(boosted).
        The boost filters split the rows into at most 8 classes of equal weight; every (query, class)
        pair is one query of the per-query-filter sweep and rf_merge_boosted merges their answers
        (DESIGN §4.4m): ceil(B * classes / 64) sweeps of the corpus.  The plain dense search only:
        one expr string, limit <= 64, no offset, radius / range_filter, group_by_field, mmr_lambda /
        mmr_fetch_k or anns_field="sparse" (ValueError); an SQ8 collection answers from its fp16 rows.
        ranker may instead be ONE DecayRanker(field, function, origin, scale, offset, decay): decayed search --
        every row's score is multiplied by a weight in [0, 1] from the distance of `field` (primary_value or an
        INT64 / DOUBLE field of the collection) to `origin`, and the hits are the exact top `limit` (of the rows
        passing expr) by (decayed desc, plain score desc, row asc); hit.score is float32(decayed).  The weights are
        computed from the live column on every call and sit inside the sweep: one sweep per 64 queries (DESIGN
        §4.4q).  The same exclusions as a boost; a list of rankers that holds a DecayRanker raises ValueError.
        offset (or param["offset"], as pymilvus accepts it; the keyword wins when both are given): the
        hits of ranks offset + 1 ... offset + limit, i.e. search(limit=offset + limit)[offset:].  An
        int >= 0 with offset + limit <= 16384 (Milvus' window), else ValueError.  With expr, range
        parameters and on an SQ8 collection (whose hits past rank 64 come from the fp16 rows, as for
        any limit above 64): the first 64 ranks through the fused path, every further 64 through one
        search-after sweep of the corpus (GpuIndex.search_large).  Not with group_by_field,
        mmr_lambda, anns_field="sparse" or inside hybrid_search (ValueError).  To walk a long result
        list page by page without searching from the top each time, see search_iterator.
        group_by_field ("period", "chunk_type", "statement_type"; "id" is the plain search): the best
        `limit` GROUPS of rows sharing that field's value, each by its best min(group_size, rows of
        the group) rows.  One flat hit list per query: group after group in group rank order (a
        group ranks by its best row), the rows of a group best first; every hit carries the group
        value, hit.entity.get(group_by_field).  With expr, groups are formed among the passing
        rows.  limit * group_size <= 64; not together with radius / range_filter;
        strict_group_size is accepted and ignored (the search is exact: every group already
        returns as many rows as it has, up to group_size).
        param["params"] may hold the range-search bounds `radius` and, optionally, `range_filter`:
        the best `limit` hits with radius < score <= range_filter (a query may return []); the
        comparison is made in fp64 on the fp64 ranking score, so a hit's fp32 `score` may equal
        float32(radius).  range_filter without radius, a bound that is no real number, NaN or
        radius >= range_filter raises ValueError.  Other keys of params (nprobe, ...) are ignored.
        mmr_lambda (a real number in [0, 1]): diversified search -- the `limit` hits are picked from
        the best mmr_fetch_k (default min(64, max(20, 4 * limit)), at most 64) by maximal marginal
        relevance on the GPU: each pick maximises lambda * score - (1 - lambda) * (largest similarity
        to a hit already picked).  The hits come in MMR order, the first is always the best hit and
        hit.score stays the relevance score; 1 gives the plain ranking.  With expr, range search and
        an SQ8 index; not with group_by_field (ValueError, as are mmr_fetch_k without mmr_lambda,
        limit > mmr_fetch_k and mmr_fetch_k > 64).
        anns_field "sparse": BM25 search of the `text` column (create_index("sparse", ...) first).
        data is a list of query STRINGS, param {"metric_type": "BM25"}, limit <= 64; a hit is a row
        that holds at least one query term (and passes expr), hit.score its BM25 score, so a list
        may be shorter than limit, or empty.  Exact and bit-reproducible.  No range,
        grouping or MMR arguments (ValueError); vectors for "sparse" or strings for "embedding"
        raise ValueError too.  To combine the two fields see hybrid_search.
        expr may also be a list or tuple with ONE ENTRY PER QUERY VECTOR, each a filter string or
        None / "" (no filter for that query): per-query filters, served by one sweep of the corpus
        per 64 queries over the union of their filters (GpuIndex.search(filt=MultiFilter)), each
        query over its own passing rows -- the hits of query b are those of
        search(data[b], expr=expr[b]).  Equal strings are built once; a list whose entries are all
        equal is the plain call with that one expression; above 64 queries the queries are ordered
        by filter internally and the results come back in the caller's order.  The list form is the
        plain search only: limit <= 64, and no offset, radius / range_filter, group_by_field,
        mmr_lambda / mmr_fetch_k or anns_field="sparse" (ValueError; neither search_iterator,
        hybrid_search arms, query nor delete take a list).  These can follow later."""
        if isinstance(ranker, DecayRanker):
            return self._search_decayed(data, anns_field, param, limit, expr, output_fields, group_by_field,
                                        mmr_lambda, mmr_fetch_k, offset, ranker)
        if isinstance(ranker, (list, tuple)) and any(isinstance(r, DecayRanker) for r in ranker):
            raise ValueError("a DecayRanker is passed on its own (ranker=DecayRanker(...)): lists of rankers and a decay "
                             "mixed with boosts are not served yet")
        if ranker is not None:
            return self._search_boosted(data, anns_field, param, limit, expr, output_fields, group_by_field,
                                        mmr_lambda, mmr_fetch_k, offset, ranker)
        if isinstance(expr, (list, tuple)):
            return self._search_expr_list(data, anns_field, param, limit, expr, output_fields, group_by_field,
                                          mmr_lambda, mmr_fetch_k, offset)
        offset = check_offset(offset, param, limit)
        field = self._text_field(anns_field)
        other_form = group_by_field is not None or mmr_lambda is not None or mmr_fetch_k is not None
        if field is not None:
            field.refuse_forms(offset, other_form)
        if offset and (anns_field == "sparse" or other_form):
            raise ValueError("offset has no BM25 (anns_field='sparse'), grouping (group_by_field) or MMR (mmr_lambda) form")
        if field is not None:
            q = field.check_search(data, param, limit)
            fields = self._check_output_fields(output_fields)
            with self._rw.read():
                return self._search_text_field(field, q, limit, expr, fields)
        mmr = check_mmr(mmr_lambda, mmr_fetch_k, limit)
        if mmr is not None and group_by_field is not None:
            raise ValueError("diversified search (mmr_lambda) cannot be combined with group_by_field")
        with self._rw.read():   # the rows handed back are marshalled below: no delete in between
            if group_by_field is None:
                return self._search(data, anns_field, param, limit, expr, output_fields, mmr=mmr, offset=offset)
            return self._search(data, anns_field, param, limit, expr, output_fields,
                                self._check_group_by(group_by_field, group_size, limit, param))

    # -- per-query filters: search(expr=[...]) ----------------------------------------
    @staticmethod
    def _query_count(data) -> int:
        """How many query vectors `data` holds, without touching the device."""
        shape = tuple(data.shape) if hasattr(data, "shape") else np.asarray(data, dtype=np.float32).shape
        return 1 if len(shape) == 1 else int(shape[0])

    def _check_expr_list(self, data, anns_field, param, limit, exprs, group_by_field, mmr_lambda, mmr_fetch_k,
                         offset) -> list:
        """Everything a list expr refuses, before anything runs -> one key per query: the filter
        string, or None for "no filter"."""
        field = self._text_field(anns_field)
        if field is not None:
            raise ValueError(f"per-query filters (a list expr) have no {field.form} form (anns_field='{field.name}')")
        if self._is_text(data):
            raise ValueError("the embedding field is searched with vectors, not with strings (BM25: anns_field='sparse')")
        if group_by_field is not None:
            raise ValueError("per-query filters (a list expr) cannot be combined with group_by_field")
        if mmr_lambda is not None or mmr_fetch_k is not None:
            raise ValueError("per-query filters (a list expr) cannot be combined with mmr_lambda / mmr_fetch_k")
        if check_offset(offset, param, limit):
            raise ValueError("per-query filters (a list expr) take no offset")
        if self._band_of(param) is not None:
            raise ValueError("per-query filters (a list expr) have no range form (radius / range_filter)")
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 1 <= limit <= _lib.RF_MAX_K:
            raise ValueError(f"per-query filters (a list expr): limit must be an integer in 1..{_lib.RF_MAX_K}, "
                             f"got {limit!r} (the list form is not paged)")
        for j, e in enumerate(exprs):
            if e is not None and not isinstance(e, str):
                raise ValueError(f"expr list: entry {j} is {type(e).__name__}; every entry is a filter string or None")
        B = self._query_count(data)
        if len(exprs) != B:
            raise ValueError(f"expr list: {len(exprs)} entries for {B} query vectors (one entry per query)")
        return [None if filter_expr.is_empty(e) else e for e in exprs]

    def _all_pass_filter(self):
        """The filter buffer that passes every row: what a query without a filter uses beside
        queries that have one."""
        torch = _torch()
        n = self.num_entities
        dev = self.index.device
        with torch.cuda.device(dev):
            words = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev)
            buf = torch.empty(self.index.lib.rf_filter_bytes(n), dtype=torch.uint8, device=dev)
            _lib.check(self.index.lib.rf_filter_from_mask(_ptr(words), n, _ptr(buf), _lib.current_stream_ptr()))
        return buf

    def _search_expr_list(self, data, anns_field, param, limit, exprs, output_fields, group_by_field, mmr_lambda,
                          mmr_fetch_k, offset):
        keys = self._check_expr_list(data, anns_field, param, limit, exprs, group_by_field, mmr_lambda, mmr_fetch_k,
                                     offset)
        distinct = list(dict.fromkeys(keys))
        if len(distinct) <= 1:   # one expression for the whole batch: the existing call, the same bits
            return self.search(data, anns_field, param, limit, expr=distinct[0] if distinct else None,
                               output_fields=output_fields)
        if anns_field != "embedding":
            raise ValueError(f"unknown vector field {anns_field!r}")
        metric = (param or {}).get("metric_type", self.metric_type).upper()
        if metric != self.metric_type:
            raise ValueError(f"collection was built for {self.metric_type}, search asked for {metric}")
        fields = self._check_output_fields(output_fields)
        number = {key: g for g, key in enumerate(distinct)}
        qfilter = [number[key] for key in keys]
        with self._rw.read():
            B = len(keys)
            if self.num_entities == 0:
                return [[] for _ in range(B)]
            # every expression is parsed and built once, before any sweep runs
            filters = [self._all_pass_filter() if key is None else self.build_filter(key) for key in distinct]
            q16 = self._prepare_queries(data)
            kk = min(int(limit), self.num_entities)
            scores = np.full((B, kk), -np.inf, dtype=np.float32)
            rows = np.full((B, kk), -1, dtype=np.int64)
            for idx, used, local in plan_filter_chunks(qfilter):
                qc = q16[idx.tolist()]   # the chunk's queries, in the order of `local`
                if len(used) == 1:   # a chunk of one filter: the single-filter sweep (or the unfiltered one)
                    s, r = self._search_rows(qc, int(limit), None if distinct[used[0]] is None else filters[used[0]])
                else:
                    mf = MultiFilter([filters[g] for g in used], local, self.num_entities, self.index.device)
                    s, r = self.index.search_host(qc, int(limit), filt=mf)
                scores[idx] = s[:, :kk]
                rows[idx] = r[:, :kk]
            return [self._hits(rows[b], scores[b], fields) for b in range(B)]

    # -- boosted search: search(ranker=...) ---------------------------------------------
    def _check_boosted(self, data, anns_field, param, limit, expr, group_by_field, mmr_lambda, mmr_fetch_k, offset,
                       ranker) -> list:
        """Everything a boosted search refuses, before anything runs -> the list of its boosts."""
        boosts = check_rankers(ranker)
        self._check_ranked_form("boosted", data, anns_field, param, limit, expr, group_by_field, mmr_lambda, mmr_fetch_k,
                                offset)
        return boosts

    def _check_ranked_form(self, kind, data, anns_field, param, limit, expr, group_by_field, mmr_lambda, mmr_fetch_k,
                           offset) -> None:
        """The forms a search with a ranker (kind: "boosted" or "decayed") does not have."""
        what = f"{kind} search (ranker)"
        if isinstance(expr, (list, tuple)):
            raise ValueError(f"{what} cannot be combined with per-query filters (a list expr)")
        field = self._text_field(anns_field)
        if field is not None:
            raise ValueError(f"{what} has no {field.form} form (anns_field='{field.name}')")
        if anns_field != "embedding":
            raise ValueError(f"unknown vector field {anns_field!r}")
        if self._is_text(data):
            raise ValueError("the embedding field is searched with vectors, not with strings (BM25: anns_field='sparse')")
        if group_by_field is not None:
            raise ValueError(f"{what} cannot be combined with group_by_field")
        if mmr_lambda is not None or mmr_fetch_k is not None:
            raise ValueError(f"{what} cannot be combined with mmr_lambda / mmr_fetch_k")
        if check_offset(offset, param, limit):
            raise ValueError(f"{what} takes no offset")
        if self._band_of(param) is not None:
            raise ValueError(f"{what} has no range form (radius / range_filter)")
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 1 <= limit <= _lib.RF_MAX_K:
            raise ValueError(f"{what}: limit must be an integer in 1..{_lib.RF_MAX_K}, "
                             f"got {limit!r} ({kind} results are not paged)")
        metric = (param or {}).get("metric_type", self.metric_type).upper()
        if metric != self.metric_type:
            raise ValueError(f"collection was built for {self.metric_type}, search asked for {metric}")

    def _search_boosted(self, data, anns_field, param, limit, expr, output_fields, group_by_field, mmr_lambda,
                        mmr_fetch_k, offset, ranker, timing: dict | None = None):
        """search(ranker=...).  timing: a dict that receives the milliseconds of the call's stages
        (filters, classes, sweeps, merge) and its sweep count; it synchronises between the stages
        (tools/bench_boost.py) -- None: the call synchronises for the class counts and the download only."""
        boosts = self._check_boosted(data, anns_field, param, limit, expr, group_by_field, mmr_lambda, mmr_fetch_k,
                                     offset, ranker)
        weights = class_weights(boosts)   # (a product that leaves the doubles raises here)
        fields = self._check_output_fields(output_fields)
        B = self._query_count(data)
        k = int(limit)
        with self._rw.read():
            n = self.num_entities
            if n == 0 or B == 0:
                return [[] for _ in range(B)]
            torch = _torch()
            device = self.index.device
            clock = _StageClock(timing, device)
            # every expression is parsed and built once, before any sweep runs
            base = None if filter_expr.is_empty(expr) else self.build_filter(expr)
            filters = [self.build_filter(b.filter) for b in boosts]
            clock.lap("filters_ms")
            masks, counts = boost_classes(filters, n, base)
            counts = counts.cpu().numpy()   # the one small download the plan needs
            live = [c for c in range(len(weights)) if counts[c] > 0]
            if not live:   # no row passes expr
                return [[] for _ in range(B)]
            q16 = self._prepare_queries(data)
            C = len(live)
            if C == 1:
                # every passing row is in one class: the plain (or filtered) search, scaled by that class's weight
                kw = {} if base is None else {"filt": base}
                clock.lap("classes_ms")
                _, ids, exact = self.index.search(q16, k, want_exact=True, **kw)
                cand_exact, cand_ids = exact.view(B, 1, k), ids.view(B, 1, k)
                sweeps = -(-B // _lib.RF_QCHUNK)
            else:
                class_filters = [filter_from_mask(masks[c], n) for c in live]
                clock.lap("classes_ms")
                # virtual query v = b C + j: query b over the rows of class live[j]; skipped slots stay padded
                cand_exact = torch.full((B * C, k), -np.inf, dtype=torch.float64, device=device)
                cand_ids = torch.full((B * C, k), -1, dtype=torch.int64, device=device)
                plan = plan_filter_chunks(np.tile(np.arange(C), B))
                for idx, used, local in plan:
                    qc = q16[(idx // C).tolist()]   # the chunk's queries, in the order of `local`
                    if len(used) == 1:
                        filt = class_filters[used[0]]
                    else:
                        filt = MultiFilter([class_filters[j] for j in used], local, n, device)
                    _, ids, exact = self.index.search(qc, k, want_exact=True, filt=filt)
                    at = torch.from_numpy(idx).to(device)
                    cand_exact[at] = exact
                    cand_ids[at] = ids
                cand_exact, cand_ids = cand_exact.view(B, C, k), cand_ids.view(B, C, k)
                sweeps = len(plan)
            clock.lap("sweeps_ms")
            scores, rows, _, _ = merge_boosted(cand_exact, cand_ids, [weights[c] for c in live], k)
            packed = torch.cat([rows, scores.view(torch.int32).to(torch.int64)], 1).cpu().numpy()   # the one download
            clock.lap("merge_ms")
            if timing is not None:
                timing.update(sweeps=sweeps, classes=C)
            rows, scores = packed[:, :k], packed[:, k:].astype(np.int32).view(np.float32)
            return [self._hits(rows[b], scores[b], fields) for b in range(B)]

    # -- decayed search: search(ranker=DecayRanker(...)) -----------------------------------
    def _check_decay_field(self, name: str):
        """The field a decay ranker reads: primary_value (-> None) or an INT64 / DOUBLE field of the
        collection's own (-> its FieldSchema).  Anything else raises ValueError naming it."""
        if name == "primary_value":
            return None
        own = self._field(name)
        if own is not None and own.dtype in (DataType.INT64, DataType.DOUBLE):
            return own
        if own is not None:
            why = "an ARRAY field" if own.is_array else f"a {own.dtype.name} field"
        elif name in SCALAR_FIELDS or name in ("embedding", "$meta") or self._text_field(name) is not None:
            why = "a reserved field that holds no number to decay over"
        elif self.enable_dynamic_field:
            why = "a dynamic key (typed per row)"
        else:
            why = "unknown"
        raise ValueError(f"decay ranker: field {name!r} is {why}; it must be primary_value or a declared INT64 / DOUBLE field")

    def _decay_column(self, own):
        """The live device column of a decay field: int64 or fp64 [n], from the mirrors the filters use."""
        with self._filter_lock:
            if own is not None:
                return self._extra_column(own).data
            if self._dcols is None:
                self._dcols = _DeviceColumns(self.index.device)
            self._dcols.sync(self.columns, self.num_entities)
            return self._dcols.values

    def _search_decayed(self, data, anns_field, param, limit, expr, output_fields, group_by_field, mmr_lambda,
                        mmr_fetch_k, offset, ranker: DecayRanker, timing: dict | None = None):
        """search(ranker=DecayRanker(...)): the weights of the live column (rf_decay_weights, per call: add, delete
        and upsert need no bookkeeping), then one weighted sweep per 64 queries through the flagged-query ladder.
        timing: a dict that receives the milliseconds of the call's stages (filter, weights, search); it
        synchronises between them (tools/bench_decay.py)."""
        own = self._check_decay_field(ranker.field)
        self._check_ranked_form("decayed", data, anns_field, param, limit, expr, group_by_field, mmr_lambda, mmr_fetch_k,
                                offset)
        fields = self._check_output_fields(output_fields)
        B = self._query_count(data)
        k = int(limit)
        with self._rw.read():
            n = self.num_entities
            if n == 0 or B == 0:
                return [[] for _ in range(B)]
            torch = _torch()
            clock = _StageClock(timing, self.index.device)
            filt = None if filter_expr.is_empty(expr) else self.build_filter(expr)
            clock.lap("filter_ms")
            weights = decay_weights(self._decay_column(own), ranker)
            clock.lap("weights_ms")
            q16 = self._prepare_queries(data)
            scores, rows, _, _ = self.index.search(q16, k, filt=filt, weights=weights)
            packed = torch.cat([rows, scores.view(torch.int32).to(torch.int64)], 1).cpu().numpy()   # the one download
            clock.lap("search_ms")
            rows, scores = packed[:, :k], packed[:, k:].astype(np.int32).view(np.float32)
            # (when no row passes, every slot is padding and the lists are empty)
            return [self._hits(rows[b], scores[b], fields) for b in range(B)]

    def _check_group_by(self, field, group_size, limit, param):
        """-> (field, group_size), or None for "id" (every row its own group: the plain search)."""
        own = self._field(field)
        if own is not None and own.dtype in (DataType.DOUBLE, DataType.ARRAY):
            raise ValueError(f"group_by_field {field!r}: {'an ARRAY' if own.is_array else 'a DOUBLE'} field cannot be grouped by")
        if self.enable_dynamic_field and field != "id" and field not in self.GROUP_BY_FIELDS and own is None:
            raise ValueError(f"group_by_field {field!r}: a dynamic key cannot be grouped by")
        if field != "id" and field not in self.GROUP_BY_FIELDS and own is None:
            raise ValueError(f"group_by_field {field!r}: only {', '.join(self.GROUP_BY_FIELDS)} (or id) can be grouped by")
        if isinstance(group_size, bool) or not isinstance(group_size, (int, np.integer)) or group_size < 1:
            raise ValueError(f"group_size must be an integer >= 1, got {group_size!r}")
        if limit < 1:
            raise ValueError("limit must be >= 1")
        if self._band_of(param) is not None:
            raise ValueError("group_by_field cannot be combined with range search (radius / range_filter)")
        if field == "id":
            return None
        if limit * group_size > _lib.RF_MAX_K:
            raise ValueError(f"grouping search: limit * group_size = {limit * group_size} > {_lib.RF_MAX_K} "
                             "(grouped results are not paged)")
        return field, int(group_size)

    # -- lexical and hybrid search (rag_fin_amd/lexical.py, rag_fin_amd/hybrid.py) --------
    _is_text = staticmethod(is_text)

    def _check_output_fields(self, output_fields) -> list:
        """With enable_dynamic_field a name that is no field is a dynamic key (the value, or None where the row
        lacks it), and "$meta" is the dict of the keys the row holds."""
        fields = list(output_fields or [])
        for f in fields:
            if f not in self.columns and not (self.enable_dynamic_field and isinstance(f, str)):
                raise KeyError(f"unknown output field {f!r}")
        return fields

    def _entity(self, r: int, fields) -> dict:
        """The output fields of row r (a row's list of an ARRAY field as a copy: the store keeps its own)."""
        if not self.enable_dynamic_field:
            return {f: _out(self.columns[f][r]) for f in fields}
        out = {}
        for f in fields:
            if f in self.columns:
                out[f] = _out(self.columns[f][r])
            elif f == filter_expr.META:
                out[f] = {key: col[r] for key, col in self.dynamic.items() if col[r] is not None}
            else:
                col = self.dynamic.get(f)
                out[f] = None if col is None else col[r]
        return out

    def _search_text_field(self, field, q, limit, expr, fields):
        """The hits of a checked search of one derived field.  Caller holds the read lock."""
        res = field.arm(q, limit, expr)
        if res is None:
            return [[] for _ in range(field.query_count(q))]
        scores, rows = res[0].cpu().numpy(), res[1].cpu().numpy()
        return [self._hits(rows[b], scores[b], fields) for b in range(rows.shape[0])]

    # -- the late-interaction field's stored vectors -----------------------------------------------
    def token_vectors(self, rows) -> list:
        """The stored float16 token vectors of the given rows of the token_embeddings field, one [n_tok, D]
        array each (rows not encoded yet are encoded first)."""
        with self._rw.read():
            return self._late.vectors(rows)

    def rerank_tokens(self, queries, candidates):
        """Candidate-mode MaxSim on the stored token vectors: queries (strings or [n_tok, D] arrays), candidates
        one list of row numbers per query -> one float32 array of scores per query, parallel to its rows (-inf:
        a row without tokens or outside the collection).  One rf_maxsim call for the whole batch."""
        with self._rw.read():
            return self._late.rerank(queries, candidates)

    def _hits(self, rows, scores, fields) -> list:
        """The Hit list of one query from its row numbers (best first, -1 ends it) and scores."""
        hits = []
        for r, s in zip(rows.tolist(), scores.tolist()):
            if r < 0:
                break
            hits.append(Hit(r, self.columns["id"][r], float(s), self._entity(r, fields)))
        return hits

    def _dense_arm(self, q16, limit: int, expr):
        """The dense arm of a hybrid search on the device -> rows i64 [B, limit]: the existing ladder
        (SQ8 first when the index has a shadow), so a flagged query is patched before the fusion."""
        kw = {}
        if not filter_expr.is_empty(expr):
            kw["filt"] = self.build_filter(expr)
        elif self._use_sq8(int(q16.shape[0]), limit):
            kw["sq8"] = True
        return self.index.search(q16, limit, **kw)[1]

    def hybrid_search(self, reqs, rerank, limit: int = 10, output_fields: Iterable[str] | None = None, ranker=None):
        """pymilvus-shaped hybrid search: every AnnSearchRequest of `reqs` (1..4; anns_field "embedding"
        with query vectors, "sparse" with query strings, "sparse_embedding" with query strings or sparse vectors, or
        "token_embeddings" with query strings or lists of token vectors) runs on the GPU with its own limit (<= 64)
        and its own expr, and `rerank` -- an RRFRanker -- fuses the arms' ranked lists per query:
        fused(d) = sum over the arms holding d of weight / (k + rank), the best `limit` (<= 64) rows by
        (fused desc, row asc).  One list of hits per query; hit.score is the fused score.  The fusion
        runs on the device (rf_fuse_rrf) and the call downloads once.  All arms must carry the same
        number of queries; range, grouping and MMR arguments have no hybrid form.  A score-normalising
        ranker is not offered (WeightedRanker raises NotImplementedError; weigh by RRFRanker(weights=...)).
        A boost ranker (ranker=, or a BoostRanker as rerank) has no hybrid form: ValueError."""
        torch = _torch()
        if ranker is not None or isinstance(rerank, (BoostRanker, DecayRanker)):
            raise ValueError("boosted / decayed search (ranker) cannot be combined with hybrid_search")
        reqs = list(reqs)
        if not 1 <= len(reqs) <= MAX_ARMS or not all(isinstance(r, AnnSearchRequest) for r in reqs):
            raise ValueError(f"hybrid_search takes 1..{MAX_ARMS} AnnSearchRequest objects")
        if not isinstance(rerank, RRFRanker):
            raise ValueError("hybrid_search: rerank must be an RRFRanker (score-normalising rankers are not "
                             "supported; use RRFRanker(weights=...))")
        weights = rerank.arm_weights(len(reqs))
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 1 <= limit <= _lib.RF_MAX_K:
            raise ValueError(f"hybrid_search: limit must be an integer in 1..{_lib.RF_MAX_K}, got {limit!r}")
        fields = self._check_output_fields(output_fields)
        with self._rw.read():
            # every arm is checked before any runs
            prepared = []
            for r in reqs:
                if isinstance(r.expr, (list, tuple)):
                    raise ValueError("hybrid_search: an arm takes one expr string, not a list (per-query filters)")
                if r.limit > _lib.RF_MAX_K:
                    raise ValueError(f"hybrid_search: an arm's limit is at most {_lib.RF_MAX_K}, got {r.limit}")
                field = self._text_field(r.anns_field)
                if field is not None:
                    q = field.check_search(r.data, r.param, r.limit)
                    prepared.append((r, q, field.query_count(q)))
                elif r.anns_field == "embedding":
                    if self._is_text(r.data):
                        raise ValueError("the embedding field is searched with vectors, not with strings")
                    metric = str(r.param.get("metric_type", self.metric_type)).upper()
                    if metric != self.metric_type:
                        raise ValueError(f"collection was built for {self.metric_type}, search asked for {metric}")
                    if self._band_of(r.param) is not None:
                        raise ValueError("hybrid_search: an arm takes no range parameters (radius / range_filter)")
                    if check_offset(None, r.param, r.limit):
                        raise ValueError("hybrid_search: an arm takes no offset")
                    q = self._prepare_queries(r.data)
                    prepared.append((r, q, int(q.shape[0])))
                else:
                    raise ValueError(f"unknown vector field {r.anns_field!r}")
            B = prepared[0][2]
            if any(n != B for _, _, n in prepared):
                raise ValueError(f"hybrid_search: the arms carry {[n for _, _, n in prepared]} queries; all must "
                                 "carry the same number")
            if self.num_entities == 0 or B == 0:
                return [[] for _ in range(B)]
            F = max(r.limit for r in reqs)
            device = self.index.device
            arms = []
            for r, q, _ in prepared:
                field = self._text_field(r.anns_field)
                if field is not None:
                    res = field.arm(q, r.limit, r.expr)
                    rows = None if res is None else res[1]
                else:
                    rows = self._dense_arm(q, r.limit, r.expr)
                block = torch.full((B, F), -1, dtype=torch.int64, device=device)
                if rows is not None:
                    block[:, :r.limit] = rows
                arms.append(block)
            _, rows, fused = fuse_rrf(torch.stack(arms), int(limit), weights, rerank.k)
            packed = torch.stack([rows, fused.view(torch.int64)]).cpu().numpy()   # the one download
            rows, fused = packed[0], packed[1].view(np.float64)
            return [self._hits(rows[b], fused[b], fields) for b in range(B)]

    def _search(self, data, anns_field, param, limit, expr, output_fields, group=None, mmr=None, offset: int = 0):
        if anns_field != "embedding":
            raise ValueError(f"unknown vector field {anns_field!r}")
        if self._is_text(data):
            raise ValueError("the embedding field is searched with vectors, not with strings (BM25: anns_field='sparse')")
        metric = (param or {}).get("metric_type", self.metric_type).upper()
        if metric != self.metric_type:
            raise ValueError(f"collection was built for {self.metric_type}, search asked for {metric}")
        fields = self._check_output_fields(output_fields)
        band = self._band_of(param)
        kw = {} if band is None else {"band": band}
        if mmr is not None:
            kw["mmr"] = mmr
        if group is not None:
            # the padded [B, limit * group_size] block; short and missing groups leave -1 slots
            filt = None if filter_expr.is_empty(expr) else self.build_filter(expr)
            scores, rows = self._search_rows(data, limit, filt, group=group)
            if group[0] not in fields:
                fields = fields + [group[0]]
        elif filter_expr.is_empty(expr):
            scores, rows = self.search_rows(data, offset + limit, **kw)
        else:
            scores, rows = self.search_rows(data, offset + limit, filt=self.build_filter(expr), **kw)
        out = []
        for b in range(rows.shape[0]):
            hits = []
            for j in range(offset, rows.shape[1]):
                r = int(rows[b, j])
                if r < 0:
                    if group is not None:
                        continue
                    break
                hits.append(Hit(r, self.columns["id"][r], float(scores[b, j]), self._entity(r, fields)))
            out.append(hits)
        return out

    def search_iterator(self, data, anns_field: str = "embedding", param: dict | None = None,
                        batch_size: int = 1000, limit: int = -1, expr=None,
                        output_fields: Iterable[str] | None = None, ranker=None):
        """pymilvus-shaped search_iterator: an object with next() -> the next batch_size hits (a list
        of Hit, [] when done) and close().  ONE query vector (ValueError for more, as pymilvus).
        The pages concatenated are search(limit=N): the iterator keeps the last hit's fp64 score and
        row on the device, and a next() costs ceil(batch_size / 64) search-after sweeps of the corpus
        (GpuIndex.search_after), not a search from the top.  expr: the filter buffer is built once.
        param["params"] may hold radius / range_filter.  limit: hits in all (-1: until the collection
        is exhausted).  The bound is a row number: an insert, delete, upsert or drop between two
        next() calls makes the next one raise RuntimeError.  A boost ranker is not paged: ValueError."""
        if ranker is not None:
            raise ValueError("boosted / decayed search (ranker) cannot be combined with search_iterator")
        if isinstance(expr, (list, tuple)):
            raise ValueError("search_iterator takes one expr string, not a list (per-query filters)")
        if anns_field == TOKEN_FIELD:
            raise ValueError("search_iterator has no late-interaction form (anns_field='token_embeddings')")
        return SearchIterator(self, data, anns_field, param, batch_size, limit, expr, output_fields)

    @staticmethod
    def _band_of(param):
        """The range-search band of a pymilvus search `param`, or None."""
        params = (param or {}).get("params")
        if params is None:
            return None
        if not isinstance(params, dict):
            raise ValueError("search: param['params'] must be a dict")
        return check_band(params.get("radius"), params.get("range_filter"))

    # -- persistence -------------------------------------------------
    # The reference leans on the Milvus server for durability and re-creates the
    # collection on every ingest ("chunking_storing (1).py":25-28); an in-process store
    # needs its own format.  Directory layout:
    #   vectors.f16   raw little-endian fp16, row-major [n, dim]   (np.memmap-able)
    #   columns.json  {"name", "dim", "metric_type", "n", "columns": {field: [...]}}
    def save(self, path: str, chunk_rows: int = 1 << 18) -> None:
        with self._rw.read():
            self._save(path, chunk_rows)

    def _save(self, path: str, chunk_rows: int) -> None:
        os.makedirs(path, exist_ok=True)
        n = self.num_entities
        tmp = os.path.join(path, "vectors.f16.tmp")
        with open(tmp, "wb") as f:
            for s0 in range(0, n, chunk_rows):
                rows = np.arange(s0, min(n, s0 + chunk_rows), dtype=np.int64)
                f.write(self.index.get_rows(rows).cpu().numpy().tobytes())
        os.replace(tmp, os.path.join(path, "vectors.f16"))
        self._write_meta(path, n)

    def _write_meta(self, path: str, n: int) -> None:
        """columns.json, written to a temporary file and moved into place."""
        meta = {"format": FORMAT, "name": self.name, "dim": self.dim,
                "metric_type": self.metric_type, "n": n, "columns": self.columns}
        if self.schema:   # (directories of a store without fields of its own stay exactly as before)
            meta["fields"] = [f.to_dict() for f in self.schema]
        if self.enable_dynamic_field:   # (None -> null; json keeps 3 apart from 3.0 and true apart from 1)
            meta["enable_dynamic_field"] = True
            meta["dynamic"] = self.dynamic
        if self.index_type != "FLAT":   # FLAT directories stay exactly as before
            meta["index_type"] = self.index_type
        if self._lexical.declared:   # (and so do directories without a lexical index)
            meta["sparse_index"] = dict(self._lexical.params)
        tmp = os.path.join(path, "columns.json.tmp")
        with open(tmp, "w", encoding="utf-8") as f:
            json.dump(meta, f, ensure_ascii=False)
        os.replace(tmp, os.path.join(path, "columns.json"))

    @staticmethod
    def _read_meta(path: str):
        """columns.json of a corpus directory -> (meta, n, dim)."""
        with open(os.path.join(path, "columns.json"), encoding="utf-8") as f:
            meta = json.load(f)
        if meta.get("format") != FORMAT:
            raise ValueError(f"{path}: not a ragfin corpus directory")
        return meta, int(meta["n"]), int(meta["dim"])

    def _load_rows(self, path: str, n: int, lo: int, hi: int, chunk_rows: int) -> None:
        """Memory-map vectors.f16 (n rows); stream rows [lo, hi) into the index chunk by chunk."""
        torch = _torch()
        if not n:
            return
        expect = n * self.dim * 2
        got = os.path.getsize(os.path.join(path, "vectors.f16"))
        if got != expect:
            raise ValueError(f"{path}/vectors.f16 holds {got} bytes, expected {expect}")
        mm = np.memmap(os.path.join(path, "vectors.f16"), dtype=np.float16, mode="r", shape=(n, self.dim))
        for s0 in range(lo, hi, chunk_rows):
            s1 = min(hi, s0 + chunk_rows)
            self.index.add(torch.from_numpy(np.ascontiguousarray(mm[s0:s1])).to(self.index.device))
        del mm

    def _adopt_columns(self, path: str, meta: dict, n: int) -> None:
        """The scalar columns of a loaded columns.json become this store's; the pk map is rebuilt."""
        cols = meta["columns"]
        if any(len(cols[f]) != n for f in SCALAR_FIELDS) or any(len(cols.get(f.name, ())) != n for f in self.schema):
            raise ValueError(f"{path}: column lengths do not match n={n}")
        self.columns = {f: list(cols[f]) for f in SCALAR_FIELDS}
        for f in self.schema:
            self.columns[f.name] = schema_.column_from_json(f, cols[f.name])
        if self.enable_dynamic_field:
            self.dynamic = schema_.check_dynamic(meta.get("dynamic"), n, what=path)
        self._pk_row = {pk: i for i, pk in enumerate(self.columns["id"])}

    @classmethod
    def load_from(cls, path: str, device=None, capacity: int | None = None,
                  chunk_rows: int = 1 << 18) -> "CorpusStore":
        """Memory-map vectors.f16 and stream it into HBM in chunks (never the whole file
        in host RAM)."""
        meta, n, dim = cls._read_meta(path)
        st = cls(meta["name"], dim=dim, capacity=max(capacity or 0, n, 1), device=device,
                 metric_type=meta["metric_type"],
                 **({"fields": [FieldSchema.from_dict(d) for d in meta["fields"]]} if meta.get("fields") else {}),
                 **({"enable_dynamic_field": True} if meta.get("enable_dynamic_field") else {}))
        st._load_rows(path, n, 0, n, chunk_rows)
        st._adopt_columns(path, meta, n)
        itype = meta.get("index_type", "FLAT")   # a missing key means FLAT
        if itype != "FLAT":
            st.create_index("embedding", {"index_type": itype, "metric_type": st.metric_type})
        st._adopt_sparse(meta)
        return st

    def _adopt_sparse(self, meta: dict) -> None:
        """Re-declare the lexical index a saved store had (the postings are rebuilt on first use)."""
        if meta.get("sparse_index") is not None:
            field = self._lexical
            self.create_index(field.name, {"index_type": field.index_type, "metric_type": field.metric_type,
                                           "params": dict(meta["sparse_index"])})

    # -- filters -------------------------------------------------------------------------
    def build_filter(self, expr: str):
        """Parse + compile `expr` (rag_fin_amd.filter_expr; ValueError on a bad expression) and
        evaluate it on the device into a fresh filter buffer for this collection's rows.  One
        buffer per call: concurrent searches with different filters do not share one.
        TEXT_MATCH / PHRASE_MATCH leaves read the lexical index (create_index("sparse", ...) first:
        ValueError without it): rf_text_match turns their posting lists into row bitmaps and the
        filter program reads those, both on the current stream.  The first PHRASE_MATCH after a
        change of the rows also builds the token positions, once (by the route that built the index).

        Lock order: the read/write lock (held by the caller: search, query and delete take it; delete
        holds the WRITE side, so nothing here may ask for it again), then `_sparse_lock` (the one lock of the
        fields derived from the text column: inside LexicalField.index and .text_index, released before the next;
        the learned sparse and token fields build under it too), then `_filter_lock`, then the
        SparseIndex's own `_lock` (inside text_match).  No path takes them the other way round."""
        node = filter_expr.parse(expr, self.analyzer, self.schema, self.enable_dynamic_field)
        term_id, sp = self._lexical.text_index(filter_expr.text_leaves(node))
        with self._filter_lock:
            n = self.num_entities
            if self._dcols is None:
                self._dcols = _DeviceColumns(self.index.device)
            self._dcols.sync(self.columns, n)
            own = {f.name: self._extra_column(f) for f in self.schema
                   if not f.is_array and f.name in filter_expr.fields_of(node)}
            # (only the ARRAY fields this expression reads are mirrored)
            arrs = {f.name: self._array_column(f) for f in self.schema
                    if f.is_array and f.name in filter_expr.array_fields_of(node)}
            # (only the dynamic keys this expression reads, and of those the ones some row holds, are mirrored)
            dyn = {key: self._dynamic_column(key) for key in sorted(filter_expr.dynamic_keys_of(node))
                   if key in self.dynamic} if self.enable_dynamic_field else None
            prog = filter_expr.compile_expr(node, self._dcols.dicts, self._pk_row, term_id, self.schema,
                                            {name: c.dict for name, c in {**own, **arrs}.items() if c.coded},
                                            None if dyn is None else {key: c.dict for key, c in dyn.items()})
            if not prog.column_leaves and not prog.dynamic_leaves and not prog.array_leaves:
                bitmaps = sp.text_match(prog.text_leaves) if prog.text_leaves else None
                return eval_filter(self.index.device, prog, self._dcols.tensors(), n, bitmaps)
            # leaves over the collection's own fields: rf_column_match writes their row bitmaps behind the
            # keyword leaves', into the one array the program's RF_FOP_BITMAP leaves index
            # and rf_dynamic_match the dynamic leaves' behind those, rf_array_match the array
            # leaves' behind those
            T, C, D = len(prog.text_leaves), len(prog.column_leaves), len(prog.dynamic_leaves)
            base, nwords = T * text_words_per_leaf(n), (n + 31) // 32
            mid = base + C * nwords
            end = mid + D * nwords
            bitmaps = _torch().empty(end + len(prog.array_leaves) * nwords, dtype=_torch().int32, device=self.index.device)
            if T:
                sp.text_match(prog.text_leaves, out=bitmaps[:base].view(T, -1))
            if C:
                column_match(self.index.device, prog, {name: c.data for name, c in own.items()}, n, out=bitmaps[base:mid])
            if D:
                dynamic_match(self.index.device, prog, {key: (c.tags, c.payload) for key, c in dyn.items()}, n,
                              out=bitmaps[mid:end])
            if prog.array_leaves:
                array_match(self.index.device, prog, {name: (c.offsets, c.values) for name, c in arrs.items()}, n,
                            out=bitmaps[end:])
            return eval_filter(self.index.device, prog, self._dcols.tensors(), n, bitmaps, column_base=base)

    def filter_rows(self, expr: str) -> np.ndarray:
        """Row numbers (ascending) that pass `expr`."""
        return np.flatnonzero(filter_mask_bits(self.build_filter(expr), self.num_entities))

    # -- scalar queries ----------------------------------------------------------------
    def query(self, expr: str = "", limit: int | None = None,
              output_fields: Iterable[str] | None = None, offset: int = 0) -> list[dict]:
        """`query(expr="id in [...]")` fetch-by-PK (key order), `query(expr="", limit=n)` scan, and
        any other filter expression (rag_fin_amd.filter_expr): the matching rows in ascending
        row order.  offset (an int >= 0, else ValueError): skip that many of the matching rows
        first, on the host; `limit` counts from there.
        output_fields=["count(*)"] (pymilvus' idiom) returns [{"count(*)": n}], the number of rows `expr` matches:
        num_entities for an empty expr, the keys present for `id in [...]`, else n_pass_rows of the filter
        buffer's header -- no row is fetched.  count(*) beside other fields, `limit` or `offset` raises ValueError.
        output_fields may also hold "sum(f)", "avg(f)", "min(f)", "max(f)" (f: primary_value or an INT64 / DOUBLE field;
        at most 4 distinct fields), beside each other and beside "count(*)": one dict keyed by those strings, from
        the one-slot group of rf_facet_stats (facets.stats_reference defines the values: an fp64 sum is the exact sum
        rounded once).  The same refusals hold."""
        if expr is not None and not isinstance(expr, str):
            raise ValueError(f"filter expression must be a string, got {type(expr).__name__}")
        if not isinstance(output_fields, str) and output_fields is not None:
            output_fields = list(output_fields)
            aggs = [facets_.parse_aggregate(f) for f in output_fields]
            if facets_.COUNT_STAR in output_fields or any(aggs):
                what = "count(*)" if facets_.COUNT_STAR in output_fields else "an aggregate"
                if any(a is None and f != facets_.COUNT_STAR for a, f in zip(aggs, output_fields)):
                    raise ValueError(f"query: {what} cannot be combined with other output_fields")
                if limit is not None:
                    raise ValueError(f"query: {what} cannot be combined with limit")
                if offset:
                    raise ValueError(f"query: {what} cannot be combined with offset")
                if not any(aggs):
                    if len(output_fields) != 1:
                        raise ValueError("query: count(*) cannot be combined with other output_fields")
                    with self._rw.read():
                        return [{facets_.COUNT_STAR: self._count(expr)}]
                # sum(f) / avg(f) / min(f) / max(f), beside each other and beside count(*): one dict keyed by them
                names = list(dict.fromkeys(a[1] for a in aggs if a))
                if len(names) > facets_.MAX_METRICS:   # (each call of the kernel takes MAX_METRICS columns)
                    raise ValueError(f"query: aggregates over at most {facets_.MAX_METRICS} fields, got {len(names)}")
                mplan = facets_.check_metrics(names, self.schema)
                with self._rw.read():
                    stats = self._aggregate(expr, mplan)
                    rec = {f: stats[a[1]][a[0]] for a, f in zip(aggs, output_fields) if a}
                    if facets_.COUNT_STAR in output_fields:
                        rec[facets_.COUNT_STAR] = self._count(expr)
                return [{f: rec[f] for f in output_fields}]
        offset = check_offset(offset, None, 1)
        with self._rw.read():
            return self._query(expr, limit, output_fields, offset)

    def _count(self, expr) -> int:
        """The rows `expr` matches.  Caller holds the read lock."""
        if filter_expr.is_empty(expr):
            return self.num_entities
        keys = _id_in_keys(expr)
        if keys is not None:
            return len({k for k in keys if k in self._pk_row})
        if self.num_entities == 0:
            return int(self._match_mask(expr).sum())   # (still rejects a bad expression)
        return self._filter_header(self.build_filter(expr))[1]

    @staticmethod
    def _filter_header(filt) -> tuple:
        """(n_rows, n_pass_rows, n_pass_blocks, n_tiles) of a filter buffer (synchronises)."""
        return tuple(int(v) for v in filt[:16].cpu().numpy().view(np.uint32))

    # -- faceted counts (rag_fin_amd/facets.py) ---------------------------------------
    def facets(self, fields=None, expr: str | None = None, limit: int = 10, min_count: int = 1, ranges=None,
               metrics=None) -> dict:
        """How many of the rows `expr` passes (every row without one; anything a filter takes) hold each value of
        `fields`, and how many fall into each of `ranges` -- facets.py has the definition, facets_reference:
            {"count": passing rows,
             "facets": {field: {"buckets": [{"value", "count"}, ...], "distinct", "missing", "other"}},
             "ranges": {field: {"ranges": [{"from", "to", "count"}, ...], "min", "max", "nan"}}}
        fields: period / chunk_type / statement_type, the collection's VARCHAR / BOOL / INT64 fields, its ARRAY
        fields of VARCHAR or BOOL elements (a row counts once per distinct element) and dynamic keys (bare or
        $meta["key"]).  ranges: {field: [(lo, hi), ...]}, each [lo, hi) with None for no bound, over primary_value
        and INT64 / DOUBLE fields.  Counted on the GPU from the columns' dictionary codes (rf_facet_counts,
        rf_facet_select, rf_facet_ranges); exact and the same on every run.  ValueError on a bad argument.
        metrics: up to 4 of primary_value and the INT64 / DOUBLE fields.  Every bucket then carries
        "metrics": {field: {"count", "nan", "sum", "avg", "min", "max"}} over the rows counted in it, and the result
        a top-level "metrics" over all passing rows (facets.stats_reference has the definition).  A DOUBLE sum is the
        exact sum rounded once -- what math.fsum returns -- accumulated in fixed point with integer atomics
        (rf_facet_stats), so it too has the same bits on every run.  On the CPU double of the index the metrics
        come from the reference."""
        mplan = None
        if metrics is None:
            fields, limit, min_count, ranges = facets_.check_args(fields, limit, min_count, ranges)
        else:
            fields, limit, min_count, ranges, mplan = facets_.check_args(fields, limit, min_count, ranges, metrics,
                                                                         self.schema)
        if expr is not None and not isinstance(expr, str):
            raise ValueError(f"filter expression must be a string, got {type(expr).__name__}")
        plan = [(name,) + facets_.resolve_value_field(name, self.schema, self.enable_dynamic_field) for name in fields]
        rplan = [(name,) + facets_.resolve_range_field(name, self.schema) for name in ranges]
        extra = {} if metrics is None else {"metrics": metrics}
        with self._rw.read():
            n = self.num_entities
            if n == 0:   # nothing to count (a bad expression is still rejected)
                if not filter_expr.is_empty(expr):
                    self._match_mask(expr)
                return facets_.facets_reference(self.columns, self.schema, self.dynamic if self.enable_dynamic_field
                                                else None, fields, [], limit, min_count, ranges, **extra)
            if mplan is not None and self._on_host():
                rows = range(n) if filter_expr.is_empty(expr) else self._expr_rows(expr)
                return facets_.facets_reference(self.columns, self.schema, self.dynamic if self.enable_dynamic_field
                                                else None, fields, rows, limit, min_count, ranges, **extra)
            filt = None if filter_expr.is_empty(expr) else self.build_filter(expr)
            return self._facets(plan, rplan, ranges, filt, n, limit, min_count, mplan)

    def _on_host(self) -> bool:
        """The index is the CPU double (tests): there is no device to aggregate on."""
        return getattr(self.index.device, "type", "cuda") == "cpu"

    def _facet_rank(self, holder, key, vals: list, dynamic: bool):
        """The value rank of every bin of a dictionary (facets.value_ranks; a dynamic key's False and True behind
        its strings) as an int32 device tensor, kept beside the mirror and derived again when the dictionary has
        grown.  Caller holds `_filter_lock`."""
        cache = holder.facet_ranks
        hit = cache.get(key)
        if hit is None or hit[0] != len(vals):
            rank = facets_.value_ranks(vals + [False, True] if dynamic else vals)
            hit = cache[key] = (len(vals), _torch().from_numpy(rank).to(self.index.device))
        return hit[1]

    def _metric_column(self, name: str, n: int):
        """The fp64 / int64 device column of a metric or range field.  Caller holds `_filter_lock`."""
        if name == "primary_value":
            if self._dcols is None:
                self._dcols = _DeviceColumns(self.index.device)
            self._dcols.sync(self.columns, n)
            return self._dcols.values.contiguous()
        return self._extra_column(self._field(name)).data.contiguous()

    @staticmethod
    def _stats_dicts(stats, kinds: list) -> list:
        """The compact records of rf_facet_stats_finish (int64 [records, RF_STATS_OUT]; record r belongs to metric
        r % len(kinds)) -> per record the stats of facets.stats_reference.  Converted to Python numbers once for all
        records: a call with limit=1000 has thousands."""
        ints, floats = stats.tolist(), np.ascontiguousarray(stats).view(np.float64).tolist()
        out = []
        for r, (rec, frec) in enumerate(zip(ints, floats)):
            count = rec[0]
            if kinds[r % len(kinds)] == "i64":
                total = rec[2] + (rec[3] << 32)
                out.append({"count": count, "nan": 0, "sum": total, "avg": total / count if count else None,
                            "min": rec[4] if count else None, "max": rec[5] if count else None})
            else:
                total = frec[2]
                out.append({"count": count, "nan": rec[1], "sum": total, "avg": total / count if count else None,
                            "min": frec[4] if count else None, "max": frec[5] if count else None})
        return out

    def _aggregate(self, expr, mplan) -> dict:
        """{field: stats} over the rows `expr` matches: the one-slot group of rf_facet_stats alone, no value field
        and no select.  Caller holds the read lock."""
        n = self.num_entities
        if n == 0 or self._on_host():
            if n == 0 and not filter_expr.is_empty(expr) and _id_in_keys(expr) is None:
                self._match_mask(expr)   # (still rejects a bad expression)
            rows = self._aggregate_rows(expr) if n else []
            return {name: facets_.stats_reference([self.columns[name][r] for r in rows], kind) for name, kind in mplan}
        keys = None if filter_expr.is_empty(expr) else _id_in_keys(expr)
        if keys is not None:   # the keys present, each once: a mask of their rows
            mask = np.zeros((n + 31) // 32 * 32, dtype=bool)
            mask[[self._pk_row[k] for k in keys if k in self._pk_row]] = True
            words = np.packbits(mask, bitorder="little").view(np.int32)   # bit r of word b = row 32 b + r
            filt = filter_from_mask(_torch().from_numpy(words).to(self.index.device), n)
        else:
            filt = None if filter_expr.is_empty(expr) else self.build_filter(expr)
        with self._filter_lock:
            cols = [(self._metric_column(name, n), kind == "f64") for name, kind in mplan]
        got = self._stats_dicts(facet_stats_all(self.index.device, filt, cols, n), [kind for _, kind in mplan])
        return {name: rec for (name, _), rec in zip(mplan, got)}

    def _aggregate_rows(self, expr) -> list:
        if filter_expr.is_empty(expr):
            return list(range(self.num_entities))
        keys = _id_in_keys(expr)
        if keys is not None:
            return sorted({self._pk_row[k] for k in keys if k in self._pk_row})
        return [int(r) for r in self._expr_rows(expr)]

    def _facets(self, plan, rplan, ranges, filt, n: int, limit: int, min_count: int, mplan=None) -> dict:
        """facets() on the device.  Caller holds the read lock.  The columns are mirrored under `_filter_lock` (after
        build_filter has released it: the lock order of build_filter holds), which is held only until the call has
        its references: a sync or a compaction replaces a mirror's tensors and never writes into them, and the read
        lock keeps the rows as they are, so the kernels and their downloads run outside it and concurrent filter
        builds do not wait for them."""
        dev = self.index.device
        out = {"count": n, "facets": {}, "ranges": {}}
        with self._filter_lock:
            specs, values = [], []
            for name, kind, what in plan:
                if kind == "builtin":
                    if self._dcols is None:
                        self._dcols = _DeviceColumns(dev)
                    self._dcols.sync(self.columns, n)
                    vals, holder = self._dcols.dicts[what], (self._dcols, what)
                    spec = {"kind": _lib.RF_FACET_CODES, "a": self._dcols.codes[what].contiguous()}
                elif kind == "own":
                    col = self._extra_column(what, coded=True)
                    vals, holder = col.dict, (col, None)
                    spec = {"kind": _lib.RF_FACET_CODES, "a": col.data.contiguous()}
                elif kind == "array":
                    col = self._array_column(what)
                    vals, holder = col.dict, (col, None)
                    spec = {"kind": _lib.RF_FACET_ARRAY, "a": col.offsets, "b": col.values, "c": col.first_occurrence()}
                elif what in self.dynamic:
                    col = self._dynamic_column(what)
                    vals, holder = col.dict, (col, None)
                    spec = {"kind": _lib.RF_FACET_DYNAMIC, "a": col.tags, "b": col.payload}
                else:   # a key no row holds: every passing row is `missing`
                    specs.append(None)
                    values.append(None)
                    continue
                # (a dictionary only grows, and under this lock: the first n_codes entries are what the codes mean)
                spec["n_codes"] = len(vals)
                spec["rank"] = self._facet_rank(*holder, vals, spec["kind"] == _lib.RF_FACET_DYNAMIC)
                specs.append(spec)
                values.append(vals)
            rcols = []
            for name, kind, colname in rplan:
                if colname == "primary_value":
                    if self._dcols is None:
                        self._dcols = _DeviceColumns(dev)
                    self._dcols.sync(self.columns, n)
                    column = self._dcols.values
                else:
                    column = self._extra_column(self._field(colname)).data
                rcols.append(column.contiguous())
            mcols = [(self._metric_column(name, n), kind == "f64") for name, kind in mplan or ()]
        live = [s for s in specs if s is not None]
        stats = None
        if not mplan:   # (metrics=[] asks for nothing more: every "metrics" is {})
            got = iter(facet_counts(dev, filt, live, n, limit, min_count)) if live else iter(())
        elif live:
            got, stats = facet_counts(dev, filt, live, n, limit, min_count, metrics=mcols)
            got = iter(got)
        else:
            got, stats = iter(()), facet_stats_all(dev, filt, mcols, n)
        rgot = []
        for (name, kind, colname), column in zip(rplan, rcols):
            bounds = []
            for lo, hi in ranges[name]:
                if kind == "i64":
                    bounds.append(facets_.int_bounds(lo, hi))
                else:
                    no_lo, no_hi, flo, fhi = facets_.float_bounds(lo, hi)
                    bounds.append((no_lo, no_hi, False, flo, fhi))
            rgot.append(facet_ranges(dev, filt, column, kind == "f64", bounds, n))
        if filt is not None:
            out["count"] = self._filter_header(filt)[1]
        S = _lib.RF_FACET_SCALARS
        nm = len(mplan or ())
        if stats is not None:
            stats = self._stats_dicts(stats, [kind for _, kind in mplan])
        at = 0   # the field's first record in `stats`: min(limit, bins) slots of one record per metric
        for (name, _, _), spec, vals in zip(plan, specs, values):
            if spec is None:
                out["facets"][name] = {"buckets": [], "distinct": 0, "missing": out["count"], "other": 0}
                continue
            row = next(got)
            sel, distinct, sel_sum, missing, total = (int(v) for v in row[:5])
            out["facets"][name] = {
                # (a dynamic key's bins n_codes and n_codes + 1 are False and True)
                "buckets": [{"value": vals[int(b)] if b < spec["n_codes"] else bool(b - spec["n_codes"]), "count": int(c)}
                            for c, b in zip(row[S:S + sel], row[S + limit:S + limit + sel])],
                "distinct": distinct, "missing": missing, "other": total - sel_sum}
            if mplan is not None:
                for slot, b in enumerate(out["facets"][name]["buckets"]):
                    b["metrics"] = {m: stats[at + slot * nm + j] for j, (m, _) in enumerate(mplan)}
                at += nm * facet_stats_slots(spec, limit)
        if mplan is not None:
            out["metrics"] = {m: stats[at + j] for j, (m, _) in enumerate(mplan)}
        for (name, kind, _), r in zip(rplan, rgot):
            M = _lib.RF_FACET_MAX_RANGES
            any_valid = int(r[M + 1]) > 0
            ext = r[M + 2:M + 4]
            lo_hi = [None, None] if not any_valid else \
                ([int(v) for v in ext] if kind == "i64" else [float(v) for v in ext.view(np.float64)])
            out["ranges"][name] = {
                "ranges": [{"from": lo, "to": hi, "count": int(c)} for (lo, hi), c in zip(ranges[name], r[:M])],
                "min": lo_hi[0], "max": lo_hi[1], "nan": int(r[M])}
        return out

    def _query(self, expr, limit, output_fields, offset: int = 0) -> list[dict]:
        fields = list(output_fields or ["id"])
        want_vec = "embedding" in fields
        fields = self._check_output_fields(f for f in fields if f != "embedding")
        if expr is None or expr.strip() == "":
            rows = list(range(self.num_entities))
        else:
            keys = _id_in_keys(expr)
            if keys is not None:
                rows = [self._pk_row[k] for k in keys if k in self._pk_row]
            else:
                rows = self._expr_rows(expr).tolist()
        if offset:
            rows = rows[offset:]
        if limit is not None:
            rows = rows[:limit]
        vecs = self.index.get_rows(np.asarray(rows, dtype=np.int64)).float().cpu().numpy() \
            if (want_vec and rows) else None
        out = []
        for j, r in enumerate(rows):
            rec = self._entity(r, fields)
            if "id" not in rec:
                rec["id"] = self.columns["id"][r]
            if vecs is not None:
                rec["embedding"] = vecs[j].tolist()
            out.append(rec)
        return out

    def _expr_rows(self, expr: str) -> np.ndarray:
        return self.filter_rows(expr)


def _out(v):
    return list(v) if isinstance(v, list) else v


def _id_in_keys(expr: str):
    """The keys of the original `id in [...]` form (a Python list literal, kept in key order),
    or None when `expr` is not of that form."""
    m = _ID_IN.match(expr)
    if not m:
        return None
    import ast
    body = m.group(1).strip()
    try:
        return list(ast.literal_eval("[" + body + "]")) if body else []
    except (ValueError, SyntaxError):
        return None
