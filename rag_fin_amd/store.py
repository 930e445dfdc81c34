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
"""
from __future__ import annotations

import contextlib
import ctypes
import itertools
import re
import threading
from ctypes import c_void_p
from typing import Any, Iterable, Sequence

import numpy as np

from . import _lib
from . import filter_expr

import os as _os
# RAGFIN_ZERO_COPY=0: search_host copies results with async memcpys instead of letting the merge kernel
# store into the pinned host buffers (A/B switch)
_ZERO_COPY = _os.environ.get("RAGFIN_ZERO_COPY", "1") != "0"

SCALAR_FIELDS = ("id", "text", "period", "chunk_type", "statement_type", "primary_value")


def _torch():
    import torch
    return torch


def require_gpu(device=None):
    """Fail loudly when there is no MI355X to run on."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError("rag_fin_amd needs a ROCm GPU (gfx950); torch.cuda.is_available() is "
                           "False and there is no CPU fallback")
    dev = torch.device(device if device is not None else "cuda:0")
    if dev.type != "cuda":
        raise RuntimeError(f"device {dev} is not a GPU")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    _lib.check(_lib.load_library().rf_device_check(idx))
    return torch.device("cuda", idx)


def rerun_flagged(q16, k: int, id_base: int, flags, sq8: bool, filt, flat, exhaustive):
    """The flagged-query ladder ("fallback"): a query the first pass could not prove
    exact (flags != 0) is re-run one tier down.  A query flagged by an SQ8 first pass (`sq8`) goes
    through the FLAT chain, and only one that flags there too goes to the exhaustive kernel; one
    flagged by a FLAT or filtered (`filt`) first pass goes straight to the exhaustive kernel, over
    the same passing rows.  The tiers are callables, on whatever device their tensors live:
      flat(q, k, id_base)             -> (scores, ids, exact | None, flags)
      exhaustive(q, k, id_base, filt) -> (scores, ids, exact | None)
    -> (bad, rows): the indices of the re-run queries (on the device of `flags`) and their
    replacement [scores, ids, exact | None], each row from the last tier that ran it; rows is
    None when nothing was flagged.  The caller patches its own destination."""
    torch = _torch()
    bad = torch.nonzero(flags != 0).flatten()
    if bad.numel() == 0:
        return bad, None
    qb = q16[bad.to(q16.device)].contiguous()
    if not sq8:
        return bad, list(exhaustive(qb, k, id_base, filt))
    *rows, f2 = flat(qb, k, id_base)
    again = torch.nonzero(f2 != 0).flatten()
    if again.numel() > 0:
        for dst, src in zip(rows, exhaustive(qb[again].contiguous(), k, id_base, filt)):
            if dst is not None:
                dst[again] = src
    return bad, rows


def mask_words(bits):
    """bool [n] (device) -> the filter mask words int32 [ceil(n / 32)]: bit r of word b = row 32 b + r."""
    torch = _torch()
    n = bits.numel()
    nblk = (n + 31) // 32
    pad = torch.zeros(nblk * 32, dtype=torch.int64, device=bits.device)
    pad[:n] = bits.to(torch.int64)
    w = (pad.view(nblk, 32) << torch.arange(32, dtype=torch.int64, device=bits.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def words_mask(words, n: int):
    """The inverse of mask_words: int32 words (device) -> bool [n]."""
    torch = _torch()
    sh = torch.arange(32, dtype=torch.int64, device=words.device)
    return (((words.to(torch.int64).unsqueeze(1) >> sh) & 1) != 0).flatten()[:n]


def grouped_exhaustive(q16, group, pass_bits, exhaustive_masked):
    """The flagged-query ladder of a grouping search, and the path of a dictionary
    above RF_GROUP_MAX_CODES: per group code g that has a row, the exhaustive fp64 kernel with
    k = group_size over "code == g AND the user's filter", then the groups ranked on their fp64
    best (score desc, row asc).  Costs one fp64 pass per group, for the given queries only.
      group = (codes int32 [n] on the device, n_codes, n_groups, group_size)
      pass_bits: bool [n] on the device (the user's filter), or None
      exhaustive_masked(q16, k, words) -> (scores f32 [B,k], ids i64 [B,k], exact f64 [B,k]) over
      the rows of the mask `words` (mask_words), ids WITHOUT an id base
    -> (scores, rows, exact) in the padded slot form [B, n_groups * group_size], host numpy."""
    torch = _torch()
    codes, n_codes, n, s = group
    B = q16.shape[0]
    ok = (codes >= 0) & (codes < n_codes)
    if pass_bits is not None:
        ok = ok & pass_bits
    per = []
    for g in torch.unique(codes[ok]).tolist():
        sc, ids, ex = exhaustive_masked(q16, s, mask_words(ok & (codes == g)))
        per.append((sc.cpu().numpy(), ids.cpu().numpy(), ex.cpu().numpy()))
    scores = np.full((B, n * s), -np.inf, dtype=np.float32)
    rows = np.full((B, n * s), -1, dtype=np.int64)
    exact = np.full((B, n * s), -np.inf, dtype=np.float64)
    for b in range(B):
        live = [p for p in per if p[1][b, 0] >= 0]
        live.sort(key=lambda p: (-p[2][b, 0], p[1][b, 0]))
        for j, (sc, ids, ex) in enumerate(live[:n]):
            scores[b, j * s:(j + 1) * s] = sc[b]
            rows[b, j * s:(j + 1) * s] = ids[b]
            exact[b, j * s:(j + 1) * s] = ex[b]
    return scores, rows, exact


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else None


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


class GpuIndex:
    """Thin object wrapper over rf_index_* / rf_search (include/ragfin.h).

    Locking: the index's own workspace (`self.workspace`) is shared by every caller that does not
    bring one.  A method that uses it holds `self._lock` while it enqueues and until the results
    it patches from are read; so do the methods that change the index under a search (compact,
    enable_sq8, disable_sq8).  A method given a caller's workspace does not lock.  The two
    exceptions are `search_raw(workspace=None)` and `enqueue_search`: the benchmark and the
    sharded lanes call them on streams of their own, and the caller serialises.  The lock is not
    re-entrant: public locked methods call the private unlocked ones (`_exhaustive`,
    `_rerun_flagged`), never each other."""

    def __init__(self, dim: int, capacity: int, device=None):
        torch = _torch()
        self.device = require_gpu(device)
        self.lib = _lib.load_library()
        self.dim = int(dim)
        self.capacity = int(capacity)
        nbytes = self.lib.rf_index_storage_bytes(self.dim, self.capacity)
        if nbytes == 0:
            raise _lib.RagfinError(-1, f"unsupported index shape dim={dim} capacity={capacity}")
        with torch.cuda.device(self.device):
            self.storage = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            handle = c_void_p()
            _lib.check(self.lib.rf_index_create(ctypes.byref(handle), self.dim, self.capacity,
                                                c_void_p(self.storage.data_ptr()), nbytes,
                                                self.device.index))
            self.handle = handle
            ws = self.lib.rf_search_workspace_bytes(self.handle)
            # one workspace serves both paths: the SQ8 one is the FLAT one plus its query area
            self.sq8_workspace_bytes = self.lib.rf_search_sq8_workspace_bytes(self.handle)
            # ... and the grouped one is the SQ8 one plus its per-(query, group) tables
            self.grouped_workspace_bytes = self.lib.rf_search_grouped_workspace_bytes(self.handle)
            self.workspace = torch.zeros(max(ws, self.sq8_workspace_bytes, self.grouped_workspace_bytes),
                                         dtype=torch.uint8, device=self.device)
            self.workspace_bytes = ws
        self._lock = threading.Lock()
        self._host_bufs = {}
        self._sq8_storage = None   # the SQ8 shadow (enable_sq8), a separate allocation

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.lib.rf_index_destroy(h)
            self.handle = None

    @property
    def size(self) -> int:
        return int(self.lib.rf_index_size(self.handle))

    def reset(self) -> None:
        torch = _torch()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rf_index_reset(self.handle, _lib.current_stream_ptr()))

    # -- ingest --------------------------------------------------------------
    def add(self, rows) -> None:
        """rows: fp16 [n, dim] tensor on this device (row-major, contiguous)."""
        torch = _torch()
        if rows.dtype != torch.float16 or rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"add expects fp16 [n, {self.dim}], got {rows.dtype} {tuple(rows.shape)}")
        rows = rows.to(self.device).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rf_index_add_f16(self.handle, c_void_p(rows.data_ptr()),
                                                 rows.shape[0], _lib.current_stream_ptr()))

    def to_fp16(self, rows_f32, normalize: bool = True):
        """fp32 [n, dim] -> (L2-normalised) fp16 on device, via rf_normalize_f32_to_f16."""
        torch = _torch()
        x = torch.as_tensor(rows_f32, dtype=torch.float32).to(self.device).contiguous()
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"expected [n, {self.dim}] vectors, got {tuple(x.shape)}")
        out = torch.empty(x.shape, dtype=torch.float16, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rf_normalize_f32_to_f16(c_void_p(x.data_ptr()), x.shape[0], self.dim,
                                                        1 if normalize else 0,
                                                        c_void_p(out.data_ptr()),
                                                        _lib.current_stream_ptr()))
        return out

    COMPACT_WINDOW_ROWS = 1 << 16   # rows per rf_index_compact window (scratch = rows * dim * 2 bytes)

    def compact(self, keep_rows, window_rows: int | None = None) -> None:
        """Keep rows `keep_rows` (strictly ascending row numbers) in that order and drop the rest,
        in place (rf_index_compact): the index then equals a fresh one given the survivors.
        window_rows: rows per compaction window (a multiple of 32; default COMPACT_WINDOW_ROWS).
        Takes the index lock, so it cannot interleave with search / search_host / a page of
        search_large."""
        torch = _torch()
        keep = np.asarray(keep_rows, dtype=np.int64).reshape(-1)
        n = keep.size
        size = self.size
        if n and (keep[0] < 0 or keep[-1] >= size or (n > 1 and bool((np.diff(keep) <= 0).any()))):
            raise ValueError(f"keep_rows must be strictly ascending row numbers in [0, {size})")
        w = self.COMPACT_WINDOW_ROWS if window_rows is None else int(window_rows)
        if w < 32 or w % 32:
            raise ValueError("window_rows must be a positive multiple of 32")
        w = min(w, max(32, (n + 31) // 32 * 32))
        with self._lock, torch.cuda.device(self.device):
            if n == 0:
                _lib.check(self.lib.rf_index_compact(self.handle, None, 0, None, 0, _lib.current_stream_ptr()))
                return
            keep_d = torch.from_numpy(keep).to(self.device)
            scratch = torch.empty(w * self.dim * 2, dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.rf_index_compact(self.handle, c_void_p(keep_d.data_ptr()), n,
                                                 c_void_p(scratch.data_ptr()), scratch.numel(),
                                                 _lib.current_stream_ptr()))
        # keep_d / scratch are released in stream order (caching allocator): no sync needed

    def get_rows(self, row_ids):
        torch = _torch()
        ids = torch.as_tensor(row_ids, dtype=torch.int64).to(self.device).contiguous()
        out = torch.empty((ids.numel(), self.dim), dtype=torch.float16, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rf_index_get_rows_f16(self.handle, c_void_p(ids.data_ptr()),
                                                      ids.numel(), c_void_p(out.data_ptr()),
                                                      _lib.current_stream_ptr()))
        return out

    # -- SQ8 shadow (include/ragfin.h, "SQ8 index") ----------------------------------------
    @property
    def sq8(self) -> bool:
        """True while an int8 shadow is attached (rf_search_sq8 can run)."""
        return self._sq8_storage is not None

    def enable_sq8(self) -> None:
        """Attach an int8 shadow (dim + 8 bytes per row of capacity) and quantize every row; adds,
        compactions and resets keep it current from then on.  Needs dim % 32 == 0."""
        torch = _torch()
        if self._sq8_storage is not None:
            return
        nbytes = self.lib.rf_sq8_storage_bytes(self.dim, self.capacity)
        if nbytes == 0:
            raise _lib.RagfinError(-2, f"SQ8 needs dim % 32 == 0 (dim {self.dim})")
        with self._lock, torch.cuda.device(self.device):
            storage = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.rf_index_attach_sq8(self.handle, c_void_p(storage.data_ptr()), nbytes,
                                                    _lib.current_stream_ptr()))
            self._sq8_storage = storage

    def disable_sq8(self) -> None:
        torch = _torch()
        if self._sq8_storage is None:
            return
        with self._lock, torch.cuda.device(self.device):
            _lib.check(self.lib.rf_index_detach_sq8(self.handle))
            # freed in stream order: a search already enqueued on this stream still reads it
            self._sq8_storage = None

    def get_rows_sq8(self, row_ids):
        """rf_index_get_rows_sq8: (int8 [n, dim], s_r fp32 [n], e_r fp32 [n]) on the device."""
        torch = _torch()
        ids = torch.as_tensor(row_ids, dtype=torch.int64).to(self.device).contiguous()
        n = ids.numel()
        out = torch.empty((n, self.dim), dtype=torch.int8, device=self.device)
        sc = torch.empty((n,), dtype=torch.float32, device=self.device)
        er = torch.empty((n,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rf_index_get_rows_sq8(self.handle, c_void_p(ids.data_ptr()), n,
                                                      c_void_p(out.data_ptr()), c_void_p(sc.data_ptr()),
                                                      c_void_p(er.data_ptr()), _lib.current_stream_ptr()))
        return out, sc, er

    def debug_scores_sq8(self, q16, n: int | None = None):
        """rf_debug_scores_sq8: (a~ fp32 [B, n], delta_q fp32 [B])."""
        torch = _torch()
        n = self.size if n is None else n
        q16 = q16.to(self.device).contiguous()
        B = q16.shape[0]
        out = torch.empty((B, n), dtype=torch.float32, device=self.device)
        delta = torch.empty((B,), dtype=torch.float32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            _lib.check(self.lib.rf_debug_scores_sq8(self.handle, c_void_p(q16.data_ptr()), B, n,
                                                    c_void_p(out.data_ptr()), c_void_p(delta.data_ptr()),
                                                    c_void_p(self.workspace.data_ptr()), self.workspace.numel(),
                                                    _lib.current_stream_ptr()))
        return out, delta

    def search_sq8_profile(self, q16, k: int):
        """rf_search_sq8_profile: per-stage HIP-event times in ms of the first 64-query sweep."""
        return self._profile(self.lib.rf_search_sq8_profile, q16, min(q16.shape[0], _lib.RF_QCHUNK), k,
                             self.workspace.numel(), ("quantize", "sample", "threshold", "emit", "merge"))

    def _profile(self, fn, q16, B: int, k: int, workspace_bytes: int, stages):
        """The first sweep of a B-query batch through a *_profile entry point -> {stage: ms}."""
        torch = _torch()
        q16 = q16.to(self.device).contiguous()
        scores, ids, _, flags = self._outputs(B, k)
        ms = (ctypes.c_float * len(stages))()
        with self._lock, torch.cuda.device(self.device):
            _lib.check(fn(self.handle, _ptr(q16), B, k, 0, _ptr(scores), _ptr(ids), None, _ptr(flags),
                          _ptr(self.workspace), workspace_bytes, _lib.current_stream_ptr(), ms))
        return dict(zip(stages, ms))

    # -- search --------------------------------------------------------------
    def new_workspace(self):
        """An extra search workspace: one per batch in flight when several streams
        search the same (immutable) index concurrently.  Large enough for SQ8 too."""
        torch = _torch()
        return torch.zeros(max(self.workspace_bytes, self.sq8_workspace_bytes, self.grouped_workspace_bytes),
                           dtype=torch.uint8, device=self.device)

    def _outputs(self, B: int, k: int, want_exact: bool = False, flags: bool = True, out=None):
        """The output tuple of a search: `out` when the caller brings one, else fresh device tensors
        (scores f32 [B,k], ids i64 [B,k], exact f64 [B,k] | None, flags i32 [B] | None)."""
        if out is not None:
            return out
        torch = _torch()
        return (torch.empty((B, k), dtype=torch.float32, device=self.device),
                torch.empty((B, k), dtype=torch.int64, device=self.device),
                torch.empty((B, k), dtype=torch.float64, device=self.device) if want_exact else None,
                torch.empty((B,), dtype=torch.int32, device=self.device) if flags else None)

    def search_raw(self, q16, k: int, id_base: int = 0, want_exact: bool = False, out=None,
                   workspace=None, stream_ptr=None, filt=None, sq8: bool = False, band=None, group=None):
        """Enqueue rf_search on the current stream (or on `stream_ptr`, a c_void_p holding a
        hipStream_t of this device); no host sync.  Returns
        (scores f32 [B,k], ids i64 [B,k], exact f64 [B,k] | None, flags u32 [B]).
        filt: a filter buffer built for this index (CorpusStore.build_filter / rf_filter_eval):
        rf_search_filtered, the same outputs over the passing rows only.
        sq8: rf_search_sq8 (needs enable_sq8; not with filt).  A workspace passed in must hold
        sq8_workspace_bytes (new_workspace does).
        band: (radius, range_filter) -- rf_search_range: the best k rows with
        radius < fp64 score <= range_filter (within the passing rows with filt; not with sq8).
        group: (codes int32 [size] on this device, n_codes, n_groups, group_size) -- rf_search_grouped:
        the best n_groups groups of rows sharing a code, each by its best group_size rows (within
        the passing rows with filt; not with sq8 or band).  k must be n_groups * group_size; the
        outputs are in the padded slot form (group of rank j in slots [j s, (j + 1) s)).
        Takes no lock, with or without a workspace of the caller's: the benchmark and the sharded
        lanes call it on their own streams, and whoever shares the index's workspace serialises."""
        torch = _torch()
        if sq8 and (filt is not None or band is not None or group is not None):
            raise ValueError("SQ8 search has no filtered, no range and no grouped form")
        if group is not None:
            if band is not None:
                raise ValueError("grouping search has no range form")
            self._check_group(group, k)
        if q16.dtype != torch.float16 or q16.dim() != 2 or q16.shape[1] != self.dim:
            raise ValueError(f"search expects fp16 [B, {self.dim}] queries")
        if not q16.is_contiguous() or q16.device != self.device:
            q16 = q16.to(self.device).contiguous()
        B = q16.shape[0]
        scores, ids, exact, flags = self._outputs(B, k, want_exact, out=out)
        args = (_ptr(q16), B, k, id_base, _ptr(scores), _ptr(ids), _ptr(exact), _ptr(flags),
                _ptr(workspace if workspace is not None else self.workspace),
                self.grouped_workspace_bytes if group is not None else
                self.sq8_workspace_bytes if sq8 else self.workspace_bytes,
                stream_ptr if stream_ptr is not None else _lib.current_stream_ptr())
        with torch.cuda.device(self.device):
            if group is not None:
                _lib.check(self.lib.rf_search_grouped(self.handle, _ptr(filt), _ptr(group[0]), int(group[1]),
                                                      args[0], B, int(group[2]), int(group[3]), *args[3:]))
            elif band is not None:
                _lib.check(self.lib.rf_search_range(self.handle, _ptr(filt), *args[:4], float(band[0]), float(band[1]),
                                                    *args[4:]))
            elif sq8:
                _lib.check(self.lib.rf_search_sq8(self.handle, *args))
            elif filt is None:
                _lib.check(self.lib.rf_search(self.handle, *args))
            else:
                _lib.check(self.lib.rf_search_filtered(self.handle, _ptr(filt), *args))
        return scores, ids, exact, flags

    def _check_group(self, group, k: int) -> None:
        torch = _torch()
        codes, n_codes, n, s = group
        if not torch.is_tensor(codes) or codes.dtype != torch.int32 or codes.dim() != 1 or \
                codes.numel() != self.size or codes.device != self.device or not codes.is_contiguous():
            raise ValueError(f"group codes must be a contiguous int32 [{self.size}] tensor on {self.device}")
        if n < 1 or s < 1 or n * s > _lib.RF_MAX_K or n * s != k:
            raise ValueError(f"grouping search: need n_groups, group_size >= 1 and k == n_groups * group_size <= "
                             f"{_lib.RF_MAX_K} (got {n}, {s}, k = {k})")

    def search_grouped_profile(self, q16, group, filt=None):
        """rf_search_grouped_profile: per-stage HIP-event times in ms of the first 64-query sweep."""
        torch = _torch()
        q16 = q16.to(self.device).contiguous()
        B = min(q16.shape[0], _lib.RF_QCHUNK)
        k = int(group[2]) * int(group[3])
        self._check_group(group, k)
        scores, ids, _, flags = self._outputs(B, k)
        ms = (ctypes.c_float * 4)()
        with self._lock, torch.cuda.device(self.device):
            _lib.check(self.lib.rf_search_grouped_profile(
                self.handle, _ptr(filt), _ptr(group[0]), int(group[1]), _ptr(q16), B, int(group[2]), int(group[3]), 0,
                _ptr(scores), _ptr(ids), None, _ptr(flags), _ptr(self.workspace), self.grouped_workspace_bytes,
                _lib.current_stream_ptr(), ms))
        return dict(zip(("group_max", "threshold", "emit", "merge"), ms))

    def enqueue_search(self, q_ptr: int, B: int, k: int, id_base: int, scores_ptr: int, ids_ptr: int,
                       exact_ptr: int, flags_ptr: int, workspace_ptr: int, stream_ptr):
        """The bare rf_search enqueue for callers that own every buffer (the sharded step: no
        tensor checks, no allocations, no stream / device context).  The caller guarantees that
        this index's device is the thread's current HIP device, and serialises the use of
        the workspace it passes: no lock is taken here."""
        rc = self.lib.rf_search(self.handle, q_ptr, B, k, id_base, scores_ptr, ids_ptr, exact_ptr, flags_ptr,
                                workspace_ptr, self.workspace_bytes, stream_ptr)
        if rc:
            _lib.check(rc)

    def search_profile(self, q16, k: int):
        """rf_search_profile: per-stage HIP-event times in ms (synchronises)."""
        # the first sweep: 64 queries, or up to 256 on the wide path
        return self._profile(self.lib.rf_search_profile, q16, min(q16.shape[0], 256), k, self.workspace_bytes,
                             ("sample", "threshold", "emit", "merge"))

    def _exhaustive(self, q16, k: int, id_base: int = 0, want_exact: bool = False, filt=None, after=None,
                    band=None):
        """The exhaustive fp64 kernel through whichever entry point the arguments need.  filt: over
        the passing rows.  after: (fp64 scores [B], i64 ids [B]), only the hits ranked strictly after
        that bound per query.  band: (radius, range_filter), only rows inside it
        (rf_search_exhaustive_range).  Uses the index workspace: the caller holds the lock."""
        torch = _torch()
        q16 = q16.to(self.device).contiguous()
        B = q16.shape[0]
        scores, ids, exact, _ = self._outputs(B, k, want_exact, flags=False)
        query = (_ptr(q16), B, k, id_base)
        bounds = (None, None) if after is None else (_ptr(after[0]), _ptr(after[1]))
        outs = (_ptr(scores), _ptr(ids), _ptr(exact), _ptr(self.workspace), self.workspace_bytes,
                _lib.current_stream_ptr())
        with torch.cuda.device(self.device):
            if band is not None:
                rc = self.lib.rf_search_exhaustive_range(self.handle, _ptr(filt), *query, float(band[0]),
                                                         float(band[1]), *bounds, *outs)
            elif filt is not None:
                rc = self.lib.rf_search_exhaustive_filtered(self.handle, _ptr(filt), *query, *bounds, *outs)
            elif after is not None:
                rc = self.lib.rf_search_exhaustive_after(self.handle, *query, *bounds, *outs)
            else:
                rc = self.lib.rf_search_exhaustive(self.handle, *query, *outs)
        _lib.check(rc)
        return scores, ids, exact

    def search_exhaustive(self, q16, k: int, id_base: int = 0, want_exact: bool = False, filt=None, band=None):
        with self._lock:
            return self._exhaustive(q16, k, id_base, want_exact, filt, band=band)

    def search_large(self, q16, k: int, id_base: int = 0, want_exact: bool = False, filt=None, band=None):
        """Limits above RF_MAX_K: the first page through the fused path, further pages
        of RF_MAX_K through the exhaustive kernel with a bound (each page = the hits ranked
        strictly after the previous page's last hit).  Returns (scores, ids) [B, k]
        (+ the fp64 ranking scores with want_exact: what a cross-shard merge ranks by).
        filt: the same over the passing rows.  band: (radius, range_filter) -- the same within the
        band: the first page through rf_search_range, later pages through the exhaustive band
        kernel; the walk ends with the first page that the band does not fill."""
        torch = _torch()
        q16 = q16.to(self.device).contiguous()
        B = q16.shape[0]
        page = _lib.RF_MAX_K
        s0, i0, e0 = self.search(q16, page, id_base, want_exact=True, filt=filt, band=band)
        scores, ids, exacts = [s0], [i0], [e0]
        last_s, last_i = e0[:, -1].contiguous(), i0[:, -1].contiguous()
        got = page
        while got < k and bool((last_i >= 0).any()):
            # exhausted queries keep a bound nothing can follow
            bs = torch.where(last_i >= 0, last_s, torch.full_like(last_s, float("-inf")))
            bi = torch.where(last_i >= 0, last_i, torch.full_like(last_i, 2 ** 62))
            with self._lock:
                s, i, e = self._exhaustive(q16, page, id_base, True, filt, after=(bs, bi), band=band)
            scores.append(s)
            ids.append(i)
            exacts.append(e)
            last_s, last_i = e[:, -1].contiguous(), i[:, -1].contiguous()
            got += page
        if got < k:   # corpus exhausted before k hits: pad like rf_search does
            scores.append(torch.full((B, k - got), float("-inf"), dtype=torch.float32, device=self.device))
            ids.append(torch.full((B, k - got), -1, dtype=torch.int64, device=self.device))
            exacts.append(torch.full((B, k - got), float("-inf"), dtype=torch.float64, device=self.device))
        out = (torch.cat(scores, 1)[:, :k].contiguous(), torch.cat(ids, 1)[:, :k].contiguous())
        return out + (torch.cat(exacts, 1)[:, :k].contiguous(),) if want_exact else out

    def _grouped_exhaustive(self, q16, group, id_base: int, want_exact: bool, filt):
        """grouped_exhaustive with this index's exhaustive kernel -> device tensors.  The caller
        holds the lock."""
        torch = _torch()
        n_rows = self.size
        nblk = (n_rows + 31) // 32
        bits = None if filt is None else words_mask(filt[16:16 + 4 * nblk].view(torch.int32), n_rows)

        def masked(q, k, words):
            buf = torch.empty(self.lib.rf_filter_bytes(n_rows), dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.rf_filter_from_mask(_ptr(words), n_rows, _ptr(buf), _lib.current_stream_ptr()))
            return self._exhaustive(q, k, 0, True, buf)

        scores, rows, exact = grouped_exhaustive(q16.to(self.device).contiguous(), group, bits, masked)
        rows = np.where(rows >= 0, rows + id_base, rows)
        return (torch.from_numpy(scores).to(self.device), torch.from_numpy(rows).to(self.device),
                torch.from_numpy(exact).to(self.device) if want_exact else None)

    def _rerun_flagged(self, q16, k: int, id_base: int, want_exact: bool, flags, sq8: bool, filt, band=None,
                       group=None):
        """rerun_flagged with this index's tiers (the band of a range search rides in them; a
        grouping search re-runs group by group).  The caller holds the lock."""
        if group is not None:
            return rerun_flagged(q16, k, id_base, flags, False, filt, None,
                                 lambda q, k, base, f: self._grouped_exhaustive(q, group, base, want_exact, f))
        return rerun_flagged(q16, k, id_base, flags, sq8, filt,
                             lambda q, k, base: self.search_raw(q, k, base, want_exact, band=band),
                             lambda q, k, base, f: self._exhaustive(q, k, base, want_exact, f, band=band))

    def _grouped_first_pass(self, q16, k: int, id_base: int, want_exact: bool, filt, group, out=None):
        """search_raw(group=...), or -- a dictionary above RF_GROUP_MAX_CODES -- outputs whose every
        query is flagged, so that the ladder answers the whole batch."""
        if int(group[1]) <= _lib.RF_GROUP_MAX_CODES:
            return self.search_raw(q16, k, id_base, want_exact, out=out, filt=filt, group=group)
        self._check_group(group, k)
        res = self._outputs(q16.shape[0], k, want_exact, out=out)
        res[3].fill_(_lib.RF_FLAG_CAND_OVERFLOW)
        return res

    def search(self, q16, k: int, id_base: int = 0, want_exact: bool = False, filt=None, sq8: bool = False,
               band=None, group=None):
        """rf_search, then the flagged-query ladder (rerun_flagged) for any query the fused path
        could not prove exact.  filt: over the passing rows.  sq8: rf_search_sq8 first.
        band: (radius, range_filter) -- rf_search_range, flagged queries through the exhaustive
        band kernel.  group: as in search_raw -- rf_search_grouped, flagged queries (and every query
        of a dictionary above RF_GROUP_MAX_CODES) group by group through the exhaustive kernel."""
        with self._lock:
            if group is not None:
                if sq8 or band is not None:
                    raise ValueError("grouping search has no SQ8 and no range form")
                scores, ids, exact, flags = self._grouped_first_pass(q16, k, id_base, want_exact, filt, group)
            else:
                scores, ids, exact, flags = self.search_raw(q16, k, id_base, want_exact, filt=filt, sq8=sq8, band=band)
            bad, rows = self._rerun_flagged(q16, k, id_base, want_exact, flags, sq8, filt, band, group)
            if rows is not None:
                for dst, src in zip((scores, ids, exact), rows):
                    if dst is not None:
                        dst[bad] = src
        return scores, ids, exact

    ZERO_COPY_MAX = 4096   # B * k up to which search_host lets the kernel write into host memory

    def search_host(self, q16, k: int, filt=None, sq8: bool = False, band=None, group=None):
        """search() whose results land on the host with ONE synchronisation: scores, ids and
        flags are copied into cached pinned buffers asynchronously.  -> (scores f32 [B,k],
        ids i64 [B,k]) numpy arrays (the caller's own copies).  filt: over the passing rows.
        sq8: rf_search_sq8 first, as in search().  band: (radius, range_filter), as in search().
        group: as in search(); k = n_groups * group_size, the padded slot form."""
        torch = _torch()
        if group is not None:
            if sq8 or band is not None:
                raise ValueError("grouping search has no SQ8 and no range form")
            with self._lock:
                scores, ids, _, flags = self._grouped_first_pass(q16, k, 0, False, filt, group)
                bad, rows = self._rerun_flagged(q16, k, 0, False, flags, False, filt, None, group)
                if rows is not None:
                    scores[bad] = rows[0]
                    ids[bad] = rows[1]
                return scores.cpu().numpy(), ids.cpu().numpy()
        with self._lock:
            B = q16.shape[0]
            key = (B, k)
            bufs = self._host_bufs.get(key)
            if bufs is None:
                bufs = self._host_bufs[key] = (torch.empty((B, k), dtype=torch.float32, pin_memory=True),
                                               torch.empty((B, k), dtype=torch.int64, pin_memory=True),
                                               torch.empty((B,), dtype=torch.int32, pin_memory=True))
            if B * k <= self.ZERO_COPY_MAX and _ZERO_COPY:
                # query-sized results: the merge kernel stores straight into the pinned host buffers
                # (host-coherent memory, mapped at the same address on the device) -- no copy commands,
                # only the synchronisation
                self.search_raw(q16, k, out=(bufs[0], bufs[1], None, bufs[2]), filt=filt, sq8=sq8, band=band)
            else:
                scores, ids, _, flags = self.search_raw(q16, k, filt=filt, sq8=sq8, band=band)
                bufs[0].copy_(scores, non_blocking=True)
                bufs[1].copy_(ids, non_blocking=True)
                bufs[2].copy_(flags, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            if bool(bufs[2].any()):
                bad, rows = self._rerun_flagged(q16, k, 0, False, bufs[2], sq8, filt, band)
                bufs[0][bad] = rows[0].cpu()
                bufs[1][bad] = rows[1].cpu()
            # private copies, taken while the lock is still held: the pinned buffers are shared by every caller with
            # this (B, k) and the next search's merge kernel stores straight into them
            return bufs[0].numpy().copy(), bufs[1].numpy().copy()

    def debug_scores(self, q16, n: int | None = None):
        torch = _torch()
        n = self.size if n is None else n
        q16 = q16.to(self.device).contiguous()
        out = torch.empty((q16.shape[0], n), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rf_debug_scores(self.handle, c_void_p(q16.data_ptr()), q16.shape[0], n,
                                                c_void_p(out.data_ptr()), _lib.current_stream_ptr()))
        return out


def eval_filter(device, program: "filter_expr.Program", columns, n_rows: int):
    """rf_filter_eval of a compiled program into a fresh filter buffer (uint8 device tensor of
    rf_filter_bytes(n_rows)), enqueued on the current stream.  columns: the device tensors
    {period, chunk_type, statement_type codes int32 [n_rows], primary_value fp64 [n_rows]}."""
    torch = _torch()
    lib = _lib.load_library()
    cs, rl = filter_expr.program_arrays(program)
    with torch.cuda.device(device):
        buf = torch.empty(lib.rf_filter_bytes(n_rows), dtype=torch.uint8, device=device)
        cs_d = torch.from_numpy(cs.view(np.int32)).to(device) if cs.size else None
        rl_d = torch.from_numpy(rl.view(np.int32)).to(device) if rl.size else None
        ptrs = (c_void_p * _lib.RF_FILTER_COLUMNS)(*[c_void_p(t.data_ptr()) if t is not None and t.numel() else None
                                                     for t in columns])
        ops = program.ops_ctypes()
        _lib.check(lib.rf_filter_eval(ops, len(ops), c_void_p(cs_d.data_ptr()) if cs_d is not None else None,
                                      c_void_p(rl_d.data_ptr()) if rl_d is not None else None, ptrs, n_rows,
                                      c_void_p(buf.data_ptr()), _lib.current_stream_ptr()))
    # (cs_d / rl_d may be freed now: the caching allocator reuses their memory in stream order)
    return buf


def filter_mask_bits(buf, n_rows: int):
    """The row mask of a filter buffer as a host bool array [n_rows] (synchronises)."""
    nblk = (n_rows + 31) // 32
    words = buf[16:16 + 4 * nblk].cpu().numpy().view(np.uint32)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    return bits[:n_rows]


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


_ID_IN = re.compile(r"^\s*id\s+in\s+\[(.*)\]\s*$", re.S)


class CorpusStore:
    """Drop-in for the reference's `Collection("fin_chunks")` on this path."""

    def __init__(self, name: str = "fin_chunks", dim: int = 384, capacity: int = 4096,
                 device=None, metric_type: str = "COSINE", index=None):
        self.name = name
        self.dim = dim
        self.metric_type = metric_type.upper()
        if self.metric_type not in ("COSINE", "IP"):
            raise ValueError("metric_type must be COSINE or IP")
        # `index`: an already-built GpuIndex (tests of the sharded store pass a CPU double)
        self.index = index if index is not None else GpuIndex(dim, capacity, device)
        self.columns: dict[str, list] = {f: [] for f in SCALAR_FIELDS}
        self._pk_row: dict[Any, int] = {}
        self._dcols = None                  # _DeviceColumns, built by the first filtered call
        self._filter_lock = threading.Lock()
        # search / query / save read; add / delete / upsert / drop write.  A search hands out row
        # numbers and then reads the host columns at those rows (search_large over several pages):
        # a delete in between would pin another row's entity on a hit.
        self._rw = _RWLock()
        self.index_type = "FLAT"            # create_index: "FLAT" (IVF_FLAT is served as FLAT) or "SQ8"
        self._index_params = None           # what create_index was given (None: no create_index call)

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
            self.index.reset()
            for col in self.columns.values():
                col.clear()
            self._pk_row.clear()
            self._dcols = None

    @property
    def num_entities(self) -> int:
        return len(self.columns["id"])

    def _grow(self, need: int) -> None:
        old = self.index
        cap = max(need, old.capacity * 2)
        new = type(old)(self.dim, cap, old.device)
        n = old.size
        step = 1 << 18
        for s in range(0, n, step):
            new.add(old.get_rows(np.arange(s, min(n, s + step), dtype=np.int64)))
        if getattr(old, "sq8", False):
            new.enable_sq8()   # re-attach: quantizes the copied rows
        self.index = new

    # -- index type: Collection.create_index / drop_index / has_index --------------------------
    INDEX_TYPES = ("FLAT", "IVF_FLAT", "SQ8")

    def create_index(self, field_name: str, index_params: dict | None = None, **kwargs) -> None:
        """pymilvus-shaped create_index ("chunking_storing (1).py":29).  index_type "FLAT" (the
        default), "IVF_FLAT" (served as FLAT: exact, `params` such as nlist are ignored) or "SQ8"
        (an int8 shadow of the vectors: fewer bytes per search, same exact answers; dim % 32 == 0).
        Any other type, a metric_type other than the collection's or a field other than
        "embedding" raises ValueError."""
        params = dict(index_params or {})
        itype, metric = self._check_index_params(field_name, params)
        with self._rw.write():
            if itype == "SQ8":
                self.index.enable_sq8()
            elif getattr(self.index, "sq8", False):
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

    def drop_index(self, **kwargs) -> None:
        """Back to FLAT (the shadow of SQ8 is freed)."""
        with self._rw.write():
            if getattr(self.index, "sq8", False):
                self.index.disable_sq8()
            self.index_type = "FLAT"
            self._index_params = None

    def has_index(self, **kwargs) -> bool:
        return self._index_params is not None

    def _use_sq8(self, B: int, limit: int, band=None) -> bool:
        # the routing rule: unfiltered, no range parameters, limit <= RF_MAX_K,
        # B <= one 64-query sweep
        return self.index_type == "SQ8" and band is None and limit <= _lib.RF_MAX_K and B <= _lib.RF_QCHUNK

    # -- ingest ------------------------------------------------------------------
    def add(self, ids: Sequence, texts: Sequence[str], embeddings, periods: Sequence[str],
            chunk_types: Sequence[str], statement_types: Sequence[str],
            primary_values: Sequence[float]) -> int:
        with self._rw.write():
            return self._add(ids, texts, embeddings, periods, chunk_types, statement_types, primary_values)

    def _add(self, ids, texts, embeddings, periods, chunk_types, statement_types, primary_values) -> int:
        torch = _torch()
        n = len(ids)
        cols = (texts, periods, chunk_types, statement_types, primary_values)
        if any(len(c) != n for c in cols):
            raise ValueError("insert columns differ in length")
        if torch.is_tensor(embeddings) and embeddings.dtype == torch.float16:
            vec = embeddings  # already normalised fp16 (embedder output)
            if vec.shape != (n, self.dim):
                raise ValueError(f"embeddings must be [{n}, {self.dim}]")
        else:
            emb = np.asarray(embeddings, dtype=np.float32) if not torch.is_tensor(embeddings) else embeddings
            if tuple(emb.shape) != (n, self.dim):
                raise ValueError(f"embeddings must be [{n}, {self.dim}], got {tuple(emb.shape)}")
            vec = self.index.to_fp16(emb, normalize=self.metric_type == "COSINE")
        for pk in ids:
            if pk in self._pk_row:
                raise ValueError(f"duplicate primary key {pk!r}")
        if len(set(ids)) != n:
            raise ValueError("duplicate primary keys in insert")
        if self.index.size + n > self.index.capacity:
            self._grow(self.index.size + n)
        base = self.index.size
        self.index.add(vec)
        for j, pk in enumerate(ids):
            self._pk_row[pk] = base + j
        self.columns["id"].extend(ids)
        self.columns["text"].extend(texts)
        self.columns["period"].extend(periods)
        self.columns["chunk_type"].extend(chunk_types)
        self.columns["statement_type"].extend(statement_types)
        self.columns["primary_value"].extend(float(v) for v in primary_values)
        return n

    def insert(self, data: Sequence[Sequence]) -> int:
        """Column-major insert in the reference's order
        [id, text, embedding, period, chunk_type, statement_type, primary_value]."""
        if len(data) != 7:
            raise ValueError("insert expects 7 columns: id, text, embedding, period, chunk_type, "
                             "statement_type, primary_value")
        ids, texts, emb, periods, ctypes_, stypes, pvals = data
        return self.add(ids, texts, emb, periods, ctypes_, stypes, pvals)

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
        if len(data) != 7:
            raise ValueError("upsert expects 7 columns: id, text, embedding, period, chunk_type, "
                             "statement_type, primary_value")
        ids, texts, emb, periods, ctypes_, stypes, pvals = data
        ids = list(ids)
        with self._rw.write():
            emb = self._check_upsert(ids, (texts, periods, ctypes_, stypes, pvals), emb)
            self._delete_mask(self._pk_mask(ids))
            n = self.add(ids, texts, emb, periods, ctypes_, stypes, pvals)
            return MutationResult(ids, insert_count=n, upsert_count=n)

    def _check_upsert(self, ids, cols, emb):
        """Everything add() would refuse, checked BEFORE the old rows go; returns the batch's
        vectors as the fp16 rows add() stores."""
        torch = _torch()
        n = len(ids)
        if any(len(c) != n for c in cols):
            raise ValueError("upsert columns differ in length")
        if len(set(ids)) != n:
            raise ValueError("duplicate primary keys in upsert")
        if torch.is_tensor(emb) and emb.dtype == torch.float16:
            if tuple(emb.shape) != (n, self.dim):
                raise ValueError(f"embeddings must be [{n}, {self.dim}]")
            return emb
        e = np.asarray(emb, dtype=np.float32) if not torch.is_tensor(emb) else emb
        if tuple(e.shape) != (n, self.dim):
            raise ValueError(f"embeddings must be [{n}, {self.dim}], got {tuple(e.shape)}")
        return self.index.to_fp16(e, normalize=self.metric_type == "COSINE")

    def _match_mask(self, expr: str) -> np.ndarray:
        """bool [num_entities]: the rows `expr` matches, evaluated on the device."""
        n = self.num_entities
        if n == 0:
            with self._filter_lock:   # still reject a bad expression
                filter_expr.compile_expr(filter_expr.parse(expr), {f: [] for f in filter_expr.VARCHAR_FIELDS}, {})
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
        self._compact_index(keep_mask, keep)
        sel = keep_mask.tolist()
        for f in SCALAR_FIELDS:
            self.columns[f] = list(itertools.compress(self.columns[f], sel))
        self._pk_row = dict(zip(self.columns["id"], range(keep.size)))
        with self._filter_lock:
            if self._dcols is not None:
                if self._dcols.n == n_old:
                    self._dcols.compact(keep)
                else:   # not synced to the old rows: the next filtered call re-encodes from row 0
                    self._dcols = None
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

    def search_rows(self, data, limit: int, filt=None, band=None):
        """(scores f32 [B,k'], rows i64 [B,k']) as host numpy, k' = min(limit, N).  filt: a
        filter buffer (build_filter): the top-k of the passing rows, padded with -1 rows.
        band: (radius, range_filter) -- range search: the top-k of the rows with
        radius < fp64 score <= range_filter, padded with -1 rows."""
        if limit < 1:
            raise ValueError("limit must be >= 1")
        if band is not None:
            band = check_band(*band)
        with self._rw.read():
            return self._search_rows(data, limit, filt, band)

    GROUP_BY_FIELDS = filter_expr.VARCHAR_FIELDS   # period, chunk_type, statement_type ("id": the plain search)

    def _group_codes(self, field: str):
        """(codes int32 [n] on the device, n_codes) of a group-by field, from the device mirror."""
        with self._filter_lock:
            if self._dcols is None:
                self._dcols = _DeviceColumns(self.index.device)
            self._dcols.sync(self.columns, self.num_entities)
            return self._dcols.codes[field].contiguous(), len(self._dcols.dicts[field])

    def _search_rows(self, data, limit: int, filt=None, band=None, group=None):
        q16 = self._prepare_queries(data)
        if group is not None:
            # (field, group_size): the padded [B, limit * group_size] block; never SQ8, never paged
            field, gsize = group
            kw = {} if filt is None else {"filt": filt}
            codes, n_codes = self._group_codes(field)
            return self.index.search_host(q16, limit * gsize, group=(codes, n_codes, limit, gsize), **kw)
        kw = {} if filt is None else {"filt": filt}
        if band is not None:
            kw["band"] = band
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
               group_by_field: str | None = None, group_size: int = 1, strict_group_size: bool = False):
        """pymilvus-shaped search: one list of hits per query vector, best first.
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
        radius >= range_filter raises ValueError.  Other keys of params (nprobe, ...) are ignored."""
        with self._rw.read():   # the rows handed back are marshalled below: no delete in between
            if group_by_field is None:
                return self._search(data, anns_field, param, limit, expr, output_fields)
            return self._search(data, anns_field, param, limit, expr, output_fields,
                                self._check_group_by(group_by_field, group_size, limit, param))

    def _check_group_by(self, field, group_size, limit, param):
        """-> (field, group_size), or None for "id" (every row its own group: the plain search)."""
        if field != "id" and field not in self.GROUP_BY_FIELDS:
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

    def _search(self, data, anns_field, param, limit, expr, output_fields, group=None):
        if anns_field != "embedding":
            raise ValueError(f"unknown vector field {anns_field!r}")
        metric = (param or {}).get("metric_type", self.metric_type).upper()
        if metric != self.metric_type:
            raise ValueError(f"collection was built for {self.metric_type}, search asked for {metric}")
        fields = list(output_fields or [])
        for f in fields:
            if f not in self.columns:
                raise KeyError(f"unknown output field {f!r}")
        band = self._band_of(param)
        kw = {} if band is None else {"band": band}
        if group is not None:
            # the padded [B, limit * group_size] block; short and missing groups leave -1 slots
            filt = None if filter_expr.is_empty(expr) else self.build_filter(expr)
            scores, rows = self._search_rows(data, limit, filt, group=group)
            if group[0] not in fields:
                fields = fields + [group[0]]
        elif filter_expr.is_empty(expr):
            scores, rows = self.search_rows(data, limit, **kw)
        else:
            scores, rows = self.search_rows(data, limit, filt=self.build_filter(expr), **kw)
        out = []
        for b in range(rows.shape[0]):
            hits = []
            for j in range(rows.shape[1]):
                r = int(rows[b, j])
                if r < 0:
                    if group is not None:
                        continue
                    break
                hits.append(Hit(r, self.columns["id"][r], float(scores[b, j]),
                                {f: self.columns[f][r] for f in fields}))
            out.append(hits)
        return out

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
        import json
        import os
        os.makedirs(path, exist_ok=True)
        n = self.num_entities
        tmp = os.path.join(path, "vectors.f16.tmp")
        with open(tmp, "wb") as f:
            for s0 in range(0, n, chunk_rows):
                rows = np.arange(s0, min(n, s0 + chunk_rows), dtype=np.int64)
                f.write(self.index.get_rows(rows).cpu().numpy().tobytes())
        os.replace(tmp, os.path.join(path, "vectors.f16"))
        meta = {"format": "ragfin-corpus-v1", "name": self.name, "dim": self.dim,
                "metric_type": self.metric_type, "n": n, "columns": self.columns}
        if self.index_type != "FLAT":   # FLAT directories stay exactly as before
            meta["index_type"] = self.index_type
        tmp = os.path.join(path, "columns.json.tmp")
        with open(tmp, "w", encoding="utf-8") as f:
            json.dump(meta, f, ensure_ascii=False)
        os.replace(tmp, os.path.join(path, "columns.json"))

    @classmethod
    def load_from(cls, path: str, device=None, capacity: int | None = None,
                  chunk_rows: int = 1 << 18) -> "CorpusStore":
        """Memory-map vectors.f16 and stream it into HBM in chunks (never the whole file
        in host RAM)."""
        import json
        import os
        torch = _torch()
        with open(os.path.join(path, "columns.json"), encoding="utf-8") as f:
            meta = json.load(f)
        if meta.get("format") != "ragfin-corpus-v1":
            raise ValueError(f"{path}: not a ragfin corpus directory")
        n, dim = int(meta["n"]), int(meta["dim"])
        st = cls(meta["name"], dim=dim, capacity=max(capacity or 0, n, 1), device=device,
                 metric_type=meta["metric_type"])
        if n:
            expect = n * dim * 2
            got = os.path.getsize(os.path.join(path, "vectors.f16"))
            if got != expect:
                raise ValueError(f"{path}/vectors.f16 holds {got} bytes, expected {expect}")
            mm = np.memmap(os.path.join(path, "vectors.f16"), dtype=np.float16, mode="r", shape=(n, dim))
            for s0 in range(0, n, chunk_rows):
                st.index.add(torch.from_numpy(np.ascontiguousarray(mm[s0:s0 + chunk_rows])).to(st.index.device))
            del mm
        cols = meta["columns"]
        if any(len(cols[f]) != n for f in SCALAR_FIELDS):
            raise ValueError(f"{path}: column lengths do not match n={n}")
        st.columns = {f: list(cols[f]) for f in SCALAR_FIELDS}
        st._pk_row = {pk: i for i, pk in enumerate(st.columns["id"])}
        itype = meta.get("index_type", "FLAT")   # a missing key means FLAT
        if itype != "FLAT":
            st.create_index("embedding", {"index_type": itype, "metric_type": st.metric_type})
        return st

    # -- filters -------------------------------------------------------------------------
    def build_filter(self, expr: str):
        """Parse + compile `expr` (rag_fin_amd.filter_expr; ValueError on a bad expression) and
        evaluate it on the device into a fresh filter buffer for this collection's rows.  One
        buffer per call: concurrent searches with different filters do not share one."""
        node = filter_expr.parse(expr)
        with self._filter_lock:
            n = self.num_entities
            if self._dcols is None:
                self._dcols = _DeviceColumns(self.index.device)
            self._dcols.sync(self.columns, n)
            prog = filter_expr.compile_expr(node, self._dcols.dicts, self._pk_row)
            return eval_filter(self.index.device, prog, self._dcols.tensors(), n)

    def filter_rows(self, expr: str) -> np.ndarray:
        """Row numbers (ascending) that pass `expr`."""
        return np.flatnonzero(filter_mask_bits(self.build_filter(expr), self.num_entities))

    # -- scalar queries ----------------------------------------------------------------
    def query(self, expr: str = "", limit: int | None = None,
              output_fields: Iterable[str] | None = None) -> list[dict]:
        """`query(expr="id in [...]")` fetch-by-PK (key order), `query(expr="", limit=n)` scan, and
        any other filter expression (rag_fin_amd.filter_expr): the matching rows in ascending
        row order."""
        with self._rw.read():
            return self._query(expr, limit, output_fields)

    def _query(self, expr, limit, output_fields) -> list[dict]:
        fields = list(output_fields or ["id"])
        want_vec = "embedding" in fields
        fields = [f for f in fields if f != "embedding"]
        for f in fields:
            if f not in self.columns:
                raise KeyError(f"unknown output field {f!r}")
        if expr is None or expr.strip() == "":
            rows = list(range(self.num_entities))
        else:
            keys = _id_in_keys(expr)
            if keys is not None:
                rows = [self._pk_row[k] for k in keys if k in self._pk_row]
            else:
                rows = self._expr_rows(expr).tolist()
        if limit is not None:
            rows = rows[:limit]
        vecs = self.index.get_rows(np.asarray(rows, dtype=np.int64)).float().cpu().numpy() \
            if (want_vec and rows) else None
        out = []
        for j, r in enumerate(rows):
            rec = {f: self.columns[f][r] for f in fields}
            if "id" not in rec:
                rec["id"] = self.columns["id"][r]
            if vecs is not None:
                rec["embedding"] = vecs[j].tolist()
            out.append(rec)
        return out

    def _expr_rows(self, expr: str) -> np.ndarray:
        return self.filter_rows(expr)


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
