"""The device layer under rag_fin_amd/store.py (which re-exports these names): `GpuIndex` over
rf_index_* / rf_search (include/ragfin.h), the flagged-query ladder, the filter-mask helpers and
rf_filter_eval; `SparseIndex` over rf_sparse_* (BM25 posting lists), `fuse_rrf` over rf_fuse_rrf, and
`boost_classes` / `merge_boosted` over rf_boost_classes / rf_merge_boosted (boosted search), and
`decay_weights` over rf_decay_weights (decayed search; the sweep itself is `GpuIndex.search(weights=)`).
All arithmetic goes through libragfin_hip.so; there is no CPU path."""
from __future__ import annotations

import ctypes
import os as _os
import threading
from ctypes import c_void_p

import numpy as np

from . import _lib
from . import filter_expr


# RAGFIN_ZERO_COPY=0: search_host copies results with async memcpys instead of letting the merge kernel
# store into the pinned host buffers (A/B switch)
_ZERO_COPY = _os.environ.get("RAGFIN_ZERO_COPY", "1") != "0"


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
    exact (flags != 0) is re-run one tier down.  A query flagged by a first pass over the int8 shadow
    (`sq8`: rf_search_sq8, or rf_search on a shadow-first index) goes through the fp16 chain
    (`flat`: rf_search_fp16), and only one that flags there too goes to the exhaustive kernel; one
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


MULTI_MAX_FILTERS = 64   # filters one multi-filter buffer holds (include/ragfin.h, "per-query filters")


class MultiFilter:
    """The per-query filters of one batch (include/ragfin.h, "per-query filters"): G <= 64 filter
    buffers built for the same rows, the multi-filter buffer over them (their union in the filter
    buffer format, then their masks block-major) and, per query of the batch, the number of its
    filter.  `GpuIndex.search_raw / search / search_host(..., filt=MultiFilter)` sweeps the union's
    blocks once for the whole batch, each query over its own rows; a flagged query goes down the
    ladder with its own filter buffer."""

    def __init__(self, filters, qfilter, n_rows: int, device):
        torch = _torch()
        lib = _lib.load_library()
        self.filters = list(filters)
        G = len(self.filters)
        if not 1 <= G <= MULTI_MAX_FILTERS:
            raise ValueError(f"per-query filters: a batch holds 1..{MULTI_MAX_FILTERS} distinct filters, got {G}")
        self.qfilter_host = np.asarray(qfilter, dtype=np.int32).reshape(-1)
        if self.qfilter_host.size == 0 or int(self.qfilter_host.min()) < 0 or int(self.qfilter_host.max()) >= G:
            raise ValueError(f"per-query filters: need one filter number in [0, {G}) per query")
        self.n_rows = int(n_rows)
        nbytes = lib.rf_multi_filter_bytes(self.n_rows, G)
        if nbytes == 0:
            raise ValueError(f"per-query filters: no buffer for {n_rows} rows and {G} filters")
        with torch.cuda.device(device):
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self.qfilter = torch.from_numpy(self.qfilter_host).to(device)
            ptrs = (c_void_p * G)(*[c_void_p(f.data_ptr()) for f in self.filters])
            _lib.check(lib.rf_multi_filter_build(ptrs, G, self.n_rows, _ptr(self.buf), _lib.current_stream_ptr()))

    def __len__(self) -> int:
        return len(self.filters)


def plan_filter_chunks(qfilter, chunk: int = _lib.RF_QCHUNK):
    """Queries with a filter number each -> the sweeps that serve them: the queries ordered by
    filter number (stable), cut into chunks of `chunk`, so that a chunk's union holds as few
    filters as the order allows.  -> [(query indices int64 [nb], their filters' numbers, ascending
    and distinct, the position of each query's filter in that list int32 [nb])]."""
    qf = np.asarray(qfilter, dtype=np.int64).reshape(-1)
    order = np.argsort(qf, kind="stable")
    out = []
    for lo in range(0, order.size, chunk):
        idx = order[lo:lo + chunk]
        distinct, local = np.unique(qf[idx], return_inverse=True)
        out.append((idx, distinct.tolist(), local.astype(np.int32)))
    return out


class GpuIndex:
    """Thin object wrapper over rf_index_* / rf_search (include/ragfin.h).

    Locking: the index's own workspace (`self.workspace`) is shared by every caller that does not
    bring one.  A method that uses it holds `self._lock` while it enqueues and until the results
    it patches from are read; so do the methods that change the index under a search (compact,
    enable_sq8, disable_sq8).  A method given a caller's workspace does not lock.  The two
    exceptions are `search_raw(workspace=None)` and `enqueue_search`: the benchmark and the
    sharded lanes call them on streams of their own, and the caller serialises.  The lock is not
    re-entrant: public locked methods call the private unlocked ones (`_exhaustive`,
    `_rerun_flagged`), never each other.

    shadow: the int8 shadow behind plain searches.  "auto" attaches one and lets
    rf_search sweep it first when capacity >= SHADOW_MIN_ROWS and dim % 32 == 0; True forces it for
    any capacity (dim % 32 == 0 still, else RagfinError); False never attaches.  The shadow costs
    dim + 8 bytes per row of capacity next to the 2 dim of the fp16 rows (+51 % at dim 384).  The
    answers do not depend on it.  `.sq8` stays "the caller enabled SQ8" (enable_sq8 reuses an
    auto-attached shadow, disable_sq8 keeps it)."""

    # Rows of capacity from which "auto" takes the shadow first (None would switch "auto" off).  Measured with
    # bench.py --rows N, shadow forced (tools/bench_shadow_rows.py lowers this attribute for one run), against
    # the parent commit (profiles/flat_shadow_min_rows.json, DESIGN
    # §5.0s): the int8 chain loses at 100 k and 250 k rows (two more launches on a launch-bound step), wins
    # 3 % at 500 k, 6 % at 2^19 and a third at 1 M; 2^19 is 500 k rounded to a power of two.
    SHADOW_MIN_ROWS = 1 << 19
    shadow_first = False      # rf_search sweeps the shadow first on this index (set by the constructor)
    _shadow_min_rows = 0
    _sq8_storage = None
    _sq8_enabled = False

    def __init__(self, dim: int, capacity: int, device=None, shadow="auto"):
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
            self._lock = threading.Lock()
            self._sq8_storage = None   # the int8 shadow: a separate allocation
            self._sq8_enabled = False  # enable_sq8 was called (the shadow may be there without it)
            if isinstance(shadow, np.bool_):
                shadow = bool(shadow)
            if not (isinstance(shadow, bool) or (isinstance(shadow, str) and shadow == "auto")):   # (1 == True: no ints)
                raise ValueError(f"shadow must be 'auto', True or False, got {shadow!r}")
            self.shadow = shadow       # as asked for: what a store passes on when it rebuilds the index
            self.shadow_first = shadow is True or (shadow == "auto" and self.SHADOW_MIN_ROWS is not None
                                                   and self.capacity >= self.SHADOW_MIN_ROWS and self.dim % 32 == 0)
            # rows from which the library takes the shadow chain (rf_index_set_shadow_first); 0: never
            self._shadow_min_rows = 0 if not self.shadow_first else 1 if shadow is True else int(self.SHADOW_MIN_ROWS)
            if self.shadow_first:   # before workspace_bytes is read: it then covers the SQ8 query area
                self._attach_shadow()
                _lib.check(self.lib.rf_index_set_shadow_first(self.handle, self._shadow_min_rows))
            ws = self.lib.rf_search_workspace_bytes(self.handle)
            # one workspace serves both paths: the SQ8 one is the FLAT one plus its query area
            self.sq8_workspace_bytes = self.lib.rf_search_sq8_workspace_bytes(self.handle)
            # ... and the grouped one is the SQ8 one plus its per-(query, group) tables
            self.grouped_workspace_bytes = self.lib.rf_search_grouped_workspace_bytes(self.handle)
            self.workspace_bytes = ws
            self._alloc_bytes = max(ws, self.sq8_workspace_bytes, self.grouped_workspace_bytes)
            self.workspace = self.new_workspace()
        self._host_bufs = {}

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
        """True while the caller has SQ8 enabled (enable_sq8; rf_search_sq8 can run).  A shadow that
        only the `shadow` argument attached does not count."""
        return self._sq8_enabled

    def _attach_shadow(self) -> None:
        torch = _torch()
        nbytes = self.lib.rf_sq8_storage_bytes(self.dim, self.capacity)
        if nbytes == 0:
            raise _lib.RagfinError(-2, f"SQ8 needs dim % 32 == 0 (dim {self.dim})")
        with self._lock, torch.cuda.device(self.device):
            storage = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.rf_index_attach_sq8(self.handle, c_void_p(storage.data_ptr()), nbytes,
                                                    _lib.current_stream_ptr()))
            self._sq8_storage = storage

    def enable_sq8(self) -> None:
        """Attach an int8 shadow (dim + 8 bytes per row of capacity) and quantize every row; adds,
        compactions and resets keep it current from then on.  Needs dim % 32 == 0.  An index that
        already carries one (the `shadow` argument) reuses it."""
        if self._sq8_storage is None:
            self._attach_shadow()
        self._sq8_enabled = True

    def disable_sq8(self) -> None:
        torch = _torch()
        self._sq8_enabled = False
        if self._sq8_storage is None or self.shadow_first:   # (the shadow behind plain searches stays)
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
                             self.workspace.numel(), ("quantize", "sample", "threshold", "emit", "refine", "merge"))

    def _profile(self, fn, q16, B: int, k: int, workspace_bytes: int, stages, lead=(), k_args=None):
        """The first sweep of a B-query batch through a *_profile entry point -> {stage: ms}.
        lead: what the entry point takes between the index and the queries; k_args: what it takes
        in the place of k (the grouped one: n_groups, group_size)."""
        torch = _torch()
        q16 = q16.to(self.device).contiguous()
        scores, ids, _, flags = self._outputs(B, k)
        ms = (ctypes.c_float * len(stages))()
        with self._lock, torch.cuda.device(self.device):
            _lib.check(fn(self.handle, *lead, _ptr(q16), B, *(k_args or (k,)), 0, _ptr(scores), _ptr(ids), None,
                          _ptr(flags), _ptr(self.workspace), workspace_bytes, _lib.current_stream_ptr(), ms))
        return dict(zip(stages, ms))

    # -- search --------------------------------------------------------------
    def new_workspace(self):
        """An extra search workspace: one per batch in flight when several streams
        search the same (immutable) index concurrently.  Large enough for SQ8 too."""
        torch = _torch()
        return torch.zeros(self._alloc_bytes, dtype=torch.uint8, device=self.device)

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
                   workspace=None, stream_ptr=None, filt=None, sq8: bool = False, band=None, group=None, mmr=None,
                   fp16: bool = False):
        """Enqueue rf_search on the current stream (or on `stream_ptr`, a c_void_p holding a
        hipStream_t of this device); no host sync.  Returns
        (scores f32 [B,k], ids i64 [B,k], exact f64 [B,k] | None, flags u32 [B]).
        filt: a filter buffer built for this index (CorpusStore.build_filter / rf_filter_eval):
        rf_search_filtered, the same outputs over the passing rows only.  Or a MultiFilter (per-query
        filters: rf_search_multi_filtered, query b over the passing rows of its own filter; built for
        exactly these B queries; no sq8, band, group or mmr form: ValueError).
        sq8: rf_search_sq8 (needs enable_sq8; not with filt).  A workspace passed in must hold
        sq8_workspace_bytes (new_workspace does).
        fp16: the plain search through rf_search_fp16 -- the fp16 chain even on a shadow-first index
        (the FLAT tier of the ladder, the sharded lanes); no effect on the other forms.
        band: (radius, range_filter) -- rf_search_range: the best k rows with
        radius < fp64 score <= range_filter (within the passing rows with filt; not with sq8).
        group: (codes int32 [size] on this device, n_codes, n_groups, group_size) -- rf_search_grouped:
        the best n_groups groups of rows sharing a code, each by its best group_size rows (within
        the passing rows with filt; not with sq8 or band).  k must be n_groups * group_size; the
        outputs are in the padded slot form (group of rank j in slots [j s, (j + 1) s)).
        mmr: (fetch_k, lam) -- diversified search: the search above runs with the limit fetch_k (into
        device tensors of its own, with the fp64 scores), then rf_mmr_select picks k of its hits by
        maximal marginal relevance with lambda = lam (1 = relevance only) into the outputs, on the
        same stream.  With filt, band or sq8; not with group.  The scores returned are the relevance
        scores, in MMR order; the flags are those of the candidate search.  (The candidate tensors
        come from torch's allocator on the current stream: with a stream_ptr of another stream the
        caller keeps that stream ahead of their reuse, as for every tensor it passes in.)
        Takes no lock, with or without a workspace of the caller's: the benchmark and the sharded
        lanes call it on their own streams, and whoever shares the index's workspace serialises."""
        torch = _torch()
        self._check_variant(filt, sq8, band, group, k, mmr)
        if sq8 and not self._sq8_enabled and self._sq8_storage is not None:   # (no shadow at all: the library says so)
            raise _lib.RagfinError(-1, "rf_search_sq8: SQ8 not enabled on this index (enable_sq8); the shadow it "
                                       "carries serves plain searches only")
        if q16.dtype != torch.float16 or q16.dim() != 2 or q16.shape[1] != self.dim:
            raise ValueError(f"search expects fp16 [B, {self.dim}] queries")
        if not q16.is_contiguous() or q16.device != self.device:
            q16 = q16.to(self.device).contiguous()
        B = q16.shape[0]
        if isinstance(filt, MultiFilter):
            if filt.qfilter.numel() != B or filt.n_rows != self.size or filt.buf.device != self.device:
                raise ValueError(f"per-query filters: built for {filt.qfilter.numel()} queries over {filt.n_rows} rows on "
                                 f"{filt.buf.device}, searched with {B} queries over {self.size} rows on {self.device}")
            scores, ids, exact, flags = self._outputs(B, k, want_exact, out=out)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.rf_search_multi_filtered(
                    self.handle, _ptr(filt.buf), len(filt), _ptr(filt.qfilter), _ptr(q16), B, k, id_base, _ptr(scores),
                    _ptr(ids), _ptr(exact), _ptr(flags), _ptr(workspace if workspace is not None else self.workspace),
                    self.workspace_bytes, stream_ptr if stream_ptr is not None else _lib.current_stream_ptr()))
            return scores, ids, exact, flags
        if mmr is not None:
            # the candidate search (its flags land in the caller's), then the MMR stage behind it
            res = self._outputs(B, k, want_exact, out=out)
            _, cand_ids, cand_exact, _ = self.search_raw(
                q16, int(mmr[0]), id_base, True, out=self._outputs(B, int(mmr[0]), True, flags=False)[:3] + (res[3],),
                workspace=workspace, stream_ptr=stream_ptr, filt=filt, sq8=sq8, band=band, fp16=fp16)
            self._mmr_select(cand_exact, cand_ids, k, mmr, id_base, res, stream_ptr)
            return res
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
                _lib.check((self.lib.rf_search_fp16 if fp16 else self.lib.rf_search)(self.handle, *args))
            else:
                _lib.check(self.lib.rf_search_filtered(self.handle, _ptr(filt), *args))
        return scores, ids, exact, flags

    def _mmr_select(self, cand_exact, cand_ids, k: int, mmr, id_base: int, out, stream_ptr=None):
        """Enqueue rf_mmr_select over the candidates (fp64 scores, ids: device tensors [B, fetch_k])
        into out = (scores, ids, exact | None, ...); no host sync."""
        torch = _torch()
        B, fetch_k = cand_ids.shape
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rf_mmr_select(self.handle, B, fetch_k, k, float(mmr[1]), id_base, _ptr(cand_exact),
                                              _ptr(cand_ids), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                              stream_ptr if stream_ptr is not None else _lib.current_stream_ptr()))

    def _check_variant(self, filt, sq8: bool, band, group, k: int, mmr=None) -> None:
        """Which of filt / sq8 / band / group / mmr go together, for every search method."""
        if isinstance(filt, MultiFilter):
            for name, on in (("SQ8", sq8), ("range (band)", band is not None), ("grouping", group is not None),
                             ("MMR", mmr is not None)):
                if on:
                    raise ValueError(f"per-query filters (MultiFilter) have no {name} form")
        if mmr is not None:
            if group is not None:
                raise ValueError("diversified search (mmr) has no grouping form")
            fetch_k, lam = mmr
            if isinstance(fetch_k, bool) or not isinstance(fetch_k, (int, np.integer)) or \
                    not 1 <= k <= fetch_k <= _lib.RF_MAX_K:
                raise ValueError(f"diversified search: need 1 <= k <= fetch_k <= {_lib.RF_MAX_K} "
                                 f"(got k = {k}, fetch_k = {fetch_k!r})")
            if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)) or \
                    not 0.0 <= float(lam) <= 1.0:
                raise ValueError(f"diversified search: lambda must be a real number in [0, 1], got {lam!r}")
        if group is not None:
            if sq8 or band is not None:
                raise ValueError("grouping search has no SQ8 and no range form")
            self._check_group(group, k)
        elif sq8 and (filt is not None or band is not None):
            raise ValueError("SQ8 search has no filtered and no range form")

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
        n, s = int(group[2]), int(group[3])
        self._check_group(group, n * s)
        return self._profile(self.lib.rf_search_grouped_profile, q16, min(q16.shape[0], _lib.RF_QCHUNK), n * s,
                             self.grouped_workspace_bytes, ("group_max", "threshold", "emit", "merge"),
                             lead=(_ptr(filt), _ptr(group[0]), int(group[1])), k_args=(n, s))

    def enqueue_search(self, q_ptr: int, B: int, k: int, id_base: int, scores_ptr: int, ids_ptr: int,
                       exact_ptr: int, flags_ptr: int, workspace_ptr: int, stream_ptr, fp16: bool = False):
        """The bare rf_search enqueue for callers that own every buffer (the sharded step: no
        tensor checks, no allocations, no stream / device context).  The caller guarantees that
        this index's device is the thread's current HIP device, and serialises the use of
        the workspace it passes: no lock is taken here.  fp16: rf_search_fp16 (the sharded lanes)."""
        fn = self.lib.rf_search_fp16 if fp16 else self.lib.rf_search
        rc = fn(self.handle, q_ptr, B, k, id_base, scores_ptr, ids_ptr, exact_ptr, flags_ptr,
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

    def search_after_raw(self, q16, k: int, after, id_base: int = 0, want_exact: bool = False, out=None,
                         workspace=None, stream_ptr=None, filt=None, band=None):
        """Enqueue rf_search_after (include/ragfin.h, "paged search"); no host sync, no lock (as
        search_raw).  after: (fp64 scores [B], int64 ids [B]) device tensors -- per query the best k
        hits ranked strictly after that (score, id), within filt / band when given.  Returns
        (scores f32 [B,k], ids i64 [B,k], exact f64 [B,k] | None, flags u32 [B])."""
        torch = _torch()
        if q16.dtype != torch.float16 or q16.dim() != 2 or q16.shape[1] != self.dim:
            raise ValueError(f"search expects fp16 [B, {self.dim}] queries")
        if not q16.is_contiguous() or q16.device != self.device:
            q16 = q16.to(self.device).contiguous()
        B = q16.shape[0]
        bs, bi = after
        if not torch.is_tensor(bs) or not torch.is_tensor(bi) or bs.dtype != torch.float64 or \
                bi.dtype != torch.int64 or tuple(bs.shape) != (B,) or tuple(bi.shape) != (B,):
            raise ValueError(f"search_after expects the bound as (float64 [{B}], int64 [{B}]) tensors")
        bs, bi = bs.to(self.device).contiguous(), bi.to(self.device).contiguous()
        lo, hi = (float("-inf"), float("inf")) if band is None else (float(band[0]), float(band[1]))
        scores, ids, exact, flags = self._outputs(B, k, want_exact, out=out)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rf_search_after(
                self.handle, _ptr(filt), _ptr(q16), B, k, id_base, lo, hi, _ptr(bs), _ptr(bi), _ptr(scores), _ptr(ids),
                _ptr(exact), _ptr(flags), _ptr(workspace if workspace is not None else self.workspace),
                self.workspace_bytes, stream_ptr if stream_ptr is not None else _lib.current_stream_ptr()))
        return scores, ids, exact, flags

    def search_after_profile(self, q16, k: int, after, filt=None, band=None):
        """rf_search_after_profile: per-stage HIP-event times in ms of the first 64-query sweep."""
        lo, hi = (float("-inf"), float("inf")) if band is None else (float(band[0]), float(band[1]))
        B = min(q16.shape[0], _lib.RF_QCHUNK)
        bs, bi = after[0][:B].contiguous(), after[1][:B].contiguous()
        torch = _torch()
        q16 = q16.to(self.device).contiguous()
        scores, ids, _, flags = self._outputs(B, k)
        ms = (ctypes.c_float * 4)()
        with self._lock, torch.cuda.device(self.device):
            _lib.check(self.lib.rf_search_after_profile(
                self.handle, _ptr(filt), _ptr(q16), B, k, 0, lo, hi, _ptr(bs), _ptr(bi), _ptr(scores), _ptr(ids), None,
                _ptr(flags), _ptr(self.workspace), self.workspace_bytes, _lib.current_stream_ptr(), ms))
        return dict(zip(("sample", "threshold", "emit", "merge"), ms))

    def _search_after(self, q16, k: int, after, id_base: int, want_exact: bool, filt, band):
        """search_after_raw, then the flagged queries again through the exhaustive kernel with the
        same filter, band and bound -> ((scores, ids, exact),).  The caller holds the lock."""
        torch = _torch()
        scores, ids, exact, flags = self.search_after_raw(q16, k, after, id_base, want_exact, filt=filt, band=band)
        bad = torch.nonzero(flags != 0).flatten()
        if bad.numel() > 0:
            q16 = q16.to(self.device)
            rows = self._exhaustive(q16[bad].contiguous(), k, id_base, want_exact, filt,
                                    after=(after[0].to(self.device)[bad].contiguous(),
                                           after[1].to(self.device)[bad].contiguous()), band=band)
            for dst, src in zip((scores, ids, exact), rows):
                if dst is not None:
                    dst[bad] = src
        return ((scores, ids, exact),)

    def search_after(self, q16, k: int, after, id_base: int = 0, want_exact: bool = False, filt=None, band=None):
        """The best k (<= RF_MAX_K) hits per query ranked strictly after the bound `after` = (fp64
        scores [B], int64 ids [B], device tensors; ids with id_base): one sweep of the corpus
        through rf_search_after whatever the depth, then the flagged-query ladder (a flagged query
        through _exhaustive(..., after=...)).  filt: over the passing rows.  band: (radius,
        range_filter), within the band.  A bound score of +inf is the first page; (-inf, any id)
        gives all padding.  -> (scores, ids, exact | None) on the device."""
        with self._lock:
            return self._search_after(q16, k, after, id_base, want_exact, filt, band)[0]

    PAGES_PER_SYNC = 16   # search_large: pages enqueued back to back before their flags are read

    @staticmethod
    def _bound_after(exact, ids):
        """The bound of the next page: the last hit of this one; a query whose page is not full is
        exhausted and keeps a bound nothing can follow.  Device tensors, no sync."""
        torch = _torch()
        last_s, last_i = exact[:, -1], ids[:, -1]
        return (torch.where(last_i >= 0, last_s, torch.full_like(last_s, float("-inf"))).contiguous(),
                torch.where(last_i >= 0, last_i, torch.full_like(last_i, 2 ** 62)).contiguous())

    def search_large(self, q16, k: int, id_base: int = 0, want_exact: bool = False, filt=None, band=None):
        """Limits above RF_MAX_K: the first page through the fused path, further pages of RF_MAX_K
        through the search-after sweep (rf_search_after: each page = the hits ranked strictly after
        the previous page's last hit, one sweep of the corpus per page whatever its depth).  The
        pages are enqueued back to back, PAGES_PER_SYNC at a time, each bound taken from the page
        before on the device; their flags are read with one synchronisation, and from the first
        page that holds a flagged query on, the pages are walked again one by one through the
        ladder (search_after: the flagged queries through the exhaustive kernel with the same
        bound).  Returns (scores, ids) [B, k] (+ the fp64 ranking scores with want_exact: what a
        cross-shard merge ranks by).  filt: the same over the passing rows.  band: (radius,
        range_filter) -- the same within the band, the first page through rf_search_range.  The
        walk ends with the first group of pages whose last one no query fills."""
        torch = _torch()
        q16 = q16.to(self.device).contiguous()
        B = q16.shape[0]
        page = _lib.RF_MAX_K
        pages = [self.search(q16, page, id_base, want_exact=True, filt=filt, band=band)]
        got = page
        more = bool((pages[0][1][:, -1] >= 0).any()) if got < k else False
        while got < k and more:
            n_pages = min(self.PAGES_PER_SYNC, -(-(k - got) // page))
            with self._lock:
                flags = []
                for _ in range(n_pages):
                    bound = self._bound_after(pages[-1][2], pages[-1][1])
                    *res, f = self.search_after_raw(q16, page, bound, id_base, True, filt=filt, band=band)
                    pages.append(tuple(res))
                    flags.append(f)
                state = torch.cat([(torch.stack(flags) != 0).any(1), (pages[-1][1][:, -1] >= 0).any().reshape(1)]).cpu()
                bad = torch.nonzero(state[:-1]).flatten()
                more = bool(state[-1])
                if bad.numel() > 0:   # unproven from page j of the group on: those again, through the ladder
                    j = int(bad[0])
                    del pages[len(pages) - n_pages + j:]
                    for _ in range(j, n_pages):
                        bound = self._bound_after(pages[-1][2], pages[-1][1])
                        pages.append(self._search_after(q16, page, bound, id_base, True, filt, band)[0])
                    more = bool((pages[-1][1][:, -1] >= 0).any())
            got += n_pages * page
        scores, ids, exacts = ([p[j] for p in pages] for j in range(3))
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
        grouping search re-runs group by group).  A MultiFilter re-runs filter by filter: one
        exhaustive call serves all flagged queries of a filter, over that filter's own buffer.
        The caller holds the lock."""
        if isinstance(filt, MultiFilter):
            torch = _torch()
            bad = torch.nonzero(flags != 0).flatten()
            if bad.numel() == 0:
                return bad, None
            bad_h = bad.cpu().numpy()
            rows = list(self._outputs(bad_h.size, k, want_exact, flags=False)[:3])
            q16 = q16.to(self.device)
            of = filt.qfilter_host[bad_h]
            for g in np.unique(of).tolist():
                at = torch.from_numpy(np.flatnonzero(of == g)).to(self.device)
                part = self._exhaustive(q16[bad.to(self.device)[at]].contiguous(), k, id_base, want_exact, filt.filters[g])
                for dst, src in zip(rows, part):
                    if dst is not None:
                        dst[at] = src
            return bad, rows
        if group is not None:
            return rerun_flagged(q16, k, id_base, flags, False, filt, None,
                                 lambda q, k, base, f: self._grouped_exhaustive(q, group, base, want_exact, f))
        # (a plain first pass on a shadow-first index swept the shadow like an SQ8 one: fp16 comes next)
        shadow = sq8 or (filt is None and band is None and self._plain_chain_is_shadow(q16.shape[0]))
        return rerun_flagged(q16, k, id_base, flags, shadow, filt,
                             lambda q, k, base: self.search_raw(q, k, base, want_exact, band=band, fp16=True),
                             lambda q, k, base, f: self._exhaustive(q, k, base, want_exact, f, band=band))

    def _plain_chain_is_shadow(self, B: int) -> bool:
        """Whether a plain rf_search of B queries takes the shadow chain: plain_chain in api.hip, condition
        for condition (switch set, size >= min_rows, size > RF_SMALL_ROWS, one 64-query sweep)."""
        if not self.shadow_first or B > _lib.RF_QCHUNK:
            return False
        n = self.size
        return n >= self._shadow_min_rows and n > _lib.RF_SMALL_ROWS

    def _grouped_first_pass(self, q16, k: int, id_base: int, want_exact: bool, filt, sq8: bool, band, group,
                            out=None):
        """search_raw(group=...), or -- a dictionary above RF_GROUP_MAX_CODES -- outputs whose every
        query is flagged, so that the ladder answers the whole batch."""
        if int(group[1]) <= _lib.RF_GROUP_MAX_CODES:
            return self.search_raw(q16, k, id_base, want_exact, out=out, filt=filt, sq8=sq8, band=band, group=group)
        self._check_variant(filt, sq8, band, group, k)
        res = self._outputs(q16.shape[0], k, want_exact, out=out)
        res[3].fill_(_lib.RF_FLAG_CAND_OVERFLOW)
        return res

    def _search_ladder(self, q16, k: int, id_base: int, want_exact: bool, filt, sq8: bool, band, group, out=None,
                       landed=None, mmr=None):
        """The first pass (search_raw, or _grouped_first_pass for a grouping search), then the
        flagged-query ladder -> ((scores, ids, exact, flags), bad, rows): the first pass's outputs
        and what _rerun_flagged gives; the caller patches rows `bad` of its own destination when
        rows is not None.  out: as in search_raw.  landed(outputs) -> flags: called between the two
        by search_host, which reads the flags on the host once it has synchronised.  Caller locks.
        mmr: as in search_raw; the first pass enqueues the candidate search and the MMR stage back to
        back, and a flagged query gets its fetch_k candidates from the ladder and the MMR stage again:
        its first-pass row is always replaced."""
        if group is not None:
            res = self._grouped_first_pass(q16, k, id_base, want_exact, filt, sq8, band, group, out)
        else:
            res = self.search_raw(q16, k, id_base, want_exact, out=out, filt=filt, sq8=sq8, band=band, mmr=mmr)
        flags = res[3]
        if landed is not None:
            flags = landed(res)
            if not bool(flags.any()):
                return res, None, None
        if mmr is None:
            return (res,) + self._rerun_flagged(q16, k, id_base, want_exact, flags, sq8, filt, band, group)
        bad, cand = self._rerun_flagged(q16, int(mmr[0]), id_base, True, flags, sq8, filt, band)
        if cand is None:
            return res, bad, None
        rows = self._outputs(cand[1].shape[0], k, want_exact, flags=False)[:3]
        self._mmr_select(cand[2].contiguous(), cand[1].contiguous(), k, mmr, id_base, rows)
        return res, bad, list(rows)

    # -- per-row weights (include/ragfin.h, "decayed search") --------------------------------
    def _check_weights(self, weights, filt, sq8: bool = False, band=None, group=None, mmr=None):
        """weights = (w32 float32 [size], w64 float64 [size]) on this device, contiguous, every weight in [0, 1]
        (decay_weights gives such a pair); with at most one filter buffer and no other form."""
        torch = _torch()
        for name, on in (("per-query filter (MultiFilter)", isinstance(filt, MultiFilter)), ("SQ8", sq8),
                         ("range (band)", band is not None), ("grouping", group is not None), ("MMR", mmr is not None)):
            if on:
                raise ValueError(f"weighted search has no {name} form")
        n = self.size
        ok = isinstance(weights, (tuple, list)) and len(weights) == 2 and all(torch.is_tensor(w) for w in weights)
        if ok:
            w32, w64 = weights
            ok = w32.dtype == torch.float32 and w64.dtype == torch.float64 and tuple(w32.shape) == (n,) and \
                tuple(w64.shape) == (n,) and w32.device == self.device and w64.device == self.device and \
                w32.is_contiguous() and w64.is_contiguous() and w32.data_ptr() % 16 == 0
        if not ok:
            raise ValueError(f"weights must be (float32 [{n}], float64 [{n}]) contiguous tensors on {self.device}, "
                             "the first 16-byte aligned")
        return weights

    def search_weighted_raw(self, q16, k: int, weights, id_base: int = 0, filt=None):
        """Enqueue rf_search_weighted on the current stream; no host sync, no lock (as search_raw).
        -> (scores f32 [B,k], ids i64 [B,k], decayed f64 [B,k], base f64 [B,k], flags i32 [B]): per
        query the best k rows (of the rows `filt` passes) by (w64[row] * s desc, s desc, row asc)."""
        torch = _torch()
        w32, w64 = self._check_weights(weights, filt)
        if q16.dtype != torch.float16 or q16.dim() != 2 or q16.shape[1] != self.dim:
            raise ValueError(f"search expects fp16 [B, {self.dim}] queries")
        if not q16.is_contiguous() or q16.device != self.device:
            q16 = q16.to(self.device).contiguous()
        B = q16.shape[0]
        scores, ids, decayed, flags = self._outputs(B, k, True)
        base = torch.empty((B, k), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rf_search_weighted(self.handle, _ptr(filt), _ptr(w32), _ptr(w64), _ptr(q16), B, k, id_base,
                                                   _ptr(scores), _ptr(ids), _ptr(decayed), _ptr(base), _ptr(flags),
                                                   _ptr(self.workspace), self.workspace_bytes, _lib.current_stream_ptr()))
        return scores, ids, decayed, base, flags

    def _exhaustive_weighted(self, q16, k: int, weights, id_base: int = 0, filt=None):
        """rf_search_exhaustive_weighted -> (scores, ids, decayed, base).  Uses the index workspace: the
        caller holds the lock."""
        torch = _torch()
        w32, w64 = weights
        q16 = q16.to(self.device).contiguous()
        B = q16.shape[0]
        scores, ids, decayed, _ = self._outputs(B, k, True, flags=False)
        base = torch.empty((B, k), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rf_search_exhaustive_weighted(
                self.handle, _ptr(filt), _ptr(w32), _ptr(w64), _ptr(q16), B, k, id_base, _ptr(scores), _ptr(ids),
                _ptr(decayed), _ptr(base), _ptr(self.workspace), self.workspace_bytes, _lib.current_stream_ptr()))
        return scores, ids, decayed, base

    def search_exhaustive_weighted(self, q16, k: int, weights, id_base: int = 0, filt=None):
        self._check_weights(weights, filt)
        with self._lock:
            return self._exhaustive_weighted(q16, k, weights, id_base, filt)

    def _search_weighted(self, q16, k: int, weights, id_base: int, filt):
        """search_weighted_raw, then the flagged queries again through the exhaustive weighted kernel,
        over the same rows and weights -> (scores, ids, decayed, base)."""
        with self._lock:
            *res, flags = self.search_weighted_raw(q16, k, weights, id_base, filt)
            bad, rows = rerun_flagged(q16, k, id_base, flags, False, filt, None,
                                      lambda q, k, base, f: self._exhaustive_weighted(q, k, weights, base, f))
            if rows is not None:
                for dst, src in zip(res, rows):
                    dst[bad] = src
        return tuple(res)

    def search(self, q16, k: int, id_base: int = 0, want_exact: bool = False, filt=None, sq8: bool = False,
               band=None, group=None, mmr=None, weights=None):
        """rf_search, then the flagged-query ladder (rerun_flagged) for any query the fused path
        could not prove exact.  filt: over the passing rows.  sq8: rf_search_sq8 first.
        band: (radius, range_filter) -- rf_search_range, flagged queries through the exhaustive
        band kernel.  group: as in search_raw -- rf_search_grouped, flagged queries (and every query
        of a dictionary above RF_GROUP_MAX_CODES) group by group through the exhaustive kernel.
        mmr: (fetch_k, lam), as in search_raw -- k of the best fetch_k hits by maximal marginal
        relevance; flagged queries get their candidates from the ladder and are selected again.
        weights: (w32, w64) per-row weights in [0, 1] (decay_weights) -- rf_search_weighted: the best k
        rows by (w64[row] * s desc, s desc, row asc), flagged queries through the exhaustive weighted
        kernel; the result is then (scores, ids, decayed f64, base f64).  With filt (one filter
        buffer) or without; no other form (ValueError)."""
        if weights is not None:
            self._check_weights(weights, filt, sq8, band, group, mmr)
            return self._search_weighted(q16, k, weights, id_base, filt)
        with self._lock:
            (scores, ids, exact, _), bad, rows = self._search_ladder(q16, k, id_base, want_exact, filt, sq8, band, group,
                                                                     mmr=mmr)
            if rows is not None:
                for dst, src in zip((scores, ids, exact), rows):
                    if dst is not None:
                        dst[bad] = src
        return scores, ids, exact

    ZERO_COPY_MAX = 4096   # B * k up to which search_host lets the kernel write into host memory

    def search_host(self, q16, k: int, filt=None, sq8: bool = False, band=None, group=None, mmr=None):
        """search() whose results land on the host with ONE synchronisation: scores, ids and
        flags are copied into cached pinned buffers asynchronously.  -> (scores f32 [B,k],
        ids i64 [B,k]) numpy arrays (the caller's own copies).  filt: over the passing rows.
        sq8: rf_search_sq8 first, as in search().  band: (radius, range_filter), as in search().
        group: as in search(); k = n_groups * group_size, the padded slot form.
        mmr: (fetch_k, lam), as in search(); still one synchronisation unless a query is flagged."""
        torch = _torch()
        with self._lock:
            B = q16.shape[0]
            key = (B, k)
            bufs = self._host_bufs.get(key)
            if bufs is None:
                bufs = self._host_bufs[key] = (torch.empty((B, k), dtype=torch.float32, pin_memory=True),
                                               torch.empty((B, k), dtype=torch.int64, pin_memory=True),
                                               torch.empty((B,), dtype=torch.int32, pin_memory=True))
            # query-sized results: the merge kernel stores straight into the pinned host buffers
            # (host-coherent memory, mapped at the same address on the device) -- no copy commands,
            # only the synchronisation.  A grouping search is downloaded, as every larger result.
            zero_copy = group is None and B * k <= self.ZERO_COPY_MAX and _ZERO_COPY

            def landed(res):
                if not zero_copy:
                    for dst, src in zip(bufs, (res[0], res[1], res[3])):
                        dst.copy_(src, non_blocking=True)
                torch.cuda.current_stream(self.device).synchronize()
                return bufs[2]

            _, bad, rows = self._search_ladder(q16, k, 0, False, filt, sq8, band, group,
                                               (bufs[0], bufs[1], None, bufs[2]) if zero_copy else None, landed, mmr)
            if rows is not None:
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


class SparseIndex:
    """Thin object wrapper over rf_sparse_* (include/ragfin.h, "lexical search"): the posting arrays
    of a `lexical.Postings` on the device, the handle over them and a search workspace.

    Locking: as in GpuIndex, the workspaces are shared by every caller, so `search` and `text_match`
    hold `self._lock` while they size a workspace and enqueue; the results are the caller's own
    tensors.  The postings are immutable: a changed corpus gets a new SparseIndex.  The token
    positions (`attach_positions`) are given once, by whoever needs a phrase first; the caller
    serialises that against `text_match` (CorpusStore: under its `_sparse_lock`).

    Index maintenance: built from postings that carry `post_tf` and `dl`, the index also
    holds the term frequencies and row lengths (`supports_update`), and `appended` / `compacted` return
    a NEW SparseIndex over new tensors -- the arrays a build of the changed corpus would give, positions
    included when attached here -- while this one stays valid for whoever still holds it."""

    def __init__(self, postings, device=None):
        torch = _torch()
        device = require_gpu(device)
        tf, dl = getattr(postings, "post_tf", None), getattr(postings, "dl", None)
        with torch.cuda.device(device):
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)   # noqa: E731
            # (uint32 rows and counts travel as their int32 bit patterns)
            self._adopt(device, postings.n_rows, postings.n_terms, up(postings.post_off, np.int64),
                        up(np.ascontiguousarray(postings.post_row, dtype=np.uint32).view(np.int32), np.int32),
                        up(postings.post_imp, np.float32),
                        None if tf is None else up(np.ascontiguousarray(tf, dtype=np.uint32).view(np.int32), np.int32),
                        None if tf is None or dl is None else up(dl, np.int32))

    def _adopt(self, device, n_rows, n_terms, post_off, post_row, post_imp, post_tf, dl, positions=None):
        """Become the index over these device tensors (the constructor's, or an update's new ones)."""
        torch = _torch()
        self.device = device
        self.lib = _lib.load_library()
        self.n_rows, self.n_terms, self.nnz = int(n_rows), int(n_terms), int(post_row.numel())
        self.post_off, self.post_row, self.post_imp = post_off, post_row, post_imp
        # what index maintenance needs beside the postings: the term frequencies and the row lengths
        self.post_tf, self.dl = post_tf, dl
        handle = c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rf_sparse_create(ctypes.byref(handle), self.n_rows, self.n_terms, self.nnz,
                                                 _ptr(self.post_off), _ptr(self.post_row), _ptr(self.post_imp),
                                                 self.device.index))
        self.handle = handle
        self.workspace = None
        self.text_workspace = None
        self.positions = None   # (pos_off, pos) device tensors once attach_positions has run
        self._lock = threading.Lock()
        if positions is not None:
            self._attach(*positions)

    # -- the device build (include/ragfin.h, "lexical index build") ------------------------
    @staticmethod
    def count_tokens(n_terms: int, tok, dl, device=None, positions: bool = False, timing: dict | None = None):
        """rf_sparse_count_plan / _apply over a token stream -> (post_off int64 [n_terms + 1] host array,
        post_row, post_tf int32 device tensors [nnz] (uint32 bit patterns), (pos_off, pos) device tensors
        or None): what lexical.counts_from_tokens defines.  tok int32 [n_tokens] (>= 1 token): the term id
        of every token in (row, position) order; dl int64 [n]: the tokens per row.  One synchronisation,
        to read post_off and the totals back.  timing: filled with the seconds of the stages (each ended
        by a synchronisation of its own: for tools)."""
        import time
        torch = _torch()
        device = require_gpu(device)
        lib = _lib.load_library()
        tok = np.ascontiguousarray(tok, dtype=np.int32)
        dl = np.asarray(dl, dtype=np.int64)
        n_tokens, n_rows, n_terms = int(tok.size), int(dl.size), int(n_terms)
        row_start = np.zeros(n_rows + 1, dtype=np.int64)
        np.cumsum(dl, out=row_start[1:])
        if n_tokens < 1 or int(row_start[-1]) != n_tokens:
            raise ValueError(f"count_tokens: {n_tokens} tokens for rows that hold {int(row_start[-1])} (at least one)")
        need = lib.rf_sparse_count_workspace_bytes(n_tokens, n_terms)
        if need == 0:
            raise ValueError(f"count_tokens: {n_tokens} tokens over {n_terms} terms is out of range")

        def lap(name, t0):
            if timing is not None:
                torch.cuda.synchronize(device)
                timing[name] = timing.get(name, 0.0) + time.perf_counter() - t0
            return time.perf_counter()
        with torch.cuda.device(device):
            t0 = time.perf_counter()
            tok_d = torch.from_numpy(tok).to(device)
            start_d = torch.from_numpy(row_start).to(device)
            t0 = lap("upload_s", t0)
            ws = torch.empty(need, dtype=torch.uint8, device=device)
            head = torch.empty(n_terms + 3, dtype=torch.int64, device=device)   # post_off, then nnz and n_pos
            stream = _lib.current_stream_ptr()
            _lib.check(lib.rf_sparse_count_plan(_ptr(tok_d), _ptr(start_d), n_tokens, n_rows, n_terms, _ptr(head),
                                                c_void_p(head.data_ptr() + 8 * (n_terms + 1)), _ptr(ws), need, stream))
            t0 = lap("plan_s", t0)
            raw = head.cpu().numpy()   # the one synchronisation
            t0 = lap("readback_s", t0)
            post_off, nnz, n_pos = raw[:n_terms + 1].copy(), int(raw[n_terms + 1]), int(raw[n_terms + 2])
            if not (1 <= nnz <= n_tokens and n_pos == n_tokens and int(post_off[-1]) == nnz and int(post_off[0]) == 0):
                raise RuntimeError(f"rf_sparse_count_plan: inconsistent totals (nnz {nnz}, n_pos {n_pos}, {n_tokens} tokens)")
            row = torch.empty(nnz, dtype=torch.int32, device=device)
            tf = torch.empty(nnz, dtype=torch.int32, device=device)
            pos = None
            if positions:
                pos = (torch.empty(nnz + 1, dtype=torch.int64, device=device),
                       torch.empty(n_tokens, dtype=torch.int32, device=device))
            out = _lib.Postings(n_rows, n_terms, nnz, n_tokens if positions else 0)
            out.post_row, out.post_tf = row.data_ptr(), tf.data_ptr()
            if positions:
                out.pos_off, out.pos = pos[0].data_ptr(), pos[1].data_ptr()
            _lib.check(lib.rf_sparse_count_apply(_ptr(start_d), n_tokens, n_rows, n_terms, _ptr(ws), need, ctypes.byref(out),
                                                 1 if positions else 0, stream))
            lap("apply_s", t0)
        return post_off, row, tf, pos

    @classmethod
    def from_tokens(cls, vocab_size: int, tok, dl, k1: float, b: float, device=None, positions: bool = False,
                    timing: dict | None = None):
        """The index of a corpus given as a token stream (lexical.analyze_native's tok and dl), built on the
        device: count_tokens, idf on the host (lexical.term_idf: numpy's log), rf_sparse_impacts.  The arrays
        equal lexical.build_postings' bit for bit; `host_post_off` keeps the term offsets for the caller's
        Postings.  build_postings' guard -- every impact a positive normal fp32 value -- is checked here on
        the device array (one reduction, one synchronisation); ValueError as there.  `supports_update` holds."""
        import time
        torch = _torch()
        from . import lexical
        device = require_gpu(device)
        k1, b = lexical.check_bm25_params(k1, b)
        dl = np.asarray(dl, dtype=np.int64)
        post_off, row, tf, pos = cls.count_tokens(vocab_size, tok, dl, device, positions, timing)
        t0 = time.perf_counter()
        seed = cls.__new__(cls)
        seed.device, seed.lib = device, _lib.load_library()
        new = seed._updated(int(dl.size), post_off, row, tf, dl, k1, b, pos)
        with torch.cuda.device(device):
            tiny = float(np.finfo(np.float32).tiny)
            ok = bool((torch.isfinite(new.post_imp) & (new.post_imp >= tiny)).all().item())
        if timing is not None:
            timing["impacts_s"] = timing.get("impacts_s", 0.0) + time.perf_counter() - t0
        if not ok:
            raise ValueError("BM25 impacts must be positive normal fp32 values (check bm25_k1 / bm25_b)")
        new.host_post_off = post_off
        return new

    def attach_token_positions(self, tok, dl) -> None:
        """The token positions of an index that from_tokens built, from the same token stream: the device
        build again, with positions, whose (pos_off, pos) are attached.  ValueError when the stream does
        not give this index's postings."""
        torch = _torch()
        post_off, row, tf, pos = self.count_tokens(self.n_terms, tok, dl, self.device, positions=True)
        with torch.cuda.device(self.device):
            same = int(row.numel()) == self.nnz and int(np.asarray(dl).size) == self.n_rows and \
                bool(torch.equal(row, self.post_row)) and (self.post_tf is None or bool(torch.equal(tf, self.post_tf)))
        if not same:
            raise ValueError("attach_token_positions: the token stream does not give the postings of this index")
        self._attach(*pos)

    @property
    def supports_update(self) -> bool:
        """`appended` / `compacted` can run: the term frequencies and row lengths are on the device."""
        return self.post_tf is not None and self.dl is not None

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.lib.rf_sparse_destroy(h)
            self.handle = None

    def attach_positions(self, pos_off, pos) -> None:
        """rf_sparse_attach_positions: the pair of lexical.build_positions (host numpy), copied to the
        device and kept alive with the handle.  PHRASE leaves of text_match need it."""
        torch = _torch()
        with torch.cuda.device(self.device):
            off_d = torch.from_numpy(np.ascontiguousarray(pos_off, dtype=np.int64)).to(self.device)
            pos_d = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.uint32).view(np.int32)).to(self.device)
        self._attach(off_d, pos_d)

    def _attach(self, off_d, pos_d) -> None:
        with _torch().cuda.device(self.device):
            _lib.check(self.lib.rf_sparse_attach_positions(self.handle, _ptr(off_d), _ptr(pos_d), pos_d.numel()))
        self.positions = (off_d, pos_d)

    # -- index maintenance (include/ragfin.h, "lexical index maintenance") -----------------
    def _desc(self, n_rows, n_terms, post_off, post_row, post_tf, positions):
        """rf_postings over device tensors (kept alive by the caller for the call)."""
        d = _lib.Postings(int(n_rows), int(n_terms), int(post_row.numel()) if post_row is not None else 0,
                          int(positions[1].numel()) if positions is not None else 0)
        d.post_off = None if post_off is None else post_off.data_ptr()
        d.post_row, d.post_tf = post_row.data_ptr(), post_tf.data_ptr()
        if positions is not None:
            d.pos_off, d.pos = positions[0].data_ptr(), positions[1].data_ptr()
        return d

    def host_array(self, name: str) -> np.ndarray:
        """post_row / post_tf (uint32) or post_imp (fp32) as a host array (synchronises)."""
        a = getattr(self, name).cpu().numpy()
        return a.view(np.uint32) if name in ("post_row", "post_tf") else a

    def _own_desc(self):
        return self._desc(self.n_rows, self.n_terms, self.post_off, self.post_row, self.post_tf, self.positions)

    def _updated(self, n_rows, post_off, post_row, post_tf, dl, k1, b, positions):
        """A new SparseIndex over freshly written counts: idf from the host (numpy's log), the impacts from
        rf_sparse_impacts.  post_off, dl: host arrays (int64); the rest device tensors.  Enqueued on the
        current stream; nothing here waits for the device."""
        torch = _torch()
        from . import lexical
        n_terms = int(post_off.size) - 1
        idf = lexical.term_idf(int(n_rows), np.diff(post_off))
        avgdl = float(dl.sum()) / int(n_rows)
        with torch.cuda.device(self.device):
            off_d = torch.from_numpy(np.ascontiguousarray(post_off, dtype=np.int64)).to(self.device)
            idf_d = torch.from_numpy(np.ascontiguousarray(idf, dtype=np.float64)).to(self.device)
            dl_d = torch.from_numpy(np.ascontiguousarray(dl, dtype=np.int32)).to(self.device)
            imp = torch.empty(post_row.numel(), dtype=torch.float32, device=self.device)
            _lib.check(self.lib.rf_sparse_impacts(_ptr(off_d), _ptr(post_row), _ptr(post_tf), _ptr(idf_d), _ptr(dl_d),
                                                  int(n_rows), n_terms, post_row.numel(), avgdl, float(k1), float(b),
                                                  _ptr(imp), _lib.current_stream_ptr()))
        new = SparseIndex.__new__(SparseIndex)
        new._adopt(self.device, n_rows, n_terms, off_d, post_row, imp, post_tf, dl_d, positions)
        return new

    def appended(self, delta, map_old, map_delta, post_off, dl, k1: float, b: float):
        """The index after an append (rf_sparse_append, rf_sparse_impacts) -> a NEW SparseIndex over new
        tensors; this one stays valid.  delta: lexical.count_terms of the appended texts; map_old /
        map_delta: lexical.merge_vocab's term maps; post_off int64 [V + 1], dl int64 [N]: the merged term
        offsets and every row's length, host arrays.  Positions are carried when attached here."""
        torch = _torch()
        if not self.supports_update:
            raise ValueError("this SparseIndex was built without term frequencies: no incremental update")
        pos = self.positions is not None
        n_rows = self.n_rows + int(delta.dl.size)
        n_terms = int(post_off.size) - 1
        nnz = self.nnz + delta.nnz
        with self._lock, torch.cuda.device(self.device):
            i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(self.device)   # noqa: E731
            i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(self.device)   # noqa: E731
            pad = lambda a, dt: np.concatenate([np.asarray(a, dtype=dt), np.zeros(1, dtype=dt)])   # noqa: E731  (never empty)
            d_off, d_row, d_tf = i64(delta.post_off), i32(pad(delta.post_row, np.uint32)), i32(pad(delta.post_tf, np.uint32))
            d_pos = (i64(delta.pos_off), i32(pad(delta.pos, np.uint32))) if pos else None
            m_old, m_delta, off_d = i64(pad(map_old, np.int64)), i64(pad(map_delta, np.int64)), i64(post_off)
            row = torch.empty(nnz, dtype=torch.int32, device=self.device)
            tf = torch.empty(nnz, dtype=torch.int32, device=self.device)
            positions = None
            if pos:
                n_pos = int(self.positions[1].numel()) + int(delta.pos.size)
                positions = (torch.empty(nnz + 1, dtype=torch.int64, device=self.device),
                             torch.empty(max(n_pos, 1), dtype=torch.int32, device=self.device))
            old_desc = self._own_desc()
            delta_desc = self._desc(delta.dl.size, len(delta.vocab), d_off, d_row, d_tf, d_pos)
            delta_desc.nnz = delta.nnz
            merged_desc = self._desc(n_rows, n_terms, off_d, row, tf, positions)
            if pos:
                delta_desc.n_pos = int(delta.pos.size)
                merged_desc.n_pos = n_pos
            need = self.lib.rf_sparse_append_workspace_bytes(self.n_terms, len(delta.vocab))
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.rf_sparse_append(ctypes.byref(old_desc), ctypes.byref(delta_desc), _ptr(m_old),
                                                 _ptr(m_delta), ctypes.byref(merged_desc), _ptr(ws), ws.numel(),
                                                 _lib.current_stream_ptr()))
            if pos and n_pos == 0:
                positions = (positions[0], positions[1][:0])
        return self._updated(n_rows, post_off, row, tf, dl, k1, b, positions)

    def compacted(self, row_map, dl, k1: float, b: float):
        """The index after a delete (rf_sparse_compact_plan / _apply, rf_sparse_impacts) -> (a NEW
        SparseIndex or None when no posting survives, alive bool [V]: the terms that keep a posting,
        post_off int64: the surviving terms' offsets).  row_map int32 [n_rows]: the new number of every
        row, -1 for a row that goes; dl int64: the surviving rows' lengths.  One synchronisation, to
        read the V + 2 raw term offsets back.  This object stays valid."""
        torch = _torch()
        if not self.supports_update:
            raise ValueError("this SparseIndex was built without term frequencies: no incremental update")
        row_map = np.ascontiguousarray(row_map, dtype=np.int32)
        if row_map.size != self.n_rows:
            raise ValueError(f"compacted: a row map of {row_map.size} rows for an index over {self.n_rows}")
        pos = self.positions is not None
        with self._lock, torch.cuda.device(self.device):
            map_d = torch.from_numpy(row_map).to(self.device)
            dst_post = torch.empty(self.nnz + 1, dtype=torch.int64, device=self.device)
            dst_pos = torch.empty(self.nnz + 1, dtype=torch.int64, device=self.device) if pos else None
            term_dst = torch.empty(self.n_terms + 2, dtype=torch.int64, device=self.device)
            need = self.lib.rf_sparse_compact_workspace_bytes(self.nnz)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            old_desc = self._own_desc()
            _lib.check(self.lib.rf_sparse_compact_plan(ctypes.byref(old_desc), _ptr(map_d), _ptr(dst_post), _ptr(dst_pos),
                                                       _ptr(term_dst), _ptr(ws), ws.numel(), _lib.current_stream_ptr()))
            raw = term_dst.cpu().numpy()   # the one synchronisation
            df = np.diff(raw[:self.n_terms + 1])
            alive = df > 0
            post_off = np.zeros(int(alive.sum()) + 1, dtype=np.int64)
            np.cumsum(df[alive], out=post_off[1:])
            nnz, n_pos = int(post_off[-1]), int(raw[self.n_terms + 1])
            if nnz == 0 or dl.size == 0:
                return None, alive, post_off
            row = torch.empty(nnz, dtype=torch.int32, device=self.device)
            tf = torch.empty(nnz, dtype=torch.int32, device=self.device)
            positions = None
            if pos:
                positions = (torch.empty(nnz + 1, dtype=torch.int64, device=self.device),
                             torch.empty(max(n_pos, 1), dtype=torch.int32, device=self.device))
            out_desc = self._desc(dl.size, post_off.size - 1, None, row, tf, positions)
            if pos:
                out_desc.n_pos = n_pos
            _lib.check(self.lib.rf_sparse_compact_apply(ctypes.byref(old_desc), _ptr(map_d), _ptr(dst_post), _ptr(dst_pos),
                                                        ctypes.byref(out_desc), _lib.current_stream_ptr()))
            if pos and n_pos == 0:
                positions = (positions[0], positions[1][:0])
        return self._updated(dl.size, post_off, row, tf, dl, k1, b, positions), alive, post_off

    def text_match(self, leaves, out=None):
        """Enqueue rf_text_match on the current stream; no host sync.  leaves: (kind, term ids,
        min_match) as in filter_expr.Program.text_leaves, 1..RF_TEXT_MAX_LEAVES of them.  -> the row
        bitmaps, an int32 device tensor [L, words_per_leaf] of uint32 bit patterns: bit r & 31 of word
        r >> 5 of row l = row r passes leaf l; words_per_leaf = ceil(n_rows / 32) rounded up to 4 (a
        leaf's words start 16-byte aligned), every word written, bits past n_rows zero.  out: a
        contiguous int32 device tensor of that shape to write into instead of a fresh one."""
        torch = _torch()
        prog = filter_expr.Program(text_leaves=list(leaves))
        arr, terms = filter_expr.text_leaf_arrays(prog)
        L = len(arr)
        words = ((self.n_rows + 31) // 32 + 3) // 4 * 4
        terms_d = torch.from_numpy(np.concatenate([terms, np.zeros(1, dtype=np.int32)])).to(self.device)
        if out is None:
            out = torch.empty((L, words), dtype=torch.int32, device=self.device)
        elif tuple(out.shape) != (L, words) or out.dtype != torch.int32 or not out.is_contiguous():
            raise ValueError(f"text_match: out must be a contiguous int32 tensor [{L}, {words}]")
        with self._lock, torch.cuda.device(self.device):
            need = self.lib.rf_text_match_workspace_bytes(self.handle, L)
            if need == 0:
                raise ValueError(f"text_match: {L} leaves, need 1..{_lib.RF_TEXT_MAX_LEAVES}")
            if self.text_workspace is None or self.text_workspace.numel() < need:
                self.text_workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.rf_text_match(self.handle, arr, L, _ptr(terms_d), int(terms.size), _ptr(out), words,
                                              _ptr(self.text_workspace), self.text_workspace.numel(),
                                              _lib.current_stream_ptr()))
        return out

    def search(self, q_off, q_term, q_weight, k: int, id_base: int = 0, filt=None, want_exact: bool = True):
        """Enqueue rf_sparse_search on the current stream; no host sync.  q_off int32 [B + 1], q_term
        int32, q_weight fp32: the CSR batch of lexical.encode_queries (numpy or tensors).  filt: a
        filter buffer built for n_rows rows.  -> (scores f32 [B,k], ids i64 [B,k], exact f64 [B,k] | None)
        on the device, padded with -inf / -1."""
        torch = _torch()
        if not 1 <= k <= _lib.RF_MAX_K:
            raise ValueError(f"BM25 search: need 1 <= k <= {_lib.RF_MAX_K}, got {k}")
        q_off = torch.as_tensor(q_off, dtype=torch.int32).to(self.device).contiguous()
        # (an empty batch of terms still needs a pointer: one spare entry)
        q_term = torch.cat([torch.as_tensor(q_term, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)]
                           ).to(self.device)
        q_weight = torch.cat([torch.as_tensor(q_weight, dtype=torch.float32), torch.zeros(1, dtype=torch.float32)]
                             ).to(self.device)
        B = q_off.numel() - 1
        scores = torch.empty((B, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((B, k), dtype=torch.int64, device=self.device)
        exact = torch.empty((B, k), dtype=torch.float64, device=self.device) if want_exact else None
        with self._lock, torch.cuda.device(self.device):
            need = self.lib.rf_sparse_search_workspace_bytes(self.handle, B, k)
            if need == 0:
                raise ValueError(f"BM25 search: batch of {B} queries with k = {k} is out of range")
            if self.workspace is None or self.workspace.numel() < need:
                # (the old one is released in stream order: a search already enqueued still owns it)
                self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.rf_sparse_search(self.handle, _ptr(filt), _ptr(q_off), _ptr(q_term), _ptr(q_weight),
                                                 B, k, id_base, _ptr(scores), _ptr(ids), _ptr(exact),
                                                 _ptr(self.workspace), self.workspace.numel(),
                                                 _lib.current_stream_ptr()))
        return scores, ids, exact


def fuse_rrf(arm_ids, k: int, weights=None, rrf_k: float = 60.0):
    """Enqueue rf_fuse_rrf on the current stream: arm_ids int64 [A, B, F] on the device (-1 =
    padding) -> (scores f32 [B,k], ids i64 [B,k], fused f64 [B,k]) on the device."""
    torch = _torch()
    if arm_ids.dim() != 3 or arm_ids.dtype != torch.int64:
        raise ValueError("fuse_rrf expects int64 [A, B, F] ids")
    arm_ids = arm_ids.contiguous()
    A, B, F = arm_ids.shape
    if weights is not None and len(weights) != A:
        raise ValueError(f"fuse_rrf: {len(weights)} weights for {A} arms")
    w = None if weights is None else (ctypes.c_double * A)(*[float(x) for x in weights])
    dev = arm_ids.device
    scores = torch.empty((B, k), dtype=torch.float32, device=dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    fused = torch.empty((B, k), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load_library().rf_fuse_rrf(A, _ptr(arm_ids), F, w, float(rrf_k), B, k, _ptr(scores), _ptr(ids),
                                                   _ptr(fused), _lib.current_stream_ptr()))
    return scores, ids, fused


BOOST_MAX = _lib.RF_BOOST_MAX   # boosts of one search (include/ragfin.h, "boosted search")


def boost_classes(filters, n_rows: int, base=None):
    """Enqueue rf_boost_classes on the current stream: m = 1..3 filter buffers built for n_rows (and
    the base filter's buffer, or None) -> (class masks int32 [2^m, stride] on the device, in the mask
    format of rf_filter_from_mask, the rows of every class int64 [2^m] on the device)."""
    torch = _torch()
    lib = _lib.load_library()
    filters = list(filters)
    m = len(filters)
    if not 1 <= m <= BOOST_MAX:
        raise ValueError(f"boost_classes: 1..{BOOST_MAX} boost filters, got {m}")
    stride = lib.rf_boost_class_stride_words(int(n_rows))
    if stride == 0:
        raise ValueError(f"boost_classes: no class masks for {n_rows} rows")
    dev = filters[0].device
    with torch.cuda.device(dev):
        masks = torch.empty((1 << m, stride), dtype=torch.int32, device=dev)
        counts = torch.empty((1 << m,), dtype=torch.int64, device=dev)
        ptrs = (c_void_p * m)(*[c_void_p(f.data_ptr()) for f in filters])
        _lib.check(lib.rf_boost_classes(_ptr(base), ptrs, m, int(n_rows), _ptr(masks), _ptr(counts),
                                        _lib.current_stream_ptr()))
    return masks, counts


def merge_boosted(cand_exact, cand_ids, class_weights, k: int):
    """Enqueue rf_merge_boosted on the current stream: the class answers fp64 / int64 [B, C, k_in] on
    the device (an id < 0 = padding) and the C class weights (host floats) -> (scores f32 [B,k],
    ids i64 [B,k], boosted f64 [B,k], base f64 [B,k]) on the device."""
    torch = _torch()
    if cand_ids.dim() != 3 or cand_ids.dtype != torch.int64 or cand_exact.dtype != torch.float64 or \
            cand_exact.shape != cand_ids.shape:
        raise ValueError("merge_boosted expects fp64 scores and int64 ids, both [B, C, k_in]")
    cand_exact, cand_ids = cand_exact.contiguous(), cand_ids.contiguous()
    B, C, k_in = cand_ids.shape
    if len(class_weights) != C:
        raise ValueError(f"merge_boosted: {len(class_weights)} weights for {C} classes")
    w = (ctypes.c_double * C)(*[float(x) for x in class_weights])
    dev = cand_ids.device
    scores = torch.empty((B, k), dtype=torch.float32, device=dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    boosted = torch.empty((B, k), dtype=torch.float64, device=dev)
    base = torch.empty((B, k), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load_library().rf_merge_boosted(_ptr(cand_exact), _ptr(cand_ids), B, C, k_in, w, k, _ptr(scores),
                                                        _ptr(ids), _ptr(boosted), _ptr(base),
                                                        _lib.current_stream_ptr()))
    return scores, ids, boosted, base


def decay_weights(column, ranker):
    """Enqueue rf_decay_weights on the current stream: the row weights of `ranker` (a ranker.DecayRanker) over
    `column`, an int64 or float64 device tensor [n] -> (w32 float32 [n], w64 float64 [n]) on its device, bit for
    bit ranker.decay_weights_reference and its float32 rounding."""
    torch = _torch()
    if not torch.is_tensor(column) or column.dim() != 1 or column.dtype not in (torch.int64, torch.float64):
        raise ValueError("decay_weights expects an int64 or float64 device tensor [n]")
    column = column.contiguous()
    n = column.numel()
    dev = column.device
    with torch.cuda.device(dev):
        w64 = torch.empty((n,), dtype=torch.float64, device=dev)
        w32 = torch.empty((n,), dtype=torch.float32, device=dev)
        if n:
            _lib.check(_lib.load_library().rf_decay_weights(
                _ptr(column), 1 if column.dtype == torch.int64 else 0, n, int(ranker.function_code), float(ranker.origin),
                float(ranker.scale), float(ranker.offset), float(ranker.shape), _ptr(w64), _ptr(w32),
                _lib.current_stream_ptr()))
    return w32, w64


def filter_from_mask(words, n_rows: int):
    """rf_filter_from_mask of mask words (int32 [>= ceil(n_rows / 32)] on the device, contiguous) into a
    fresh filter buffer, enqueued on the current stream."""
    torch = _torch()
    lib = _lib.load_library()
    with torch.cuda.device(words.device):
        buf = torch.empty(lib.rf_filter_bytes(n_rows), dtype=torch.uint8, device=words.device)
        _lib.check(lib.rf_filter_from_mask(_ptr(words), n_rows, _ptr(buf), _lib.current_stream_ptr()))
    return buf


def text_words_per_leaf(n_rows: int) -> int:
    """Words of one keyword leaf's bitmap (SparseIndex.text_match)."""
    return ((n_rows + 31) // 32 + 3) // 4 * 4


def column_match(device, program: "filter_expr.Program", extra_columns: dict, n_rows: int, out=None):
    """rf_column_match of program.column_leaves, enqueued on the current stream; no host sync.
    extra_columns: field -> its device column (int32 codes | int64 | fp64, [n_rows]).  -> the row bitmaps,
    an int32 device tensor [C * ceil(n_rows / 32)] of uint32 bit patterns, leaf after leaf (`out`: a
    contiguous int32 tensor of that size to write into).  One launch per RF_COLUMN_MAX_LEAVES leaves."""
    torch = _torch()
    lib = _lib.load_library()
    C = len(program.column_leaves)
    nwords = (n_rows + 31) // 32
    ptrs = {f: (c_void_p(t.data_ptr()) if t.numel() else None) for f, t in extra_columns.items()}
    arr, words, values = filter_expr.column_leaf_arrays(program, ptrs)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty(C * nwords, dtype=torch.int32, device=device)
        elif out.numel() != C * nwords or out.dtype != torch.int32 or not out.is_contiguous():
            raise ValueError(f"column_match: out must be a contiguous int32 tensor of {C * nwords} words")
        cs_d = torch.from_numpy(words.view(np.int32)).to(device) if words.size else None
        vs_d = torch.from_numpy(values).to(device) if values.size else None
        step = _lib.RF_COLUMN_MAX_LEAVES
        for c0 in range(0, C, step):
            c1 = min(C, c0 + step)
            part = (_lib.ColumnLeaf * (c1 - c0)).from_buffer(arr, c0 * ctypes.sizeof(_lib.ColumnLeaf))
            _lib.check(lib.rf_column_match(part, c1 - c0, _ptr(cs_d), _ptr(vs_d), n_rows,
                                           c_void_p(out.data_ptr() + 4 * c0 * nwords) if nwords else None,
                                           _lib.current_stream_ptr()))
    # (cs_d / vs_d may be freed now: the caching allocator reuses their memory in stream order)
    return out


def dynamic_match(device, program: "filter_expr.Program", columns: dict, n_rows: int, out=None):
    """rf_dynamic_match of program.dynamic_leaves, enqueued on the current stream; no host sync.
    columns: dynamic key -> (tags uint8 [n_rows], payload int64 [n_rows]) on the device.  -> the row bitmaps, an
    int32 device tensor [D * ceil(n_rows / 32)] of uint32 bit patterns, leaf after leaf (`out`: a contiguous
    int32 tensor of that size to write into).  One launch per RF_DYNAMIC_MAX_LEAVES leaves."""
    torch = _torch()
    lib = _lib.load_library()
    D = len(program.dynamic_leaves)
    nwords = (n_rows + 31) // 32
    ptrs = {k: ((t.data_ptr(), p.data_ptr()) if t.numel() else (None, None)) for k, (t, p) in columns.items()}
    arr, words, ints, floats = filter_expr.dynamic_leaf_arrays(program, ptrs)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty(D * nwords, dtype=torch.int32, device=device)
        elif out.numel() != D * nwords or out.dtype != torch.int32 or not out.is_contiguous():
            raise ValueError(f"dynamic_match: out must be a contiguous int32 tensor of {D * nwords} words")
        cs_d = torch.from_numpy(words.view(np.int32)).to(device) if words.size else None
        is_d = torch.from_numpy(ints).to(device) if ints.size else None
        fs_d = torch.from_numpy(floats).to(device) if floats.size else None
        step = _lib.RF_DYNAMIC_MAX_LEAVES
        for d0 in range(0, D, step):
            d1 = min(D, d0 + step)
            part = (_lib.DynamicLeaf * (d1 - d0)).from_buffer(arr, d0 * ctypes.sizeof(_lib.DynamicLeaf))
            _lib.check(lib.rf_dynamic_match(part, d1 - d0, _ptr(cs_d), _ptr(is_d), _ptr(fs_d), n_rows,
                                            c_void_p(out.data_ptr() + 4 * d0 * nwords) if nwords else None,
                                            _lib.current_stream_ptr()))
    # (the sets may be freed now: the caching allocator reuses their memory in stream order)
    return out


def array_match(device, program: "filter_expr.Program", columns: dict, n_rows: int, out=None):
    """rf_array_match of program.array_leaves, enqueued on the current stream; no host sync.
    columns: ARRAY field -> (offsets int64 [n_rows + 1], values int32 codes | int64 | fp64) on the device.  -> the
    row bitmaps, an int32 device tensor [A * ceil(n_rows / 32)] of uint32 bit patterns, leaf after leaf (`out`: a
    contiguous int32 tensor of that size to write into).  One launch per RF_ARRAY_MAX_LEAVES leaves."""
    torch = _torch()
    lib = _lib.load_library()
    A = len(program.array_leaves)
    nwords = (n_rows + 31) // 32
    # (a field whose rows are all empty has no element to point at: its offsets stand in, and none is read)
    ptrs = {f: (o.data_ptr(), v.data_ptr() if v.numel() else o.data_ptr()) for f, (o, v) in columns.items()}
    arr, words, values, floats = filter_expr.array_leaf_arrays(program, ptrs)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty(A * nwords, dtype=torch.int32, device=device)
        elif out.numel() != A * nwords or out.dtype != torch.int32 or not out.is_contiguous():
            raise ValueError(f"array_match: out must be a contiguous int32 tensor of {A * nwords} words")
        cs_d = torch.from_numpy(words.view(np.int32)).to(device) if words.size else None
        vs_d = torch.from_numpy(values).to(device) if values.size else None
        fs_d = torch.from_numpy(floats).to(device) if floats.size else None
        step = _lib.RF_ARRAY_MAX_LEAVES
        for a0 in range(0, A, step):
            a1 = min(A, a0 + step)
            part = (_lib.ArrayLeaf * (a1 - a0)).from_buffer(arr, a0 * ctypes.sizeof(_lib.ArrayLeaf))
            _lib.check(lib.rf_array_match(part, a1 - a0, _ptr(cs_d), _ptr(vs_d), _ptr(fs_d), n_rows,
                                          c_void_p(out.data_ptr() + 4 * a0 * nwords) if nwords else None,
                                          _lib.current_stream_ptr()))
    # (the sets may be freed now: the caching allocator reuses their memory in stream order)
    return out


def array_first_occurrence(device, offsets, values, row_lo: int, row_hi: int, flags) -> None:
    """rf_array_first_occurrence over rows [row_lo, row_hi) of a CSR mirror of int32 codes, enqueued on the current
    stream: flags (uint8, one per element) gets 1 where no earlier element of the row holds the same code."""
    torch = _torch()
    lib = _lib.load_library()
    if row_hi == row_lo or not values.numel():
        return
    with torch.cuda.device(device):
        _lib.check(lib.rf_array_first_occurrence(_ptr(offsets), _ptr(values), row_lo, row_hi, _ptr(flags),
                                                 _lib.current_stream_ptr()))


def facet_stats_slots(spec: dict, limit: int) -> int:
    """The slots rf_facet_stats gives a field: min(limit, its value bins)."""
    return min(limit, spec["n_codes"] + (2 if spec["kind"] == _lib.RF_FACET_DYNAMIC else 0))


def _stats_metrics(metrics: list, n_rows: int):
    """The rf_stats_metric array of [(int64 / fp64 device tensor [>= n_rows], is_f64), ...]."""
    torch = _torch()
    if not 1 <= len(metrics) <= _lib.RF_STATS_MAX_METRICS:
        raise ValueError(f"facet stats: 1..{_lib.RF_STATS_MAX_METRICS} metrics per call, got {len(metrics)}")
    marr = (_lib.StatsMetric * len(metrics))()
    for i, (col, is_f64) in enumerate(metrics):
        if col.dtype != (torch.float64 if is_f64 else torch.int64) or col.numel() < n_rows or not col.is_contiguous():
            raise ValueError(f"facet stats: metric {i} must be a contiguous {'fp64' if is_f64 else 'int64'} tensor of "
                             f"{n_rows} rows")
        marr[i].column_dev, marr[i].is_f64 = col.data_ptr(), 1 if is_f64 else 0
    return marr


def _facet_stats(lib, device, filt, arr, n_fields: int, marr, slot_of, n_counters: int, limit: int, n_rows: int, grid: int):
    """rf_facet_stats + rf_facet_stats_finish on the current stream -> the finished records, on the device."""
    torch = _torch()
    M = len(marr)
    n_records = lib.rf_facet_stats_records(arr, n_fields, M, limit)
    if n_records < 1:
        raise ValueError("facet stats: bad arguments")
    acc = torch.empty(n_records * _lib.RF_STATS_WORDS, dtype=torch.int64, device=device)
    out = torch.empty((n_records, _lib.RF_STATS_OUT), dtype=torch.int64, device=device)
    st = _lib.current_stream_ptr()
    _lib.check(lib.rf_facet_stats(_ptr(filt), arr, n_fields, marr, M, _ptr(slot_of), n_counters, limit, n_rows, _ptr(acc),
                                  n_records, grid, st))
    _lib.check(lib.rf_facet_stats_finish(_ptr(acc), marr, M, n_records, _ptr(out), st))
    return out


def facet_stats_all(device, filt, metrics: list, n_rows: int, grid: int = 0) -> np.ndarray:
    """The metric aggregations of all the rows `filt` passes (None: every row): rf_facet_stats with its one-slot
    group alone -- no value field, no select -- then rf_facet_stats_finish and ONE download.  metrics: [(int64 /
    fp64 device tensor [n_rows], is_f64), ...].  -> int64 [len(metrics), RF_STATS_OUT]: {count, nan, sum bits |
    limb 0, limb 1, min, max, 0, 0} per metric.  grid: workgroups (0: the default)."""
    torch = _torch()
    lib = _lib.load_library()
    marr = _stats_metrics(metrics, n_rows)
    with torch.cuda.device(device):
        return _facet_stats(lib, device, filt, None, 0, marr, None, 0, 1, n_rows, grid).cpu().numpy()


def facet_counts(device, filt, specs: list, n_rows: int, limit: int, min_count: int, metrics=None, grid: int = 0):
    """rf_facet_counts + rf_facet_select of one facets() call: one launch each for all fields, on the current
    stream, then ONE download.  filt: a filter buffer for n_rows rows, or None (every row).  specs: per field
    {"kind": RF_FACET_*, "n_codes": dictionary size, "a" / "b" / "c": the device tensors rf_facet_field names (None
    where unused), "rank": int32 device tensor [n_bins]}.  -> int64 [len(specs), RF_FACET_SCALARS + 2 * limit]:
    per field the scalars {selected, distinct, selected sum, missing, sum of all bins, ...}, the selected counts and
    their bin numbers, best first.  Buffers are allocated per call.
    metrics: [(int64 / fp64 device tensor [n_rows], is_f64), ...] adds rf_facet_stats_slots, rf_facet_stats and
    rf_facet_stats_finish behind the select, on the same stream and without a host round trip, and returns
    (the array above, int64 [records, RF_STATS_OUT]): per field facet_stats_slots(spec, limit) slots of one record
    per metric, in bucket order, then one record per metric over all passing rows.  grid: the stats launch's
    workgroups per column (0: the default)."""
    torch = _torch()
    lib = _lib.load_library()
    F = len(specs)
    if not 1 <= F <= _lib.RF_FACET_MAX_FIELDS:
        raise ValueError(f"facet_counts: 1..{_lib.RF_FACET_MAX_FIELDS} fields per call, got {F}")
    arr = (_lib.FacetField * F)()
    with torch.cuda.device(device):
        n_counters = 0
        for i, s in enumerate(specs):
            n_bins = s["n_codes"] + (2 if s["kind"] == _lib.RF_FACET_DYNAMIC else 0)
            if s["rank"].numel() != n_bins or s["rank"].dtype != torch.int32 or not s["rank"].is_contiguous():
                raise ValueError(f"facet_counts: field {i}: rank must be a contiguous int32 tensor of {n_bins} bins")
            arr[i].kind, arr[i].n_codes, arr[i].counter_off = s["kind"], s["n_codes"], n_counters
            a, b, c = s.get("a"), s.get("b"), s.get("c")
            arr[i].a_dev = a.data_ptr() if a is not None else None
            # (an ARRAY field whose rows are all empty has no element to point at: its offsets stand in, none is read)
            arr[i].b_dev = None if b is None else (b.data_ptr() if b.numel() else a.data_ptr())
            arr[i].c_dev = None if c is None else (c.data_ptr() if c.numel() else a.data_ptr())
            arr[i].rank_dev = s["rank"].data_ptr() if n_bins else None
            n_counters += n_bins + 1
        counters = torch.empty(n_counters, dtype=torch.int64, device=device)
        out = torch.empty((F, _lib.RF_FACET_SCALARS + 2 * limit), dtype=torch.int64, device=device)
        st = _lib.current_stream_ptr()
        _lib.check(lib.rf_facet_counts(_ptr(filt), arr, F, n_rows, _ptr(counters), n_counters, st))
        _lib.check(lib.rf_facet_select(arr, F, _ptr(counters), n_counters, limit, min_count, _ptr(out), st))
        if metrics is None:
            return out.cpu().numpy()
        marr = _stats_metrics(metrics, n_rows)
        slot_of = torch.empty(n_counters, dtype=torch.int32, device=device)
        _lib.check(lib.rf_facet_stats_slots(arr, F, _ptr(out), limit, _ptr(slot_of), n_counters, st))
        stats = _facet_stats(lib, device, filt, arr, F, marr, slot_of, n_counters, limit, n_rows, grid)
        return out.cpu().numpy(), stats.cpu().numpy()


def facet_ranges(device, filt, column, is_f64: bool, bounds: list, n_rows: int) -> np.ndarray:
    """rf_facet_ranges of one numeric column (int64 or fp64 device tensor [n_rows]) on the current stream.  bounds:
    per range (no_lo, no_hi, empty, lo, hi), lo / hi ints for an int64 column and floats for an fp64 one.
    -> int64 [RF_FACET_MAX_RANGES + 4]: the range counts, then {NaN rows, non-NaN rows, min bits, max bits}."""
    torch = _torch()
    lib = _lib.load_library()
    arr = (_lib.FacetRange * len(bounds))()
    for i, (no_lo, no_hi, empty, lo, hi) in enumerate(bounds):
        arr[i].flags = (_lib.RF_FRANGE_NO_LO if no_lo else 0) | (_lib.RF_FRANGE_NO_HI if no_hi else 0) | \
            (_lib.RF_FRANGE_EMPTY if empty else 0)
        if is_f64:
            arr[i].flo, arr[i].fhi = lo, hi
        else:
            arr[i].ilo, arr[i].ihi = lo, hi
    with torch.cuda.device(device):
        out = torch.empty(_lib.RF_FACET_MAX_RANGES + 4, dtype=torch.int64, device=device)
        _lib.check(lib.rf_facet_ranges(_ptr(filt), _ptr(column), 1 if is_f64 else 0, arr, len(bounds), n_rows, _ptr(out),
                                       _lib.current_stream_ptr()))
        return out.cpu().numpy()


def eval_filter(device, program: "filter_expr.Program", columns, n_rows: int, bitmaps=None, column_base: int = 0):
    """rf_filter_eval of a compiled program into a fresh filter buffer (uint8 device tensor of
    rf_filter_bytes(n_rows)), enqueued on the current stream.  columns: the device tensors
    {period, chunk_type, statement_type codes int32 [n_rows], primary_value fp64 [n_rows]}.
    bitmaps: SparseIndex.text_match(program.text_leaves), enqueued on the same stream, when the
    program has keyword leaves (rf_filter_eval_bitmaps).  With column leaves (program.column_leaves),
    bitmaps is the one flat int32 array that holds the keyword leaves' bitmaps (text_words_per_leaf(n_rows)
    words each) and, from word column_base, the column leaves' (column_match; ceil(n_rows / 32) words each) and
    behind them the dynamic leaves' (program.dynamic_leaves; dynamic_match, the same width) and the array leaves'
    (program.array_leaves; array_match, the same width)."""
    torch = _torch()
    lib = _lib.load_library()
    cs, rl = filter_expr.program_arrays(program)
    if program.column_leaves or program.dynamic_leaves or program.array_leaves:
        ops = program.ops_ctypes(text_words_per_leaf(n_rows), column_base, (n_rows + 31) // 32)
        if column_base + (len(program.column_leaves) + len(program.dynamic_leaves) + len(program.array_leaves)) * \
                ((n_rows + 31) // 32) > 0x7FFFFFFF:
            raise ValueError("filter expression: the leaves' bitmaps do not fit int32 word offsets")
    else:
        ops = program.ops_ctypes(0 if bitmaps is None else int(bitmaps.shape[1]))
    with torch.cuda.device(device):
        buf = torch.empty(lib.rf_filter_bytes(n_rows), dtype=torch.uint8, device=device)
        cs_d = torch.from_numpy(cs.view(np.int32)).to(device) if cs.size else None
        rl_d = torch.from_numpy(rl.view(np.int32)).to(device) if rl.size else None
        ptrs = (c_void_p * _lib.RF_FILTER_COLUMNS)(*[c_void_p(t.data_ptr()) if t is not None and t.numel() else None
                                                     for t in columns])
        _lib.check(lib.rf_filter_eval_bitmaps(ops, len(ops), c_void_p(cs_d.data_ptr()) if cs_d is not None else None,
                                              c_void_p(rl_d.data_ptr()) if rl_d is not None else None, _ptr(bitmaps),
                                              ptrs, n_rows, c_void_p(buf.data_ptr()), _lib.current_stream_ptr()))
    # (cs_d / rl_d may be freed now: the caching allocator reuses their memory in stream order)
    return buf


def filter_mask_bits(buf, n_rows: int):
    """The row mask of a filter buffer as a host bool array [n_rows] (synchronises)."""
    nblk = (n_rows + 31) // 32
    words = buf[16:16 + 4 * nblk].cpu().numpy().view(np.uint32)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    return bits[:n_rows]
