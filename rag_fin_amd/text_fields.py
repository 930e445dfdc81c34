"""The fields a CorpusStore derives from its `text` column, each with an index of its own on the GPU:

  "sparse"            LexicalField         BM25 posting lists (lexical.py; DESIGN §4.4g, k, l)
  "sparse_embedding"  LearnedSparseField   SPLADE term vectors, served by a SparseIndex
  "token_embeddings"  TokenVectorField     ColBERT token vectors, a late_interaction.TokenField

The store makes one object per field for its whole life and keeps them by name (CorpusStore._text_fields); every
call that names a field looks it up and talks to it through TextField's methods.  A field reads `columns["text"]`,
`num_entities`, `index.device`, `analyzer` and `build_filter` of its store and builds under the store's
`_sparse_lock`, the one lock of all three (lock order: CorpusStore.build_filter).  declare / undeclare / reset and
the mutation hooks run under the store's write lock, the builds and arm() under its read side.  What a fourth
field has to provide: DESIGN §4.5h."""
from __future__ import annotations

import itertools
import os

import numpy as np

from . import _lib
from . import filter_expr
from . import lexical
from .index import SparseIndex

LEARNED_FIELD = "sparse_embedding"   # the learned sparse field (create_index(..., encoder=))
TOKEN_FIELD = "token_embeddings"     # the late-interaction field (create_index(..., encoder=))


def is_text(data) -> bool:
    return isinstance(data, str) or (isinstance(data, (list, tuple)) and len(data) > 0
                                     and all(isinstance(t, str) for t in data))


class TextField:
    """What the three fields share: the declaration and its check, the checks of a search, and the hooks the
    store calls.  The messages are each field's own: where they differ, the difference is class data."""

    name = index_type = metric_type = None
    form = None                   # "BM25": the messages say "<form> search" and "no <form> form"
    encoder_attrs = ()            # what create_index(encoder=) must have; (): the field takes no encoder
    encoder_hint = None           # ... and how the refusal names it
    data_first = False            # a search looks at the data before the metric (else last)
    refuses_param_offset = True   # a search refuses param["offset"] itself (hybrid arms: nothing else looks)
    bad_limit = "limit must be an integer >= 1"
    big_limit = "{form} search: limit = {limit} > {max} (the sparse arm is not paged)"

    def __init__(self, store):
        self.store = store
        self.params = None        # what check_params made of the declaration (None: not declared)
        self.reset()              # `built`: what the field built from the rows (None: to be built)

    declared = property(lambda self: self.params is not None)
    where = property(lambda self: f"{self.form} search (anns_field='{self.name}')")   # as the refusals say it

    # -- create_index / drop_index / drop and the mutations (caller holds the write lock) -----------------------
    def check_params(self, index_params: dict, encoder=None) -> dict:
        """Everything create_index refuses for the field -> what declare() keeps."""
        itype = str(index_params.get("index_type", self.index_type)).upper()
        if itype != self.index_type:
            raise ValueError(f"create_index: the {self.name} field takes index_type {self.index_type}, got {itype!r}")
        metric = str(index_params.get("metric_type", self.metric_type)).upper()
        if metric != self.metric_type:
            raise ValueError(f"create_index: the {self.name} field takes metric_type {self.metric_type}, got {metric!r}")
        p = index_params.get("params")
        if p is not None and not isinstance(p, dict):
            raise ValueError("create_index: params must be a dict")
        if self.encoder_attrs and (encoder is None or not all(hasattr(encoder, a) for a in self.encoder_attrs)):
            raise ValueError(f"create_index: the {self.name} field is derived from the text column and needs "
                             f"encoder={self.encoder_hint}")
        return {"encoder": encoder}

    def declare(self, params) -> None:
        """create_index with what check_params returned; drop_index with None."""
        self.params = params
        self.reset()

    def reset(self) -> None:
        """Forget what was built (drop(), and a new or dropped declaration); the declaration stays."""
        self.built = None

    def rows_appended(self, texts) -> None:
        """Rows with these texts are about to be appended."""

    def rows_deleted(self, keep_mask) -> None:
        """The rows not set in keep_mask (bool [num_entities]) are about to go (a replaced row: before its append)."""

    # -- search ----------------------------------------------------------------------------------------------------
    def refuse_forms(self, offset: int, other: bool) -> None:
        """search() was given an offset, or (other) grouping or MMR arguments."""
        if offset or other:
            raise ValueError(f"{self.where} has no offset, grouping or MMR form")

    def check_search(self, data, param, limit):
        """Everything a search of the field refuses -> its queries, as queries() gives them."""
        if not self.declared:
            encoder = ", encoder=..." if self.encoder_attrs else ""
            raise ValueError(f"no {self.name} index: call create_index('{self.name}', {{'index_type': "
                             f"'{self.index_type}', 'metric_type': '{self.metric_type}'}}{encoder}) first")
        q = self.queries(data) if self.data_first else None
        metric = str((param or {}).get("metric_type", self.metric_type)).upper()
        if metric != self.metric_type:
            raise ValueError(f"the {self.name} field is searched with metric_type {self.metric_type}, search asked for {metric}")
        params = (param or {}).get("params")
        if params is not None and not isinstance(params, dict):
            raise ValueError("search: param['params'] must be a dict")
        if params and (params.get("radius") is not None or params.get("range_filter") is not None):
            raise ValueError(f"{self.where} has no range form (radius / range_filter)")
        if self.refuses_param_offset and isinstance(param, dict) and param.get("offset"):
            raise ValueError(f"{self.where} takes no offset")
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or limit < 1:
            raise ValueError(self.bad_limit)
        if limit > _lib.RF_MAX_K:
            raise ValueError(self.big_limit.format(form=self.form, limit=limit, max=_lib.RF_MAX_K))
        return self.queries(data) if q is None else q

    def queries(self, data):
        """The data of a search, in a form the field accepts -> the queries arm() takes; else ValueError."""
        raise NotImplementedError

    def query_count(self, q) -> int:
        return len(q)

    def arm(self, q, limit: int, expr):
        """The search on the device -> (scores f32 [B, limit], rows i64 [B, limit]) tensors, or None when
        nothing can hit.  Caller holds the read lock."""
        raise NotImplementedError

    def _filt(self, expr) -> dict:
        return {} if filter_expr.is_empty(expr) else {"filt": self.store.build_filter(expr)}


class LexicalField(TextField):
    """create_index("sparse", ...): the BM25 posting lists over the text column, built by the first BM25 search
    or keyword filter after a change of the rows (`built`: None = to be built)."""

    name, index_type, metric_type, form = "sparse", "SPARSE_INVERTED_INDEX", "BM25", "BM25"
    data_first = True
    refuses_param_offset = False

    fallback_reason = None   # why the device route last gave way to the host's (None: it never did)
    route = "host"           # what built the retained index whole: "host" or "device" 

    def check_params(self, index_params, encoder=None) -> dict:
        super().check_params(index_params)
        p = index_params.get("params") or {}
        k1, b = lexical.check_bm25_params(p.get("bm25_k1", lexical.DEFAULT_K1), p.get("bm25_b", lexical.DEFAULT_B))
        return {"bm25_k1": k1, "bm25_b": b}

    def reset(self) -> None:
        super().reset()   # built: (postings, SparseIndex | None); the token positions a PHRASE_MATCH filter needs
        self.forget()     # live on that SparseIndex: attached once, by the first such filter, and gone with it

    # index maintenance: the last built (postings, SparseIndex, analyzer, params) and, in order,
    # the mutations since -- ("delete", keep mask) / ("append", texts) -- which the next index() replays through
    # SparseIndex.compacted / .appended instead of building whole.  Written under the write lock, replayed under
    # `_sparse_lock` with the read side held.
    def forget(self) -> None:
        """Drop the retained lexical state: the next index() builds whole."""
        self.kept = None
        self.log = []

    def _log(self, kind: str, arg) -> None:
        """Record a mutation for the next replay (caller holds the write lock).  A log longer than
        LEXICAL_LOG_MAX is not worth replaying step by step: the state is dropped."""
        self.built = None   # the index is brought up to date by the next BM25 search
        if self.kept is None:
            return
        if len(self.log) >= self.store.LEXICAL_LOG_MAX:
            self.forget()
            return
        self.log.append((kind, arg))

    def rows_appended(self, texts) -> None:
        self._log("append", list(texts))

    def rows_deleted(self, keep_mask) -> None:
        self._log("delete", keep_mask)

    def refuse_forms(self, offset, other) -> None:
        if other and not offset:   # (an offset: search() refuses it next, in the words it has for the dense field's)
            raise ValueError("BM25 search (anns_field='sparse') has no grouping and no MMR form")

    def queries(self, data) -> list:
        if not is_text(data):
            raise ValueError("the sparse field is searched with query strings (a list of str), not with vectors")
        return [data] if isinstance(data, str) else list(data)

    def index(self):
        """(postings, SparseIndex | None) over the current text column.  After a mutation the last one
        is brought up to date on the GPU (_replay); it is built whole the first
        time and whenever there is nothing to replay from -- on the device (_build_device), or on
        the host with a custom analyzer, with RAGFIN_LEXICAL_BUILD=host or when the device route raised.
        None: no row holds a term.  Caller holds the read lock."""
        st = self.store
        with st._sparse_lock:
            if self.built is None:
                p = self.params
                built = self._replay((p["bm25_k1"], p["bm25_b"]))
                if built is None:
                    built = self._build_device(p["bm25_k1"], p["bm25_b"])
                    self.route = "device" if built is not None else "host"
                if built is None:
                    postings = lexical.build_postings(st.columns["text"], p["bm25_k1"], p["bm25_b"], st.analyzer)
                    built = (postings, SparseIndex(postings, st.index.device) if postings.nnz else None)
                self.log = []
                self.kept = None
                if built[1] is not None and getattr(built[1], "supports_update", False):
                    self.kept = (built[0], built[1], st.analyzer, (p["bm25_k1"], p["bm25_b"]))
                self.built = built   # (published whole: a replay that raised left nothing behind)
            return self.built

    def _build_route(self) -> str:
        """"device" or "host" for a whole build of the lexical index: RAGFIN_LEXICAL_BUILD=host|device|auto
        (default auto: the device for every non-empty corpus -- it was the faster route at every size
        measured, 10 k rows included: DESIGN §5.0m).  A custom analyzer and an empty corpus always build
        on the host."""
        want = os.environ.get("RAGFIN_LEXICAL_BUILD", "auto").strip().lower() or "auto"
        if want not in ("host", "device", "auto"):
            raise ValueError(f"RAGFIN_LEXICAL_BUILD must be host, device or auto, got {want!r}")
        n = self.store.num_entities
        if self.store.analyzer is not None or n == 0 or want == "host":
            return "host"
        return "device"

    def _build_device(self, k1, b):
        """The whole build through the native analyzer and SparseIndex.from_tokens ->
        (LivePostings, SparseIndex), or None when the route is the host's, no row holds a term, or the
        native route raised (the caller then builds on the host, exactly as before; _fell_back says so)."""
        if self._build_route() != "device":
            return None
        try:
            vocab, tok, dl = lexical.analyze_native(self.store.columns["text"])
            if tok.size == 0:
                return None
            sp = SparseIndex.from_tokens(len(vocab), tok, dl, k1, b, self.store.index.device)
            return lexical.LivePostings(vocab, None, sp.host_post_off, dl, k1, b, sp.host_array), sp
        except Exception as e:
            if isinstance(e, ValueError) and "BM25 impacts" in str(e):   # build_postings' guard: the host build raises the same
                raise
            self._fell_back("the first build", e)
            return None

    def _fell_back(self, what: str, exc: Exception) -> None:
        """The device route raised and the host route takes over: the answers are the same, the build is
        many times slower, so it must not pass unseen -- one RuntimeWarning, and the reason
        kept in `fallback_reason` (CorpusStore.lexical_fallback_reason) for whoever looks later."""
        import warnings
        self.fallback_reason = f"{what}: {type(exc).__name__}: {exc}"
        warnings.warn(f"lexical index: the device route failed for {self.fallback_reason}; building on the host",
                      RuntimeWarning, stacklevel=3)   # (the caller of _build_device / _attach_positions_device)

    def _replay(self, params):
        """The pending mutations applied to the retained index, in order, through SparseIndex.compacted /
        .appended -> (postings, SparseIndex), or None when there is nothing to replay from, the retained
        state was built with other parameters or another analyzer, no posting survives, or a step raised
        (the caller then builds whole).  The analyzer sees the appended texts only, once."""
        kept, analyzer = self.kept, self.store.analyzer
        if kept is None or kept[2] is not analyzer or kept[3] != params:
            return None
        postings, sp = kept[0], kept[1]
        k1, b = params
        try:
            vocab, term_id, post_off, dl = postings.vocab, postings.term_id, postings.post_off, postings.dl
            for kind, arg in self.log:
                if kind == "delete":
                    row_map = np.where(arg, np.cumsum(arg) - 1, -1).astype(np.int32)
                    dl = dl[arg]
                    sp, alive, post_off = sp.compacted(row_map, dl, k1, b)
                    if sp is None:
                        return None
                    if not alive.all():
                        vocab, term_id = list(itertools.compress(vocab, alive.tolist())), None
                else:
                    delta = lexical.count_terms(arg, analyzer)
                    if term_id is None:
                        term_id = {t: i for i, t in enumerate(vocab)}
                    merged, map_old, map_delta = lexical.merge_vocab(vocab, term_id, delta.vocab)
                    if merged is not vocab:
                        vocab, term_id = merged, None
                    post_off = lexical.merged_offsets(len(vocab), post_off, map_old, delta.post_off, map_delta)
                    dl = np.concatenate([dl, delta.dl])
                    sp = sp.appended(delta, map_old, map_delta, post_off, dl, k1, b)
            if dl.size != self.store.num_entities:
                return None
            return lexical.LivePostings(vocab, term_id, post_off, dl, k1, b, sp.host_array), sp
        except Exception:   # a half-updated index is never published: the caller builds whole
            return None

    def arm(self, texts, limit: int, expr):
        postings, sp = self.index()
        if sp is None:   # no row holds a term
            return None
        q_off, q_term, q_weight = lexical.encode_queries(postings, texts, self.store.analyzer)
        scores, rows, _ = sp.search(q_off, q_term, q_weight, limit, want_exact=False, **self._filt(expr))
        return scores, rows

    def text_index(self, leaves):
        """What the keyword leaves of a filter need -> (term -> id map, SparseIndex), (None, None)
        without such leaves.  No postings at all (no row holds a term): an empty map and no index,
        so every leaf compiles to RF_FOP_FALSE."""
        if not leaves:
            return None, None
        if not self.declared:
            raise ValueError("filter expression: " + filter_expr.NO_LEXICAL_INDEX)
        postings, sp = self.index()
        if sp is not None and any(isinstance(n, filter_expr.PhraseMatch) for n in leaves):
            with self.store._sparse_lock:
                if sp.positions is None and not self._attach_positions_device(postings, sp):
                    sp.attach_positions(*lexical.build_positions(postings, self.store.columns["text"], self.store.analyzer))
        return postings.term_id, sp

    def _attach_positions_device(self, postings, sp) -> bool:
        """The token positions of an index that came from the device route, through the device route again
        (native analysis, rf_sparse_count_* with positions); False: not that route, or it raised, and the
        caller builds them on the host.  The stream must give the index's own dictionary and postings."""
        if self.route != "device" or self.store.analyzer is not None:
            return False
        try:
            vocab, tok, dl = lexical.analyze_native(self.store.columns["text"])
            if vocab != postings.vocab:
                raise ValueError("the native analysis does not give the dictionary of the index")
            sp.attach_token_positions(tok, dl)
            return True
        except Exception as e:
            self._fell_back("the token positions", e)
            return False


class LearnedSparseField(TextField):
    """create_index("sparse_embedding", ..., encoder=): the per-row term vectors of the rows encoded so far as host
    CSR (`rows`: indptr int64, indices int32, data fp32 -- a prefix of the rows; the rest is encoded by the next
    search) and the (TermPostings, SparseIndex | None) over them (`built`: None = to be transposed again)."""

    name, index_type, metric_type, form = LEARNED_FIELD, "SPARSE_INVERTED_INDEX", "IP", "learned sparse"
    encoder_attrs = ("encode_document", "encode_query", "vocab_size")
    encoder_hint = "<a SparseEncoder> (encode_document, encode_query, vocab_size)"

    def reset(self) -> None:
        super().reset()
        self.rows = None

    def rows_appended(self, texts) -> None:
        self.built = None   # the new rows are encoded by the next search of the field

    def rows_deleted(self, keep_mask) -> None:
        """The encoded rows that go are dropped from the host CSR (rows not encoded yet are simply not there)."""
        self.built = None
        if self.rows is None:
            return
        indptr, indices, data = self.rows
        done = indptr.size - 1
        keep = np.asarray(keep_mask[:done], dtype=bool)
        counts = np.diff(indptr)
        entry = np.repeat(keep, counts)
        new_ptr = np.zeros(int(keep.sum()) + 1, dtype=np.int64)
        np.cumsum(counts[keep], out=new_ptr[1:])
        self.rows = (new_ptr, indices[entry], data[entry])

    def queries(self, data):
        """-> a list of strings (encoded with the attached encoder's encode_query) or the checked CSR batch
        (q_off, q_term, q_weight) of supplied vectors."""
        from .sparse_encoder import check_query_rows
        if is_text(data):
            return [data] if isinstance(data, str) else list(data)
        if hasattr(data, "tocsr") or (isinstance(data, (list, tuple)) and all(isinstance(r, dict) for r in data)):
            return check_query_rows(data, int(self.params["encoder"].vocab_size))
        raise ValueError("the sparse_embedding field is searched with query strings, a scipy sparse matrix or a "
                         "list of {term_id: weight} dicts")

    def query_count(self, q) -> int:
        return len(q) if isinstance(q, list) else int(q[0].size - 1)

    def postings(self):
        """(TermPostings, SparseIndex | None) over the current text column: the rows not encoded yet go through
        the attached encoder, then the per-row vectors are transposed on the host."""
        from .sparse_encoder import TermPostings
        st = self.store
        with st._sparse_lock:
            if self.built is None:
                enc = self.params["encoder"]
                V, n = int(enc.vocab_size), st.num_entities
                rows = self.rows or (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
                done = rows[0].size - 1
                if done < n:
                    new = enc.encode_document(st.columns["text"][done:n]).tocsr()
                    new.sort_indices()
                    if new.shape != (n - done, V):
                        raise ValueError(f"the sparse encoder returned {new.shape}, expected {(n - done, V)}")
                    rows = (np.concatenate([rows[0], rows[0][-1] + np.asarray(new.indptr[1:], dtype=np.int64)]),
                            np.concatenate([rows[1], np.asarray(new.indices, dtype=np.int32)]),
                            np.concatenate([rows[2], np.asarray(new.data, dtype=np.float32)]))
                    self.rows = rows
                tp = TermPostings(rows[0], rows[1], rows[2], V)
                self.built = (tp, SparseIndex(tp, st.index.device) if tp.nnz else None)
            return self.built

    def arm(self, q, limit: int, expr):
        if not (self.store.num_entities and self.query_count(q)):
            return None
        _, sp = self.postings()
        if sp is None:   # no row holds a term
            return None
        if isinstance(q, list):
            m = self.params["encoder"].encode_query(q).tocsr()
            m.sort_indices()
            q = (np.asarray(m.indptr, dtype=np.int32), np.asarray(m.indices, dtype=np.int32),
                 np.asarray(m.data, dtype=np.float32))
        scores, rows, _ = sp.search(q[0], q[1], q[2], limit, want_exact=False, **self._filt(expr))
        return scores, rows


class TokenVectorField(TextField):
    """create_index("token_embeddings", ..., encoder=): the token vectors of the rows encoded so far (`built`: a
    late_interaction.TokenField -- device CSR over a prefix of the rows, grown by doubling; the rest is encoded
    by the next search, so an append needs no hook)."""

    name, index_type, metric_type, form = TOKEN_FIELD, "EMB_LIST_FLAT", "MAX_SIM_IP", "late-interaction"
    encoder_attrs = ("encode", "dim")
    encoder_hint = "<a ColBERT> (encode(texts, is_query=), dim)"
    bad_limit = "late-interaction search (anns_field='token_embeddings'): limit must be an integer >= 1"
    big_limit = "late-interaction search (anns_field='token_embeddings'): limit = {limit} > {max}"

    def rows_deleted(self, keep_mask) -> None:
        if self.built is not None:
            self.built.keep(keep_mask)

    def queries(self, data):
        """-> a list of strings (encoded with the attached encoder, is_query=True) or the supplied list of
        [n_tok <= 32, D] arrays, checked."""
        from . import late_interaction
        if is_text(data):
            return [data] if isinstance(data, str) else list(data)
        if isinstance(data, (list, tuple)) and all(isinstance(q, np.ndarray) and q.ndim == 2 for q in data):
            try:
                late_interaction.pack_queries(list(data), int(self.params["encoder"].dim))
            except ValueError as e:
                raise ValueError(f"the token_embeddings field: {e}") from None
            return [np.asarray(q) for q in data]
        raise ValueError("the token_embeddings field is searched with query strings or a list of [n_tok, D] arrays")

    def index(self):
        """The TokenField over the current text column: the rows not encoded yet go through the attached
        encoder and are appended."""
        from . import late_interaction
        st = self.store
        with st._sparse_lock:
            enc = self.params["encoder"]
            if self.built is None:
                self.built = late_interaction.TokenField(int(enc.dim), st.index.device)
            f, n = self.built, st.num_entities
            if f.n_rows < n:
                new = enc.encode(st.columns["text"][f.n_rows:n], is_query=False)
                if len(new) != n - f.n_rows:
                    raise ValueError(f"the token encoder returned {len(new)} rows, expected {n - f.n_rows}")
                f.append(new)
            return f

    def _encoded(self, q):
        if q and isinstance(q[0], str):
            return self.params["encoder"].encode(q, is_query=True)
        return q

    def arm(self, q, limit: int, expr):
        """All-rows MaxSim of the passing rows, then the exact top-k."""
        if not self.store.num_entities or not q:
            return None
        filt = None if filter_expr.is_empty(expr) else self.store.build_filter(expr)
        return self.index().search(self._encoded(q), limit, filt)

    def _require(self) -> None:
        if not self.declared:
            raise ValueError("no token_embeddings index: call create_index('token_embeddings', ...) first")

    def vectors(self, rows) -> list:
        """CorpusStore.token_vectors.  Caller holds the read lock."""
        self._require()
        return self.index().vectors(rows)

    def rerank(self, queries, candidates):
        """CorpusStore.rerank_tokens.  Caller holds the read lock."""
        from . import late_interaction
        self._require()
        queries = [queries] if isinstance(queries, str) else list(queries)
        if len(queries) != len(candidates):
            raise ValueError(f"{len(candidates)} candidate lists for {len(queries)} queries")
        if not queries:
            return []
        scores = late_interaction.maxsim(self.index(), self._encoded(queries), [list(c) for c in candidates])
        scores = np.asarray(scores.cpu().numpy() if hasattr(scores, "cpu") else scores, dtype=np.float32)
        cut = np.cumsum([len(c) for c in candidates])[:-1]
        return np.split(scores, cut)
