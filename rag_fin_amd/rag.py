"""`VectorRAG`: the object the reference's MCP server is built around
(vector_rag_mcp/main.py:36-123; CLI twin `SimpleRAG`, retrieve.py:6-82), with the
same method names, defaults and return keys, backed by the in-process GPU
embedder + corpus store instead of sentence-transformers + a Milvus server.

The LLM generation step (Gemini, main.py:40,97) is outside this build's scope: a
`generator` callable can be plugged in.  Without one, a `reader`
(rag_fin_amd.reader.ExtractiveReader) answers with a span of a retrieved chunk; with
neither, `search_and_answer` returns the reference's own failure shape
{"error", "contexts", "context_count"}.
"""
from __future__ import annotations

import logging
import time
from typing import Callable, Sequence

logger = logging.getLogger(__name__)

OUTPUT_FIELDS = ["text", "period", "chunk_type", "statement_type", "primary_value"]

# The LLM step (Gemini, vector_rag_mcp/main.py:72-108) is out of scope; the prompt wording is
# the caller's business.  This default only lays the retrieved contexts out for a generator;
# deployments that want the reference's wording pass their own `prompt_template`
# (placeholders: {question}, {context}).
DEFAULT_PROMPT = "Question: {question}\n\nRetrieved contexts:\n{context}\n\nAnswer from the contexts only."


class VectorRAG:
    # (class-level defaults: the context dicts keep exactly the reference's keys)
    extra_output_fields: tuple = ()
    output_fields = OUTPUT_FIELDS

    def __init__(self, gemini_api_key: str | None = None, collection_name: str = "fin_chunks", *,
                 embedder=None, store=None, generator: Callable[[str], str] | None = None,
                 llm_delay_s: float = 1.0, prompt_template: str = DEFAULT_PROMPT, reranker=None, reader=None,
                 sparse_encoder=None, late_encoder=None, extra_output_fields=None, tagger=None,
                 entity_field: str | None = None):
        """embedder: .encode(list[str]) -> [n, dim] (rag_fin_amd.embedder.Embedder);
        store: rag_fin_amd.store.CorpusStore.  `gemini_api_key` is accepted for
        signature compatibility and only handed to `generator` factories upstream.
        reranker: .predict(list[(query, text)]) -> [n] scores (rag_fin_amd.reranker.CrossEncoder), the
        second stage of search(..., rerank=True).
        reader: .predict(question, list[text], top_k=1) -> [{"answer", "score", "start", "end",
        "context_index"}] (rag_fin_amd.reader.ExtractiveReader): the answer step of search_and_answer when no
        generator is set.
        sparse_encoder: .encode_document / .encode_query(list[str]) -> sparse [n, V] (rag_fin_amd.sparse_encoder.
        SparseEncoder): declared on the store as its learned sparse field ("sparse_embedding"), the arm of
        search(..., hybrid=True, lexical="learned" | "both").
        late_encoder: .encode(list[str], is_query=) -> one [n_tok, D] matrix per text (rag_fin_amd.late_interaction.
        ColBERT): declared on the store as its late-interaction field ("token_embeddings"), the second stage of
        search(..., rerank=True, rerank_with="late").
        extra_output_fields: names of the store's own fields (CorpusStore(fields=...)) whose values are added to
        the context dicts under their names; by default the keys stay exactly the reference's.  On a store with
        enable_dynamic_field a name that is no declared field is a dynamic key (None where a chunk lacks it).
        tagger / entity_field (both or neither): .tags(list[str]) -> the entity strings of each text
        (rag_fin_amd.tagger.TokenClassifier) and the ARRAY VARCHAR field of the store that holds the chunks' entities
        (service.ingest(..., tagger=, entity_field=) fills it): what search(..., match_entities=) filters on."""
        if (tagger is None) != (entity_field is None):
            raise ValueError("tagger and entity_field go together")
        self.tagger, self.entity_field = tagger, entity_field
        if embedder is None or store is None:
            raise ValueError("VectorRAG needs an embedder and a corpus store (see rag_fin_amd.service."
                             "build_rag); there is no remote Milvus/sentence-transformers fallback")
        self.similarity_model = embedder
        self.reranker = reranker
        self.reader = reader
        self.sparse_encoder = sparse_encoder
        self.collection = store
        if extra_output_fields:
            own = [f.name for f in getattr(store, "schema", ())]
            for name in extra_output_fields:
                if name not in own and not (getattr(store, "enable_dynamic_field", False) and isinstance(name, str)
                                            and name not in OUTPUT_FIELDS):
                    raise ValueError(f"extra_output_fields: {name!r} is not a field the store declares"
                                     + (f" ({', '.join(own)})" if own else ""))
            self.extra_output_fields = tuple(dict.fromkeys(extra_output_fields))
            self.output_fields = OUTPUT_FIELDS + list(self.extra_output_fields)
        if sparse_encoder is not None:
            store.create_index("sparse_embedding", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "IP"},
                               encoder=sparse_encoder)
        self.late_encoder = late_encoder
        if late_encoder is not None:
            store.create_index("token_embeddings", {"index_type": "EMB_LIST_FLAT", "metric_type": "MAX_SIM_IP"},
                               encoder=late_encoder)
        self.collection_name = collection_name
        self.generator = generator
        self.prompt_template = prompt_template
        self.llm_delay_s = llm_delay_s
        self.collection.load()
        logger.info("VectorRAG ready on collection %s (%d chunks)", collection_name,
                    self.collection.num_entities)

    # -- retrieval ---------------------------------------------------------------------
    def _contexts(self, hits) -> list[dict]:
        return [{"rank": i + 1, "text": h.entity.text, "period": h.entity.period,
                 "chunk_type": h.entity.chunk_type, "statement_type": h.entity.statement_type,
                 "primary_value": h.entity.primary_value, "score": float(h.score),
                 **{name: h.entity.get(name) for name in self.extra_output_fields}}
                for i, h in enumerate(hits)]

    @staticmethod
    def _search_param(min_score, max_score, metric: str = "COSINE") -> dict:
        """The pymilvus search param: a score cut-off becomes range search (radius = min_score,
        range_filter = max_score; max_score alone: a band with only a ceiling)."""
        param = {"metric_type": metric}
        if min_score is not None or max_score is not None:
            param["params"] = {"radius": float("-inf") if min_score is None else min_score}
            if max_score is not None:
                param["params"]["range_filter"] = max_score
        return param

    @staticmethod
    def _group_args(group_by, group_size) -> dict:
        """The store's grouping arguments; nothing when group_by is absent (the call of before)."""
        return {} if group_by is None else {"group_by_field": group_by, "group_size": group_size}

    @staticmethod
    def _mmr_args(mmr_lambda, fetch_k) -> dict:
        """The store's diversified-search arguments, each only when it was given."""
        return {name: v for name, v in (("mmr_lambda", mmr_lambda), ("mmr_fetch_k", fetch_k)) if v is not None}

    def search(self, query: str, top_k: int = 3, expr: str | None = None, min_score: float | None = None,
               max_score: float | None = None, group_by: str | None = None, group_size: int = 1,
               mmr_lambda: float | None = None, fetch_k: int | None = None, rerank: bool = False,
               hybrid: bool = False, offset: int | None = None, boost=None, lexical: str = "bm25",
               rerank_with: str = "cross", decay=None, match_entities: str | None = None) -> list[dict]:
        """Ranked context dicts, keys exactly as vector_rag_mcp/main.py:59-70.  expr: a filter
        over the scalar fields (rag_fin_amd.filter_expr), e.g. 'period == "Q1_FY2024"'.
        min_score / max_score: only chunks with min_score < score <= max_score (range search;
        the list may be shorter than top_k, or empty).
        group_by ("period", "chunk_type", "statement_type"): grouping search -- the best top_k
        groups by that field, each by its best group_size chunks, as one flat list (group after
        group, `rank` = the 1-based position in it); every dict carries the field already.
        mmr_lambda (0..1): diversified search -- the top_k chunks are picked from the best fetch_k
        (default min(64, max(20, 4 top_k))) by maximal marginal relevance, so near-copies of one
        chunk do not crowd out the rest; `rank` is the MMR order, `score` stays the relevance.
        rerank: two-stage search -- the best fetch_k chunks (same default) are scored as (query, text)
        pairs by the cross-encoder and the best top_k of them are kept; `rank` is the rerank order,
        `score` stays the cosine and `rerank_score` (only here) is the cross-encoder's.
        rerank_with (with rerank): "cross" (the default: the cross-encoder) or "late" -- the fetch_k chunks are
        scored by MaxSim of the query's token vectors against the chunks' STORED token vectors (the
        late-interaction field; no forward per candidate), the best top_k by (MaxSim descending, retrieval order)
        are kept and `rerank_score` is the MaxSim.  Needs VectorRAG(..., late_encoder=), else ValueError.
        hybrid: the dense search and a BM25 search of the chunk texts (the store needs its lexical
        index: create_index("sparse", ...), service.build_rag(..., hybrid=True)) run at fetch_k each
        (same default), their lists are fused by reciprocal rank (RRF, k = 60) and the best top_k are
        kept; `score` is the fused score.  With expr (both arms) and with rerank (the cross-encoder
        scores the fused candidates); not with min_score / max_score, group_by or mmr_lambda
        (ValueError).
        lexical (with hybrid): which lexical arm is fused with the dense one -- "bm25" (the default), "learned"
        (the learned sparse field: the query's SPLADE vector against the chunks', inner product; needs
        VectorRAG(..., sparse_encoder=)) or "both" (three arms).  Anything but "bm25" without hybrid or
        without a sparse encoder raises ValueError.
        offset: skip that many of the best chunks first -- the chunks of ranks offset + 1 ...
        offset + top_k (`rank` counts from 1 within the page); with expr and min_score / max_score,
        not with rerank, hybrid, mmr_lambda or group_by (ValueError).
        boost: {"filter": expression, "weight": w > 0}, or a list of up to 3 such dicts -- a soft
        filter: the chunks the expression selects have their score multiplied by w (below 1:
        demoted; several boosts multiply) and the top_k are the exact best of the whole store under
        that boosted score, which is what `score` then holds.  With expr (one string); not with
        rerank, hybrid, group_by, mmr_lambda, min_score / max_score or offset (ValueError).
        decay: {"field", "function", "origin", "scale"} and optionally "offset" (default 0) and "decay" (default
        0.5) -- time decay: every chunk's score is multiplied by a weight in [0, 1] that is 1 where the numeric
        field (primary_value, or an INT64 / DOUBLE field of the store) lies within `offset` of `origin` and falls
        to `decay` at distance offset + scale, along a "gauss", "exp" or "linear" curve; the top_k are the exact
        best of the whole store under that decayed score, which is what `score` then holds.  With expr (one
        string); with the same exclusions as boost, and not together with boost (ValueError).
        match_entities: "any" or "all" -- the entities the tagger finds in the query become
        ARRAY_CONTAINS_ANY / ARRAY_CONTAINS_ALL(<entity_field>, [...]), and-ed with expr: only chunks that mention
        one (all) of them are ranked.  A query without entities searches unfiltered.  Needs VectorRAG(...,
        tagger=, entity_field=), else ValueError."""
        if match_entities is not None:
            expr = self._entity_exprs([query], expr, match_entities)[0]
        ranker = self._boost_args(boost, rerank, hybrid, group_by, mmr_lambda, min_score, max_score, offset, expr)
        ranker = self._decay_args(decay, ranker, rerank, hybrid, group_by, mmr_lambda, min_score, max_score, offset, expr)
        self._check_offset(offset, rerank, hybrid, mmr_lambda, group_by)
        self._check_lexical(lexical, hybrid)
        self._check_rerank_with(rerank_with, rerank)
        if hybrid:
            self._check_hybrid(min_score, max_score, group_by, mmr_lambda)
        if rerank:
            return self._search_reranked([query], top_k, expr, min_score, max_score, group_by, mmr_lambda, fetch_k,
                                         hybrid, lexical, rerank_with)[0]
        if hybrid:
            return self._contexts(self._search_hybrid([query], top_k, top_k, expr, fetch_k, lexical)[0])
        q = self._embed([query])
        results = self.collection.search(q, "embedding", self._search_param(min_score, max_score, self._metric()), top_k,
                                         expr=expr, output_fields=self.output_fields,
                                         **self._group_args(group_by, group_size),
                                         **self._mmr_args(mmr_lambda, fetch_k), **self._offset_args(offset), **ranker)
        return self._contexts(results[0])

    @staticmethod
    def _boost_args(boost, rerank, hybrid, group_by, mmr_lambda, min_score, max_score, offset, expr) -> dict:
        """The store's ranker argument from `boost`; nothing when it was not given (the call of before)."""
        if boost is None:
            return {}
        if rerank or hybrid or group_by is not None or mmr_lambda is not None or min_score is not None or \
                max_score is not None or offset is not None or isinstance(expr, (list, tuple)):
            raise ValueError("boost re-weighs the plain ranking: it does not combine with rerank, hybrid, group_by, "
                             "mmr_lambda, min_score / max_score, offset or a list expr")
        from .ranker import MAX_BOOSTS, BoostRanker
        items = list(boost) if isinstance(boost, (list, tuple)) else [boost]
        if not 1 <= len(items) <= MAX_BOOSTS or not all(isinstance(b, dict) and set(b) == {"filter", "weight"}
                                                        for b in items):
            raise ValueError(f'boost must be {{"filter": str, "weight": float}} or a list of 1..{MAX_BOOSTS} such dicts')
        return {"ranker": [BoostRanker(b["filter"], b["weight"]) for b in items]}

    @staticmethod
    def _decay_args(decay, boosts: dict, rerank, hybrid, group_by, mmr_lambda, min_score, max_score, offset, expr) -> dict:
        """The store's ranker argument from `decay`; `boosts` (what _boost_args gave) when it was not given."""
        if decay is None:
            return boosts
        if boosts:
            raise ValueError("decay and boost do not combine yet: pass one of them")
        if rerank or hybrid or group_by is not None or mmr_lambda is not None or min_score is not None or \
                max_score is not None or offset is not None or isinstance(expr, (list, tuple)):
            raise ValueError("decay re-weighs the plain ranking: it does not combine with rerank, hybrid, group_by, "
                             "mmr_lambda, min_score / max_score, offset or a list expr")
        from .ranker import DecayRanker
        keys = {"field", "function", "origin", "scale", "offset", "decay"}
        if not isinstance(decay, dict) or not {"field", "function", "origin", "scale"} <= set(decay) <= keys:
            raise ValueError('decay must be {"field": str, "function": "gauss" | "exp" | "linear", "origin": float, '
                             '"scale": float} with optional "offset" and "decay"')
        return {"ranker": DecayRanker(decay["field"], decay["function"], decay["origin"], decay["scale"],
                                      decay.get("offset", 0.0), decay.get("decay", 0.5))}

    def _entity_exprs(self, queries, expr, match_entities) -> list:
        """Per query: expr (one string or None for all, or one entry per query) and-ed with the filter on the
        query's entities (rag_fin_amd.tagger.entity_expr); a query without entities keeps its expr."""
        from .tagger import entity_expr
        if match_entities not in ("any", "all"):
            raise ValueError(f"match_entities must be 'any' or 'all', got {match_entities!r}")
        if self.tagger is None:
            raise ValueError("match_entities needs a tagger (VectorRAG(..., tagger=TokenClassifier.from_local(dir), "
                             "entity_field=<the ARRAY VARCHAR field ingest filled>))")
        own = list(expr) if isinstance(expr, (list, tuple)) else [expr] * len(queries)
        if len(own) != len(queries):
            raise ValueError(f"expr list: {len(own)} entries for {len(queries)} queries (one entry per query)")
        out = []
        for e, found in zip(own, self.tagger.tags(list(queries))):
            f = entity_expr(self.entity_field, found, match_entities)
            e = e if e and e.strip() else None
            out.append(e if f is None else (f if e is None else f"({e}) and {f}"))
        return out

    def _embed(self, texts):
        """`.encode(texts)` of the reference (main.py:50) -- kept on the device when the embedder
        offers it: the unit-norm fp16 rows rf_encode writes are exactly what the store searches
        with, so the download / re-upload / re-normalise round trip of the numpy form is skipped."""
        # a model with a query prompt ("query: ", an instruction) embeds its queries behind it; the keyword is
        # absent otherwise, so an embedder with the signature of before is called as before
        prompt = getattr(self.similarity_model, "query_prompt", None)
        kw = {"prompt": prompt} if isinstance(prompt, str) and prompt else {}
        to_dev = getattr(self.similarity_model, "encode_to_device", None)
        return to_dev(texts, **kw) if to_dev is not None else self.similarity_model.encode(texts, **kw)

    def _metric(self) -> str:
        """The metric the store was built for (IP for a dot-product model: service.build_rag); COSINE otherwise."""
        m = getattr(self.collection, "metric_type", None)
        return m if isinstance(m, str) and m else "COSINE"

    @staticmethod
    def _offset_args(offset) -> dict:
        """The store's offset argument; nothing when it was not given (the call of before)."""
        return {} if offset is None else {"offset": offset}

    @staticmethod
    def _check_offset(offset, rerank, hybrid, mmr_lambda, group_by) -> None:
        if offset is not None and (rerank or hybrid or mmr_lambda is not None or group_by is not None):
            raise ValueError("offset pages through the plain ranking: it does not combine with rerank, hybrid, "
                             "mmr_lambda or group_by")

    @staticmethod
    def _default_fetch_k(top_k: int) -> int:
        return min(64, max(20, 4 * top_k))

    @staticmethod
    def _check_hybrid(min_score, max_score, group_by, mmr_lambda) -> None:
        if min_score is not None or max_score is not None:
            raise ValueError("hybrid search ranks by a fused score: it takes no min_score / max_score")
        if group_by is not None:
            raise ValueError("hybrid search does not combine with group_by")
        if mmr_lambda is not None:
            raise ValueError("hybrid search does not combine with mmr_lambda")

    def _check_lexical(self, lexical, hybrid) -> None:
        if lexical not in ("bm25", "learned", "both"):
            raise ValueError(f"lexical must be 'bm25', 'learned' or 'both', got {lexical!r}")
        if lexical != "bm25":
            if not hybrid:
                raise ValueError(f"lexical={lexical!r} chooses the lexical arm of a hybrid search: pass hybrid=True")
            if self.sparse_encoder is None:
                raise ValueError(f"lexical={lexical!r} needs a sparse encoder (VectorRAG(..., sparse_encoder="
                                 "SparseEncoder.from_local(dir)))")

    def _check_rerank_with(self, rerank_with, rerank) -> None:
        if rerank_with not in ("cross", "late"):
            raise ValueError(f"rerank_with must be 'cross' or 'late', got {rerank_with!r}")
        if rerank_with == "late":
            if not rerank:
                raise ValueError("rerank_with='late' chooses the second stage of a reranked search: pass rerank=True")
            if self.late_encoder is None:
                raise ValueError("rerank_with='late' needs a late encoder (VectorRAG(..., late_encoder="
                                 "ColBERT.from_local(dir)))")

    def _search_hybrid(self, queries, top_k, limit, expr, fetch_k, lexical: str = "bm25"):
        """The dense arm and the lexical arm(s) -- BM25, the learned sparse field, or both -- at fetch_k each,
        fused by RRF -> `limit` hits per query."""
        from .hybrid import AnnSearchRequest, RRFRanker
        fk = self._default_fetch_k(top_k) if fetch_k is None else fetch_k
        if isinstance(fk, bool) or not isinstance(fk, int) or not 1 <= fk <= 64:
            raise ValueError(f"hybrid search: fetch_k must be an integer in 1..64, got {fk!r}")
        if not 1 <= limit <= fk:
            raise ValueError(f"hybrid search: need 1 <= top_k <= fetch_k (got top_k = {limit}, fetch_k = {fk})")
        reqs = [AnnSearchRequest(self._embed(list(queries)), "embedding", {"metric_type": self._metric()}, fk, expr)]
        if lexical in ("bm25", "both"):
            reqs.append(AnnSearchRequest(list(queries), "sparse", {"metric_type": "BM25"}, fk, expr))
        if lexical in ("learned", "both"):
            reqs.append(AnnSearchRequest(list(queries), "sparse_embedding", {"metric_type": "IP"}, fk, expr))
        return self.collection.hybrid_search(reqs, RRFRanker(), limit, output_fields=self.output_fields)

    def _search_reranked(self, queries, top_k, expr, min_score, max_score, group_by, mmr_lambda, fetch_k,
                         hybrid: bool = False, lexical: str = "bm25", rerank_with: str = "cross"):
        if rerank_with == "cross" and self.reranker is None:
            raise ValueError("rerank=True needs a reranker (VectorRAG(..., reranker=CrossEncoder.from_local(dir)))")
        if mmr_lambda is not None:
            raise ValueError("rerank and mmr_lambda both re-order the best fetch_k chunks: give one of them")
        if group_by is not None:
            raise ValueError("rerank does not combine with group_by")
        fk = self._default_fetch_k(top_k) if fetch_k is None else fetch_k
        if fk < top_k:
            raise ValueError(f"fetch_k={fk} is less than top_k={top_k}")
        if hybrid:   # the fused candidates: `score` is then the fused score
            results = self._search_hybrid(queries, top_k, fk, expr, fk, lexical)
        else:
            q = self._embed(list(queries))
            results = self.collection.search(q, "embedding", self._search_param(min_score, max_score, self._metric()), fk,
                                             expr=expr, output_fields=self.output_fields)
        hits = [list(r) for r in results]
        if rerank_with == "late":
            # every query's candidates in ONE candidate-mode MaxSim call on the stored token vectors
            per_query = self.collection.rerank_tokens(list(queries), [[h.row for h in r] for r in hits])
            scores = [v for s in per_query for v in s]
        else:
            # every query's candidates in ONE cross-encoder call
            pairs = [(query, h.entity.text) for query, r in zip(queries, hits) for h in r]
            scores = self.reranker.predict(pairs) if pairs else []
        out, at = [], 0
        for r in hits:
            s = [float(v) for v in scores[at:at + len(r)]]
            at += len(r)
            # best rerank score first; equal scores keep the retrieval order
            keep = sorted(range(len(r)), key=lambda i: (-s[i], i))[:top_k]
            ctx = self._contexts([r[i] for i in keep])
            for c, i in zip(ctx, keep):
                c["rerank_score"] = s[i]
            out.append(ctx)
        return out

    retrieve = search  # BASELINE.json's "retrieve(query, k)" name for the same call

    def search_batch(self, queries: Sequence[str], top_k: int = 3, expr: str | None = None,
                     min_score: float | None = None, max_score: float | None = None,
                     group_by: str | None = None, group_size: int = 1,
                     mmr_lambda: float | None = None, fetch_k: int | None = None,
                     rerank: bool = False, hybrid: bool = False, offset: int | None = None,
                     boost=None, lexical: str = "bm25", rerank_with: str = "cross", decay=None,
                     match_entities: str | None = None) -> list[list[dict]]:
        """Many queries in one embed + one corpus sweep per 64 (new: the reference
        is strictly one query per call); expr, min_score / max_score, group_by / group_size,
        mmr_lambda / fetch_k: one filter, one score band, one grouping and one diversification for
        the whole batch; rerank: every query's fetch_k candidates in one cross-encoder call (rerank_with="late": in
        one MaxSim call on the stored token vectors); hybrid:
        dense + BM25 (lexical: or the learned sparse arm, or both) fused by reciprocal rank for every query, as
        in search(); offset: one for the whole batch, as in search().
        expr may also be a list or tuple with one entry per query (a filter string, or None for "no
        filter"): per-query filters, still one corpus sweep per 64 queries
        (CorpusStore.search(expr=[...])).  The list form is the plain path only: with rerank, hybrid,
        min_score / max_score, group_by, mmr_lambda or offset it raises ValueError.
        boost: one boost (or up to 3) for the whole batch, as in search(); not with a list expr.
        decay: one time decay for the whole batch, as in search(); not with a list expr.
        match_entities: as in search(), per query: every query is filtered on its own entities, so expr becomes
        the list form (one tagger call for the batch) with the list form's limits."""
        if match_entities is not None and queries:
            expr = self._entity_exprs(list(queries), expr, match_entities)
        ranker = self._boost_args(boost, rerank, hybrid, group_by, mmr_lambda, min_score, max_score, offset, expr)
        ranker = self._decay_args(decay, ranker, rerank, hybrid, group_by, mmr_lambda, min_score, max_score, offset, expr)
        if isinstance(expr, (list, tuple)):
            if rerank or hybrid or min_score is not None or max_score is not None or group_by is not None or \
                    mmr_lambda is not None or offset is not None:
                raise ValueError("per-query filters (a list expr) serve the plain search only: not with rerank, hybrid, "
                                 "min_score / max_score, group_by, mmr_lambda or offset")
            if len(expr) != len(queries):
                raise ValueError(f"expr list: {len(expr)} entries for {len(queries)} queries (one entry per query)")
        self._check_offset(offset, rerank, hybrid, mmr_lambda, group_by)
        self._check_lexical(lexical, hybrid)
        self._check_rerank_with(rerank_with, rerank)
        if hybrid:
            self._check_hybrid(min_score, max_score, group_by, mmr_lambda)
        if not queries:
            return []
        if rerank:
            return self._search_reranked(list(queries), top_k, expr, min_score, max_score, group_by, mmr_lambda,
                                         fetch_k, hybrid, lexical, rerank_with)
        if hybrid:
            return [self._contexts(r) for r in self._search_hybrid(list(queries), top_k, top_k, expr, fetch_k, lexical)]
        q = self._embed(list(queries))
        results = self.collection.search(q, "embedding", self._search_param(min_score, max_score, self._metric()), top_k,
                                         expr=expr, output_fields=self.output_fields,
                                         **self._group_args(group_by, group_size),
                                         **self._mmr_args(mmr_lambda, fetch_k), **self._offset_args(offset), **ranker)
        return [self._contexts(r) for r in results]

    # -- generation (out of scope; interface kept) -----------------------------------------
    def build_prompt(self, question: str, contexts: list[dict]) -> str:
        ctx = "\n\n".join(f"Context {i + 1} [{c['period']} - {c['chunk_type']}]:\n{c['text']}"
                          for i, c in enumerate(contexts))
        return self.prompt_template.format(question=question, context=ctx)

    def search_and_answer(self, question: str, top_k: int = 3, min_score: float | None = None) -> dict:
        """min_score: only chunks scoring above it reach the prompt (possibly none: the prompt is
        then built from zero contexts and the payload keeps its keys).
        With a generator: {"answer", "contexts", "context_count"}, as ever.  Without one but with a reader the
        answer is the reader's best span over the retrieved chunks' texts:
        {"answer", "answer_span": {"context_index", "start", "end", "score"}, "answer_source": "reader",
        "contexts", "context_count"} with answer == contexts[context_index]["text"][start:end]; zero contexts
        or no candidate span give answer "" and answer_span None.  With neither: the error payload."""
        contexts = self.search(question, top_k) if min_score is None else \
            self.search(question, top_k, min_score=min_score)
        prompt = self.build_prompt(question, contexts)
        try:
            if self.generator is None and self.reader is not None:
                best = self.reader.predict(question, [c["text"] for c in contexts], top_k=1) if contexts else []
                span = {k: best[0][k] for k in ("context_index", "start", "end", "score")} if best else None
                return {"answer": best[0]["answer"] if best else "", "answer_span": span, "answer_source": "reader",
                        "contexts": contexts, "context_count": len(contexts)}
            if self.generator is None:
                raise RuntimeError("no LLM generator configured (generation is outside this build)")
            if self.llm_delay_s:
                time.sleep(self.llm_delay_s)
            answer = self.generator(prompt)
            return {"answer": str(answer).strip(), "contexts": contexts, "context_count": len(contexts)}
        except Exception as e:  # the reference's blanket handler (main.py:103-108)
            return {"error": str(e), "contexts": contexts, "context_count": len(contexts)}

    def facets(self, fields=None, expr=None, limit: int = 10, min_count: int = 1, ranges=None, metrics=None) -> dict:
        """Faceted counts of the collection (CorpusStore.facets): how many of the chunks `expr` matches hold
        each value of `fields`, and how many fall into each of `ranges`; with `metrics` (numeric fields) also the
        exact sum, avg, min and max of each per bucket and over all matching chunks."""
        extra = {} if metrics is None else {"metrics": metrics}
        return self.collection.facets(fields, expr=expr, limit=limit, min_count=min_count, ranges=ranges, **extra)

    def health_check(self) -> dict:
        try:
            n = self.collection.num_entities
            llm = "available" if self.generator is not None else "not configured"
            m = self.similarity_model
            # the ends of the embedder's forward, where the embedder states them (rag_fin_amd.embedder.Embedder
            # does); an embedder that says nothing keeps the reference's keys
            ends = {} if not hasattr(m, "pooling") else {
                "pooling": m.pooling, "normalize": bool(getattr(m, "normalize", True)),
                "prompts": bool(getattr(m, "prompts", None))}
            return {"status": "healthy", "milvus": "in-process MI355X store", "gemini": llm,
                    "collection": self.collection_name, "total_chunks": n, **ends}
        except Exception as e:
            return {"status": "unhealthy", "error": str(e)}
