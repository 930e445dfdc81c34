"""MCP tool surface of the vector-RAG server (port 9006), same four tools, parameter
names, defaults and payload keys as vector_rag_mcp/main.py:127-178.

The tool bodies are plain functions over a lazily built `rag` so they can be called
(and tested) without FastMCP; `main()` registers them on a FastMCP("VectorRAG")
server when the `fastmcp` package is installed.
"""
from __future__ import annotations

import logging
import os
import sys

logger = logging.getLogger(__name__)

COLLECTION_NAME = os.getenv("MILVUS_COLLECTION", "fin_chunks")
# kept in the stats payload for drop-in compatibility; the store is in-process
MILVUS_HOST = os.getenv("MILVUS_HOST", "in-process")
MILVUS_PORT = os.getenv("MILVUS_PORT", "hbm")

_rag = None


def set_rag(rag) -> None:
    global _rag
    _rag = rag


def get_rag():
    global _rag
    if _rag is None:
        from .service import build_rag_from_env
        _rag = build_rag_from_env()
    return _rag


def health_check():
    """Check Vector RAG system health"""
    return get_rag().health_check()


_batcher = None


def _searcher():
    """RAGFIN_MICROBATCH_MS > 0: coalesce concurrent tool calls into one GPU batch
    (rag_fin_amd.batching); default: one search per call, like the reference."""
    global _batcher
    ms = float(os.getenv("RAGFIN_MICROBATCH_MS", "0") or 0)
    if ms <= 0:
        return get_rag()
    if _batcher is None or _batcher.rag is not get_rag():
        from .batching import MicroBatcher
        _batcher = MicroBatcher(get_rag(), max_batch=64, max_wait_ms=ms)
    return _batcher


def search_vectors(query: str, top_k: int = 3, filter: str = "", min_score: float | None = None,
                   max_score: float | None = None, group_by: str | None = None, group_size: int = 1,
                   mmr_lambda: float | None = None, fetch_k: int | None = None, rerank: bool = False,
                   hybrid: bool = False, offset: int | None = None, boost_filter: str = "",
                   boost_weight: float | None = None, lexical: str | None = None, rerank_with: str | None = None,
                   decay_field: str = "", decay_function: str | None = None, decay_origin: float | None = None,
                   decay_scale: float | None = None, decay_offset: float | None = None,
                   decay_rate: float | None = None, match_entities: str | None = None):
    """Semantic search in vector store.  filter: an optional boolean expression over the
    scalar fields, e.g. 'period == "Q1_FY2024" and primary_value > 0' (Milvus syntax).
    min_score / max_score: optional score cut-offs, min_score < score <= max_score.
    group_by: optional grouping field (period, chunk_type, statement_type): the best top_k groups,
    each by its best group_size chunks, as one flat ranked list.
    mmr_lambda: optional diversification, 0..1 (maximal marginal relevance: 1 = relevance only, lower
    values trade relevance for chunks unlike those already returned); fetch_k: how many best chunks
    the top_k are picked from (at most 64).
    rerank: optional second stage -- the best fetch_k chunks are re-scored as (query, text) pairs by the
    cross-encoder and the best top_k of them returned, each with a rerank_score.
    rerank_with: optional choice of that second stage -- "cross" (the default) or "late" (MaxSim of the query's
    token vectors against the chunks' stored ones, ColBERT late interaction; needs COLBERT_MODEL_DIR).
    hybrid: optional lexical arm -- the semantic search and a BM25 search of the chunk texts run at
    fetch_k each and are fused by reciprocal rank; `score` is then the fused score.  With filter and
    rerank; not with min_score / max_score, group_by or mmr_lambda.  Needs the store's lexical index
    (LEXICAL_INDEX=1 at ingest).
    lexical: optional choice of the lexical arm of a hybrid search -- "bm25" (the default), "learned" (the
    learned sparse vectors of a SPLADE model; needs SPARSE_MODEL_DIR) or "both" (three arms fused).
    offset: optional paging -- skip that many of the best chunks, return the next top_k.  With filter and
    min_score / max_score; not with rerank, hybrid, mmr_lambda or group_by.
    boost_filter / boost_weight: optional soft filter -- the chunks the expression boost_filter selects
    have their score multiplied by boost_weight (> 0; below 1 demotes), the rest stay in the ranking;
    `score` is then the boosted score.  Both or neither; with filter, not with min_score / max_score,
    group_by, mmr_lambda, rerank, hybrid or offset.
    decay_field / decay_function / decay_origin / decay_scale (and optionally decay_offset, default 0, and
    decay_rate, default 0.5): optional time decay -- every chunk's score is multiplied by a weight that is 1
    where the numeric field decay_field lies within decay_offset of decay_origin and falls to decay_rate at
    distance decay_offset + decay_scale, along a "gauss", "exp" or "linear" curve; `score` is then the decayed
    score.  The first four go together; with filter, with the exclusions of the boost and not together with it.
    match_entities: optional entity filter -- "any" or "all": only chunks that mention one (all) of the entities
    the tagger finds in the query are ranked, and-ed with filter; a query without entities searches unfiltered
    (needs TAGGER_MODEL_DIR at ingest)."""
    try:
        decay_given = [v is not None for v in (decay_function, decay_origin, decay_scale, decay_offset, decay_rate)]
        if bool(decay_field and decay_field.strip()) or any(decay_given):
            # a decayed call bypasses the micro-batcher like a boosted one: one batch shares one decay
            if not (decay_field and decay_field.strip()) or not all(decay_given[:3]):
                raise ValueError("decay_field, decay_function, decay_origin and decay_scale go together")
            decay = {"field": decay_field, "function": decay_function, "origin": decay_origin, "scale": decay_scale}
            if decay_offset is not None:
                decay["offset"] = decay_offset
            if decay_rate is not None:
                decay["decay"] = decay_rate
            kw = {name: v for name, v in (("min_score", min_score), ("max_score", max_score), ("group_by", group_by),
                                          ("mmr_lambda", mmr_lambda), ("fetch_k", fetch_k), ("offset", offset))
                  if v is not None}
            if rerank:
                kw["rerank"] = True
            if hybrid:
                kw["hybrid"] = True
            if match_entities is not None:
                kw["match_entities"] = match_entities
            if bool(boost_filter and boost_filter.strip()) or boost_weight is not None:
                kw["boost"] = {"filter": boost_filter, "weight": boost_weight}   # (VectorRAG refuses the combination)
            contexts = get_rag().search(query, top_k, expr=filter if filter and filter.strip() else None, decay=decay, **kw)
            return {"status": "success", "query": query, "results": contexts, "result_count": len(contexts)}
        boosted = bool(boost_filter and boost_filter.strip()) or boost_weight is not None
        if boosted:
            # a boosted call bypasses the micro-batcher: one batch shares one boost (VectorRAG refuses
            # what does not combine with it, and a filter without a weight or the reverse)
            if not (boost_filter and boost_filter.strip()) or boost_weight is None:
                raise ValueError("boost_filter and boost_weight go together")
            kw = {name: v for name, v in (("min_score", min_score), ("max_score", max_score), ("group_by", group_by),
                                          ("mmr_lambda", mmr_lambda), ("fetch_k", fetch_k), ("offset", offset))
                  if v is not None}
            if rerank:
                kw["rerank"] = True
            if hybrid:
                kw["hybrid"] = True
            if lexical is not None:
                kw["lexical"] = lexical
            if rerank_with is not None:
                kw["rerank_with"] = rerank_with
            if match_entities is not None:
                kw["match_entities"] = match_entities
            contexts = get_rag().search(query, top_k, expr=filter if filter and filter.strip() else None,
                                        boost={"filter": boost_filter, "weight": boost_weight}, **kw)
            return {"status": "success", "query": query, "results": contexts, "result_count": len(contexts)}
        # (only what was given travels on; diversified, reranked and hybrid calls bypass the micro-batcher as well)
        mmr = {name: v for name, v in (("mmr_lambda", mmr_lambda), ("fetch_k", fetch_k)) if v is not None}
        if rerank:
            mmr["rerank"] = True
        if hybrid:
            mmr["hybrid"] = True
        if lexical is not None:
            mmr["lexical"] = lexical
        if rerank_with is not None:
            mmr["rerank_with"] = rerank_with
        if match_entities is not None:   # (an entity-filtered call bypasses the micro-batcher like a filtered one)
            mmr["match_entities"] = match_entities
        if offset is not None:   # (a paged call bypasses the micro-batcher too: one batch shares one offset)
            mmr["offset"] = offset
        if group_by is not None:
            # grouped calls bypass the micro-batcher like filtered ones: one batch shares one grouping
            kw = {"group_by": group_by, "group_size": group_size}
            if min_score is not None or max_score is not None:
                kw.update(min_score=min_score, max_score=max_score)   # (the store refuses the combination)
            contexts = get_rag().search(query, top_k, expr=filter if filter and filter.strip() else None, **kw, **mmr)
        elif min_score is not None or max_score is not None:
            # like filtered calls, banded calls bypass the micro-batcher: one batch shares one band
            contexts = get_rag().search(query, top_k, expr=filter if filter and filter.strip() else None,
                                        min_score=min_score, max_score=max_score, **mmr)
        elif filter and filter.strip():
            # filtered calls bypass the micro-batcher: one batch shares one filter -- unless
            # RAGFIN_MICROBATCH_FILTERS=1 (with RAGFIN_MICROBATCH_MS > 0): a call that carries only a
            # filter is then coalesced too, each request over its own filter in one sweep
            batcher = _searcher() if not mmr and os.getenv("RAGFIN_MICROBATCH_FILTERS", "0") == "1" else None
            if batcher is not None and batcher is not get_rag():
                contexts = batcher.search(query, top_k, expr=filter)
            else:
                contexts = get_rag().search(query, top_k, expr=filter, **mmr)
        elif mmr:
            contexts = get_rag().search(query, top_k, **mmr)
        else:
            contexts = _searcher().search(query, top_k)
        return {"status": "success", "query": query, "results": contexts,
                "result_count": len(contexts)}
    except Exception as e:
        return {"status": "error", "message": str(e), "query": query}


def answer_question(question: str, top_k: int = 3, min_score: float | None = None):
    """Answer question using RAG.  min_score: only chunks scoring above it are used."""
    try:
        result = get_rag().search_and_answer(question, top_k) if min_score is None else \
            get_rag().search_and_answer(question, top_k, min_score=min_score)
        return {"status": "success", "question": question, **result}
    except Exception as e:
        return {"status": "error", "message": str(e), "question": question}


def get_collection_stats(expr: str | None = None, facet_fields: list | None = None, facet_limit: int = 10,
                         metric_fields: list | None = None):
    """Get collection statistics.  expr and / or facet_fields: also "count", the chunks `expr` matches (all
    without one), and "facets", their count per value of each of facet_fields (the best facet_limit values).
    metric_fields (at most 4 numeric fields): also "metrics", the exact sum / avg / min / max of each over the
    matching chunks, and the same inside every facet bucket."""
    try:
        out = {"status": "success", "collection_name": COLLECTION_NAME,
               "total_chunks": get_rag().collection.num_entities,
               "milvus_host": MILVUS_HOST, "milvus_port": MILVUS_PORT}
        if expr is not None or facet_fields or metric_fields:
            expr = expr if expr and expr.strip() else None
            if metric_fields:
                got = get_rag().facets(list(facet_fields or []), expr=expr, limit=facet_limit, metrics=list(metric_fields))
                out["count"], out["facets"], out["metrics"] = got["count"], got["facets"], got["metrics"]
            elif facet_fields:
                got = get_rag().facets(list(facet_fields), expr=expr, limit=facet_limit)
                out["count"], out["facets"] = got["count"], got["facets"]
            else:
                out["count"] = get_rag().collection.query(expr or "", output_fields=["count(*)"])[0]["count(*)"]
                out["facets"] = {}
        return out
    except Exception as e:
        return {"status": "error", "message": str(e)}


TOOLS = (health_check, search_vectors, answer_question, get_collection_stats)


def main() -> None:
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s: %(message)s",
                        handlers=[logging.StreamHandler(sys.stdout)])
    os.environ.setdefault("PORT", "9006")
    try:
        from fastmcp import FastMCP
    except ImportError as e:
        raise SystemExit("the MCP transport needs the `fastmcp` package (not installed here); the "
                         "tool functions in rag_fin_amd.mcp_server work without it") from e
    # N > 1 (torch.distributed.run, one process per GPU): every rank builds its shard; ranks > 0
    # then follow rank 0's searches and never reach the MCP transport
    rag = get_rag()
    if hasattr(rag.collection, "start_workers"):
        rag.collection.start_workers()
        if rag.collection.rank != 0:
            return
    mcp = FastMCP("VectorRAG")
    for fn in TOOLS:
        mcp.tool()(fn)
    get_rag()
    logger.info("Starting Vector RAG MCP Server on port %s (collection %s)", os.environ["PORT"],
                COLLECTION_NAME)
    try:
        mcp.run(transport="streamable-http")
    finally:   # release the ranks parked in start_workers(), however the server ends
        if hasattr(rag.collection, "stop_workers"):
            rag.collection.stop_workers()


if __name__ == "__main__":
    main()
