"""REST -> MCP bridge for the vector-RAG server (port 9001 -> MCP 9006).

Same routes, request bounds and error mapping as adapters/vectorrag_adapter.py:
  GET /            service card                         (:121-132)
  GET /health      {"status": "healthy", "mcp": ...} | {"status": "unhealthy", "mcp": "unavailable"}
  POST /search     {query: str >= 5 chars, top_k: 1..20 = 3, filter: str (optional), rerank: bool (optional),
                   hybrid: bool (optional), lexical: "bm25" | "learned" | "both" (optional), rerank_with: "cross" | "late" (optional), match_entities: "any" | "all" (optional), offset: int >= 0 (optional), boost_filter: str + boost_weight: float > 0
                   (optional), decay_field: str + decay_function: "gauss" | "exp" | "linear" + decay_origin: float +
                   decay_scale: float > 0 [+ decay_offset: float >= 0, decay_rate: 0 < float < 1] (optional)}
                                                               -> tool search_vectors
  POST /answer     {question: str >= 5 chars, top_k: 1..10 = 3} -> tool answer_question
  GET /stats       -> tool get_collection_stats
  POST /stats      {expr: str (optional), facet_fields: [str] (optional), facet_limit: 1..1000 = 10,
                    metric_fields: [str] (optional, at most 4)}
                                                               -> tool get_collection_stats (faceted counts and
                                                                  metric aggregations; new)
Transport: JSON-RPC 2.0 over MCP streamable HTTP; one session, initialised on
first use ("initialize" + "notifications/initialized"); tool calls are streamed
and the first SSE `data:` line carrying a "result" wins; non-200 -> 503, a
JSON-RPC "error" -> 500, a stream without result -> 500 (:91-111).
"""
from __future__ import annotations

import json
import logging
import os
from typing import Optional

import httpx
from fastapi import FastAPI, HTTPException
from pydantic import BaseModel, Field

logger = logging.getLogger(__name__)

MCP_URL = os.getenv("VECTOR_RAG_MCP_URL", "http://localhost:9006/mcp")
TIMEOUT = 300
PROTOCOL_VERSION = "2024-11-05"


class SearchRequest(BaseModel):
    query: str = Field(..., min_length=5)
    top_k: int = Field(default=3, ge=1, le=20)
    # boolean expression over the scalar fields (rag_fin_amd.filter_expr); new, not in the reference
    filter: Optional[str] = None
    # score cut-offs (range search: min_score < score <= max_score); new, not in the reference
    min_score: Optional[float] = None
    max_score: Optional[float] = None
    # grouping search (the best top_k groups by a scalar field, group_size chunks each); new
    group_by: Optional[str] = None
    group_size: Optional[int] = Field(default=None, ge=1)
    # diversified search (maximal marginal relevance over the best fetch_k chunks); new
    mmr_lambda: Optional[float] = Field(default=None, ge=0.0, le=1.0)
    fetch_k: Optional[int] = Field(default=None, ge=1, le=64)
    # two-stage search (the best fetch_k chunks re-scored by the cross-encoder); new
    rerank: bool = False
    # hybrid search (the dense and a BM25 arm fused by reciprocal rank); new
    hybrid: bool = False
    # the lexical arm of a hybrid search: "bm25" (the default), "learned" (SPLADE vectors) or "both"; new
    lexical: Optional[str] = None
    # the second stage of a reranked search: "cross" (the default: the cross-encoder) or "late" (MaxSim); new
    rerank_with: Optional[str] = None
    # entity filter: only chunks that mention any / all of the entities the tagger finds in the query; new
    match_entities: Optional[str] = None
    # paging (skip the best `offset` chunks, return the next top_k); new
    offset: Optional[int] = Field(default=None, ge=0)
    # boosted search (the chunks boost_filter selects have their score multiplied by boost_weight); new
    boost_filter: Optional[str] = None
    boost_weight: Optional[float] = Field(default=None, gt=0.0)
    # decayed search (scores fall off with the distance of the numeric field decay_field from decay_origin:
    # to decay_rate at decay_offset + decay_scale, along decay_function = "gauss" | "exp" | "linear"); new
    decay_field: Optional[str] = None
    decay_function: Optional[str] = None
    decay_origin: Optional[float] = None
    decay_scale: Optional[float] = Field(default=None, gt=0.0)
    decay_offset: Optional[float] = Field(default=None, ge=0.0)
    decay_rate: Optional[float] = Field(default=None, gt=0.0, lt=1.0)


def search_args(req: SearchRequest) -> dict:
    """Tool arguments of POST /search: `filter`, `min_score`, `max_score`, `group_by`, `group_size`,
    `mmr_lambda`, `fetch_k`, `offset`, `boost_filter`, `boost_weight`, `decay_*`, `lexical`, `rerank_with` and `match_entities` only when they were given, `rerank` and
    `hybrid` only when set, so the reference's payload {"query", "top_k"} is unchanged."""
    args = {"query": req.query, "top_k": req.top_k}
    for name in ("filter", "min_score", "max_score", "group_by", "group_size", "mmr_lambda", "fetch_k", "offset",
                 "boost_filter", "boost_weight", "lexical", "rerank_with", "match_entities", "decay_field", "decay_function", "decay_origin",
                 "decay_scale", "decay_offset", "decay_rate"):
        if getattr(req, name) is not None:
            args[name] = getattr(req, name)
    if req.rerank:
        args["rerank"] = True
    if req.hybrid:
        args["hybrid"] = True
    return args


class AnswerRequest(BaseModel):
    question: str = Field(..., min_length=5)
    top_k: int = Field(default=3, ge=1, le=10)


def first_sse_result(lines):
    """Scan SSE lines; return the first JSON-RPC result, raise on a JSON-RPC error."""
    for line in lines:
        if not line.startswith("data: "):
            continue
        try:
            msg = json.loads(line[len("data: "):])
        except json.JSONDecodeError:
            continue
        if "result" in msg:
            return msg["result"]
        if "error" in msg:
            raise HTTPException(500, f"Tool error: {msg['error']}")
    return None


class MCPClient:
    def __init__(self, url: str = MCP_URL, client: httpx.AsyncClient | None = None):
        self.url = url
        self.client = client or httpx.AsyncClient(timeout=TIMEOUT)
        self.session_id = None

    def _headers(self) -> dict:
        h = {"Content-Type": "application/json", "Accept": "application/json, text/event-stream"}
        if self.session_id:
            h["mcp-session-id"] = self.session_id
        return h

    @staticmethod
    def _rpc(method: str, params: dict | None = None, notify: bool = False) -> dict:
        msg = {"jsonrpc": "2.0", "method": method}
        if not notify:
            msg["id"] = 1   # the reference always sends id 1
        if params is not None:
            msg["params"] = params
        return msg

    async def init_session(self) -> None:
        if self.session_id:
            return
        hello = self._rpc("initialize", {"protocolVersion": PROTOCOL_VERSION, "capabilities": {},
                                         "clientInfo": {"name": "vectorrag-adapter", "version": "1.0.0"}})
        resp = await self.client.post(self.url, json=hello, headers=self._headers())
        self.session_id = resp.headers.get("mcp-session-id")
        await self.client.post(self.url, json=self._rpc("notifications/initialized", notify=True),
                               headers=self._headers())
        logger.info("Session initialized: %s", self.session_id)

    async def call_tool(self, tool_name: str, args: dict) -> dict:
        await self.init_session()
        call = self._rpc("tools/call", {"name": tool_name, "arguments": args})
        logger.info("Calling tool: %s", tool_name)
        async with self.client.stream("POST", self.url, json=call, headers=self._headers()) as resp:
            if resp.status_code != 200:
                raise HTTPException(503, f"MCP error: {resp.status_code}")
            result = None
            async for line in resp.aiter_lines():
                result = first_sse_result([line])
                if result is not None:
                    break
            if result is None:
                raise HTTPException(500, "No result from MCP")
            return result


mcp = MCPClient()
app = FastAPI(title="Vector RAG Adapter")


@app.get("/")
def root():
    return {"service": "vector-rag-adapter", "mcp_server": MCP_URL,
            "endpoints": {"health": "/health", "search": "/search", "answer": "/answer",
                          "stats": "/stats"}}


@app.get("/health")
async def health():
    try:
        return {"status": "healthy", "mcp": await mcp.call_tool("health_check", {})}
    except Exception:
        return {"status": "unhealthy", "mcp": "unavailable"}


@app.post("/search")
async def search(req: SearchRequest):
    return await mcp.call_tool("search_vectors", search_args(req))


@app.post("/answer")
async def answer(req: AnswerRequest):
    return await mcp.call_tool("answer_question", {"question": req.question, "top_k": req.top_k})


@app.get("/stats")
async def stats():
    return await mcp.call_tool("get_collection_stats", {})


class StatsRequest(BaseModel):
    # faceted counts: the chunks `expr` matches and their count per value of facet_fields; new
    expr: Optional[str] = None
    facet_fields: Optional[list[str]] = Field(default=None, max_length=16)
    facet_limit: int = Field(default=10, ge=1, le=1000)
    # metric aggregations: the exact sum / avg / min / max of numeric fields, per bucket and over all matches; new
    metric_fields: Optional[list[str]] = Field(default=None, max_length=4)


def stats_args(req: StatsRequest) -> dict:
    """Tool arguments of POST /stats: only what was given, so an empty body is the call of GET /stats."""
    args = {}
    if req.expr is not None:
        args["expr"] = req.expr
    if req.facet_fields:
        args["facet_fields"], args["facet_limit"] = list(req.facet_fields), req.facet_limit
    if req.metric_fields:
        args["metric_fields"] = list(req.metric_fields)
    return args


@app.post("/stats")
async def stats_faceted(req: StatsRequest):
    return await mcp.call_tool("get_collection_stats", stats_args(req))


def main() -> None:
    import uvicorn
    logging.basicConfig(level=logging.INFO)
    logger.info("Vector RAG Adapter on port 9001 -> %s", MCP_URL)
    uvicorn.run(app, host="0.0.0.0", port=9001)


if __name__ == "__main__":
    main()
