"""Keyword filters through the public surface, with fakes (CPU only): VectorRAG, the search_vectors
tool and the REST request hand a TEXT_MATCH / PHRASE_MATCH expression to the store unchanged."""
import numpy as np
import pytest

from rag_fin_amd import filter_expr, mcp_server

KEYWORD = 'TEXT_MATCH(text, "eps")'
PHRASE = 'PHRASE_MATCH(text, "net interest income") and period == "Q1_FY2024"'


class Store:
    num_entities = 0

    def __init__(self):
        self.exprs = []

    def load(self):
        pass

    def search(self, data, anns_field, param, limit, expr=None, output_fields=None):
        self.exprs.append(expr)
        return [[] for _ in range(np.asarray(data).shape[0])]


class Emb:
    def encode(self, texts):
        return np.zeros((len(texts), 4), dtype=np.float32)


def test_vector_rag_hands_a_keyword_expr_to_the_store():
    from rag_fin_amd.rag import VectorRAG
    rag = VectorRAG("k", embedder=Emb(), store=Store())
    rag.search("q", 3, expr=KEYWORD)
    rag.search_batch(["a", "b"], 2, expr=PHRASE)
    assert rag.collection.exprs == [KEYWORD, PHRASE]


class FakeRag:
    """Records how the tool layer calls it; parses filters like the store does."""

    def __init__(self):
        self.calls = []

    def search(self, query, top_k=3, expr=None):
        self.calls.append((query, top_k, expr))
        if not filter_expr.is_empty(expr):
            filter_expr.parse(expr)
        return [{"rank": 1, "text": "basic eps", "period": "Q1_FY2024", "chunk_type": "c", "statement_type": "s",
                 "primary_value": 1.0, "score": 0.5}][:top_k]

    def search_batch(self, queries, top_k=3, expr=None):
        return [self.search(q, top_k, expr) for q in queries]


@pytest.fixture
def fake_rag():
    rag = FakeRag()
    mcp_server.set_rag(rag)
    yield rag
    mcp_server.set_rag(None)


def test_search_vectors_passes_a_keyword_filter_as_expr(fake_rag):
    r = mcp_server.search_vectors("earnings per share", 2, filter=KEYWORD)
    assert r["status"] == "success" and fake_rag.calls[-1] == ("earnings per share", 2, KEYWORD)
    r = mcp_server.search_vectors("net interest income", 3, filter=PHRASE)
    assert r["status"] == "success" and fake_rag.calls[-1] == ("net interest income", 3, PHRASE)
    r = mcp_server.search_vectors("earnings per share", 3, filter='PHRASE_MATCH(text, "a b", 2)')
    assert r["status"] == "error" and "exact adjacency" in r["message"]
    r = mcp_server.search_vectors("earnings per share", 3, filter='TEXT_MATCH(period, "a")')
    assert r["status"] == "error" and "'period'" in r["message"]


def test_rest_body_carries_the_keyword_filter():
    from rag_fin_amd.adapter import SearchRequest, search_args
    assert search_args(SearchRequest(query="hello", top_k=4, filter=KEYWORD)) == \
        {"query": "hello", "top_k": 4, "filter": KEYWORD}
    assert search_args(SearchRequest(query="hello", filter=PHRASE))["filter"] == PHRASE
