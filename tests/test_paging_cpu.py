"""Paged search through the public surface, with fakes (CPU only): the validation of `offset` in
CorpusStore.search, the calls the index receives with and without it, query(offset=), the
bookkeeping of search_iterator and its mutation guard, the upper surfaces (VectorRAG, the MCP tool,
the REST request, the sharded store's refusal) and the host-side argument checks of rf_search_after."""
import ctypes
import math

import numpy as np
import pytest
import torch

from rag_fin_amd import _lib, mcp_server
from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
from rag_fin_amd.store import CorpusStore, check_offset
from test_range_search_cpu import FakeIndex as RangeFakeIndex, FakeRag, RecStore, Emb, one_rank_group  # noqa: F401

INF = float("inf")
RF_ERR_INVALID = -1      # include/ragfin.h
Q = np.ones((1, 8), dtype=np.float32)


class FakeIndex(RangeFakeIndex):
    """The CPU double of tests/test_range_search_cpu.py whose rows 0..n-1 rank in row order with the
    scores 1 - row / 1000, plus search_after over that ranking."""

    def __init__(self, *a, total=40, **kw):
        super().__init__(*a, **kw)
        self.total = total

    def _result(self, B, k):
        scores = np.full((B, k), -np.inf, dtype=np.float32)
        rows = np.full((B, k), -1, dtype=np.int64)
        m = min(k, self.total)
        rows[:, :m] = np.arange(m)
        scores[:, :m] = 1.0 - np.arange(m) / 1000.0
        return scores, rows

    def search_after(self, q16, k, after, id_base=0, want_exact=False, **kw):
        bs, bi = after
        self.calls.append(("after", k, (float(bs[0]), int(bi[0])), kw))
        first = 0 if bs[0] == INF else (self.total if bs[0] == -INF else int(bi[0]) + 1)
        rows = np.full((1, k), -1, dtype=np.int64)
        m = max(0, min(k, self.total - first))
        rows[0, :m] = np.arange(first, first + m)
        exact = np.where(rows >= 0, 1.0 - rows / 1000.0, -np.inf)
        return torch.from_numpy(exact.astype(np.float32)), torch.from_numpy(rows), torch.from_numpy(exact)


def make_store(n=40, **kw):
    ix = FakeIndex(capacity=max(64, n), total=n, **kw)       # (room for every row: the store never swaps the index)
    st = CorpusStore("c", dim=8, capacity=max(64, n), index=ix)
    st.add([f"k{i}" for i in range(n)], ["t"] * n, np.ones((n, 8), dtype=np.float32), ["Q1"] * n, ["c"] * n,
           ["s"] * n, [float(i) for i in range(n)])
    return st, ix


# ---- offset: validation -------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [-1, True, False, 2.0, "3", [1]])
def test_bad_offsets_raise_value_error(offset):
    st, ix = make_store()
    with pytest.raises(ValueError, match="offset"):
        st.search(Q, "embedding", None, limit=5, offset=offset)
    with pytest.raises(ValueError, match="offset"):
        st.search(Q, "embedding", {"offset": offset}, limit=5)
    assert ix.calls == []


def test_the_window_is_milvus_16384():
    st, ix = make_store()
    with pytest.raises(ValueError, match="16384"):
        st.search(Q, "embedding", None, limit=5, offset=16380)
    with pytest.raises(ValueError, match="16384"):
        st.search(Q, "embedding", None, limit=16384, offset=1)
    assert ix.calls == []
    st.search(Q, "embedding", None, limit=4, offset=16380)
    assert ix.calls[-1] == ("large", 16384, {})
    assert check_offset(None, None, 5) == 0 and check_offset(None, {"offset": 3}, 5) == 3 and check_offset(np.int64(2), None, 5) == 2


def test_keyword_wins_over_param():
    st, ix = make_store()
    hits = st.search(Q, "embedding", {"metric_type": "COSINE", "offset": 9}, limit=5, offset=2)
    assert ix.calls[-1] == ("host", 7, {}) and [h.id for h in hits[0]] == ["k2", "k3", "k4", "k5", "k6"]
    hits = st.search(Q, "embedding", {"metric_type": "COSINE", "offset": 9}, limit=5)
    assert ix.calls[-1] == ("host", 14, {}) and [h.id for h in hits[0]] == [f"k{i}" for i in range(9, 14)]
    hits = st.search(Q, "embedding", {"offset": 9}, limit=5, offset=0)
    assert ix.calls[-1] == ("host", 5, {}) and hits[0][0].id == "k0"


def test_offset_refusals(monkeypatch):
    st, ix = make_store()
    st.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
    with pytest.raises(ValueError, match="offset"):
        st.search(Q, "embedding", None, limit=2, offset=1, group_by_field="period")
    with pytest.raises(ValueError, match="offset"):
        st.search(Q, "embedding", None, limit=2, offset=1, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="offset"):
        st.search(["net profit"], "sparse", {"metric_type": "BM25"}, limit=2, offset=1)
    with pytest.raises(ValueError, match="offset"):
        st.search(["net profit"], "sparse", {"metric_type": "BM25", "offset": 1}, limit=2)
    with pytest.raises(ValueError, match="offset"):
        st.hybrid_search([AnnSearchRequest(Q, "embedding", {"metric_type": "COSINE", "offset": 3}, 5)], RRFRanker(), 5)
    assert ix.calls == []


# ---- the calls the index receives ----------------------------------------------------------------------
def test_with_an_offset_the_index_gets_the_sum_and_the_list_is_sliced(monkeypatch):
    st, ix = make_store()
    hits = st.search(np.ones((2, 8), dtype=np.float32), "embedding", None, limit=10, offset=7)
    assert ix.calls == [("host", 17, {})]
    assert [[h.id for h in hl] for hl in hits] == [[f"k{i}" for i in range(7, 17)]] * 2
    assert hits[0][0].score == np.float32(1.0 - 7 / 1000.0)
    hits = st.search(Q, "embedding", None, limit=30, offset=60)          # past the 64 of one sweep: the paged path
    assert ix.calls[-1] == ("large", 90, {}) and hits == [[]]            # (40 rows: the page lies past the end)
    hits = st.search(Q, "embedding", None, limit=30, offset=35)
    assert ix.calls[-1] == ("large", 65, {}) and [h.id for h in hits[0]] == [f"k{i}" for i in range(35, 40)]
    monkeypatch.setattr(st, "build_filter", lambda expr: "FILTER")
    st.search(Q, "embedding", {"params": {"radius": 0.1, "range_filter": 0.4}}, limit=5, offset=3, expr='period == "Q1"')
    assert ix.calls[-1] == ("host", 8, {"filt": "FILTER", "band": (0.1, 0.4)})
    st.create_index("embedding", {"index_type": "SQ8", "metric_type": "COSINE"})
    st.search(Q, "embedding", None, limit=5, offset=3)
    assert ix.calls[-1] == ("host", 8, {"sq8": True})
    st.search(Q, "embedding", None, limit=5, offset=60)                   # pages past 64 come from the fp16 rows
    assert ix.calls[-1] == ("large", 65, {})


@pytest.mark.parametrize("param", [None, {}, {"metric_type": "COSINE"}, {"metric_type": "COSINE", "params": {"nprobe": 8}}])
def test_without_an_offset_the_calls_are_those_of_today(param):
    st, ix = make_store()
    for kw in ({}, {"offset": 0}, {"offset": None}):
        st.search(Q, "embedding", param, limit=5, **kw)
        assert ix.calls[-1] == ("host", 5, {})
        st.search(Q, "embedding", param, limit=200, **kw)
        assert ix.calls[-1] == ("large", 200, {})
    st.search(Q, "embedding", {"params": {"radius": 0.25}}, limit=200)
    assert ix.calls[-1] == ("large", 200, {"band": (0.25, INF)})
    st.search(Q, "embedding", None, limit=20000)                           # no offset, no window: as today
    assert ix.calls[-1] == ("large", 20000, {})


# ---- query(offset=) ------------------------------------------------------------------------------------
def test_query_offset(monkeypatch):
    st, ix = make_store()
    assert [r["id"] for r in st.query("", limit=3, offset=4)] == ["k4", "k5", "k6"]
    assert [r["id"] for r in st.query("", offset=37)] == ["k37", "k38", "k39"]
    assert st.query("", limit=3, offset=40) == [] and len(st.query("", limit=3)) == 3
    assert [r["id"] for r in st.query('id in ["k9", "k2", "k5"]', offset=1)] == ["k2", "k5"]
    monkeypatch.setattr(st, "_expr_rows", lambda expr: np.arange(10, 20))
    assert [r["id"] for r in st.query("primary_value >= 10", limit=2, offset=3)] == ["k13", "k14"]
    for bad in (-1, True, 1.5):
        with pytest.raises(ValueError, match="offset"):
            st.query("", limit=3, offset=bad)


# ---- search_iterator -----------------------------------------------------------------------------------
def test_iterator_bookkeeping(monkeypatch):
    st, ix = make_store(n=150)
    built = []
    monkeypatch.setattr(st, "build_filter", lambda expr: built.append(expr) or "FILTER")
    it = st.search_iterator(Q, "embedding", {"metric_type": "COSINE", "params": {"radius": 0.5}}, batch_size=100,
                            expr='period == "Q1"', output_fields=["period"])
    a = it.next()
    assert [h.id for h in a] == [f"k{i}" for i in range(100)] and a[3].entity.get("period") == "Q1"
    # ceil(100 / 64) sweeps, each from the last hit of the one before; one filter for all of them
    kw = {"filt": "FILTER", "band": (0.5, INF)}
    assert ix.calls == [("after", 64, (INF, -1), kw), ("after", 36, (1.0 - 63 / 1000.0, 63), kw)]
    b = it.next()
    assert [h.id for h in b] == [f"k{i}" for i in range(100, 150)]
    assert ix.calls[2:] == [("after", 64, (1.0 - 99 / 1000.0, 99), kw)]         # the short page ends the walk
    assert it.next() == [] and it.next() == [] and len(ix.calls) == 3 and built == ['period == "Q1"']
    it.close()


def test_iterator_limit_and_close():
    st, ix = make_store(n=150)
    it = st.search_iterator(Q, batch_size=40, limit=100)
    sizes = [len(it.next()) for _ in range(4)]
    assert sizes == [40, 40, 20, 0]
    assert [c[1] for c in ix.calls] == [40, 40, 20]
    it = st.search_iterator(Q, batch_size=10)
    assert len(it.next()) == 10
    it.close()
    assert it.next() == []
    st0, ix0 = make_store(n=0)
    assert st0.search_iterator(Q).next() == [] and ix0.calls == []


def test_iterator_arguments():
    st, ix = make_store()
    with pytest.raises(ValueError, match="one query vector"):
        st.search_iterator(np.ones((2, 8), dtype=np.float32))
    for kw in ({"batch_size": 0}, {"batch_size": True}, {"batch_size": 16385}, {"limit": 0}, {"limit": -2},
               {"anns_field": "sparse"}, {"param": {"metric_type": "L2"}}, {"param": {"offset": 4}},
               {"param": {"params": {"radius": 0.5, "range_filter": 0.1}}}):
        with pytest.raises(ValueError):
            st.search_iterator(Q, **kw)
    with pytest.raises(KeyError):
        st.search_iterator(Q, output_fields=["nope"])
    assert ix.calls == []


@pytest.mark.parametrize("mutate", ["insert", "delete", "upsert", "drop"])
def test_iterator_refuses_to_go_on_after_a_mutation(mutate, monkeypatch):
    st, ix = make_store(n=30)
    ix.compact = lambda keep: None
    ix.reset = lambda: None
    it = st.search_iterator(Q, batch_size=5)
    assert len(it.next()) == 5
    row = [["new"], ["t"], np.ones((1, 8), dtype=np.float32), ["Q1"], ["c"], ["s"], [1.0]]
    if mutate == "insert":
        st.insert(row)
    elif mutate == "upsert":
        st.upsert(row)
    elif mutate == "drop":
        st.drop()
    else:
        monkeypatch.setattr(st, "_match_mask", lambda expr: np.arange(st.num_entities) == 3)
        st.delete('id in ["k3"]')
    with pytest.raises(RuntimeError, match="changed"):
        it.next()
    fresh = st.search_iterator(Q, batch_size=5)       # a new iterator starts from the collection as it is
    fresh.next()


# ---- upper surfaces -------------------------------------------------------------------------------------
class RecStoreKw(RecStore):
    def __init__(self):
        super().__init__()
        self.kw = []

    def search(self, data, anns_field, param, limit, expr=None, output_fields=None, **kw):
        self.kw.append(kw)
        return super().search(data, anns_field, param, limit, expr, output_fields)


def test_vector_rag_passes_offset_only_when_given():
    from rag_fin_amd.rag import VectorRAG
    rag = VectorRAG("k", embedder=Emb(), store=RecStoreKw())
    rag.search("q", 3)
    rag.search("q", 3, offset=20)
    rag.search("q", 3, offset=0, min_score=0.2)
    rag.search_batch(["a", "b"], 2, offset=5)
    rag.search_batch(["a", "b"], 2)
    assert rag.collection.kw == [{}, {"offset": 20}, {"offset": 0}, {"offset": 5}, {}]
    assert rag.collection.params[2] == {"metric_type": "COSINE", "params": {"radius": 0.2}}
    plain = VectorRAG("k", embedder=Emb(), store=RecStore())          # a store that knows no offset keyword
    plain.search("q", 3)
    plain.search_batch(["a"], 3)
    for kw in ({"rerank": True}, {"hybrid": True}, {"mmr_lambda": 0.5}, {"group_by": "period"}):
        with pytest.raises(ValueError, match="offset"):
            rag.search("q", 3, offset=2, **kw)
        with pytest.raises(ValueError, match="offset"):
            rag.search_batch(["q"], 3, offset=2, **kw)


@pytest.fixture
def fake_rag():
    rag = FakeRag()
    mcp_server.set_rag(rag)
    yield rag
    mcp_server.set_rag(None)


def test_mcp_tool_and_rest_request_carry_offset_only_when_given(fake_rag):
    from rag_fin_amd.adapter import SearchRequest, search_args
    r = mcp_server.search_vectors("net profit Q1", 2, offset=40)
    assert r == {"status": "success", "query": "net profit Q1", "results": [], "result_count": 0}
    assert fake_rag.calls[-1] == ("search", "net profit Q1", 2, None, {"offset": 40})
    mcp_server.search_vectors("net profit Q1", 2, filter="primary_value > 0", offset=0)
    assert fake_rag.calls[-1] == ("search", "net profit Q1", 2, "primary_value > 0", {"offset": 0})
    mcp_server.search_vectors("net profit Q1", 2, min_score=0.1, offset=3)
    assert fake_rag.calls[-1] == ("search", "net profit Q1", 2, None, {"min_score": 0.1, "max_score": None, "offset": 3})
    mcp_server.search_vectors("net profit Q1")                      # the call of today
    assert fake_rag.calls[-1] == ("search", "net profit Q1", 3, None, {})
    assert search_args(SearchRequest(query="hello", top_k=4)) == {"query": "hello", "top_k": 4}
    assert search_args(SearchRequest(query="hello", offset=0)) == {"query": "hello", "top_k": 3, "offset": 0}
    assert search_args(SearchRequest(query="hello", filter="id == 1", offset=60)) == \
        {"query": "hello", "top_k": 3, "filter": "id == 1", "offset": 60}
    for bad in (-1, "many"):
        with pytest.raises(Exception):
            SearchRequest(query="hello", offset=bad)


def test_sharded_store_refuses_paging(one_rank_group):
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    st = ShardedCorpusStore("c", dim=8, capacity=4, index=RangeFakeIndex(8, 4), backend=object())
    with pytest.raises(NotImplementedError, match="offset"):
        st.search(Q, limit=3, offset=2)
    with pytest.raises(NotImplementedError, match="offset"):
        st.search(Q, limit=3, param={"metric_type": "COSINE", "offset": 2})
    with pytest.raises(ValueError):
        st.search(Q, limit=3, offset=-1)
    with pytest.raises(NotImplementedError, match="search_iterator"):
        st.search_iterator(Q)


# ---- C ABI: host-side argument checks (no GPU needed) ----------------------------------------------------
def test_search_after_abi_argument_checks():
    lib = _lib.load_library()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every case below fails its checks first
    big = 1 << 30

    def call(ix=fake, filt=None, k=10, lo=-INF, hi=INF, bs=fake, bi=fake, fn=lib.rf_search_after, extra=()):
        return fn(ix, filt, fake, 1, k, 0, lo, hi, bs, bi, fake, fake, None, fake, fake, big, None, *extra)

    assert call(bs=None) == RF_ERR_INVALID and b"bound" in lib.rf_last_error()
    assert call(bi=None) == RF_ERR_INVALID
    assert call(lo=0.5, hi=0.5) == RF_ERR_INVALID and b"radius" in lib.rf_last_error()
    assert call(lo=0.6, hi=0.5) == RF_ERR_INVALID
    assert call(lo=math.nan) == RF_ERR_INVALID and call(hi=math.nan) == RF_ERR_INVALID
    assert call(k=_lib.RF_MAX_K + 1) == RF_ERR_INVALID and call(k=0) != 0
    assert call(ix=None) == RF_ERR_INVALID
    assert call(filt=ctypes.c_void_p(4100)) == RF_ERR_INVALID            # misaligned filter
    ms = (ctypes.c_float * 4)()
    assert call(fn=lib.rf_search_after_profile, extra=(ms,), ix=None) == RF_ERR_INVALID
    assert call(fn=lib.rf_search_after_profile, extra=(None,)) == RF_ERR_INVALID
