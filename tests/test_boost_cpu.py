"""Boosted search without a GPU: BoostRanker and its params form, the class weights, the
numpy definition on a hand-worked case, every refusal of CorpusStore.search(ranker=...), VectorRAG
(boost=...), the MCP tool and the REST request, and the host-side argument checks of rf_boost_classes
and rf_merge_boosted (no device call)."""
import ctypes
import math

import numpy as np
import pytest

from rag_fin_amd import _lib, mcp_server, ranker
from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
from rag_fin_amd.ranker import BoostRanker, boost_reference, class_weights
from test_hybrid_surface_cpu import Emb, FakeRag, FakeIndex, RecStore, make_store, one_rank_group  # noqa: F401

COS = {"metric_type": "COSINE"}
Q = np.ones((2, 8), dtype=np.float32)
Q4 = 'period == "Q1"'


# ---- the ranker object ----------------------------------------------------------------------------------
def test_boost_ranker_keeps_its_arguments():
    b = BoostRanker(Q4, 1.5)
    assert (b.filter, b.weight, b.name) == (Q4, 1.5, "boost")
    assert BoostRanker(Q4, 2, name="latest").weight == 2.0 and isinstance(BoostRanker(Q4, 2).weight, float)
    assert BoostRanker(Q4, np.float32(0.5)).weight == 0.5
    assert _lib.RF_BOOST_MAX == ranker.MAX_BOOSTS == 3


@pytest.mark.parametrize("weight", [True, False, float("nan"), float("inf"), -float("inf"), 0, 0.0, -1.5, "2", None,
                                    [1.5]])
def test_a_weight_that_is_no_positive_real_number_raises(weight):
    with pytest.raises(ValueError, match="weight"):
        BoostRanker(Q4, weight)
    with pytest.raises(ValueError, match="weight"):
        BoostRanker.from_params({"reranker": "boost", "filter": Q4, "weight": weight})


@pytest.mark.parametrize("expr", ["", "   ", None, 3, ["period"]])
def test_an_empty_or_non_string_filter_raises(expr):
    with pytest.raises(ValueError, match="filter"):
        BoostRanker(expr, 1.5)


def test_from_params_takes_the_milvus_dict():
    b = BoostRanker.from_params({"reranker": "boost", "filter": Q4, "weight": 0.25})
    assert (b.filter, b.weight) == (Q4, 0.25)
    for params in [{"reranker": "decay", "filter": Q4, "weight": 2.0}, {"filter": Q4, "weight": 2.0},
                   {"reranker": "boost", "filter": Q4, "weight": 2.0, "random_score": {"seed": 1}},
                   {"reranker": "boost", "filter": Q4}, {"reranker": "boost", "weight": 2.0},
                   {"reranker": "boost", "filter": Q4, "weight": 2.0, "boost_mode": "sum"}, "boost", None]:
        with pytest.raises(ValueError, match="boost ranker"):
            BoostRanker.from_params(params)


# ---- class weights ------------------------------------------------------------------------------------------
def test_class_weights_are_the_products_over_the_set_bits_in_boost_order():
    assert class_weights([BoostRanker(Q4, 2.0)]) == [1.0, 2.0]
    assert class_weights([BoostRanker(Q4, 2.0), BoostRanker(Q4, 0.5)]) == [1.0, 2.0, 0.5, 1.0]
    w = [1.1, 1.3, 0.7]
    got = class_weights([BoostRanker(Q4, x) for x in w])
    assert got == [1.0, w[0], w[1], w[0] * w[1], w[2], w[0] * w[2], w[1] * w[2], (w[0] * w[1]) * w[2]]
    assert all(isinstance(x, float) for x in got)


def test_class_weights_refuse_a_product_that_leaves_the_doubles():
    with pytest.raises(ValueError, match="class"):
        class_weights([BoostRanker(Q4, 1e200), BoostRanker(Q4, 1e200)])         # overflows to inf
    with pytest.raises(ValueError, match="class"):
        class_weights([BoostRanker(Q4, 1e-200), BoostRanker(Q4, 1e-200)])       # underflows to 0
    assert class_weights([BoostRanker(Q4, 1e200), BoostRanker(Q4, 1e-200)])[3] == 1e200 * 1e-200
    with pytest.raises(ValueError):
        class_weights([BoostRanker(Q4, 2.0)] * 4)
    with pytest.raises(ValueError):
        class_weights([])


# ---- the definition ---------------------------------------------------------------------------------------
def test_boost_reference_on_a_hand_worked_case():
    #            row:  0     1     2      3     4     5
    s = np.array([[0.5, 0.25, 0.9, -0.4, 0.25, -0.2]])
    cls = np.array([0, 1, 0, 1, 1, 0])
    W = [1.0, 2.0]
    # boosted:        0.5   0.5   0.9   -0.8   0.5   -0.2
    sc, ids, boosted, base = boost_reference(s, None, cls, W, 6)
    # 0.9 first; then three rows tie at 0.5: the base score decides (row 0, s = 0.5), then the row (1 before 4)
    assert ids.tolist() == [[2, 0, 1, 4, 5, 3]]
    assert boosted.tolist() == [[0.9, 0.5, 0.5, 0.5, -0.2, -0.8]]
    assert base.tolist() == [[0.9, 0.5, 0.25, 0.25, -0.2, -0.4]]
    assert sc.dtype == np.float32 and sc.tolist() == [[float(np.float32(x)) for x in boosted[0]]]
    # a weight above 1 pushes a negative score down, one below 1 pulls it up
    assert boost_reference(s, None, cls, [1.0, 0.25], 6)[1].tolist() == [[2, 0, 1, 4, 3, 5]]
    # only passing rows take part; fewer than k: -inf / -1 / -inf / -inf
    sc, ids, boosted, base = boost_reference(s, np.array([0, 1, 0, 1, 0, 0], bool), cls, W, 3)
    assert ids.tolist() == [[1, 3, -1]] and boosted.tolist() == [[0.5, -0.8, -math.inf]]
    assert base.tolist() == [[0.25, -0.4, -math.inf]] and sc.tolist() == [[0.5, float(np.float32(-0.8)), -math.inf]]
    # k below the row count cuts the list
    assert boost_reference(np.vstack([s, -s]), None, cls, W, 2)[1].tolist() == [[2, 0], [3, 5]]


def test_boost_reference_ranks_a_rounding_tie_by_the_base_score():
    """Two scores one ulp apart whose products round to the same double: the larger base score is first,
    whatever the rows."""
    w = 0.7
    x = next(x for x in (0.6 + 1e-3 * i for i in range(1000)) if w * x == w * np.nextafter(x, 1.0))
    s = np.array([[x, np.nextafter(x, 1.0)]])
    sc, ids, boosted, base = boost_reference(s, None, np.array([1, 1]), [1.0, w], 2)
    assert boosted[0, 0] == boosted[0, 1] and ids.tolist() == [[1, 0]] and base[0, 0] > base[0, 1]


# ---- CorpusStore.search(ranker=...) ---------------------------------------------------------------------
BOOST = BoostRanker(Q4, 1.5)


@pytest.mark.parametrize("kw,match", [
    (dict(expr=[Q4, None]), "list expr"),
    (dict(expr=(Q4, Q4)), "list expr"),
    (dict(offset=2), "offset"),
    (dict(param={"metric_type": "COSINE", "offset": 1}), "offset"),
    (dict(param={"metric_type": "COSINE", "params": {"radius": 0.2}}), "range"),
    (dict(param={"metric_type": "COSINE", "params": {"radius": 0.2, "range_filter": 0.9}}), "range"),
    (dict(group_by_field="period"), "group_by_field"),
    (dict(mmr_lambda=0.5), "mmr_lambda"),
    (dict(mmr_fetch_k=20), "mmr_lambda"),
    (dict(anns_field="sparse", data=["net profit"]), "BM25"),
    (dict(data=["net profit"]), "strings"),
    (dict(limit=65), "limit"),
    (dict(limit=0), "limit"),
    (dict(limit=True), "limit"),
    (dict(param={"metric_type": "IP"}), "COSINE"),
])
def test_store_refuses_what_has_no_boosted_form_before_anything_runs(kw, match):
    st = make_store(sparse=False)
    args = dict(data=Q, anns_field="embedding", param=COS, limit=3, ranker=BOOST)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        st.search(**args)
    assert st.index.calls == []


@pytest.mark.parametrize("bad", [Q4, {"filter": Q4, "weight": 1.5}, [], [BOOST] * 4, [BOOST, "x"], RRFRanker(), 1.5])
def test_store_refuses_a_ranker_that_is_no_boost_ranker(bad):
    st = make_store(sparse=False)
    with pytest.raises(ValueError, match="BoostRanker"):
        st.search(Q, "embedding", COS, 3, ranker=bad)
    assert st.index.calls == []


def test_store_refuses_class_weights_that_leave_the_doubles():
    st = make_store(sparse=False)
    with pytest.raises(ValueError, match="class"):
        st.search(Q, "embedding", COS, 3, ranker=[BoostRanker(Q4, 1e200), BoostRanker('period == "Q0"', 1e200)])
    assert st.index.calls == []


def test_iterator_and_hybrid_search_take_no_ranker():
    st = make_store(sparse=False)
    with pytest.raises(ValueError, match="search_iterator"):
        st.search_iterator(Q[:1], "embedding", COS, batch_size=2, ranker=BOOST)
    arms = [AnnSearchRequest(Q, "embedding", COS, 2)]
    with pytest.raises(ValueError, match="hybrid_search"):
        st.hybrid_search(arms, RRFRanker(), limit=2, ranker=BOOST)
    with pytest.raises(ValueError, match="hybrid_search"):
        st.hybrid_search(arms, BOOST, limit=2)
    assert st.index.calls == []


def test_an_empty_store_answers_empty_lists_without_a_launch():
    from rag_fin_amd.store import CorpusStore
    st = CorpusStore("c", dim=8, capacity=4, index=FakeIndex(8, 4))
    assert st.search(Q, "embedding", COS, 3, ranker=BOOST) == [[], []]
    assert st.search(Q, "embedding", COS, 3, expr=Q4, ranker=[BOOST, BoostRanker(Q4, 0.5)]) == [[], []]
    assert st.index.calls == []


def test_sharded_store_refuses_a_ranker(one_rank_group):  # noqa: F811
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    st = ShardedCorpusStore("c", dim=8, capacity=4, index=FakeIndex(8, 4), backend=object())
    with pytest.raises(NotImplementedError, match="boosted search"):
        st.search(Q, "embedding", COS, 3, ranker=BOOST)


# ---- VectorRAG ----------------------------------------------------------------------------------------------
def make_rag():
    from rag_fin_amd.rag import VectorRAG
    return VectorRAG("k", embedder=Emb(), store=RecStore())


def test_vector_rag_passes_the_boosts_on_as_rankers():
    from rag_fin_amd.rag import OUTPUT_FIELDS
    rag = make_rag()
    rag.search("net interest margin", 3, boost={"filter": Q4, "weight": 1.5})
    name, param, limit, kw = rag.collection.calls[-1]
    assert (name, param, limit) == ("search", COS, 3) and set(kw) == {"expr", "output_fields", "ranker"}
    assert [(b.filter, b.weight) for b in kw["ranker"]] == [(Q4, 1.5)] and kw["expr"] is None
    rag.search_batch(["a", "b"], 5, expr='chunk_type == "x"',
                     boost=[{"filter": Q4, "weight": 2}, {"filter": 'TEXT_MATCH(text, "npa")', "weight": 0.5}])
    name, param, limit, kw = rag.collection.calls[-1]
    assert limit == 5 and kw["expr"] == 'chunk_type == "x"'
    assert [(b.filter, b.weight) for b in kw["ranker"]] == [(Q4, 2.0), ('TEXT_MATCH(text, "npa")', 0.5)]
    rag.search("net interest margin", 3)                                           # without it: the call of before
    assert rag.collection.calls[-1] == ("search", COS, 3, {"expr": None, "output_fields": OUTPUT_FIELDS})
    rag.search_batch(["a"], 3, boost=None)
    assert rag.collection.calls[-1] == ("search", COS, 3, {"expr": None, "output_fields": OUTPUT_FIELDS})


@pytest.mark.parametrize("kw", [{"rerank": True}, {"hybrid": True}, {"group_by": "period"}, {"mmr_lambda": 0.5},
                                {"min_score": 0.2}, {"max_score": 0.9}, {"offset": 3}, {"offset": 0}])
def test_vector_rag_refuses_what_does_not_combine_with_a_boost(kw):
    rag = make_rag()
    with pytest.raises(ValueError, match="boost"):
        rag.search("net interest margin", 3, boost={"filter": Q4, "weight": 1.5}, **kw)
    with pytest.raises(ValueError, match="boost"):
        rag.search_batch(["net interest margin"], 3, boost={"filter": Q4, "weight": 1.5}, **kw)
    assert rag.collection.calls == []


@pytest.mark.parametrize("boost", [{"filter": Q4}, {"filter": Q4, "weight": 0}, {"filter": "", "weight": 2.0}, [],
                                   [{"filter": Q4, "weight": 2.0}] * 4, "period", {"filter": Q4, "weight": 2.0, "x": 1},
                                   [BOOST]])
def test_vector_rag_refuses_a_malformed_boost(boost):
    rag = make_rag()
    with pytest.raises(ValueError):
        rag.search("net interest margin", 3, boost=boost)
    with pytest.raises(ValueError, match="list expr"):
        rag.search_batch(["a", "b"], 3, expr=[Q4, None], boost={"filter": Q4, "weight": 2.0})
    assert rag.collection.calls == []


# ---- the MCP tool and the REST request -------------------------------------------------------------------
def test_mcp_tool_carries_one_boost_and_bypasses_the_batcher(monkeypatch):
    def no_batcher():
        raise AssertionError("a boosted call must not reach the micro-batcher")

    rag = FakeRag()
    mcp_server.set_rag(rag)
    monkeypatch.setattr(mcp_server, "_searcher", no_batcher)
    try:
        r = mcp_server.search_vectors("net interest margin", 4, boost_filter=Q4, boost_weight=1.5)
        assert r == {"status": "success", "query": "net interest margin", "results": [], "result_count": 0}
        assert rag.calls[-1] == ("net interest margin", 4, None, {"boost": {"filter": Q4, "weight": 1.5}})
        mcp_server.search_vectors("q", 2, filter='chunk_type == "x"', boost_filter=Q4, boost_weight=0.5)
        assert rag.calls[-1] == ("q", 2, 'chunk_type == "x"', {"boost": {"filter": Q4, "weight": 0.5}})
        mcp_server.search_vectors("q", 2, min_score=0.2, rerank=True, boost_filter=Q4, boost_weight=2.0)
        assert rag.calls[-1] == ("q", 2, None, {"boost": {"filter": Q4, "weight": 2.0}, "min_score": 0.2,
                                                "rerank": True})                   # (VectorRAG refuses the combination)
        n = len(rag.calls)
        for kw in ({"boost_filter": Q4}, {"boost_weight": 1.5}, {"boost_filter": "  ", "boost_weight": 1.5}):
            r = mcp_server.search_vectors("q", 2, **kw)
            assert r["status"] == "error" and "go together" in r["message"]
        assert len(rag.calls) == n
        mcp_server.set_rag(make_rag())
        r = mcp_server.search_vectors("q", 4, group_by="period", boost_filter=Q4, boost_weight=1.5)
        assert r["status"] == "error" and "boost" in r["message"]
        r = mcp_server.search_vectors("q", 4, boost_filter=Q4, boost_weight=-1.0)
        assert r["status"] == "error" and "weight" in r["message"]
    finally:
        mcp_server.set_rag(None)


def test_mcp_tool_without_a_boost_is_the_call_of_before():
    rag = FakeRag()
    mcp_server.set_rag(rag)
    try:
        mcp_server.search_vectors("q", 2)
        assert rag.calls[-1] == ("q", 2, None, {})
        mcp_server.search_vectors("q", 2, filter="primary_value > 0", boost_filter="", boost_weight=None)
        assert rag.calls[-1] == ("q", 2, "primary_value > 0", {})
    finally:
        mcp_server.set_rag(None)


def test_search_request_carries_the_boost_fields():
    from rag_fin_amd.adapter import SearchRequest, search_args
    assert search_args(SearchRequest(query="hello", top_k=4)) == {"query": "hello", "top_k": 4}
    assert search_args(SearchRequest(query="hello", boost_filter=Q4, boost_weight=1.5)) == \
        {"query": "hello", "top_k": 3, "boost_filter": Q4, "boost_weight": 1.5}
    assert search_args(SearchRequest(query="hello", filter="id == 1", boost_filter=Q4, boost_weight=0.5)) == \
        {"query": "hello", "top_k": 3, "filter": "id == 1", "boost_filter": Q4, "boost_weight": 0.5}
    for w in (0, -1.0, "much"):
        with pytest.raises(Exception):
            SearchRequest(query="hello", boost_filter=Q4, boost_weight=w)


# ---- host-side argument checks of the entry points (no device call) ---------------------------------------
P = ctypes.c_void_p(0x1000)   # a non-null, 16-byte aligned address that is never read: every call below is refused


def last_error():
    return _lib.load_library().rf_last_error().decode()


def test_boost_class_stride():
    lib = _lib.load_library()
    assert [lib.rf_boost_class_stride_words(n) for n in (1, 32, 33, 128, 129, 100_003)] == [4, 4, 4, 4, 8, 3128]
    assert [lib.rf_boost_class_stride_words(n) for n in (0, -1, 2 ** 32 - 32, 2 ** 40)] == [0, 0, 0, 0]
    assert lib.rf_boost_class_stride_words(2 ** 32 - 33) == 2 ** 27


def test_boost_classes_abi_argument_checks():
    lib = _lib.load_library()

    def call(filters=(P, P), m=None, n=1000, base=None, masks=P, counts=P, array=True):
        arr = (ctypes.c_void_p * max(1, len(filters)))(*filters) if array else None
        return lib.rf_boost_classes(base, arr, len(filters) if m is None else m, n, masks, counts, None)

    inv = -1
    assert call(array=False) == inv and "rf_boost_classes" in last_error()
    assert call(masks=None) == inv and call(counts=None) == inv
    assert call(m=0) == inv and "outside 1..3" in last_error()
    assert call(filters=(P, P, P, P)) == inv and call(m=-1) == inv
    for n in (0, -5, 2 ** 32 - 32):
        assert call(n=n) == inv and "n_rows" in last_error()
    assert call(masks=ctypes.c_void_p(0x1008)) == inv and "aligned" in last_error()
    assert call(counts=ctypes.c_void_p(0x1004)) == inv and "aligned" in last_error()
    assert call(base=ctypes.c_void_p(0x1004)) == inv and "base filter" in last_error()
    assert call(filters=(P, None)) == inv and "boost filter 1" in last_error()
    assert call(filters=(ctypes.c_void_p(0x1004),)) == inv and "boost filter 0" in last_error()


def test_merge_boosted_abi_argument_checks():
    lib = _lib.load_library()

    def call(exact=P, ids=P, B=2, C=2, k_in=10, w=(1.0, 2.0), k=10, scores=P, out=P, weights=True):
        wh = (ctypes.c_double * max(1, len(w)))(*w) if weights else None
        return lib.rf_merge_boosted(exact, ids, B, C, k_in, wh, k, scores, out, None, None, None)

    inv = -1
    assert call(exact=None) == inv and "rf_merge_boosted" in last_error()
    assert call(ids=None) == inv and call(scores=None) == inv and call(out=None) == inv and call(weights=False) == inv
    assert call(B=0) == inv and call(B=-3) == inv
    assert call(C=0, w=()) == inv and call(C=9, w=(1.0,) * 9) == inv
    assert call(k=0) == inv and call(k=65) == inv and call(k_in=0) == inv and call(k_in=65) == inv
    for bad in (float("nan"), float("inf"), 0.0, -2.0):
        assert call(w=(1.0, bad)) == inv and "class weight 1" in last_error()
