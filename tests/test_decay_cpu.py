"""Decayed search without a GPU: DecayRanker and its params form, the weight definition
(anchors, range, monotonicity, the closed form), the numpy definition of the ranking against a brute-force
sort, every refusal of CorpusStore.search(ranker=DecayRanker(...)), VectorRAG (decay=...), the MCP tool and the
REST request, and the host-side argument checks of the three entry points (no device call)."""
import ctypes
import math

import numpy as np
import pytest

from rag_fin_amd import _lib, mcp_server
from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
from rag_fin_amd.ranker import (DECAY_FUNCTIONS, BoostRanker, DecayRanker, check_rankers, decay_reference,
                                decay_weights_reference, exp2_neg)
from rag_fin_amd.schema import DataType, FieldSchema
from test_dynamic_fields_cpu import HostStore as DynStore, rows as dyn_rows
from test_hybrid_surface_cpu import Emb, FakeRag, FakeIndex, RecStore, make_store, one_rank_group  # noqa: F401

COS = {"metric_type": "COSINE"}
Q = np.ones((2, 8), dtype=np.float32)
Q4 = 'period == "Q1"'
DECAY = DecayRanker("primary_value", "gauss", origin=3.0, scale=2.0)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ULP = 2.0 ** -53


# ---- the ranker object ----------------------------------------------------------------------------------
def test_decay_ranker_keeps_its_arguments():
    d = DecayRanker("fiscal_year", "GAUSS", 2024, 2, offset=1, decay=0.25, name="recent")
    assert (d.field, d.function, d.origin, d.scale, d.offset, d.decay, d.name) == \
        ("fiscal_year", "gauss", 2024.0, 2.0, 1.0, 0.25, "recent")
    assert all(isinstance(v, float) for v in (d.origin, d.scale, d.offset, d.decay))
    assert d.shape == 2.0 and d.function_code == _lib.RF_DECAY_GAUSS == 0          # L = -log2(1/4)
    e = DecayRanker("primary_value", "exp", np.float32(1.5), np.int64(3))
    assert (e.offset, e.decay, e.name, e.shape, e.function_code) == (0.0, 0.5, "decay", 1.0, _lib.RF_DECAY_EXP)
    lin = DecayRanker("primary_value", "Linear", 0, 3, decay=0.25)
    assert lin.shape == 4.0 and lin.function_code == _lib.RF_DECAY_LINEAR == 2     # S = scale / (1 - decay)
    assert DECAY_FUNCTIONS == ("gauss", "exp", "linear")


@pytest.mark.parametrize("kw,match", [
    (dict(field=""), "field"), (dict(field=None), "field"), (dict(field=3), "field"),
    (dict(function="cosine"), "function"), (dict(function=None), "function"), (dict(function=1), "function"),
    (dict(origin=float("nan")), "origin"), (dict(origin=float("inf")), "origin"), (dict(origin="2024"), "origin"),
    (dict(origin=True), "origin"), (dict(origin=None), "origin"),
    (dict(scale=0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=float("inf")), "scale"),
    (dict(scale=float("nan")), "scale"), (dict(scale=True), "scale"), (dict(scale="1"), "scale"),
    (dict(offset=-0.5), "offset"), (dict(offset=float("inf")), "offset"), (dict(offset=float("nan")), "offset"),
    (dict(offset=False), "offset"),
    (dict(decay=0), "decay"), (dict(decay=1), "decay"), (dict(decay=1.5), "decay"), (dict(decay=-0.1), "decay"),
    (dict(decay=float("nan")), "decay"), (dict(decay=True), "decay"), (dict(decay="0.5"), "decay"),
    (dict(name=3), "name"),
    (dict(function="linear", scale=1e308, decay=1 - 2.0 ** -53), "overflows"),
])
def test_a_malformed_decay_ranker_raises(kw, match):
    args = dict(field="primary_value", function="gauss", origin=0.0, scale=1.0)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        DecayRanker(**args)


def test_from_params_round_trip():
    p = {"reranker": "decay", "function": "exp", "origin": 2024, "scale": 3, "offset": 1, "decay": 0.25}
    d = DecayRanker.from_params(p, "fiscal_year")
    assert (d.field, d.function, d.origin, d.scale, d.offset, d.decay) == ("fiscal_year", "exp", 2024.0, 3.0, 1.0, 0.25)
    assert d.to_params() == {"reranker": "decay", "function": "exp", "origin": 2024.0, "scale": 3.0, "offset": 1.0,
                             "decay": 0.25}
    again = DecayRanker.from_params(d.to_params(), d.field)
    assert again.to_params() == d.to_params() and again.shape == d.shape
    short = DecayRanker.from_params({"reranker": "decay", "function": "linear", "origin": 0, "scale": 1}, "primary_value")
    assert (short.offset, short.decay) == (0.0, 0.5)
    for bad, match in (({**p, "random_score": 1}, "unknown"), ({**p, "filter": Q4}, "unknown"),
                       ({**p, "reranker": "boost"}, "decay"), ({k: v for k, v in p.items() if k != "scale"}, "scale"),
                       ({k: v for k, v in p.items() if k != "function"}, "function"), ("decay", "dict")):
        with pytest.raises(ValueError, match=match):
            DecayRanker.from_params(bad, "fiscal_year")


def test_boost_ranker_and_check_rankers_answer_as_before():
    with pytest.raises(ValueError, match="boost ranker"):
        BoostRanker.from_params({"reranker": "decay", "function": "gauss", "origin": 0, "scale": 1})
    for bad in (DECAY, [DECAY], [BoostRanker(Q4, 2.0), DECAY]):
        with pytest.raises(ValueError, match="BoostRanker"):
            check_rankers(bad)
    assert len(check_rankers(BoostRanker(Q4, 2.0))) == 1


# ---- the weights ------------------------------------------------------------------------------------------
def rankers(origin=10.0, scale=4.0, offset=1.5, decay=0.5):
    return [DecayRanker("primary_value", f, origin, scale, offset, decay) for f in DECAY_FUNCTIONS]


def test_weight_anchors():
    for decay in (0.5, 0.25, 0.125):          # L = 1, 2, 3 exactly
        for r in rankers(decay=decay):
            inside = np.array([10.0, 8.5, 11.5, 9.25, np.nextafter(11.5, 0.0)])
            assert decay_weights_reference(inside, r).tolist() == [1.0] * 5, r
            if r.function == "linear" and decay < 0.25:
                # (S - scale) / S with S = scale / (1 - decay) rounded once: the rounding of S comes back
                # (1 - decay) / decay times as large, 7 half-ulps at 1/8; within 2 ulp from decay = 1/4 up
                continue
            at = decay_weights_reference(np.array([10.0 + 1.5 + 4.0, 10.0 - 1.5 - 4.0]), r)
            assert np.all(np.abs(at - decay) <= 2 * np.spacing(decay)), (r, at)
            dead = decay_weights_reference(np.array([np.nan, np.inf, -np.inf]), r)
            assert dead.tolist() == [0.0, 0.0, 0.0], r
    lin = rankers()[2]                         # S = 8: zero from distance offset + 8 on
    assert decay_weights_reference(np.array([19.5, 20.0, 1e300, 0.5, -1e300]), lin).tolist() == [0.0] * 5
    assert decay_weights_reference(np.array([19.0]), lin)[0] == 0.0625
    # int64 columns are rounded to the nearest double first
    y = np.array([2024, 2023, 2026, 2030], dtype=np.int64)
    g = DecayRanker("fiscal_year", "gauss", 2024, 2)
    assert np.array_equal(decay_weights_reference(y, g), decay_weights_reference(y.astype(np.float64), g))
    assert decay_weights_reference(y, g)[[0, 2]].tolist() == [1.0, 0.5]
    with pytest.raises(ValueError, match="int64 or float64"):
        decay_weights_reference(np.array([1.0], dtype=np.float32), g)


def test_int64_extremes_with_a_far_origin_stay_in_range():
    v = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], dtype=np.int64)
    for origin in (-1e300, -9.3e18, 0.0, 9.3e18, 1e300):
        for scale in (1e-300, 1.0, 1e18, 1e300):
            for r in rankers(origin, scale, 0.0) + rankers(origin, scale, 1e19, 0.999):
                w = decay_weights_reference(v, r)
                assert np.all((w >= 0.0) & (w <= 1.0)), (r, w)


def test_exp2_neg_is_exact_at_zero_never_above_one_and_dies_at_the_cutoff():
    assert exp2_neg(np.array([0.0]))[0] == 1.0
    assert exp2_neg(np.array([1.0, 2.0, 10.0, 1022.0, 1074.0])).tolist() == [0.5, 0.25, 2.0 ** -10, 2.0 ** -1022, 2.0 ** -1074]
    assert exp2_neg(np.array([1075.0, 1099.99, 1100.0, 1e300, np.inf, np.nan])).tolist() == [0.0] * 6
    t = np.sort(np.concatenate([np.random.default_rng(1).uniform(0, 1100, 200_000), np.arange(0, 1101, 0.5)]))
    w = exp2_neg(t)
    assert w.max() <= 1.0 and w.min() >= 0.0 and not (np.diff(w) > 0).any()


def test_weights_against_the_closed_form_and_monotone_in_the_distance():
    """For weights >= 2^-64 the relative error against np.exp2 / np.exp is at most 1e-13: the roundings of the
    argument t give about (4 + 4 t) 2^-53, 2.9e-14 at t = 64."""
    rng = np.random.default_rng(2)
    origin, scale, offset = 100.0, 7.0, 3.0
    v = np.sort(np.concatenate([origin + rng.uniform(0, 80, 100_000), origin + np.arange(0, 80, 0.25)]))
    d = np.maximum(0.0, np.abs(v - origin) - offset)
    for decay in (0.5, 0.3, 0.9, 1e-3):
        L = -math.log2(decay)
        g, e, lin = (decay_weights_reference(v, r) for r in rankers(origin, scale, offset, decay))
        for got, want in ((g, np.exp2(-L * (d / scale) ** 2)), (e, np.exp2(-L * (d / scale))),
                          (e, np.exp(math.log(decay) * (d / scale)))):
            big = want >= 2.0 ** -64
            assert big.sum() > 1000
            rel = np.abs(got[big] - want[big]) / want[big]
            assert rel.max() <= 1e-13, (decay, rel.max())
        S = scale / (1 - decay)
        assert np.abs(lin - np.maximum(0.0, (S - d) / S)).max() <= 4 * ULP
        for w in (g, e, lin):          # v ascends from the origin, so the distance does
            assert not (np.diff(w) > 0).any() and w.min() >= 0.0 and w.max() <= 1.0
        # ... and the other side of the origin mirrors it
        assert np.array_equal(decay_weights_reference(2 * origin - v, rankers(origin, scale, offset, decay)[0]), g)


# ---- the ranking ------------------------------------------------------------------------------------------
def brute(s, passing, w, k):
    """The k best passing rows by (w s desc, s desc, row asc), with a plain Python sort."""
    out = []
    for b in range(s.shape[0]):
        rows = [r for r in range(s.shape[1]) if passing is None or passing[r]]
        rows.sort(key=lambda r: (-(w[r] * s[b, r]), -s[b, r], r))
        out.append(rows[:k] + [-1] * (k - len(rows[:k])))
    return out


def check_against_brute(s, passing, w, k):
    sc, ids, dec, base = decay_reference(s, passing, w, k)
    assert ids.tolist() == brute(s, passing, w, k)
    for b in range(s.shape[0]):
        n = int((ids[b] >= 0).sum())
        r = ids[b, :n]
        assert np.array_equal(dec[b, :n], w[r] * s[b, r]) and np.array_equal(base[b, :n], s[b, r])
        assert np.array_equal(sc[b, :n], (w[r] * s[b, r]).astype(np.float32)) and sc.dtype == np.float32
        assert np.all(np.isneginf(dec[b, n:])) and np.all(np.isneginf(base[b, n:])) and np.all(np.isneginf(sc[b, n:]))
    return ids


def test_decay_reference_against_a_brute_force_sort():
    rng = np.random.default_rng(3)
    s = rng.uniform(-1, 1, (3, 60))
    s[:, 30:] = s[:, :30]                                    # duplicated rows: the row number breaks the tie
    w = np.tile(rng.uniform(0, 1, 30), 2)
    w[::5] = 0.0
    check_against_brute(s, None, w, 10)
    check_against_brute(s, rng.uniform(size=60) < 0.4, w, 64)                      # fewer than k passing rows
    ids = check_against_brute(s, None, np.zeros(60), 12)                            # all-zero weights: s, then the row
    order = np.lexsort((np.arange(60), -s[0]))[:12]
    assert ids[0].tolist() == order.tolist()
    neg = -np.abs(s) - 0.01                                                         # all-negative scores
    ids = check_against_brute(neg, None, w, 60)
    assert np.all(w[ids[0, :12]] == 0.0)                                            # weight 0 lifts them to -0: on top
    ids = check_against_brute(neg, w > 0, w, 5)
    check_against_brute(s, np.zeros(60, bool), w, 4)                                # no passing row: all padding
    with pytest.raises(ValueError, match="B, N"):
        decay_reference(s[0], None, w, 3)


def test_decay_reference_on_a_hand_worked_case():
    s = np.array([[0.5, 0.25, 0.9, -0.4, 0.5, -0.2]])
    w = np.array([1.0, 1.0, 0.5, 0.5, 1.0, 0.0])
    sc, ids, dec, base = decay_reference(s, None, w, 6)
    # 0.5 0.25 0.45 -0.2 0.5 -0: rows 0 and 4 tie on both scores, the row decides; -0 == 0 > -0.2
    assert ids.tolist() == [[0, 4, 2, 1, 5, 3]]
    assert dec.tolist() == [[0.5, 0.5, 0.45, 0.25, -0.0, -0.2]] and base.tolist() == [[0.5, 0.5, 0.9, 0.25, -0.2, -0.4]]
    assert decay_reference(s, np.array([0, 1, 0, 1, 0, 0], bool), w, 3)[1].tolist() == [[1, 3, -1]]


# ---- CorpusStore.search(ranker=DecayRanker(...)) ----------------------------------------------------------
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
    (dict(anns_field="vectors"), "unknown vector field"),
    (dict(data=["net profit"]), "strings"),
    (dict(limit=65), "limit"),
    (dict(limit=0), "limit"),
    (dict(limit=True), "limit"),
    (dict(param={"metric_type": "IP"}), "COSINE"),
    (dict(ranker=[DECAY]), "on its own"),
    (dict(ranker=[DECAY, DECAY]), "on its own"),
    (dict(ranker=[BoostRanker(Q4, 2.0), DECAY]), "on its own"),
    (dict(ranker=(DECAY, BoostRanker(Q4, 2.0))), "on its own"),
])
def test_store_refuses_what_has_no_decayed_form_before_anything_runs(kw, match):
    st = make_store(sparse=False)
    args = dict(data=Q, anns_field="embedding", param=COS, limit=3, ranker=DECAY)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        st.search(**args)
    assert st.index.calls == []


FIELDS = [FieldSchema("bank", DataType.VARCHAR), FieldSchema("fiscal_year", DataType.INT64, default=2024),
          FieldSchema("audited", DataType.BOOL, default=False), FieldSchema("weight", DataType.DOUBLE, default=1.0)]


@pytest.mark.parametrize("field,match", [
    ("bank", "VARCHAR"), ("audited", "BOOL"), ("period", "reserved"), ("text", "reserved"), ("id", "reserved"),
    ("embedding", "reserved"), ("$meta", "reserved"), ("listed", "dynamic"), ("nope", "dynamic"),
])
def test_store_refuses_a_field_that_holds_no_number_and_names_it(field, match):
    st = DynStore(fields=FIELDS, enable_dynamic_field=True)
    st.add(*dyn_rows(["a", "b"]), extra={"bank": ["x", "y"], "listed": [1, 2.5]})
    with pytest.raises(ValueError, match=match) as e:
        st.search(np.ones((1, 32), np.float32), "embedding", COS, 2, ranker=DecayRanker(field, "exp", 0, 1))
    assert repr(field) in str(e.value)
    # without dynamic fields a name that is no field is unknown
    with pytest.raises(ValueError, match="unknown") as e:
        DynStore(fields=FIELDS).search(np.ones((1, 32), np.float32), "embedding", COS, 2,
                                       ranker=DecayRanker("nope", "exp", 0, 1))
    assert "'nope'" in str(e.value)


def test_the_numeric_fields_are_accepted():
    st = DynStore(fields=FIELDS)
    assert st._check_decay_field("primary_value") is None
    assert st._check_decay_field("fiscal_year").dtype == DataType.INT64
    assert st._check_decay_field("weight").dtype == DataType.DOUBLE


def test_iterator_and_hybrid_search_take_no_decay_ranker():
    st = make_store(sparse=False)
    with pytest.raises(ValueError, match="search_iterator"):
        st.search_iterator(Q[:1], "embedding", COS, batch_size=2, ranker=DECAY)
    arms = [AnnSearchRequest(Q, "embedding", COS, 2)]
    with pytest.raises(ValueError, match="hybrid_search"):
        st.hybrid_search(arms, RRFRanker(), limit=2, ranker=DECAY)
    with pytest.raises(ValueError, match="hybrid_search"):
        st.hybrid_search(arms, DECAY, limit=2)
    assert st.index.calls == []


def test_an_empty_store_answers_empty_lists_without_a_launch():
    from rag_fin_amd.store import CorpusStore
    st = CorpusStore("c", dim=8, capacity=4, index=FakeIndex(8, 4))
    assert st.search(Q, "embedding", COS, 3, ranker=DECAY) == [[], []]
    assert st.search(Q, "embedding", COS, 3, expr=Q4, ranker=DECAY) == [[], []]
    assert st.index.calls == []


def test_sharded_store_refuses_a_decay_ranker(one_rank_group):  # noqa: F811
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    st = ShardedCorpusStore("c", dim=8, capacity=4, index=FakeIndex(8, 4), backend=object())
    with pytest.raises(NotImplementedError, match="decayed search"):
        st.search(Q, "embedding", COS, 3, ranker=DECAY)


# ---- VectorRAG ----------------------------------------------------------------------------------------------
D = {"field": "fiscal_year", "function": "gauss", "origin": 2024, "scale": 2}


def make_rag():
    from rag_fin_amd.rag import VectorRAG
    return VectorRAG("k", embedder=Emb(), store=RecStore())


def test_vector_rag_passes_the_decay_on_as_a_ranker():
    from rag_fin_amd.rag import OUTPUT_FIELDS
    rag = make_rag()
    rag.search("net interest margin", 3, decay=D)
    name, param, limit, kw = rag.collection.calls[-1]
    assert (name, param, limit) == ("search", COS, 3) and set(kw) == {"expr", "output_fields", "ranker"}
    r = kw["ranker"]
    assert isinstance(r, DecayRanker) and kw["expr"] is None
    assert (r.field, r.function, r.origin, r.scale, r.offset, r.decay) == ("fiscal_year", "gauss", 2024.0, 2.0, 0.0, 0.5)
    rag.search_batch(["a", "b"], 5, expr='chunk_type == "x"', decay={**D, "function": "linear", "offset": 1, "decay": 0.25})
    name, param, limit, kw = rag.collection.calls[-1]
    r = kw["ranker"]
    assert limit == 5 and kw["expr"] == 'chunk_type == "x"' and (r.function, r.offset, r.decay) == ("linear", 1.0, 0.25)
    rag.search("net interest margin", 3, decay=None)                                # without it: the call of before
    assert rag.collection.calls[-1] == ("search", COS, 3, {"expr": None, "output_fields": OUTPUT_FIELDS})


@pytest.mark.parametrize("kw", [{"rerank": True}, {"hybrid": True}, {"group_by": "period"}, {"mmr_lambda": 0.5},
                                {"min_score": 0.2}, {"max_score": 0.9}, {"offset": 3}, {"offset": 0},
                                {"boost": {"filter": Q4, "weight": 1.5}}])
def test_vector_rag_refuses_what_does_not_combine_with_a_decay(kw):
    rag = make_rag()
    with pytest.raises(ValueError, match="decay"):
        rag.search("net interest margin", 3, decay=D, **kw)
    with pytest.raises(ValueError, match="decay"):
        rag.search_batch(["net interest margin"], 3, decay=D, **kw)
    assert rag.collection.calls == []


@pytest.mark.parametrize("decay", [{"field": "fiscal_year"}, {**D, "scale": 0}, {**D, "function": "cosine"}, {**D, "x": 1},
                                   [D], "fiscal_year", DECAY, {**D, "decay": 1.0}])
def test_vector_rag_refuses_a_malformed_decay(decay):
    rag = make_rag()
    with pytest.raises(ValueError):
        rag.search("net interest margin", 3, decay=decay)
    with pytest.raises(ValueError, match="list expr"):
        rag.search_batch(["a", "b"], 3, expr=[Q4, None], decay=D)
    assert rag.collection.calls == []


# ---- the MCP tool and the REST request -------------------------------------------------------------------
def test_mcp_tool_carries_the_decay_and_bypasses_the_batcher(monkeypatch):
    def no_batcher():
        raise AssertionError("a decayed call must not reach the micro-batcher")

    rag = FakeRag()
    mcp_server.set_rag(rag)
    monkeypatch.setattr(mcp_server, "_searcher", no_batcher)
    try:
        r = mcp_server.search_vectors("net interest margin", 4, decay_field="fiscal_year", decay_function="gauss",
                                      decay_origin=2024, decay_scale=2)
        assert r == {"status": "success", "query": "net interest margin", "results": [], "result_count": 0}
        assert rag.calls[-1] == ("net interest margin", 4, None, {"decay": D})
        mcp_server.search_vectors("q", 2, filter='chunk_type == "x"', decay_field="primary_value", decay_function="exp",
                                  decay_origin=0.0, decay_scale=1.5, decay_offset=0.5, decay_rate=0.25)
        assert rag.calls[-1] == ("q", 2, 'chunk_type == "x"', {"decay": {
            "field": "primary_value", "function": "exp", "origin": 0.0, "scale": 1.5, "offset": 0.5, "decay": 0.25}})
        n = len(rag.calls)
        for kw in ({"decay_field": "fiscal_year"}, {"decay_scale": 1.5}, {"decay_field": " ", "decay_function": "exp",
                                                                          "decay_origin": 0, "decay_scale": 1},
                   {"decay_field": "fiscal_year", "decay_function": "exp", "decay_origin": 0}):
            r = mcp_server.search_vectors("q", 2, **kw)
            assert r["status"] == "error" and "go together" in r["message"]
        assert len(rag.calls) == n
        mcp_server.set_rag(make_rag())
        kw = dict(decay_field="fiscal_year", decay_function="gauss", decay_origin=2024, decay_scale=2)
        r = mcp_server.search_vectors("q", 4, group_by="period", **kw)
        assert r["status"] == "error" and "decay" in r["message"]
        r = mcp_server.search_vectors("q", 4, boost_filter=Q4, boost_weight=2.0, **kw)
        assert r["status"] == "error" and "decay" in r["message"]
        r = mcp_server.search_vectors("q", 4, **{**kw, "decay_scale": -1.0})
        assert r["status"] == "error" and "scale" in r["message"]
    finally:
        mcp_server.set_rag(None)


def test_search_request_carries_the_decay_fields():
    from rag_fin_amd.adapter import SearchRequest, search_args
    assert search_args(SearchRequest(query="hello", top_k=4)) == {"query": "hello", "top_k": 4}
    req = SearchRequest(query="hello", decay_field="fiscal_year", decay_function="gauss", decay_origin=2024, decay_scale=2)
    assert search_args(req) == {"query": "hello", "top_k": 3, "decay_field": "fiscal_year", "decay_function": "gauss",
                                "decay_origin": 2024.0, "decay_scale": 2.0}
    req = SearchRequest(query="hello", filter="id == 1", decay_field="f", decay_function="exp", decay_origin=0,
                        decay_scale=1, decay_offset=0.5, decay_rate=0.25)
    assert search_args(req)["decay_offset"] == 0.5 and search_args(req)["decay_rate"] == 0.25
    for kw in ({"decay_scale": 0}, {"decay_offset": -1}, {"decay_rate": 1.0}, {"decay_rate": 0}, {"decay_origin": "then"}):
        with pytest.raises(Exception):
            SearchRequest(query="hello", **kw)


# ---- host-side argument checks of the entry points (no device call) ---------------------------------------
P = ctypes.c_void_p(0x1000)   # a non-null, 16-byte aligned address that is never read: every call below is refused


def last_error():
    return _lib.load_library().rf_last_error().decode()


def test_decay_weights_abi_argument_checks():
    lib = _lib.load_library()

    def call(col=P, n=1000, fn=0, origin=0.0, scale=1.0, offset=0.0, shape=1.0, w64=P, w32=P):
        return lib.rf_decay_weights(col, 1, n, fn, origin, scale, offset, shape, w64, w32, None)

    inv = -1
    assert call(col=None) == inv and "rf_decay_weights" in last_error()
    assert call(w64=None) == inv and call(w32=None) == inv
    assert call(n=-1) == inv and call(n=2 ** 32 - 32) == inv
    assert call(fn=3) == inv and call(fn=-1) == inv and "function" in last_error()
    for bad in (dict(origin=math.nan), dict(origin=math.inf), dict(scale=0.0), dict(scale=-1.0), dict(scale=math.inf),
                dict(scale=math.nan), dict(offset=-1.0), dict(offset=math.nan), dict(offset=math.inf), dict(shape=0.0),
                dict(shape=math.nan), dict(shape=math.inf)):
        assert call(**bad) == inv, bad
    assert call(col=ctypes.c_void_p(0x1004)) == inv and call(w32=ctypes.c_void_p(0x1002)) == inv
    assert call(n=0) == 0                                                           # nothing to do, nothing launched


def test_search_weighted_abi_argument_checks():
    lib = _lib.load_library()
    big = lib.rf_search_workspace_bytes(None)

    def call(fn, ix=P, filt=None, w32=P, w64=P, q=P, B=1, k=10, scores=P, ids=P, ws=P, nbytes=big, flags=True):
        tail = (P,) if flags else ()
        return fn(ix, filt, w32, w64, q, B, k, 0, scores, ids, None, None, *tail, ws, nbytes, None)

    for fn, flags in ((lib.rf_search_weighted, True), (lib.rf_search_exhaustive_weighted, False)):
        inv = -1
        assert call(fn, flags=flags, ix=None) == inv
        assert call(fn, flags=flags, w32=None) == inv and "weights" in last_error()
        assert call(fn, flags=flags, w64=None) == inv
        assert call(fn, flags=flags, w32=ctypes.c_void_p(0x1004)) == inv and call(fn, flags=flags, w64=ctypes.c_void_p(0x1004)) == inv
        assert call(fn, flags=flags, q=None) == inv and call(fn, flags=flags, B=0) == inv
        assert call(fn, flags=flags, k=65) == -2 and call(fn, flags=flags, k=0) == -2
        assert call(fn, flags=flags, nbytes=1024) == -3
