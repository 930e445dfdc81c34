"""Per-query filters through the public surface, with fakes (CPU only): what CorpusStore.search does
with a list expr (refusals, collapse to the existing call, one build per distinct expression, the
caller's order after the internal ordering by filter), VectorRAG.search_batch, the micro-batcher, the
MCP tool's routing, the sharded store's refusal and the host-side argument checks of the new C-ABI
entry points."""
import ctypes
import threading

import numpy as np
import pytest
import torch

from rag_fin_amd import _lib, mcp_server, store as store_mod
from rag_fin_amd.batching import MicroBatcher
from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
from rag_fin_amd.index import plan_filter_chunks
from rag_fin_amd.store import CorpusStore
from test_range_search_cpu import FakeIndex as RangeFakeIndex, one_rank_group  # noqa: F401

RF_ERR_INVALID = -1      # include/ragfin.h
E1, E2, E3 = 'period == "Q1"', 'period == "Q2"', 'primary_value > 3'


class FakeIndex(RangeFakeIndex):
    """The CPU double of tests/test_range_search_cpu.py whose best hit of a query is the row numbered
    by the query's first component: a result names the query it answers."""

    def search_host(self, q16, k, **kw):
        self.calls.append(("host", k, kw, [int(x) for x in q16[:, 0].tolist()]))
        B = q16.shape[0]
        scores = np.full((B, k), -np.inf, dtype=np.float32)
        rows = np.full((B, k), -1, dtype=np.int64)
        scores[:, 0] = 0.5
        rows[:, 0] = q16[:, 0].numpy().astype(np.int64)
        return scores, rows


class FakeMulti:
    def __init__(self, filters, qfilter, n_rows, device):
        self.filters, self.qfilter, self.n_rows = list(filters), [int(g) for g in qfilter], n_rows


def queries(B):
    q = np.zeros((B, 8), dtype=np.float32)
    q[:, 0] = np.arange(B)
    return q


@pytest.fixture
def fake_store(monkeypatch):
    n = 200
    ix = FakeIndex(capacity=256)
    st = CorpusStore("c", dim=8, capacity=256, index=ix)
    st.add([f"k{i}" for i in range(n)], ["t"] * n, np.ones((n, 8), dtype=np.float32), ["Q1"] * n, ["c"] * n,
           ["s"] * n, [float(i) for i in range(n)])
    built = []
    monkeypatch.setattr(st, "build_filter", lambda e: built.append(e) or "F:" + e)
    monkeypatch.setattr(st, "_all_pass_filter", lambda: built.append(None) or "ALL")
    monkeypatch.setattr(store_mod, "MultiFilter", FakeMulti)
    return st, ix, built


# ---- refusals: before anything runs -------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", [
    ({"limit": 65}, "limit"),
    ({"limit": 0}, "limit"),
    ({"offset": 2}, "offset"),
    ({"param": {"metric_type": "COSINE", "offset": 2}}, "offset"),
    ({"param": {"params": {"radius": 0.2}}}, "range"),
    ({"param": {"params": {"radius": 0.2, "range_filter": 0.9}}}, "range"),
    ({"group_by_field": "period"}, "group_by_field"),
    ({"mmr_lambda": 0.5}, "mmr_lambda"),
    ({"mmr_fetch_k": 20}, "mmr_lambda"),
    ({"anns_field": "sparse"}, "sparse"),
])
def test_a_list_expr_refuses_every_other_variant(fake_store, kw, match):
    st, ix, built = fake_store
    args = {"data": queries(2), "anns_field": "embedding", "param": None, "limit": 3, "expr": [E1, E2], **kw}
    with pytest.raises(ValueError, match=match):
        st.search(**args)
    assert ix.calls == [] and built == []


def test_length_and_type_checks_of_the_list(fake_store):
    st, ix, built = fake_store
    with pytest.raises(ValueError, match="3 entries for 2 query vectors"):
        st.search(queries(2), limit=3, expr=[E1, E2, E3])
    with pytest.raises(ValueError, match="1 entries for 2 query vectors"):
        st.search(queries(2), limit=3, expr=(E1,))
    with pytest.raises(ValueError, match="2 entries for 1 query vectors"):
        st.search(queries(1)[0], limit=3, expr=[E1, E2])     # one vector given flat
    with pytest.raises(ValueError, match="entry 1 is int"):
        st.search(queries(2), limit=3, expr=[E1, 7])
    with pytest.raises(ValueError, match="entry 0 is list"):
        st.search(queries(2), limit=3, expr=[[E1], E2])
    assert ix.calls == [] and built == []


def test_the_other_entry_points_take_no_list(fake_store):
    st, ix, built = fake_store
    with pytest.raises(ValueError, match="search_iterator"):
        st.search_iterator(queries(1), limit=5, expr=[E1])
    with pytest.raises(ValueError, match="hybrid_search"):
        st.hybrid_search([AnnSearchRequest(queries(2), "embedding", {"metric_type": "COSINE"}, 5, [E1, E2])], RRFRanker(), 5)
    st2 = CorpusStore("c", dim=8, capacity=8, index=RangeFakeIndex())
    with pytest.raises(ValueError, match="must be a string"):
        st2.query(expr=[E1])
    with pytest.raises(ValueError, match="must be a string"):
        st2.delete([E1])
    assert ix.calls == [] and built == []


# ---- what the index receives ---------------------------------------------------------------------------
def test_equal_entries_collapse_to_the_existing_call(fake_store):
    st, ix, built = fake_store
    res = st.search(queries(3), "embedding", {"metric_type": "COSINE"}, 3, expr=[E1, E1, E1])
    assert built == [E1] and ix.calls == [("host", 3, {"filt": "F:" + E1}, [0, 1, 2])]
    assert [h[0].id for h in res] == ["k0", "k1", "k2"]
    ix.calls.clear()
    st.search(queries(3), "embedding", {"metric_type": "COSINE"}, 3, expr=E1)
    assert ix.calls == [("host", 3, {"filt": "F:" + E1}, [0, 1, 2])]     # the string call: the same arguments
    ix.calls.clear()
    built.clear()
    st.search(queries(3), limit=3, expr=[None, "", "  "])                # no filter anywhere: the unfiltered call
    assert built == [] and ix.calls == [("host", 3, {}, [0, 1, 2])]
    ix.calls.clear()
    st.search(queries(3), limit=3)
    assert ix.calls == [("host", 3, {}, [0, 1, 2])]


def test_distinct_expressions_are_built_once_and_travel_as_one_multi_filter(fake_store):
    st, ix, built = fake_store
    lst = [E2, E1, None, E2, E1, E2, ""]
    res = st.search(queries(7), limit=2, expr=lst, output_fields=["period"])
    assert built == [E2, E1, None]                 # first appearance, each once (None: the all-pass filter)
    assert len(ix.calls) == 1
    kind, k, kw, qs = ix.calls[0]
    assert (kind, k) == ("host", 2) and set(kw) == {"filt"} and isinstance(kw["filt"], FakeMulti)
    mf = kw["filt"]
    assert mf.n_rows == 200 and len(mf.filters) == 3 and len(mf.qfilter) == 7
    want = {None: "ALL", "": "ALL", E1: "F:" + E1, E2: "F:" + E2}
    assert [mf.filters[g] for g in mf.qfilter] == [want[lst[b]] for b in qs]
    assert [h[0].id for h in res] == [f"k{b}" for b in range(7)] and res[0][0].entity.period == "Q1"


def test_caller_order_is_restored_after_the_ordering_by_filter(fake_store):
    st, ix, built = fake_store
    B = 130
    exprs = [E1, E2, E3, None]
    lst = [exprs[(b * 7) % 4] for b in range(B)]
    res = st.search(queries(B), limit=1, expr=lst)
    assert [h[0].id for h in res] == [f"k{b}" for b in range(B)]
    assert sorted(built, key=str) == sorted(exprs, key=str)
    assert [len(c[3]) for c in ix.calls] == [64, 64, 2]
    want = {None: "ALL", E1: "F:" + E1, E2: "F:" + E2, E3: "F:" + E3}
    seen = []
    for _, _, kw, qs in ix.calls:
        f = kw.get("filt")
        if isinstance(f, FakeMulti):
            assert len(f.filters) <= 3 and [f.filters[g] for g in f.qfilter] == [want[lst[b]] for b in qs]
        else:   # a sweep whose queries share one filter: the single-filter call (none: the unfiltered one)
            assert {want[lst[b]] for b in qs} == {f if f is not None else "ALL"}
        seen += qs
    assert sorted(seen) == list(range(B))
    # every sweep holds as few filters as the order by filter allows
    assert sum(len(c[2]["filt"].filters) if isinstance(c[2].get("filt"), FakeMulti) else 1 for c in ix.calls) <= 6


def test_plan_filter_chunks():
    plan = plan_filter_chunks([2, 0, 2, 1, 0], chunk=3)
    assert [(idx.tolist(), used, local.tolist()) for idx, used, local in plan] == \
        [([1, 4, 3], [0, 1], [0, 0, 1]), ([0, 2], [2], [0, 0])]
    assert len(plan_filter_chunks(list(range(200)))) == 4 and all(len(u) <= 64 for _, u, _ in plan_filter_chunks(list(range(200))))


# ---- VectorRAG ----------------------------------------------------------------------------------------
class RecStore:
    num_entities = 0

    def __init__(self):
        self.calls = []

    def load(self):
        pass

    def search(self, data, anns_field, param, limit, expr=None, output_fields=None, **kw):
        self.calls.append((expr, kw))
        return [[] for _ in range(np.asarray(data).shape[0])]


class Emb:
    def encode(self, texts):
        return np.zeros((len(texts), 4), dtype=np.float32)


def test_vector_rag_hands_a_list_through_only_when_given_one():
    from rag_fin_amd.rag import VectorRAG
    rag = VectorRAG("k", embedder=Emb(), store=RecStore())
    rag.search_batch(["a", "b"], 2)
    rag.search_batch(["a", "b"], 2, expr=E1)
    rag.search_batch(["a", "b"], 2, expr=[E1, None])
    assert rag.collection.calls == [(None, {}), (E1, {}), ([E1, None], {})]
    for kw in ({"rerank": True}, {"hybrid": True}, {"min_score": 0.2}, {"max_score": 0.9}, {"group_by": "period"},
               {"mmr_lambda": 0.5}, {"offset": 0}):
        with pytest.raises(ValueError, match="per-query filters"):
            rag.search_batch(["a", "b"], 2, expr=[E1, E2], **kw)
    with pytest.raises(ValueError, match="3 entries for 2 queries"):
        rag.search_batch(["a", "b"], 2, expr=[E1, E2, E3])
    assert len(rag.collection.calls) == 3


# ---- the micro-batcher ---------------------------------------------------------------------------------
class TwoArgRag:
    """search_batch(queries, top_k) as the fakes of tests/test_batching.py: two positional arguments."""

    def __init__(self):
        self.calls = []

    def search_batch(self, queries, top_k):
        self.calls.append((list(queries), top_k))
        return [[{"text": q}] * top_k for q in queries]


class ExprRag(TwoArgRag):
    def search_batch(self, queries, top_k, expr=None):
        self.calls.append((list(queries), top_k, expr))
        return [[{"text": q, "expr": None if expr is None else expr[i]}] * top_k for i, q in enumerate(queries)]


def run_together(mb, requests):
    """One thread per request; max_batch == len(requests), so the worker fires when all are queued."""
    out, errs = {}, {}

    def work(i, args):
        try:
            out[i] = mb.search(*args)
        except Exception as e:   # noqa: BLE001
            errs[i] = e
    ts = [threading.Thread(target=work, args=(i, a)) for i, a in enumerate(requests)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return out, errs


def test_an_unfiltered_batch_calls_search_batch_with_two_positional_arguments():
    rag = TwoArgRag()
    mb = MicroBatcher(rag, max_batch=3, max_wait_ms=60_000)
    out, errs = run_together(mb, [("a", 1), ("b", 2, None), ("c", 1, "  ")])
    mb.close()
    assert not errs and len(rag.calls) == 1
    assert sorted(rag.calls[0][0]) == ["a", "b", "c"] and rag.calls[0][1] == 2 and len(rag.calls[0]) == 2
    assert [len(out[i]) for i in range(3)] == [1, 2, 1]


def test_a_mixed_batch_passes_the_list_with_none_for_the_unfiltered_requests():
    rag = ExprRag()
    mb = MicroBatcher(rag, max_batch=3, max_wait_ms=60_000)
    out, errs = run_together(mb, [("a", 1, E1), ("b", 2), ("c", 1, E2)])
    mb.close()
    assert not errs and len(rag.calls) == 1
    qs, k, exprs = rag.calls[0]
    assert k == 2 and dict(zip(qs, exprs)) == {"a": E1, "b": None, "c": E2}
    assert out[0] == [{"text": "a", "expr": E1}] and out[1][0]["expr"] is None and out[2][0]["expr"] == E2


def test_a_malformed_filter_raises_in_its_own_caller_and_the_others_are_answered():
    rag = ExprRag()
    mb = MicroBatcher(rag, max_batch=2, max_wait_ms=60_000)
    out, errs = run_together(mb, [("a", 1, E1), ("bad", 1, "period >"), ("c", 1)])
    mb.close()
    assert set(errs) == {1} and isinstance(errs[1], ValueError)
    assert len(rag.calls) == 1 and sorted(rag.calls[0][0]) == ["a", "c"] and mb.requests == 2
    assert out[0][0]["expr"] == E1 and out[2][0]["expr"] is None


# ---- the MCP tool ------------------------------------------------------------------------------------
class ToolRag:
    def __init__(self):
        self.single, self.batched = [], []

    def search(self, query, top_k=3, expr=None, **kw):
        self.single.append((query, top_k, expr, kw))
        return []

    def search_batch(self, queries, top_k=3, expr=None):
        self.batched.append((list(queries), top_k, expr))
        return [[] for _ in queries]


@pytest.mark.parametrize("ms,filters,batched", [("5", "1", True), ("5", None, False), ("5", "0", False),
                                                 (None, "1", False), ("0", "1", False)])
def test_a_filter_only_call_is_batched_only_with_both_variables_set(monkeypatch, ms, filters, batched):
    for name, v in (("RAGFIN_MICROBATCH_MS", ms), ("RAGFIN_MICROBATCH_FILTERS", filters)):
        monkeypatch.delenv(name, raising=False) if v is None else monkeypatch.setenv(name, v)
    monkeypatch.setattr(mcp_server, "_batcher", None)
    rag = ToolRag()
    mcp_server.set_rag(rag)
    try:
        assert mcp_server.search_vectors("q", 2, filter=E1)["status"] == "success"
        if batched:
            assert rag.batched == [(["q"], 2, [E1])] and rag.single == []
        else:
            assert rag.single == [("q", 2, E1, {})] and rag.batched == []
        # a filter with any other option is the direct call, as before
        assert mcp_server.search_vectors("q", 2, filter=E1, min_score=0.1)["status"] == "success"
        assert mcp_server.search_vectors("q", 2, filter=E1, mmr_lambda=0.5)["status"] == "success"
        assert len(rag.single) == (2 if batched else 3) and len(rag.batched) == (1 if batched else 0)
        # a malformed filter on the batched route comes back as the error dict of before
        r = mcp_server.search_vectors("q", 2, filter="period >")
        assert (r["status"] == "error") if batched else True
    finally:
        if mcp_server._batcher is not None:
            mcp_server._batcher.close()
        mcp_server.set_rag(None)


# ---- the sharded store ---------------------------------------------------------------------------------
def test_sharded_store_refuses_a_list(one_rank_group):
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    st = ShardedCorpusStore("c", dim=8, capacity=4, index=RangeFakeIndex(8, 4), backend=object())
    for lst in ([E1, E2], [None, None], (E1,)):
        with pytest.raises(NotImplementedError, match="filtered search"):
            st.search(queries(2), limit=3, expr=lst)


# ---- C ABI: host-side argument checks (no GPU needed) --------------------------------------------------
def test_multi_filter_abi_argument_checks():
    lib = _lib.load_library()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every case below fails its checks first
    big = 1 << 30
    assert lib.rf_multi_filter_bytes(100, 0) == 0 and lib.rf_multi_filter_bytes(100, 65) == 0
    assert lib.rf_multi_filter_bytes(-1, 4) == 0 and lib.rf_multi_filter_bytes(1 << 40, 4) == 0
    nblk = (100_003 + 31) // 32
    base = (lib.rf_filter_bytes(100_003) + 255) // 256 * 256
    assert lib.rf_multi_filter_bytes(100_003, 3) == base + nblk * 4 * 4      # G = 3 -> 4 columns
    assert lib.rf_multi_filter_bytes(100_003, 64) == base + nblk * 64 * 4
    two = (ctypes.c_void_p * 2)(fake, fake)
    assert lib.rf_multi_filter_build(None, 2, 100, fake, None) == RF_ERR_INVALID
    assert b"rf_multi_filter_build" in lib.rf_last_error()
    assert lib.rf_multi_filter_build(two, 0, 100, fake, None) == RF_ERR_INVALID
    assert lib.rf_multi_filter_build(two, 65, 100, fake, None) == RF_ERR_INVALID
    assert lib.rf_multi_filter_build(two, 2, 100, None, None) == RF_ERR_INVALID
    assert lib.rf_multi_filter_build(two, 2, 100, ctypes.c_void_p(4100), None) == RF_ERR_INVALID
    assert lib.rf_multi_filter_build(two, 2, -1, fake, None) == RF_ERR_INVALID
    assert lib.rf_multi_filter_build((ctypes.c_void_p * 2)(fake, None), 2, 100, fake, None) == RF_ERR_INVALID
    assert b"filter 1" in lib.rf_last_error()
    assert lib.rf_multi_filter_build((ctypes.c_void_p * 2)(fake, ctypes.c_void_p(4100)), 2, 100, fake, None) == RF_ERR_INVALID
    search = lib.rf_search_multi_filtered
    rest = (fake, 1, 10, 0, fake, fake, None, fake, fake, big, None)
    for G in (0, 65, -3):
        assert search(None, fake, G, fake, *rest) == RF_ERR_INVALID and b"n_filters" in lib.rf_last_error()
    assert search(None, fake, 2, None, *rest) == RF_ERR_INVALID and b"qfilter" in lib.rf_last_error()
    assert search(None, None, 2, fake, *rest) == RF_ERR_INVALID and b"filter buffer" in lib.rf_last_error()
    assert search(None, ctypes.c_void_p(4100), 2, fake, *rest) == RF_ERR_INVALID and b"aligned" in lib.rf_last_error()
    assert search(None, fake, 2, fake, *rest) == RF_ERR_INVALID and b"null argument" in lib.rf_last_error()   # no index
