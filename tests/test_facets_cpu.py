"""Faceted counts on the CPU: facets_reference (the definition the device is tested against, rag_fin_amd/facets.py)
against hand-written expectations, the helpers the device path shares with it (value ranks, int64 and fp64 range
bounds), the argument checks of facets() and query(..., ["count(*)"]) on a store over the CPU double of GpuIndex,
the sharded store's refusal, and the tool and REST plumbing through a fake rag.  The device side is covered by
tests/test_facets_gpu.py."""
import math

import numpy as np
import pytest

from rag_fin_amd import _lib, facets, mcp_server
from rag_fin_amd.schema import DataType, FieldSchema
from rag_fin_amd.store import CorpusStore
from test_extra_fields_cpu import CpuIndex, rows

NAN, INF = float("nan"), float("inf")
FIELDS = [FieldSchema("bank", DataType.VARCHAR, default="ICICI"), FieldSchema("fiscal_year", DataType.INT64, default=2024),
          FieldSchema("audited", DataType.BOOL, default=False), FieldSchema("weight", DataType.DOUBLE, default=1.0),
          FieldSchema("tags", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=8, default=[]),
          FieldSchema("years", DataType.ARRAY, element_type=DataType.INT64, max_capacity=8, default=[])]


class HostStore(CorpusStore):
    def __init__(self, fields=None, enable_dynamic_field=False):
        super().__init__("t", dim=32, capacity=16, index=CpuIndex(32, 16), fields=fields,
                         enable_dynamic_field=enable_dynamic_field)

    def _grow(self, need):
        self.index.capacity = max(need, 2 * self.index.capacity)


def ref(columns, fields, rows_, schema=FIELDS, dynamic=None, **kw):
    return facets.facets_reference(columns, schema, dynamic, fields, rows_, **kw)


# ---- the definition ------------------------------------------------------------------------------------
def test_buckets_order_and_a_tie_cut_by_value_not_by_first_seen_order():
    # first-seen order zeta, alpha, mid: a dictionary's codes would be 0, 1, 2, the sorted order is alpha, mid, zeta
    cols = {"bank": ["zeta", "alpha", "mid", "zeta", "alpha", "mid", "top", "top", "top"]}
    got = ref(cols, ["bank"], range(9), limit=2)["facets"]["bank"]
    assert got == {"buckets": [{"value": "top", "count": 3}, {"value": "alpha", "count": 2}], "distinct": 4,
                   "missing": 0, "other": 4}
    assert list(facets.value_ranks(["zeta", "alpha", "mid", "top"])) == [3, 0, 1, 2]
    got = ref(cols, ["bank"], range(9), limit=3)["facets"]["bank"]
    assert [b["value"] for b in got["buckets"]] == ["top", "alpha", "mid"] and got["other"] == 2
    # code points, not locale: "Z" < "a"; ints numerically; False < True
    assert [b["value"] for b in ref({"bank": ["a", "Z"]}, ["bank"], [0, 1])["facets"]["bank"]["buckets"]] == ["Z", "a"]
    assert [b["value"] for b in ref({"fiscal_year": [10, 9, -1]}, ["fiscal_year"], range(3))["facets"]["fiscal_year"]["buckets"]] \
        == [-1, 9, 10]
    assert [b["value"] for b in ref({"audited": [True, False]}, ["audited"], range(2))["facets"]["audited"]["buckets"]] \
        == [False, True]


def test_other_missing_distinct_identities_and_min_count():
    cols = {"bank": list("aaabbc") + ["gone"], "period": ["p"] * 7}
    got = ref(cols, ["bank", "period"], range(6), limit=1)
    assert got["count"] == 6
    f = got["facets"]["bank"]
    assert f == {"buckets": [{"value": "a", "count": 3}], "distinct": 3, "missing": 0, "other": 3}   # "gone" passes nowhere
    assert sum(b["count"] for b in f["buckets"]) + f["other"] + f["missing"] == got["count"]
    f = ref(cols, ["bank"], range(6), min_count=2)["facets"]["bank"]
    assert f == {"buckets": [{"value": "a", "count": 3}, {"value": "b", "count": 2}], "distinct": 3, "missing": 0, "other": 1}
    f = ref(cols, ["bank"], [], min_count=2)["facets"]["bank"]
    assert f == {"buckets": [], "distinct": 0, "missing": 0, "other": 0}


def test_an_array_row_counts_once_per_distinct_element():
    cols = {"tags": [["npa", "npa", "casa"], [], ["npa"], ["casa", "casa"], []]}
    got = ref(cols, ["tags"], range(5))
    f = got["facets"]["tags"]
    assert f == {"buckets": [{"value": "casa", "count": 2}, {"value": "npa", "count": 2}], "distinct": 2, "missing": 2,
                 "other": 0}
    units = f["missing"] + 4   # (row, distinct value) pairs: (0, npa) (0, casa) (2, npa) (3, casa)
    assert sum(b["count"] for b in f["buckets"]) + f["other"] + f["missing"] == units
    assert ref(cols, ["tags"], [1, 4])["facets"]["tags"] == {"buckets": [], "distinct": 0, "missing": 2, "other": 0}


def test_dynamic_keys_of_mixed_classes():
    dyn = {"rating": ["AA", True, 3, 2.5, None, "AA", False, True]}
    cols = {"id": list(range(8))}
    for name in ("rating", '$meta["rating"]', "$meta['rating']"):
        f = ref(cols, [name], range(8), schema=(), dynamic=dyn)["facets"][name]
        assert f == {"buckets": [{"value": True, "count": 2}, {"value": "AA", "count": 2}, {"value": False, "count": 1}],
                     "distinct": 3, "missing": 3, "other": 0}
    # a key no row holds: every passing row is missing
    assert ref(cols, ["nope"], range(8), schema=(), dynamic=dyn)["facets"]["nope"] == \
        {"buckets": [], "distinct": 0, "missing": 8, "other": 0}
    with pytest.raises(ValueError, match="enable_dynamic_field"):
        ref(cols, ['$meta["rating"]'], range(8), schema=(), dynamic=None)


def test_ranges_int64_never_go_through_a_double():
    big = 2 ** 53
    cols = {"fiscal_year": [big, big + 1, -2 ** 63, 2 ** 63 - 1, 0]}
    rs = [(None, big + 1), (big + 1, None), (-2 ** 63, 2 ** 63), (-2 ** 64, -2 ** 63), (2 ** 63, None), (0.5, 1.5), (-0.5, 0.5)]
    got = ref(cols, [], range(5), ranges={"fiscal_year": rs})["ranges"]["fiscal_year"]
    assert [r["count"] for r in got["ranges"]] == [3, 2, 5, 0, 0, 0, 1]
    assert (got["min"], got["max"], got["nan"]) == (-2 ** 63, 2 ** 63 - 1, 0)
    assert got["ranges"][0] == {"from": None, "to": big + 1, "count": 3}
    # what the device compares with: clamped as the expression compiler clamps
    assert facets.int_bounds(None, big + 1) == (True, False, False, 0, big + 1)
    assert facets.int_bounds(-2 ** 63, 2 ** 63) == (False, True, False, -2 ** 63, 0)
    assert facets.int_bounds(-2 ** 64, -2 ** 63)[:3] == (True, False, True)
    assert facets.int_bounds(2 ** 63, None)[2] is True
    assert facets.int_bounds(0.5, 1.5) == (False, False, False, 1, 2)
    assert facets.int_bounds(-INF, INF)[:3] == (True, True, False) and facets.int_bounds(INF, None)[2] and \
        facets.int_bounds(None, -INF)[2]
    for lo, hi in rs:   # the clamped bounds select the same int64 values
        no_lo, no_hi, empty, ilo, ihi = facets.int_bounds(lo, hi)
        for v in cols["fiscal_year"] + [1, -1, big - 1]:
            want = (lo is None or v >= lo) and (hi is None or v < hi)
            assert want == (not empty and (no_lo or v >= ilo) and (no_hi or v < ihi)), (lo, hi, v)


def test_ranges_nan_infinities_and_overlaps():
    cols = {"primary_value": [NAN, -INF, INF, 0.0, 999.999, 1000.0, -1.5, NAN]}
    rs = [(None, 0), (0, 1000), (1000, None), (None, None), (-INF, INF), (500, 2000), (-2, 1000.0)]
    got = ref(cols, [], range(8), ranges={"primary_value": rs})["ranges"]["primary_value"]
    assert [r["count"] for r in got["ranges"]] == [2, 2, 2, 6, 5, 2, 3]
    assert (got["min"], got["max"], got["nan"]) == (-INF, INF, 2)
    got = ref(cols, [], [0, 7], ranges={"primary_value": [(None, None)]})["ranges"]["primary_value"]
    assert got == {"ranges": [{"from": None, "to": None, "count": 0}], "min": None, "max": None, "nan": 2}
    # an int bound no double holds is moved up to the next double: the same doubles pass
    no_lo, no_hi, flo, fhi = facets.float_bounds(2 ** 53 + 1, None)
    assert (no_lo, no_hi, flo) == (False, True, float(2 ** 53 + 2))
    assert facets.float_bounds(None, 10 ** 400)[3] == INF and facets.float_bounds(-10 ** 400, 0.5)[2:] == (-INF, 0.5)


@pytest.mark.parametrize("name", ["weight", "primary_value", "text", "id", "embedding", "years", "nope", "$meta"])
def test_fields_that_cannot_be_value_faceted(name):
    with pytest.raises(ValueError, match="facets: .*" + name.replace("$", r"\$") + ".*offered on period"):
        facets.resolve_value_field(name, FIELDS, False)


def test_fields_that_can_and_range_fields():
    kinds = {n: facets.resolve_value_field(n, FIELDS, True)[0] for n in
             ("period", "chunk_type", "statement_type", "bank", "fiscal_year", "audited", "tags", "anything", '$meta["a b"]')}
    assert kinds == {"period": "builtin", "chunk_type": "builtin", "statement_type": "builtin", "bank": "own",
                     "fiscal_year": "own", "audited": "own", "tags": "array", "anything": "dynamic", '$meta["a b"]': "dynamic"}
    assert facets.resolve_value_field('$meta["a b"]', FIELDS, True)[1] == "a b"
    assert facets.resolve_range_field("primary_value", FIELDS) == ("f64", "primary_value")
    assert facets.resolve_range_field("fiscal_year", FIELDS) == ("i64", "fiscal_year")
    assert facets.resolve_range_field("weight", FIELDS) == ("f64", "weight")
    for bad in ("bank", "years", "audited", "nope", "period"):
        with pytest.raises(ValueError, match="range facets are offered on"):
            facets.resolve_range_field(bad, FIELDS)


@pytest.mark.parametrize("kw, match", [
    (dict(fields="bank"), "list of field names"), (dict(fields=[1]), "non-empty string"),
    (dict(fields=["bank", "bank"]), "twice"), (dict(fields=[f"f{i}" for i in range(17)]), "at most 16"),
    (dict(fields=["bank"], limit=0), "limit"), (dict(fields=["bank"], limit=1001), "limit"),
    (dict(fields=["bank"], limit=True), "limit"), (dict(fields=["bank"], limit=2.0), "limit"),
    (dict(fields=["bank"], min_count=0), "min_count"), (dict(fields=["bank"], min_count="1"), "min_count"),
    (dict(fields=[]), "nothing to count"), (dict(fields=None, ranges={}), "nothing to count"),
    (dict(fields=[], ranges=[("a", 1)]), "ranges must be a dict"),
    (dict(fields=[], ranges={"fiscal_year": []}), "1..64"),
    (dict(fields=[], ranges={"fiscal_year": [(0, 1)] * 65}), "1..64"),
    (dict(fields=[], ranges={"fiscal_year": [(0, 1, 2)]}), "pair"),
    (dict(fields=[], ranges={"fiscal_year": [(0, "1")]}), "real number or None"),
    (dict(fields=[], ranges={"fiscal_year": [(NAN, 1)]}), "real number or None"),
    (dict(fields=[], ranges={"fiscal_year": [(0, np.float32("nan"))]}), "real number or None"),
    (dict(fields=[], ranges={"weight": [(np.float64("nan"), None)]}), "real number or None"),
    (dict(fields=[], ranges={"fiscal_year": [(True, 1)]}), "real number or None"),
    (dict(fields=[], ranges={"bank": [(0, 1)]}), "range facets are offered on"),
    (dict(fields=["weight"]), "DOUBLE"), (dict(fields=["bank"], expr=5), "must be a string"),
])
def test_facets_refuses_bad_arguments_before_any_device_call(kw, match):
    st = HostStore(fields=FIELDS)
    d = rows(["a", "b"])
    st.add(d[0], d[1], d[2], *d[3:])
    with pytest.raises(ValueError, match=match):
        st.facets(**kw)


def test_an_empty_store_facets_to_nothing():
    st = HostStore(fields=FIELDS)
    assert st.facets(["bank", "tags"], ranges={"fiscal_year": [(0, None)]}) == {
        "count": 0, "facets": {"bank": {"buckets": [], "distinct": 0, "missing": 0, "other": 0},
                               "tags": {"buckets": [], "distinct": 0, "missing": 0, "other": 0}},
        "ranges": {"fiscal_year": {"ranges": [{"from": 0, "to": None, "count": 0}], "min": None, "max": None, "nan": 0}}}
    with pytest.raises(ValueError):
        st.facets(["bank"], expr="bank ==")


def test_count_star_on_a_host_store():
    st = HostStore(fields=FIELDS)
    assert st.query("", output_fields=["count(*)"]) == [{"count(*)": 0}]
    d = rows(["a", "b", "c"])
    st.add(d[0], d[1], d[2], *d[3:])
    assert st.query("", output_fields=["count(*)"]) == [{"count(*)": 3}]
    assert st.query(None, output_fields=("count(*)",)) == [{"count(*)": 3}]
    assert st.query('id in ["a", "zz", "c", "a"]', output_fields=["count(*)"]) == [{"count(*)": 2}]
    for kw, match in ((dict(output_fields=["count(*)", "id"]), "output_fields"), (dict(output_fields=["count(*)"], limit=1), "limit"),
                      (dict(output_fields=["count(*)"], offset=1), "offset")):
        with pytest.raises(ValueError, match="count\\(\\*\\) cannot be combined with (other )?" + match):
            st.query("", **kw)
    # every other query is as before
    assert [r["id"] for r in st.query("", limit=2)] == ["a", "b"]
    assert st.query('id in ["c"]', output_fields=["period"]) == [{"period": "Q1_FY2024", "id": "c"}]
    with pytest.raises(KeyError):
        st.query("", output_fields=["count"])


def test_the_sharded_store_raises():
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    with pytest.raises(NotImplementedError, match="faceted counts are not implemented for the sharded store"):
        ShardedCorpusStore.facets(object(), ["period"])
    # count(*) keeps the sharded query's refusal of a general expression, before any filter is built

    class Stub:
        _expr_rows = ShardedCorpusStore._expr_rows
    with pytest.raises(NotImplementedError, match="supports '' and 'id in"):
        ShardedCorpusStore._count(Stub(), "period == 'Q1'")


def test_constants_agree_with_the_library():
    assert (facets.MAX_LIMIT, facets.MAX_RANGES, facets.MAX_FIELDS) == \
        (_lib.RF_FACET_MAX_LIMIT, _lib.RF_FACET_MAX_RANGES, _lib.RF_FACET_MAX_FIELDS)
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ragfin.h")).read()
    for name in ("RF_FACET_MAX_FIELDS", "RF_FACET_LDS_CODES", "RF_FACET_MAX_LIMIT", "RF_FACET_SCALARS", "RF_FACET_MAX_RANGES",
                 "RF_FACET_CODES", "RF_FACET_ARRAY", "RF_FACET_DYNAMIC", "RF_FRANGE_NO_LO", "RF_FRANGE_NO_HI", "RF_FRANGE_EMPTY"):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(_lib, name), name


def test_the_library_checks_its_arguments_without_a_gpu():
    """Every refusal comes before any device call."""
    import ctypes
    lib = _lib.load_library()
    f = (_lib.FacetField * 1)()
    f[0].kind, f[0].n_codes, f[0].a_dev, f[0].counter_off = _lib.RF_FACET_CODES, 4, 64, 0
    buf = ctypes.c_void_p(4096)
    assert lib.rf_facet_counts(None, f, 1, 10, None, 5, None) == -1
    assert lib.rf_facet_counts(None, f, 0, 10, buf, 5, None) == -1
    assert lib.rf_facet_counts(None, f, 17, 10, buf, 5, None) == -1
    assert lib.rf_facet_counts(None, f, 1, 10, buf, 4, None) == -1          # 4 bins + missing need 5 counters
    assert lib.rf_facet_counts(None, f, 1, -1, buf, 5, None) == -1
    assert lib.rf_facet_counts(ctypes.c_void_p(8), f, 1, 10, buf, 5, None) == -1   # a misaligned filter
    f[0].kind = 9
    assert lib.rf_facet_counts(None, f, 1, 10, buf, 5, None) == -1
    f[0].kind, f[0].a_dev = _lib.RF_FACET_ARRAY, 64
    assert lib.rf_facet_counts(None, f, 1, 10, buf, 5, None) == -1          # no values, no flags
    f[0].kind = _lib.RF_FACET_CODES
    assert lib.rf_facet_select(f, 1, buf, 5, 10, 1, buf, None) == -1         # no ranks
    f[0].rank_dev = 64
    assert lib.rf_facet_select(f, 1, buf, 5, 0, 1, buf, None) == -1
    assert lib.rf_facet_select(f, 1, buf, 5, 1001, 1, buf, None) == -1
    assert lib.rf_facet_select(f, 1, buf, 5, 10, 0, buf, None) == -1
    assert b"rf_facet_select" in lib.rf_last_error()
    r = (_lib.FacetRange * 1)()
    assert lib.rf_facet_ranges(None, buf, 1, r, 0, 10, buf, None) == -1
    assert lib.rf_facet_ranges(None, buf, 1, r, 65, 10, buf, None) == -1
    assert lib.rf_facet_ranges(None, None, 1, r, 1, 10, buf, None) == -1
    r[0].flags = 1
    assert lib.rf_facet_ranges(None, buf, 1, r, 1, 10, buf, None) == -1
    assert lib.rf_array_first_occurrence(None, buf, 0, 1, buf, None) == -1
    assert lib.rf_array_first_occurrence(buf, buf, 2, 1, buf, None) == -1


# ---- the tool and the REST body, through a fake rag -----------------------------------------------------------
class FakeRag:
    def __init__(self):
        self.calls = []
        outer = self

        class Collection:
            num_entities = 5

            def query(self, expr="", limit=None, output_fields=None, offset=0):
                outer.calls.append(("query", expr, tuple(output_fields)))
                return [{"count(*)": 2}]
        self.collection = Collection()

    def facets(self, fields=None, expr=None, limit=10, min_count=1, ranges=None):
        self.calls.append(("facets", tuple(fields), expr, limit))
        return {"count": 3, "facets": {f: {"buckets": [], "distinct": 0, "missing": 0, "other": 0} for f in fields},
                "ranges": {}}


def test_the_tool_carries_the_call_through():
    rag = FakeRag()
    mcp_server.set_rag(rag)
    try:
        plain = mcp_server.get_collection_stats()
        assert set(plain) == {"status", "collection_name", "total_chunks", "milvus_host", "milvus_port"} and not rag.calls
        got = mcp_server.get_collection_stats(expr="fiscal_year >= 2023", facet_fields=["period", "bank"], facet_limit=4)
        assert rag.calls == [("facets", ("period", "bank"), "fiscal_year >= 2023", 4)]
        assert got["count"] == 3 and set(got["facets"]) == {"period", "bank"} and got["total_chunks"] == 5
        assert set(got) == set(plain) | {"count", "facets"}
        got = mcp_server.get_collection_stats(expr="period == 'Q1'")
        assert rag.calls[-1] == ("query", "period == 'Q1'", ("count(*)",)) and got["count"] == 2 and got["facets"] == {}
        mcp_server.get_collection_stats(expr="  ", facet_fields=["period"])
        assert rag.calls[-1] == ("facets", ("period",), None, 10)
        rag.facets = lambda *a, **k: (_ for _ in ()).throw(ValueError("facets: unknown field 'x'"))
        assert mcp_server.get_collection_stats(facet_fields=["x"]) == {"status": "error", "message": "facets: unknown field 'x'"}
        assert [f.__name__ for f in mcp_server.TOOLS] == ["health_check", "search_vectors", "answer_question",
                                                          "get_collection_stats"]
    finally:
        mcp_server.set_rag(None)


def test_vector_rag_hands_the_call_on():
    from rag_fin_amd.rag import VectorRAG
    seen = {}

    class Store:
        num_entities = 0

        def load(self):
            pass

        def facets(self, fields, expr=None, limit=10, min_count=1, ranges=None):
            seen.update(fields=fields, expr=expr, limit=limit, min_count=min_count, ranges=ranges)
            return {"count": 0, "facets": {}, "ranges": {}}
    rag = VectorRAG("k", "c", embedder=object(), store=Store())
    assert rag.facets(["period"], expr="x > 1", limit=3, min_count=2, ranges={"primary_value": [(0, 1)]}) == \
        {"count": 0, "facets": {}, "ranges": {}}
    assert seen == dict(fields=["period"], expr="x > 1", limit=3, min_count=2, ranges={"primary_value": [(0, 1)]})


def test_the_rest_body(monkeypatch):
    import json

    import httpx
    from fastapi.testclient import TestClient
    from pydantic import ValidationError
    from rag_fin_amd import adapter
    assert adapter.stats_args(adapter.StatsRequest()) == {}
    assert adapter.stats_args(adapter.StatsRequest(expr="a > 1")) == {"expr": "a > 1"}
    assert adapter.stats_args(adapter.StatsRequest(facet_fields=["period"], facet_limit=5)) == \
        {"facet_fields": ["period"], "facet_limit": 5}
    for bad in (dict(facet_limit=0), dict(facet_limit=1001), dict(facet_fields=["f"] * 17)):
        with pytest.raises(ValidationError):
            adapter.StatsRequest(**bad)
    seen = []

    def handler(request: httpx.Request):
        body = json.loads(request.content)
        if body["method"] == "initialize":
            return httpx.Response(200, headers={"mcp-session-id": "s"}, json={"result": {}})
        if body["method"] == "notifications/initialized":
            return httpx.Response(202)
        seen.append(body["params"])
        payload = "event: message\ndata: " + json.dumps({"jsonrpc": "2.0", "id": 1, "result": {"status": "success"}}) + "\n\n"
        return httpx.Response(200, text=payload, headers={"content-type": "text/event-stream"})
    monkeypatch.setattr(adapter, "mcp", adapter.MCPClient("http://mcp.test/mcp",
                                                          httpx.AsyncClient(transport=httpx.MockTransport(handler))))
    tc = TestClient(adapter.app)
    assert tc.post("/stats", json={"expr": "fiscal_year >= 2023", "facet_fields": ["period"]}).json() == {"status": "success"}
    assert seen[-1] == {"name": "get_collection_stats",
                        "arguments": {"expr": "fiscal_year >= 2023", "facet_fields": ["period"], "facet_limit": 10}}
    assert tc.get("/stats").status_code == 200 and seen[-1] == {"name": "get_collection_stats", "arguments": {}}
    assert tc.post("/stats", json={"facet_limit": 0}).status_code == 422
    assert tc.get("/").json()["endpoints"] == {"health": "/health", "search": "/search", "answer": "/answer",
                                               "stats": "/stats"}
