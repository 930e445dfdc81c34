"""Metric aggregations on the CPU: stats_reference (the definition the device is tested against,
rag_fin_amd/facets.py) against math.fsum and hand-written expectations, facets_reference(..., metrics=...), the
argument checks, facets(metrics=) and the query aggregates on a store over the CPU double of GpuIndex, and the tool
and REST plumbing.  GROUPS below is shared with tests/test_exact_sum_native.py, which runs the device's arithmetic
(csrc/exact_sum.h) on the host; the device side is covered by tests/test_facet_stats_gpu.py."""
import math
import random
import struct

import numpy as np
import pytest

from rag_fin_amd import _lib, facets, filter_expr, mcp_server
from rag_fin_amd.schema import DataType, FieldSchema
from rag_fin_amd.store import CorpusStore
from test_extra_fields_cpu import CpuIndex, rows

NAN, INF = float("nan"), float("inf")
DBL_MAX = 1.7976931348623157e308
FIELDS = [FieldSchema("bank", DataType.VARCHAR, default="ICICI"), FieldSchema("fiscal_year", DataType.INT64, default=2024),
          FieldSchema("audited", DataType.BOOL, default=False), FieldSchema("weight", DataType.DOUBLE, default=1.0),
          FieldSchema("tags", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=8, default=[])]


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def random_groups(n_groups=200, seed=1):
    rng = random.Random(seed)
    return [[rng.choice([-1, 1]) * math.ldexp(rng.random(), rng.randint(-1074, 1023)) for _ in range(rng.randint(0, 40))]
            for _ in range(n_groups)]


# name -> group of doubles; every one is compared with stats_reference by the native test too
GROUPS = {
    "cancellation": [1e16, 1.0, -1e16],
    "half-even tie, even below": [2.0 ** 53, 1.0],
    "half-even tie, odd below": [2.0 ** 53 + 2, 1.0],
    "subnormals": [5e-324 * k for k in range(1, 40)],
    "subnormals cancel": [5e-324, -5e-324],
    "smallest normal less one": [2.2250738585072014e-308, -5e-324],
    "intermediate overflow": [1e308, 1e308, -1e308],
    "overflow": [DBL_MAX, DBL_MAX],
    "negative overflow": [-DBL_MAX, -DBL_MAX, 1.0],
    "max plus half an ulp rounds to even: inf": [DBL_MAX, 2.0 ** 970],
    "max plus less than half an ulp": [DBL_MAX, 2.0 ** 969],
    "+inf": [INF, 1.0, -1e308], "-inf": [-INF, 1e308], "both infinities": [INF, -INF, 1.0],
    "nan": [NAN, 1.0, NAN], "only nan": [NAN], "nan and inf": [NAN, INF],
    "all -0.0": [-0.0, -0.0, -0.0], "zeros": [0.0, -0.0], "empty": [],
    "one": [0.1], "thirds": [0.1] * 10,
}


# ---- stats_reference ------------------------------------------------------------------------------------
def test_the_sum_equals_fsum_on_random_groups_across_the_range():
    for g in random_groups():
        want = math.fsum(g)
        got = facets.stats_reference(g, "f64")
        assert bits(got["sum"]) == bits(want + 0.0), g   # (fsum may return -0.0 for an exact zero; the definition +0.0)
        assert got["count"] == len(g) and got["nan"] == 0
        assert got["avg"] == (None if not g else got["sum"] / len(g))
        assert (got["min"], got["max"]) == ((min(g), max(g)) if g else (None, None))


def test_the_sum_is_the_rational_sum_rounded_once():
    """stats_reference adds integers over the denominator 2^1074; the definition is float(sum(Fraction(v)))."""
    from fractions import Fraction
    for g in list(GROUPS.values()) + random_groups(60, seed=3):
        finite = [v for v in g if v == v and abs(v) != INF]
        if len(finite) != len(g):
            continue
        try:
            want = float(sum((Fraction(v) for v in g), Fraction(0)))
        except OverflowError:
            want = INF if sum(Fraction(v) for v in g) > 0 else -INF
        assert bits(facets.stats_reference(g, "f64")["sum"]) == bits(want + 0.0), g


def test_the_sum_equals_fsum_wherever_fsum_returns():
    for name, g in GROUPS.items():
        finite = [v for v in g if v == v and abs(v) != INF]
        if len(finite) != len(g):
            continue
        try:
            want = math.fsum(g)
        except OverflowError:
            continue
        assert bits(facets.stats_reference(g, "f64")["sum"]) == bits(want + 0.0), name


def test_the_adversarial_groups():
    s = lambda g: facets.stats_reference(g, "f64")["sum"]   # noqa: E731
    assert s(GROUPS["cancellation"]) == 1.0
    assert s([2.0 ** 53, 1.0]) == 2.0 ** 53 and s([2.0 ** 53 + 2, 1.0]) == 2.0 ** 53 + 4   # ties to even, both ways
    assert s([5e-324 * k for k in range(1, 40)]) == 5e-324 * (39 * 40 // 2)
    assert s([1e308, 1e308, -1e308]) == 1e308                    # math.fsum raises on this one
    with pytest.raises(OverflowError):
        math.fsum([1e308, 1e308, -1e308])
    assert s([DBL_MAX, DBL_MAX]) == INF and s([-DBL_MAX, -DBL_MAX, 1.0]) == -INF
    assert s([DBL_MAX, 2.0 ** 970]) == INF and s([DBL_MAX, 2.0 ** 969]) == DBL_MAX
    assert s([INF, 1.0, -1e308]) == INF and s([-INF, 1e308]) == -INF and math.isnan(s([INF, -INF, 1.0]))
    assert bits(s([-0.0, -0.0, -0.0])) == 0 and bits(s([0.0, -0.0])) == 0 and bits(s([5e-324, -5e-324])) == 0
    got = facets.stats_reference([NAN, 1.0, NAN], "f64")
    assert got == {"count": 1, "nan": 2, "sum": 1.0, "avg": 1.0, "min": 1.0, "max": 1.0}
    assert facets.stats_reference([NAN], "f64") == {"count": 0, "nan": 1, "sum": 0.0, "avg": None, "min": None, "max": None}
    got = facets.stats_reference([NAN, INF], "f64")
    assert (got["count"], got["nan"], got["sum"], got["avg"], got["min"], got["max"]) == (1, 1, INF, INF, INF, INF)
    assert facets.stats_reference([], "f64") == {"count": 0, "nan": 0, "sum": 0.0, "avg": None, "min": None, "max": None}
    assert bits(facets.stats_reference([], "f64")["sum"]) == 0
    got = facets.stats_reference([1e308, 1e308, -1e308], "f64")
    assert got["avg"] == 1e308 / 3 and (got["min"], got["max"]) == (-1e308, 1e308)


def test_int64_sums_are_exact_python_ints():
    g = [2 ** 63 - 1] * 5 + [2 ** 53 + 1]
    got = facets.stats_reference(g, "i64")
    assert got == {"count": 6, "nan": 0, "sum": 5 * (2 ** 63 - 1) + 2 ** 53 + 1, "avg": sum(g) / 6, "min": 2 ** 53 + 1,
                   "max": 2 ** 63 - 1}
    assert got["sum"] > 2 ** 64 and isinstance(got["sum"], int)
    got = facets.stats_reference([-2 ** 63] * 3 + [np.int64(0)], "i64")
    assert (got["sum"], got["min"], got["max"]) == (-3 * 2 ** 63, -2 ** 63, 0) and got["sum"] < -2 ** 64
    assert facets.stats_reference([], "i64") == {"count": 0, "nan": 0, "sum": 0, "avg": None, "min": None, "max": None}
    assert isinstance(facets.stats_reference([], "i64")["sum"], int)


# ---- facets_reference --------------------------------------------------------------------------------------
COLS = {"bank": ["a", "b", "a", "c", "a", "b"], "fiscal_year": [2020, 2021, 2 ** 62, 2 ** 62, 2 ** 62, -5],
        "weight": [1e16, NAN, 1.0, 5.0, -1e16, INF], "primary_value": [0.1, 0.2, 0.3, 0.4, 0.5, 0.6],
        "period": ["Q1", "Q1", "Q2", "Q2", "Q1", "Q2"],
        "tags": [["x", "x", "y"], [], ["y"], ["x"], [], ["z", "z"]]}


def ref(fields, rows_, dynamic=None, **kw):
    return facets.facets_reference(COLS, FIELDS, dynamic, fields, rows_, **kw)


def test_without_metrics_the_output_is_unchanged():
    got = ref(["bank", "tags"], range(6), ranges={"weight": [(0, None)]})
    assert set(got) == {"count", "facets", "ranges"}
    assert got["facets"]["bank"] == {"buckets": [{"value": "a", "count": 3}, {"value": "b", "count": 2}, {"value": "c", "count": 1}],
                                     "distinct": 3, "missing": 0, "other": 0}
    assert "metrics" not in repr(got)
    assert got == ref(["bank", "tags"], range(6), ranges={"weight": [(0, None)]}, metrics=None)


def test_buckets_carry_the_metrics_of_their_units():
    got = ref(["bank", "period", "fiscal_year", "tags"], range(6), metrics=["weight", "fiscal_year", "primary_value"])
    a, b, c = got["facets"]["bank"]["buckets"]
    assert (a["value"], a["count"]) == ("a", 3)
    assert a["metrics"]["weight"] == {"count": 3, "nan": 0, "sum": 1.0, "avg": 1.0 / 3, "min": -1e16, "max": 1e16}
    assert a["metrics"]["fiscal_year"] == {"count": 3, "nan": 0, "sum": 2020 + 2 ** 63, "avg": (2020 + 2 ** 63) / 3,
                                           "min": 2020, "max": 2 ** 62}
    assert b["metrics"]["weight"] == {"count": 1, "nan": 1, "sum": INF, "avg": INF, "min": INF, "max": INF}
    assert c["metrics"]["weight"]["sum"] == 5.0 and c["metrics"]["primary_value"]["sum"] == 0.4
    assert a["metrics"]["primary_value"]["sum"] == math.fsum([0.1, 0.3, 0.5])
    assert list(a["metrics"]) == ["weight", "fiscal_year", "primary_value"]
    # an INT64 value field: a declared field as buckets
    y = {bk["value"]: bk["metrics"]["primary_value"]["sum"] for bk in got["facets"]["fiscal_year"]["buckets"]}
    assert y[2 ** 62] == math.fsum([0.3, 0.4, 0.5]) and y[-5] == 0.6
    # an ARRAY row belongs once to each distinct element's bucket: row 0 holds x twice and counts once
    t = {bk["value"]: bk for bk in got["facets"]["tags"]["buckets"]}
    assert t["x"]["count"] == 2 and t["x"]["metrics"]["primary_value"]["sum"] == math.fsum([0.1, 0.4])
    assert t["y"]["metrics"]["primary_value"]["sum"] == math.fsum([0.1, 0.3]) and t["z"]["metrics"]["primary_value"]["count"] == 1
    assert "metrics" not in got["facets"]["tags"] and got["facets"]["tags"]["missing"] == 2
    # the top level: all passing rows
    assert got["metrics"]["weight"] == {"count": 5, "nan": 1, "sum": INF, "avg": INF, "min": -1e16, "max": INF}
    assert got["metrics"]["primary_value"]["sum"] == math.fsum(COLS["primary_value"])
    # a filter, a limit: the buckets that are cut carry nothing, ranges are as before
    got = ref(["bank"], [0, 2, 3], limit=1, metrics=["weight"], ranges={"weight": [(None, 2)]})
    assert got["facets"]["bank"] == {"buckets": [{"value": "a", "count": 2, "metrics": {"weight": facets.stats_reference([1e16, 1.0], "f64")}}],
                                     "distinct": 2, "missing": 0, "other": 1}
    assert got["metrics"]["weight"]["sum"] == 1e16 + 6 and got["ranges"] == ref([], [0, 2, 3], ranges={"weight": [(None, 2)]})["ranges"]
    # nothing passes
    got = ref(["bank"], [], metrics=["weight", "fiscal_year"])
    assert got["facets"]["bank"]["buckets"] == [] and got["metrics"]["fiscal_year"] == facets.stats_reference([], "i64")
    # metrics alone are something to count
    assert ref([], range(6), metrics=["weight"]) == {"count": 6, "facets": {}, "ranges": {}, "metrics": got_all_weight()}


def got_all_weight():
    return {"weight": facets.stats_reference(COLS["weight"], "f64")}


def test_a_dynamic_key_as_buckets():
    dyn = {"rating": ["AA", True, 3, None, "AA", True]}
    got = ref(["rating"], range(6), dynamic=dyn, metrics=["primary_value"])
    by = {(type(b["value"]), b["value"]): b["metrics"]["primary_value"] for b in got["facets"]["rating"]["buckets"]}
    assert by[(str, "AA")]["sum"] == math.fsum([0.1, 0.5]) and by[(bool, True)]["sum"] == math.fsum([0.2, 0.6])
    assert got["facets"]["rating"]["missing"] == 2 and got["metrics"]["primary_value"]["count"] == 6


@pytest.mark.parametrize("metrics, match", [
    ("weight", "metrics must be a list"), ([3], "non-empty string"), (["weight", "weight"], "twice"),
    (["nope"], "no numeric field"), (["bank"], "no numeric field"), (["tags"], "no numeric field"), (["audited"], "no numeric field"),
    (["weight", "fiscal_year", "primary_value", "a", "b"], "at most 4 metrics")])
def test_check_args_refuses_bad_metrics(metrics, match):
    with pytest.raises(ValueError, match=match):
        facets.check_args(["bank"], metrics=metrics, schema=FIELDS)
    with pytest.raises(ValueError, match=match):
        ref(["bank"], range(6), metrics=metrics)


def test_check_args_stays_backwards_compatible():
    assert facets.check_args(["bank"], 5, 2, {"weight": [(0, 1)]}) == (["bank"], 5, 2, {"weight": [(0, 1)]})
    assert facets.check_args(["bank"], metrics=["weight", "fiscal_year"], schema=FIELDS) == \
        (["bank"], 10, 1, {}, [("weight", "f64"), ("fiscal_year", "i64")])
    assert facets.check_args([], metrics=["primary_value"])[4] == [("primary_value", "f64")]
    with pytest.raises(ValueError, match="nothing to count"):
        facets.check_args([], metrics=[])
    assert facets.MAX_METRICS == _lib.RF_STATS_MAX_METRICS == 4
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ragfin.h")).read()
    for name in ("RF_STATS_MAX_METRICS", "RF_STATS_WORDS", "RF_STATS_OUT", "RF_STATS_LDS_RECORDS"):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(_lib, name), name


def test_the_library_checks_its_arguments_without_a_gpu():
    """Every refusal comes before any device call."""
    import ctypes
    lib = _lib.load_library()
    f = (_lib.FacetField * 2)()
    f[0].kind, f[0].n_codes, f[0].a_dev, f[0].counter_off = _lib.RF_FACET_CODES, 4, 64, 0
    f[1].kind, f[1].n_codes, f[1].a_dev, f[1].b_dev, f[1].counter_off = _lib.RF_FACET_DYNAMIC, 2000, 64, 64, 5
    m = (_lib.StatsMetric * 4)()
    m[0].column_dev, m[0].is_f64 = 64, 1
    buf = ctypes.c_void_p(4096)
    # the record layout: min(limit, bins) slots per field and one for all rows, each of n_metrics records
    assert lib.rf_facet_stats_records(f, 2, 3, 10) == (4 + 10 + 1) * 3
    assert lib.rf_facet_stats_records(f, 2, 1, 1000) == 4 + 1000 + 1 and lib.rf_facet_stats_records(None, 0, 4, 1) == 4
    assert lib.rf_facet_stats_records(f, 2, 0, 10) == -1 and lib.rf_facet_stats_records(f, 2, 5, 10) == -1
    assert lib.rf_facet_stats_records(f, 17, 1, 10) == -1 and lib.rf_facet_stats_records(f, 1, 1, 1001) == -1
    ok = dict(n_counters=5 + 2003, limit=10, n_rows=100)
    call = lambda filt=None, fields=f, nf=1, metrics=m, nm=1, slot=buf, acc=buf, n_records=5, grid=0, **kw: lib.rf_facet_stats(   # noqa: E731
        filt, fields, nf, metrics, nm, slot, kw.get("n_counters", ok["n_counters"]), kw.get("limit", ok["limit"]),
        kw.get("n_rows", ok["n_rows"]), acc, n_records, grid, None)
    assert call(acc=None) == -1 and call(acc=ctypes.c_void_p(4100)) == -1
    assert call(n_rows=2 ** 31) == -1 and b"2^31" in lib.rf_last_error()      # the bound of the limbs
    assert call(n_rows=-1) == -1 and call(filt=ctypes.c_void_p(8)) == -1
    assert call(nm=0) == -1 and call(nm=5) == -1 and call(metrics=None) == -1
    assert call(nm=2) == -1                                                    # metric 1 has no column
    assert call(slot=None) == -1 and call(limit=0) == -1 and call(limit=1001) == -1 and call(grid=-1) == -1
    assert call(n_records=4) == -1 and b"rf_facet_stats_records" in lib.rf_last_error()
    assert call(nf=17) == -1 and call(n_counters=4) == -1
    assert lib.rf_facet_stats_slots(f, 1, None, 10, buf, 5, None) == -1
    assert lib.rf_facet_stats_slots(f, 1, buf, 10, None, 5, None) == -1
    assert lib.rf_facet_stats_slots(f, 1, buf, 0, buf, 5, None) == -1
    assert lib.rf_facet_stats_slots(f, 0, buf, 10, buf, 5, None) == -1
    assert lib.rf_facet_stats_slots(f, 1, buf, 10, buf, 4, None) == -1
    assert lib.rf_facet_stats_finish(None, m, 1, 5, buf, None) == -1
    assert lib.rf_facet_stats_finish(buf, m, 1, 5, None, None) == -1
    assert lib.rf_facet_stats_finish(buf, m, 0, 5, buf, None) == -1
    assert lib.rf_facet_stats_finish(buf, m, 2, 5, buf, None) == -1            # no multiple of the metrics
    assert lib.rf_facet_stats_finish(buf, m, 1, 0, buf, None) == -1
    assert b"rf_facet_stats_finish" in lib.rf_last_error()


# ---- the surface, on a store over the CPU double ----------------------------------------------------------------
class HostStore(CorpusStore):
    def __init__(self, fields=None, enable_dynamic_field=False):
        super().__init__("t", dim=32, capacity=16, index=CpuIndex(32, 16), fields=fields,
                         enable_dynamic_field=enable_dynamic_field)

    def _grow(self, need):
        self.index.capacity = max(need, 2 * self.index.capacity)

    def _match_mask(self, expr):
        node = filter_expr.parse(expr, schema=self.schema)
        return np.array([node.eval({f: c[r] for f, c in self.columns.items()}) for r in range(self.num_entities)], dtype=bool)

    def _expr_rows(self, expr):
        return np.flatnonzero(self._match_mask(expr))


def host_store():
    st = HostStore(fields=FIELDS)
    d = rows(["k0", "k1", "k2", "k3", "k4", "k5"])
    d[6] = COLS["primary_value"]
    st.add(d[0], d[1], d[2], *d[3:], extra={k: COLS[k] for k in ("bank", "fiscal_year", "weight", "tags")})
    return st


def test_facets_with_metrics_on_a_host_store_goes_through_the_reference():
    st = host_store()
    want = facets.facets_reference(st.columns, st.schema, None, ["bank", "tags"], range(6), metrics=["weight", "fiscal_year"])
    got = st.facets(["bank", "tags"], metrics=["weight", "fiscal_year"])
    assert repr(got) == repr(want) and got["facets"]["bank"]["buckets"][0]["metrics"]["weight"]["sum"] == 1.0
    got = st.facets(["bank"], expr="fiscal_year >= 2021", metrics=["primary_value"], limit=1)
    assert got == facets.facets_reference(st.columns, st.schema, None, ["bank"], [1, 2, 3, 4], limit=1, metrics=["primary_value"])
    assert got["count"] == 4 and got["metrics"]["primary_value"]["sum"] == math.fsum([0.2, 0.3, 0.4, 0.5])
    assert st.facets([], metrics=["primary_value"])["metrics"]["primary_value"]["count"] == 6
    for kw, match in ((dict(metrics=["bank"]), "no numeric field"), (dict(metrics=["weight"] * 2), "twice"),
                      (dict(metrics="weight"), "must be a list"), (dict(metrics=["w1", "w2", "w3", "w4", "w5"]), "at most 4")):
        with pytest.raises(ValueError, match=match):
            st.facets(["bank"], **kw)
    # an empty store
    empty = HostStore(fields=FIELDS)
    assert empty.facets(["bank"], metrics=["weight", "fiscal_year"]) == {
        "count": 0, "facets": {"bank": {"buckets": [], "distinct": 0, "missing": 0, "other": 0}}, "ranges": {},
        "metrics": {"weight": {"count": 0, "nan": 0, "sum": 0.0, "avg": None, "min": None, "max": None},
                    "fiscal_year": {"count": 0, "nan": 0, "sum": 0, "avg": None, "min": None, "max": None}}}


def test_query_aggregates_on_a_host_store():
    st = host_store()
    got = st.query("", output_fields=["sum(primary_value)", "avg(primary_value)", "min(weight)", "max(weight)", "count(*)",
                                      "sum(fiscal_year)"])
    pv = facets.stats_reference(COLS["primary_value"], "f64")
    assert got == [{"sum(primary_value)": pv["sum"], "avg(primary_value)": pv["avg"], "min(weight)": -1e16, "max(weight)": INF,
                    "count(*)": 6, "sum(fiscal_year)": sum(COLS["fiscal_year"])}]
    assert list(got[0]) == ["sum(primary_value)", "avg(primary_value)", "min(weight)", "max(weight)", "count(*)", "sum(fiscal_year)"]
    assert st.query("fiscal_year >= 2021", output_fields=["sum( primary_value )"]) == \
        [{"sum( primary_value )": math.fsum([0.2, 0.3, 0.4, 0.5])}]
    assert st.query('id in ["k1", "zz", "k3", "k1"]', output_fields=["sum(primary_value)", "count(*)"]) == \
        [{"sum(primary_value)": math.fsum([0.2, 0.4]), "count(*)": 2}]
    assert st.query("fiscal_year < -100", output_fields=["sum(weight)", "min(weight)", "avg(fiscal_year)"]) == \
        [{"sum(weight)": 0.0, "min(weight)": None, "avg(fiscal_year)": None}]
    assert math.isnan(st.query(None, output_fields=("sum(weight)",))[0]["sum(weight)"]) is False   # one infinity: +inf
    assert st.query(None, output_fields=("sum(weight)",)) == [{"sum(weight)": INF}]
    empty = HostStore(fields=FIELDS)
    assert empty.query("", output_fields=["sum(weight)", "count(*)"]) == [{"sum(weight)": 0.0, "count(*)": 0}]
    # the refusals of count(*), for every aggregate
    for kw, match in ((dict(output_fields=["sum(weight)", "id"]), "an aggregate cannot be combined with other output_fields"),
                      (dict(output_fields=["count(*)", "id"]), "count\\(\\*\\) cannot be combined with other output_fields"),
                      (dict(output_fields=["count(*)", "sum(weight)", "text"]), "cannot be combined with other output_fields"),
                      (dict(output_fields=["max(weight)"], limit=1), "an aggregate cannot be combined with limit"),
                      (dict(output_fields=["avg(weight)"], offset=1), "an aggregate cannot be combined with offset"),
                      (dict(output_fields=["sum(bank)"]), "no numeric field"), (dict(output_fields=["sum(nope)"]), "no numeric field")):
        with pytest.raises(ValueError, match=match):
            st.query("", **kw)
    with pytest.raises(KeyError):
        st.query("", output_fields=["median(weight)"])   # no aggregate: an unknown field, as before
    assert [r["id"] for r in st.query("", limit=2)] == ["k0", "k1"]


def test_the_sharded_store_keeps_its_refusal():
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    with pytest.raises(NotImplementedError, match="faceted counts are not implemented for the sharded store"):
        ShardedCorpusStore.facets(object(), ["period"], metrics=["primary_value"])
    with pytest.raises(NotImplementedError, match="metric aggregations are not implemented for the sharded store"):
        ShardedCorpusStore._aggregate(object(), "", [("primary_value", "f64")])


# ---- the tool, VectorRAG and the REST body ------------------------------------------------------------------------
class FakeRag:
    def __init__(self):
        self.calls = []

        class Collection:
            num_entities = 5
        self.collection = Collection()

    def facets(self, fields=None, expr=None, limit=10, min_count=1, ranges=None, metrics=None):
        self.calls.append((tuple(fields), expr, limit, metrics))
        return {"count": 3, "facets": {f: {"buckets": []} for f in fields}, "ranges": {},
                "metrics": {m: {"count": 3, "sum": 1.5} for m in metrics}}


def test_the_tool_and_vector_rag_hand_metric_fields_on():
    rag = FakeRag()
    mcp_server.set_rag(rag)
    try:
        got = mcp_server.get_collection_stats(expr="fiscal_year >= 2023", facet_fields=["bank"], facet_limit=4,
                                              metric_fields=["primary_value", "fiscal_year"])
        assert rag.calls == [(("bank",), "fiscal_year >= 2023", 4, ["primary_value", "fiscal_year"])]
        assert got["status"] == "success" and got["count"] == 3 and set(got["metrics"]) == {"primary_value", "fiscal_year"}
        got = mcp_server.get_collection_stats(metric_fields=["primary_value"])
        assert rag.calls[-1] == ((), None, 10, ["primary_value"]) and got["facets"] == {} and got["metrics"]["primary_value"]["sum"] == 1.5
    finally:
        mcp_server.set_rag(None)
    from rag_fin_amd.rag import VectorRAG
    seen = {}

    class Store:
        num_entities = 0

        def load(self):
            pass

        def facets(self, fields, **kw):
            seen.update(fields=fields, **kw)
            return {"count": 0}
    rag = VectorRAG("k", "c", embedder=object(), store=Store())
    rag.facets(["period"], expr="x > 1", metrics=["primary_value"])
    assert seen == dict(fields=["period"], expr="x > 1", limit=10, min_count=1, ranges=None, metrics=["primary_value"])
    seen.clear()
    rag.facets(["period"])
    assert "metrics" not in seen


def test_the_rest_body_carries_metric_fields():
    from pydantic import ValidationError
    from rag_fin_amd import adapter
    assert adapter.stats_args(adapter.StatsRequest(facet_fields=["period"], metric_fields=["primary_value"])) == \
        {"facet_fields": ["period"], "facet_limit": 10, "metric_fields": ["primary_value"]}
    assert adapter.stats_args(adapter.StatsRequest(expr="a > 1", metric_fields=["w", "x", "y", "z"])) == \
        {"expr": "a > 1", "metric_fields": ["w", "x", "y", "z"]}
    assert "metric_fields" not in adapter.stats_args(adapter.StatsRequest(expr="a > 1"))
    with pytest.raises(ValidationError):
        adapter.StatsRequest(metric_fields=["f"] * 5)
