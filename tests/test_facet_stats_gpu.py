"""Metric aggregations on the GPU: CorpusStore.facets(..., metrics=) and the query aggregates against the definition
(rag_fin_amd/facets.py: facets_reference(..., metrics=), stats_reference) -- device result == reference: NaN sums
compared as "is NaN", everything else by value, sums additionally by their bits.  There is no tolerance: the device
adds integers into a fixed-point accumulator and rounds once (include/ragfin.h, "metric aggregations").

Row counts 1, 33, 2 049 and 70 001, each under filters that pass nothing, everything, one row per block and only the
last row.  The metric columns cycle adversarial values: the DOUBLE ones the WEIGHTS of test_facets_gpu.py (NaN, both
infinities, 1e300, a subnormal) extended with a cancellation triple, 2^53, -0.0 and the largest double; a third
DOUBLE column only the finite ones below it, so that groups of every size also have a finite sum to round; the INT64
one the extremes of int64.  Buckets over CODES fields of 1, 6 and 65 values, an ARRAY field with empty rows and duplicates, a dynamic key
of mixed types."""
import math
import struct

import numpy as np
import pytest

from rag_fin_amd import _lib, facets
from rag_fin_amd.schema import DataType, FieldSchema
from test_facets_gpu import RATINGS, TAGS, WEIGHTS, make_store

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
DBL_MAX = 1.7976931348623157e308
DVALS = WEIGHTS + (1e16, 1.0, -1e16, 2.0 ** 53, -0.0, DBL_MAX)                  # 16 values
CLEAN = tuple(v for v in DVALS if abs(v) < DBL_MAX)                             # the 12 that keep every sum finite
IVALS = (2 ** 63 - 1, -2 ** 63, 2 ** 53 + 1, 0)
METRICS = ["primary_value", "weight", "clean", "big"]

FIELDS = [FieldSchema("c1", DataType.VARCHAR), FieldSchema("c6", DataType.VARCHAR), FieldSchema("c65", DataType.VARCHAR),
          FieldSchema("uniq", DataType.VARCHAR), FieldSchema("row", DataType.INT64), FieldSchema("pos", DataType.INT64),
          FieldSchema("year", DataType.INT64), FieldSchema("weight", DataType.DOUBLE), FieldSchema("clean", DataType.DOUBLE),
          FieldSchema("big", DataType.INT64),
          FieldSchema("tags", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=8)]
VALUE_FIELDS = ["c1", "c6", "c65", "year", "period", "tags", "rating"]


def table_of(n):
    ii = range(n)
    return {
        "id": [f"k{i}" for i in ii],
        "text": [("npa rose sharply" if i % 3 == 0 else "casa ratio fell") + f" in unit {i}" for i in ii],
        "period": [f"Q{i % 4 + 1}_FY{2020 + i % 3}" for i in ii],
        "chunk_type": [("table", "text", "note")[(i * i) % 3] for i in ii],
        "statement_type": ["consolidated" if i % 5 else "standalone" for i in ii],
        # (i // 32 in the index: the rows "one per block" passes do not all hold the same value)
        "primary_value": [DVALS[(i * 7 + i // 32) % len(DVALS)] for i in ii],
        "c1": ["only"] * n, "c6": [f"b{(i * i + i // 7) % 6}" for i in ii], "c65": [f"v{(i * 7919) % 65}" for i in ii],
        "uniq": [f"u{(i * 7919) % n}" for i in ii],
        "row": list(ii), "pos": [i % 32 for i in ii], "year": [2015 + (i * i) % 11 for i in ii],
        "weight": [DVALS[(i * 3 + 1 + i // 32) % len(DVALS)] for i in ii],
        "clean": [CLEAN[(i * 5 + i // 32) % len(CLEAN)] for i in ii],
        "big": [IVALS[(i + i // 32) % len(IVALS)] for i in ii],
        "tags": [[TAGS[(i + j * j) % len(TAGS)] for j in range(i % 6)] for i in ii],       # empty rows, duplicates
        "rating": [RATINGS[i % len(RATINGS)] for i in ii],
    }


def reference(st, fields, rows, **kw):
    return facets.facets_reference(st.columns, st.schema, st.dynamic if st.enable_dynamic_field else None, fields, rows, **kw)


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def assert_same(got, want, path="result"):
    """got == want, where a NaN equals a NaN and a float under "sum" also has the same bits."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), path
        for k in want:
            assert_same(got[k], want[k], f"{path}[{k!r}]")
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, f"{path}[{i}]")
    elif isinstance(want, float) and want != want:
        assert isinstance(got, float) and got != got, (path, got)
    else:
        assert got == want and isinstance(got, float) == isinstance(want, float), (path, got, want)
        if isinstance(want, float) and path.endswith("['sum']"):
            assert bits(got) == bits(want), (path, got, want)


_WORLDS = {}


def world(device, n):
    """One store per row count, and the reference of every filter, computed once."""
    if n not in _WORLDS:
        st = make_store(device, table_of(n), fields=FIELDS)
        filters = {"nothing": ("row < 0", []), "everything": ("row >= 0", list(range(n))),
                   "one per block": ("pos == 0", list(range(0, n, 32))), "last row": (f"row == {n - 1}", [n - 1])}
        refs = {name: reference(st, VALUE_FIELDS, rows, metrics=METRICS) for name, (_, rows) in filters.items()}
        _WORLDS[n] = (st, filters, refs)
    return _WORLDS[n]


# ---- row counts and filters --------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["nothing", "everything", "one per block", "last row"])
@pytest.mark.parametrize("n", [1, 33, 2049, 70001])
def test_metrics_equal_the_reference_under_every_filter(gpu_device, n, which):
    st, filters, refs = world(gpu_device, n)
    expr, rows = filters[which]
    got = st.facets(VALUE_FIELDS, expr=expr, metrics=METRICS)
    want = refs[which]
    assert got["count"] == len(rows)
    assert_same(got, want)
    # without metrics the answer is the one of before, and has no "metrics" anywhere
    plain = st.facets(VALUE_FIELDS, expr=expr)
    assert "metrics" not in repr(plain) and plain == reference(st, VALUE_FIELDS, rows)
    # what the device returned obeys the definition's identities
    for name in VALUE_FIELDS:
        for b in got["facets"][name]["buckets"]:
            for m in METRICS:
                s = b["metrics"][m]
                assert s["count"] + s["nan"] == b["count"], (name, b["value"], m)
    if rows:
        assert got["metrics"]["big"]["sum"] == sum(st.columns["big"][r] for r in rows)
        assert got["metrics"]["clean"]["sum"] == facets.stats_reference([st.columns["clean"][r] for r in rows], "f64")["sum"]


def test_the_sums_exercise_what_they_should(gpu_device):
    """The columns above do produce finite, infinite, NaN and beyond-64-bit sums."""
    st, filters, refs = world(gpu_device, 70001)
    top = refs["everything"]["metrics"]
    assert math.isnan(top["primary_value"]["sum"]) and top["primary_value"]["nan"] > 4000
    assert math.isfinite(top["clean"]["sum"]) and top["clean"]["sum"] != 0.0
    assert abs(top["big"]["sum"]) > 2 ** 64 and (top["big"]["min"], top["big"]["max"]) == (-2 ** 63, 2 ** 63 - 1)
    assert math.isfinite(refs["one per block"]["metrics"]["clean"]["sum"])
    assert refs["everything"]["metrics"]["clean"]["sum"] == math.fsum(st.columns["clean"])


# ---- limits: one bucket, a cut through a tie group, the global-atomic path ---------------------------------------
def test_limit_one_and_a_limit_inside_a_tie_group(gpu_device):
    st, filters, _ = world(gpu_device, 2049)
    for kw in (dict(limit=1), dict(limit=10), dict(limit=7, min_count=2)):
        # c65: 2 049 rows over 65 values, 31 or 32 each -- a limit of 10 or 7 cuts the group of the 32s
        got = st.facets(["c65", "c6", "uniq"], expr="row >= 5", metrics=["clean", "big"], **kw)
        assert_same(got, reference(st, ["c65", "c6", "uniq"], range(5, 2049), metrics=["clean", "big"], **kw))
    counts = [b["count"] for b in st.facets(["c65"], limit=10, metrics=["clean"])["facets"]["c65"]["buckets"]]
    # no metric: every "metrics" is there and empty
    assert_same(st.facets(["c6"], metrics=[]), reference(st, ["c6"], range(2049), metrics=[]))
    from collections import Counter
    assert counts == [32] * 10 and sum(1 for c in Counter(st.columns["c65"]).values() if c == 32) > 10


def test_limit_1000_with_four_metrics_takes_the_global_atomic_path(gpu_device):
    """1 000 slots x 4 metrics = 4 000 records of `uniq` (as many values as rows) exceed RF_STATS_LDS_RECORDS = 64, the
    records a workgroup keeps in LDS: the kernel adds straight into global memory.  c6 beside it (6 slots x 4 = 24
    records) stays in LDS in the same launch."""
    assert _lib.RF_STATS_LDS_RECORDS == 64 and 1000 * len(METRICS) > _lib.RF_STATS_LDS_RECORDS >= 6 * len(METRICS)
    st, filters, _ = world(gpu_device, 2049)
    for expr, rows in ((None, range(2049)), ("pos < 3", [r for r in range(2049) if r % 32 < 3])):
        got = st.facets(["uniq", "c6"], expr=expr, limit=1000, metrics=METRICS)
        assert_same(got, reference(st, ["uniq", "c6"], rows, limit=1000, metrics=METRICS))
    assert len(got["facets"]["uniq"]["buckets"]) == len(rows) == 193 and got["facets"]["uniq"]["buckets"][0]["metrics"]["big"]["count"] == 1
    # 17 slots x 4 metrics = 68 records: the first size past the LDS bound; 16 x 4 = 64: the last one inside it
    for limit in (16, 17):
        got = st.facets(["c65"], limit=limit, metrics=METRICS)
        assert_same(got, reference(st, ["c65"], range(2049), limit=limit, metrics=METRICS))


# ---- ARRAY fields and dynamic keys -------------------------------------------------------------------------------
def test_a_long_array_row_beside_short_ones(gpu_device):
    fields = [FieldSchema("tags", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=4096),
              FieldSchema("row", DataType.INT64), FieldSchema("weight", DataType.DOUBLE), FieldSchema("big", DataType.INT64)]
    n = 65
    t = {k: v for k, v in table_of(n).items() if k in ("id", "text", "period", "chunk_type", "statement_type", "primary_value",
                                                        "row", "weight", "big", "rating")}
    t["tags"] = [[TAGS[(i + j) % 5] for j in range(i % 4)] for i in range(n)]
    t["tags"][40] = [("x", "y", "npa")[(j + j // 7) % 3] for j in range(4096)]    # 4 096 elements over 3 values
    t["tags"][41] = []
    st = make_store(gpu_device, t, fields=fields, dynamic=())
    m = ["primary_value", "weight", "big"]
    for expr, rows in ((None, range(n)), ("row != 40", [r for r in range(n) if r != 40]), ("row == 40", [40]),
                       ("row >= 32", range(32, n)), ("row == 41", [41])):
        assert_same(st.facets(["tags"], expr=expr, metrics=m), reference(st, ["tags"], rows, metrics=m))
    got = st.facets(["tags"], expr="row == 40", metrics=["big"])["facets"]["tags"]["buckets"]
    # the row holds each of its three values more than a thousand times and is counted, and summed, once
    assert [(b["value"], b["count"], b["metrics"]["big"]["sum"]) for b in got] == [(v, 1, t["big"][40]) for v in ("npa", "x", "y")]


def test_a_dynamic_key_of_mixed_types(gpu_device):
    st, filters, refs = world(gpu_device, 2049)
    for name in ("rating", '$meta["rating"]', "absent_key"):
        got = st.facets([name], expr="pos < 9", metrics=["clean", "big"])
        assert_same(got, reference(st, [name], [r for r in range(2049) if r % 32 < 9], metrics=["clean", "big"]))
    values = [b["value"] for b in st.facets(["rating"], metrics=["clean"])["facets"]["rating"]["buckets"]]
    assert True in values and False in values and "AA" in values and 3 not in values


# ---- the one-slot group: query aggregates --------------------------------------------------------------------------
def test_query_aggregates(gpu_device):
    st, filters, _ = world(gpu_device, 2049)
    n = 2049
    if not st.has_index(field_name="sparse"):
        st.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
    out = ["sum(clean)", "avg(clean)", "min(clean)", "max(clean)", "count(*)", "sum(big)", "avg(big)", "min(big)", "max(big)",
           "sum(primary_value)", "min(primary_value)", "sum(weight)"]
    keys = ["k1", "absent", "k2048", "k77", "k1"]
    for expr, rows in (("", range(n)), (None, range(n)), ("TEXT_MATCH(text, 'npa')", range(0, n, 3)),
                       ("TEXT_MATCH(text, 'npa') and row < 0", []), (f"id in {keys!r}".replace("'", '"'), [1, 77, 2048]),
                       ("year >= 2020 and pos == 5", [r for r in range(n) if st.columns["year"][r] >= 2020 and r % 32 == 5])):
        got = st.query(expr, output_fields=out)
        want = {}
        for f in out:
            if f == "count(*)":
                want[f] = len(rows)
            else:
                fn, col = facets.parse_aggregate(f)
                want[f] = facets.stats_reference([st.columns[col][r] for r in rows], "i64" if col == "big" else "f64")[fn]
        assert len(got) == 1 and list(got[0]) == out
        for f in out:
            assert_same(got[0][f], want[f], f"{expr!r}['sum']" if f.startswith("sum(") else f"{expr!r}[{f!r}]")
    with pytest.raises(ValueError, match="limit"):
        st.query("", limit=3, output_fields=["sum(clean)"])
    with pytest.raises(ValueError, match="other output_fields"):
        st.query("", output_fields=["count(*)", "id"])


# ---- the same bits on every run, whatever the grid ------------------------------------------------------------------
def test_the_same_bits_twice_on_other_grids_and_under_filters_built_differently(gpu_device):
    import torch
    from rag_fin_amd.index import facet_counts, facet_stats_all
    st, filters, refs = world(gpu_device, 70001)
    n = 70001
    first = st.facets(VALUE_FIELDS, expr="pos == 0", metrics=METRICS)
    assert_same(first, refs["one per block"])
    assert repr(st.facets(VALUE_FIELDS, expr="pos == 0", metrics=METRICS)) == repr(first)
    # the same passing rows from three different filters, and from none
    every = [st.facets(["c6", "tags"], expr=e, metrics=METRICS) for e in (None, "row >= 0", "pos >= 0 or year < 0", "pos < 32")]
    assert all(repr(e) == repr(every[0]) for e in every[1:])
    # the wrapper exposes the grid: 1, 3 and 512 workgroups against the default, for the one-slot group ...
    cols = [(torch.tensor(st.columns["clean"], dtype=torch.float64, device=gpu_device), True),
            (torch.tensor(st.columns["primary_value"], dtype=torch.float64, device=gpu_device), True),
            (torch.tensor(st.columns["big"], dtype=torch.int64, device=gpu_device), False)]
    filt = st.build_filter("pos < 7")
    base = facet_stats_all(gpu_device, filt, cols, n)
    assert base.shape == (3, _lib.RF_STATS_OUT)
    for grid in (1, 3, 512):
        assert np.array_equal(facet_stats_all(gpu_device, filt, cols, n, grid=grid), base), grid
    want = facets.stats_reference([v for r, v in enumerate(st.columns["clean"]) if r % 32 < 7], "f64")
    assert int(base[0, 0]) == want["count"] and int(base[0, 2]) == struct.unpack("<q", struct.pack("<d", want["sum"]))[0]
    # ... and for buckets, in LDS (limit 6) and in global memory (limit 1000), over a coded column built here
    codes = (torch.arange(n, dtype=torch.int64, device=gpu_device) * 7919 % 4000).to(torch.int32)
    spec = {"kind": _lib.RF_FACET_CODES, "n_codes": 4000, "a": codes, "rank": torch.arange(4000, dtype=torch.int32, device=gpu_device)}
    for limit in (6, 1000):
        sel0, stats0 = facet_counts(gpu_device, filt, [spec], n, limit, 1, metrics=cols)
        for grid in (1, 3, 512):
            sel, stats = facet_counts(gpu_device, filt, [spec], n, limit, 1, metrics=cols, grid=grid)
            assert np.array_equal(sel, sel0) and np.array_equal(stats, stats0), (limit, grid)
        assert stats0.shape == ((limit + 1) * 3, _lib.RF_STATS_OUT)
        assert np.array_equal(stats0[-3:], base)   # the all-rows group behind the field's slots
