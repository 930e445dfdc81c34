"""Faceted counts: the definition, in pure Python (no GPU).

`CorpusStore.facets(fields, expr, limit, min_count, ranges)` answers "how many of the rows `expr` passes hold
each value of a field" and "how many fall into each range of a numeric field".  This module holds what every
layer shares and is tested against: the argument checks, which fields can be faceted, the order of the
buckets, and `facets_reference`, the whole answer over the host columns with collections.Counter.  The
device side (include/ragfin.h, "faceted counts") must equal it exactly: counts are integers
and the result does not depend on any order, so there is no tolerance anywhere.

Value facets.  For a field the facet is
    {"buckets": [{"value": v, "count": c}, ...], "distinct": d, "missing": m, "other": o}
  buckets   the `limit` (1..MAX_LIMIT, default 10) values with the highest count among the passing rows, ordered
            by (count descending, value ascending); only counts >= min_count (>= 1, default 1)
  distinct  the values with count >= 1 among the passing rows (a value that lives on in a dictionary after a
            delete but occurs in no passing row is never reported)
  missing   passing rows that contribute nothing: 0 for a declared scalar field; the rows with an empty list
            for an ARRAY field; the rows that lack a dynamic key or hold a number or None under it
  other     counted units that are in no bucket: sum(bucket counts) + other + missing == units, where units is
            the passing rows for a scalar field and missing + the (row, distinct value) pairs for an ARRAY
            field -- a row counts ONCE per distinct element it holds: ["npa", "npa", "casa"] adds 1 to "npa"
Values order by (class, value): bools (False < True) before ints (numerically) before strings (by code point).
Only a dynamic key can mix classes; its strings and bools are counted.

Fields that can be value-faceted: period, chunk_type, statement_type; the collection's own VARCHAR, BOOL and
INT64 fields; its ARRAY fields of VARCHAR or BOOL elements; with enable_dynamic_field a dynamic key, bare or
as $meta["key"].  Anything else raises ValueError.

Range facets.  ranges = {field: [(lo, hi), ...]} over primary_value and the collection's own INT64 / DOUBLE
fields: 1..MAX_RANGES ranges per field, each [lo, hi) with None for no bound; they may overlap and each is
counted on its own.  The result is
    {"ranges": [{"from": lo, "to": hi, "count": c}, ...], "min": x, "max": y, "nan": n}
min / max over the passing non-NaN values (None when there is none).  DOUBLE compares as IEEE doubles: a NaN
falls in no range and is counted in "nan".  INT64 compares as integers, never through a double (a bound of any
size, or a float, is compared mathematically).

Metric aggregations.  metrics = [field, ...] (at most MAX_METRICS of primary_value and the collection's own INT64 /
DOUBLE fields: the fields a range facet takes) adds "metrics": {field: stats} to every bucket of every value facet,
over the bucket's units (a unit is a passing row that holds the value: an ARRAY row belongs once to each distinct
element's bucket, exactly as it is counted), and a top-level "metrics": {field: stats} over all passing rows;
`missing` and `other` get none.  stats (stats_reference) is {"count", "nan", "sum", "avg", "min", "max"}:
  DOUBLE  nan: the NaN values, which take part in nothing else; count: the others; sum: NaN when +inf and -inf
          both occur, that infinity when one does, else the EXACT rational sum of the finite values rounded once
          to the nearest double, ties to even (float(sum(Fraction(v)))): +-inf when that exceeds the double range,
          +0.0 when it is exactly zero.  It equals math.fsum wherever math.fsum returns.  The exact sum does not
          depend on an order, so the device (integer adds into a fixed-point accumulator, one rounding at the end)
          must give the same bits.  avg: sum / count, one IEEE division (None without a value); min / max over the
          non-NaN values (None without one; which zero a -0.0 / +0.0 tie returns is unspecified)
  INT64   sum: the exact Python int (it may exceed 64 bits); nan 0; avg: Python's sum / count; min / max ints
An empty group: count 0, sum 0.0 (INT64: 0), avg / min / max None.  Without `metrics` no "metrics" key appears.
"""
from __future__ import annotations

import math
import numbers
import re
from collections import Counter
from fractions import Fraction

import numpy as np

from . import filter_expr
from .schema import INT64_MAX, INT64_MIN, DataType

COUNT_STAR = "count(*)"      # query(expr, output_fields=["count(*)"]): pymilvus' idiom
MAX_LIMIT = 1000             # buckets per field (RF_FACET_MAX_LIMIT)
MAX_RANGES = 64              # ranges per field (RF_FACET_MAX_RANGES)
MAX_FIELDS = 16              # value fields of one call (RF_FACET_MAX_FIELDS)
MAX_METRICS = 4              # metric fields of one call (RF_STATS_MAX_METRICS)

_TWO_1074 = 2 ** 1074        # every finite double is an integer over it
_AGGREGATE = re.compile(r"^(sum|avg|min|max)\(\s*([^()\s]+)\s*\)$")
_META_KEY = re.compile(r"""^\$meta\[\s*(?:"([^"]+)"|'([^']+)')\s*\]$""")
_NOT_FACETABLE = ("id", "text", "embedding", "primary_value")


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_metrics(metrics, schema=()):
    """metrics= of facets() -> [(field, "f64" | "i64"), ...] (resolve_range_field says which fields are numeric), or
    ValueError: no list, more than MAX_METRICS names, a duplicate, an unknown or a non-numeric field."""
    if metrics is None:
        return []
    if isinstance(metrics, str) or not isinstance(metrics, (list, tuple)):
        raise ValueError(f"facets: metrics must be a list of field names, got {metrics!r}")
    metrics = list(metrics)
    for f in metrics:
        if not isinstance(f, str) or not f:
            raise ValueError(f"facets: metrics: a field name must be a non-empty string, got {f!r}")
    if len(set(metrics)) != len(metrics):
        raise ValueError("facets: metrics names a field twice")
    if len(metrics) > MAX_METRICS:
        raise ValueError(f"facets: at most {MAX_METRICS} metrics per call, got {len(metrics)}")
    out = []
    for f in metrics:
        try:
            out.append((f, resolve_range_field(f, schema)[0]))
        except ValueError:
            raise ValueError(f"facets: metrics: field {f!r} is no numeric field; metrics are offered on primary_value "
                             "and the collection's INT64 / DOUBLE fields") from None
    return out


def parse_aggregate(name):
    """("sum" | "avg" | "min" | "max", field) of an output field such as "sum(primary_value)", else None."""
    m = _AGGREGATE.match(name) if isinstance(name, str) else None
    return (m.group(1), m.group(2)) if m else None


def check_args(fields, limit=10, min_count=1, ranges=None, metrics=None, schema=()):
    """The arguments of facets() -> (list of field names, limit, min_count, {field: [(lo, hi), ...]}), or
    ValueError naming the argument.  With metrics= (a list, checked against `schema` by check_metrics) a fifth
    element follows: [(field, "f64" | "i64"), ...]; metrics alone are something to count."""
    if fields is None:
        fields = []
    if isinstance(fields, str) or not isinstance(fields, (list, tuple)):
        raise ValueError(f"facets: fields must be a list of field names, got {fields!r}")
    fields = list(fields)
    for f in fields:
        if not isinstance(f, str) or not f:
            raise ValueError(f"facets: a field name must be a non-empty string, got {f!r}")
    if len(set(fields)) != len(fields):
        raise ValueError("facets: fields names a field twice")
    if len(fields) > MAX_FIELDS:
        raise ValueError(f"facets: at most {MAX_FIELDS} fields per call, got {len(fields)}")
    if not _is_int(limit) or not 1 <= limit <= MAX_LIMIT:
        raise ValueError(f"facets: limit must be an integer in 1..{MAX_LIMIT}, got {limit!r}")
    if not _is_int(min_count) or min_count < 1:
        raise ValueError(f"facets: min_count must be an integer >= 1, got {min_count!r}")
    out = {}
    if ranges is not None:
        if not isinstance(ranges, dict):
            raise ValueError(f"facets: ranges must be a dict of field -> list of (lo, hi), got {ranges!r}")
        for name, rs in ranges.items():
            if not isinstance(name, str) or not name:
                raise ValueError(f"facets: ranges: a field name must be a non-empty string, got {name!r}")
            if not isinstance(rs, (list, tuple)) or not 1 <= len(rs) <= MAX_RANGES:
                raise ValueError(f"facets: ranges[{name!r}] must hold 1..{MAX_RANGES} (lo, hi) pairs")
            checked = []
            for r in rs:
                if not isinstance(r, (list, tuple)) or len(r) != 2:
                    raise ValueError(f"facets: ranges[{name!r}]: a range is a (lo, hi) pair, got {r!r}")
                for b in r:
                    if b is not None and (isinstance(b, (bool, np.bool_)) or not isinstance(b, numbers.Real) or b != b):
                        raise ValueError(f"facets: ranges[{name!r}]: a bound is a real number or None, got {b!r}")
                checked.append((r[0], r[1]))
            out[name] = checked
    checked_metrics = check_metrics(metrics, schema)
    if not fields and not out and not checked_metrics:
        raise ValueError("facets: nothing to count: give fields and / or ranges")
    if metrics is not None:
        return fields, int(limit), int(min_count), out, checked_metrics
    return fields, int(limit), int(min_count), out


_OFFERED = ("period, chunk_type, statement_type, the collection's VARCHAR / BOOL / INT64 fields, its ARRAY fields "
            "of VARCHAR or BOOL elements and, with enable_dynamic_field, dynamic keys")


def resolve_value_field(name: str, schema=(), dynamic_enabled: bool = False):
    """Where the values of a value facet come from: ("builtin", name) | ("own", FieldSchema) |
    ("array", FieldSchema) | ("dynamic", key); ValueError naming the field and what is offered."""
    m = _META_KEY.match(name)
    if m:
        if not dynamic_enabled:
            raise ValueError(f"facets: {name!r} reads a dynamic key, but the collection was made without "
                             f"enable_dynamic_field; value facets are offered on {_OFFERED}")
        return "dynamic", m.group(1) or m.group(2)
    if name in filter_expr.VARCHAR_FIELDS:
        return "builtin", name
    own = next((f for f in schema if f.name == name), None)
    if own is not None:
        if own.is_array:
            if own.element_type in (DataType.VARCHAR, DataType.BOOL):
                return "array", own
            raise ValueError(f"facets: field {name!r} is an ARRAY of {own.element_type.name}; value facets are "
                             f"offered on {_OFFERED}")
        if own.dtype in (DataType.VARCHAR, DataType.BOOL, DataType.INT64):
            return "own", own
        raise ValueError(f"facets: field {name!r} is {own.dtype.name} (use ranges= for a numeric field); value "
                         f"facets are offered on {_OFFERED}")
    if name in _NOT_FACETABLE or name == filter_expr.META:
        raise ValueError(f"facets: field {name!r} cannot be value-faceted; value facets are offered on {_OFFERED}")
    if dynamic_enabled:
        return "dynamic", name
    raise ValueError(f"facets: unknown field {name!r}; value facets are offered on {_OFFERED}")


def resolve_range_field(name: str, schema=()):
    """("f64" | "i64", the host column's name) of a range facet, or ValueError."""
    if name == "primary_value":
        return "f64", name
    own = next((f for f in schema if f.name == name), None)
    if own is not None and not own.is_array and own.dtype in (DataType.INT64, DataType.DOUBLE):
        return ("i64" if own.dtype == DataType.INT64 else "f64"), name
    raise ValueError(f"facets: ranges: field {name!r} is no numeric field; range facets are offered on "
                     "primary_value and the collection's INT64 / DOUBLE fields")


def sort_key(v):
    """The order of bucket values: bools, then ints, then strings."""
    if isinstance(v, (bool, np.bool_)):
        return (0, bool(v))
    if isinstance(v, (int, np.integer)):
        return (1, int(v))
    return (2, v)


def value_ranks(values) -> np.ndarray:
    """int32 [len(values)]: the position of each (distinct) value in the sorted order (sort_key).  A dictionary is
    in first-seen order, so a code is not a rank; the device breaks count ties by this."""
    order = sorted(range(len(values)), key=lambda i: sort_key(values[i]))
    rank = np.empty(len(values), dtype=np.int32)
    rank[order] = np.arange(len(values), dtype=np.int32)
    return rank


def int_bounds(lo, hi):
    """[lo, hi) over an int64 column -> (no_lo, no_hi, empty, ilo, ihi) with int64 ilo <= x < ihi: a float
    bound is compared mathematically (x >= 0.5 is x >= 1), a bound outside int64 is clamped away."""
    no_lo = no_hi = empty = False
    ilo = ihi = 0
    if lo is None or lo == -math.inf:
        no_lo = True
    elif lo == math.inf:
        empty = True
    else:
        ilo = math.ceil(lo)
        if ilo > INT64_MAX:
            empty, ilo = True, 0
        elif ilo < INT64_MIN:
            no_lo, ilo = True, 0
    if hi is None or hi == math.inf:
        no_hi = True
    elif hi == -math.inf:
        empty = True
    else:
        ihi = math.ceil(hi)
        if ihi > INT64_MAX:
            no_hi, ihi = True, 0
        elif ihi <= INT64_MIN:
            empty, ihi = True, 0
    return no_lo, no_hi, empty, int(ilo), int(ihi)


def _double_at_or_above(v) -> float:
    """The smallest double >= v (v a real number: an int of any size too)."""
    try:
        f = float(v)
    except OverflowError:
        return math.inf if v > 0 else -math.inf
    if f < v:
        f = float(np.nextafter(f, math.inf))
    return f


def float_bounds(lo, hi):
    """[lo, hi) over an fp64 column -> (no_lo, no_hi, flo, fhi): for a double x, x >= lo iff x >= the smallest
    double at or above lo, and x < hi iff x < the smallest double at or above hi."""
    return (lo is None, hi is None, 0.0 if lo is None else _double_at_or_above(lo),
            0.0 if hi is None else _double_at_or_above(hi))


def value_facet(counts: Counter, missing: int, limit: int, min_count: int) -> dict:
    """The facet of one field from the count of every value among the passing rows."""
    live = [(v, c) for v, c in counts.items() if c >= 1]
    best = sorted((vc for vc in live if vc[1] >= min_count), key=lambda vc: (-vc[1], sort_key(vc[0])))[:limit]
    total = sum(c for _, c in live)
    return {"buckets": [{"value": v, "count": int(c)} for v, c in best], "distinct": len(live),
            "missing": int(missing), "other": int(total - sum(c for _, c in best))}


def range_facet(values, kind: str, rs) -> dict:
    """The range facet of the passing rows' values (kind "i64": Python ints; "f64": floats)."""
    nan = 0
    if kind == "f64":
        nan = sum(1 for v in values if v != v)
        values = [v for v in values if v == v]
    out = []
    for lo, hi in rs:
        out.append({"from": lo, "to": hi,
                    "count": sum(1 for v in values if (lo is None or v >= lo) and (hi is None or v < hi))})
    return {"ranges": out, "min": min(values) if values else None, "max": max(values) if values else None, "nan": nan}


def stats_reference(values, kind: str) -> dict:
    """The metrics of one group of values (kind "f64": floats; "i64": ints): {"count", "nan", "sum", "avg", "min",
    "max"} as the module's docstring defines them.  The fp64 sum is the exact rational sum rounded once."""
    if kind == "i64":
        vals = [int(v) for v in values]
        total = sum(vals)
        return {"count": len(vals), "nan": 0, "sum": total, "avg": total / len(vals) if vals else None,
                "min": min(vals) if vals else None, "max": max(vals) if vals else None}
    vals = [float(v) for v in values]
    nan = sum(1 for v in vals if v != v)
    vals = [v for v in vals if v == v]
    pos, neg = math.inf in vals, -math.inf in vals
    if pos and neg:
        total = math.nan
    elif pos or neg:
        total = math.inf if pos else -math.inf
    else:
        # sum(Fraction(v) for v in vals), over the common denominator 2^1074 every double has: integer adds
        scaled = 0
        for v in vals:
            num, den = v.as_integer_ratio()   # (den is a power of two, at most 2^1074)
            scaled += num * (_TWO_1074 // den)
        exact = Fraction(scaled, _TWO_1074)
        try:
            total = float(exact)   # (correctly rounded, ties to even)
        except OverflowError:
            total = math.inf if exact > 0 else -math.inf
        if total == 0.0:
            total = 0.0   # (an exact zero sum is +0.0; a non-zero sum never rounds to zero: it is a multiple of 2^-1074)
    return {"count": len(vals), "nan": nan, "sum": total, "avg": total / len(vals) if vals else None,
            "min": min(vals) if vals else None, "max": max(vals) if vals else None}


def facets_reference(columns: dict, schema, dynamic, fields, passing_rows, limit: int = 10, min_count: int = 1,
                     ranges=None, metrics=None) -> dict:
    """What CorpusStore.facets returns, over the host columns.  columns: {field: list} (a store's `columns`);
    schema: the collection's own FieldSchema objects; dynamic: {key: column with None where the row lacks it}, or
    None for a collection without enable_dynamic_field; passing_rows: the row numbers the filter passes."""
    if metrics is None:
        fields, limit, min_count, ranges = check_args(fields, limit, min_count, ranges)
        mplan = None
    else:
        fields, limit, min_count, ranges, mplan = check_args(fields, limit, min_count, ranges, metrics, schema)
    rows = [int(r) for r in passing_rows]
    out = {"count": len(rows), "facets": {}, "ranges": {}}

    def stats_of(rs):
        return {name: stats_reference([columns[name][r] for r in rs], kind) for name, kind in mplan}
    for name in fields:
        kind, what = resolve_value_field(name, schema, dynamic is not None)
        counts: Counter = Counter()
        units: dict = {}   # value -> the rows that hold it (with metrics)
        missing = 0
        if kind in ("builtin", "own"):
            col = columns[what if kind == "builtin" else what.name]
            for r in rows:
                counts[col[r]] += 1
                units.setdefault(col[r], []).append(r)
        elif kind == "array":
            col = columns[what.name]
            for r in rows:
                held = set(col[r])
                counts.update(held)
                missing += not held
                for v in held:
                    units.setdefault(v, []).append(r)
        else:
            col = dynamic.get(what)
            for r in rows:
                v = None if col is None else col[r]
                if isinstance(v, (bool, str)):
                    counts[v] += 1
                    units.setdefault(v, []).append(r)   # (True == 1 cannot collide: only bools and strings come here)
                else:
                    missing += 1
        out["facets"][name] = value_facet(counts, missing, limit, min_count)
        if mplan is not None:
            for b in out["facets"][name]["buckets"]:
                b["metrics"] = stats_of(units[b["value"]])
    if mplan is not None:
        out["metrics"] = stats_of(rows)
    for name, rs in ranges.items():
        kind, col = resolve_range_field(name, schema)
        vals = [columns[col][r] for r in rows]
        out["ranges"][name] = range_facet([float(v) for v in vals] if kind == "f64" else [int(v) for v in vals], kind, rs)
    return out
