"""Dynamic fields (enable_dynamic_field / $meta) on the CPU: what the parser accepts and refuses with and without
`dynamic`, the reference semantics on a table that mixes all five tags in every key, the compiled leaves
(filter_expr.dynamic_leaf_reference) combined by the program against a row-by-row evaluation of the AST, the
exact fp64 interval of an integer literal no double represents, the value checks of an insert, the 64-key
limit, mutation and save / load on a CPU double of GpuIndex, the sharded refusals and the upper layers'
plumbing.  The device side (rf_dynamic_match, the filter buffer, the searches) is covered by
tests/test_dynamic_fields_gpu.py."""
import json
import math

import numpy as np
import pytest
import torch

from oracle import filter_program as ofp, search as osearch
from rag_fin_amd import _lib, filter_expr, schema, service
from rag_fin_amd.schema import DataType, FieldSchema
from rag_fin_amd.store import CorpusStore

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
P53 = 1 << 53
FIELDS = [FieldSchema("bank", DataType.VARCHAR), FieldSchema("fiscal_year", DataType.INT64, default=2024)]

# every kind of value a key can hold; the numbers are the ones where "both to double" goes wrong
VALUES = [None, True, False, 0, 1, 3, -5, 7, P53 - 1, P53, P53 + 1, -P53 + 1, -P53, -P53 - 1, I64_MIN, I64_MAX,
          0.0, -0.0, 3.0, 2.5, -0.3, float("nan"), math.inf, -math.inf, float(P53), -float(P53), float(1 << 63), 1e300,
          "10-K", "10-Q", "annual", "", "Deloitte", "déjà"]


class CpuIndex:
    """CPU double of GpuIndex: fp16 rows in numpy."""

    def __init__(self, dim, capacity, device=None):
        self.dim, self.capacity, self.device = dim, int(capacity), torch.device("cpu")
        self.rows = np.zeros((0, dim), dtype=np.float16)

    @property
    def size(self):
        return self.rows.shape[0]

    def add(self, rows):
        self.rows = np.concatenate([self.rows, rows.numpy().astype(np.float16)])

    def reset(self):
        self.rows = self.rows[:0]

    def get_rows(self, ids):
        return torch.from_numpy(self.rows[np.asarray(ids, dtype=np.int64)])

    def to_fp16(self, x, normalize=True):
        x = np.asarray(x, dtype=np.float32)
        return torch.from_numpy((osearch.l2_normalize_f32(x) if normalize else x).astype(np.float16))

    def compact(self, keep_rows, window_rows=None):
        self.rows = self.rows[np.asarray(keep_rows, dtype=np.int64)]


class HostStore(CorpusStore):
    """CorpusStore on the double, with the constructor signature load_from calls; the row mask of an
    expression comes from the AST's host semantics."""

    def __init__(self, name="t", dim=32, capacity=16, device=None, metric_type="COSINE", fields=None,
                 enable_dynamic_field=False):
        super().__init__(name, dim=dim, capacity=capacity, metric_type=metric_type, index=CpuIndex(dim, capacity),
                         fields=fields, enable_dynamic_field=enable_dynamic_field)

    def _grow(self, need):
        self.index.capacity = max(need, 2 * self.index.capacity)

    def flush(self):
        pass

    def _match_mask(self, expr):
        node = filter_expr.parse(expr, schema=self.schema, dynamic=self.enable_dynamic_field)
        return np.array([node.eval(dict({f: c[r] for f, c in self.columns.items()},
                                        **{"$meta": {k: c[r] for k, c in self.dynamic.items()}}))
                         for r in range(self.num_entities)], dtype=bool)

    def _expr_rows(self, expr):
        return np.flatnonzero(self._match_mask(expr))


def rows(keys, seed=0):
    n = len(keys)
    v = np.random.default_rng(seed).normal(size=(n, 32)).astype(np.float32)
    return [list(keys), [f"text {k}" for k in keys], v, ["Q1_FY2024"] * n, ["c"] * n, ["s"] * n, [float(i) for i in range(n)]]


def same(a, b):
    """Equality that keeps 3 apart from 3.0, True from 1 and NaN equal to NaN."""
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True) and repr(a) == repr(b)


# ---- parser --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("expr", ['source == "x"', '$meta["a"] == 1', "exists a"])
def test_without_dynamic_the_expressions_raise_as_before(expr):
    want = {'source == "x"': "unknown field 'source': 'source' at position 0",
            '$meta["a"] == 1': "unexpected character '\\$' at position 0",
            "exists a": "unknown field 'exists': 'exists' at position 0"}[expr]
    for kw in ({}, {"dynamic": False}, {"schema": FIELDS}):
        with pytest.raises(ValueError, match=want):
            filter_expr.parse(expr, **kw)


def test_parser_accepts_the_dynamic_forms():
    P = lambda e: filter_expr.parse(e, schema=FIELDS, dynamic=True)   # noqa: E731
    assert P('source == "10-K"') == filter_expr.DynCmp("source", "==", "10-K")
    assert P("$meta['page no'] > 3") == filter_expr.DynCmp("page no", ">", 3)
    assert P('$meta["period"] != "x"') == filter_expr.DynCmp("period", "!=", "x")     # not the declared period
    assert P('period != "x"') == filter_expr.Cmp("period", "!=", "x")
    assert P('bank == "a"') == filter_expr.Cmp("bank", "==", "a")                     # a declared field stays one
    assert P("3 >= pages") == filter_expr.DynCmp("pages", "<=", 3)
    assert P("1 < pages <= 5") == filter_expr.And(filter_expr.DynCmp("pages", ">", 1), filter_expr.DynCmp("pages", "<=", 5))
    assert P("-1.5 < $meta[\"x\"] < 1e3") == filter_expr.And(filter_expr.DynCmp("x", ">", -1.5), filter_expr.DynCmp("x", "<", 1000.0))
    assert P("restated == TRUE") == filter_expr.DynCmp("restated", "==", True)
    assert P("pages in [1, 2.5, 3]") == filter_expr.DynIn("pages", [1, 2.5, 3])
    assert P('auditor not in ["a", "b"]') == filter_expr.DynIn("auditor", ["a", "b"], True)
    assert P("flag in [true]") == filter_expr.DynIn("flag", [True]) and P("k in []") == filter_expr.DynIn("k", [])
    assert P('auditor like "Del%"') == filter_expr.DynLike("auditor", "Del%")
    assert P("exists auditor") == filter_expr.Exists("auditor") and P('EXISTS $meta["a b"]') == filter_expr.Exists("a b")
    assert P("not exists a and b == 1") == filter_expr.And(filter_expr.Not(filter_expr.Exists("a")), filter_expr.DynCmp("b", "==", 1))
    assert filter_expr.dynamic_keys_of(P('a == 1 or not ($meta["b c"] like "x%" and exists d) and bank == "x"')) == {"a", "b c", "d"}
    assert filter_expr.fields_of(P('a == 1 and bank == "x" and period == "p"')) == {"bank", "period"}


@pytest.mark.parametrize("expr, match", [
    ("pages < true", "a boolean supports == != in / not in only, not '<': '<' at position 6"),
    ("false >= pages", "a boolean supports == != in / not in only, not '>=': '>=' at position 6"),
    ('pages in [1, "a"]', "holds one type class, numbers here: '\"a\"' at position 13"),
    ("pages in [true, 1]", "holds one type class, booleans here: '1' at position 16"),
    ("exists", "'exists' takes a dynamic key: 'exists' at position 0"),
    ("exists == 3", "'exists' takes a dynamic key: '==' at position 7"),
    ("exists period", "'exists' takes a dynamic key, 'period' is a field of the collection: 'period' at position 7"),
    ("exists bank", "'bank' is a field of the collection: 'bank' at position 7"),
    ("$meta[0] == 1", "\\$meta takes a non-empty string key, as in \\$meta\\[\"key\"\\]: '0' at position 6"),
    ('$meta[""] == 1', "non-empty string key"),
    ("$meta == 1", "expected '\\[' after \\$meta: '==' at position 6"),
    ('$meta["a" == 1', "expected '\\]': '==' at position 10"),
    ('$meta["a"]["b"] == 1', "ARRAY and JSON fields are not supported\\): '\\[' at position 10"),
    ("a[0] == 1", "ARRAY and JSON fields are not supported\\): '\\[' at position 1"),
    ("a == b", "a field compared with a field is not supported\\): 'b' at position 5"),
    ("a + 1 == 2", "arithmetic is not supported\\): '\\+' at position 2"),
    ("a == 1 + 2", "arithmetic is not supported\\): '\\+' at position 7"),
    ("json_contains(a, 1)", "unknown function 'json_contains' \\(ARRAY and JSON fields are not supported\\)"),
    ("array_length(a) == 1", "unknown function 'array_length'"),
    ("sparse == 1", "unknown field 'sparse': 'sparse' at position 0"),
    ("token_embeddings == 1", "unknown field 'token_embeddings'"),
    ('text == "x"', "field 'text' cannot be filtered on"),
    ("$metadata == 1", "unexpected character '\\$' at position 0"),
    ('a like "x%y"', "'like' supports 'p%', '%s' and '%i%' only"),
    ("a like 3", "'like' needs a string pattern: '3' at position 7"),
    ("a", "expected a comparison, 'in' or 'like': end of expression"),
    ("fiscal_year == \"x\"", "fiscal_year is INT64, the literal is a string"),
])
def test_dynamic_refusals_name_the_token_and_its_position(expr, match):
    with pytest.raises(ValueError, match=match):
        filter_expr.parse(expr, schema=FIELDS, dynamic=True)


# ---- the reference semantics -----------------------------------------------------------------------------
def ev(expr, v):
    return filter_expr.parse(expr, dynamic=True).eval({"k": v} if v is not None else {})


def test_reference_semantics_of_single_values():
    assert ev("k == 3", 3) and ev("k == 3", 3.0) and ev("k == 3.0", 3) and not ev("k == 3", True) and not ev("k == 1", True)
    assert not ev("k == true", 1) and ev("k == true", True) and ev("k != true", False) and not ev("k != true", 0)
    assert ev(f"k > {float(P53)!r}", P53 + 1) and not ev(f"k > {P53 + 1}", float(P53)) and ev(f"k < {P53 + 1}", float(P53))
    assert not ev(f"k == {P53 + 1}", float(P53)) and ev(f"k != {P53 + 1}", float(P53)) and ev(f"k >= {P53}", float(P53))
    assert ev(f"k > {I64_MAX}", float(1 << 63)) and not ev(f"k >= {I64_MAX}", I64_MAX - 1) and ev(f"k <= {I64_MIN}", I64_MIN)
    nan = float("nan")
    assert ev("k != 3", nan) and not any(ev(f"k {op} 3", nan) for op in ("==", "<", "<=", ">", ">="))
    assert ev("k not in [3]", nan) and not ev("k in [3]", nan)
    assert ev("k == 0", -0.0) and ev("k in [0.0]", -0.0) and ev("k < 1e999", 1e300) and not ev("k < 1e999", math.inf)
    assert ev('k < "b"', "a") and ev('k > "Z"', "a") and ev('k == ""', "") and not ev('k == "3"', 3) and not ev("k == 3", "3")
    assert ev('k like "10-%"', "10-K") and not ev('k like "10-%"', 10) and ev('k like "%é%"', "déjà")
    # a row that lacks the key, or holds another class, fails every leaf -- != and not in included
    for expr in ("k == 3", "k != 3", "k < 3", "k in [3]", "k not in [3]", 'k != "a"', 'k not in ["a"]', "k != true", 'k like "a%"',
                 "k in []", "k not in []"):
        assert not ev(expr, None), expr
    assert not ev("k != 3", "3") and not ev("k != 3", True) and not ev('k != "a"', 3) and not ev("k not in [true]", "a")
    assert not ev("k not in []", 3) and not ev("k in []", 3)
    # plain negation; exists
    assert ev("not (k == 3)", None) and ev("not (k != 3)", None) and ev("not (k == 3)", "x") and not ev("not (k == 3)", 3.0)
    assert ev("exists k", False) and ev("exists k", "") and ev("exists k", nan) and not ev("exists k", None)
    assert ev('exists $meta["k"]', 0) and ev("not exists k", None)
    # a row may keep its dynamic keys under $meta
    node = filter_expr.parse('$meta["period"] == 3 and period == "p"', dynamic=True)
    assert node.eval({"period": "p", "$meta": {"period": 3}}) and not node.eval({"period": "p", "$meta": {}})


def test_dynamic_class_and_encoding():
    assert [filter_expr.dynamic_class(v) for v in (None, True, 1, 1.5, "x")] == [None, "boolean", "number", "number", "string"]
    code, strings = {"old": 0}, ["old"]
    tags, payload = filter_expr.encode_dynamic([None, True, False, -5, 2.5, "b", "old", "b", I64_MIN, float("nan")], code, strings)
    assert tags.dtype == np.uint8 and payload.dtype == np.int64
    assert tags.tolist() == [0, 1, 1, 2, 3, 4, 4, 4, 2, 3] and strings == ["old", "b"] and code == {"old": 0, "b": 1}
    assert payload[:4].tolist() == [0, 1, 0, -5] and payload[5:9].tolist() == [1, 0, 1, I64_MIN]
    f = payload.view(np.float64)
    assert f[4] == 2.5 and math.isnan(f[9])
    assert (_lib.RF_DTAG_ABSENT, _lib.RF_DTAG_BOOL, _lib.RF_DTAG_INT, _lib.RF_DTAG_DOUBLE, _lib.RF_DTAG_STRING) == (0, 1, 2, 3, 4)


# ---- the compiled leaves, combined by the program == the AST, row by row -----------------------------------
def mixed_table(n, seed):
    """n rows; the keys `k`, `page no` and `aud` each hold all five tags (in different rows), `rare` is held by
    one row in 50, and the declared / built-in columns are those of the extra-fields test."""
    rng = np.random.default_rng(seed)
    pick = lambda off: [VALUES[(i * 7 + off) % len(VALUES)] for i in range(n)]   # noqa: E731  (7 and 34 are coprime)
    return {
        "id": [f"k{i}" for i in range(n)],
        "period": [("Q1_FY2024", "Q2_FY2024", "Q3_FY2024", "")[i] for i in rng.integers(4, size=n)],
        "chunk_type": [("balance_sheet", "key_ratios", "segment")[i] for i in rng.integers(3, size=n)],
        "statement_type": [("consolidated", "standalone")[i] for i in rng.integers(2, size=n)],
        "primary_value": [float(v) for v in rng.normal(size=n).round(1)],
        "bank": [("ICICI", "HDFC", "SBI", "")[i] for i in rng.integers(4, size=n)],
        "fiscal_year": [int(v) for v in rng.integers(2015, 2030, size=n)],
    }, {"k": pick(0), "page no": pick(11), "aud": pick(23), "rare": [i if i % 50 == 7 else None for i in range(n)]}


TABLE, DYN = mixed_table(340, 3)


def encode(values):
    d, code = [], {}
    out = np.array([code.setdefault(v, len(code)) for v in values], dtype=np.int32)
    d.extend(code)
    return d, out


def run_compiled(expr, table=TABLE, dyn=DYN):
    """compile_expr's output interpreted in numpy: the column and dynamic leaves' bitmaps from their definitions
    (column_leaf_reference, dynamic_leaf_reference), then the postfix program by oracle/filter_program.py."""
    n = len(table["id"])
    dicts, codes = {}, {}
    for c, f in enumerate(filter_expr.VARCHAR_FIELDS):
        dicts[f], codes[c] = encode(table[f])
    xd, xcol = {}, {"fiscal_year": np.array(table["fiscal_year"], dtype=np.int64)}
    xd["bank"], xcol["bank"] = encode(table["bank"])
    mirror, strings = {}, {}
    for key, col in dyn.items():
        strings[key] = []
        mirror[key] = filter_expr.encode_dynamic(col, {}, strings[key])
    prog = filter_expr.compile_expr(filter_expr.parse(expr, schema=FIELDS, dynamic=True), dicts,
                                    {k: i for i, k in enumerate(table["id"])}, None, FIELDS, xd, strings)
    nwords = (n + 31) // 32
    bitmaps = np.concatenate([ofp.pack_rows(filter_expr.column_leaf_reference(leaf, xcol[leaf[1]])) for leaf in prog.column_leaves]
                             + [ofp.pack_rows(filter_expr.dynamic_leaf_reference(leaf, *mirror[leaf[1]])) for leaf in prog.dynamic_leaves]
                             + [np.zeros(0, np.uint32)])
    assert bitmaps.size == (len(prog.column_leaves) + len(prog.dynamic_leaves)) * nwords
    ops = prog.resolved_ops(0, 0, nwords)
    offs = [o[2] for o in ops if o[0] == _lib.RF_FOP_BITMAP]
    assert all(o[1] == 0 and o[3] == nwords for o in ops if o[0] == _lib.RF_FOP_BITMAP)
    assert sorted(offs) == [i * nwords for i in range(len(offs))]   # every leaf's bitmap is read exactly once
    return ofp.run_ops(ops, prog.code_sets, prog.row_lists, bitmaps, codes, np.array(table["primary_value"]), n), prog


def run_ast(expr, table=TABLE, dyn=DYN):
    node = filter_expr.parse(expr, schema=FIELDS, dynamic=True)
    n = len(table["id"])
    return np.array([node.eval(dict({f: c[r] for f, c in table.items()}, **{"$meta": {k: c[r] for k, c in dyn.items()}}))
                     for r in range(n)], dtype=bool)


_NUMS = [0, 1, 3, -5, 2.5, -0.3, 3.0, P53, P53 + 1, P53 - 1, -P53 - 1, float(P53), I64_MIN, I64_MAX, I64_MAX + 1, I64_MIN - 1,
         10 ** 30, -10 ** 400, 1e300, "1e999", "-1e999", 0.0]
LEAF_EXPRS = [f"k {op} {v}" for op in ("==", "!=", "<", "<=", ">", ">=") for v in _NUMS] + [
    f"{P53} < k <= {P53 + 1}", "-1 <= k < 3.0", "k in [1, 3, 2.5]", "k not in [1, 3.0]", "k in []", "k not in []",
    f"k in [{P53 + 1}, {I64_MAX}, {I64_MIN}, 1e999, {10 ** 30}, 0]", f"k not in [{P53 + 1}, -1e999, 0.0]",
    f"k in [{', '.join(str(v) for v in range(-2000, 2096))}]",
    'k == "10-K"', 'k != "10-K"', 'k < "a"', 'k >= "10-Q"', 'k == ""', 'k == "none"', 'k != "none"', 'k like "10-%"', 'k like "%e"',
    'k like "%j%"', 'k in ["annual", "x", ""]', 'k not in ["annual"]', 'k not in ["none"]',
    "k == true", "k != true", "k == false", "k in [true, false]", "k not in [false]", "k in [false]",
    "exists k", "not exists k", 'exists $meta["page no"]', "exists rare", "exists nobody", "nobody == 1", "nobody != 1",
    "not (nobody != 1)", 'nobody like "x%"', "rare > 100", "rare != 107", "not (rare != 107)",
]
MIXED_EXPRS = [
    'k == "10-K" and fiscal_year >= 2024', '$meta["page no"] > 3 or bank == "ICICI"', 'not (aud == "Deloitte") and period == "Q1_FY2024"',
    'exists aud and not exists rare and primary_value > 0', 'k != 3 and $meta["page no"] != 3 and aud != 3 and bank != "SBI"',
    'id in ["k3", "k77", "zz"] or (k in [true] and statement_type == "standalone")',
    'not (k < 0 or $meta["page no"] like "%a%") and (aud in [1, 3, 7] or chunk_type like "%ratio%") and fiscal_year in [2020, 2024]',
    '(k == true || k == 1 || k == "annual") && !(bank == "") && $meta["period"] == 1',
    '1 <= k <= 7 and 1 <= $meta["page no"] <= 7 or not (aud not in ["10-K", "10-Q"] or id == "k5")',
]


@pytest.mark.parametrize("expr", LEAF_EXPRS + MIXED_EXPRS)
def test_compiled_program_equals_the_ast(expr):
    got, prog = run_compiled(expr)
    want = run_ast(expr)
    assert np.array_equal(got, want), [(r, DYN["k"][r]) for r in np.flatnonzero(got != want)[:5]]
    assert len(prog.ops) <= _lib.RF_FILTER_MAX_OPS


def test_every_key_of_the_table_holds_every_tag():
    for key in ("k", "page no", "aud"):
        tags, _ = filter_expr.encode_dynamic(DYN[key], {}, [])
        assert set(tags.tolist()) == {0, 1, 2, 3, 4}
    assert run_ast("k != 3").sum() > 0 and run_ast(f"k > {P53}").sum() > 0 and run_ast("not exists k").sum() > 0


def test_leaf_composition():
    C = lambda e: filter_expr.compile_expr(e, {}, {}, None, FIELDS, {}, {"k": ["a", "b", "c"]})   # noqa: E731
    B, F, NOT, AND = _lib.RF_FOP_BITMAP, _lib.RF_FOP_FALSE, _lib.RF_FOP_NOT, _lib.RF_FOP_AND
    inf = math.inf
    p = C("k != 3")   # TAGS(number) and not EQ
    assert [o[0] for o in p.ops] == [B, B, NOT, AND] and [o[1] for o in p.ops[:2]] == [filter_expr.DYNAMIC_LEAF] * 2
    assert p.dynamic_leaves == [("tags", "k", 0b01100), ("nrange", "k", 3, 3, 3, 3.0, 3.0)]
    assert C("exists k").dynamic_leaves == [("tags", "k", 0b11110)]
    assert C("k > 2.5").dynamic_leaves == [("nrange", "k", 3, I64_MAX, _lib.RF_FRANGE_HI_INCL, 2.5, inf)]
    assert C("k == 2.5").dynamic_leaves == [("nrange", "k", 0, -1, 3, 2.5, 2.5)]       # no int row passes
    # an integer literal no double represents: the fp64 side rounds outward, and == passes no double
    assert C(f"k > {P53 + 1}").dynamic_leaves == [("nrange", "k", P53 + 2, I64_MAX, _lib.RF_FRANGE_HI_INCL, float(P53), inf)]
    assert C(f"k >= {P53 + 1}").dynamic_leaves == [("nrange", "k", P53 + 1, I64_MAX, 3, float(P53 + 2), inf)]
    assert C(f"k < {P53 + 1}").dynamic_leaves == [("nrange", "k", I64_MIN, P53, _lib.RF_FRANGE_LO_INCL, -inf, float(P53 + 2))]
    assert C(f"k <= {P53 + 1}").dynamic_leaves == [("nrange", "k", I64_MIN, P53 + 1, 3, -inf, float(P53))]
    assert C(f"k == {P53 + 1}").dynamic_leaves == [("nrange", "k", P53 + 1, P53 + 1, 0, inf, -inf)]
    assert C(f"k > {I64_MAX}").dynamic_leaves == [("nrange", "k", 0, -1, _lib.RF_FRANGE_HI_INCL, float((1 << 63) - 1024), inf)]
    assert C("k in [3, 2.5, 3.0, 1]").dynamic_leaves == [("nset", "k", [1, 3], [1.0, 2.5, 3.0])]
    assert C(f"k in [{P53 + 1}, 1e999]").dynamic_leaves == [("nset", "k", [P53 + 1], [inf])]
    assert C('k >= "b"').dynamic_leaves == [("codeset", "k", [0b110])] and C('k != "b"').dynamic_leaves == [("codeset", "k", [0b101])]
    assert C("k == true").dynamic_leaves == [("bool", "k", 2)] and C("k != true").dynamic_leaves == [("bool", "k", 1)]
    assert C("k in [true, false]").dynamic_leaves == [("bool", "k", 3)]
    for dead in ('k == "z"', "k not in [true, false]", "k in []", "k not in []", "nobody == 1", "exists nobody"):
        assert [o[0] for o in C(dead).ops] == [F] and not C(dead).dynamic_leaves
    many = ", ".join(str(i) for i in range(filter_expr.MAX_INT_SET + 1))
    with pytest.raises(ValueError, match="65537 distinct values, at most 65536"):
        C(f"k in [{many}]")
    assert len(C(f"k in [{many[:-7]}]").dynamic_leaves[0][2]) == filter_expr.MAX_INT_SET
    # column leaves first, dynamic leaves behind them
    p = C('fiscal_year > 1 and k == 1 and bank == "x" and exists k')
    assert len(p.column_leaves) == 1 and len(p.dynamic_leaves) == 2   # (bank's dictionary is empty: FALSE)
    assert [o[2] for o in p.resolved_ops(0, 100, 10) if o[0] == B] == [100, 110, 120]


@pytest.mark.parametrize("v", [P53 + 1, -P53 - 1, I64_MAX, I64_MIN, I64_MAX - 1, 3, 0, 2.5, -0.0, 10 ** 30, -10 ** 400, 10 ** 400,
                               math.inf, -math.inf, (1 << 62) + 1], ids=lambda v: f"{v:.6g}" if isinstance(v, float) else f"int{v.bit_length()}{'-' if v < 0 else ''}")
@pytest.mark.parametrize("op", ["==", "<", "<=", ">", ">="])
def test_f64_interval_selects_exactly_the_doubles_python_does(op, v):
    """The interval's neighbourhood, by Python's exact int-against-float comparison."""
    flags, lo, hi = filter_expr.f64_interval(op, v)
    xs = {-math.inf, math.inf, 0.0, -0.0, 5e-324, -5e-324, 1.7976931348623157e308, -1.7976931348623157e308}
    try:
        f = float(v)
    except OverflowError:
        f = math.inf if v > 0 else -math.inf
    for base in (f, lo, hi):
        x = base
        for _ in range(3):
            x = math.nextafter(x, math.inf)
            xs.add(x)
        x = base
        for _ in range(3):
            x = math.nextafter(x, -math.inf)
            xs.add(x)
        xs.add(base)
    for x in xs:
        got = (x >= lo if flags & _lib.RF_FRANGE_LO_INCL else x > lo) and (x <= hi if flags & _lib.RF_FRANGE_HI_INCL else x < hi)
        assert got == filter_expr._compare(x, op, v), (x, op, v)


# ---- the store: values, the key limit, mutation, persistence ----------------------------------------------
def test_the_flag_off_refuses_as_before():
    st = HostStore(fields=FIELDS)
    assert st.enable_dynamic_field is False and st.dynamic == {}
    with pytest.raises(ValueError, match="insert: unknown extra field 'source' \\(declared: bank, fiscal_year\\)"):
        st.add(*rows(["a"]), extra={"bank": ["x"], "source": ["10-K"]})
    with pytest.raises(ValueError, match="insert: unknown extra field 'source' \\(the collection declares none\\)"):
        HostStore().add(*rows(["a"]), extra={"source": ["10-K"]})
    with pytest.raises(ValueError, match="insert expects 9 columns"):
        st.insert(rows(["a"]) + [["x"], [1], [{"source": "10-K"}]])
    with pytest.raises(ValueError, match="insert expects 7 columns"):
        HostStore().insert(rows(["a"]) + [[{"source": "10-K"}]])
    st.add(*rows(["a"]), extra={"bank": ["x"]})
    with pytest.raises(ValueError, match="unknown field 'source'"):
        st.query('source == "10-K"')
    with pytest.raises(KeyError, match="unknown output field 'source'"):
        st.query("", output_fields=["source"])
    with pytest.raises(KeyError, match="unknown output field '\\$meta'"):
        st.query("", output_fields=["$meta"])


def test_add_insert_and_read_back():
    st = HostStore(fields=FIELDS, enable_dynamic_field=True)
    st.add(*rows(["a", "b", "c"]), extra={"bank": ["x", "y", "z"], "source": ["10-K", None, 3], "page no": [1, 2.0, True]})
    assert st.columns["bank"] == ["x", "y", "z"] and st.columns["fiscal_year"] == [2024] * 3 and "source" not in st.columns
    assert same(st.dynamic, {"source": ["10-K", None, 3], "page no": [1, 2.0, True]})
    # insert: one optional trailing column of dicts; rows without a key lack it; a new key back-fills None
    st.insert(rows(["d", "e"], 1) + [["p", "q"], [2020, 2021], [{"auditor": "Deloitte", "source": "10-Q"}, None]])
    st.insert(rows(["f"], 2) + [["r"], [2022]])
    st.add(*rows(["g"], 3), extra={"bank": ["s"], "np": np.array([np.int64(5)]), "nf": [np.float32(0.5)], "nb": [np.bool_(True)]})
    assert same(st.dynamic["source"], ["10-K", None, 3, "10-Q", None, None, None])
    assert same(st.dynamic["auditor"], [None, None, None, "Deloitte", None, None, None])
    assert same([st.dynamic[k][-1] for k in ("np", "nf", "nb")], [5, 0.5, True])
    got = st.query('id in ["a", "c", "d", "e"]', output_fields=["source", "page no", "$meta", "bank", "nobody"])
    assert same(got, [
        {"source": "10-K", "page no": 1, "$meta": {"source": "10-K", "page no": 1}, "bank": "x", "nobody": None, "id": "a"},
        {"source": 3, "page no": True, "$meta": {"source": 3, "page no": True}, "bank": "z", "nobody": None, "id": "c"},
        {"source": "10-Q", "page no": None, "$meta": {"source": "10-Q", "auditor": "Deloitte"}, "bank": "p", "nobody": None, "id": "d"},
        {"source": None, "page no": None, "$meta": {}, "bank": "q", "nobody": None, "id": "e"}])
    assert [r["id"] for r in st.query('source == "10-K" or $meta["page no"] >= 2 or exists auditor')] == ["a", "b", "d"]
    assert [r["id"] for r in st.query("source != 3")] == [] and [r["id"] for r in st.query('source != "x"')] == ["a", "d"]
    with pytest.raises(ValueError, match="group_by_field 'source': a dynamic key cannot be grouped by"):
        st.search(np.zeros((1, 32), np.float32), limit=2, group_by_field="source")


@pytest.mark.parametrize("bad, match", [
    ({"k": [[1], 2]}, "dynamic field 'k': value \\[1\\] \\(list\\) is not a bool, an int, a float, a str or None"),
    ({"k": [1, {"a": 1}]}, "\\(dict\\) is not"),
    ({"k": [1, (1, 2)]}, "\\(tuple\\) is not"),
    ({"k": [1, b"x"]}, "\\(bytes\\) is not"),
    ({"k": [1, 1 << 63]}, "dynamic field 'k': value 9223372036854775808 is outside the int64 range"),
    ({"k": [-(1 << 63) - 1, 1]}, "outside the int64 range"),
    ({"k": [1]}, "insert columns differ in length \\(dynamic field 'k': 1 values for 2 rows\\)"),
    ({"": [1, 2]}, "a dynamic key is a non-empty string, got ''"),
    ({3: [1, 2]}, "a dynamic key is a non-empty string, got 3"),
])
def test_bad_values_raise_before_anything_changes(bad, match):
    st = HostStore(enable_dynamic_field=True)
    st.add(*rows(["z"]), extra={"k": [1]})
    writes = [lambda: st.add(*rows(["a", "b"]), extra={"good": [1, 2], **bad})]
    if "differ in length" not in match:   # (a column of dicts cannot differ in length from itself)
        writes.append(lambda: st.upsert(rows(["z", "b"]) + [[{k: v[j] for k, v in bad.items()} for j in range(2)]]))
    for write in writes:
        with pytest.raises(ValueError, match=match):
            write()
        assert st.num_entities == 1 and same(st.dynamic, {"k": [1]}) and st.index.size == 1 and st.columns["id"] == ["z"]
    with pytest.raises(ValueError, match="the \\$meta column holds one dict \\(or None\\) per row, got list"):
        st.insert(rows(["a"]) + [[[1]]])
    with pytest.raises(ValueError, match="\\$meta: 2 values for 1 rows"):
        st.insert(rows(["a"]) + [[{}, {}]])
    with pytest.raises(ValueError, match="insert expects 7 columns"):
        st.insert(rows(["a"]) + [[{}], [{}]])
    fs = HostStore(fields=FIELDS, enable_dynamic_field=True)
    with pytest.raises(ValueError, match="\\$meta holds the declared field 'bank'"):
        fs.insert(rows(["a"]) + [["x"], [1], [{"bank": "y"}]])
    assert st.num_entities == 1 and fs.num_entities == 0


def test_at_most_64_distinct_keys():
    assert schema.MAX_DYNAMIC_KEYS == 64
    st = HostStore(enable_dynamic_field=True)
    st.add(*rows(["a"]), extra={f"key {i}": [i] for i in range(60)})
    st.add(*rows(["b"]), extra={f"key {i}": [i] for i in range(58, 64)})     # 4 new ones: 64
    st.add(*rows(["n"]), extra={"one more": [None]})                         # held by no row: no key
    assert len(st.dynamic) == 64
    with pytest.raises(ValueError, match="65 distinct dynamic keys, a collection holds at most 64"):
        st.add(*rows(["c"]), extra={"key 0": [1], "one more": [1]})
    with pytest.raises(ValueError, match="65 distinct dynamic keys"):
        st.insert(rows(["c"]) + [[{"one more": 1}]])
    assert st.num_entities == 3 and "one more" not in st.dynamic
    st.delete('id == "b"')     # keys 60..63 were held by b alone: gone with it, as in a fresh store
    assert len(st.dynamic) == 60
    st.add(*rows(["c"]), extra={"one more": [1]})
    assert len(st.dynamic) == 61 and same(st.dynamic["one more"], [None, None, 1])


def fresh(st):
    """A fresh store of st's rows."""
    out = HostStore(fields=st.schema, enable_dynamic_field=True)
    n = st.num_entities
    if n:
        out.add(st.columns["id"], st.columns["text"], st.index.get_rows(np.arange(n)).float().numpy(), st.columns["period"],
                st.columns["chunk_type"], st.columns["statement_type"], st.columns["primary_value"],
                extra=dict({f.name: st.columns[f.name] for f in st.schema}, **st.dynamic))
    return out


def test_delete_upsert_and_growth_equal_a_fresh_store():
    st = HostStore(capacity=4, enable_dynamic_field=True)
    keys = [f"r{i}" for i in range(40)]
    st.add(*rows(keys), extra={"k": [VALUES[i % len(VALUES)] for i in range(40)], "only r7": [1 if i == 7 else None for i in range(40)]})
    assert st.index.capacity >= 40
    st.delete("k == 3 or k == true or not exists k")
    assert same(st.dynamic, fresh(st).dynamic) and st.num_entities < 40 and "only r7" in st.dynamic
    st.upsert(rows(["r7", "new", "r9"], 5) + [[{"k": "up"}, {"j": 2.5}, None]])
    assert "only r7" not in st.dynamic and st.columns["id"][-3:] == ["r7", "new", "r9"]
    assert same([st.dynamic["k"][-3:], st.dynamic["j"][-3:]], [["up", None, None], [None, 2.5, None]])
    assert same(st.dynamic, fresh(st).dynamic) and all(len(c) == st.num_entities for c in st.dynamic.values())
    st.delete("exists k or exists j")
    assert st.dynamic == {} and st.num_entities > 0
    st.drop()
    assert st.dynamic == {} and st.num_entities == 0


def test_save_and_load_round_trip(tmp_path):
    st = HostStore(fields=FIELDS, enable_dynamic_field=True)
    n = len(VALUES)
    st.add(*rows([f"r{i}" for i in range(n)]), extra={"bank": ["b"] * n, "k": VALUES, "page no": VALUES[::-1]})
    st.save(str(tmp_path / "d"))
    meta = json.load(open(tmp_path / "d" / "columns.json"))
    assert meta["enable_dynamic_field"] is True and list(meta["dynamic"]) == ["k", "page no"] and "k" not in meta["columns"]
    raw = open(tmp_path / "d" / "columns.json").read()
    assert '"k": [null, true, false, 0, 1, 3, -5, 7,' in raw and "0.0, -0.0, 3.0, 2.5" in raw
    back = HostStore.load_from(str(tmp_path / "d"))
    assert back.enable_dynamic_field and same(back.dynamic, st.dynamic) and back.schema == st.schema
    assert [type(v) for v in back.dynamic["k"]] == [type(v) for v in VALUES]
    for expr in ("k == 3", "k != 3", 'k < "b"', "k == true", "exists k", f"k > {P53}"):
        assert np.array_equal(back._match_mask(expr), st._match_mask(expr))
    # without the flag the directory is what it was: no new key
    plain = HostStore(fields=FIELDS)
    plain.add(*rows(["a"]), extra={"bank": ["b"]})
    plain.save(str(tmp_path / "p"))
    assert set(json.load(open(tmp_path / "p" / "columns.json"))) == {"format", "name", "dim", "metric_type", "n", "columns", "fields"}
    assert HostStore.load_from(str(tmp_path / "p")).enable_dynamic_field is False
    # an empty store with the flag keeps the flag
    HostStore(enable_dynamic_field=True).save(str(tmp_path / "e"))
    assert HostStore.load_from(str(tmp_path / "e")).enable_dynamic_field is True


def test_sharded_store_refuses_dynamic_fields(tmp_path):
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    with pytest.raises(NotImplementedError, match="dynamic fields \\(enable_dynamic_field\\) are not implemented for the sharded store"):
        ShardedCorpusStore(enable_dynamic_field=True)
    st = HostStore(enable_dynamic_field=True)
    st.add(*rows(["a"]), extra={"k": [1]})
    st.save(str(tmp_path / "d"))
    with pytest.raises(NotImplementedError, match="holds dynamic fields, which are not implemented for the sharded store"):
        ShardedCorpusStore.load_from(str(tmp_path / "d"))


# ---- upper layers -------------------------------------------------------------------------------------
class Emb:
    dim = 32

    def encode_to_device(self, texts):
        return np.random.default_rng(0).normal(size=(len(texts), 32)).astype(np.float32)

    def encode(self, texts):
        return np.zeros((len(texts), 32), np.float32)


def test_service_ingest_carries_dynamic_keys():
    chunks = [{"id": f"c{i}", "text": f"chunk {i}", "period": p, "chunk_type": "c", "statement_type": "s",
               "primary_value": 1.0, "page": i} for i, p in enumerate(["Q1_FY2024", "Q3_FY2023", "Q4_FY2023"])]
    values = {"bank": "ICICI", "auditor": "Deloitte", "page no": lambda c: c["page"] or None,
              "restated": lambda c: True if c["period"].startswith("Q3") else None}
    with pytest.raises(ValueError, match="'auditor' is not a declared field"):
        service.extra_columns(FIELDS, chunks, values)
    assert service.extra_columns(FIELDS, chunks, values, dynamic=True) == {
        "bank": ["ICICI"] * 3, "auditor": ["Deloitte"] * 3, "page no": [None, 1, 2], "restated": [None, True, None]}
    st = HostStore(fields=FIELDS, enable_dynamic_field=True)
    assert service.ingest(st, Emb(), chunks, field_values=values) == 3
    assert st.columns["bank"] == ["ICICI"] * 3 and st.columns["fiscal_year"] == [2024] * 3
    assert same(st.dynamic, {"auditor": ["Deloitte"] * 3, "page no": [None, 1, 2], "restated": [None, True, None]})
    assert service.ingest(st, Emb(), chunks[:1], upsert=True, field_values={"bank": "HDFC"}) == 1
    assert same(st.dynamic["auditor"], ["Deloitte", "Deloitte", None]) and st.columns["bank"][-1] == "HDFC"
    with pytest.raises(ValueError, match="'auditor' is not a declared field"):
        service.ingest(HostStore(fields=FIELDS), Emb(), chunks, field_values=values)


def test_vector_rag_takes_dynamic_output_fields():
    from rag_fin_amd.rag import OUTPUT_FIELDS, VectorRAG
    st = HostStore(fields=FIELDS, enable_dynamic_field=True)
    rag = VectorRAG("k", embedder=Emb(), store=st, extra_output_fields=["bank", "auditor", "page no"])
    assert rag.output_fields == OUTPUT_FIELDS + ["bank", "auditor", "page no"]
    with pytest.raises(ValueError, match="'auditor' is not a field the store declares"):
        VectorRAG("k", embedder=Emb(), store=HostStore(fields=FIELDS), extra_output_fields=["auditor"])
    with pytest.raises(ValueError, match="'text' is not a field the store declares"):
        VectorRAG("k", embedder=Emb(), store=st, extra_output_fields=["text"])


def test_micro_batcher_parses_with_the_stores_flag():
    from rag_fin_amd.batching import MicroBatcher

    class Rag:
        class collection:
            analyzer = None
            schema = tuple(FIELDS)
            enable_dynamic_field = True

        def search_batch(self, queries, top_k, expr=None):
            return [[{"q": q, "expr": e}] for q, e in zip(queries, expr if isinstance(expr, (list, tuple)) else [expr] * len(queries))]

    mb = MicroBatcher(Rag(), max_wait_ms=1.0)
    try:
        assert mb.search("q", 1, expr='$meta["page no"] > 3 and source == "10-K"')[0]["expr"] == '$meta["page no"] > 3 and source == "10-K"'
        with pytest.raises(ValueError, match="a field compared with a field"):
            mb.search("q", 1, expr="source == other")
    finally:
        mb.close()


# ---- the entry point's checks ---------------------------------------------------------------------------
def test_dynamic_match_checks_its_arguments_without_a_gpu():
    """Every refusal of rf_dynamic_match comes before any device call."""
    import ctypes
    lib = _lib.load_library()
    INVALID = -1

    def leaf(**kw):
        a = (_lib.DynamicLeaf * 17)()
        for l in a:
            l.kind, l.tags_dev, l.payload_dev, l.ihi = _lib.RF_DLEAF_NUM_RANGE, 4097, 4096, 1
        for k, v in kw.items():
            setattr(a[0], k, v)
        return a

    def call(a, n_leaves=1, cs=4096, iv=4096, fv=4096, n_rows=100, out=4096):
        return lib.rf_dynamic_match(a, n_leaves, cs, iv, fv, n_rows, out, None)

    K = _lib
    assert call(None) == INVALID and call(leaf(), out=None) == INVALID
    assert call(leaf(), n_leaves=0) == INVALID and call(leaf(), n_leaves=17) == INVALID
    assert call(leaf(), n_rows=-1) == INVALID and call(leaf(), n_rows=1 << 32) == INVALID
    assert call(leaf(), out=4098) == INVALID and call(leaf(), cs=4097) == INVALID
    assert call(leaf(), iv=4100) == INVALID and call(leaf(), fv=4100) == INVALID
    assert call(leaf(kind=0)) == INVALID and call(leaf(kind=6)) == INVALID and call(leaf(kind=-1)) == INVALID
    assert call(leaf(tags_dev=None)) == INVALID and call(leaf(payload_dev=None)) == INVALID and call(leaf(payload_dev=4100)) == INVALID
    assert call(leaf(kind=K.RF_DLEAF_TAGS, payload_dev=4100)) == INVALID
    assert call(leaf(kind=K.RF_DLEAF_TAGS, flags=0x100)) == INVALID and call(leaf(kind=K.RF_DLEAF_BOOL, flags=4)) == INVALID
    assert call(leaf(kind=K.RF_DLEAF_NUM_RANGE, flags=4)) == INVALID and call(leaf(kind=K.RF_DLEAF_NUM_SET, flags=1)) == INVALID
    assert call(leaf(kind=K.RF_DLEAF_STR_CODESET, flags=1)) == INVALID and call(leaf(kind=K.RF_DLEAF_TAGS, flags=-1)) == INVALID
    for kind, null in ((K.RF_DLEAF_STR_CODESET, {"cs": None}), (K.RF_DLEAF_NUM_SET, {"iv": None})):
        assert call(leaf(kind=kind, off=-1, len=1)) == INVALID and call(leaf(kind=kind, off=0, len=-1)) == INVALID
        assert call(leaf(kind=kind, off=0, len=1), **null) == INVALID
    assert call(leaf(kind=K.RF_DLEAF_NUM_SET, foff=-1, flen=1)) == INVALID and call(leaf(kind=K.RF_DLEAF_NUM_SET, flen=-1)) == INVALID
    assert call(leaf(kind=K.RF_DLEAF_NUM_SET, flen=1), fv=None) == INVALID
    assert call(leaf(kind=K.RF_DLEAF_NUM_SET, len=65537)) == INVALID and call(leaf(kind=K.RF_DLEAF_NUM_SET, flen=65537)) == INVALID
    a = leaf()
    a[1].kind = 9   # a later leaf is checked too
    assert call(a, n_leaves=2) == INVALID
    assert b"rf_dynamic_match" in lib.rf_last_error()
    # nothing to write: no launch -- and a set of length 0, or TAGS without a payload, is legal
    assert call(leaf(), n_rows=0) == 0 and call(leaf(kind=K.RF_DLEAF_NUM_SET), n_rows=0, iv=None, fv=None) == 0
    assert call(leaf(kind=K.RF_DLEAF_STR_CODESET), n_rows=0, cs=None) == 0
    assert call(leaf(kind=K.RF_DLEAF_TAGS, flags=0xFF, payload_dev=None, tags_dev=None), n_rows=0) == 0
    assert ctypes.sizeof(_lib.DynamicLeaf) == 88
    assert "dynamic_match.hip" in __import__("rag_fin_amd.build", fromlist=["SOURCES"]).SOURCES
