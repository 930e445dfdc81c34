"""ARRAY fields on the CPU: the schema's forms and refusals, the value checks of an insert, what the expression
parser and compiler accept and refuse for ARRAY_CONTAINS / ARRAY_CONTAINS_ALL / ARRAY_CONTAINS_ANY / ARRAY_LENGTH
and F[i], the compiled program interpreted in numpy (array_leaf_reference) against a row-by-row evaluation of the
AST (a hypothesis property over random arrays and expressions included), mutation and save / load on a CPU double
of GpuIndex, the CSR mirror's compaction on CPU tensors, the upper layers' plumbing, and the condition the GPU store
test relies on.  The device side (rf_array_match, the filter buffer, the searches) is covered by
tests/test_array_fields_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch
from hypothesis import given, settings, strategies as hs

import array_fields_common as common
from array_fields_common import I64_MAX, I64_MIN
from oracle import filter_program as ofp
from rag_fin_amd import _lib, filter_expr, schema, service
from rag_fin_amd.schema import DataType, FieldSchema
from rag_fin_amd.store import CorpusStore, _ArrayColumn
from test_extra_fields_cpu import CpuIndex, rows

GOLD_STORE = os.path.join(os.path.dirname(__file__), "golden", "store_v1")
NAN, INF = float("nan"), float("inf")


def array(name, elem, cap=8, **kw):
    return FieldSchema(name, DataType.ARRAY, element_type=elem, max_capacity=cap, **kw)


FIELDS = [array("tags", DataType.VARCHAR, 4, default=[]), array("years", DataType.INT64, 4),
          array("weights", DataType.DOUBLE, 4, default=[1.0]), array("flags", DataType.BOOL, 4, default=[]),
          FieldSchema("bank", DataType.VARCHAR, default="ICICI")]


class HostStore(CorpusStore):
    """CorpusStore on the CPU double of GpuIndex, with the constructor signature load_from calls; the row mask of
    an expression comes from the AST's host semantics."""

    def __init__(self, name="t", dim=32, capacity=16, device=None, metric_type="COSINE", fields=None):
        super().__init__(name, dim=dim, capacity=capacity, metric_type=metric_type, index=CpuIndex(dim, capacity),
                         fields=fields)

    def _grow(self, need):
        self.index.capacity = max(need, 2 * self.index.capacity)

    def flush(self):
        pass

    def _match_mask(self, expr):
        node = filter_expr.parse(expr, schema=self.schema)
        return np.array([node.eval({f: c[r] for f, c in self.columns.items()}) for r in range(self.num_entities)],
                        dtype=bool)

    def _expr_rows(self, expr):
        return np.flatnonzero(self._match_mask(expr))


def extras(n, base=0):
    return {"tags": [["npa", "nim", "casa"][:(base + i) % 4] for i in range(n)],
            "years": [[2019 + (base + i) % 5] * ((base + i) % 3) for i in range(n)],
            "weights": [[0.5 * (base + i), NAN][:(base + i) % 3] for i in range(n)],
            "flags": [[(base + i) % 2 == 0] * ((base + i) % 2) for i in range(n)]}


# ---- schema ------------------------------------------------------------------------------------------
def test_array_field_schema_forms():
    f = FieldSchema("tags", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=16)
    assert (f.name, f.dtype, f.element_type, f.max_capacity, f.default, f.is_array) == \
        ("tags", DataType.ARRAY, DataType.VARCHAR, 16, None, True)
    assert DataType.ARRAY == 22 and DataType.ARRAY.name == "ARRAY"
    assert [t.name for t in DataType] == ["BOOL", "INT64", "DOUBLE", "VARCHAR"] and len(list(DataType)) == 4
    for dtype in ("ARRAY", "array", 22, DataType.ARRAY):
        for elem in ("int64", 5, DataType.INT64):
            g = FieldSchema("y", dtype, element_type=elem, max_capacity=4096)
            assert (g.dtype, g.element_type, g.max_capacity) == (DataType.ARRAY, DataType.INT64, 4096)
    assert array("t", DataType.VARCHAR, default=[]).default == [] and array("t", DataType.DOUBLE, default=(1, 2)).default == [1.0, 2.0]
    assert not FieldSchema("b", DataType.VARCHAR).is_array and FieldSchema("b", DataType.VARCHAR).element_type is None
    for f in FIELDS + [array("d", DataType.DOUBLE, default=[NAN, INF][1:])]:
        d = json.loads(json.dumps(f.to_dict()))
        assert FieldSchema.from_dict(d) == f and repr(FieldSchema.from_dict(d)) == repr(f)
    assert FIELDS[0].to_dict() == {"name": "tags", "dtype": "ARRAY", "element_type": "VARCHAR", "max_capacity": 4, "default": []}
    assert repr(FIELDS[1]) == "FieldSchema('years', DataType.ARRAY, element_type=DataType.INT64, max_capacity=4)"
    assert array("t", DataType.INT64, 4) != array("t", DataType.INT64, 5) and array("t", DataType.INT64) != array("t", DataType.DOUBLE)
    st = HostStore(fields=FIELDS)
    assert list(st.schema) == FIELDS and list(st.columns)[-5:] == ["tags", "years", "weights", "flags", "bank"]
    assert len(schema.check_fields([array(f"a{i}", DataType.BOOL) for i in range(32)])) == 32
    with pytest.raises(ValueError, match="33 extra fields declared"):
        schema.check_fields([array(f"a{i}", DataType.BOOL) for i in range(33)])


@pytest.mark.parametrize("make, match", [
    (lambda: FieldSchema("t", DataType.ARRAY), "needs element_type and max_capacity"),
    (lambda: FieldSchema("t", DataType.ARRAY, element_type=DataType.INT64), "needs element_type and max_capacity"),
    (lambda: FieldSchema("t", DataType.ARRAY, max_capacity=4), "needs element_type and max_capacity"),
    (lambda: array("t", DataType.INT64, 0), "max_capacity must be an integer in 1..4096, got 0"),
    (lambda: array("t", DataType.INT64, 4097), "max_capacity must be an integer in 1..4096, got 4097"),
    (lambda: array("t", DataType.INT64, True), "max_capacity must be an integer"),
    (lambda: array("t", DataType.INT64, 2.0), "max_capacity must be an integer"),
    (lambda: array("t", DataType.ARRAY), "element_type .* is not supported"),
    (lambda: array("t", "JSON"), "element_type 'JSON' is not supported"),
    (lambda: array("t", 101), "element_type 101 is not supported"),
    (lambda: FieldSchema("b", DataType.VARCHAR, element_type=DataType.INT64), "belong to an ARRAY field"),
    (lambda: FieldSchema("b", DataType.INT64, max_capacity=4), "belong to an ARRAY field"),
    (lambda: FieldSchema("x", 101), "not supported"),
    (lambda: FieldSchema("x", "JSON"), "not supported"),
    (lambda: array("t", DataType.INT64, 2, default=[1, 2, 3]), "default holds 3 elements, max_capacity is 2"),
    (lambda: array("t", DataType.INT64, 2, default=3), "default 3 \\(int\\) is not a list"),
    (lambda: array("t", DataType.INT64, 2, default=["a"]), "is an ARRAY of INT64, element 'a' \\(str\\) is not"),
])
def test_schema_refusals(make, match):
    with pytest.raises(ValueError, match=match):
        make()


def test_check_value_of_an_array():
    f, g, h, b = FIELDS[1], FIELDS[2], FIELDS[0], FIELDS[3]
    assert schema.check_value(f, (1, np.int64(2))) == [1, 2] and all(type(x) is int for x in schema.check_value(f, np.array([1, 2])))
    assert schema.check_value(f, [I64_MIN, I64_MAX]) == [I64_MIN, I64_MAX] and schema.check_value(f, []) == []
    assert schema.check_value(g, [1, np.float32(0.5)]) == [1.0, 0.5] and type(schema.check_value(g, [1])[0]) is float
    assert schema.check_value(h, np.array(["a", "b"])) == ["a", "b"] and type(schema.check_value(h, np.array(["a"]))[0]) is str
    assert schema.check_value(b, np.array([True, False])) == [True, False]
    assert schema.column_from_json(g, [[1, 2.5], []]) == [[1.0, 2.5], []] and type(schema.column_from_json(g, [[1]])[0][0]) is float
    with pytest.raises(ValueError, match="not a bool, an int, a float, a str or None"):
        schema.dynamic_value("k", ["a"])                       # dynamic fields keep refusing lists


# ---- insert checks: nothing changes on a refused batch ---------------------------------------------------
@pytest.mark.parametrize("extra, match", [
    ({"tags": [["a"] * 5, []]}, "field 'tags': value holds 5 elements, max_capacity is 4"),
    ({"tags": [["a", 1], []]}, "field 'tags' is an ARRAY of VARCHAR, element 1 \\(int\\) is not"),
    ({"years": [[2020, "x"], []]}, "field 'years' is an ARRAY of INT64, element 'x' \\(str\\) is not"),
    ({"years": [[2020, True], []]}, "field 'years' is an ARRAY of INT64, element True \\(bool\\) is not"),
    ({"years": [[2020.0], []]}, "field 'years' is an ARRAY of INT64, element 2020.0 \\(float\\) is not"),
    ({"years": [[1 << 63], []]}, "field 'years': element 9223372036854775808 is outside the int64 range"),
    ({"years": [2020, 2021]}, "field 'years' is ARRAY, value 2020 \\(int\\) is not a list"),
    ({"years": [[1], "ab"]}, "field 'years' is ARRAY, value 'ab' \\(str\\) is not a list"),
    ({"years": [[1], np.zeros((2, 2))]}, "is not a list"),
    ({"years": [[1]]}, "columns differ in length \\(field 'years': 1 values for 2 rows\\)"),
    ({"years": 5}, "the column of ARRAY field 'years' is a list of lists, got int"),
    ({"flags": [[1], []], "years": [[], []]}, "field 'flags' is an ARRAY of BOOL, element 1 \\(int\\) is not"),
    ({"weights": [["x"], []], "years": [[], []]}, "field 'weights' is an ARRAY of DOUBLE"),
    ({}, "field 'years' has no default and no column was supplied"),
])
def test_value_checks_are_made_before_anything_changes(extra, match):
    st = HostStore(fields=FIELDS)
    st.add(*_add_args(["a", "b", "c"]), extra=extras(3))
    before = json.dumps(st.columns)
    for call in (lambda: st.add(*_add_args(["x", "y"]), extra=extra),
                 lambda: st.insert(rows(["x", "y"]) + [extra.get(f.name) for f in FIELDS]),
                 lambda: st.upsert(rows(["a", "y"]) + [extra.get(f.name) for f in FIELDS])):
        with pytest.raises(ValueError, match=match):
            call()
        assert json.dumps(st.columns) == before and st.index.size == 3 and st.num_entities == 3


def _add_args(keys):
    r = rows(keys)
    return r[0], r[1], r[2], r[3], r[4], r[5], r[6]


# ---- parser -------------------------------------------------------------------------------------------
A, L, E = filter_expr.ArrContains, filter_expr.ArrLength, filter_expr.ArrElem
Cmp, In, Like, And, Not = filter_expr.Cmp, filter_expr.In, filter_expr.Like, filter_expr.And, filter_expr.Not


@pytest.mark.parametrize("expr, node", [
    ('ARRAY_CONTAINS(tags, "npa")', A("tags", ["npa"], "any")),
    ("array_contains(years, 2020)", A("years", [2020], "any")),
    ("Array_Contains(weights, 1)", A("weights", [1.0], "any")),
    ("ARRAY_CONTAINS(flags, TRUE)", A("flags", [True], "any")),
    ('ARRAY_CONTAINS_ALL(tags, ["a", "b", "a"])', A("tags", ["a", "b", "a"], "all")),
    ("array_contains_all(years, [])", A("years", [], "all")),
    ("ARRAY_CONTAINS_ANY(years, [1, 2.5, -3])", A("years", [1, 2.5, -3], "any")),
    ("array_contains_any(weights, [1e999, -0.0])", A("weights", [INF, -0.0], "any")),
    ("ARRAY_LENGTH(tags) > 2", L("tags", ">", 2)),
    ("array_length(tags) != 0", L("tags", "!=", 0)),
    ("3 >= ARRAY_LENGTH(tags)", L("tags", "<=", 3)),
    ("1 <= array_length(years) < 3", And(L("years", ">=", 1), L("years", "<", 3))),
    ("ARRAY_LENGTH(years) == -1", L("years", "==", -1)),
    ('tags[0] == "npa"', E("tags", 0, Cmp("tags", "==", "npa"))),
    ('tags[4095] != "npa"', E("tags", 4095, Cmp("tags", "!=", "npa"))),
    ("years[2] >= 2020.5", E("years", 2, Cmp("years", ">=", 2020.5))),
    ("2020 == years[1]", E("years", 1, Cmp("years", "==", 2020))),
    ('"a" < tags[1] <= "c"', And(E("tags", 1, Cmp("tags", ">", "a")), E("tags", 1, Cmp("tags", "<=", "c")))),
    ("-1 < weights[0] <= 0.5", And(E("weights", 0, Cmp("weights", ">", -1.0)), E("weights", 0, Cmp("weights", "<=", 0.5)))),
    ("years[0] in [1, 2]", E("years", 0, In("years", [1, 2], False))),
    ('tags[3] not in ["x"]', E("tags", 3, In("tags", ["x"], True))),
    ('tags[0] like "n%"', E("tags", 0, Like("tags", "n%"))),
    ("flags[0] == false", E("flags", 0, Cmp("flags", "==", False))),
    ('not (tags[0] == "a") and !ARRAY_CONTAINS(tags, "b")', And(Not(E("tags", 0, Cmp("tags", "==", "a"))), Not(A("tags", ["b"], "any")))),
])
def test_accepted_forms(expr, node):
    assert repr(filter_expr.parse(expr, schema=FIELDS)) == repr(node)
    assert filter_expr.array_fields_of(filter_expr.parse(expr, schema=FIELDS)) == {node.field if not isinstance(node, And) else
                                                                                  filter_expr.array_fields_of(node).pop()}


@pytest.mark.parametrize("expr, match", [
    ('tags == "npa"', r"'tags' is an ARRAY field: .* not compared whole: 'tags' at position 0"),
    ('tags in ["npa"]', r"'tags' is an ARRAY field: .*: 'tags' at position 0"),
    ('tags like "n%"', r"'tags' is an ARRAY field: .*: 'tags' at position 0"),
    ('"npa" == tags', r"'tags' is an ARRAY field: .*: 'tags' at position 9"),
    ('bank == "x" and years > 3', r"'years' is an ARRAY field: .*: 'years' at position 16"),
    ('tags[-1] == "a"', r"an array index is a non-negative integer literal below 4096: '-' at position 5"),
    ('tags[1.5] == "a"', r"an array index is a non-negative integer literal below 4096: '1.5' at position 5"),
    ('tags["a"] == "a"', r"an array index is a non-negative integer literal below 4096: '\"a\"' at position 5"),
    ('tags[4096] == "a"', r"an array index is a non-negative integer literal below 4096: '4096' at position 5"),
    ('tags[0 == "a"', r"expected '\]': '==' at position 7"),
    ("tags[0] == 1", r"tags is VARCHAR, the literal is not a string: '1' at position 11"),
    ('years[0] == "a"', r"years is INT64, the literal is a string: '\"a\"' at position 12"),
    ("years[0] == true", r"years is INT64, the literal is a boolean: 'true' at position 12"),
    ('years[0] like "2%"', r"'like' needs a VARCHAR field, 'years' is not one: 'like' at position 9"),
    ("flags[0] > false", r"a BOOL field supports == != in / not in only, not '>': '>' at position 9"),
    ("flags[0] == 1", r"flags is BOOL, the literal is not true or false: '1' at position 12"),
    ('weights[0] == "x"', r"weights is DOUBLE, the literal is a string"),
    ("years[0] in [1, \"a\"]", r"years is INT64, the literal is a string: '\"a\"' at position 16"),
    ("years[0] == 9223372036854775808", r"outside the int64 range: '9223372036854775808' at position 12"),
    ("ARRAY_CONTAINS(tags, 1)", r"tags is VARCHAR, the literal is not a string: '1' at position 21"),
    ('ARRAY_CONTAINS(years, "a")', r"years is INT64, the literal is a string: '\"a\"' at position 22"),
    ("ARRAY_CONTAINS(flags, 0)", r"flags is BOOL, the literal is not true or false: '0' at position 22"),
    ('ARRAY_CONTAINS(tags, ["a"])', r"expected a literal: '\[' at position 21"),
    ('ARRAY_CONTAINS_ANY(tags, "a")', r"expected '\[': '\"a\"' at position 25"),
    ('ARRAY_CONTAINS_ALL(tags, ["a", 2])', r"tags is VARCHAR, the literal is not a string: '2' at position 31"),
    ('ARRAY_CONTAINS(tags "a")', r"expected ',': '\"a\"' at position 20"),
    ('ARRAY_CONTAINS(tags, "a"', r"expected '\)': end of expression"),
    ("ARRAY_LENGTH(tags) > 1.5", r"ARRAY_LENGTH is compared with an integer: '1.5' at position 21"),
    ('ARRAY_LENGTH(tags) == "a"', r"ARRAY_LENGTH is compared with an integer: '\"a\"' at position 22"),
    ("true == ARRAY_LENGTH(tags)", r"ARRAY_LENGTH is compared with an integer: 'true' at position 0"),
    ("ARRAY_LENGTH(tags) in [1]", r"expected a comparison operator after ARRAY_LENGTH\(...\): 'in' at position 19"),
    ("ARRAY_LENGTH(tags)", r"expected a comparison operator after ARRAY_LENGTH\(...\): end of expression"),
    ('TEXT_MATCH(tags, "npa")', r"TEXT_MATCH takes the field 'text' only, not 'tags': 'tags' at position 11"),
    # the messages existing tests pin stay word for word
    ('bank[0] == "x"', r"expected a comparison, 'in' or 'like' \(ARRAY and JSON fields are not supported\): '\[' at position 4"),
    ("array_length(bank) > 1", r"unknown function 'array_length' \(ARRAY and JSON fields are not supported\): 'array_length' at position 0"),
    ('ARRAY_CONTAINS(bank, "x")', r"unknown function 'ARRAY_CONTAINS' \(ARRAY and JSON fields are not supported\): 'ARRAY_CONTAINS' at position 0"),
    ('array_contains_any(nope, ["x"])', r"unknown function 'array_contains_any' \(ARRAY and JSON fields are not supported\)"),
    ('array_sum(years) > 1', r"unknown function 'array_sum' \(ARRAY and JSON fields are not supported\)"),
    ('json_contains(tags, "x")', r"unknown function 'json_contains' \(ARRAY and JSON fields are not supported\): 'json_contains' at position 0"),
    ('json_contains(bank, "x")', r"ARRAY and JSON fields are not supported\): 'json_contains' at position 0"),
])
def test_refusals_name_the_token_and_its_position(expr, match):
    with pytest.raises(ValueError, match=match):
        filter_expr.parse(expr, schema=FIELDS)


def test_pinned_messages_on_a_dynamic_store():
    for expr, match in [("a[0] == 1", "ARRAY and JSON fields are not supported\\): '\\[' at position 1"),
                        ('$meta["a"]["b"] == 1', "ARRAY and JSON fields are not supported\\): '\\[' at position 10"),
                        ("array_length(a) == 1", "unknown function 'array_length'"),
                        ("json_contains(a, 1)", "unknown function 'json_contains' \\(ARRAY and JSON fields are not supported\\)")]:
        with pytest.raises(ValueError, match=match):
            filter_expr.parse(expr, schema=FIELDS, dynamic=True)
    assert isinstance(filter_expr.parse('tags[0] == "a" and a == 1', schema=FIELDS, dynamic=True), And)


# ---- compiler ---------------------------------------------------------------------------------------------
def compile_(expr, dicts=None):
    return filter_expr.compile_expr(filter_expr.parse(expr, schema=FIELDS), {}, {}, None, FIELDS,
                                    dicts if dicts is not None else {"tags": ["npa", "nim", "casa"], "flags": [False, True]})


def ops_of(prog):
    return [o[0] for o in prog.ops]


def test_constants_and_limits():
    T, F, B, NOT, AND = _lib.RF_FOP_TRUE, _lib.RF_FOP_FALSE, _lib.RF_FOP_BITMAP, _lib.RF_FOP_NOT, _lib.RF_FOP_AND
    for expr, want in [("ARRAY_CONTAINS_ALL(tags, [])", [T]), ("ARRAY_CONTAINS_ANY(tags, [])", [F]),
                       ('ARRAY_CONTAINS_ALL(tags, ["npa", "none"])', [F]), ('ARRAY_CONTAINS(tags, "none")', [F]),
                       ("ARRAY_LENGTH(tags) < 0", [F]), ("ARRAY_LENGTH(tags) == -1", [F]), ("ARRAY_LENGTH(tags) != -1", [F, NOT]),
                       ("ARRAY_CONTAINS(years, 2.5)", [F]), ("ARRAY_CONTAINS_ALL(years, [1, 2.5])", [F]),
                       ("ARRAY_CONTAINS_ANY(years, [2.5, 1e30])", [F]), ('tags[0] == "none"', [F])]:
        p = compile_(expr)
        assert ops_of(p) == want and not p.array_leaves, expr
    assert compile_('ARRAY_CONTAINS_ANY(tags, ["casa", "none", "npa", "npa"])').array_leaves == [("match", "tags", "code", [0, 2], 1)]
    assert compile_('ARRAY_CONTAINS_ALL(tags, ["casa", "npa", "casa"])').array_leaves == [("match", "tags", "code", [0, 2], 2)]
    assert compile_("ARRAY_CONTAINS_ANY(years, [3, 1, 2.5, 3.0])").array_leaves == [("match", "years", "i64", [1, 3], 1)]
    assert compile_("ARRAY_CONTAINS_ALL(weights, [0.0, -0.0, 1])").array_leaves == [("match", "weights", "f64", [0.0, 1.0], 2)]
    assert compile_("ARRAY_CONTAINS(flags, true)").array_leaves == [("match", "flags", "code", [1], 1)]
    assert compile_("ARRAY_LENGTH(tags) >= 2").array_leaves == [("length", "tags", 2, I64_MAX)]
    assert compile_("ARRAY_LENGTH(tags) <= 2").array_leaves == [("length", "tags", 0, 2)]
    p = compile_("years[2] != 5")                                 # LENGTH(F) > i AND NOT (F[i] == v)
    assert ops_of(p) == [B, B, NOT, AND] and p.array_leaves == [("length", "years", 3, I64_MAX), ("elem", "years", 2, ("irange", "years", 5, 5))]
    p = compile_("not (years[2] == 5)")                           # plain negation: passes the short rows
    assert ops_of(p) == [B, NOT] and p.array_leaves == [("elem", "years", 2, ("irange", "years", 5, 5))]
    assert compile_('tags[1] != "npa"').array_leaves == [("elem", "tags", 1, ("codeset", "tags", [0b110]))]
    many = ", ".join(str(i) for i in range(65))
    assert len(compile_(f"ARRAY_CONTAINS_ALL(years, [{many[:-4]}])").array_leaves[0][3]) == 64
    with pytest.raises(ValueError, match="ARRAY_CONTAINS_ALL\\(years, \\[...\\]\\) holds 65 distinct values, at most 64"):
        compile_(f"ARRAY_CONTAINS_ALL(years, [{many}])")
    big = filter_expr.ArrContains("years", list(range(65537)), "any")
    with pytest.raises(ValueError, match="holds 65537 distinct values, at most 65536"):
        filter_expr.compile_expr(big, {}, {}, None, FIELDS, {})
    ok = filter_expr.compile_expr(filter_expr.ArrContains("years", list(range(65536)) + [5, 7], "any"), {}, {}, None, FIELDS, {})
    assert len(ok.array_leaves[0][3]) == 65536


def test_array_bitmaps_follow_the_dynamic_leaves():
    p = filter_expr.compile_expr(filter_expr.parse('bank == "ICICI" and k == 1 and tags[0] == "npa" and ARRAY_LENGTH(years) > 1',
                                                   schema=FIELDS, dynamic=True), {}, {}, None, FIELDS,
                                 {"bank": ["ICICI"], "tags": ["npa"]}, {"k": []})
    assert (len(p.column_leaves), len(p.dynamic_leaves), len(p.array_leaves)) == (1, 1, 2)
    bitmap_ops = [o for o in p.resolved_ops(8, 100, 10) if o[0] == _lib.RF_FOP_BITMAP]
    assert [(o[1], o[2], o[3]) for o in bitmap_ops] == [(0, 100, 10), (0, 110, 10), (0, 120, 10), (0, 130, 10)]
    assert filter_expr.ARRAY_LEAF == 3 and [o[1] for o in p.ops if o[0] == _lib.RF_FOP_BITMAP] == [1, 2, 3, 3]
    arr = p.ops_ctypes(8, 100, 10)
    assert [(a.off, a.len) for a in arr if a.op == _lib.RF_FOP_BITMAP] == [(100, 10), (110, 10), (120, 10), (130, 10)]
    # a program without array leaves resolves exactly as before
    q = filter_expr.compile_expr(filter_expr.parse('bank == "ICICI" and k == 1', schema=FIELDS, dynamic=True), {}, {}, None,
                                 FIELDS, {"bank": ["ICICI"]}, {"k": []})
    assert [o[2] for o in q.resolved_ops(8, 100, 10) if o[0] == _lib.RF_FOP_BITMAP] == [100, 110] and q.array_leaves == []


# ---- the compiled program, interpreted in numpy, equals the AST row by row ------------------------------------
NP_OF = {DataType.INT64: np.int64, DataType.DOUBLE: np.float64}


def encode(values):
    code = {}
    out = np.array([code.setdefault(v, len(code)) for v in values], dtype=np.int32)
    return list(code), out


def run_compiled(expr, table, fields):
    """compile_expr's output interpreted in numpy: the column and array leaves' bitmaps from their references, then
    the postfix program by oracle/filter_program.py."""
    n = len(table["id"])
    dicts, codes = {}, {}
    for c, f in enumerate(filter_expr.VARCHAR_FIELDS):
        dicts[f], codes[c] = encode(table[f])
    xd, xcol, csr = {}, {}, {}
    for f in fields:
        coded = (f.element_type if f.is_array else f.dtype) in (DataType.VARCHAR, DataType.BOOL)
        if f.is_array:
            d, code = [], {}
            lens, vals = filter_expr.encode_array(table[f.name], NP_OF.get(f.element_type, np.int32), code if coded else None, d)
            csr[f.name] = (np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), vals)
            if coded:
                xd[f.name] = d
        elif coded:
            xd[f.name], xcol[f.name] = encode(table[f.name])
        else:
            xcol[f.name] = np.array(table[f.name], dtype=NP_OF[f.dtype])
    prog = filter_expr.compile_expr(filter_expr.parse(expr, schema=fields), dicts, {k: i for i, k in enumerate(table["id"])},
                                    None, fields, xd)
    nwords = (n + 31) // 32
    bitmaps = np.concatenate([ofp.pack_rows(filter_expr.column_leaf_reference(leaf, xcol[leaf[1]])) for leaf in prog.column_leaves] +
                             [ofp.pack_rows(filter_expr.array_leaf_reference(leaf, *csr[leaf[1]])) for leaf in prog.array_leaves] +
                             [np.zeros(0, np.uint32)])
    assert bitmaps.size == (len(prog.column_leaves) + len(prog.array_leaves)) * nwords
    ops = prog.resolved_ops(0, 0, nwords)
    return ofp.run_ops(ops, prog.code_sets, prog.row_lists, bitmaps, codes, np.array(table["primary_value"]), n), prog


def run_ast(expr, table, fields):
    node = filter_expr.parse(expr, schema=fields)
    return np.array([node.eval({f: c[r] for f, c in table.items()}) for r in range(len(table["id"]))], dtype=bool)


TABLE = {k: v for k, v in common.make_table(400, seed=2).items() if k != common.DYNAMIC_KEY}
STATIC_EXPRS = [e for e, _ in common.STORE_EXPRS if "pages" not in e and "_MATCH" not in e]


@pytest.mark.parametrize("expr", STATIC_EXPRS)
def test_compiled_program_equals_the_ast(expr):
    got, _ = run_compiled(expr, TABLE, common.FIELDS)
    assert np.array_equal(got, run_ast(expr, TABLE, common.FIELDS))


# hypothesis: random arrays of all four element types AND random expressions over them.  At most 4 leaves of at
# most 5 operations each (F[i] not in [..] over doubles: 3 leaves, 2 ORs, a NOT, a LENGTH and an AND make 8), 3
# connectives and a NOT per node: below RF_FILTER_MAX_OPS = 64 by construction, so nothing is discarded.
_TAGS = ["npa", "nim", "casa", "", "zz"]
_INTV = [I64_MIN, I64_MAX, 0, -1, 2019, 2020, 2021]
_DBLV = [NAN, 0.0, -0.0, INF, -INF, 0.5, -0.5, 1.0]


def _rows_of(values):
    # (duplicate elements and empty rows come by themselves from 5..8 values and lengths 0..4)
    return hs.lists(hs.lists(hs.sampled_from(values), min_size=0, max_size=4), min_size=9, max_size=9)


@hs.composite
def tables(draw):
    n = 9
    return {"id": [f"k{i}" for i in range(n)], "period": ["Q1_FY2024"] * n, "chunk_type": ["c"] * n,
            "statement_type": ["s"] * n, "primary_value": [float(i) for i in range(n)],
            "tags": draw(_rows_of(_TAGS)), "years": draw(_rows_of(_INTV)), "weights": draw(_rows_of(_DBLV)),
            "flags": draw(_rows_of([True, False])), "bank": [("ICICI", "HDFC", "SBI")[i % 3] for i in range(n)]}


_STR = hs.sampled_from(_TAGS + ["none"]).map(json.dumps)
_INT = hs.one_of(hs.sampled_from(_INTV + [2022]), hs.sampled_from([2019.5, 2020.0, 1e30, -1e30])).map(repr)
_DBL = hs.sampled_from([0.0, -0.0, 0.5, -0.5, 1.0, 2.5, 1e999, -1e999]).map(lambda v: repr(v).replace("inf", "1e999"))
_BOOL = hs.sampled_from(["true", "false", "TRUE"])
_CMPS = hs.sampled_from(["==", "!=", "<", "<=", ">", ">="])
_EQ = hs.sampled_from(["==", "!="])
_IDX = hs.sampled_from(["0", "1", "3", "4", "4095"])
_NEG = hs.sampled_from(["in", "not in"])
_CASE = hs.sampled_from([str.upper, str.lower, str.title])


def _list(lits):
    return hs.lists(lits, min_size=0, max_size=3).map(lambda v: "[" + ", ".join(v) + "]")


def _leaves_of(name, lit, cmps):
    return [
        hs.builds(lambda c, v: f"{c('array_contains')}({name}, {v})", _CASE, lit),
        hs.builds(lambda c, k, v: f"{c('array_contains_' + k)}({name}, {v})", _CASE, hs.sampled_from(["all", "any"]), _list(lit)),
        hs.builds(lambda c, o, v: f"{c('array_length')}({name}) {o} {v}", _CASE, _CMPS, hs.integers(-1, 5)),
        hs.builds(lambda a, o1, o2, b: f"{a} {o1} ARRAY_LENGTH({name}) {o2} {b}", hs.integers(-1, 3), hs.sampled_from(["<", "<="]),
                  hs.sampled_from(["<", "<="]), hs.integers(0, 5)),
        hs.builds(lambda i, o, v: f"{name}[{i}] {o} {v}", _IDX, cmps, lit),
        hs.builds(lambda v, o, i: f"{v} {o} {name}[{i}]", lit, cmps, _IDX),
        hs.builds(lambda i, o, v: f"{name}[{i}] {o} {v}", _IDX, _NEG, _list(lit)),
    ]


LEAVES = hs.one_of(
    *_leaves_of("tags", _STR, _CMPS), *_leaves_of("years", _INT, _CMPS), *_leaves_of("weights", _DBL, _CMPS),
    *_leaves_of("flags", _BOOL, _EQ),
    hs.builds(lambda i, p: f"tags[{i}] like {json.dumps(p)}", _IDX, hs.sampled_from(["n%", "%a", "%a%", "npa"])),
    hs.builds(lambda a, i, b: f"{a} < years[{i}] <= {b}", _INT, _IDX, _INT),
    hs.sampled_from(['bank == "ICICI"', "primary_value > 3", 'id in ["k0", "k5"]']),
)


@hs.composite
def expressions(draw):
    terms = draw(hs.lists(LEAVES, min_size=1, max_size=4))
    terms = [("not " if draw(hs.booleans()) else "") + "(" + t + ")" for t in terms]
    while len(terms) > 1:   # join two neighbours at a time: every tree shape
        i = draw(hs.integers(0, len(terms) - 2))
        joined = "(" + terms[i] + draw(hs.sampled_from([" and ", " or ", " && ", " || "])) + terms[i + 1] + ")"
        terms[i:i + 2] = [("not " if draw(hs.booleans()) else "") + joined]
    return terms[0]


@settings(max_examples=300, deadline=None)
@given(tables(), expressions())
def test_random_arrays_and_expressions_compile_to_what_the_ast_says(table, expr):
    got, prog = run_compiled(expr, table, FIELDS)
    assert len(prog.ops) <= _lib.RF_FILTER_MAX_OPS and prog.max_depth() <= _lib.RF_FILTER_MAX_DEPTH
    assert np.array_equal(got, run_ast(expr, table, FIELDS)), (expr, table)


# ---- the store on the CPU double ------------------------------------------------------------------------------
def same_columns(a, b):
    return json.dumps(a.columns) == json.dumps(b.columns)          # (json spells NaN, so NaN rows compare equal)


def test_mutations_equal_a_fresh_store_of_the_surviving_rows():
    st = HostStore(fields=FIELDS, capacity=4)
    st.add(*_add_args(list("abcd")), extra=extras(4))
    st.insert(rows(list("efgh"), seed=1) + [extras(4, 4)[f.name] for f in FIELDS[:4]] + [["HDFC"] * 4])   # growth past 4
    assert st.num_entities == 8 and st.index.capacity >= 8
    assert st.columns["tags"] == extras(8)["tags"] and st.columns["bank"] == ["ICICI"] * 4 + ["HDFC"] * 4
    assert st.delete("ARRAY_LENGTH(tags) == 0").delete_count == 2                     # rows a, e
    assert st.delete('ARRAY_CONTAINS(tags, "casa") and ARRAY_LENGTH(years) == 0').delete_count == 1   # row d
    up = rows(["b", "z"], seed=2) + [[["up"], []], [[1], [2, 3]], [[], [NAN]], [[True], []], ["SBI", "SBI"]]
    assert st.upsert(up).upsert_count == 2
    keys = ["c", "f", "g", "h", "b", "z"]
    assert st.columns["id"] == keys
    fresh = HostStore(fields=FIELDS)
    e = extras(8)
    pick = [2, 5, 6, 7]
    fresh.add(*_add_args(["c", "f", "g", "h"]), extra={k: [v[i] for i in pick] for k, v in e.items()} | {"bank": ["ICICI", "HDFC", "HDFC", "HDFC"]})
    fresh.upsert(up)
    for f in ["id", "text"] + [f.name for f in FIELDS]:
        assert json.dumps(st.columns[f]) == json.dumps(fresh.columns[f]), f
    for expr in ('ARRAY_CONTAINS(tags, "npa")', "ARRAY_LENGTH(years) >= 1", "weights[0] != 1", "flags[0] == true"):
        out = ["tags", "years", "flags"]
        assert st.query(expr, output_fields=out) == fresh.query(expr, output_fields=out)
    assert st.query('ARRAY_CONTAINS(tags, "up")', output_fields=["tags", "years", "weights", "flags", "bank"]) == \
        [{"tags": ["up"], "years": [1], "weights": [], "flags": [True], "bank": "SBI", "id": "b"}]
    got = st.query('id in ["z"]', output_fields=["tags"])[0]["tags"]
    got.append("mutated")                                           # a hit's list is a copy
    assert st.columns["tags"][-1] == []
    # a column that is not supplied takes the default, a fresh list per row
    st.add(*_add_args(["p", "q"]), extra={"years": [[1], [2]]})
    assert st.columns["tags"][-2:] == [[], []] and st.columns["tags"][-1] is not st.columns["tags"][-2]
    assert st.columns["weights"][-2:] == [[1.0], [1.0]]
    st.drop()
    assert st.num_entities == 0 and st.columns["tags"] == []


def test_save_load_round_trip_and_old_directories(tmp_path):
    st = HostStore(fields=FIELDS)
    st.add(*_add_args(list("abcdef")), extra=extras(6) | {"weights": [[NAN, INF], [-0.0], [], [1.0], [2.5, 2.5], [-INF]]})
    st.save(str(tmp_path / "a"))
    back = HostStore.load_from(str(tmp_path / "a"))
    assert back.schema == st.schema and same_columns(back, st)
    assert repr(back.columns["weights"]) == repr(st.columns["weights"])       # -0.0, nan and inf survive
    assert all(type(x) is float for r in back.columns["weights"] for x in r)
    meta = json.load(open(tmp_path / "a" / "columns.json"))
    assert meta["fields"][0] == {"name": "tags", "dtype": "ARRAY", "element_type": "VARCHAR", "max_capacity": 4, "default": []}
    # a store without ARRAY fields writes the columns.json it wrote before: no new key
    plain = [FieldSchema("bank", DataType.VARCHAR), FieldSchema("fiscal_year", DataType.INT64, default=2024)]
    old = HostStore(fields=plain)
    old.add(*_add_args(list("ab")), extra={"bank": ["x", "y"]})
    old.save(str(tmp_path / "b"))
    meta = json.load(open(tmp_path / "b" / "columns.json"))
    assert list(meta) == ["format", "name", "dim", "metric_type", "n", "columns", "fields"]
    assert meta["fields"] == [{"name": "bank", "dtype": "VARCHAR"}, {"name": "fiscal_year", "dtype": "INT64", "default": 2024}]
    none = HostStore()
    none.add(*_add_args(list("ab")))
    none.save(str(tmp_path / "c"))
    assert list(json.load(open(tmp_path / "c" / "columns.json"))) == ["format", "name", "dim", "metric_type", "n", "columns"]
    gold = HostStore.load_from(GOLD_STORE)
    assert gold.schema == () and gold.num_entities > 0


def test_the_csr_mirror_follows_appends_and_compaction():
    """_ArrayColumn on CPU tensors: synced append-only, and after a compaction equal to a fresh mirror of the
    surviving rows (the dictionary stays append-only)."""
    cpu = torch.device("cpu")
    rows_ = [["a", "b"], [], ["b"], [], [], ["c", "a", "a"], ["d"], []]
    col = _ArrayColumn(cpu, DataType.VARCHAR)
    col.sync(rows_, 3)
    col.sync(rows_, 8)
    assert col.offsets.tolist() == [0, 2, 2, 3, 3, 3, 6, 7, 7] and col.values.tolist() == [0, 1, 1, 2, 0, 0, 3]
    assert col.dict == ["a", "b", "c", "d"] and (col.n, col.nnz) == (8, 7) and col.values.dtype == torch.int32
    keep = [1, 2, 5, 7]
    col.compact(torch.tensor(keep))
    fresh = _ArrayColumn(cpu, DataType.VARCHAR)
    fresh.sync([rows_[i] for i in keep], 4)
    assert col.offsets.tolist() == fresh.offsets.tolist() == [0, 0, 1, 4, 4] and (col.n, col.nnz) == (4, 4)
    assert [col.dict[c] for c in col.values.tolist()] == [fresh.dict[c] for c in fresh.values.tolist()] == ["b", "c", "a", "a"]
    assert col.dict == ["a", "b", "c", "d"]
    col.sync([rows_[i] for i in keep] + [["e"]], 5)                # appends go on behind a compaction
    assert col.offsets.tolist() == [0, 0, 1, 4, 4, 5] and col.dict[-1] == "e"
    col.compact(torch.tensor([], dtype=torch.int64))
    assert col.offsets.tolist() == [0] and col.values.numel() == 0 and (col.n, col.nnz) == (0, 0)
    ints = _ArrayColumn(cpu, DataType.INT64)
    ints.sync([[I64_MIN], [], [I64_MAX, 7]], 3)
    assert ints.values.tolist() == [I64_MIN, I64_MAX, 7] and ints.values.dtype == torch.int64 and not ints.coded
    dbl = _ArrayColumn(cpu, DataType.DOUBLE)
    dbl.sync([[NAN, -0.0], [INF]], 2)
    assert dbl.values.dtype == torch.float64 and repr(dbl.values.tolist()) == "[nan, -0.0, inf]"
    flags = _ArrayColumn(cpu, DataType.BOOL)
    flags.sync([[True, False, True]], 1)
    assert flags.values.tolist() == [0, 1, 0] and flags.dict == [True, False]
    flags.sync([], 0)                                               # a shorter collection: re-encoded from row 0
    assert flags.offsets.tolist() == [0] and flags.dict == [True, False]


def test_array_fields_are_refused_where_a_scalar_is_needed():
    from rag_fin_amd.ranker import DecayRanker
    st = HostStore(fields=FIELDS)
    st.add(*_add_args(list("ab")), extra=extras(2))
    q = np.zeros((1, 32), np.float32)
    with pytest.raises(ValueError, match="group_by_field 'tags': an ARRAY field cannot be grouped by"):
        st.search(q, limit=1, group_by_field="tags")
    with pytest.raises(ValueError, match="decay ranker: field 'years' is an ARRAY field; it must be primary_value or"):
        st.search(q, limit=1, ranker=DecayRanker("years", "gauss", origin=2024, scale=3))
    with pytest.raises(ValueError, match="takes the field 'text' only, not 'tags'"):
        st.query('TEXT_MATCH(tags, "npa")')


# ---- upper layers ------------------------------------------------------------------------------------
def test_service_ingest_carries_lists():
    chunks = [{"id": f"c{i}", "text": f"chunk {i}", "period": p, "chunk_type": "c", "statement_type": "s",
               "primary_value": 1.0, "years": [2020 + i]} for i, p in enumerate(["Q1_FY2024", "Q3_FY2023"])]
    values = {"tags": lambda c: ["npa", c["period"][:2]], "flags": [True, False]}
    cols = service.extra_columns(FIELDS, chunks, values)
    assert cols == {"tags": [["npa", "Q1"], ["npa", "Q3"]], "years": [[2020], [2021]], "flags": [[True, False]] * 2}

    class Emb:
        dim = 32

        def encode_to_device(self, texts):
            return np.random.default_rng(0).normal(size=(len(texts), 32)).astype(np.float32)

    st = HostStore(fields=FIELDS)
    assert service.ingest(st, Emb(), chunks, field_values=values) == 2
    assert st.columns["tags"] == [["npa", "Q1"], ["npa", "Q3"]] and st.columns["years"] == [[2020], [2021]]
    assert st.columns["flags"] == [[True, False]] * 2 and st.columns["flags"][0] is not st.columns["flags"][1]
    assert st.columns["weights"] == [[1.0], [1.0]] and st.columns["bank"] == ["ICICI"] * 2
    assert service.ingest(st, Emb(), [dict(chunks[0], years=[1, 2])], upsert=True, field_values={"tags": []}) == 1
    assert st.columns["id"] == ["c1", "c0"] and st.columns["tags"][-1] == [] and st.columns["years"][-1] == [1, 2]
    with pytest.raises(ValueError, match="field 'tags' is an ARRAY of VARCHAR, element 3"):
        service.ingest(st, Emb(), [dict(chunks[0], id="n")], field_values={"tags": [3]})
    assert st.num_entities == 2


def test_vector_rag_tool_and_rest_bodies_carry_lists():
    from rag_fin_amd import adapter, mcp_server
    from rag_fin_amd.rag import OUTPUT_FIELDS, VectorRAG
    from rag_fin_amd.store import Hit

    class Emb:
        dim = 32

        def encode(self, texts):
            return np.zeros((len(texts), 32), np.float32)

    class Store:
        schema = tuple(FIELDS)
        num_entities = 1
        analyzer = None

        def load(self):
            pass

        def search(self, data, anns_field, param, limit, **kw):
            self.kw = kw
            row = {"text": "t", "period": "Q1", "chunk_type": "c", "statement_type": "s", "primary_value": 1.0,
                   "tags": ["npa", "nim"], "years": []}
            return [[Hit(0, "a", 0.5, {f: row[f] for f in kw["output_fields"]})] for _ in range(len(data))]

    st = Store()
    rag = VectorRAG("k", embedder=Emb(), store=st, extra_output_fields=["tags", "years"])
    expr = 'ARRAY_CONTAINS(tags, "npa") and ARRAY_LENGTH(years) == 0'
    (ctx,) = rag.search("net profit", 1, expr=expr)
    assert st.kw["output_fields"] == OUTPUT_FIELDS + ["tags", "years"] and st.kw["expr"] == expr
    assert (ctx["tags"], ctx["years"]) == (["npa", "nim"], [])
    mcp_server.set_rag(rag)
    try:
        r = mcp_server.search_vectors("net profit", 1, filter=expr)
        assert r["status"] == "success" and json.loads(json.dumps(r))["results"][0]["tags"] == ["npa", "nim"]
        args = adapter.search_args(adapter.SearchRequest(query="net profit", top_k=1, filter=expr))   # the body of POST /search
        r = mcp_server.search_vectors(**args)
        assert r["status"] == "success" and r["results"][0]["years"] == [] and st.kw["expr"] == expr
    finally:
        mcp_server.set_rag(None)


# ---- the condition the GPU store test relies on -------------------------------------------------------------
def test_every_store_expression_of_the_gpu_test_selects_some_rows_and_not_all():
    table = common.make_table()
    assert len(table["id"]) == common.N == 5000 and len(common.STORE_EXPRS) >= 50
    for expr, const in common.STORE_EXPRS:
        passed = int(common.ast_mask(expr, table).sum())
        if const is None:
            assert 0.01 * common.N <= passed <= 0.99 * common.N, (expr, passed)
        else:
            assert passed == (common.N if const else 0), (expr, passed)
    many = common.parse(common.STORE_EXPRS[-7][0])
    prog = filter_expr.compile_expr(many, {}, {}, None, common.FIELDS, {"tags": list(common.VOCAB)}, {})
    assert len(prog.array_leaves) == 18 > _lib.RF_ARRAY_MAX_LEAVES               # two rf_array_match launches


def test_array_match_checks_its_arguments_without_a_gpu():
    """Every refusal of rf_array_match comes before any device call."""
    import ctypes
    lib = _lib.load_library()
    INVALID = -1
    M, EL, LEN = _lib.RF_ALEAF_MATCH, _lib.RF_ALEAF_ELEM, _lib.RF_ALEAF_LENGTH

    def leaf(**kw):
        a = (_lib.ArrayLeaf * 17)()
        for l in a:
            l.kind, l.offsets_dev, l.values_dev = LEN, 4096, 4096
        for k, v in kw.items():
            setattr(a[0], k, v)
        return a

    def call(a, n_leaves=1, cs=4096, vs=4096, fs=4096, n_rows=100, out=4096):
        return lib.rf_array_match(a, n_leaves, cs, vs, fs, n_rows, out, None)

    assert call(None) == INVALID and call(leaf(), out=None) == INVALID
    assert call(leaf(), n_leaves=0) == INVALID and call(leaf(), n_leaves=17) == INVALID
    assert call(leaf(), n_rows=-1) == INVALID and call(leaf(), n_rows=1 << 32) == INVALID
    assert call(leaf(), out=4098) == INVALID and call(leaf(), vs=4100) == INVALID and call(leaf(), cs=4097) == INVALID
    assert call(leaf(), fs=4100) == INVALID
    assert call(leaf(kind=0)) == INVALID and call(leaf(kind=4)) == INVALID
    assert call(leaf(kind=EL, elem=0)) == INVALID and call(leaf(kind=EL, elem=5)) == INVALID
    assert call(leaf(kind=M, elem=0, need=1)) == INVALID and call(leaf(kind=M, elem=4, need=1)) == INVALID
    assert call(leaf(offsets_dev=None)) == INVALID and call(leaf(offsets_dev=4100)) == INVALID
    assert call(leaf(kind=EL, elem=_lib.RF_CLEAF_I64_RANGE, values_dev=None)) == INVALID
    assert call(leaf(kind=M, elem=_lib.RF_AELEM_I64, need=1, values_dev=None)) == INVALID
    assert call(leaf(kind=M, elem=_lib.RF_AELEM_I64, need=1, values_dev=4100)) == INVALID
    assert call(leaf(kind=M, elem=_lib.RF_AELEM_CODE, need=1, values_dev=4098)) == INVALID
    for kw in ({"off": -1}, {"len": -1}, {"index": -1}):
        assert call(leaf(kind=EL, elem=_lib.RF_CLEAF_I64_RANGE, **kw)) == INVALID
        assert call(leaf(kind=M, elem=_lib.RF_AELEM_I64, need=1, **kw)) == INVALID
    for need, ln in ((2, 3), (0, 3), (65, 65), (-1, 3), (3, 2)):
        assert call(leaf(kind=M, elem=_lib.RF_AELEM_I64, need=need, len=ln)) == INVALID
    assert call(leaf(kind=M, elem=_lib.RF_AELEM_I64, need=1, len=65537)) == INVALID
    assert call(leaf(kind=EL, elem=_lib.RF_CLEAF_I64_SET, len=65537)) == INVALID
    assert call(leaf(kind=EL, elem=_lib.RF_CLEAF_F64_RANGE, flags=4)) == INVALID
    assert call(leaf(kind=M, elem=_lib.RF_AELEM_I64, need=1, len=1), vs=None) == INVALID
    assert call(leaf(kind=M, elem=_lib.RF_AELEM_CODE, need=1, len=1), vs=None) == INVALID
    assert call(leaf(kind=M, elem=_lib.RF_AELEM_F64, need=1, len=1), fs=None) == INVALID
    assert call(leaf(kind=EL, elem=_lib.RF_CLEAF_CODESET, len=1), cs=None) == INVALID
    assert call(leaf(kind=EL, elem=_lib.RF_CLEAF_I64_SET, len=1), vs=None) == INVALID
    assert b"rf_array_match" in lib.rf_last_error()
    assert call(leaf(), n_rows=0) == 0 and call(leaf(values_dev=None), n_rows=0) == 0   # nothing to write: no launch
    assert call(leaf(kind=M, elem=_lib.RF_AELEM_I64, need=64, len=64), n_rows=0) == 0
    assert ctypes.sizeof(_lib.ArrayLeaf) == 88
