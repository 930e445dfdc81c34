"""User-defined scalar fields on the CPU: the schema's refusals, the value checks of an insert, what the
expression parser and compiler accept and refuse for the four types, the INT64 literal normalisation, the
compiled program interpreted in numpy against a row-by-row evaluation of the AST (a hypothesis property
included), mutation and save / load on a CPU double of GpuIndex, and the upper layers' plumbing.  The device
side (rf_column_match, the filter buffer, the searches) is covered by tests/test_extra_fields_gpu.py."""
import json
import math
import os

import numpy as np
import pytest
import torch
from hypothesis import given, settings, strategies as hs

from oracle import filter_program as ofp, search as osearch
from rag_fin_amd import _lib, filter_expr, schema, service
from rag_fin_amd.schema import DataType, FieldSchema
from rag_fin_amd.store import CorpusStore

GOLD_STORE = os.path.join(os.path.dirname(__file__), "golden", "store_v1")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

FIELDS = [FieldSchema("bank", DataType.VARCHAR), FieldSchema("fiscal_year", DataType.INT64, default=2024),
          FieldSchema("audited", DataType.BOOL, default=False), FieldSchema("weight", DataType.DOUBLE, default=1.0)]


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


def rows(keys, seed=0):
    n = len(keys)
    v = np.random.default_rng(seed).normal(size=(n, 32)).astype(np.float32)
    return [list(keys), [f"text {k}" for k in keys], v, ["Q1_FY2024"] * n, ["c"] * n, ["s"] * n, [float(i) for i in range(n)]]


def extras(n, base=0):
    return {"bank": [("ICICI", "HDFC", "SBI")[(base + i) % 3] for i in range(n)],
            "fiscal_year": [2019 + (base + i) % 7 for i in range(n)],
            "audited": [(base + i) % 2 == 0 for i in range(n)],
            "weight": [0.5 * (base + i) for i in range(n)]}


# ---- schema ------------------------------------------------------------------------------------------
def test_field_schema_and_data_types():
    f = FieldSchema("bank", DataType.VARCHAR)
    assert (f.name, f.dtype, f.default) == ("bank", DataType.VARCHAR, None)
    assert FieldSchema("y", "int64", 3).dtype == DataType.INT64
    assert FieldSchema.from_dict(FieldSchema("w", DataType.DOUBLE, 2).to_dict()) == FieldSchema("w", DataType.DOUBLE, 2.0)
    assert [t.name for t in DataType] == ["BOOL", "INT64", "DOUBLE", "VARCHAR"]
    st = HostStore(fields=FIELDS)
    assert list(st.schema) == FIELDS and HostStore().schema == ()
    assert list(st.columns)[-4:] == ["bank", "fiscal_year", "audited", "weight"]


@pytest.mark.parametrize("make, match", [
    (lambda: FieldSchema("2x", DataType.INT64), "not an identifier"),
    (lambda: FieldSchema("a b", DataType.INT64), "not an identifier"),
    (lambda: FieldSchema("and", DataType.INT64), "expression grammar"),
    (lambda: FieldSchema("x", 101), "not supported"),          # pymilvus' FLOAT_VECTOR
    (lambda: FieldSchema("x", "JSON"), "not supported"),
    (lambda: FieldSchema("x", DataType.INT64, default="1"), "is INT64"),
    (lambda: FieldSchema("x", DataType.INT64, default=True), "is INT64"),
    (lambda: FieldSchema("x", DataType.BOOL, default=1), "is BOOL"),
    (lambda: FieldSchema("x", DataType.INT64, default=1 << 63), "int64 range"),
    (lambda: HostStore(fields=[FieldSchema("period", DataType.VARCHAR)]), "collides"),
    (lambda: HostStore(fields=[FieldSchema("id", DataType.INT64)]), "collides"),
    (lambda: HostStore(fields=[FieldSchema("embedding", DataType.DOUBLE)]), "collides"),
    (lambda: HostStore(fields=[FieldSchema("sparse", DataType.VARCHAR)]), "collides"),
    (lambda: HostStore(fields=[FieldSchema("sparse_embedding", DataType.VARCHAR)]), "collides"),
    (lambda: HostStore(fields=[FieldSchema("token_embeddings", DataType.VARCHAR)]), "collides"),
    (lambda: HostStore(fields=[FieldSchema("a", DataType.INT64), FieldSchema("a", DataType.BOOL)]), "twice"),
    (lambda: HostStore(fields=[FieldSchema(f"f{i}", DataType.INT64) for i in range(33)]), "at most 32"),
    (lambda: HostStore(fields=["bank"]), "FieldSchema"),
])
def test_schema_refusals(make, match):
    with pytest.raises(ValueError, match=match):
        make()


def test_thirty_two_fields_are_taken():
    assert len(HostStore(fields=[FieldSchema(f"f{i}", DataType.INT64) for i in range(32)]).schema) == 32


def test_sharded_store_refuses_fields():
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    with pytest.raises(NotImplementedError, match="fields"):
        ShardedCorpusStore("t", dim=32, fields=FIELDS)


# ---- ingest and mutation -----------------------------------------------------------------------------
def test_add_insert_defaults_and_output_fields():
    st = HostStore(fields=FIELDS)
    d = rows(["a", "b", "c"])
    st.add(d[0], d[1], d[2], *d[3:], extra=extras(3))
    st.insert(rows(["d", "e"], 1) + [["AXIS", "DBS"], [I64_MIN, I64_MAX], [True, False], [float("nan"), float("inf")]])
    st.add(["f"], ["t"], rows(["f"], 2)[2], ["Q2"], ["c"], ["s"], [0.0], extra={"bank": ["KOTAK"]})   # the defaults
    assert st.columns["bank"] == ["ICICI", "HDFC", "SBI", "AXIS", "DBS", "KOTAK"]
    assert st.columns["fiscal_year"] == [2019, 2020, 2021, I64_MIN, I64_MAX, 2024]
    assert st.columns["audited"] == [True, False, True, True, False, False]
    assert st.columns["weight"][:3] == [0.0, 0.5, 1.0] and math.isnan(st.columns["weight"][3]) and st.columns["weight"][5] == 1.0
    got = st.query(expr='id in ["e", "a"]', output_fields=["bank", "fiscal_year", "audited", "weight"])
    assert got == [{"bank": "DBS", "fiscal_year": I64_MAX, "audited": False, "weight": float("inf"), "id": "e"},
                   {"bank": "ICICI", "fiscal_year": 2019, "audited": True, "weight": 0.0, "id": "a"}]
    assert [r["id"] for r in st.query(expr="fiscal_year >= 2021 and audited == false")] == ["e", "f"]
    with pytest.raises(KeyError):
        st.query(expr="", output_fields=["branch"])


@pytest.mark.parametrize("extra, match", [
    ({"fiscal_year": [1, 2]}, "'bank' has no default"),
    ({"bank": ["a", "b"], "branch": [1, 2]}, "unknown extra field 'branch'"),
    ({"bank": ["a"]}, "differ in length"),
    ({"bank": ["a", 3]}, "is VARCHAR"),
    ({"bank": ["a", "b"], "fiscal_year": [1, 2.0]}, "is INT64"),
    ({"bank": ["a", "b"], "fiscal_year": [1, True]}, "is INT64"),
    ({"bank": ["a", "b"], "fiscal_year": [1, 1 << 63]}, "int64 range"),
    ({"bank": ["a", "b"], "fiscal_year": [1, -(1 << 63) - 1]}, "int64 range"),
    ({"bank": ["a", "b"], "audited": [True, 1]}, "is BOOL"),
    ({"bank": ["a", "b"], "weight": [1.0, "x"]}, "is DOUBLE"),
    ({"bank": ["a", "b"], "weight": [1.0, True]}, "is DOUBLE"),
])
def test_value_checks_are_made_before_anything_changes(extra, match):
    st = HostStore(fields=FIELDS)
    d = rows(["a"])
    st.add(d[0], d[1], d[2], *d[3:], extra=extras(1))
    d = rows(["b", "c"], 1)
    with pytest.raises(ValueError, match=match):
        st.add(d[0], d[1], d[2], *d[3:], extra=extra)
    if set(extra) <= {f.name for f in FIELDS} and all(len(c) == 2 for c in extra.values()):
        with pytest.raises(ValueError, match=match):
            st.upsert(rows(["a", "c"], 1) + [extra.get(f.name) for f in FIELDS])
    assert st.num_entities == 1 and st.index.size == 1 and {f: len(c) for f, c in st.columns.items()} == dict.fromkeys(st.columns, 1)
    assert st.columns["bank"] == ["ICICI"]


def test_column_counts():
    st = HostStore(fields=FIELDS)
    with pytest.raises(ValueError, match="expects 11 columns.*primary_value, bank, fiscal_year, audited, weight"):
        st.insert(rows(["a"]))
    with pytest.raises(ValueError, match="expects 11 columns"):
        st.upsert(rows(["a"]) + [["x"]])
    with pytest.raises(ValueError, match="expects 7 columns"):
        HostStore().insert(rows(["a"]) + [["x"]])
    with pytest.raises(ValueError, match="unknown extra field"):
        d = rows(["a"])
        HostStore().add(d[0], d[1], d[2], *d[3:], extra={"bank": ["x"]})


def test_delete_upsert_drop_and_growth_carry_the_columns():
    st = HostStore(capacity=4, fields=FIELDS)
    keys = [f"k{i}" for i in range(40)]
    x = extras(40)
    st.insert(rows(keys) + [x[f.name] for f in FIELDS])                 # grows past the capacity
    assert st.delete("fiscal_year < 2021").delete_count == sum(y < 2021 for y in x["fiscal_year"])
    keep = [i for i in range(40) if x["fiscal_year"][i] >= 2021]
    for f in FIELDS:
        assert st.columns[f.name] == [x[f.name][i] for i in keep]
    st.upsert(rows(["k2", "new"], 3) + [["AXIS", "AXIS"], [1999, 2000], [True, True], [9.0, 9.5]])
    assert st.columns["id"][-2:] == ["k2", "new"] and st.columns["bank"][-2:] == ["AXIS", "AXIS"]
    assert st.columns["id"].count("k2") == 1 and st.num_entities == len(keep) + 1 == st.index.size
    assert [r["id"] for r in st.query(expr='bank == "AXIS" and fiscal_year in [2000, 1999]')] == ["k2", "new"]
    assert st.delete('bank like "AX%"').delete_count == 2
    st.drop()
    assert all(len(c) == 0 for c in st.columns.values()) and list(st.schema) == FIELDS
    st.insert(rows(["z"]) + [["B"], [1], [True], [0.0]])
    assert st.query(expr="audited == true", output_fields=["bank"]) == [{"bank": "B", "id": "z"}]


def test_save_load_round_trip_and_old_directories(tmp_path):
    st = HostStore(fields=FIELDS)
    st.insert(rows(["a", "b", "c"]) + [["X", "Y", "X"], [I64_MIN, 0, I64_MAX], [True, False, True],
                                        [float("nan"), float("-inf"), -0.0]])
    st.save(str(tmp_path / "s"))
    meta = json.load(open(tmp_path / "s" / "columns.json"))
    assert meta["fields"] == [f.to_dict() for f in FIELDS] and meta["columns"]["fiscal_year"] == [I64_MIN, 0, I64_MAX]
    back = HostStore.load_from(str(tmp_path / "s"))
    assert list(back.schema) == FIELDS
    for f in ("id", "bank", "fiscal_year", "audited"):
        assert back.columns[f] == st.columns[f]
    w = back.columns["weight"]
    assert math.isnan(w[0]) and w[1] == float("-inf") and w[2] == 0.0 and math.copysign(1, w[2]) == -1
    assert np.array_equal(back.index.rows, st.index.rows)
    # a store without fields of its own writes no "fields" key, and a directory without it loads without extras
    HostStore().save(str(tmp_path / "p"))
    assert "fields" not in json.load(open(tmp_path / "p" / "columns.json"))
    old = HostStore.load_from(GOLD_STORE)
    assert old.schema == () and old.num_entities == 5 and list(old.columns) == list(HostStore().columns)


# ---- expressions: what parses, what is refused and where ------------------------------------------------
def test_defaults_reproduce_the_store_without_fields():
    with pytest.raises(ValueError, match=r"unknown field 'bank': 'bank' at position 0"):
        filter_expr.parse('bank == "ICICI"')
    with pytest.raises(ValueError, match=r"unknown field 'fiscal_year'"):
        filter_expr.compile_expr('period == "Q1" and fiscal_year > 3', {"period": ["Q1"]}, {})
    p = filter_expr.compile_expr('period == "Q1" and primary_value > 3', {"period": ["Q1"]}, {})
    assert p.column_leaves == [] and [o[0] for o in p.ops] == [_lib.RF_FOP_CODESET, _lib.RF_FOP_RANGE, _lib.RF_FOP_AND]


@pytest.mark.parametrize("expr, match", [
    ('branch == "x"', r"unknown field 'branch': 'branch' at position 0"),
    ("bank == 3", r"bank is VARCHAR, the literal is not a string: '3' at position 8"),
    ("bank == true", r"bank is VARCHAR.*'true' at position 8"),
    ('fiscal_year == "2024"', r"fiscal_year is INT64, the literal is a string: '\"2024\"' at position 15"),
    ("fiscal_year == true", r"fiscal_year is INT64, the literal is a boolean: 'true' at position 15"),
    ("fiscal_year > 9223372036854775808", r"outside the int64 range: '9223372036854775808' at position 14"),
    ("fiscal_year < -9223372036854775809", r"outside the int64 range: '-' at position 14"),
    ("fiscal_year in [1, 9223372036854775808]", r"outside the int64 range: '9223372036854775808' at position 19"),
    ("fiscal_year > 1e999", r"fiscal_year is INT64, the literal is not finite: '1e999' at position 14"),
    ("fiscal_year like \"2%\"", r"'like' needs a VARCHAR field, 'fiscal_year' is not one: 'like' at position 12"),
    ("audited == 1", r"audited is BOOL, the literal is not true or false: '1' at position 11"),
    ('audited == "true"', r"audited is BOOL"),
    ("audited > false", r"a BOOL field supports == != in / not in only, not '>': '>' at position 8"),
    ('weight == "x"', r"weight is DOUBLE, the literal is a string"),
    ("weight == true", r"weight is DOUBLE, the literal is a boolean: 'true' at position 10"),
    ("fiscal_year + 1 > 2024", r"arithmetic is not supported\): '\+' at position 12"),
    ("fiscal_year > 2023 + 1", r"arithmetic is not supported\): '\+' at position 19"),
    ("fiscal_year == weight", r"a field compared with a field is not supported\): 'weight' at position 15"),
    ("bank[0] == \"x\"", r"ARRAY and JSON fields are not supported\): '\[' at position 4"),
    ('json_contains(bank, "x")', r"ARRAY and JSON fields are not supported\): 'json_contains' at position 0"),
    ('array_length(bank) > 1', r"ARRAY and JSON fields are not supported\): 'array_length' at position 0"),
    ("primary_value == true", r"primary_value is DOUBLE, the literal is a boolean"),
    ('TEXT_MATCH(bank, "x")', r"takes the field 'text' only, not 'bank'"),
])
def test_refusals_name_the_token_and_its_position(expr, match):
    with pytest.raises(ValueError, match=match):
        filter_expr.parse(expr, schema=FIELDS)


def test_boolean_literals_are_case_insensitive():
    for text in ("audited == true", "audited == TRUE", "True == audited", "audited in [true]", "not audited != True"):
        node = filter_expr.parse(text, schema=FIELDS)
        assert node.eval({"audited": True}) and not node.eval({"audited": False}), text
    assert filter_expr.parse("audited != false", schema=FIELDS).eval({"audited": True})


# ---- the INT64 literal normalisation --------------------------------------------------------------------
FULL = (I64_MIN, I64_MAX)
TWO63 = "9.223372036854775808e18"   # 2^63 as a float literal


@pytest.mark.parametrize("op, lit, want", [
    ("==", "5", (5, 5)), ("==", "2.5", None), ("==", "2.0", (2, 2)), ("==", "-0.0", (0, 0)),
    (">", "2.5", (3, I64_MAX)), (">=", "2.5", (3, I64_MAX)), ("<", "2.5", (I64_MIN, 2)), ("<=", "2.5", (I64_MIN, 2)),
    (">", "2.0", (3, I64_MAX)), (">=", "2.0", (2, I64_MAX)), ("<", "2.0", (I64_MIN, 1)), ("<=", "2.0", (I64_MIN, 2)),
    (">", "-2.5", (-2, I64_MAX)), (">=", "-2.5", (-2, I64_MAX)), ("<", "-2.5", (I64_MIN, -3)), ("<=", "-2.5", (I64_MIN, -3)),
    (">", "2024", (2025, I64_MAX)), ("<", "2024", (I64_MIN, 2023)),
    ("==", str(I64_MAX), (I64_MAX, I64_MAX)), ("==", str(I64_MIN), (I64_MIN, I64_MIN)),
    (">", str(I64_MAX), None), (">=", str(I64_MAX), (I64_MAX, I64_MAX)), ("<=", str(I64_MAX), FULL),
    ("<", str(I64_MIN), None), ("<=", str(I64_MIN), (I64_MIN, I64_MIN)), (">=", str(I64_MIN), FULL),
    (">", "1e30", None), ("<", "1e30", FULL), ("==", "1e30", None), ("<", "-1e30", None), (">", "-1e30", FULL),
    ("==", TWO63, None), ("<", TWO63, FULL), (">=", TWO63, None), (">=", "-" + TWO63, FULL), ("<", "-" + TWO63, None),
    ("==", "9007199254740993", (9007199254740993, 9007199254740993)),   # 2^53 + 1: an integer literal stays exact
])
def test_int64_comparisons_become_inclusive_intervals(op, lit, want):
    prog = filter_expr.compile_expr(f"fiscal_year {op} {lit}", {}, {}, None, FIELDS, {})
    if want is None:
        assert prog.column_leaves == [] and prog.ops == [(_lib.RF_FOP_FALSE, 0, 0, 0, 0, 0.0, 0.0)]
    else:
        assert prog.column_leaves == [("irange", "fiscal_year") + want]
        assert prog.ops == [(_lib.RF_FOP_BITMAP, filter_expr.COLUMN_LEAF, 0, 0, 0, 0.0, 0.0)]
    # the flipped form, and != as the negation of ==
    flipped = filter_expr.compile_expr(f"{lit} {filter_expr._FLIP[op]} fiscal_year", {}, {}, None, FIELDS, {})
    assert flipped.column_leaves == prog.column_leaves
    if op == "==":
        ne = filter_expr.compile_expr(f"fiscal_year != {lit}", {}, {}, None, FIELDS, {})
        assert ne.column_leaves == prog.column_leaves and ne.ops == prog.ops + [(_lib.RF_FOP_NOT, 0, 0, 0, 0, 0.0, 0.0)]


def test_int64_chains_and_sets():
    c = lambda e: filter_expr.compile_expr(e, {}, {}, None, FIELDS, {})   # noqa: E731
    assert c("2019 <= fiscal_year < 2024").column_leaves == [("irange", "fiscal_year", 2019, I64_MAX),
                                                              ("irange", "fiscal_year", I64_MIN, 2023)]
    assert c("fiscal_year in [3, 1, 2.0, 2.5, 3, 1]").column_leaves == [("iset", "fiscal_year", [1, 2, 3])]
    assert c(f"fiscal_year in [{I64_MAX}, {I64_MIN}]").column_leaves == [("iset", "fiscal_year", [I64_MIN, I64_MAX])]
    assert [o[0] for o in c("fiscal_year not in [7]").ops] == [_lib.RF_FOP_BITMAP, _lib.RF_FOP_NOT]
    assert [o[0] for o in c("fiscal_year in []").ops] == [_lib.RF_FOP_FALSE]
    assert [o[0] for o in c("fiscal_year not in [2.5]").ops] == [_lib.RF_FOP_FALSE, _lib.RF_FOP_NOT]
    assert [o[0] for o in c("fiscal_year in [1e30, -1e30, 2.5]").ops] == [_lib.RF_FOP_FALSE]     # no int64 equals them
    assert c(f"fiscal_year in [1e30, 4.0, {TWO63}]").column_leaves == [("iset", "fiscal_year", [4])]


def test_int64_in_takes_65536_distinct_values_and_no_more():
    many = ", ".join(str(3 * i - 70000) for i in range(65536))
    prog = filter_expr.compile_expr(f"fiscal_year in [{many}, -70000, -69997]", {}, {}, None, FIELDS, {})
    (leaf,) = prog.column_leaves
    assert leaf[0] == "iset" and len(leaf[2]) == 65536 and leaf[2] == sorted(leaf[2]) and leaf[2][0] == -70000
    arr, words, values = filter_expr.column_leaf_arrays(prog, {"fiscal_year": 4096})
    assert (arr[0].kind, arr[0].off, arr[0].len, arr[0].column_dev) == (_lib.RF_CLEAF_I64_SET, 0, 65536, 4096)
    assert values.dtype == np.int64 and values.size == 65536 and words.size == 0
    for neg in ("", "not "):
        with pytest.raises(ValueError, match="65537 distinct values, at most 65536"):
            filter_expr.compile_expr(f"fiscal_year {neg}in [{many}, 1]", {}, {}, None, FIELDS, {})


# ---- the compiled program in numpy == the AST, row by row -----------------------------------------------
def host_table(n, seed):
    rng = np.random.default_rng(seed)
    ints = np.concatenate([[I64_MIN, I64_MAX, 0, -1, 2024], rng.integers(2015, 2030, size=n)])[:n]
    dbl = rng.normal(size=n).round(1)
    dbl[::7] = np.nan
    dbl[3::11] = np.inf
    dbl[5::13] = -0.0
    return {
        "id": [f"k{i}" for i in range(n)],
        "period": [("Q1_FY2024", "Q2_FY2024", "Q3_FY2024", "")[i] for i in rng.integers(4, size=n)],
        "chunk_type": [("balance_sheet", "key_ratios", "segment")[i] for i in rng.integers(3, size=n)],
        "statement_type": [("consolidated", "standalone")[i] for i in rng.integers(2, size=n)],
        "primary_value": [float(v) for v in rng.normal(size=n).round(1)],
        "bank": [("ICICI", "HDFC", "SBI", "AXIS", "")[i] for i in rng.integers(5, size=n)],
        "fiscal_year": [int(v) for v in ints],
        "audited": [bool(v) for v in rng.integers(2, size=n)],
        "weight": [float(v) for v in dbl],
    }


def encode(values):
    d, code = [], {}
    out = np.array([code.setdefault(v, len(code)) for v in values], dtype=np.int32)
    for v in code:
        d.append(v)
    return d, out


def run_compiled(expr, table):
    """compile_expr's output interpreted in numpy: the column leaves' bitmaps from their definition, then the
    postfix program by oracle/filter_program.py."""
    n = len(table["id"])
    dicts, codes = {}, {}
    for c, f in enumerate(filter_expr.VARCHAR_FIELDS):
        dicts[f], codes[c] = encode(table[f])
    xd, xcol = {}, {}
    for f in FIELDS:
        if f.dtype in (DataType.VARCHAR, DataType.BOOL):
            xd[f.name], xcol[f.name] = encode(table[f.name])
        else:
            xcol[f.name] = np.array(table[f.name], dtype=np.int64 if f.dtype == DataType.INT64 else np.float64)
    prog = filter_expr.compile_expr(filter_expr.parse(expr, schema=FIELDS), dicts, {k: i for i, k in enumerate(table["id"])},
                                    None, FIELDS, xd)
    nwords = (n + 31) // 32
    bitmaps = np.concatenate([ofp.pack_rows(filter_expr.column_leaf_reference(leaf, xcol[leaf[1]]))
                              for leaf in prog.column_leaves] + [np.zeros(0, np.uint32)])
    assert bitmaps.size == len(prog.column_leaves) * nwords
    ops = prog.resolved_ops(0, 0, nwords)
    assert all(o[1] == 0 and o[3] == nwords and o[2] % nwords == 0 for o in ops if o[0] == _lib.RF_FOP_BITMAP)
    return ofp.run_ops(ops, prog.code_sets, prog.row_lists, bitmaps, codes, np.array(table["primary_value"]), n), prog


def run_ast(expr, table):
    node = filter_expr.parse(expr, schema=FIELDS)
    n = len(table["id"])
    return np.array([node.eval({f: c[r] for f, c in table.items()}) for r in range(n)], dtype=bool)


TABLE = host_table(333, 1)

EXPRS = [
    'bank == "ICICI"', 'bank != "ICICI"', 'bank > "HDFC"', 'bank <= "ICICI"', 'bank in ["SBI", "AXIS", "none"]',
    'bank not in ["SBI"]', 'bank like "IC%"', 'bank like "%I"', 'bank like "%D%"', 'bank == "none"', 'bank == ""',
    "audited == true", "audited != true", "audited == false", "audited in [true, false]", "audited not in [false]",
    "fiscal_year == 2024", "fiscal_year != 2024", "fiscal_year > 2023.5", "2019 <= fiscal_year < 2024",
    f"fiscal_year == {I64_MIN}", f"fiscal_year >= {I64_MAX}", "fiscal_year in [2016, 2024, 1]", "fiscal_year not in [2016, 0]",
    "fiscal_year == 2.5", "fiscal_year != 2.5", "fiscal_year < -1e30", "fiscal_year in [2020.0, 2020.5]",
    "weight > 0", "weight != 0", "weight == 0", "weight in [0.1, -0.3]", "weight not in [0.1]", "-1 < weight <= 0.5",
    "weight < 1 or weight >= 1", "weight == 1e999",
    'bank == "ICICI" and fiscal_year >= 2024', 'period == "Q1_FY2024" and bank != "SBI" or not audited == true',
    'not (fiscal_year in [2020, 2021] or weight < 0) and primary_value > 0 and chunk_type like "%ratio%"',
    'id in ["k3", "k77", "zz"] or (audited == false and statement_type == "standalone" and bank < "I")',
]


@pytest.mark.parametrize("expr", EXPRS)
def test_compiled_program_equals_the_ast(expr):
    got, _ = run_compiled(expr, TABLE)
    assert np.array_equal(got, run_ast(expr, TABLE))


def test_a_copied_period_column_compiles_to_the_built_in_code_set():
    """The same predicate over `period` and over an extra VARCHAR copy of it selects the same codes."""
    table = dict(TABLE, bank=list(TABLE["period"]))
    a, pa = run_compiled('period in ["Q1_FY2024", ""]', table)
    b, pb = run_compiled('bank in ["Q1_FY2024", ""]', table)
    assert np.array_equal(a, b) and pb.column_leaves == [("codeset", "bank", pa.code_sets)]


# hypothesis: random expressions over built-in and extra leaves.  At most 6 leaves of at most 7 operations each
# (a DOUBLE `not in` of 3 values: 3 leaves, 2 ORs, 1 NOT... ), 5 connectives and a NOT per node: below
# RF_FILTER_MAX_OPS = 64 and far below the depth limit by construction, so nothing is discarded.
_STR = lambda vs: hs.sampled_from(vs).map(json.dumps)   # noqa: E731
_CMP = hs.sampled_from(["==", "!=", "<", "<=", ">", ">="])
_INTS = hs.one_of(hs.integers(2014, 2031), hs.sampled_from([I64_MIN, I64_MAX, 0, -1]),
                  hs.sampled_from([2019.5, 2024.0, -0.5, 1e30, -1e30])).map(repr)
_DBLS = hs.sampled_from([0.0, -0.0, 0.1, -0.3, 1.0, 2.5, 1e999, -1e999]).map(lambda v: repr(v).replace("inf", "1e999"))


def _lists(lits):
    return hs.lists(lits, min_size=0, max_size=3).map(lambda v: "[" + ", ".join(v) + "]")


_NEG = hs.sampled_from(["in", "not in"])
LEAVES = hs.one_of(
    hs.tuples(hs.just("bank"), _CMP, _STR(["ICICI", "HDFC", "SBI", "AXIS", "", "none"])).map(" ".join),
    hs.tuples(hs.just("bank"), _NEG, _lists(_STR(["ICICI", "SBI", "none"]))).map(" ".join),
    hs.tuples(hs.just("bank like"), _STR(["IC%", "%I", "%D%", "SBI"])).map(" ".join),
    hs.tuples(hs.just("audited"), hs.sampled_from(["==", "!="]), hs.sampled_from(["true", "false", "TRUE"])).map(" ".join),
    hs.tuples(hs.just("fiscal_year"), _CMP, _INTS).map(" ".join),
    hs.tuples(_INTS, hs.sampled_from(["<", "<="]), hs.just("fiscal_year"), hs.sampled_from(["<", "<="]), _INTS).map(" ".join),
    hs.tuples(hs.just("fiscal_year"), _NEG, _lists(_INTS)).map(" ".join),
    hs.tuples(hs.just("weight"), _CMP, _DBLS).map(" ".join),
    hs.tuples(hs.just("weight"), _NEG, _lists(_DBLS)).map(" ".join),
    hs.tuples(hs.just("period"), _CMP, _STR(["Q1_FY2024", "Q3_FY2024", ""])).map(" ".join),
    hs.tuples(hs.just("chunk_type like"), _STR(["%ratio%", "seg%"])).map(" ".join),
    hs.tuples(hs.just("primary_value"), _CMP, _DBLS).map(" ".join),
    hs.tuples(hs.just("id in"), _lists(_STR(["k0", "k5", "k332", "zz"]))).map(" ".join),
)


@hs.composite
def expressions(draw):
    terms = draw(hs.lists(LEAVES, min_size=1, max_size=6))
    terms = [("not " if draw(hs.booleans()) else "") + "(" + t + ")" for t in terms]
    while len(terms) > 1:   # join two neighbours at a time: every tree shape
        i = draw(hs.integers(0, len(terms) - 2))
        joined = "(" + terms[i] + draw(hs.sampled_from([" and ", " or ", " && ", " || "])) + terms[i + 1] + ")"
        terms[i:i + 2] = [("not " if draw(hs.booleans()) else "") + joined]
    return terms[0]


@settings(max_examples=150, deadline=None)
@given(expressions())
def test_random_expressions_compile_to_what_the_ast_says(expr):
    got, prog = run_compiled(expr, TABLE)
    assert len(prog.ops) <= _lib.RF_FILTER_MAX_OPS and prog.max_depth() <= _lib.RF_FILTER_MAX_DEPTH
    assert np.array_equal(got, run_ast(expr, TABLE)), expr


# ---- upper layers ------------------------------------------------------------------------------------
def test_service_extra_columns_and_ingest():
    chunks = [{"id": f"c{i}", "text": f"chunk {i}", "period": p, "chunk_type": "c", "statement_type": "s",
               "primary_value": 1.0, "page": i} for i, p in enumerate(["Q1_FY2024", "Q3_FY2023"])]
    fields = [FieldSchema("bank", DataType.VARCHAR), FieldSchema("fiscal_year", DataType.INT64),
              FieldSchema("page", DataType.INT64), FieldSchema("audited", DataType.BOOL, default=True)]
    values = {"bank": "ICICI", "fiscal_year": lambda c: 2000 + int(c["period"][-2:])}
    assert service.extra_columns(fields, chunks, values) == {"bank": ["ICICI", "ICICI"], "fiscal_year": [2024, 2023],
                                                             "page": [0, 1]}
    with pytest.raises(ValueError, match="'branch' is not a declared field"):
        service.extra_columns(fields, chunks, {"branch": 1})

    class Emb:
        dim = 32

        def encode_to_device(self, texts):
            return np.random.default_rng(0).normal(size=(len(texts), 32)).astype(np.float32)

    st = HostStore(fields=fields)
    assert service.ingest(st, Emb(), chunks, field_values=values) == 2
    assert st.columns["bank"] == ["ICICI", "ICICI"] and st.columns["fiscal_year"] == [2024, 2023]
    assert st.columns["page"] == [0, 1] and st.columns["audited"] == [True, True]
    with pytest.raises(ValueError, match="no value for the field\\(s\\) bank, fiscal_year"):
        service.ingest(HostStore(fields=fields), Emb(), chunks)
    plain = HostStore()
    assert service.ingest(plain, Emb(), chunks) == 2 and list(plain.columns) == list(HostStore().columns)


def test_vector_rag_extra_output_fields():
    from rag_fin_amd.rag import OUTPUT_FIELDS, VectorRAG
    from rag_fin_amd.store import Hit

    class Emb:
        dim = 32

        def encode(self, texts):
            return np.zeros((len(texts), 32), np.float32)

    class Store:
        schema = tuple(FIELDS)
        num_entities = 1

        def load(self):
            pass

        def search(self, data, anns_field, param, limit, **kw):
            self.kw = kw
            row = {"text": "t", "period": "Q1", "chunk_type": "c", "statement_type": "s", "primary_value": 1.0,
                   "bank": "ICICI", "fiscal_year": 2024}
            return [[Hit(0, "a", 0.5, {f: row[f] for f in kw["output_fields"]})] for _ in range(len(data))]

    st = Store()
    rag = VectorRAG("k", embedder=Emb(), store=st, extra_output_fields=["bank", "fiscal_year"])
    (ctx,) = rag.search("net profit", 1, expr='bank == "ICICI"')
    assert st.kw["output_fields"] == OUTPUT_FIELDS + ["bank", "fiscal_year"] and st.kw["expr"] == 'bank == "ICICI"'
    assert list(ctx) == ["rank", "text", "period", "chunk_type", "statement_type", "primary_value", "score", "bank",
                         "fiscal_year"] and (ctx["bank"], ctx["fiscal_year"]) == ("ICICI", 2024)
    plain = VectorRAG("k", embedder=Emb(), store=st)
    (ctx,) = plain.search("net profit", 1)
    assert st.kw["output_fields"] == OUTPUT_FIELDS
    assert list(ctx) == ["rank", "text", "period", "chunk_type", "statement_type", "primary_value", "score"]
    with pytest.raises(ValueError, match="'branch' is not a field the store declares"):
        VectorRAG("k", embedder=Emb(), store=st, extra_output_fields=["branch"])


def test_micro_batcher_checks_an_expression_against_the_stores_schema():
    from rag_fin_amd.batching import MicroBatcher

    class Rag:
        class collection:
            analyzer = None
            schema = tuple(FIELDS)

        def search_batch(self, queries, top_k, expr=None):
            return [[{"q": q, "expr": e}] for q, e in zip(queries, expr if isinstance(expr, (list, tuple)) else [expr] * len(queries))]

    mb = MicroBatcher(Rag(), max_wait_ms=1.0)
    try:
        assert mb.search("q", 1, expr='bank == "ICICI" and fiscal_year >= 2024')[0]["expr"] == 'bank == "ICICI" and fiscal_year >= 2024'
        with pytest.raises(ValueError, match="unknown field 'branch'"):
            mb.search("q", 1, expr="branch == 1")
    finally:
        mb.close()


def test_column_match_checks_its_arguments_without_a_gpu():
    """Every refusal of rf_column_match comes before any device call."""
    import ctypes
    lib = _lib.load_library()
    INVALID = -1

    def leaf(**kw):
        a = (_lib.ColumnLeaf * 17)()
        for l in a:
            l.kind, l.column_dev = _lib.RF_CLEAF_I64_RANGE, 4096
        for k, v in kw.items():
            setattr(a[0], k, v)
        return a

    def call(a, n_leaves=1, cs=4096, vs=4096, n_rows=100, out=4096):
        return lib.rf_column_match(a, n_leaves, cs, vs, n_rows, out, None)

    assert call(None) == INVALID and call(leaf(), out=None) == INVALID
    assert call(leaf(), n_leaves=0) == INVALID and call(leaf(), n_leaves=17) == INVALID
    assert call(leaf(), n_rows=-1) == INVALID and call(leaf(), n_rows=1 << 32) == INVALID
    assert call(leaf(), out=4098) == INVALID and call(leaf(), vs=4100) == INVALID and call(leaf(), cs=4097) == INVALID
    assert call(leaf(kind=0)) == INVALID and call(leaf(kind=5)) == INVALID
    assert call(leaf(column_dev=None)) == INVALID and call(leaf(column_dev=4100)) == INVALID
    assert call(leaf(kind=_lib.RF_CLEAF_CODESET, column_dev=4098)) == INVALID
    for kind, null in ((_lib.RF_CLEAF_CODESET, {"cs": None}), (_lib.RF_CLEAF_I64_SET, {"vs": None})):
        assert call(leaf(kind=kind, off=-1, len=1)) == INVALID and call(leaf(kind=kind, off=0, len=-1)) == INVALID
        assert call(leaf(kind=kind, off=0, len=1), **null) == INVALID
    assert call(leaf(kind=_lib.RF_CLEAF_I64_SET, len=65537)) == INVALID
    assert call(leaf(kind=_lib.RF_CLEAF_F64_RANGE, flags=4)) == INVALID
    assert b"rf_column_match" in lib.rf_last_error()
    assert call(leaf(), n_rows=0) == 0   # nothing to write: no launch
    assert ctypes.sizeof(_lib.ColumnLeaf) == 64
