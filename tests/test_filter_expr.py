"""Filter expressions on the host: parser, AST semantics, compiled postfix program (CPU only).

The compiled program is run by the numpy interpreter of the device program's semantics
(oracle/filter_program.py; include/ragfin.h, "filtered search") and compared with an evaluator written here, over random
expressions and random columns (duplicate strings, NaN, +-0.0, empty strings)."""
import math

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from oracle.filter_program import run_program
from rag_fin_amd import _lib, filter_expr as fe

STRS = ["", "Q1_FY2024", "Q2_FY2024", "Q1", "a", "ab", "b", "key_ratios", "ratios_key", "Z"]
NUMS = [0.0, -0.0, 1.0, -1.5, 2.5, 3.0, 1e6, float("nan"), float("inf"), float("-inf")]
LITS = [0.0, 1.0, -1.5, 2.5, 3, -3, 1e6]
VARCHAR = ["period", "chunk_type", "statement_type"]


def compile_on(table, expr):
    """Dictionaries in first-seen order, as the store's device mirror builds them."""
    n = len(table["id"])
    dicts, codes = {}, {}
    for j, f in enumerate(VARCHAR):
        d = list(dict.fromkeys(table[f]))
        dicts[f] = d
        pos = {s: i for i, s in enumerate(d)}
        codes[j] = np.array([pos[s] for s in table[f]], dtype=np.int32)
    pk = {k: i for i, k in enumerate(table["id"])}
    prog = fe.compile_expr(expr, dicts, pk)
    return run_program(prog, codes, np.asarray(table["primary_value"], dtype=np.float64), n)


def ast_rows(table, expr):
    node = fe.parse(expr)
    n = len(table["id"])
    return np.array([node.eval({f: table[f][i] for f in table}) for i in range(n)], dtype=bool)


# ---- random expressions with their own evaluator ---------------------------------------------------
def q(s):
    return '"' + s.replace("\\", "\\\\").replace('"', '\\"') + '"'


def num(v):
    return repr(float(v)) if isinstance(v, float) else str(v)


def ieee(x, op, v):
    return {"==": x == v, "!=": x != v, "<": x < v, "<=": x <= v, ">": x > v, ">=": x >= v}[op]


@st.composite
def leaf(draw):
    kind = draw(st.sampled_from(["str_cmp", "str_in", "like", "num_cmp", "num_in", "chain", "rev", "id"]))
    ops = st.sampled_from(["==", "!=", "<", "<=", ">", ">="])
    if kind == "str_cmp":
        f, op, v = draw(st.sampled_from(VARCHAR)), draw(ops), draw(st.sampled_from(STRS + ["missing"]))
        return f"{f} {op} {q(v)}", lambda r: ieee(r[f], op, v)
    if kind == "str_in":
        f, vs, neg = draw(st.sampled_from(VARCHAR)), draw(st.lists(st.sampled_from(STRS), max_size=3)), draw(st.booleans())
        txt = f"{f} {'not in' if neg else 'in'} [{', '.join(q(v) for v in vs)}]"
        return txt, lambda r: (r[f] in vs) != neg
    if kind == "like":
        f, core = draw(st.sampled_from(VARCHAR)), draw(st.sampled_from(["Q1", "key", "_", "a", "ratios"]))
        form = draw(st.integers(0, 2))
        pat = [core + "%", "%" + core, "%" + core + "%"][form]
        fn = [lambda s: s.startswith(core), lambda s: s.endswith(core), lambda s: core in s][form]
        return f"{f} like {q(pat)}", lambda r: fn(r[f])
    if kind == "num_cmp":
        op, v = draw(ops), draw(st.sampled_from(LITS))
        return f"primary_value {op} {num(v)}", lambda r: ieee(r["primary_value"], op, float(v))
    if kind == "num_in":
        vs, neg = draw(st.lists(st.sampled_from(LITS), max_size=3)), draw(st.booleans())
        txt = f"primary_value {'not in' if neg else 'in'} [{', '.join(num(v) for v in vs)}]"
        return txt, lambda r: any(r["primary_value"] == float(v) for v in vs) != neg
    if kind == "chain":
        o1, o2 = draw(st.sampled_from(["<", "<="])), draw(st.sampled_from(["<", "<="]))
        a, b = draw(st.sampled_from(LITS)), draw(st.sampled_from(LITS))
        return (f"{num(a)} {o1} primary_value {o2} {num(b)}",
                lambda r: ieee(float(a), o1, r["primary_value"]) and ieee(r["primary_value"], o2, float(b)))
    if kind == "rev":
        op, v = draw(ops), draw(st.sampled_from(STRS))
        return f"{q(v)} {op} period", lambda r: ieee(v, op, r["period"])
    keys, neg = draw(st.lists(st.sampled_from([0, 1, 5, 17, 40, 99]), max_size=4)), draw(st.booleans())
    if len(keys) == 1 and draw(st.booleans()):
        op = "!=" if neg else "=="
        return f"id {op} {keys[0]}", lambda r: (r["id"] == keys[0]) != neg
    return f"id {'not in' if neg else 'in'} {keys}", lambda r: (r["id"] in keys) != neg


def expr_tree(depth=3):
    base = leaf()
    if depth == 0:
        return base

    @st.composite
    def node(draw):
        kind = draw(st.sampled_from(["leaf", "and", "or", "not"]))
        if kind == "leaf":
            return draw(base)
        if kind == "not":
            t, f = draw(expr_tree(depth - 1))
            word = draw(st.sampled_from(["not ", "!", "NOT "]))
            return f"{word}({t})", lambda r: not f(r)
        (ta, fa), (tb, fb) = draw(expr_tree(depth - 1)), draw(expr_tree(depth - 1))
        word = draw(st.sampled_from(["and", "&&", "AND"] if kind == "and" else ["or", "||", "OR"]))
        if kind == "and":
            return f"({ta}) {word} ({tb})", lambda r: fa(r) and fb(r)
        return f"({ta}) {word} ({tb})", lambda r: fa(r) or fb(r)
    return node()


@st.composite
def table(draw):
    n = draw(st.integers(1, 70))
    cols = {f: draw(st.lists(st.sampled_from(STRS), min_size=n, max_size=n)) for f in VARCHAR}
    cols["primary_value"] = draw(st.lists(st.sampled_from(NUMS), min_size=n, max_size=n))
    cols["id"] = list(range(n))
    cols["text"] = [""] * n
    return cols


@settings(max_examples=300, deadline=None)
@given(table(), expr_tree())
def test_random_expressions_select_the_rows_of_an_independent_evaluator(tab, tree):
    text, fn = tree
    n = len(tab["id"])
    want = np.array([fn({f: tab[f][i] for f in tab}) for i in range(n)], dtype=bool)
    assert np.array_equal(compile_on(tab, text), want), text
    assert np.array_equal(ast_rows(tab, text), want), text


def fixed_table():
    return {"id": [0, 1, 2, 3, 4, 5],
            "period": ["Q1_FY2024", "Q2_FY2024", "Q1_FY2024", "", "Q3_FY2024", "Q2_FY2024"],
            "chunk_type": ["key_ratios", "balance", "pl", "pl", "key_ratios", ""],
            "statement_type": ["c", "s", "c", "c", "s", "s"],
            "primary_value": [1.0, float("nan"), -0.0, 0.0, 5.0, -2.0],
            "text": [""] * 6}


@pytest.mark.parametrize("expr,rows", [
    ('period == "Q1_FY2024"', [0, 2]),
    ("period == 'Q1_FY2024'", [0, 2]),
    ('period == "Q9"', []),                                  # not in the dictionary: matches nothing
    ('period != "Q9"', [0, 1, 2, 3, 4, 5]),
    ('period < "Q2"', [0, 2, 3]),                            # code-point order
    ('chunk_type like "key%"', [0, 4]),
    ('chunk_type like "%a%"', [0, 1, 4]),
    ('chunk_type like "%l"', [2, 3]),
    ("primary_value == 0", [2, 3]),                          # -0.0 == 0.0
    ("primary_value != 1", [1, 2, 3, 4, 5]),                 # NaN != 1 holds
    ("primary_value > -1", [0, 2, 3, 4]),                    # NaN fails
    ("not primary_value > -1", [1, 5]),
    ("-1 < primary_value <= 1", [0, 2, 3]),
    ("primary_value in [5, -2]", [4, 5]),
    ("primary_value not in [5, -2]", [0, 1, 2, 3]),
    ("id in [4, 0, 99]", [0, 4]),
    ("id not in [4, 0]", [1, 2, 3, 5]),
    ("id != 3", [0, 1, 2, 4, 5]),
    ("primary_value in []", []),
    # precedence: not > and > or
    ('period == "Q1_FY2024" or period == "Q2_FY2024" and statement_type == "c"', [0, 2]),
    ('(period == "Q1_FY2024" or period == "Q2_FY2024") and statement_type == "s"', [1, 5]),
    ('not period == "Q1_FY2024" and statement_type == "c"', [3]),
    ('not (period == "Q1_FY2024" and statement_type == "c")', [1, 3, 4, 5]),
    ("!(id == 1) && id != 9 || id == 1", [0, 1, 2, 3, 4, 5]),
    ('period in ["Q1_FY2024"] AND primary_value >= 0 OR NOT chunk_type != ""', [0, 2, 5]),
])
def test_fixed_cases_and_precedence(expr, rows):
    tab = fixed_table()
    assert np.flatnonzero(compile_on(tab, expr)).tolist() == rows
    assert np.flatnonzero(ast_rows(tab, expr)).tolist() == rows


@pytest.mark.parametrize("expr,match", [
    ("", "empty"),
    ("   ", "empty"),
    ("period ==", "literal"),
    ('period == "Q1" and', "field name"),
    ('(period == "Q1"', r"expected '\)'"),
    ('period == "Q1")', "unexpected token"),
    ('period == "Q1', "unterminated"),
    ("period > 3", "VARCHAR"),
    ('primary_value == "x"', "DOUBLE"),
    ('primary_value in [1, "x"]', "DOUBLE"),
    ('text == "a"', "cannot be filtered"),
    ("embedding == 1", "cannot be filtered"),
    ("foo == 1", "unknown field"),
    ("id < 3", "primary key"),
    ('primary_value like "1%"', "VARCHAR"),
    ('period like "a%b"', "like"),
    ("period like 3", "string pattern"),
    ("period in 'a'", r"expected '\['"),
    ("period == 'a' ; drop", "unexpected character"),
    ("period", "comparison"),
    ("3 < 4", "field name"),
])
def test_every_error_class_raises_value_error(expr, match):
    with pytest.raises(ValueError, match=match):
        fe.compile_expr(expr, {f: ["a"] for f in VARCHAR}, {})


def test_error_names_the_position():
    with pytest.raises(ValueError, match="position 17"):
        fe.parse('primary_value == "x"')


def test_program_limits():
    big = " or ".join(f"primary_value == {i}" for i in range(40))
    with pytest.raises(ValueError, match="operations"):
        fe.compile_expr(big, {}, {})
    deep = "".join("(primary_value > 1 and " for _ in range(40)) + "primary_value > 2" + ")" * 40
    with pytest.raises(ValueError):
        fe.compile_expr(deep, {}, {})
    ok = fe.compile_expr("primary_value in [1, 2, 3] and id in [1]", {}, {1: 0})
    assert len(ok.ops) <= _lib.RF_FILTER_MAX_OPS and ok.max_depth() <= _lib.RF_FILTER_MAX_DEPTH


def test_is_empty():
    assert fe.is_empty(None) and fe.is_empty("") and fe.is_empty(" \t\n")
    assert not fe.is_empty("id == 1")


def test_string_escapes_and_numbers():
    node = fe.parse(r'period == "a\"b" and primary_value > -1.5e3 and primary_value < +2')
    assert node.a.a.value == 'a"b' and node.a.b.value == -1500.0 and node.b.value == 2.0
    assert math.isinf(fe.compile_expr("primary_value > 1", {}, {}).ops[0][6])
