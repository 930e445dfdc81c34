"""Boolean filter expressions of filtered search: `CorpusStore.search(..., expr=...)` and
`CorpusStore.query(expr=...)`, the `expr` argument of pymilvus `Collection.search` / `query`.

A Milvus boolean-expression subset over the reference's scalar schema
("chunking_storing (1).py":14-22) is parsed by recursive descent into an AST, then compiled into
the postfix program `rf_filter_eval` runs on the device (include/ragfin.h, "filtered search").

Grammar (keywords case-insensitive; precedence not > and > or)::

    expr    := and_ (("or" | "||") and_)*
    and_    := unary (("and" | "&&") unary)*
    unary   := ("not" | "!") unary | "(" expr ")" | compare
    compare := FIELD CMP literal | literal CMP FIELD [CMP literal]
             | "exists" FIELD                       (dynamic fields only; there FIELD is also NAME | $meta[STRING])
             | FIELD ["not"] "in" "[" [literal ("," literal)*] "]" | FIELD "like" STRING
             | FUNC "(" "text" "," STRING ["," (NAME "=" NUM | NUM)] ")"
             | "ARRAY_CONTAINS" "(" F "," literal ")"                  (F: a declared ARRAY field; function names
             | ("ARRAY_CONTAINS_ALL" | "ARRAY_CONTAINS_ANY") "(" F "," "[" [literal ("," literal)*] "]" ")"
             | "ARRAY_LENGTH" "(" F ")" CMP INT | INT CMP "ARRAY_LENGTH" "(" F ")" [CMP INT]     case-insensitive)
             | F "[" INT "]" wherever a scalar FIELD of F's element type stands
    FUNC    := "TEXT_MATCH" | "PHRASE_MATCH"

Fields and what they accept:
  period, chunk_type, statement_type (VARCHAR)  == != < <= > >= (code-point order), in / not in,
                                                like "p%" / "%s" / "%i%" (no other wildcard)
  primary_value (DOUBLE)                        == != < <= > >= (chains such as 1 < x <= 5),
                                                in / not in; IEEE semantics: NaN fails every
                                                comparison except !=
  id (primary key)                              == != in / not in
  text (VARCHAR with the lexical index)         TEXT_MATCH(text, 'terms' [, minimum_should_match=N]),
                                                PHRASE_MATCH(text, 'a b c' [, slop=0]); nothing else
Keyword filters (Milvus TEXT_MATCH / PHRASE_MATCH).  The terms of a string are those of
the analyzer the caller gives `parse` (the store's), else `lexical.analyze`: punctuation characters
are terms of their own, so 'Q1_FY2024' is the three terms q1, _, fy2024.
  TEXT_MATCH    Q = the distinct terms of the string; a row passes iff it holds at least N of them
                (N an integer >= 1, default 1 = OR).  N > |Q| and an empty Q pass no row; more than
                64 distinct terms raise ValueError.
  PHRASE_MATCH  p_0 .. p_{m-1} = the terms in order (repeats allowed, m <= 64); a row with the term
                sequence d passes iff some j has d[j + i] == p_i for every i.  Only slop 0 (exact
                adjacency) is offered; m = 0 passes no row.
Both need the lexical index (create_index("sparse", ...)): compiling one without it raises ValueError.
String literals take single or double quotes (backslash escapes the next character).  Anything
else -- an unknown field, `embedding`, `text` outside the two functions, a type mismatch such as `period > 3` or
`primary_value == "x"`, a syntax error -- raises ValueError naming the token and its position.

Dynamic fields (`parse(..., dynamic=True)`, what a store with enable_dynamic_field=True passes; pymilvus'
`$meta`).  A dynamic operand stands wherever a scalar field does: a bare identifier that is no field of the
collection, no reserved name and no word of the grammar, or `$meta["any key"]` (single or double quotes).  It
takes == != < <= > >= (literal-first and chained forms included), in / not in (at most RF_COLUMN_MAX_SET values
of one type class), like, and `exists KEY`.  A row holds under a key a bool, an int (int64), a float or a str,
or lacks the key.  The semantics below are THIS PROJECT'S definition (Milvus leaves mixed types to its JSON
engine), written once as the `eval` of DynCmp / DynIn / DynLike / Exists and, for the compiled leaves, as
`dynamic_leaf_reference`:
  * three type classes: string, number (int and float together), boolean;
  * a comparison leaf passes a row iff the row holds the key, the value's class is the literal's class, and the
    comparison holds: strings in code-point order; numbers as Python compares them -- an int against a float
    exactly, not "both to double" (2**53 + 1 > 2.0**53 holds, 3 == 3.0 holds); floats by IEEE, so a NaN row
    fails everything except !=; booleans take == != in / not in only;
  * a row that lacks the key, or holds a value of another class, fails EVERY leaf, `!=` and `not in` included
    (as an SQL NULL would); `k in []` and `k not in []` name no class and pass no row;
  * `not (...)` is plain negation, as everywhere in the grammar, so `not (k == 1)` passes the rows that lack k;
  * `exists k` passes iff the row holds k;
  * a key that no row holds is no error: its leaves are FALSE.
A dynamic leaf compiles into entries of `Program.dynamic_leaves`, which rf_dynamic_match evaluates over the
key's tagged column (tag uint8, payload 8 bytes; `encode_dynamic`) into row bitmaps: TAGS (the tag is in a
mask: `exists`, and the class guard of a numeric `!=` / `not in`, which is TAGS(number) and not EQ), STR_CODESET
(the leaf evaluated against the key's dictionary, as a VARCHAR leaf), BOOL, NUM_RANGE (an int64 interval for the
int rows and an fp64 interval for the float rows, both derived exactly from the one literal: `int_interval` and
`f64_interval`) and NUM_SET (a sorted int64 set and a sorted fp64 set).

ARRAY fields (a FieldSchema of DataType.ARRAY in `schema`: a row holds a list of 0 .. max_capacity elements of one
of the four scalar types).  The semantics below are THIS PROJECT'S definition, written once as the `eval` of
ArrContains / ArrLength / ArrElem and, for the compiled leaves, as `array_leaf_reference`:
  * ARRAY_CONTAINS(F, v): some element equals v -- strings by equality, int64 exactly, booleans by equality,
    doubles by IEEE == (a NaN element is never contained, -0.0 contains 0.0).  Literals are typed by the element
    type as a scalar field's are (an INT64 array takes 2.0 for 2; 2.5 equals no element);
  * ARRAY_CONTAINS_ALL(F, [..]): every distinct listed value occurs in the row (duplicates in the row or the list
    do not matter); ARRAY_CONTAINS_ANY(F, [..]): at least one does.  ALL(F, []) passes every row, ANY(F, []) none
    (they compile to TRUE / FALSE).  ALL takes at most 64 distinct values, ANY at most RF_COLUMN_MAX_SET.  A value
    no element can equal (a string the field's dictionary does not hold, 2.5 for an INT64 array) is dropped from
    ANY and makes ALL FALSE;
  * ARRAY_LENGTH(F) CMP n compares the row's element count with the integer n;
  * F[i] (i an integer literal, 0 <= i < 4096) takes every leaf a scalar field of the element type takes (CMP,
    chains, in / not in, like).  A row with len <= i fails EVERY leaf on F[i], `!=` and `not in` included -- the
    rule a dynamic key follows for a row that lacks it: F[i] != v is LENGTH(F) > i AND NOT (F[i] == v);
  * `not (...)` is plain negation: `not (F[i] == v)` passes the short rows.
A bare F (F == .., F in .., F like ..), a negative or non-integer index and a literal of the wrong type raise
ValueError naming the token.  An array leaf compiles into entries of `Program.array_leaves`, which rf_array_match
evaluates over the field's CSR mirror (offsets int64 [n + 1], values: int32 dictionary codes | int64 | fp64) into
row bitmaps: LENGTH (an inclusive interval of the count, through `int_interval`), ELEM (element i under the scalar
leaf a column leaf would be) and MATCH (sorted distinct needles and `need`: 1 for ANY / CONTAINS, their number for
ALL).

Compilation.  A VARCHAR leaf is evaluated once against the column's dictionary (every distinct
string, in first-seen order = its code) and becomes a set of codes, so a literal that is not in
the dictionary matches nothing; numeric leaves become interval tests; id leaves become a sorted
list of row numbers; a keyword leaf becomes the ids of its terms in the lexical index's dictionary
(`Program.text_leaves`, which rf_text_match turns into a row bitmap) and an RF_FOP_BITMAP leaf that
reads the bitmap; and / or / not become stack operations.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass, field
from typing import Any, Sequence

import numpy as np

from . import _lib, lexical
from .schema import INT64_MAX, INT64_MIN, RESERVED, DataType

VARCHAR_FIELDS = ("period", "chunk_type", "statement_type")   # device columns 0, 1, 2
DOUBLE_FIELDS = ("primary_value",)                             # device column 3
PK_FIELD = "id"
UNFILTERABLE = ("text", "embedding")
COLUMN_OF = {"period": 0, "chunk_type": 1, "statement_type": 2, "primary_value": 3}

_CMP = ("==", "!=", "<", "<=", ">", ">=")
TEXT_FUNCS = ("text_match", "phrase_match")
TEXT_FIELD = "text"
NO_LEXICAL_INDEX = ("TEXT_MATCH / PHRASE_MATCH need the lexical index over the text column: call "
                    "create_index('sparse', {'index_type': 'SPARSE_INVERTED_INDEX', 'metric_type': 'BM25'}) first")
DYNAMIC_KEYWORDS = ("and", "or", "not", "in", "like", "true", "false", "exists")   # never a bare dynamic key
_FLIP = {"<": ">", "<=": ">=", ">": "<", ">=": "<=", "==": "==", "!=": "!="}


def _scalar_type(f):
    """The DataType that types a field's literals: its own, or an ARRAY field's element type."""
    return f.element_type if f.dtype == DataType.ARRAY else f.dtype


def is_empty(expr) -> bool:
    """None, "" and whitespace mean "no filter"."""
    return expr is None or (isinstance(expr, str) and expr.strip() == "")


# ---- tokens ------------------------------------------------------------------------------------
@dataclass
class Tok:
    kind: str      # "name" | "str" | "num" | "op" | "end" | "meta" ($meta, with dynamic fields only)
    value: Any
    pos: int
    text: str


_TOKEN = re.compile(r"""
    (?P<ws>\s+)
  | (?P<num>(?:\d+\.\d*|\.\d+|\d+)(?:[eE][+-]?\d+)?)
  | (?P<name>[A-Za-z_][A-Za-z0-9_]*)
  | (?P<op>==|!=|<=|>=|&&|\|\||=|[<>()\[\],!+-])
""", re.X)


META = "$meta"   # the dynamic field's name: $meta["key"] in expr, "$meta" as an output field
_META = re.compile(r"\$meta(?![A-Za-z0-9_])")


def _err(msg: str, tok: Tok | None = None, pos: int | None = None) -> ValueError:
    if tok is not None:
        where = "end of expression" if tok.kind == "end" else f"{tok.text!r} at position {tok.pos}"
        return ValueError(f"filter expression: {msg}: {where}")
    return ValueError(f"filter expression: {msg} at position {pos}")


def tokenize(s: str, dynamic: bool = False) -> list[Tok]:
    out: list[Tok] = []
    i = 0
    while i < len(s):
        c = s[i]
        if dynamic and _META.match(s, i):
            out.append(Tok("meta", META, i, META))
            i += len(META)
            continue
        if c in "'\"":
            j = i + 1
            buf = []
            while j < len(s) and s[j] != c:
                if s[j] == "\\" and j + 1 < len(s):
                    j += 1
                buf.append(s[j])
                j += 1
            if j >= len(s):
                raise _err("unterminated string", pos=i)
            out.append(Tok("str", "".join(buf), i, s[i:j + 1]))
            i = j + 1
            continue
        m = _TOKEN.match(s, i)
        if not m:
            raise _err(f"unexpected character {c!r}", pos=i)
        kind = m.lastgroup
        text = m.group(0)
        if kind == "num":
            out.append(Tok("num", float(text) if any(ch in text for ch in ".eE") else int(text), i, text))
        elif kind == "name":
            out.append(Tok("name", text, i, text))
        elif kind == "op":
            out.append(Tok("op", text, i, text))
        i = m.end()
    out.append(Tok("end", None, len(s), ""))
    return out


# ---- AST ---------------------------------------------------------------------------------------
class Node:
    def eval(self, row: dict) -> bool:   # host reference semantics (tests, docs)
        raise NotImplementedError


@dataclass
class Cmp(Node):
    field: str
    op: str
    value: Any

    def eval(self, row):
        return _compare(row[self.field], self.op, self.value)


@dataclass
class In(Node):
    field: str
    values: list
    negate: bool = False

    def eval(self, row):
        x = row[self.field]
        hit = any(_compare(x, "==", v) for v in self.values)
        return not hit if self.negate else hit


@dataclass
class Like(Node):
    field: str
    pattern: str

    def eval(self, row):
        return like_match(row[self.field], self.pattern)


def _terms_of(analyzer, text: str) -> list:
    return list((analyzer or lexical.analyze)([text])[0])


@dataclass
class TextMatch(Node):
    """TEXT_MATCH(text, query, minimum_should_match=min_match).  analyzer: list[str] -> list[list[str]],
    None = lexical.analyze."""
    field: str
    query: str
    min_match: int = 1
    analyzer: Any = None

    def terms(self) -> list:
        """The distinct terms of the query, sorted."""
        return sorted(set(_terms_of(self.analyzer, self.query)))

    def eval(self, row):
        return len(set(self.terms()) & set(_terms_of(self.analyzer, row[self.field]))) >= self.min_match


@dataclass
class PhraseMatch(Node):
    """PHRASE_MATCH(text, query): the query's terms, adjacent and in order."""
    field: str
    query: str
    slop: int = 0
    analyzer: Any = None

    def terms(self) -> list:
        """The terms of the phrase in order."""
        return _terms_of(self.analyzer, self.query)

    def eval(self, row):
        p = self.terms()
        d = _terms_of(self.analyzer, row[self.field])
        m = len(p)
        return m > 0 and any(d[j:j + m] == p for j in range(len(d) - m + 1))


# -- dynamic fields: the semantics of a leaf over a key of $meta (module docstring), in pure Python --
def dynamic_class(v) -> str | None:
    """The type class of a dynamic value: "boolean", "number" (int and float together), "string"; None: the
    row lacks the key."""
    if v is None:
        return None
    if isinstance(v, bool):
        return "boolean"
    return "string" if isinstance(v, str) else "number"


def _dynamic_value(row: dict, key: str):
    """row: {field or dynamic key: value}, or a row that keeps its dynamic keys under "$meta"."""
    meta = row.get(META)
    return (row if meta is None else meta).get(key)


@dataclass
class DynCmp(Node):
    key: str
    op: str
    value: Any
    field = None

    def eval(self, row):
        x = _dynamic_value(row, self.key)
        return x is not None and dynamic_class(x) == dynamic_class(self.value) and _compare(x, self.op, self.value)


@dataclass
class DynIn(Node):
    key: str
    values: list
    negate: bool = False
    field = None

    def eval(self, row):
        x = _dynamic_value(row, self.key)
        if x is None or not self.values or dynamic_class(x) != dynamic_class(self.values[0]):
            return False
        return any(x == v for v in self.values) != self.negate


@dataclass
class DynLike(Node):
    key: str
    pattern: str
    field = None

    def eval(self, row):
        x = _dynamic_value(row, self.key)
        return isinstance(x, str) and like_match(x, self.pattern)


@dataclass
class Exists(Node):
    key: str
    field = None

    def eval(self, row):
        return _dynamic_value(row, self.key) is not None


DYNAMIC_NODES = (DynCmp, DynIn, DynLike, Exists)


# -- ARRAY fields: the semantics of a leaf over a declared ARRAY field (module docstring), in pure Python --
def _contains(arr, v) -> bool:
    return any(x == v for x in arr)   # (IEEE == for floats: NaN is never contained, -0.0 contains 0.0)


@dataclass
class ArrContains(Node):
    """ARRAY_CONTAINS(field, v) = ("any", [v]); ARRAY_CONTAINS_ANY / ARRAY_CONTAINS_ALL(field, values)."""
    field: str
    values: list
    mode: str = "any"   # "any" | "all"

    def eval(self, row):
        arr = row[self.field]
        hits = (_contains(arr, v) for v in self.values)
        return all(hits) if self.mode == "all" else any(hits)


@dataclass
class ArrLength(Node):
    """ARRAY_LENGTH(field) op value."""
    field: str
    op: str
    value: int

    def eval(self, row):
        return _compare(len(row[self.field]), self.op, self.value)


@dataclass
class ArrElem(Node):
    """field[index] under the scalar leaf `inner` (a Cmp, In or Like over the field's name): a row with
    len <= index fails it, `!=` and `not in` included."""
    field: str
    index: int
    inner: Node

    def eval(self, row):
        arr = row[self.field]
        return len(arr) > self.index and self.inner.eval({self.field: arr[self.index]})


ARRAY_NODES = (ArrContains, ArrLength, ArrElem)
ARRAY_FUNCS = ("array_contains", "array_contains_all", "array_contains_any", "array_length")
MAX_ARRAY_INDEX = 4096   # F[i]: i below Milvus' capacity limit


@dataclass
class And(Node):
    a: Node
    b: Node

    def eval(self, row):
        return self.a.eval(row) and self.b.eval(row)


@dataclass
class Or(Node):
    a: Node
    b: Node

    def eval(self, row):
        return self.a.eval(row) or self.b.eval(row)


@dataclass
class Not(Node):
    a: Node

    def eval(self, row):
        return not self.a.eval(row)


def _compare(x, op: str, v) -> bool:
    # IEEE for floats (NaN: only != holds), code-point order for str
    if op == "==":
        return x == v
    if op == "!=":
        return x != v
    if op == "<":
        return x < v
    if op == "<=":
        return x <= v
    if op == ">":
        return x > v
    return x >= v


def like_match(s: str, pattern: str) -> bool:
    core = pattern.strip("%")
    lead, trail = pattern.startswith("%"), pattern.endswith("%") and len(pattern) > 1
    if lead and trail:
        return core in s
    if lead:
        return s.endswith(core)
    if trail:
        return s.startswith(core)
    return s == pattern


# ---- parser ------------------------------------------------------------------------------------
class _Parser:
    def __init__(self, text: str, analyzer=None, schema=None, dynamic: bool = False):
        self.toks = tokenize(text, dynamic)
        self.i = 0
        self.analyzer = analyzer
        self.dynamic = dynamic   # a name that is no field of the collection is a key of $meta
        # the collection's own fields (schema.py); an ARRAY field stands with its element type, which types the
        # literals of its leaves, and its name is in `arrays`
        self.extra = {f.name: _scalar_type(f) for f in schema or ()}
        self.arrays = {f.name for f in schema or () if f.dtype == DataType.ARRAY}

    def peek(self, k: int = 0) -> Tok:
        return self.toks[min(self.i + k, len(self.toks) - 1)]

    def take(self) -> Tok:
        t = self.toks[self.i]
        self.i = min(self.i + 1, len(self.toks) - 1)
        return t

    def kw(self, word: str, k: int = 0) -> bool:
        t = self.peek(k)
        return t.kind == "name" and t.value.lower() == word

    def op(self, sym: str, k: int = 0) -> bool:
        t = self.peek(k)
        return t.kind == "op" and t.value == sym

    def parse(self) -> Node:
        if self.peek().kind == "end":
            raise _err("empty expression", self.peek())
        node = self.expr()
        if self.peek().kind != "end":
            t = self.peek()
            raise _err("unexpected token" + (" (arithmetic is not supported)" if t.kind == "op" and t.value in "+-" else ""), t)
        return node

    def expr(self) -> Node:
        node = self.and_()
        while self.kw("or") or self.op("||"):
            self.take()
            node = Or(node, self.and_())
        return node

    def and_(self) -> Node:
        node = self.unary()
        while self.kw("and") or self.op("&&"):
            self.take()
            node = And(node, self.unary())
        return node

    def unary(self) -> Node:
        if self.kw("not") or self.op("!"):
            self.take()
            return Not(self.unary())
        if self.op("("):
            self.take()
            node = self.expr()
            if not self.op(")"):
                raise _err("expected ')'", self.peek())
            self.take()
            return node
        return self.compare()

    # -- leaves ------------------------------------------------------------------------------
    def field(self) -> tuple[str, Tok]:
        t = self.take()
        if t.kind != "name" or t.value.lower() in ("and", "or", "not", "in", "like"):
            raise _err("expected a field name", t)
        name = t.value
        if name in UNFILTERABLE:
            raise _err(f"field {name!r} cannot be filtered on", t)
        if not self.known(name):
            if name.lower().startswith(("json_", "array_")) and self.op("("):
                raise _err(f"unknown function {name!r} (ARRAY and JSON fields are not supported)", t)
            if not self.dynamic or name in RESERVED or name.lower() in DYNAMIC_KEYWORDS:
                raise _err(f"unknown field {name!r}", t)
        return name, t

    def known(self, name: str) -> bool:
        return name in VARCHAR_FIELDS + DOUBLE_FIELDS + (PK_FIELD,) or name in self.extra

    def operand(self) -> tuple[str, Tok, bool]:
        """A scalar field, or with dynamic fields a key of $meta: (name, its token, is a dynamic key)."""
        t = self.peek()
        if t.kind != "meta":
            name, ft = self.field()
            if name in self.arrays:
                raise _err(f"{name!r} is an ARRAY field: it is read through ARRAY_CONTAINS / ARRAY_CONTAINS_ALL / "
                           f"ARRAY_CONTAINS_ANY / ARRAY_LENGTH or an index {name}[i], not compared whole", ft)
            return name, ft, not self.known(name)
        self.take()
        if not self.op("["):
            raise _err("expected '[' after $meta", self.peek())
        self.take()
        kt = self.take()
        if kt.kind != "str" or kt.value == "":
            raise _err("$meta takes a non-empty string key, as in $meta[\"key\"]", kt)
        if not self.op("]"):
            raise _err("expected ']'", self.peek())
        self.take()
        return kt.value, t, True

    def dtype(self, name: str):
        """The DataType of a filterable scalar field (None: the primary key)."""
        if name in VARCHAR_FIELDS:
            return DataType.VARCHAR
        if name in DOUBLE_FIELDS:
            return DataType.DOUBLE
        return self.extra.get(name)

    def literal(self) -> tuple[Any, Tok]:
        t = self.take()
        if t.kind == "str":
            return t.value, t
        sign = 1
        first = t
        if t.kind == "op" and t.value in "+-":
            sign = -1 if t.value == "-" else 1
            t = self.take()
        if t.kind == "num":
            return sign * t.value, first
        if first is t and t.kind == "name" and t.value.lower() in ("true", "false"):
            return t.value.lower() == "true", t
        if first.kind == "name":
            raise _err("expected a literal (a field compared with a field is not supported)", first)
        raise _err("expected a literal", first)

    def cmp_op(self) -> Tok | None:
        t = self.peek()
        if t.kind == "op" and t.value in _CMP:
            return self.take()
        return None

    def compare(self) -> Node:
        t = self.peek()
        if t.kind in ("str", "num") or (t.kind == "op" and t.value in "+-") or \
                (t.kind == "name" and t.value.lower() in ("true", "false") and t.value not in self.extra):
            # literal CMP field [CMP literal]
            lit, lt = self.literal()
            o1 = self.cmp_op()
            if o1 is None:
                raise _err("expected a comparison operator", self.peek())
            arr = self.array_operand()
            if arr is not None:
                name, ft, dyn = arr[1], arr[-1], False
                leaf = lambda *a: self._array_cmp(arr, *a[2:])   # noqa: E731
            else:
                name, ft, dyn = self.operand()
                leaf = self._dynamic_cmp if dyn else self._leaf_cmp
            left = leaf(name, ft, _FLIP[o1.value], lit, lt, o1)
            o2 = self.cmp_op()
            if o2 is None:
                return left
            lit2, lt2 = self.literal()
            return And(left, leaf(name, ft, o2.value, lit2, lt2, o2))
        if t.kind == "name" and t.value.lower() in TEXT_FUNCS and self.op("(", 1):
            return self.text_func()
        if t.kind == "name" and t.value.lower() in ARRAY_FUNCS[:3] and self.op("(", 1) and self._array_name(2):
            return self.array_func()
        arr = self.array_operand()
        if arr is not None:
            if arr[0] == "elem":   # F[i] stands where a scalar field of the element type does
                return ArrElem(arr[1], arr[2], self._after_operand(arr[1], arr[-1], False))
            o = self.cmp_op()
            if o is None:
                raise _err("expected a comparison operator after ARRAY_LENGTH(...)", self.peek())
            lit, lt = self.literal()
            return self._array_cmp(arr, o.value, lit, lt, o)
        if self.dynamic and self.kw("exists") and not self.known("exists"):
            et = self.take()
            if self.peek().kind not in ("name", "meta"):
                raise _err("'exists' takes a dynamic key", self.peek() if self.peek().kind != "end" else et)
            name, ft, dyn = self.operand()
            if not dyn:
                raise _err(f"'exists' takes a dynamic key, {name!r} is a field of the collection", ft)
            return Exists(name)
        return self._after_operand(*self.operand())

    def _after_operand(self, name, ft, dyn) -> Node:
        """CMP literal | [not] in [...] | like STRING behind a scalar operand."""
        o = self.cmp_op()
        if o is not None:
            lit, lt = self.literal()
            return (self._dynamic_cmp if dyn else self._leaf_cmp)(name, ft, o.value, lit, lt, o)
        negate = False
        if self.kw("not") and self.kw("in", 1):
            self.take()
            negate = True
        if self.kw("in"):
            kt = self.take()
            if dyn:
                return DynIn(name, self._list(name, kt, dynamic=True), negate)
            return In(name, self._list(name, kt), negate)
        if self.kw("like"):
            kt = self.take()
            if not dyn and self.dtype(name) != DataType.VARCHAR:
                raise _err(f"'like' needs a VARCHAR field, {name!r} is not one", kt)
            pt = self.take()
            if pt.kind != "str":
                raise _err("'like' needs a string pattern", pt)
            if "%" in pt.value.strip("%") or pt.value in ("%", "%%"):
                raise _err("'like' supports 'p%', '%s' and '%i%' only", pt)
            return DynLike(name, pt.value) if dyn else Like(name, pt.value)
        nt = self.peek()
        if nt.kind == "op" and nt.value in "+-":
            raise _err("expected a comparison, 'in' or 'like' (arithmetic is not supported)", nt)
        if nt.kind == "op" and nt.value == "[":
            raise _err("expected a comparison, 'in' or 'like' (ARRAY and JSON fields are not supported)", nt)
        raise _err("expected a comparison, 'in' or 'like'", nt)

    # -- ARRAY fields ---------------------------------------------------------------------------
    def _array_name(self, k: int = 0) -> bool:
        t = self.peek(k)
        return t.kind == "name" and t.value in self.arrays

    def array_operand(self):
        """ARRAY_LENGTH ( F ) -> ("length", F, token) | F [ INT ] -> ("elem", F, index, token) over a declared
        ARRAY field F, consumed; None (and nothing consumed) when neither stands here."""
        t = self.peek()
        if t.kind == "name" and t.value.lower() == "array_length" and self.op("(", 1) and self._array_name(2):
            self.take()
            self.take()
            name = self.take().value
            if not self.op(")"):
                raise _err("expected ')'", self.peek())
            self.take()
            return "length", name, t
        if self._array_name() and self.op("[", 1):
            self.take()
            self.take()
            it = self.take()
            if it.kind != "num" or not isinstance(it.value, int) or it.value >= MAX_ARRAY_INDEX:
                raise _err(f"an array index is a non-negative integer literal below {MAX_ARRAY_INDEX}", it)
            if not self.op("]"):
                raise _err("expected ']'", self.peek())
            self.take()
            return "elem", t.value, it.value, t
        return None

    def _array_cmp(self, arr, op, lit, lt, ot) -> Node:
        """The comparison leaf of an array operand (array_operand) with a literal."""
        if arr[0] == "elem":
            return ArrElem(arr[1], arr[2], self._leaf_cmp(arr[1], arr[-1], op, lit, lt, ot))
        if isinstance(lit, bool) or not isinstance(lit, int):
            raise _err("ARRAY_LENGTH is compared with an integer", lt)
        return ArrLength(arr[1], op, lit)

    def array_func(self) -> Node:
        """ARRAY_CONTAINS ( F , literal ) | ARRAY_CONTAINS_ALL / _ANY ( F , [ literal, ... ] )."""
        ft = self.take()
        func = ft.value.lower()
        self.take()   # "("
        name = self.take().value
        if not self.op(","):
            raise _err("expected ','", self.peek())
        kt = self.take()
        if func == "array_contains":
            lit, lt = self.literal()
            node = ArrContains(name, [self._check_type(name, lit, lt)], "any")
        else:
            node = ArrContains(name, self._list(name, kt), "all" if func == "array_contains_all" else "any")
        if not self.op(")"):
            raise _err("expected ')'", self.peek())
        self.take()
        return node

    def text_func(self) -> Node:
        """The keyword leaf of the grammar: FUNC ( text , STRING [, NAME = NUM | , NUM] )."""
        ft = self.take()
        func = ft.value.upper()
        phrase = func == "PHRASE_MATCH"
        self.take()   # "("
        t = self.take()
        if t.kind != "name":
            raise _err(f"{func} expects the field name first", t)
        if t.value != TEXT_FIELD:
            raise _err(f"{func} takes the field {TEXT_FIELD!r} only, not {t.value!r}", t)
        if not self.op(","):
            raise _err("expected ','", self.peek())
        self.take()
        st = self.take()
        if st.kind != "str":
            raise _err(f"{func} expects a string of terms", st)
        option, arg = ("slop", 0) if phrase else ("minimum_should_match", 1)
        if self.op(","):
            self.take()
            if self.peek().kind == "name":
                nt = self.take()
                if nt.value.lower() != option:
                    raise _err(f"{func} takes the option {option} only", nt)
                if not self.op("="):
                    raise _err("expected '='", self.peek())
                self.take()
            vt = self.take()
            if vt.kind != "num" or not isinstance(vt.value, int):
                raise _err(f"{option} must be an integer" + ("" if phrase else " >= 1"), vt)
            if phrase and vt.value != 0:
                raise _err("PHRASE_MATCH offers exact adjacency only (slop 0)", vt)
            if not phrase and vt.value < 1:
                raise _err("minimum_should_match must be an integer >= 1", vt)
            arg = vt.value
        if not self.op(")"):
            raise _err("expected ')'", self.peek())
        self.take()
        node = (PhraseMatch if phrase else TextMatch)(TEXT_FIELD, st.value, arg, self.analyzer)
        n_terms = len(node.terms())
        if n_terms > lexical.MAX_QUERY_TERMS:
            raise _err(f"{func}: {n_terms} {'terms in the phrase' if phrase else 'distinct terms'}, at most "
                       f"{lexical.MAX_QUERY_TERMS} are taken", st)
        return node

    def _list(self, name: str, kt: Tok, dynamic: bool = False) -> list:
        if not self.op("["):
            raise _err("expected '['", self.peek())
        self.take()
        vals = []
        if not self.op("]"):
            while True:
                lit, lt = self.literal()
                if dynamic and vals and dynamic_class(lit) != dynamic_class(vals[0]):
                    raise _err(f"an 'in' list over a dynamic key holds one type class, {dynamic_class(vals[0])}s here", lt)
                vals.append(lit if dynamic else self._check_type(name, lit, lt))
                if self.op(","):
                    self.take()
                    continue
                break
        if not self.op("]"):
            raise _err("expected ']'", self.peek())
        self.take()
        return vals

    def _dynamic_cmp(self, key, ft, op, lit, lt, ot) -> Node:
        if isinstance(lit, bool) and op not in ("==", "!="):
            raise _err(f"a boolean supports == != in / not in only, not {ot.value!r}", ot)
        return DynCmp(key, op, lit)

    def _leaf_cmp(self, name, ft, op, lit, lt, ot) -> Node:
        if name == PK_FIELD and op not in ("==", "!="):
            raise _err(f"the primary key supports == != in / not in only, not {ot.value!r}", ot)
        if self.dtype(name) == DataType.BOOL and op not in ("==", "!="):
            raise _err(f"a BOOL field supports == != in / not in only, not {ot.value!r}", ot)
        return Cmp(name, op, self._check_type(name, lit, lt))

    def _check_type(self, name: str, lit, tok: Tok):
        t = self.dtype(name)
        if t == DataType.VARCHAR:
            if not isinstance(lit, str):
                raise _err(f"{name} is VARCHAR, the literal is not a string", tok)
            return lit
        if t == DataType.DOUBLE:
            if isinstance(lit, str):
                raise _err(f"{name} is DOUBLE, the literal is a string", tok)
            if isinstance(lit, bool):
                raise _err(f"{name} is DOUBLE, the literal is a boolean", tok)
            return float(lit)
        if t == DataType.BOOL:
            if not isinstance(lit, bool):
                raise _err(f"{name} is BOOL, the literal is not true or false", tok)
            return lit
        if t == DataType.INT64:
            if isinstance(lit, (str, bool)):
                raise _err(f"{name} is INT64, the literal is a {'string' if isinstance(lit, str) else 'boolean'}", tok)
            if isinstance(lit, float):
                if not math.isfinite(lit):
                    raise _err(f"{name} is INT64, the literal is not finite", tok)
                return lit   # compared mathematically: x > 2.5 is x >= 3
            if not INT64_MIN <= lit <= INT64_MAX:
                raise _err(f"{name} is INT64, the literal is outside the int64 range", tok)
            return lit
        if isinstance(lit, bool):
            raise _err("the primary key is compared with its keys, not with a boolean", tok)
        return lit   # id: int or str keys, as inserted


def parse(text: str, analyzer=None, schema=None, dynamic: bool = False) -> Node:
    """analyzer: what the keyword leaves analyse their strings with (None = lexical.analyze).
    schema: the collection's own fields (a sequence of schema.FieldSchema; None = none: a name outside
    the reference's fields is an unknown field).  dynamic: the collection has enable_dynamic_field: such a
    name is a key of $meta instead, and $meta["key"] and `exists key` are taken (module docstring)."""
    if not isinstance(text, str):
        raise ValueError(f"filter expression must be a string, got {type(text).__name__}")
    return _Parser(text, analyzer, schema, dynamic).parse()


def text_leaves(node: Node) -> list:
    """The TextMatch / PhraseMatch leaves of a tree, in evaluation order."""
    if isinstance(node, (And, Or)):
        return text_leaves(node.a) + text_leaves(node.b)
    if isinstance(node, Not):
        return text_leaves(node.a)
    return [node] if isinstance(node, (TextMatch, PhraseMatch)) else []


def fields_of(node: Node) -> set:
    """The names of the fields a tree's leaves read."""
    if isinstance(node, (And, Or)):
        return fields_of(node.a) | fields_of(node.b)
    if isinstance(node, Not):
        return fields_of(node.a)
    return set() if isinstance(node, DYNAMIC_NODES) else {node.field}


def array_fields_of(node: Node) -> set:
    """The names of the ARRAY fields a tree's leaves read."""
    if isinstance(node, (And, Or)):
        return array_fields_of(node.a) | array_fields_of(node.b)
    if isinstance(node, Not):
        return array_fields_of(node.a)
    return {node.field} if isinstance(node, ARRAY_NODES) else set()


def dynamic_keys_of(node: Node) -> set:
    """The dynamic keys a tree's leaves read."""
    if isinstance(node, (And, Or)):
        return dynamic_keys_of(node.a) | dynamic_keys_of(node.b)
    if isinstance(node, Not):
        return dynamic_keys_of(node.a)
    return {node.key} if isinstance(node, DYNAMIC_NODES) else set()


# ---- compilation -------------------------------------------------------------------------------
@dataclass
class Program:
    """The postfix program of rf_filter_eval: ops (tuples op, column, off, len, flags, lo, hi),
    the code-set bitmap words and the sorted row lists the leaves point into.  text_leaves: the
    keyword leaves as (kind RF_TEXT_*, term ids, min_match), the input of rf_text_match; the
    RF_FOP_BITMAP op of leaf l carries l in `off`, and ops_ctypes turns it into the leaf's word range
    once the caller knows how many words a leaf's bitmap has.
    column_leaves: the leaves over the collection's own fields (schema.py), the input of rf_column_match:
    ("codeset", field, code-set words) | ("irange", field, lo, hi) -- inclusive int64 bounds |
    ("iset", field, sorted distinct int64 values) | ("frange", field, RF_FRANGE_* flags, lo, hi).  The
    RF_FOP_BITMAP op of column leaf c carries c in `off` and COLUMN_LEAF in `column`; the column leaves'
    bitmaps (column_words words each) follow the keyword leaves' from word column_base of the one
    bitmap array the program indexes.
    dynamic_leaves: the leaves over dynamic keys, the input of rf_dynamic_match:
    ("tags", key, tag mask) | ("codeset", key, code-set words) | ("bool", key, 2-bit value set) |
    ("nrange", key, ilo, ihi, RF_FRANGE_* flags, flo, fhi) | ("nset", key, sorted int64 values, sorted fp64
    values).  The RF_FOP_BITMAP op of dynamic leaf d carries d in `off` and DYNAMIC_LEAF in `column`; their
    bitmaps (column_words words each) follow the column leaves'.
    array_leaves: the leaves over ARRAY fields, the input of rf_array_match:
    ("length", field, lo, hi) -- inclusive bounds of the row's element count |
    ("elem", field, index, scalar leaf) -- scalar leaf: an entry as in column_leaves, tested on element `index` |
    ("match", field, "code" | "i64" | "f64", sorted distinct needles, need) -- need 1 (ANY / CONTAINS) or
    len(needles) <= 64 (ALL).  The RF_FOP_BITMAP op of array leaf a carries a in `off` and ARRAY_LEAF in
    `column`; their bitmaps (column_words words each) follow the dynamic leaves'."""
    ops: list = field(default_factory=list)
    code_sets: list = field(default_factory=list)
    row_lists: list = field(default_factory=list)
    text_leaves: list = field(default_factory=list)
    column_leaves: list = field(default_factory=list)
    dynamic_leaves: list = field(default_factory=list)
    array_leaves: list = field(default_factory=list)

    def resolved_ops(self, words_per_leaf: int = 0, column_base: int = 0, column_words: int = 0) -> list:
        """The op tuples as the device takes them: every RF_FOP_BITMAP leaf with its word range."""
        out = []
        for op, col, off, ln, flags, lo, hi in self.ops:
            if op == _lib.RF_FOP_BITMAP and col == COLUMN_LEAF:
                col, off, ln = 0, column_base + off * column_words, column_words
            elif op == _lib.RF_FOP_BITMAP and col == DYNAMIC_LEAF:
                col, off, ln = 0, column_base + (len(self.column_leaves) + off) * column_words, column_words
            elif op == _lib.RF_FOP_BITMAP and col == ARRAY_LEAF:
                behind = len(self.column_leaves) + len(self.dynamic_leaves)
                col, off, ln = 0, column_base + (behind + off) * column_words, column_words
            elif op == _lib.RF_FOP_BITMAP:
                off, ln = off * words_per_leaf, words_per_leaf
            out.append((op, col, off, ln, flags, lo, hi))
        return out

    def ops_ctypes(self, words_per_leaf: int = 0, column_base: int = 0, column_words: int = 0):
        arr = (_lib.FilterOp * len(self.ops))()
        for i, (op, col, off, ln, flags, lo, hi) in enumerate(self.resolved_ops(words_per_leaf, column_base,
                                                                                column_words)):
            arr[i].op, arr[i].column, arr[i].off, arr[i].len = op, col, off, ln
            arr[i].flags, arr[i].lo, arr[i].hi = flags, lo, hi
        return arr

    def max_depth(self) -> int:
        d = m = 0
        for o in self.ops:
            d += 1 if o[0] <= _lib.RF_FOP_FALSE or o[0] == _lib.RF_FOP_BITMAP else (-1 if o[0] in (_lib.RF_FOP_AND, _lib.RF_FOP_OR) else 0)
            m = max(m, d)
        return m


COLUMN_LEAF = 1   # `column` of an RF_FOP_BITMAP op in Program.ops: the bitmap of a column leaf, not of a keyword leaf
DYNAMIC_LEAF = 2  # ... the bitmap of a dynamic leaf
ARRAY_LEAF = 3    # ... the bitmap of an array leaf
MAX_ALL = _lib.RF_ARRAY_MAX_ALL   # distinct values of one ARRAY_CONTAINS_ALL
MAX_INT_SET = _lib.RF_COLUMN_MAX_SET
NUMBER_TAGS = 1 << _lib.RF_DTAG_INT | 1 << _lib.RF_DTAG_DOUBLE
HELD_TAGS = 1 << _lib.RF_DTAG_BOOL | NUMBER_TAGS | 1 << _lib.RF_DTAG_STRING   # every tag but ABSENT


def int_interval(op: str, v) -> tuple[int, int] | None:
    """An INT64 comparison `x op v` (v an int, or a finite float compared mathematically) as the inclusive
    int64 interval (lo, hi) it selects; None: no int64 passes.  `!=` is the caller's (not ==)."""
    lo, hi = INT64_MIN, INT64_MAX
    if op == "==":
        if v != math.floor(v):
            return None
        lo = hi = int(v)
    elif op == ">":
        lo = math.floor(v) + 1
    elif op == ">=":
        lo = math.ceil(v)
    elif op == "<":
        hi = math.ceil(v) - 1
    else:
        hi = math.floor(v)
    lo, hi = max(lo, INT64_MIN), min(hi, INT64_MAX)
    return (lo, hi) if lo <= hi else None


def _int_interval(op: str, v) -> tuple[int, int] | None:
    """int_interval for any number literal: an infinite float too."""
    if isinstance(v, float) and math.isinf(v):
        return (INT64_MIN, INT64_MAX) if op in (("<", "<=") if v > 0 else (">", ">=")) else None
    return int_interval(op, v)


def _exact_float(v) -> float | None:
    """The double that equals the number v (an int of any size, or a float), or None when there is none."""
    try:
        f = float(v)
    except OverflowError:
        return None
    return f if f == v else None   # (Python compares an int with a float exactly)


def _float_below(v) -> float:
    """The largest double <= v."""
    try:
        f = float(v)   # round to nearest: at most one step off
    except OverflowError:
        return -math.inf if v < 0 else math.nextafter(math.inf, 0.0)   # (an int beyond the doubles' range)
    return f if f <= v else math.nextafter(f, -math.inf)


def _float_above(v) -> float:
    """The smallest double >= v."""
    return -_float_below(-v)


def f64_interval(op: str, v) -> tuple[int, float, float]:
    """A comparison `x op v` of an fp64 x with a number literal v (an int of any size, or a float), compared
    mathematically, as the IEEE interval test (RF_FRANGE_* flags, lo, hi) that selects exactly the same doubles.
    An int that no double represents lies strictly between two neighbouring doubles, so rounding it DOWN for a
    lower bound of `>` (UP for `>=`) and UP for the upper bound of `<` (DOWN for `<=`) loses nothing; `==` with
    such an int passes nothing (lo = +inf, hi = -inf, both exclusive).  `!=` is the caller's (not ==)."""
    inf = math.inf
    L, H = _lib.RF_FRANGE_LO_INCL, _lib.RF_FRANGE_HI_INCL
    if op == "==":
        f = _exact_float(v)
        return (0, inf, -inf) if f is None else (L | H, f, f)
    if op == ">":
        return H, _float_below(v), inf
    if op == ">=":
        return L | H, _float_above(v), inf
    if op == "<":
        return L, -inf, _float_above(v)
    return L | H, -inf, _float_below(v)


class _Compiler:
    def __init__(self, dicts: dict[str, Sequence[str]], pk_row: dict, term_id: dict | None = None, schema=None,
                 extra_dicts: dict | None = None, dynamic: dict | None = None):
        self.dynamic = dynamic or {}   # dynamic key some row holds -> its dictionary of strings (code = index)
        self.dicts = dicts
        self.pk_row = pk_row
        self.term_id = term_id
        self.extra = {f.name: _scalar_type(f) for f in schema or ()}
        self.arrays = {f.name for f in schema or () if f.dtype == DataType.ARRAY}
        self._elem = None   # (field, index) while the scalar leaf under an ArrElem is compiled
        self.extra_dicts = extra_dicts or {}
        self.p = Program()

    def leaf(self, op, col=0, off=0, ln=0, flags=0, lo=0.0, hi=0.0):
        self.p.ops.append((op, col, off, ln, flags, lo, hi))

    def emit(self, n: Node) -> None:
        if isinstance(n, (And, Or)):
            self.emit(n.a)
            self.emit(n.b)
            self.leaf(_lib.RF_FOP_AND if isinstance(n, And) else _lib.RF_FOP_OR)
        elif isinstance(n, Not):
            self.emit(n.a)
            self.leaf(_lib.RF_FOP_NOT)
        elif isinstance(n, (TextMatch, PhraseMatch)):
            self.text(n)
        elif isinstance(n, DYNAMIC_NODES):
            self.dynamic_node(n)
        elif isinstance(n, ARRAY_NODES):
            self.array_node(n)
        elif n.field in self.extra:
            self.column(n, self.extra[n.field])
        elif n.field in VARCHAR_FIELDS:
            self.codeset(n)
        elif n.field in DOUBLE_FIELDS:
            self.numeric(n)
        else:
            self.pk(n)

    def text(self, n: Node) -> None:
        if self.term_id is None:
            raise ValueError("filter expression: " + NO_LEXICAL_INDEX)
        terms = n.terms()
        ids = [self.term_id.get(t) for t in terms]
        if isinstance(n, TextMatch):
            # a term no row holds matches nothing: dropped; fewer than N left can never reach N
            ids = sorted(i for i in ids if i is not None)
            kind, need = _lib.RF_TEXT_MATCH, n.min_match
            dead = len(ids) < need
        else:
            kind, need = _lib.RF_TEXT_PHRASE, 1
            dead = not ids or any(i is None for i in ids)
        if dead:
            self.leaf(_lib.RF_FOP_FALSE)
            return
        if len(self.p.text_leaves) == _lib.RF_TEXT_MAX_LEAVES:
            raise ValueError(f"filter expression: more than {_lib.RF_TEXT_MAX_LEAVES} TEXT_MATCH / PHRASE_MATCH leaves")
        self.leaf(_lib.RF_FOP_BITMAP, 0, len(self.p.text_leaves))
        self.p.text_leaves.append((kind, ids, need))

    # -- leaves over the collection's own fields: one RF_FOP_BITMAP op + one entry of column_leaves each --
    def column_leaf(self, *leaf) -> None:
        if self._elem is not None:   # the scalar leaf under F[i]: an array leaf that tests element i with it
            self.array_leaf("elem", self._elem[0], self._elem[1], leaf)
            return
        self.leaf(_lib.RF_FOP_BITMAP, COLUMN_LEAF, len(self.p.column_leaves))
        self.p.column_leaves.append(leaf)

    def column(self, n: Node, t) -> None:
        negate = (isinstance(n, Cmp) and n.op == "!=") or (isinstance(n, In) and n.negate)
        if t in (DataType.VARCHAR, DataType.BOOL):
            # against the field's dictionary (first-seen order = code), as for period
            d = self.extra_dicts.get(n.field, ())
            codes = [c for c, s in enumerate(d) if n.eval({n.field: s})]
            if not codes:
                self.leaf(_lib.RF_FOP_FALSE)
                return
            words = [0] * ((max(codes) >> 5) + 1)
            for c in codes:
                words[c >> 5] |= 1 << (c & 31)
            self.column_leaf("codeset", n.field, words)
            return
        if t == DataType.INT64:
            if isinstance(n, Cmp):
                iv = int_interval("==" if n.op == "!=" else n.op, n.value)
                if iv is None:
                    self.leaf(_lib.RF_FOP_FALSE)
                else:
                    self.column_leaf("irange", n.field, iv[0], iv[1])
            else:
                # (2.5 equals no integer, 1e30 no int64)
                vals = sorted({int(v) for v in n.values if v == math.floor(v) and INT64_MIN <= v <= INT64_MAX})
                if len(vals) > MAX_INT_SET:
                    raise ValueError(f"filter expression: {n.field} {'not in' if n.negate else 'in'} [...] holds "
                                     f"{len(vals)} distinct values, at most {MAX_INT_SET} are taken")
                if vals:
                    self.column_leaf("iset", n.field, vals)
                else:
                    self.leaf(_lib.RF_FOP_FALSE)
            if negate:
                self.leaf(_lib.RF_FOP_NOT)
            return
        # DOUBLE: as primary_value, IEEE semantics
        if isinstance(n, Cmp):
            self.column_frange(n.field, "==" if n.op == "!=" else n.op, n.value)
        else:
            if not n.values:
                self.leaf(_lib.RF_FOP_FALSE)
            for j, v in enumerate(n.values):
                self.column_frange(n.field, "==", v)
                if j:
                    self.leaf(_lib.RF_FOP_OR)
        if negate:   # NaN != v holds: the negation of an IEEE == test
            self.leaf(_lib.RF_FOP_NOT)

    def column_frange(self, name: str, op: str, v: float) -> None:
        inf = math.inf
        L, H = _lib.RF_FRANGE_LO_INCL, _lib.RF_FRANGE_HI_INCL
        lo, hi, flags = {"==": (v, v, L | H), "<": (-inf, v, L), "<=": (-inf, v, L | H),
                         ">": (v, inf, H), ">=": (v, inf, L | H)}[op]
        self.column_leaf("frange", name, flags, lo, hi)

    # -- leaves over ARRAY fields: RF_FOP_BITMAP ops + entries of array_leaves (module docstring) --
    def array_leaf(self, *leaf) -> None:
        self.leaf(_lib.RF_FOP_BITMAP, ARRAY_LEAF, len(self.p.array_leaves))
        self.p.array_leaves.append(leaf)

    def array_length(self, name: str, op: str, v: int) -> None:
        iv = int_interval(op, v)
        lo, hi = (max(iv[0], 0), iv[1]) if iv is not None else (1, 0)   # (a length is never negative)
        if lo > hi:
            self.leaf(_lib.RF_FOP_FALSE)
        else:
            self.array_leaf("length", name, lo, hi)

    def array_node(self, n: Node) -> None:
        t = self.extra[n.field]   # the element type
        if isinstance(n, ArrLength):
            self.array_length(n.field, "==" if n.op == "!=" else n.op, n.value)
            if n.op == "!=":
                self.leaf(_lib.RF_FOP_NOT)
            return
        if isinstance(n, ArrElem):
            # a row with len <= index fails every leaf.  The leaf of a positive test already says so; the NOT
            # that column() puts behind a numeric `!=` / `not in` would pass the short rows, so those become
            # LENGTH(F) > index AND NOT (F[index] == v).  (VARCHAR / BOOL: the code set holds the negation.)
            inner = n.inner
            guard = t in (DataType.INT64, DataType.DOUBLE) and \
                ((isinstance(inner, Cmp) and inner.op == "!=") or (isinstance(inner, In) and inner.negate))
            if guard:
                self.array_length(n.field, ">", n.index)
            self._elem = (n.field, n.index)
            try:
                self.column(inner, t)
            finally:
                self._elem = None
            if guard:
                self.leaf(_lib.RF_FOP_AND)
            return
        self.array_contains(n, t)

    def array_contains(self, n: "ArrContains", t) -> None:
        every = n.mode == "all"
        what = "ARRAY_CONTAINS_ALL" if every else "ARRAY_CONTAINS_ANY"
        if every and len(set(n.values)) > MAX_ALL:   # (before anything is dropped: the text's own count)
            raise ValueError(f"filter expression: {what}({n.field}, [...]) holds {len(set(n.values))} distinct values, "
                             f"at most {MAX_ALL} are taken")
        if not n.values:   # ALL of nothing holds everywhere, ANY of nothing nowhere
            self.leaf(_lib.RF_FOP_TRUE if every else _lib.RF_FOP_FALSE)
            return
        # the needles as the device compares them; a value no element can equal is None
        if t in (DataType.VARCHAR, DataType.BOOL):
            code = {v: c for c, v in enumerate(self.extra_dicts.get(n.field, ()))}   # (first-seen order = code)
            kind, needles = "code", [code.get(v) for v in n.values]
        elif t == DataType.INT64:   # (2.5 equals no integer, 1e30 no int64)
            kind, needles = "i64", [int(v) if not (isinstance(v, float) and math.isinf(v)) and v == math.floor(v)
                                    and INT64_MIN <= v <= INT64_MAX else None for v in n.values]
        else:   # DOUBLE: IEEE ==, so NaN equals nothing and -0.0 is the needle 0.0
            kind, needles = "f64", [None if v != v else v + 0.0 for v in n.values]
        if every and any(v is None for v in needles):
            self.leaf(_lib.RF_FOP_FALSE)
            return
        needles = sorted({v for v in needles if v is not None})
        if len(needles) > MAX_INT_SET:
            raise ValueError(f"filter expression: {what}({n.field}, [...]) holds {len(needles)} distinct values, at most "
                             f"{MAX_INT_SET} are taken")
        if not needles:
            self.leaf(_lib.RF_FOP_FALSE)
            return
        self.array_leaf("match", n.field, kind, needles, len(needles) if every else 1)

    # -- leaves over dynamic keys: RF_FOP_BITMAP ops + entries of dynamic_leaves (module docstring) --
    def dynamic_leaf(self, *leaf) -> None:
        self.leaf(_lib.RF_FOP_BITMAP, DYNAMIC_LEAF, len(self.p.dynamic_leaves))
        self.p.dynamic_leaves.append(leaf)

    def dynamic_node(self, n: Node) -> None:
        key = n.key
        if key not in self.dynamic:   # no row holds the key
            self.leaf(_lib.RF_FOP_FALSE)
            return
        if isinstance(n, Exists):
            self.dynamic_leaf("tags", key, HELD_TAGS)
            return
        cls = "string" if isinstance(n, DynLike) else \
            dynamic_class(n.value if isinstance(n, DynCmp) else (n.values[0] if n.values else None))
        if cls is None:   # k in [] / k not in []
            self.leaf(_lib.RF_FOP_FALSE)
        elif cls == "string":
            # against the key's dictionary (first-seen order = code), as for period; != and not in included
            codes = [c for c, s in enumerate(self.dynamic[key]) if n.eval({key: s})]
            if not codes:
                self.leaf(_lib.RF_FOP_FALSE)
                return
            words = [0] * ((max(codes) >> 5) + 1)
            for c in codes:
                words[c >> 5] |= 1 << (c & 31)
            self.dynamic_leaf("codeset", key, words)
        elif cls == "boolean":
            bits = sum(1 << int(b) for b in (False, True) if n.eval({key: b}))
            if bits:
                self.dynamic_leaf("bool", key, bits)
            else:
                self.leaf(_lib.RF_FOP_FALSE)
        else:
            self.dynamic_number(n)

    def dynamic_number(self, n: Node) -> None:
        negate = (isinstance(n, DynCmp) and n.op == "!=") or (isinstance(n, DynIn) and n.negate)
        if negate:   # k != v: holds a number, and not k == v (a NaN row passes, a row without a number does not)
            self.dynamic_leaf("tags", n.key, NUMBER_TAGS)
        if isinstance(n, DynCmp):
            op = "==" if negate else n.op
            iv = _int_interval(op, n.value) or (0, -1)   # (ilo > ihi: no int row passes)
            self.dynamic_leaf("nrange", n.key, iv[0], iv[1], *f64_interval(op, n.value))
        else:
            ints = sorted({int(v) for v in n.values if not (isinstance(v, float) and math.isinf(v))
                           and v == math.floor(v) and INT64_MIN <= v <= INT64_MAX})
            floats = sorted({f for f in map(_exact_float, n.values) if f is not None})
            if max(len(ints), len(floats)) > MAX_INT_SET:
                raise ValueError(f"filter expression: {n.key} {'not in' if n.negate else 'in'} [...] holds "
                                 f"{max(len(ints), len(floats))} distinct values, at most {MAX_INT_SET} are taken")
            self.dynamic_leaf("nset", n.key, ints, floats)
        if negate:
            self.leaf(_lib.RF_FOP_NOT)
            self.leaf(_lib.RF_FOP_AND)

    def codeset(self, n: Node) -> None:
        d = self.dicts.get(n.field, ())
        codes = [c for c, s in enumerate(d) if n.eval({n.field: s})]
        if not codes:
            self.leaf(_lib.RF_FOP_FALSE)
            return
        words = [0] * ((max(codes) >> 5) + 1)
        for c in codes:
            words[c >> 5] |= 1 << (c & 31)
        off = len(self.p.code_sets)
        self.p.code_sets.extend(words)
        self.leaf(_lib.RF_FOP_CODESET, COLUMN_OF[n.field], off, len(words))

    def interval(self, op: str, v: float) -> None:
        inf = math.inf
        L, H = _lib.RF_FRANGE_LO_INCL, _lib.RF_FRANGE_HI_INCL
        lo, hi, flags = {"==": (v, v, L | H), "<": (-inf, v, L), "<=": (-inf, v, L | H),
                         ">": (v, inf, H), ">=": (v, inf, L | H)}[op]
        self.leaf(_lib.RF_FOP_RANGE, 3, 0, 0, flags, lo, hi)

    def numeric(self, n: Node) -> None:
        if isinstance(n, Cmp):
            if n.op == "!=":     # NaN != v holds: the negation of an IEEE == test
                self.interval("==", n.value)
                self.leaf(_lib.RF_FOP_NOT)
            else:
                self.interval(n.op, n.value)
            return
        # in / not in: an or-chain of equality tests
        if not n.values:
            self.leaf(_lib.RF_FOP_FALSE)
        for j, v in enumerate(n.values):
            self.interval("==", v)
            if j:
                self.leaf(_lib.RF_FOP_OR)
        if n.negate:
            self.leaf(_lib.RF_FOP_NOT)

    def pk(self, n: Node) -> None:
        keys = [n.value] if isinstance(n, Cmp) else n.values
        rows = sorted({self.pk_row[k] for k in keys if _hashable(k) and k in self.pk_row})
        if rows:
            off = len(self.p.row_lists)
            self.p.row_lists.extend(rows)
            self.leaf(_lib.RF_FOP_ROWLIST, 0, off, len(rows))
        else:
            self.leaf(_lib.RF_FOP_FALSE)
        if (isinstance(n, Cmp) and n.op == "!=") or (isinstance(n, In) and n.negate):
            self.leaf(_lib.RF_FOP_NOT)


def _hashable(k) -> bool:
    try:
        hash(k)
        return True
    except TypeError:
        return False


def compile_expr(node: Node | str, dicts: dict[str, Sequence[str]], pk_row: dict,
                 term_id: dict | None = None, schema=None, extra_dicts: dict | None = None,
                 dynamic: dict | None = None) -> Program:
    """AST (or expression text) -> Program.  dicts: VARCHAR field -> its dictionary (code i =
    dicts[field][i]); pk_row: primary key -> row number; term_id: term -> id in the lexical index's
    dictionary (`Postings.term_id`), None = no lexical index: a keyword leaf raises ValueError.
    schema: the collection's own fields (schema.FieldSchema; None = none); extra_dicts: VARCHAR / BOOL
    field of the schema -> its dictionary of values, code i = extra_dicts[field][i].
    dynamic: None = the collection has no dynamic field; else dynamic key that some row holds -> the
    dictionary of its strings, code i = dynamic[key][i] (a key that is not in it compiles to FALSE)."""
    if isinstance(node, str):
        node = parse(node, schema=schema, dynamic=dynamic is not None)
    c = _Compiler(dicts, pk_row, term_id, schema, extra_dicts, dynamic)
    c.emit(node)
    p = c.p
    if len(p.ops) > _lib.RF_FILTER_MAX_OPS:
        raise ValueError(f"filter expression: compiles to {len(p.ops)} operations, more than the "
                         f"{_lib.RF_FILTER_MAX_OPS} the device program holds")
    if p.max_depth() > _lib.RF_FILTER_MAX_DEPTH:
        raise ValueError(f"filter expression: nests deeper than {_lib.RF_FILTER_MAX_DEPTH} operands")
    return p


def text_leaf_arrays(p: Program):
    """(rf_text_leaf array, the leaves' term ids int32 back to back) of p.text_leaves."""
    arr = (_lib.TextLeaf * len(p.text_leaves))()
    terms: list = []
    for i, (kind, ids, need) in enumerate(p.text_leaves):
        arr[i].kind, arr[i].term_off, arr[i].n_terms, arr[i].min_match = kind, len(terms), len(ids), need
        terms.extend(ids)
    return arr, np.asarray(terms, dtype=np.int32).reshape(-1)


def column_leaf_arrays(p: Program, column_ptr: dict):
    """(rf_column_leaf array, code-set words uint32, value sets int64) of p.column_leaves.  column_ptr: field ->
    the device address of its column."""
    arr = (_lib.ColumnLeaf * len(p.column_leaves))()
    words: list = []
    values: list = []
    for i, leaf in enumerate(p.column_leaves):
        kind, name = leaf[0], leaf[1]
        arr[i].column_dev = column_ptr[name]
        if kind == "codeset":
            arr[i].kind, arr[i].off, arr[i].len = _lib.RF_CLEAF_CODESET, len(words), len(leaf[2])
            words.extend(leaf[2])
        elif kind == "irange":
            arr[i].kind, arr[i].ilo, arr[i].ihi = _lib.RF_CLEAF_I64_RANGE, leaf[2], leaf[3]
        elif kind == "iset":
            arr[i].kind, arr[i].off, arr[i].len = _lib.RF_CLEAF_I64_SET, len(values), len(leaf[2])
            values.extend(leaf[2])
        else:
            arr[i].kind, arr[i].flags, arr[i].flo, arr[i].fhi = _lib.RF_CLEAF_F64_RANGE, leaf[2], leaf[3], leaf[4]
    return arr, np.asarray(words, dtype=np.uint32).reshape(-1), np.asarray(values, dtype=np.int64).reshape(-1)


def column_leaf_reference(leaf, column: np.ndarray) -> np.ndarray:
    """What rf_column_match computes for one entry of Program.column_leaves, in numpy: bool [n].  column: the
    field's device representation (int32 codes | int64 | fp64)."""
    kind = leaf[0]
    if kind == "codeset":
        words = np.asarray(leaf[2], dtype=np.uint32)
        c = column.astype(np.int64)
        ok = (c >= 0) & (c < 32 * words.size)
        w = words[np.clip(c >> 5, 0, words.size - 1)]
        return ok & (((w >> (c & 31).astype(np.uint32)) & 1) == 1)
    if kind == "irange":
        return (column >= np.int64(leaf[2])) & (column <= np.int64(leaf[3])) if leaf[2] <= leaf[3] \
            else np.zeros(column.size, bool)
    if kind == "iset":
        return np.isin(column, np.asarray(leaf[2], dtype=np.int64))
    flags, lo, hi = leaf[2], leaf[3], leaf[4]
    with np.errstate(invalid="ignore"):
        a = column >= lo if flags & _lib.RF_FRANGE_LO_INCL else column > lo
        b = column <= hi if flags & _lib.RF_FRANGE_HI_INCL else column < hi
    return a & b


def encode_array(rows, np_dtype, code: dict | None = None, values_of: list | None = None):
    """The CSR of an ARRAY column's rows (lists): (lengths int64 [n], values np_dtype [sum of lengths]).  With
    `code` (value -> code) the elements are dictionary-coded int32: a new value is appended to `values_of` and
    entered into `code` (first-seen order, as a scalar VARCHAR / BOOL column)."""
    lens = np.fromiter((len(r) for r in rows), dtype=np.int64, count=len(rows))
    flat = [x for r in rows for x in r]
    if code is None:
        return lens, np.asarray(flat, dtype=np_dtype).reshape(-1)
    enc = np.empty(len(flat), dtype=np.int32)
    for j, v in enumerate(flat):
        c = code.get(v)
        if c is None:
            c = code[v] = len(values_of)
            values_of.append(v)
        enc[j] = c
    return lens, enc


_AELEM = {"code": _lib.RF_AELEM_CODE, "i64": _lib.RF_AELEM_I64, "f64": _lib.RF_AELEM_F64}


def array_leaf_arrays(p: Program, column_ptr: dict, leaves=None):
    """(rf_array_leaf array, code-set words uint32, value sets int64, fp64 sets) of p.array_leaves (or of
    `leaves`).  column_ptr: field -> (the device address of its offsets, of its values)."""
    leaves = p.array_leaves if leaves is None else leaves
    arr = (_lib.ArrayLeaf * len(leaves))()
    words: list = []
    values: list = []
    floats: list = []
    for i, leaf in enumerate(leaves):
        kind, name = leaf[0], leaf[1]
        arr[i].offsets_dev, arr[i].values_dev = column_ptr[name]
        if kind == "length":
            arr[i].kind, arr[i].ilo, arr[i].ihi = _lib.RF_ALEAF_LENGTH, leaf[2], leaf[3]
        elif kind == "elem":
            arr[i].kind, arr[i].index = _lib.RF_ALEAF_ELEM, leaf[2]
            sub = leaf[3]
            if sub[0] == "codeset":
                arr[i].elem, arr[i].off, arr[i].len = _lib.RF_CLEAF_CODESET, len(words), len(sub[2])
                words.extend(sub[2])
            elif sub[0] == "irange":
                arr[i].elem, arr[i].ilo, arr[i].ihi = _lib.RF_CLEAF_I64_RANGE, sub[2], sub[3]
            elif sub[0] == "iset":
                arr[i].elem, arr[i].off, arr[i].len = _lib.RF_CLEAF_I64_SET, len(values), len(sub[2])
                values.extend(sub[2])
            else:
                arr[i].elem, arr[i].flags, arr[i].flo, arr[i].fhi = _lib.RF_CLEAF_F64_RANGE, sub[2], sub[3], sub[4]
        else:
            arr[i].kind, arr[i].elem, arr[i].need = _lib.RF_ALEAF_MATCH, _AELEM[leaf[2]], leaf[4]
            sets = floats if leaf[2] == "f64" else values
            arr[i].off, arr[i].len = len(sets), len(leaf[3])
            sets.extend(leaf[3])
    return (arr, np.asarray(words, dtype=np.uint32).reshape(-1), np.asarray(values, dtype=np.int64).reshape(-1),
            np.asarray(floats, dtype=np.float64).reshape(-1))


def array_leaf_reference(leaf, offsets: np.ndarray, values: np.ndarray) -> np.ndarray:
    """What rf_array_match computes for one entry of Program.array_leaves, in numpy: bool [n].  offsets int64
    [n + 1], values: the field's CSR mirror (int32 codes | int64 | fp64)."""
    kind = leaf[0]
    offsets = np.asarray(offsets, dtype=np.int64)
    n = offsets.size - 1
    lens = np.diff(offsets)
    if kind == "length":
        return (lens >= np.int64(leaf[2])) & (lens <= np.int64(leaf[3])) if leaf[2] <= leaf[3] else np.zeros(n, bool)
    if kind == "elem":
        out = np.zeros(n, bool)
        has = lens > leaf[2]
        out[has] = column_leaf_reference(leaf[3], values[offsets[:-1][has] + leaf[2]])
        return out
    needles = np.asarray(leaf[3], dtype=np.float64 if leaf[2] == "f64" else np.int64)
    x = values.astype(needles.dtype, copy=False)
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    if needles.size == 0:
        return np.full(n, leaf[4] <= 0)
    pos = np.searchsorted(needles, x)   # (a NaN element sorts behind every needle)
    hit = pos < needles.size
    hit[hit] = needles[pos[hit]] == x[hit]
    pairs = np.unique(row[hit] * np.int64(needles.size) + pos[hit])   # the distinct (row, needle) pairs
    return np.bincount(pairs // np.int64(needles.size), minlength=n)[:n] >= leaf[4]


def encode_dynamic(values, code: dict, strings: list) -> tuple[np.ndarray, np.ndarray]:
    """The tagged column of a dynamic key's values (None | bool | int | float | str, one per row): (tags uint8
    [n], payload int64 [n]).  payload: the int64, the fp64's bits, a bool as 0 / 1, or the string's code; a new
    string is appended to `strings` and entered into `code` (string -> code: first-seen order)."""
    n = len(values)
    tags = np.zeros(n, dtype=np.uint8)
    payload = np.zeros(n, dtype=np.int64)
    fbits = payload.view(np.float64)
    for j, v in enumerate(values):
        if v is None:
            continue
        if isinstance(v, bool):
            tags[j], payload[j] = _lib.RF_DTAG_BOOL, int(v)
        elif isinstance(v, int):
            tags[j], payload[j] = _lib.RF_DTAG_INT, v
        elif isinstance(v, float):
            tags[j], fbits[j] = _lib.RF_DTAG_DOUBLE, v
        else:
            c = code.get(v)
            if c is None:
                c = code[v] = len(strings)
                strings.append(v)
            tags[j], payload[j] = _lib.RF_DTAG_STRING, c
    return tags, payload


def dynamic_leaf_arrays(p: Program, column_ptr: dict):
    """(rf_dynamic_leaf array, code-set words uint32, int sets int64, fp64 sets) of p.dynamic_leaves.
    column_ptr: key -> (device address of its tags, of its payload)."""
    arr = (_lib.DynamicLeaf * len(p.dynamic_leaves))()
    words: list = []
    ints: list = []
    floats: list = []
    for i, leaf in enumerate(p.dynamic_leaves):
        kind, key = leaf[0], leaf[1]
        arr[i].tags_dev, arr[i].payload_dev = column_ptr[key]
        if kind == "tags":
            arr[i].kind, arr[i].flags = _lib.RF_DLEAF_TAGS, leaf[2]
        elif kind == "codeset":
            arr[i].kind, arr[i].off, arr[i].len = _lib.RF_DLEAF_STR_CODESET, len(words), len(leaf[2])
            words.extend(leaf[2])
        elif kind == "bool":
            arr[i].kind, arr[i].flags = _lib.RF_DLEAF_BOOL, leaf[2]
        elif kind == "nrange":
            arr[i].kind = _lib.RF_DLEAF_NUM_RANGE
            arr[i].ilo, arr[i].ihi, arr[i].flags, arr[i].flo, arr[i].fhi = leaf[2:7]
        else:
            arr[i].kind = _lib.RF_DLEAF_NUM_SET
            arr[i].off, arr[i].len, arr[i].foff, arr[i].flen = len(ints), len(leaf[2]), len(floats), len(leaf[3])
            ints.extend(leaf[2])
            floats.extend(leaf[3])
    return (arr, np.asarray(words, dtype=np.uint32).reshape(-1), np.asarray(ints, dtype=np.int64).reshape(-1),
            np.asarray(floats, dtype=np.float64).reshape(-1))


def dynamic_leaf_reference(leaf, tags: np.ndarray, payload: np.ndarray) -> np.ndarray:
    """What rf_dynamic_match computes for one entry of Program.dynamic_leaves, in numpy: bool [n].  tags uint8
    [n], payload int64 [n]: the key's tagged column (encode_dynamic)."""
    kind = leaf[0]
    tags = np.asarray(tags, dtype=np.uint8)
    payload = np.ascontiguousarray(payload, dtype=np.int64)
    if kind == "tags":
        return (tags < 8) & (((leaf[2] >> np.minimum(tags, 7).astype(np.int64)) & 1) == 1)
    if kind == "codeset":
        words = np.asarray(leaf[2], dtype=np.uint32)
        if words.size == 0:
            return np.zeros(tags.size, bool)
        ok = (tags == _lib.RF_DTAG_STRING) & (payload >= 0) & (payload < 32 * words.size)
        w = words[np.clip(payload >> 5, 0, words.size - 1)]
        return ok & (((w >> (payload & 31).astype(np.uint32)) & 1) == 1)
    if kind == "bool":
        ok = (tags == _lib.RF_DTAG_BOOL) & (payload >= 0) & (payload < 2)
        return ok & (((leaf[2] >> np.clip(payload, 0, 1)) & 1) == 1)
    is_int, is_f64 = tags == _lib.RF_DTAG_INT, tags == _lib.RF_DTAG_DOUBLE
    x = payload.view(np.float64)
    if kind == "nrange":
        ilo, ihi, flags, lo, hi = leaf[2:7]
        i_ok = (payload >= np.int64(ilo)) & (payload <= np.int64(ihi)) if ilo <= ihi else np.zeros(tags.size, bool)
        with np.errstate(invalid="ignore"):
            a = x >= lo if flags & _lib.RF_FRANGE_LO_INCL else x > lo
            b = x <= hi if flags & _lib.RF_FRANGE_HI_INCL else x < hi
        return (is_int & i_ok) | (is_f64 & a & b)
    return (is_int & np.isin(payload, np.asarray(leaf[2], dtype=np.int64))) | \
        (is_f64 & np.isin(x, np.asarray(leaf[3], dtype=np.float64)))


def program_arrays(p: Program) -> tuple[np.ndarray, np.ndarray]:
    """(code-set words uint32, row lists uint32) as contiguous numpy arrays."""
    return (np.asarray(p.code_sets, dtype=np.uint32).reshape(-1),
            np.asarray(p.row_lists, dtype=np.uint32).reshape(-1))
