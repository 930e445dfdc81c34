"""User-defined fields of a collection: `CorpusStore(..., fields=[FieldSchema(...), ...])`.

The reference's collection has seven fields ("chunking_storing (1).py":14-22); a pymilvus user declares
further `FieldSchema`s of their own, and `DataType` / `FieldSchema` here take pymilvus' shape for the four
scalar types this store serves: VARCHAR, INT64, DOUBLE and BOOL, and for ARRAY fields of those:
`FieldSchema("tags", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=16)` -- a row holds a list of
0 .. max_capacity (at most MAX_CAPACITY = 4096, Milvus' limit) elements of the one element type.  JSON and
nullable fields are not offered.

Dynamic fields (`CorpusStore(..., enable_dynamic_field=True)`, pymilvus' `$meta`): a row may carry keys that
no FieldSchema declares.  A key is any non-empty string, a collection holds at most MAX_DYNAMIC_KEYS distinct
ones, and a row holds under a key a bool, an int in the int64 range, a float (NaN and +-inf allowed) or a str
-- or lacks the key (None).  Lists, dicts and everything else are refused (`check_dynamic`).
"""
from __future__ import annotations

import enum
import numbers
import re
from typing import Any, Iterable, Sequence

import numpy as np

MAX_FIELDS = 32
MAX_DYNAMIC_KEYS = 64   # distinct dynamic keys of one collection
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1

# the reference's seven fields, the vector fields this store derives, and the words of the expression grammar
REFERENCE_FIELDS = ("id", "text", "embedding", "period", "chunk_type", "statement_type", "primary_value")
RESERVED = REFERENCE_FIELDS + ("sparse", "sparse_embedding", "token_embeddings")
_KEYWORDS = ("and", "or", "not", "in", "like", "true", "false", "text_match", "phrase_match")
_IDENT = re.compile(r"^[A-Za-z_][A-Za-z0-9_]*$")


MAX_CAPACITY = 4096     # elements of one row of an ARRAY field (Milvus' limit)


class DataType(enum.IntEnum):
    """pymilvus' numbering, for the types offered.  The enum's members are the element / scalar types: what a
    scalar field holds and what an ARRAY field's elements are.  `DataType.ARRAY` (22, pymilvus' number) is an
    attribute of the class and no member -- iterating DataType yields the four scalar types only."""
    BOOL = 1
    INT64 = 5
    DOUBLE = 11
    VARCHAR = 21


class _ArrayType(int):
    """DataType.ARRAY: an int (22) with the `name` a member has."""
    name = "ARRAY"

    def __repr__(self):
        return "<DataType.ARRAY: 22>"


DataType.ARRAY = _ArrayType(22)   # (set after the class body: an attribute, not a member)


def _data_type(dtype):
    """DataType.ARRAY or a member of DataType for a name or pymilvus' number; KeyError / ValueError / TypeError."""
    if isinstance(dtype, str):
        return DataType.ARRAY if dtype.upper() == "ARRAY" else DataType[dtype.upper()]
    return DataType.ARRAY if int(dtype) == DataType.ARRAY else DataType(int(dtype))


class FieldSchema:
    """One extra field: its name (an identifier), its DataType and, optionally, the value a row takes
    when an insert does not supply the column.  An ARRAY field also names its element_type (VARCHAR, INT64,
    DOUBLE or BOOL) and its max_capacity (1..MAX_CAPACITY elements per row), both required; its default is a
    list ([] included).  A scalar field takes neither."""

    def __init__(self, name: str, dtype, default: Any = None, element_type=None, max_capacity=None, **_ignored):
        if not isinstance(name, str) or not _IDENT.match(name):
            raise ValueError(f"field name {name!r} is not an identifier")
        if name.lower() in _KEYWORDS:
            raise ValueError(f"field name {name!r} is a word of the expression grammar")
        try:
            dtype = _data_type(dtype)
        except (KeyError, ValueError, TypeError):
            raise ValueError(f"field {name!r}: dtype {dtype!r} is not supported (VARCHAR, INT64, DOUBLE, BOOL or "
                             "ARRAY of those; JSON and vector fields cannot be declared)") from None
        self.name = name
        self.dtype = dtype
        self.element_type = self.max_capacity = None
        if dtype == DataType.ARRAY:
            if element_type is None or max_capacity is None:
                raise ValueError(f"field {name!r}: an ARRAY field needs element_type and max_capacity")
            try:
                element_type = _data_type(element_type)
                if element_type == DataType.ARRAY:
                    raise ValueError
            except (KeyError, ValueError, TypeError):
                raise ValueError(f"field {name!r}: element_type {element_type!r} is not supported (VARCHAR, INT64, "
                                 "DOUBLE or BOOL)") from None
            if isinstance(max_capacity, bool) or not isinstance(max_capacity, (int, np.integer)) or \
                    not 1 <= max_capacity <= MAX_CAPACITY:
                raise ValueError(f"field {name!r}: max_capacity must be an integer in 1..{MAX_CAPACITY}, got {max_capacity!r}")
            self.element_type, self.max_capacity = element_type, int(max_capacity)
        elif element_type is not None or max_capacity is not None:
            raise ValueError(f"field {name!r}: element_type and max_capacity belong to an ARRAY field, {dtype.name} is scalar")
        self.default = None if default is None else check_value(self, default, "default")

    def to_dict(self) -> dict:
        d = {"name": self.name, "dtype": self.dtype.name}
        if self.is_array:
            d["element_type"], d["max_capacity"] = self.element_type.name, self.max_capacity
        if self.default is not None:
            d["default"] = self.default   # (json spells NaN / Infinity, as it does for primary_value)
        return d

    @classmethod
    def from_dict(cls, d: dict) -> "FieldSchema":
        default = d.get("default")
        if d["dtype"] == "ARRAY":
            if default is not None and d.get("element_type") == "DOUBLE":
                default = [float(v) for v in default]
            return cls(d["name"], d["dtype"], default, element_type=d.get("element_type"),
                       max_capacity=d.get("max_capacity"))
        if default is not None and DataType[d["dtype"]] == DataType.DOUBLE:
            default = float(default)
        return cls(d["name"], d["dtype"], default)

    @property
    def is_array(self) -> bool:
        return self.dtype == DataType.ARRAY

    def __eq__(self, other):
        return isinstance(other, FieldSchema) and self.to_dict() == other.to_dict()

    def __repr__(self):
        return f"FieldSchema({self.name!r}, DataType.{self.dtype.name}" + \
            (f", element_type=DataType.{self.element_type.name}, max_capacity={self.max_capacity}" if self.is_array else "") + \
            ("" if self.default is None else f", default={self.default!r}") + ")"


def check_value(field: FieldSchema, v, where: str = "value"):
    """`v` as the field stores it (str / int / float / bool; a list of those for an ARRAY field), or ValueError."""
    t = field.dtype
    if t == DataType.ARRAY:
        return check_array(field, v, where)
    return _check_scalar(field.name, t, v, where)


def check_array(field: FieldSchema, v, where: str = "value") -> list:
    """A row of an ARRAY field as stored: a list of at most max_capacity elements, each as the element type's
    scalar check leaves it (bool is no int, the int64 range applies).  v: a list, a tuple or a 1-D numpy array."""
    if isinstance(v, np.ndarray) and v.ndim == 1:
        v = v.tolist()
    if not isinstance(v, (list, tuple)):
        raise ValueError(f"field {field.name!r} is ARRAY, {where} {v!r} ({type(v).__name__}) is not a list")
    if len(v) > field.max_capacity:
        raise ValueError(f"field {field.name!r}: {where} holds {len(v)} elements, max_capacity is {field.max_capacity}")
    return [_check_scalar(field.name, field.element_type, x, "element", "an ARRAY of ") for x in v]


def _check_scalar(name: str, t, v, where: str, of: str = ""):
    if t == DataType.VARCHAR:
        if isinstance(v, str):
            return v
    elif t == DataType.BOOL:
        if isinstance(v, (bool, np.bool_)):
            return bool(v)
    elif t == DataType.INT64:
        if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)):
            if not INT64_MIN <= int(v) <= INT64_MAX:
                raise ValueError(f"field {name!r}: {where} {v!r} is outside the int64 range")
            return int(v)
    else:
        if isinstance(v, (numbers.Real, np.floating, np.integer)) and not isinstance(v, (bool, np.bool_)):
            return float(v)
    raise ValueError(f"field {name!r} is {of}{t.name}, {where} {v!r} ({type(v).__name__}) is not")


def check_fields(fields: Iterable | None) -> tuple:
    """The declared extra fields as a tuple of FieldSchema, or ValueError: at most MAX_FIELDS, and no name that
    collides with the reference's fields, the derived vector fields or another declared field."""
    out = []
    for f in fields or ():
        if isinstance(f, dict):
            f = FieldSchema.from_dict(f)
        if not isinstance(f, FieldSchema):
            raise ValueError(f"fields takes FieldSchema objects, got {type(f).__name__}")
        if f.name in RESERVED:
            raise ValueError(f"field name {f.name!r} collides with a field of the collection")
        if any(f.name == g.name for g in out):
            raise ValueError(f"field name {f.name!r} is declared twice")
        out.append(f)
    if len(out) > MAX_FIELDS:
        raise ValueError(f"{len(out)} extra fields declared, at most {MAX_FIELDS} are taken")
    return tuple(out)


def check_columns(fields: Sequence[FieldSchema], extra: dict | None, n: int, what: str = "insert") -> list:
    """The extra columns of a batch of n rows, in schema order and as stored; a column that is not supplied is
    filled with the field's default.  ValueError: an unknown name, a length other than n, a value of the wrong
    type, a missing column of a field without a default.  Nothing is changed."""
    extra = dict(extra or {})
    names = [f.name for f in fields]
    for name in extra:
        if name not in names:
            raise ValueError(f"{what}: unknown extra field {name!r}" + (f" (declared: {', '.join(names)})" if names else
                                                                       " (the collection declares none)"))
    cols = []
    for f in fields:
        if f.name not in extra or extra[f.name] is None:
            if f.default is None:
                raise ValueError(f"{what}: field {f.name!r} has no default and no column was supplied")
            cols.append([list(f.default) for _ in range(n)] if f.is_array else [f.default] * n)
            continue
        col = extra[f.name]
        if f.is_array and not isinstance(col, (list, tuple, np.ndarray)):
            raise ValueError(f"{what}: the column of ARRAY field {f.name!r} is a list of lists, got {type(col).__name__}")
        col = list(col)
        if len(col) != n:
            raise ValueError(f"{what} columns differ in length (field {f.name!r}: {len(col)} values for {n} rows)")
        cols.append([check_value(f, v) for v in col])
    return cols


def column_from_json(field: FieldSchema, values) -> list:
    if field.is_array:
        if field.element_type == DataType.DOUBLE:   # (json spells 3.0 as 3.0, but a whole number may come back an int)
            values = [[float(x) for x in v] if isinstance(v, list) else v for v in values]
        return [check_array(field, v) for v in values]
    if field.dtype == DataType.DOUBLE:
        return [float(v) for v in values]
    return [check_value(field, v) for v in values]


def dynamic_value(key: str, v):
    """`v` as a dynamic key stores it (None = the row lacks the key | bool | int | float | str), or ValueError."""
    if v is None or isinstance(v, str):
        return v
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        if not INT64_MIN <= int(v) <= INT64_MAX:
            raise ValueError(f"dynamic field {key!r}: value {v!r} is outside the int64 range")
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    raise ValueError(f"dynamic field {key!r}: value {v!r} ({type(v).__name__}) is not a bool, an int, a float, a str "
                     "or None (nested and ARRAY / JSON values are not supported)")


def check_dynamic(columns: dict | None, n: int, held: Iterable[str] = (), what: str = "insert") -> dict:
    """The dynamic columns of a batch of n rows as stored, {key: n values}; a key whose every value is None is
    dropped.  ValueError: a key that is no non-empty string, a length other than n, a value dynamic_value
    refuses, more than MAX_DYNAMIC_KEYS distinct keys together with `held` (the collection's).  Nothing is
    changed."""
    out = {}
    for key, col in (columns or {}).items():
        if not isinstance(key, str) or key == "":
            raise ValueError(f"{what}: a dynamic key is a non-empty string, got {key!r}")
        col = [None] * n if col is None else list(col)
        if len(col) != n:
            raise ValueError(f"{what} columns differ in length (dynamic field {key!r}: {len(col)} values for {n} rows)")
        col = [dynamic_value(key, v) for v in col]
        if any(v is not None for v in col):
            out[key] = col
    total = len(set(held) | set(out))
    if total > MAX_DYNAMIC_KEYS:
        raise ValueError(f"{what}: {total} distinct dynamic keys, a collection holds at most {MAX_DYNAMIC_KEYS}")
    return out


def dynamic_columns_of_rows(rows, n: int, what: str = "insert") -> dict:
    """The $meta column of a column-major insert -- n dicts (or None), one per row -- as {key: n values}."""
    rows = [None] * n if rows is None else list(rows)
    if len(rows) != n:
        raise ValueError(f"{what} columns differ in length ($meta: {len(rows)} values for {n} rows)")
    out: dict = {}
    for j, meta in enumerate(rows):
        if meta is None:
            continue
        if not isinstance(meta, dict):
            raise ValueError(f"{what}: the $meta column holds one dict (or None) per row, got {type(meta).__name__}")
        for key, v in meta.items():
            if not isinstance(key, str) or key == "":   # (before it becomes a dict key of its own)
                raise ValueError(f"{what}: a dynamic key is a non-empty string, got {key!r}")
            out.setdefault(key, [None] * n)[j] = v
    return out
