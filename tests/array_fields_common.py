"""What tests/test_array_fields_cpu.py and tests/test_array_fields_gpu.py share: the 5 000-row table with ARRAY
fields of all four element types beside two scalar fields and a dynamic key, the expressions the GPU store test
filters by (the CPU test asserts that each non-constant one passes between 1 % and 99 % of the rows, so an all-zero
or all-one bitmap cannot pass on the GPU), and the row-by-row evaluation of an expression's AST."""
import numpy as np

from rag_fin_amd import filter_expr
from rag_fin_amd.schema import DataType, FieldSchema

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
N = 5000
VOCAB = ["npa", "nim", "casa", "roe", "roa", "car", "pcr", "slr", "crr", "eps", "gnpa", "nnpa"]   # 12 tags
WORDS = ["net", "profit", "rose", "deposits", "fell", "npa", "ratio", "capital"]
FIELDS = [FieldSchema("tags", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=16, default=[]),
          FieldSchema("years", DataType.ARRAY, element_type=DataType.INT64, max_capacity=8),
          FieldSchema("weights", DataType.ARRAY, element_type=DataType.DOUBLE, max_capacity=8),
          FieldSchema("flags", DataType.ARRAY, element_type=DataType.BOOL, max_capacity=8),
          FieldSchema("bank", DataType.VARCHAR), FieldSchema("fiscal_year", DataType.INT64)]
DYNAMIC_KEY = "pages"
NAN, INF = float("nan"), float("inf")

# the hand-made rows: (tags, years, weights, flags)
EDGE_ROWS = [
    ([], [], [], []),
    (["npa"], [2020], [0.5], [True]),
    (["npa", "npa"], [2020, 2020], [0.5, 0.5], [True, True]),                 # duplicates: one distinct value
    (["nim", "npa"], [2021, 2020], [-0.0, NAN], [False, True]),
    (["npa", "nim", "casa", "roe", "roa", "car"], [2015, 2016, 2017, 2018, 2019, 2020], [NAN] * 6, [False] * 6),
    (list(VOCAB), [I64_MIN, I64_MAX], [INF, -INF], [True, False, True]),      # every tag; the int64 extremes
    (["zzz"], [0], [0.0], [False]),                                           # a tag outside the vocabulary
    (["casa"] * 16, [2030] * 8, [1.0] * 8, [True] * 8),                       # at capacity
    ([""], [-1], [5e-324], []),
    (["nim"], [I64_MAX], [NAN], [True]),
]


def make_table(n=N, seed=5):
    """Tags from the 12-word vocabulary, lengths uniform 0..6, int arrays from 2015..2030; the first 50 rows are
    the hand-made edge rows, five times over."""
    rng = np.random.default_rng(seed)
    t = {"id": [f"k{i}" for i in range(n)]}
    t["text"] = [" ".join(WORDS[j] for j in rng.integers(len(WORDS), size=rng.integers(2, 7))) for _ in range(n)]
    t["period"] = [f"Q{1 + j}_FY2024" for j in rng.integers(4, size=n)]
    t["chunk_type"] = [("balance_sheet", "key_ratios", "segment")[j] for j in rng.integers(3, size=n)]
    t["statement_type"] = [("consolidated", "standalone")[j] for j in rng.integers(2, size=n)]
    t["primary_value"] = [float(v) for v in rng.normal(size=n).round(2)]
    dbl = [0.0, -0.0, 0.5, -0.5, 1.0, 2.5, NAN, INF]
    t["tags"] = [[VOCAB[j] for j in rng.integers(len(VOCAB), size=rng.integers(0, 7))] for _ in range(n)]
    t["years"] = [[int(v) for v in rng.integers(2015, 2031, size=rng.integers(0, 7))] for _ in range(n)]
    t["weights"] = [[dbl[j] for j in rng.integers(len(dbl), size=rng.integers(0, 7))] for _ in range(n)]
    t["flags"] = [[bool(v) for v in rng.integers(2, size=rng.integers(0, 7))] for _ in range(n)]
    for j in range(min(n, 50)):
        e = EDGE_ROWS[j % len(EDGE_ROWS)]
        t["tags"][j], t["years"][j], t["weights"][j], t["flags"][j] = (list(x) for x in e)
    t["bank"] = [("ICICI", "HDFC", "SBI", "AXIS", "KOTAK")[j] for j in rng.integers(5, size=n)]
    t["fiscal_year"] = [int(v) for v in rng.integers(2016, 2027, size=n)]
    # the dynamic key: an int on two rows of three, a string on some, absent on the rest
    pages = rng.integers(100, size=n)
    t[DYNAMIC_KEY] = [None if i % 3 == 0 else ("cover" if i % 31 == 0 else int(pages[i])) for i in range(n)]
    return t


# (expression, constant: None = passes between 1 % and 99 % of the rows | True | False)
_MANY = " or ".join(f'tags[{i % 6}] == "{VOCAB[i % 12]}"' for i in range(18))   # 18 array leaves: two launches
STORE_EXPRS = [(e, None) for e in [
    'ARRAY_CONTAINS(tags, "npa")', 'array_contains(tags, "nnpa")', 'ARRAY_CONTAINS_ALL(tags, ["npa", "nim"])',
    'ARRAY_CONTAINS_ALL(tags, ["npa", "npa"])', 'Array_Contains_Any(tags, ["casa", "roe", "none"])',
    "ARRAY_LENGTH(tags) == 0", "array_length(tags) != 0", "2 <= ARRAY_LENGTH(tags) < 5", "5 < ARRAY_LENGTH(tags)",
    'tags[0] == "npa"', 'tags[0] != "npa"', 'tags[5] != "npa"', 'tags[1] like "n%"', 'tags[0] in ["npa", "nim"]',
    'tags[2] not in ["npa"]', '"c" < tags[0] <= "n"', 'not (tags[3] == "npa")',
    "ARRAY_CONTAINS(years, 2020)", "ARRAY_CONTAINS(years, 2020.0)", "ARRAY_CONTAINS_ALL(years, [2020, 2021])",
    "ARRAY_CONTAINS_ANY(years, [2015, 2.5, 1e30, 2016])", f"ARRAY_CONTAINS_ANY(years, [{I64_MIN}, {I64_MAX}, 2029])",
    "years[0] >= 2025", "years[1] != 2020", "2018 < years[0] <= 2022", "years[0] not in [2015, 2016]",
    "years[2] in [2020, 2021, 2022]", "years[0] > 2019.5", "not (years[4] != 2020)",
    "ARRAY_CONTAINS(weights, 0)", "ARRAY_CONTAINS_ANY(weights, [0.5, 1e999])", "ARRAY_CONTAINS_ALL(weights, [0.5, 1])",
    "weights[0] > 0", "weights[0] != 0.5", "not (weights[0] == 0.5)", "weights[1] in [0.5, -0.5]",
    "weights[1] not in [0.5]", "-1 < weights[0] <= 0",
    "ARRAY_CONTAINS(flags, true)", "ARRAY_CONTAINS_ALL(flags, [true, false])", "flags[0] == false", "flags[0] != TRUE",
    "flags[2] in [true]", "ARRAY_LENGTH(flags) <= 1",
    'ARRAY_CONTAINS(tags, "npa") and bank == "ICICI"', 'not ARRAY_CONTAINS(tags, "npa") or fiscal_year >= 2024',
    'ARRAY_CONTAINS(tags, "nim") and pages > 10', 'ARRAY_LENGTH(years) >= 3 and (pages == "cover" or not exists pages)',
    'TEXT_MATCH(text, "npa") and ARRAY_LENGTH(tags) > 2', 'PHRASE_MATCH(text, "net profit") or tags[0] == "casa"',
    'period == "Q1_FY2024" and ARRAY_CONTAINS_ANY(years, [2016, 2017]) and not (flags[0] == true) or id in ["k7", "k4999"]',
    _MANY,
]] + [
    ("ARRAY_CONTAINS_ALL(tags, [])", True), ("ARRAY_CONTAINS_ANY(tags, [])", False),
    ('ARRAY_CONTAINS_ALL(tags, ["npa", "no such tag"])', False), ("ARRAY_LENGTH(tags) < 0", False),
    ("ARRAY_CONTAINS(years, 2.5)", False), ("ARRAY_LENGTH(years) >= 0", True),
]


def parse(expr):
    return filter_expr.parse(expr, schema=FIELDS, dynamic=True)


def ast_mask(expr, table):
    """The rows `expr` passes by the AST's host semantics: bool [n]."""
    node = parse(expr)
    n = len(table["id"])
    return np.array([node.eval({f: c[r] for f, c in table.items()}) for r in range(n)], dtype=bool)
