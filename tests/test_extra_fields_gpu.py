"""User-defined scalar fields on the GPU: rf_column_match against numpy for every leaf kind at the word, wave
and workgroup edges; CorpusStore.filter_rows over a 5 000-row store with all four types against numpy masks;
filtered search against the C oracle on the passing rows; delete / upsert / growth against a fresh store of
the surviving rows; grouping, boosts and per-query filters over extra fields; and one search end to end
through VectorRAG, the tool function and the REST body.  Integers and bits only: every comparison is ==."""
import os
from ctypes import c_void_p

import numpy as np
import pytest

from oracle import encoder as oenc, search as osearch
from rag_fin_amd.ranker import BoostRanker, boost_reference, class_weights
from rag_fin_amd.schema import DataType, FieldSchema
from test_filtered_search_gpu import oracle_on_subset, read_filter

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
COS = {"metric_type": "COSINE"}


# ---- 1. rf_column_match against numpy -----------------------------------------------------------------
def leaf_reference(leaf, col):
    kind = leaf[0]
    if kind == "codeset":
        words = leaf[2]
        return np.array([0 <= int(c) < 32 * len(words) and (words[int(c) >> 5] >> (int(c) & 31)) & 1 == 1 for c in col])
    if kind == "irange":
        return np.array([leaf[2] <= int(x) <= leaf[3] for x in col])
    if kind == "iset":
        return np.isin(col, np.array(leaf[2], dtype=np.int64))
    flags, lo, hi = leaf[2:]
    with np.errstate(invalid="ignore"):
        return (col >= lo if flags & 1 else col > lo) & (col <= hi if flags & 2 else col < hi)


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").astype(bool)[:n]


def run_column_match(device, leaves, columns, n, fill=0xFFFFFFFF):
    """One rf_column_match call through ctypes into a buffer pre-filled with `fill` -> uint32 [L, nwords]."""
    import torch
    from rag_fin_amd import _lib, filter_expr
    lib = _lib.load_library()
    dev = {f: torch.from_numpy(c).to(device) for f, c in columns.items()}
    arr, words, values = filter_expr.column_leaf_arrays(filter_expr.Program(column_leaves=list(leaves)),
                                                        {f: c_void_p(t.data_ptr()) for f, t in dev.items()})
    nwords = (n + 31) // 32
    out = torch.full((len(leaves) * nwords + 8,), fill - (1 << 32), dtype=torch.int32, device=device)
    cs = torch.from_numpy(words.view(np.int32)).to(device) if words.size else None
    vs = torch.from_numpy(values).to(device) if values.size else None
    with torch.cuda.device(device):
        _lib.check(lib.rf_column_match(arr, len(leaves), c_void_p(cs.data_ptr()) if cs is not None else None,
                                       c_void_p(vs.data_ptr()) if vs is not None else None, n, c_void_p(out.data_ptr()),
                                       _lib.current_stream_ptr()))
    torch.cuda.synchronize(device)
    got = out.cpu().numpy().view(np.uint32)
    assert (got[len(leaves) * nwords:] == fill).all()          # nothing past the last leaf's words
    return got[:len(leaves) * nwords].reshape(len(leaves), nwords)


def edge_columns(n, seed):
    rng = np.random.default_rng(seed)
    ints = rng.integers(-50, 50, size=n)
    ints[rng.random(n) < 0.1] = I64_MIN
    ints[rng.random(n) < 0.1] = I64_MAX
    ints[-1] = I64_MAX if n % 2 else I64_MIN
    big = (rng.integers(0, 65536 * 3, size=n) * 5 - 70000).astype(np.int64)   # hits and misses of the 65 536-value set
    dbl = rng.normal(size=n)
    for j, v in enumerate([np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1.0]):
        dbl[j::9][rng.random(dbl[j::9].size) < 0.5] = v
    dbl[-1] = np.nan
    codes = rng.integers(-1, 70, size=n).astype(np.int32)       # -1, 63, 64 and the codes past the set's words
    codes[::5] = (63, 64, -1, 31, 32)[n % 5]
    return {"i": ints.astype(np.int64), "big": big, "d": dbl, "c": codes}


def edge_leaves():
    tiny = 5e-324
    set65536 = [5 * i - 70000 for i in range(65534)] + [I64_MIN, I64_MAX]
    return [
        ("codeset", "c", [0x80000001, 0x80000000]),          # codes 0, 31 and 63 = 32 len - 1; 64 = 32 len is out
        ("codeset", "c", [0xFFFFFFFF]),
        ("irange", "i", 7, 7), ("irange", "i", I64_MIN, I64_MIN), ("irange", "i", I64_MAX, I64_MAX),
        ("irange", "i", 8, 7), ("irange", "i", I64_MIN, I64_MAX), ("irange", "i", -10, I64_MAX),
        ("iset", "i", [3]), ("iset", "i", [I64_MIN, I64_MAX]), ("iset", "big", sorted(set65536)),
        ("iset", "i", [-1000, 1000]),                           # values the column does not hold
        ("frange", "d", 0, -tiny, 1.0), ("frange", "d", 1, 0.0, np.inf), ("frange", "d", 2, -np.inf, -0.0),
        ("frange", "d", 3, -np.inf, np.inf),
    ]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 65_537])
def test_column_match_equals_numpy_at_every_edge(gpu_device, n):
    cols, leaves = edge_columns(n, n), edge_leaves()
    assert len(leaves) == 16 and len(leaves[10][2]) == 65536
    got = run_column_match(gpu_device, leaves, cols, n)
    for l, leaf in enumerate(leaves):
        want = leaf_reference(leaf, cols[leaf[1]])
        assert np.array_equal(unpack(got[l], n), want), (n, leaf[:2])
        assert not unpack(got[l], 32 * got.shape[1])[n:].any()    # the bits past n_rows are zero
    assert unpack(got[15], n).sum() == (~np.isnan(cols["d"])).sum()   # [-inf, inf] passes all but NaN
    for flags in range(4):                                            # all four inclusive-bit combinations, one bound pair
        one = run_column_match(gpu_device, [("frange", "d", flags, -0.0, 1.0)], cols, n, fill=0xA5A5A5A5)
        assert np.array_equal(unpack(one[0], n), leaf_reference(("frange", "d", flags, -0.0, 1.0), cols["d"]))


def test_an_invalid_call_launches_nothing(gpu_device):
    import torch
    from rag_fin_amd import _lib
    lib = _lib.load_library()
    col = torch.zeros(64, dtype=torch.int64, device=gpu_device)
    out = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device=gpu_device)
    bad = []
    for kind, off, ln, flags in [(0, 0, 0, 0), (9, 0, 0, 0), (_lib.RF_CLEAF_I64_SET, 0, 1, 0), (_lib.RF_CLEAF_I64_SET, -1, 1, 0),
                                 (_lib.RF_CLEAF_CODESET, 0, 1, 0), (_lib.RF_CLEAF_F64_RANGE, 0, 0, 8),
                                 (_lib.RF_CLEAF_I64_SET, 0, 65537, 0)]:
        a = (_lib.ColumnLeaf * 1)()
        a[0].kind, a[0].off, a[0].len, a[0].flags, a[0].column_dev = kind, off, ln, flags, col.data_ptr()
        bad.append(lib.rf_column_match(a, 1, None, None, 64, c_void_p(out.data_ptr()), _lib.current_stream_ptr()))
    ok = (_lib.ColumnLeaf * 1)()
    ok[0].kind, ok[0].column_dev = _lib.RF_CLEAF_I64_RANGE, col.data_ptr()
    for n_leaves, n_rows, ptr in [(0, 64, out.data_ptr()), (17, 64, out.data_ptr()), (1, -1, out.data_ptr()),
                                  (1, 64, None), (1, 64, out.data_ptr() + 2)]:
        bad.append(lib.rf_column_match(ok, n_leaves, None, None, n_rows, c_void_p(ptr) if ptr else None,
                                       _lib.current_stream_ptr()))
    torch.cuda.synchronize(gpu_device)
    assert bad == [-1] * len(bad) and (out.cpu().numpy() == 0x5A5A5A5A).all()


# ---- the 5 000-row store with all four types -------------------------------------------------------------
N, D = 5000, 64
FIELDS = [FieldSchema("bank", DataType.VARCHAR), FieldSchema("fiscal_year", DataType.INT64),
          FieldSchema("audited", DataType.BOOL, default=False), FieldSchema("weight", DataType.DOUBLE, default=1.0),
          FieldSchema("period2", DataType.VARCHAR), FieldSchema("page", DataType.INT64, default=0)]
WORDS = ["net", "profit", "rose", "deposits", "fell", "npa", "ratio", "capital"]


def make_table(n, seed=3):
    rng = np.random.default_rng(seed)
    t = {"id": [f"k{i}" for i in range(n)]}
    t["text"] = [" ".join(WORDS[j] for j in rng.integers(len(WORDS), size=rng.integers(2, 7))) for _ in range(n)]
    t["period"] = [f"Q{1 + j}_FY2024" for j in rng.integers(4, size=n)]
    t["chunk_type"] = [("balance_sheet", "key_ratios", "segment")[j] for j in rng.integers(3, size=n)]
    t["statement_type"] = [("consolidated", "standalone")[j] for j in rng.integers(2, size=n)]
    t["primary_value"] = [float(v) for v in rng.normal(size=n).round(2)]
    bank = np.array(["ICICI", "HDFC", "SBI", "AXIS", "KOTAK"])[rng.integers(5, size=n)]
    bank[rng.choice(n, 7, replace=False)] = "RARE"                # 7 rows: fewer than k = 10
    t["bank"] = [str(b) for b in bank]
    fy = rng.integers(2016, 2027, size=n)
    fy[n // 2] = I64_MIN                                          # one row each
    fy[n // 3] = I64_MAX
    t["fiscal_year"] = [int(v) for v in fy]
    t["audited"] = [bool(v) for v in rng.integers(2, size=n)]
    w = rng.normal(size=n).round(1)
    w[::17] = np.nan
    w[5::29] = np.inf
    w[7::31] = -0.0
    t["weight"] = [float(v) for v in w]
    t["period2"] = list(t["period"])
    t["page"] = [int(v) for v in rng.integers(100, size=n)]
    return t


def make_store(device, table, c16, capacity=None, lexical=True):
    import torch
    from rag_fin_amd.store import CorpusStore
    st = CorpusStore("t", dim=D, capacity=capacity or len(table["id"]), device=device, fields=FIELDS)
    st.add(table["id"], table["text"], torch.from_numpy(c16).to(device), table["period"], table["chunk_type"],
           table["statement_type"], table["primary_value"], extra={f.name: table[f.name] for f in FIELDS})
    if lexical:
        st.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
    return st


_WORLD = {}


def world(device):
    if not _WORLD:
        table = make_table(N)
        c16 = osearch.synth_unit_rows(N, D, 21)
        q16 = osearch.synth_unit_rows(3, D, 22)
        _WORLD.update(table=table, c16=c16, q16=q16, st=make_store(device, table, c16),
                      scores=osearch.exact_scores(q16, c16))
    return _WORLD


def arrays(table):
    a = {f: np.array(v) for f, v in table.items() if f not in ("fiscal_year", "page")}
    a["fiscal_year"] = np.array(table["fiscal_year"], dtype=np.int64)
    a["page"] = np.array(table["page"], dtype=np.int64)
    a["has"] = {w: np.array([w in t.split() for t in table["text"]]) for w in WORDS}
    a["phrase"] = np.array([" net profit " in f" {t} " for t in table["text"]])
    return a


# (expression, its mask in numpy over arrays(table))
CASES = [
    ('bank == "ICICI"', lambda a: a["bank"] == "ICICI"),
    ('bank != "ICICI"', lambda a: a["bank"] != "ICICI"),
    ('bank > "ICICI"', lambda a: a["bank"] > "ICICI"),
    ('bank <= "HDFC"', lambda a: a["bank"] <= "HDFC"),
    ('bank in ["SBI", "AXIS", "none"]', lambda a: np.isin(a["bank"], ["SBI", "AXIS"])),
    ('bank not in ["SBI"]', lambda a: a["bank"] != "SBI"),
    ('bank like "%A%"', lambda a: np.char.find(a["bank"], "A") >= 0),
    ('bank like "K%"', lambda a: np.char.startswith(a["bank"], "K")),
    ('bank == "RARE"', lambda a: a["bank"] == "RARE"),
    ('bank == "none"', lambda a: np.zeros(a["bank"].size, bool)),
    ("audited == true", lambda a: a["audited"]),
    ("audited != TRUE", lambda a: ~a["audited"]),
    ("audited in [false]", lambda a: ~a["audited"]),
    ("fiscal_year == 2024", lambda a: a["fiscal_year"] == 2024),
    ("fiscal_year != 2024", lambda a: a["fiscal_year"] != 2024),
    ("2019 <= fiscal_year < 2024", lambda a: (a["fiscal_year"] >= 2019) & (a["fiscal_year"] < 2024)),
    ("fiscal_year > 2023.5", lambda a: a["fiscal_year"] >= 2024),
    ("fiscal_year == 2023.5", lambda a: np.zeros(a["bank"].size, bool)),
    ("fiscal_year != 2023.5", lambda a: np.ones(a["bank"].size, bool)),
    (f"fiscal_year == {I64_MIN}", lambda a: a["fiscal_year"] == I64_MIN),
    (f"fiscal_year >= {I64_MAX}", lambda a: a["fiscal_year"] == I64_MAX),
    ("fiscal_year == 1900", lambda a: np.zeros(a["bank"].size, bool)),
    (f"fiscal_year in [2016, 2026, 1, {I64_MAX}]", lambda a: np.isin(a["fiscal_year"], [2016, 2026, I64_MAX])),
    ("fiscal_year not in [2020, 2021]", lambda a: ~np.isin(a["fiscal_year"], [2020, 2021])),
    ("weight > 0", lambda a: a["weight"] > 0),
    ("weight != 0", lambda a: a["weight"] != 0),               # NaN != 0 holds; -0.0 == 0
    ("weight in [0.5, 1e999]", lambda a: (a["weight"] == 0.5) | (a["weight"] == np.inf)),
    ("-1 < weight <= 0", lambda a: (a["weight"] > -1) & (a["weight"] <= 0)),
    ('bank == "ICICI" and fiscal_year >= 2024', lambda a: (a["bank"] == "ICICI") & (a["fiscal_year"] >= 2024)),
    ('period == "Q1_FY2024" and bank != "SBI" or not audited == true and primary_value > 0.5',
     lambda a: (a["period"] == "Q1_FY2024") & (a["bank"] != "SBI") | ~a["audited"] & (a["primary_value"] > 0.5)),
    ('TEXT_MATCH(text, "npa") and fiscal_year in [2022, 2023]', lambda a: a["has"]["npa"] & np.isin(a["fiscal_year"], [2022, 2023])),
    ('PHRASE_MATCH(text, "net profit") or bank == "RARE"', lambda a: a["phrase"] | (a["bank"] == "RARE")),
    ('TEXT_MATCH(text, "npa capital", minimum_should_match=2) and not (audited == false or weight < 0) and chunk_type like "%ratio%"',
     lambda a: a["has"]["npa"] & a["has"]["capital"] & ~(~a["audited"] | (a["weight"] < 0)) & (a["chunk_type"] == "key_ratios")),
    ('id in ["k3", "k77", "k4999", "zz"] or (page in [5, 50, 99] and statement_type == "standalone")',
     lambda a: np.isin(a["id"], ["k3", "k77", "k4999"]) | (np.isin(a["page"], [5, 50, 99]) & (a["statement_type"] == "standalone"))),
]
MANY = " or ".join(f"page == {j}" for j in range(0, 90, 5))   # 18 column leaves: more than one rf_column_match call
CASES.append((MANY, lambda a: np.isin(a["page"], list(range(0, 90, 5)))))


def masks_of(table):
    a = arrays(table)
    with np.errstate(invalid="ignore"):
        return [(expr, np.asarray(fn(a), dtype=bool)) for expr, fn in CASES]


# ---- 2. filter_rows(expr) equals numpy ----------------------------------------------------------------
def test_filter_rows_equal_numpy(gpu_device):
    w = world(gpu_device)
    assert len(CASES) >= 30
    for expr, mask in masks_of(w["table"]):
        assert np.array_equal(w["st"].filter_rows(expr), np.flatnonzero(mask)), expr
    counts = {e: int(m.sum()) for e, m in masks_of(w["table"])}
    assert counts["fiscal_year == 1900"] == 0 and counts[f"fiscal_year == {I64_MIN}"] == 1 and counts['bank == "RARE"'] == 7


def test_an_extra_copy_of_period_gives_the_built_in_filter_buffer_bit_for_bit(gpu_device):
    st = world(gpu_device)["st"]
    for tail in ('== "Q1_FY2024"', 'in ["Q2_FY2024", "Q4_FY2024"]', 'like "Q3%"', '> "Q2_FY2024"'):
        a = read_filter(st.build_filter("period " + tail), N)
        b = read_filter(st.build_filter("period2 " + tail), N)
        assert int(a[0][1]) > 0 and all(np.array_equal(x, y) for x, y in zip(a, b)), tail
        ta, tb = (st.build_filter(f + " " + tail).cpu().numpy().view(np.uint32) for f in ("period", "period2"))
        n_tiles = int(a[0][3])
        assert np.array_equal(ta[-2048:][:2 * n_tiles], tb[-2048:][:2 * n_tiles])     # the compaction's tile counts


# ---- 3. search(expr=...) equals the oracle on the passing rows ----------------------------------------------
SEARCH_EXPRS = ["fiscal_year == 1900", f"fiscal_year == {I64_MIN}", 'bank == "RARE"', "fiscal_year >= 2020",
                'bank == "ICICI" and audited == true', "weight != 0 and page in [1, 2, 3, 4, 5, 6, 7, 8]"]


def check_searches(st, table, c16, q16, device, exprs=SEARCH_EXPRS, k=10):
    import torch
    lookup = dict(masks_of(table))
    a = arrays(table)
    extra = {"fiscal_year >= 2020": a["fiscal_year"] >= 2020, 'bank == "ICICI" and audited == true': (a["bank"] == "ICICI") & a["audited"],
             "weight != 0 and page in [1, 2, 3, 4, 5, 6, 7, 8]": (a["weight"] != 0) & np.isin(a["page"], range(1, 9))}
    q = torch.from_numpy(q16).to(device)
    for expr in exprs:
        mask = lookup[expr] if expr in lookup else extra[expr]
        es, ei = oracle_on_subset(q16, c16, np.flatnonzero(mask), k)
        scores, ids, exact = st.index.search(q, k, want_exact=True, filt=st.build_filter(expr))
        assert np.array_equal(ids.cpu().numpy(), ei), expr
        assert np.array_equal(exact.cpu().numpy(), es) and np.array_equal(scores.cpu().numpy(), es.astype(np.float32)), expr
        res = st.search(q, "embedding", COS, k, expr=expr, output_fields=["bank", "fiscal_year", "audited", "weight"])
        for b, hits in enumerate(res):
            live = ei[b] >= 0
            assert [h.row for h in hits] == ei[b][live].tolist(), expr
            assert [h.score for h in hits] == [float(np.float32(s)) for s in es[b][live]]
            assert [(h.entity.bank, h.entity.fiscal_year, h.entity.audited) for h in hits] == \
                [(table["bank"][r], table["fiscal_year"][r], table["audited"][r]) for r in ei[b][live]]
    return {e: int((lookup[e] if e in lookup else extra[e]).sum()) for e in exprs}


def test_filtered_search_equals_the_oracle(gpu_device):
    w = world(gpu_device)
    counts = check_searches(w["st"], w["table"], w["c16"], w["q16"], gpu_device)
    assert list(counts.values())[:3] == [0, 1, 7] and counts["fiscal_year >= 2020"] > 2000


# ---- 4. mutation: the store after delete / upsert / growth equals a fresh store of the surviving rows --------
@pytest.mark.parametrize("synced", [True, False])
def test_delete_upsert_and_growth_equal_a_fresh_store(gpu_device, synced):
    import torch
    n = 2000
    table = make_table(n, seed=9)
    c16 = osearch.synth_unit_rows(n + 1500, D, 31)
    q16 = osearch.synth_unit_rows(3, D, 32)
    st = make_store(gpu_device, table, c16[:n], capacity=n)
    if synced:   # the device mirrors of every field follow the delete; else they are built afterwards
        for expr in ('bank == "x"', "fiscal_year == 1", "audited == true", "weight > 0", 'period2 == "x"', "page == 1"):
            st.filter_rows(expr)
        st.search(torch.from_numpy(q16).to(gpu_device), limit=4, group_by_field="page")
    else:
        st.filter_rows('bank == "x"')     # one mirror synced, the others not: both branches of the compaction
        st.add(["late"], ["net"], torch.from_numpy(c16[:1]).to(gpu_device), ["Q9"], ["c"], ["s"], [0.0],
               extra={"bank": ["LATE"], "fiscal_year": [2000], "period2": ["Q9"]})
        st.delete('id == "late"')         # the bank mirror is now behind the rows: dropped, not compacted
        st.filter_rows("fiscal_year == 1")
    assert st.delete("fiscal_year < 2023").delete_count == sum(y < 2023 for y in table["fiscal_year"])
    keep = [i for i in range(n) if table["fiscal_year"][i] >= 2023]
    # upsert: 150 surviving rows replaced (they move to the end), 1 500 new rows: past the capacity
    up = keep[:150]
    new = make_table(1500, seed=10)
    new["id"] = [f"n{i}" for i in range(1500)]
    assert len(keep) + 1500 > n
    rows_up = {f: [table[f][i] for i in up] for f in table}
    rows_up["bank"] = ["UPSERTED"] * 150
    rows_up["fiscal_year"] = [2030] * 150
    batch = {f: rows_up[f] + new[f] for f in table}
    vec = np.concatenate([c16[up], c16[n:]])
    st.upsert([batch["id"], batch["text"], torch.from_numpy(vec).to(gpu_device), batch["period"], batch["chunk_type"],
               batch["statement_type"], batch["primary_value"]] + [batch[f.name] for f in FIELDS])
    assert st.num_entities > n and st.index.capacity > n     # grown past the capacity it was made with
    rest = keep[150:]
    final = {f: [table[f][i] for i in rest] + batch[f] for f in table}
    c_final = np.concatenate([c16[rest], vec])
    assert st.columns["id"] == final["id"] and st.columns["fiscal_year"] == final["fiscal_year"]
    fresh = make_store(gpu_device, final, c_final)
    for expr, mask in masks_of(final):
        got = st.filter_rows(expr)
        assert np.array_equal(got, fresh.filter_rows(expr)) and np.array_equal(got, np.flatnonzero(mask)), expr
    assert np.array_equal(st.filter_rows('bank == "UPSERTED" and fiscal_year == 2030'), np.arange(len(rest), len(rest) + 150))
    check_searches(st, final, c_final, q16, gpu_device)
    q = torch.from_numpy(q16).to(gpu_device)
    for kw in ({"group_by_field": "page", "group_size": 2}, {"group_by_field": "bank"}, {"expr": "audited == true"}):
        a, b = (s.search(q, "embedding", COS, 5, **kw) for s in (st, fresh))
        assert [[(h.id, h.score) for h in r] for r in a] == [[(h.id, h.score) for h in r] for r in b], kw


# ---- 5. the forms that take a field name or a filter ------------------------------------------------------------
def grouped_by_filtered_searches(st, q, field, values, limit, gsize, expr=None):
    """The grouping search's definition: one filtered search per group, merged on the host by the groups' best
    rows (fp64 score desc, row asc)."""
    B = q.shape[0]
    per = []
    for v in values:
        lit = ('"%s"' % v) if isinstance(v, str) else ("true" if v is True else "false" if v is False else repr(v))
        e = f"{field} == {lit}" + (f" and ({expr})" if expr else "")
        s, i, x = st.index.search(q, gsize, want_exact=True, filt=st.build_filter(e))
        per.append((s.cpu().numpy(), i.cpu().numpy(), x.cpu().numpy()))
    out = []
    for b in range(B):
        groups = [(-x[b, 0], int(i[b, 0]), g) for g, (s, i, x) in enumerate(per) if i[b, 0] >= 0]
        flat = []
        for _, _, g in sorted(groups)[:limit]:
            s, i, _ = per[g]
            flat += [(int(r), float(sc), values[g]) for r, sc in zip(i[b], s[b]) if r >= 0]
        out.append(flat)
    return out


@pytest.mark.parametrize("field, limit, gsize, expr", [
    ("period2", 3, 3, None), ("period2", 4, 2, "fiscal_year >= 2022"), ("audited", 2, 5, None),
    ("page", 8, 2, None), ("page", 5, 3, 'bank in ["ICICI", "SBI"]'), ("bank", 6, 1, "audited == false")])
def test_grouping_by_an_extra_field(gpu_device, field, limit, gsize, expr):
    import torch
    from rag_fin_amd import _lib
    w = world(gpu_device)
    st, q = w["st"], torch.from_numpy(w["q16"]).to(gpu_device)
    values = list(dict.fromkeys(w["table"][field]))
    assert len(values) == {"period2": 4, "audited": 2, "page": 100, "bank": 6}[field]
    assert (len(values) > _lib.RF_GROUP_MAX_CODES) == (field == "page")
    res = st.search(q, "embedding", COS, limit, expr=expr, group_by_field=field, group_size=gsize)
    got = [[(h.row, h.score, h.entity.get(field)) for h in hits] for hits in res]
    assert got == grouped_by_filtered_searches(st, q, field, values, limit, gsize, expr)
    assert all(len(r) > gsize for r in got)


def test_grouping_refuses_a_double_field(gpu_device):
    w = world(gpu_device)
    with pytest.raises(ValueError, match="DOUBLE field cannot be grouped by"):
        w["st"].search(w["q16"].astype(np.float32), limit=3, group_by_field="weight")


def test_boost_on_an_extra_field_filter_equals_the_reference(gpu_device):
    import torch
    w = world(gpu_device)
    st, a = w["st"], arrays(w["table"])
    boosts = [BoostRanker('bank == "ICICI"', 1.5), BoostRanker("fiscal_year >= 2024 and audited == true", 0.4)]
    cls = (a["bank"] == "ICICI").astype(np.int64) | (((a["fiscal_year"] >= 2024) & a["audited"]).astype(np.int64) << 1)
    for expr, mask in ((None, None), ("page < 50", a["page"] < 50)):
        want = boost_reference(w["scores"], mask, cls, class_weights(boosts), 10)
        res = st.search(torch.from_numpy(w["q16"]).to(gpu_device), "embedding", COS, 10, expr=expr, ranker=boosts)
        for b, hits in enumerate(res):
            assert [h.row for h in hits] == want[1][b].tolist() and [h.score for h in hits] == [float(x) for x in want[0][b]]


def test_an_expr_list_equals_one_call_per_query(gpu_device):
    import torch
    w = world(gpu_device)
    st, q = w["st"], torch.from_numpy(w["q16"]).to(gpu_device)
    exprs = ['bank == "RARE" or fiscal_year in [2016, 2017]', 'period == "Q1_FY2024"', None]
    res = st.search(q, "embedding", COS, 10, expr=exprs, output_fields=["bank"])
    for b, e in enumerate(exprs):
        one = st.search(q[b:b + 1], "embedding", COS, 10, expr=e, output_fields=["bank"])[0]
        assert [(h.row, h.score, h.entity.bank) for h in res[b]] == [(h.row, h.score, h.entity.bank) for h in one] and len(one) == 10


def test_iterator_range_and_mmr_take_extra_field_filters(gpu_device):
    """An extra-field filter that equals a built-in one (period2 is a copy of period) gives the same hits through
    every form that takes expr; the built-in side of each is covered by that form's own tests."""
    import torch
    w = world(gpu_device)
    st, q = w["st"], torch.from_numpy(w["q16"]).to(gpu_device)
    hits = lambda res: [[(h.row, h.score) for h in r] for r in res]   # noqa: E731
    band = {"metric_type": "COSINE", "params": {"radius": 0.05, "range_filter": 0.3}}
    for kw in ({"param": band}, {"param": COS, "mmr_lambda": 0.5, "mmr_fetch_k": 32}, {"param": COS, "offset": 70}):
        a, b = (st.search(q, "embedding", limit=10, expr=f'{f} == "Q2_FY2024" and fiscal_year > 2018', **kw)
                for f in ("period2", "period"))
        assert hits(a) == hits(b) and all(a), kw
    it = st.search_iterator(q[:1], "embedding", COS, batch_size=40, limit=100, expr="fiscal_year == 2024 and audited == true")
    pages = []
    while True:
        page = it.next()
        if not page:
            break
        pages += [(h.row, h.score) for h in page]
    assert pages == hits(st.search(q[:1], "embedding", COS, 100, expr="fiscal_year == 2024 and audited == true"))[0] and len(pages) == 100
    assert [r["id"] for r in st.query(expr='bank == "RARE"', output_fields=["fiscal_year"])] == \
        [w["table"]["id"][i] for i in range(N) if w["table"]["bank"][i] == "RARE"]


# ---- 6. end to end: VectorRAG, the tool function, the REST body ------------------------------------------------
def test_vector_rag_tool_and_rest_body_with_an_extra_field_expression(gpu_device):
    from rag_fin_amd import adapter, chunker, mcp_server
    from rag_fin_amd.embedder import Embedder
    from rag_fin_amd.rag import VectorRAG
    from rag_fin_amd.service import ingest
    from rag_fin_amd.store import CorpusStore
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    chunks = chunker.build_all_chunks(os.path.join(GOLD, "extract_data"))
    probe = WordPieceTokenizer(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"])
    words = sorted({w for c in chunks for w in probe.basic_tokens(c["text"])})
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words + list("abcdefghijklmnopqrstuvwxyz0123456789")
    tok = WordPieceTokenizer(list(dict.fromkeys(vocab)))
    cfg = dict(oenc.MINILM_L6, vocab_size=len(tok.vocab))
    emb = Embedder(oenc.random_weights(cfg, 42), cfg, tokenizer=tok, device=gpu_device)
    fields = [FieldSchema("bank", DataType.VARCHAR), FieldSchema("fiscal_year", DataType.INT64)]
    store = CorpusStore("fin_chunks", dim=384, capacity=16, device=gpu_device, fields=fields)
    half = len(chunks) // 2   # a second bank's statements: the same chunks under other ids, a year earlier
    other = [dict(c, id=f"hdfc-{c['id']}") for c in chunks[:half]]
    year = lambda c: 2000 + int(c["period"][-2:])   # noqa: E731
    ingest(store, emb, chunks, field_values={"bank": "ICICI", "fiscal_year": year})
    ingest(store, emb, other, field_values={"bank": "HDFC", "fiscal_year": lambda c: year(c) - 1})
    rag = VectorRAG("no-key", "fin_chunks", embedder=emb, store=store, extra_output_fields=["bank", "fiscal_year"])
    expr = 'bank == "ICICI" and fiscal_year >= 2024'
    q = "net profit in Q3 FY2024"
    mask = np.array([b == "ICICI" and y >= 2024 for b, y in zip(store.columns["bank"], store.columns["fiscal_year"])])
    assert 3 <= mask.sum() < store.num_entities
    got = rag.search(q, 3, expr=expr)
    assert len(got) == 3 and all(c["bank"] == "ICICI" and c["fiscal_year"] >= 2024 for c in got)
    q16 = emb.encode_to_device([q])
    c16 = store.index.get_rows(np.arange(store.num_entities)).cpu().numpy()
    es, ei = oracle_on_subset(q16.cpu().numpy(), c16, np.flatnonzero(mask), 3)
    assert [c["text"] for c in got] == [store.columns["text"][r] for r in ei[0]]
    assert [c["score"] for c in got] == [float(np.float32(s)) for s in es[0]]
    assert "bank" not in VectorRAG("no-key", "fin_chunks", embedder=emb, store=store).search(q, 1, expr=expr)[0]
    mcp_server.set_rag(rag)
    try:
        r = mcp_server.search_vectors(q, 3, filter=expr)
        assert r["status"] == "success" and [c["text"] for c in r["results"]] == [c["text"] for c in got]
        args = adapter.search_args(adapter.SearchRequest(query=q, top_k=3, filter=expr))   # the body of POST /search
        r = mcp_server.search_vectors(**args)
        assert r["status"] == "success" and [(c["text"], c["score"]) for c in r["results"]] == [(c["text"], c["score"]) for c in got]
        assert mcp_server.search_vectors(q, 3, filter="fiscal_year >= 9223372036854775808")["status"] == "error"
    finally:
        mcp_server.set_rag(None)
