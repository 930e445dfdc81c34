"""Dynamic fields on the GPU: rf_dynamic_match against a row-by-row reference for every leaf kind at the word,
wave and workgroup edges; CorpusStore.filter_rows over a 3 000-row store whose keys mix all five tags against the
AST's semantics for the CPU test's expression list; filtered search against the C oracle on the passing rows; a
dynamic copy of `period` against the built-in filter buffer; delete / upsert / growth against a fresh store;
per-query filters, boosts, the iterator, range and MMR forms; save / load_from; and one search end to end through
VectorRAG, the tool function and the REST body.  Integers and bits only: every comparison is ==."""
import math
import os
import struct
from ctypes import c_void_p

import numpy as np
import pytest

from oracle import encoder as oenc, search as osearch
from rag_fin_amd.ranker import BoostRanker, boost_reference, class_weights
from test_dynamic_fields_cpu import FIELDS, LEAF_EXPRS, MIXED_EXPRS, P53, mixed_table, same
from test_filtered_search_gpu import oracle_on_subset, read_filter

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
COS = {"metric_type": "COSINE"}
ABSENT, BOOL, INT, DOUBLE, STRING = range(5)


# ---- 1. rf_dynamic_match against a row-by-row reference ------------------------------------------------------
def as_double(bits):
    return struct.unpack("<d", struct.pack("<q", bits))[0]


def row_passes(leaf, tag, p):
    """The contract of include/ragfin.h for one row: tag, and the payload p as a signed 64-bit integer."""
    kind = leaf[0]
    if kind == "tags":
        return bool((leaf[2] >> tag) & 1)
    if kind == "codeset":
        words = leaf[2]
        return tag == STRING and 0 <= p < 32 * len(words) and (words[p >> 5] >> (p & 31)) & 1 == 1
    if kind == "bool":
        return tag == BOOL and p in (0, 1) and (leaf[2] >> p) & 1 == 1
    if kind == "nrange":
        ilo, ihi, flags, lo, hi = leaf[2:7]
        if tag == INT:
            return ilo <= p <= ihi
        if tag != DOUBLE:
            return False
        x = as_double(p)
        return (x >= lo if flags & 1 else x > lo) and (x <= hi if flags & 2 else x < hi)
    if tag == INT:
        return p in leaf[4]
    return tag == DOUBLE and as_double(p) in leaf[5]   # (a Python set: NaN is in none, -0.0 == 0.0 hashes alike)


def with_sets(leaves):
    return [leaf + (set(leaf[2]), set(leaf[3])) if leaf[0] == "nset" else leaf for leaf in leaves]


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").astype(bool)[:n]


def run_dynamic_match(device, leaves, tags, payload, n, fill=0xFFFFFFFF):
    """One rf_dynamic_match call through ctypes into a buffer pre-filled with `fill` -> uint32 [L, nwords]."""
    import torch
    from rag_fin_amd import _lib, filter_expr
    lib = _lib.load_library()
    t_d, p_d = torch.from_numpy(tags).to(device), torch.from_numpy(payload).to(device)
    arr, words, ints, floats = filter_expr.dynamic_leaf_arrays(filter_expr.Program(dynamic_leaves=[l[:4 if l[0] == "nset" else None] for l in leaves]),
                                                               {"c": (t_d.data_ptr(), p_d.data_ptr())})
    nwords = (n + 31) // 32
    out = torch.full((len(leaves) * nwords + 8,), fill - (1 << 32), dtype=torch.int32, device=device)
    sets = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device) if a.size else None for a in (words, ints, floats)]
    with torch.cuda.device(device):
        _lib.check(lib.rf_dynamic_match(arr, len(leaves), *[c_void_p(s.data_ptr()) if s is not None else None for s in sets], n,
                                        c_void_p(out.data_ptr()), _lib.current_stream_ptr()))
    torch.cuda.synchronize(device)
    got = out.cpu().numpy().view(np.uint32)
    assert (got[len(leaves) * nwords:] == fill).all()          # nothing past the last leaf's words
    return got[:len(leaves) * nwords].reshape(len(leaves), nwords)


EXTREME_INTS = [0, 1, 3, -1, P53 - 1, P53, P53 + 1, -P53 - 1, -P53, I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1]
EXTREME_F64 = [math.nan, math.inf, -math.inf, -0.0, 0.0, 5e-324, -5e-324, 3.0, 2.5, float(P53), float(P53 + 2), -float(P53),
               float(1 << 63), -float(1 << 63), 1.7976931348623157e308]


def edge_column(n, seed, only=None):
    """(tags uint8 [n], payload int64 [n]): every wave of 64 rows holds every tag (the tag pattern shifts by one per
    wave), or `only` that tag.  Absent rows carry payload bits that would pass if they were read."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    tags = ((i + i // 64) % 5).astype(np.uint8) if only is None else np.full(n, only, dtype=np.uint8)
    payload = np.zeros(n, dtype=np.int64)
    ints = np.where(rng.random(n) < 0.5, rng.integers(-6, 6, size=n), np.array(EXTREME_INTS, dtype=np.int64)[rng.integers(len(EXTREME_INTS), size=n)])
    dbl = np.where(rng.random(n) < 0.4, rng.integers(-6, 6, size=n) / 2.0, np.array(EXTREME_F64)[rng.integers(len(EXTREME_F64), size=n)])
    set_hits = rng.integers(0, 3 * 4096, size=n) * 5 - 10000        # hits and misses of the 4 096-value sets
    ints = np.where(rng.random(n) < 0.3, set_hits, ints)
    dbl = np.where(rng.random(n) < 0.3, set_hits + 0.5, dbl)
    codes = rng.integers(0, 70, size=n)                              # 63, 64 and the codes past the set's words
    codes[::7] = (63, 64, 0, 31, 32)[n % 5]
    payload[tags == ABSENT] = 3                                      # an int 3, a code 3, "true"-ish: never read
    payload[tags == BOOL] = rng.integers(0, 2, size=n)[tags == BOOL]
    payload[tags == INT] = ints[tags == INT]
    payload[tags == DOUBLE] = dbl.astype(np.float64).view(np.int64)[tags == DOUBLE]
    payload[tags == STRING] = codes[tags == STRING]
    return tags, payload


def edge_leaves():
    from rag_fin_amd.filter_expr import f64_interval, int_interval
    inf = math.inf
    nr = lambda op, v: ("nrange", "c") + (int_interval(op, v) or (0, -1)) + f64_interval(op, v)   # noqa: E731
    big = [5 * j - 10000 for j in range(4094)] + [I64_MIN, I64_MAX]
    return [
        ("tags", "c", 0b11110), ("tags", "c", 0b01100), ("tags", "c", 0b00001), ("tags", "c", 0),
        ("codeset", "c", [0x80000001, 0x80000000]),     # codes 0, 31 and 63 = 32 len - 1; 64..69 lie past the set's words
        ("codeset", "c", []),                           # a set of length 0 passes nothing
        ("bool", "c", 1), ("bool", "c", 3),
        nr("==", 3), nr(">", P53 + 1), nr("<=", I64_MIN), ("nrange", "c", I64_MIN, I64_MAX, 3, -inf, inf), ("nrange", "c", 0, -1, 0, inf, -inf),
        ("nset", "c", [], []), ("nset", "c", [3], [3.0]),
        ("nset", "c", sorted(big), sorted([v + 0.5 for v in big[:4094]] + [-inf, inf])),
    ]


def check_kernel(device, n, seed, only=None):
    from rag_fin_amd import filter_expr
    tags, payload = edge_column(n, seed, only)
    leaves = with_sets(edge_leaves())
    assert len(leaves) == 16 and len(leaves[15][2]) == 4096 and len(leaves[15][3]) == 4096
    got = run_dynamic_match(device, leaves, tags, payload, n)
    rows = list(zip(tags.tolist(), payload.tolist()))
    for l, leaf in enumerate(leaves):
        want = np.array([row_passes(leaf, t, p) for t, p in rows], dtype=bool)
        assert np.array_equal(unpack(got[l], n), want), (n, only, leaf[:2])
        assert not unpack(got[l], 32 * got.shape[1])[n:].any()    # the bits past n_rows are zero
        assert np.array_equal(filter_expr.dynamic_leaf_reference(leaf[:4 if leaf[0] == "nset" else None], tags, payload), want)
    return tags, payload, got


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 65_537])
def test_dynamic_match_equals_the_reference_at_every_edge(gpu_device, n):
    tags, payload, got = check_kernel(gpu_device, n, n)
    if n >= 64:
        assert all(set(tags[s:s + 64].tolist()) == {0, 1, 2, 3, 4} for s in range(0, n - 63, 64))   # every full wave: every tag
    assert unpack(got[0], n).sum() == (tags != ABSENT).sum() and not got[3].any() and not got[5].any() and not got[13].any()
    if n >= 256:
        assert all(unpack(got[l], n).any() for l in (0, 1, 2, 4, 6, 7, 8, 9, 10, 11, 14, 15))
    # one leaf alone, another fill, all four inclusive-bit combinations of one bound pair
    for flags in range(4):
        leaf = ("nrange", "c", 0, -1, flags, -0.0, 3.0)
        one = run_dynamic_match(gpu_device, [leaf], tags, payload, n, fill=0xA5A5A5A5)
        assert np.array_equal(unpack(one[0], n), np.array([row_passes(leaf, t, p) for t, p in zip(tags.tolist(), payload.tolist())], dtype=bool))


@pytest.mark.parametrize("only", [ABSENT, BOOL, INT, DOUBLE, STRING])
def test_single_tag_and_all_absent_columns(gpu_device, only):
    for n in (65, 257):
        tags, payload, got = check_kernel(gpu_device, n, 100 + only, only)
        assert unpack(got[0], n).all() == (only != ABSENT) and unpack(got[2], n).all() == (only == ABSENT)
        if only == ABSENT:
            assert not got[[0, 1] + list(range(3, 16))].any()


def test_an_invalid_call_launches_nothing(gpu_device):
    import torch
    from rag_fin_amd import _lib
    lib = _lib.load_library()
    K = _lib
    tags = torch.zeros(64, dtype=torch.uint8, device=gpu_device)
    pay = torch.zeros(64, dtype=torch.int64, device=gpu_device)
    out = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device=gpu_device)
    bad = []
    for kind, off, ln, foff, flen, flags in [(0, 0, 0, 0, 0, 0), (9, 0, 0, 0, 0, 0), (K.RF_DLEAF_NUM_SET, 0, 1, 0, 0, 0),
                                             (K.RF_DLEAF_NUM_SET, 0, 0, 0, 1, 0), (K.RF_DLEAF_NUM_SET, -1, 1, 0, 0, 0),
                                             (K.RF_DLEAF_STR_CODESET, 0, 1, 0, 0, 0), (K.RF_DLEAF_NUM_RANGE, 0, 0, 0, 0, 8),
                                             (K.RF_DLEAF_TAGS, 0, 0, 0, 0, 0x100), (K.RF_DLEAF_BOOL, 0, 0, 0, 0, 4),
                                             (K.RF_DLEAF_NUM_SET, 0, 65537, 0, 0, 0)]:
        a = (_lib.DynamicLeaf * 1)()
        a[0].kind, a[0].off, a[0].len, a[0].foff, a[0].flen, a[0].flags = kind, off, ln, foff, flen, flags
        a[0].tags_dev, a[0].payload_dev = tags.data_ptr(), pay.data_ptr()
        bad.append(lib.rf_dynamic_match(a, 1, None, None, None, 64, c_void_p(out.data_ptr()), _lib.current_stream_ptr()))
    ok = (_lib.DynamicLeaf * 1)()
    ok[0].kind, ok[0].flags, ok[0].tags_dev, ok[0].payload_dev = K.RF_DLEAF_TAGS, 1, tags.data_ptr(), pay.data_ptr()
    for n_leaves, n_rows, ptr in [(0, 64, out.data_ptr()), (17, 64, out.data_ptr()), (1, -1, out.data_ptr()),
                                  (1, 64, None), (1, 64, out.data_ptr() + 2)]:
        bad.append(lib.rf_dynamic_match(ok, n_leaves, None, None, None, n_rows, c_void_p(ptr) if ptr else None,
                                        _lib.current_stream_ptr()))
    for field, value in (("tags_dev", None), ("payload_dev", pay.data_ptr() + 4)):
        setattr(ok[0], field, value)
        bad.append(lib.rf_dynamic_match(ok, 1, None, None, None, 64, c_void_p(out.data_ptr()), _lib.current_stream_ptr()))
        ok[0].tags_dev, ok[0].payload_dev = tags.data_ptr(), pay.data_ptr()
    assert lib.rf_dynamic_match(ok, 1, None, None, None, 0, c_void_p(out.data_ptr()), _lib.current_stream_ptr()) == 0   # n_rows == 0
    torch.cuda.synchronize(gpu_device)
    assert bad == [-1] * len(bad) and (out.cpu().numpy() == 0x5A5A5A5A).all()
    assert lib.rf_dynamic_match(ok, 1, None, None, None, 64, c_void_p(out.data_ptr()), _lib.current_stream_ptr()) == 0    # the valid call
    torch.cuda.synchronize(gpu_device)
    assert out.cpu().numpy().view(np.uint32).tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0x5A5A5A5A, 0x5A5A5A5A]


# ---- the 3 000-row store whose keys mix all five tags ----------------------------------------------------------
N, D = 3000, 64
WORDS = ["net", "profit", "rose", "deposits", "fell", "npa", "ratio", "capital"]


def make_table(n, seed):
    table, dyn = mixed_table(n, seed)
    rng = np.random.default_rng(seed + 1)
    table["text"] = [" ".join(WORDS[j] for j in rng.integers(len(WORDS), size=rng.integers(2, 7))) for _ in range(n)]
    dyn["period copy"] = list(table["period"])
    return table, dyn


def make_store(device, table, dyn, c16, capacity=None):
    import torch
    from rag_fin_amd.store import CorpusStore
    st = CorpusStore("t", dim=D, capacity=capacity or len(table["id"]), device=device, fields=FIELDS, enable_dynamic_field=True)
    st.add(table["id"], table["text"], torch.from_numpy(c16).to(device), table["period"], table["chunk_type"],
           table["statement_type"], table["primary_value"], extra=dict({f.name: table[f.name] for f in FIELDS}, **dyn))
    st.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
    return st


def ast_mask(expr, table, dyn):
    """The AST's semantics row by row (filter_expr's docstring), memoised on the values the expression reads."""
    from rag_fin_amd import filter_expr
    node = filter_expr.parse(expr, schema=FIELDS, dynamic=True)
    names = sorted(filter_expr.fields_of(node))
    keys = sorted(filter_expr.dynamic_keys_of(node))
    cols = [table[f] for f in names] + [dyn.get(k) or [None] * len(table["id"]) for k in keys]
    memo = {}
    out = np.zeros(len(table["id"]), dtype=bool)
    for r, vals in enumerate(zip(*cols)):
        key = tuple((type(v), v if v == v else "nan", math.copysign(1, v) if isinstance(v, float) and v == 0 else 0) for v in vals)
        if key not in memo:
            memo[key] = node.eval(dict(zip(names, vals[:len(names)]), **{"$meta": dict(zip(keys, vals[len(names):]))}))
        out[r] = memo[key]
    return out


_WORLD = {}


def world(device):
    if not _WORLD:
        table, dyn = make_table(N, 5)
        c16 = osearch.synth_unit_rows(N, D, 21)
        q16 = osearch.synth_unit_rows(3, D, 22)
        _WORLD.update(table=table, dyn=dyn, c16=c16, q16=q16, st=make_store(device, table, dyn, c16),
                      scores=osearch.exact_scores(q16, c16))
    return _WORLD


KEYWORD_EXPRS = ['TEXT_MATCH(text, "npa") and k != 3 and fiscal_year > 2020',
                 'PHRASE_MATCH(text, "net profit") or (exists rare and bank == "ICICI") or $meta["page no"] == "10-K"']
MANY = " or ".join(f"k == {j}" for j in range(-5, 13))   # 18 dynamic leaves: more than one rf_dynamic_match call


def keyword_mask(expr, table, dyn):
    text = np.array(table["text"])
    if expr == KEYWORD_EXPRS[0]:
        return np.array(["npa" in t.split() for t in text]) & ast_mask("k != 3 and fiscal_year > 2020", table, dyn)
    return np.array([" net profit " in f" {t} " for t in text]) | ast_mask('(exists rare and bank == "ICICI") or $meta["page no"] == "10-K"', table, dyn)


# ---- 2. filter_rows(expr) equals the reference ------------------------------------------------------------------
def check_filter_rows(st, table, dyn, exprs):
    for expr in exprs:
        assert np.array_equal(st.filter_rows(expr), np.flatnonzero(ast_mask(expr, table, dyn))), expr
    for expr in KEYWORD_EXPRS:
        assert np.array_equal(st.filter_rows(expr), np.flatnonzero(keyword_mask(expr, table, dyn))), expr


def test_filter_rows_equal_the_reference(gpu_device):
    w = world(gpu_device)
    st = w["st"]
    assert len(LEAF_EXPRS + MIXED_EXPRS) >= 150
    check_filter_rows(st, w["table"], w["dyn"], LEAF_EXPRS + MIXED_EXPRS + [MANY])
    assert {"aud", "k", "page no", "rare"} <= set(st._dyncols) and not {"nobody", "period"} & set(st._dyncols)   # mirrored on first read
    counts = {e: int(ast_mask(e, w["table"], w["dyn"]).sum()) for e in ("exists k", "k != 3", f"k > {float(P53)!r}", "exists rare", "nobody != 1")}
    assert counts["exists k"] == N - sum(v is None for v in w["dyn"]["k"]) and counts["nobody != 1"] == 0
    assert 0 < counts[f"k > {float(P53)!r}"] < counts["k != 3"] < counts["exists k"] and counts["exists rare"] == N // 50
    for tensor in (st._dyncols["k"].tags, st._dyncols["k"].payload):
        assert tensor.numel() == N
    assert (st._dyncols["k"].tags.element_size(), st._dyncols["k"].payload.element_size()) == (1, 8)     # 9 bytes per row


def test_a_dynamic_copy_of_period_gives_the_built_in_filter_buffer_bit_for_bit(gpu_device):
    st = world(gpu_device)["st"]
    for tail in ('== "Q1_FY2024"', 'in ["Q2_FY2024", ""]', 'like "Q3%"', '> "Q2_FY2024"', '!= "Q1_FY2024"', 'not in ["Q2_FY2024"]'):
        a = read_filter(st.build_filter("period " + tail), N)
        b = read_filter(st.build_filter('$meta["period copy"] ' + tail), N)
        assert int(a[0][1]) > 0 and all(np.array_equal(x, y) for x, y in zip(a, b)), tail
        ta, tb = (st.build_filter(f + " " + tail).cpu().numpy().view(np.uint32) for f in ("period", '$meta["period copy"]'))
        n_tiles = int(a[0][3])
        assert np.array_equal(ta[-2048:][:2 * n_tiles], tb[-2048:][:2 * n_tiles])     # the compaction's tile counts


# ---- 3. search(expr=...) equals the oracle on the passing rows --------------------------------------------------
SEARCH_EXPRS = ["nobody == 1", "rare == 107", f"k > {P53}", 'k == "10-K" and fiscal_year >= 2024', "k != 3 and exists aud",
                '$meta["page no"] in [1, 3, 2.5] or aud like "10-%"']


def check_searches(st, table, dyn, c16, q16, device, exprs=SEARCH_EXPRS, k=10):
    import torch
    q = torch.from_numpy(q16).to(device)
    counts = []
    for expr in exprs:
        mask = ast_mask(expr, table, dyn)
        counts.append(int(mask.sum()))
        es, ei = oracle_on_subset(q16, c16, np.flatnonzero(mask), k)
        scores, ids, exact = st.index.search(q, k, want_exact=True, filt=st.build_filter(expr))
        assert np.array_equal(ids.cpu().numpy(), ei), expr
        assert np.array_equal(exact.cpu().numpy(), es) and np.array_equal(scores.cpu().numpy(), es.astype(np.float32)), expr
        res = st.search(q, "embedding", COS, k, expr=expr, output_fields=["bank", "k", "rare", "$meta"])
        for b, hits in enumerate(res):
            live = ei[b] >= 0
            assert [h.row for h in hits] == ei[b][live].tolist(), expr
            assert [h.score for h in hits] == [float(np.float32(s)) for s in es[b][live]]
            assert same([(h.entity.bank, h.entity.k, h.entity.rare) for h in hits],
                        [(table["bank"][r], dyn["k"][r], dyn["rare"][r]) for r in ei[b][live]])
            assert same([h.entity.get("$meta") for h in hits], [{key: c[r] for key, c in dyn.items() if c[r] is not None} for r in ei[b][live]])
    return counts


def test_filtered_search_equals_the_oracle(gpu_device):
    w = world(gpu_device)
    counts = check_searches(w["st"], w["table"], w["dyn"], w["c16"], w["q16"], gpu_device)
    assert counts[:2] == [0, 1] and all(c > 10 for c in counts[2:])


# ---- 4. mutation: the store after delete / upsert / growth equals a fresh store of the surviving rows --------------
@pytest.mark.parametrize("synced", [True, False])
def test_delete_upsert_and_growth_equal_a_fresh_store(gpu_device, synced):
    import torch
    n, n_new = 1500, 1200
    table, dyn = make_table(n, seed=9)
    c16 = osearch.synth_unit_rows(n + n_new, D, 31)
    q16 = osearch.synth_unit_rows(3, D, 32)
    st = make_store(gpu_device, table, dyn, c16[:n], capacity=n)
    if synced:   # the mirrors of every key follow the delete; else they are built afterwards
        for key in dyn:
            st.filter_rows(f'exists $meta["{key}"]')
    else:
        st.filter_rows("exists k")        # one mirror synced, the others not: both branches of the compaction
        st.add(["late"], ["net"], torch.from_numpy(c16[:1]).to(gpu_device), ["Q9"], ["c"], ["s"], [0.0],
               extra={"bank": ["LATE"], "k": [7], "late only": ["x"]})
        st.filter_rows('exists $meta["late only"]')
        st.delete('id == "late"')         # the k mirror is now behind the rows: dropped, not compacted; `late only` is gone
        assert "late only" not in st.dynamic and "late only" not in (st._dyncols or {})
        st.filter_rows("exists aud")
    gone = ast_mask('k == true or k < 0 or k like "10-%"', table, dyn)
    assert st.delete('k == true or k < 0 or k like "10-%"').delete_count == gone.sum() > 100
    keep = np.flatnonzero(~gone).tolist()
    # upsert: 100 surviving rows replaced (they move to the end) with other metadata, n_new new rows: past the capacity
    up = keep[:100]
    new, new_dyn = make_table(n_new, seed=10)
    new["id"] = [f"n{i}" for i in range(n_new)]
    assert len(keep) + n_new > n
    batch = {f: [table[f][i] for i in up] + new[f] for f in table}
    batch_dyn = {key: [("UP" if key == "k" else None)] * 100 + new_dyn[key] for key in dyn}
    batch_dyn["fresh key"] = [2.5] * 100 + [None] * n_new
    vec = np.concatenate([c16[up], c16[n:]])
    meta = [{key: c[j] for key, c in batch_dyn.items() if c[j] is not None} for j in range(100 + n_new)]
    st.upsert([batch["id"], batch["text"], torch.from_numpy(vec).to(gpu_device), batch["period"], batch["chunk_type"],
               batch["statement_type"], batch["primary_value"], batch["bank"], batch["fiscal_year"], meta])
    assert st.num_entities > n and st.index.capacity > n     # grown past the capacity it was made with
    rest = keep[100:]
    final = {f: [table[f][i] for i in rest] + batch[f] for f in table}
    final_dyn = {key: [dyn[key][i] if key in dyn else None for i in rest] + batch_dyn[key] for key in batch_dyn}
    c_final = np.concatenate([c16[rest], vec])
    assert st.columns["id"] == final["id"] and same(st.dynamic, final_dyn)
    fresh = make_store(gpu_device, final, final_dyn, c_final)
    exprs = LEAF_EXPRS[::4] + MIXED_EXPRS + ['k == "UP"', "$meta['fresh key'] == 2.5 and not exists aud", 'exists $meta["late only"]']
    for expr in exprs:
        got = st.filter_rows(expr)
        assert np.array_equal(got, fresh.filter_rows(expr)) and np.array_equal(got, np.flatnonzero(ast_mask(expr, final, final_dyn))), expr
    assert np.array_equal(st.filter_rows('k == "UP"'), np.arange(len(rest), len(rest) + 100))
    check_searches(st, final, final_dyn, c_final, q16, gpu_device, SEARCH_EXPRS[2:])


# ---- 5. the forms that take a filter -------------------------------------------------------------------------------
def test_an_expr_list_equals_one_call_per_query(gpu_device):
    import torch
    w = world(gpu_device)
    st, q = w["st"], torch.from_numpy(w["q16"]).to(gpu_device)
    exprs = ['k == "10-K" or $meta["page no"] in [1, 3]', 'period == "Q1_FY2024" and exists aud', None]
    res = st.search(q, "embedding", COS, 10, expr=exprs, output_fields=["k"])
    for b, e in enumerate(exprs):
        one = st.search(q[b:b + 1], "embedding", COS, 10, expr=e, output_fields=["k"])[0]
        assert same([(h.row, h.score, h.entity.k) for h in res[b]], [(h.row, h.score, h.entity.k) for h in one]) and len(one) == 10


def test_boost_on_a_dynamic_filter_equals_the_reference(gpu_device):
    import torch
    w = world(gpu_device)
    st, m = w["st"], lambda e: ast_mask(e, w["table"], w["dyn"])   # noqa: E731
    boosts = [BoostRanker('k == "10-K"', 1.5), BoostRanker('$meta["page no"] >= 3 and exists aud', 0.4)]
    cls = m('k == "10-K"').astype(np.int64) | (m('$meta["page no"] >= 3 and exists aud').astype(np.int64) << 1)
    for expr in (None, "aud != 3"):
        want = boost_reference(w["scores"], None if expr is None else m(expr), cls, class_weights(boosts), 10)
        res = st.search(torch.from_numpy(w["q16"]).to(gpu_device), "embedding", COS, 10, expr=expr, ranker=boosts)
        for b, hits in enumerate(res):
            assert [h.row for h in hits] == want[1][b].tolist() and [h.score for h in hits] == [float(x) for x in want[0][b]]


def test_iterator_range_and_mmr_take_dynamic_filters(gpu_device):
    """A dynamic filter that equals a built-in one (`period copy` is a copy of period) gives the same hits through
    every form that takes expr; the built-in side of each is covered by that form's own tests."""
    import torch
    w = world(gpu_device)
    st, q = w["st"], torch.from_numpy(w["q16"]).to(gpu_device)
    hits = lambda res: [[(h.row, h.score) for h in r] for r in res]   # noqa: E731
    band = {"metric_type": "COSINE", "params": {"radius": 0.05, "range_filter": 0.3}}
    for kw in ({"param": band}, {"param": COS, "mmr_lambda": 0.5, "mmr_fetch_k": 32}, {"param": COS, "offset": 70}):
        a, b = (st.search(q, "embedding", limit=10, expr=f'{f} == "Q2_FY2024" and fiscal_year > 2018', **kw)
                for f in ('$meta["period copy"]', "period"))
        assert hits(a) == hits(b) and all(a), kw
    expr = "exists k and not (k == true)"
    it = st.search_iterator(q[:1], "embedding", COS, batch_size=40, limit=100, expr=expr, output_fields=["k"])
    pages = []
    while True:
        page = it.next()
        if not page:
            break
        pages += [(h.row, h.score) for h in page]
        assert all(h.entity.k is not None and h.entity.k is not True for h in page)
    assert pages == hits(st.search(q[:1], "embedding", COS, 100, expr=expr))[0] and len(pages) == 100
    assert [r["id"] for r in st.query(expr="exists rare", output_fields=["rare"])] == [f"k{i}" for i in range(N) if i % 50 == 7]
    with pytest.raises(ValueError, match="a dynamic key cannot be grouped by"):
        st.search(q, "embedding", COS, 3, group_by_field="k")


def test_save_and_load_from_round_trip(gpu_device, tmp_path):
    from rag_fin_amd.store import CorpusStore
    w = world(gpu_device)
    w["st"].save(str(tmp_path / "d"))
    back = CorpusStore.load_from(str(tmp_path / "d"), device=gpu_device)
    assert back.enable_dynamic_field and same(back.dynamic, w["st"].dynamic) and back.schema == w["st"].schema
    for expr in LEAF_EXPRS[::6] + MIXED_EXPRS[:3]:
        assert np.array_equal(back.filter_rows(expr), w["st"].filter_rows(expr)), expr


# ---- 6. end to end: VectorRAG, the tool function, the REST body --------------------------------------------------------
def test_vector_rag_tool_and_rest_body_with_a_dynamic_expression(gpu_device):
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
    store = CorpusStore("fin_chunks", dim=384, capacity=16, device=gpu_device, enable_dynamic_field=True)
    half = len(chunks) // 2   # the first quarter's ingest knew no metadata; a later one learns of source and page
    ingest(store, emb, chunks[:half])
    page = {c["id"]: j for j, c in enumerate(chunks)}
    ingest(store, emb, chunks[half:], field_values={"source": "10-K", "page no": lambda c: page[c["id"]] if page[c["id"]] % 3 else None})
    rag = VectorRAG("no-key", "fin_chunks", embedder=emb, store=store, extra_output_fields=["source", "page no"])
    expr = 'source == "10-K" and $meta["page no"] > 3'
    q = "net profit in Q3 FY2024"
    mask = np.array([s == "10-K" and p is not None and p > 3 for s, p in zip(store.dynamic["source"], store.dynamic["page no"])])
    assert 3 <= mask.sum() < store.num_entities - half
    got = rag.search(q, 3, expr=expr)
    assert len(got) == 3 and all(c["source"] == "10-K" and c["page no"] > 3 for c in got)
    q16 = emb.encode_to_device([q])
    c16 = store.index.get_rows(np.arange(store.num_entities)).cpu().numpy()
    es, ei = oracle_on_subset(q16.cpu().numpy(), c16, np.flatnonzero(mask), 3)
    assert [c["text"] for c in got] == [store.columns["text"][r] for r in ei[0]]
    assert [c["score"] for c in got] == [float(np.float32(s)) for s in es[0]]
    assert [c["source"] for c in rag.search(q, 3, expr="not exists source")] == [None] * 3
    assert "source" not in VectorRAG("no-key", "fin_chunks", embedder=emb, store=store).search(q, 1, expr=expr)[0]
    mcp_server.set_rag(rag)
    try:
        r = mcp_server.search_vectors(q, 3, filter=expr)
        assert r["status"] == "success" and [c["text"] for c in r["results"]] == [c["text"] for c in got]
        args = adapter.search_args(adapter.SearchRequest(query=q, top_k=3, filter=expr))   # the body of POST /search
        r = mcp_server.search_vectors(**args)
        assert r["status"] == "success" and [(c["text"], c["score"]) for c in r["results"]] == [(c["text"], c["score"]) for c in got]
        assert mcp_server.search_vectors(q, 3, filter="source == other")["status"] == "error"
    finally:
        mcp_server.set_rag(None)
