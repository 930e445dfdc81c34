"""The references the filter GPU tests compare against, checked on the CPU (no GPU needed):

  * the tile plan of oracle/filter_program.py at the row counts where a filter buffer changes regime
    (tests/test_filter_scale_gpu.py asserts the device's header word 3 against it);
  * the random postfix programs of tests/test_filter_programs_gpu.py: the generator lives here, and
    the premise test counts, over the frozen set, every feature the GPU test claims to run;
  * the interpreter itself, BITMAP leaf included, against filter_expr.Node.eval on compiled
    expressions with TEXT_MATCH / PHRASE_MATCH, the bitmaps taken from lexical.text_match_reference.
"""
import functools
from dataclasses import dataclass

import numpy as np
import pytest

from oracle import filter_program as fp
from rag_fin_amd import _lib, filter_expr as fe, lexical

# ---- the tile plan -------------------------------------------------------------------------------------
# n -> (nblk, tile_words, n_tiles); the sizes of tests/test_filter_scale_gpu.py
PLAN_TABLE = {
    1_048_576: (32_768, 32, 1024),      # the last size of the first regime: one k_filter_eval trip per tile
    1_048_577: (32_769, 64, 513),       # second trip of k_filter_eval's wave loop; the last tile is one word
    8_388_641: (262_146, 288, 911),     # k_filter_compact: a full 256-word chunk, then a partial one
    33_554_465: (1_048_578, 1056, 993), # k_filter_copy: a second stride of its 1024 threads
}


@pytest.mark.parametrize("n", sorted(PLAN_TABLE))
def test_plan_table(n):
    assert fp.plan(n) == PLAN_TABLE[n]


def test_plan_regimes_begin_where_the_design_says():
    assert fp.plan(0) == (0, 32, 0) and fp.plan(1) == (1, 32, 1) and fp.plan(1_000_000) == (31_250, 32, 977)
    for n, tw in ((1_048_576, 32), (1_048_577, 64), (8_388_608, 256), (8_388_609, 288), (33_554_432, 1024),
                  (33_554_433, 1056)):
        nblk, tile_words, n_tiles = fp.plan(n)
        assert tile_words == tw and tile_words % 32 == 0
        assert n_tiles <= fp.FILTER_MAX_TILES and (n_tiles - 1) * tile_words < nblk <= n_tiles * tile_words


def test_the_restated_constants_are_the_bindings():
    names = ["CODESET", "RANGE", "ROWLIST", "TRUE", "FALSE", "AND", "OR", "NOT", "BITMAP"]
    assert [getattr(fp, "FOP_" + s) for s in names] == [getattr(_lib, "RF_FOP_" + s) for s in names]
    assert (fp.FRANGE_LO_INCL, fp.FRANGE_HI_INCL) == (_lib.RF_FRANGE_LO_INCL, _lib.RF_FRANGE_HI_INCL)
    assert (fp.FILTER_MAX_OPS, fp.FILTER_MAX_DEPTH) == (_lib.RF_FILTER_MAX_OPS, _lib.RF_FILTER_MAX_DEPTH)


# ---- random programs -----------------------------------------------------------------------------------
SEED = 31
N_MAIN = 2081                        # nblk = 66: an even word count with a partial last word
SMALL_NS = (1, 63, 64, 65, 2049)     # 2049: nblk = 65, the odd word count of k_filter_eval's w + 1 < w1 guard
N_PROGRAMS = 200
N_SUBSET = 20                        # the programs repeated at SMALL_NS

INF = float("inf")
BOUNDS = (-INF, -1.5, -0.0, 0.0, 2.5, INF)
SUBNORMAL = 5e-324
SPECIAL_VALUES = (float("nan"), 0.0, -0.0, INF, -INF, SUBNORMAL, -SUBNORMAL)
EXACT_VALUES = (-1.5, 2.5, 1.0, -3.0)                   # two of them are bounds: inclusivity decides
SPECIAL_CODES = (-1, -2 ** 31, 31, 32, 64, 95, 96, 1000, 2 ** 31 - 1)


@dataclass
class ProgramSet:
    n: int
    codes: dict          # column 0..2 -> int32 [n]
    values: np.ndarray   # fp64 [n]
    programs: list       # each a list of op tuples (op, column, off, len, flags, lo, hi)
    code_sets: np.ndarray
    row_lists: np.ndarray
    bitmaps: np.ndarray


def make_table(n, rng):
    codes = {}
    for c in range(3):
        col = rng.integers(0, 64, n)
        special = rng.random(n) < 0.2
        col[special] = rng.choice(SPECIAL_CODES, int(special.sum()))
        codes[c] = col.astype(np.int32)
    values = rng.normal(size=n) * 2.0
    kind = rng.random(n)
    values[kind < 0.3] = rng.choice(EXACT_VALUES, int((kind < 0.3).sum()))
    values[kind > 0.7] = rng.choice(SPECIAL_VALUES, int((kind > 0.7).sum()))
    return codes, values


def make_shape(rng, depth, n_ops, deep_not=False):
    """'L' (leaf) / 'B' (AND or OR) / 'N' (NOT) tokens of a valid postfix program of exactly n_ops
    operations whose stack reaches exactly `depth`.  L leaves, L - 1 binaries and U NOTs: n_ops =
    2 L - 1 + U with L >= depth.  deep_not: one NOT stands where the stack holds >= 30 entries."""
    assert 1 <= depth <= fp.FILTER_MAX_DEPTH and 2 * depth - 1 <= n_ops <= fp.FILTER_MAX_OPS
    if depth == 1:
        n_nots = n_ops - 1
    else:
        options = [u for u in range(n_ops - (2 * depth - 1) + 1) if (n_ops - u) % 2 == 1]
        if deep_not:
            options = [u for u in options if u >= 1]
        n_nots = int(rng.choice(options[:3]))
    leaves = (n_ops - n_nots + 1) // 2
    toks, after = [], []     # after[j]: stack depth behind token j
    d, left, reached = 0, leaves, False
    while left > 0 or d > 1:
        can_push = left > 0 and d < depth
        can_fold = d >= 2 and (reached or left >= depth - (d - 1))   # the target stays reachable
        push = rng.random() < (0.5 if reached else 0.75) if can_push and can_fold else can_push
        assert can_push or can_fold
        if push:
            toks.append("L")
            d, left = d + 1, left - 1
            reached = reached or d == depth
        else:
            toks.append("B")
            d -= 1
        after.append(d)
    for j in range(n_nots):
        spots = np.arange(len(toks))
        if deep_not and j == 0:
            spots = np.flatnonzero(np.asarray(after) >= 30)
        at = int(rng.choice(spots))
        toks.insert(at + 1, "N")
        after.insert(at + 1, after[at])
    assert len(toks) == n_ops and max(after) == depth and after[-1] == 1
    return toks


def shape_target(i, rng):
    """(depth, n_ops, deep_not) of program i: the first ten of every run of ten are forced shapes, so
    that the N_SUBSET programs run at the small sizes hold each of them twice."""
    j = i % 10
    if j == 0:
        return 32, 64, False
    if j == 1:
        return 32, int(rng.integers(63, 65)), False
    if j == 2:
        return int(rng.integers(2, 32)), 64, False
    if j == 3:
        return int(rng.integers(30, 33)), 64, True
    if j == 4:
        return 1, int(rng.integers(1, 4)), False
    depth = int(rng.integers(2, 33))
    return depth, int(rng.integers(2 * depth - 1, 65)), False


class _Pools:
    def __init__(self):
        self.code_sets, self.row_lists, self.bitmaps = [0], [0], [0]   # never empty: a leaf of len 0 points at a word


def make_leaf(rng, n, pools):
    nblk = (n + 31) // 32
    kind = rng.choice(["codeset", "range", "rowlist", "bitmap", "true", "false"], p=[0.25, 0.25, 0.2, 0.24, 0.03, 0.03])
    if kind == "codeset":
        ln = int(rng.choice([0, 1, 2, 2, 2, 3]))
        off = len(pools.code_sets)
        pools.code_sets.extend(rng.integers(0, 2 ** 32, ln, dtype=np.uint64).tolist())
        return (fp.FOP_CODESET, int(rng.integers(0, 3)), off, ln, 0, 0.0, 0.0)
    if kind == "range":
        lo, hi = (float(x) for x in rng.choice(BOUNDS, 2))
        if rng.random() < 0.7 and lo > hi:
            lo, hi = hi, lo
        return (fp.FOP_RANGE, 3, 0, 0, int(rng.integers(0, 4)), lo, hi)
    if kind == "rowlist":
        form = rng.choice(["empty", "one", "ends", "random"], p=[0.1, 0.1, 0.1, 0.7])
        if form == "empty":
            rows = []
        elif form == "one":
            rows = [int(rng.integers(0, n))]
        elif form == "ends":
            rows = sorted({0, n - 1})
        else:
            rows = np.flatnonzero(rng.random(n) < rng.choice([0.1, 0.5, 0.9])).tolist()
        off = len(pools.row_lists)
        pools.row_lists.extend(rows)
        return (fp.FOP_ROWLIST, 0, off, len(rows), 0, 0.0, 0.0)
    if kind == "bitmap":
        # full: the last word carries random bits past n, which the kernel must not let through
        form = rng.choice(["full", "short", "zero"], p=[0.6, 0.25, 0.15])
        ln = nblk if form == "full" else (nblk // 2 if form == "short" else 0)
        off = len(pools.bitmaps)
        pools.bitmaps.extend(rng.integers(0, 2 ** 32, ln, dtype=np.uint64).tolist())
        return (fp.FOP_BITMAP, 0, off, ln, 0, 0.0, 0.0)
    return (fp.FOP_TRUE if kind == "true" else fp.FOP_FALSE, 0, 0, 0, 0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def program_set(n, count=N_PROGRAMS):
    rng = np.random.default_rng([SEED, n])
    codes, values = make_table(n, rng)
    pools = _Pools()
    programs = []
    for i in range(count):
        prog = []
        for tok in make_shape(rng, *shape_target(i, rng)):
            if tok == "L":
                prog.append(make_leaf(rng, n, pools))
            elif tok == "B":
                prog.append((fp.FOP_AND if rng.random() < 0.5 else fp.FOP_OR, 0, 0, 0, 0, 0.0, 0.0))
            else:
                prog.append((fp.FOP_NOT, 0, 0, 0, 0, 0.0, 0.0))
        programs.append(prog)
    return ProgramSet(n, codes, values, programs, np.asarray(pools.code_sets, dtype=np.uint32),
                      np.asarray(pools.row_lists, dtype=np.uint32), np.asarray(pools.bitmaps, dtype=np.uint32))


def interpret(ps, prog):
    return fp.run_ops(prog, ps.code_sets, ps.row_lists, ps.bitmaps, ps.codes, ps.values, ps.n)


def depths(prog):
    """The stack depth each op finds (before it runs), and the deepest the program reaches."""
    d, found, top = 0, [], 0
    for o in prog:
        found.append(d)
        d += 1 if o[0] in fp.LEAF_OPS else (-1 if o[0] in (fp.FOP_AND, fp.FOP_OR) else 0)
        assert d >= 1
        top = max(top, d)
    assert d == 1
    return found, top


def test_the_generated_programs_hold_what_the_gpu_test_claims_to_run():
    ps = program_set(N_MAIN)
    n, nblk = ps.n, (ps.n + 31) // 32
    assert (n, nblk, len(ps.programs)) == (2081, 66, N_PROGRAMS)
    leaves = [o for p in ps.programs for o in p if o[0] in fp.LEAF_OPS]
    assert {o[0] for o in leaves} == set(fp.LEAF_OPS)                              # every leaf kind
    tops = [depths(p)[1] for p in ps.programs]
    assert all(1 <= len(p) <= fp.FILTER_MAX_OPS for p in ps.programs) and max(tops) == fp.FILTER_MAX_DEPTH
    assert sum(t == 32 for t in tops) >= 10                                          # the bool stack fills the register
    assert sum(len(p) == 64 for p in ps.programs) >= 10
    assert sum(len(p) == 64 and t == 32 for p, t in zip(ps.programs, tops)) >= 10
    deep_not = [any(o[0] == fp.FOP_NOT and d >= 30 for o, d in zip(p, depths(p)[0])) for p in ps.programs]
    assert sum(deep_not) >= 10
    assert any(o[0] == fp.FOP_NOT and d == 32 for p in ps.programs for o, d in zip(p, depths(p)[0]))
    # code sets: len 0 and len 1, over columns that hold -1, 31, 32 and codes at or past 32 len
    cs = [o for o in leaves if o[0] == fp.FOP_CODESET]
    assert {0, 1, 2, 3} <= {o[3] for o in cs} and {o[1] for o in cs} == {0, 1, 2}
    for c in range(3):
        col = ps.codes[c]
        assert {-1, 31, 32} <= set(col.tolist()) and col.min() == -2 ** 31 and col.max() >= 32 * max(o[3] for o in cs)
    # row lists: empty, one row, {0, n - 1}
    lists = [ps.row_lists[o[2]:o[2] + o[3]].tolist() for o in leaves if o[0] == fp.FOP_ROWLIST]
    assert [] in lists and any(len(x) == 1 for x in lists) and [0, n - 1] in lists
    assert all(x == sorted(set(x)) and (not x or x[-1] < n) for x in lists)
    # bitmaps: len = the row words, shorter, 0; a full one with bits set past n
    bm = [o for o in leaves if o[0] == fp.FOP_BITMAP]
    assert {0, nblk // 2, nblk} == {o[3] for o in bm}
    assert any(o[3] == nblk and ps.bitmaps[o[2] + nblk - 1] >> (n % 32) for o in bm)
    # ranges: all four inclusivity combinations, every bound, and every kind of value in the column
    rg = [o for o in leaves if o[0] == fp.FOP_RANGE]
    assert {o[4] for o in rg} == {0, 1, 2, 3}
    for side in (5, 6):
        got = {(x, np.signbit(x)) for x in (o[side] for o in rg)}
        assert got == {(b, np.signbit(b)) for b in BOUNDS}
    v = ps.values
    assert np.isnan(v).any() and (v == INF).any() and (v == -INF).any() and (np.abs(v) == SUBNORMAL).any()
    assert ((v == 0) & np.signbit(v)).any() and ((v == 0) & ~np.signbit(v)).any()
    assert (v == -1.5).any() and (v == 2.5).any() and (np.isfinite(v) & (np.abs(v) > 1e-3)).sum() > n // 2


def test_at_least_half_of_the_programs_are_far_from_constant():
    ps = program_set(N_MAIN)
    share = np.array([interpret(ps, p).mean() for p in ps.programs])
    assert ((share >= 0.01) & (share <= 0.99)).sum() >= N_PROGRAMS // 2, np.sort(share)
    # and among the deepest ones too: a 32-deep program is not a long way round to TRUE or FALSE
    deep = np.array([depths(p)[1] == 32 for p in ps.programs])
    assert ((share[deep] >= 0.01) & (share[deep] <= 0.99)).sum() >= deep.sum() // 2


@pytest.mark.parametrize("n", SMALL_NS)
def test_the_small_tables_run_the_forced_shapes(n):
    ps = program_set(n, N_SUBSET)
    assert ps.n == n and len(ps.programs) == N_SUBSET
    tops = [depths(p)[1] for p in ps.programs]
    assert sum(t == 32 and len(p) == 64 for p, t in zip(ps.programs, tops)) >= 2
    assert {o[0] for p in ps.programs for o in p} >= {fp.FOP_CODESET, fp.FOP_RANGE, fp.FOP_ROWLIST, fp.FOP_BITMAP,
                                                       fp.FOP_AND, fp.FOP_OR, fp.FOP_NOT}
    assert all(interpret(ps, p).shape == (n,) for p in ps.programs)


# ---- the interpreter against the per-row definition ----------------------------------------------------
PERIODS = ["Q1_FY2024", "Q2_FY2024", "Q3_FY2024", ""]
TYPES = ["key_ratios", "balance", "pl"]
KEYWORD_EXPRS = [
    'TEXT_MATCH(text, "alpha")',
    'PHRASE_MATCH(text, "alpha beta")',
    'not PHRASE_MATCH(text, "beta alpha") and TEXT_MATCH(text, "alpha beta gamma", minimum_should_match=2)',
    'TEXT_MATCH(text, "gamma delta", minimum_should_match=2) or period == "Q1_FY2024" and primary_value > 0',
    'PHRASE_MATCH(text, "alpha alpha beta") or id in [0, 5, 69] and not TEXT_MATCH(text, "delta")',
    'not (TEXT_MATCH(text, "alpha") or PHRASE_MATCH(text, "gamma delta")) or chunk_type like "%l%"',
    'TEXT_MATCH(text, "nosuchword alpha") and PHRASE_MATCH(text, "alpha nosuchword") or primary_value == 0',
    'PHRASE_MATCH(text, "delta") and PHRASE_MATCH(text, "alpha beta gamma delta") or statement_type != "c"',
]


def keyword_table():
    rng = np.random.default_rng(5)
    n = 70    # three mask words, the last one partial
    words = ["alpha", "beta", "gamma", "delta", "w0", "w1"]
    tab = {"id": list(range(n)),
           "text": [" ".join(rng.choice(words, int(rng.integers(0, 9)))) for _ in range(n)],
           "period": rng.choice(PERIODS, n).tolist(), "chunk_type": rng.choice(TYPES, n).tolist(),
           "statement_type": rng.choice(["c", "s"], n).tolist(),
           "primary_value": rng.choice([0.0, -0.0, 1.0, -1.5, float("nan"), 2.5], n).tolist()}
    tab["text"][3] = "alpha alpha beta gamma delta"
    return tab


@pytest.mark.parametrize("expr", KEYWORD_EXPRS)
def test_interpreter_with_bitmap_leaves_equals_the_per_row_definition(expr):
    tab = keyword_table()
    n = len(tab["id"])
    dicts, codes = {}, {}
    for j, f in enumerate(fe.VARCHAR_FIELDS):
        dicts[f] = list(dict.fromkeys(tab[f]))
        codes[j] = np.array([dicts[f].index(s) for s in tab[f]], dtype=np.int32)
    postings = lexical.build_postings(tab["text"])
    positions = lexical.build_positions(postings, tab["text"])
    node = fe.parse(expr)
    prog = fe.compile_expr(node, dicts, {k: i for i, k in enumerate(tab["id"])}, postings.term_id)
    assert any(o[0] == fp.FOP_BITMAP for o in prog.ops)
    bitmaps = lexical.text_match_reference(postings, positions, prog.text_leaves, n)
    assert bitmaps.shape == (len(prog.text_leaves), 3)
    got = fp.run_program(prog, codes, np.asarray(tab["primary_value"], dtype=np.float64), n, bitmaps)
    want = np.array([node.eval({f: tab[f][i] for f in tab}) for i in range(n)], dtype=bool)
    assert 0 < want.sum() < n
    assert np.array_equal(got, want)
    # a leaf's words may be padded (SparseIndex.text_match rounds a leaf up to four words): same rows
    padded = np.concatenate([bitmaps, np.zeros((bitmaps.shape[0], 1), dtype=np.uint32)], axis=1)
    assert np.array_equal(fp.run_program(prog, codes, np.asarray(tab["primary_value"], dtype=np.float64), n, padded), want)


def test_bitmap_leaf_shorter_than_the_rows_passes_nothing_past_its_words():
    words = np.array([0xFFFFFFFF, 0x1, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
    op = lambda off, ln: [(fp.FOP_BITMAP, 0, off, ln, 0, 0.0, 0.0)]   # noqa: E731
    assert np.flatnonzero(fp.run_ops(op(0, 3), None, None, words, {}, None, 70)).tolist() == list(range(33)) + list(range(64, 70))
    assert np.flatnonzero(fp.run_ops(op(1, 1), None, None, words, {}, None, 70)).tolist() == [0]
    assert np.flatnonzero(fp.run_ops(op(1, 2), None, None, words, {}, None, 70)).tolist() == [0] + list(range(32, 64))
    assert not fp.run_ops(op(2, 0), None, None, words, {}, None, 70).any()
