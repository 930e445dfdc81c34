"""Keyword filters without a GPU: the grammar of TEXT_MATCH / PHRASE_MATCH, the definition over the
posting arrays (lexical.text_match_reference) against the per-row definition on strings (the AST's
eval), the positions, the compiled program, and the host-side argument checks of the C entries."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from rag_fin_amd import _lib, filter_expr as fe, lexical

GOLD = os.path.join(os.path.dirname(__file__), "golden")


# ---- parser -----------------------------------------------------------------------------------------
def test_accepted_forms():
    a = fe.parse('TEXT_MATCH(text, "net profit")')
    assert isinstance(a, fe.TextMatch) and a.min_match == 1 and a.terms() == ["net", "profit"]
    b = fe.parse("text_match(text, 'Net NET profit', minimum_should_match=2)")
    assert isinstance(b, fe.TextMatch) and b.min_match == 2 and b.terms() == ["net", "profit"]
    assert fe.parse("Text_Match(text, 'a', 3)").min_match == 3
    c = fe.parse('phrase_match(text, "Q1_FY2024")')
    assert isinstance(c, fe.PhraseMatch) and c.terms() == ["q1", "_", "fy2024"]
    assert fe.parse('PHRASE_MATCH(text, "a b a", 0)').terms() == ["a", "b", "a"]
    assert fe.parse('PHRASE_MATCH(text, "a b", slop=0)').slop == 0
    d = fe.parse('not (TEXT_MATCH(text, "eps") or PHRASE_MATCH(text, "net npa")) and period == "Q1_FY2024"')
    assert isinstance(d, fe.And) and isinstance(d.a, fe.Not) and isinstance(d.a.a, fe.Or)
    assert [type(n) for n in fe.text_leaves(d)] == [fe.TextMatch, fe.PhraseMatch]
    assert d.eval({"text": "gross NPA fell", "period": "Q1_FY2024"})
    assert not d.eval({"text": "Net NPA fell", "period": "Q1_FY2024"})
    # the analyzer is the caller's
    e = fe.parse('TEXT_MATCH(text, "A-B")', analyzer=lambda ts: [t.split() for t in ts])
    assert e.terms() == ["A-B"] and e.eval({"text": "x A-B"}) and not e.eval({"text": "a - b"})


@pytest.mark.parametrize("expr,match", [
    ('TEXT_MATCH(period, "a")', "'period'"),
    ('PHRASE_MATCH(chunk_type, "a")', "'chunk_type'"),
    ('TEXT_MATCH(text, "a", minimum_should_match=0)', "'0'"),
    ('TEXT_MATCH(text, "a", minimum_should_match=1.5)', "'1.5'"),
    ('TEXT_MATCH(text, "a", slop=0)', "'slop'"),
    ('PHRASE_MATCH(text, "a b", 1)', "exact adjacency"),
    ('PHRASE_MATCH(text, "a b", slop=2)', "exact adjacency"),
    ('TEXT_MATCH(text)', r"expected ','"),
    ('TEXT_MATCH(text, )', r"string of terms: '\)'"),
    ('TEXT_MATCH(text, 3)', "string of terms: '3'"),
    ('TEXT_MATCH(text, "a"', r"expected '\)'"),
    ('TEXT_MATCH(text, "' + " ".join(f"w{i}" for i in range(65)) + '")', "65 distinct terms"),
    ('PHRASE_MATCH(text, "' + "a " * 65 + '")', "65 terms in the phrase"),
    ('text == "a"', "cannot be filtered"),
    ('text like "a%"', "cannot be filtered"),
    ('text in ["a"]', "cannot be filtered"),
])
def test_rejected_forms(expr, match):
    with pytest.raises(ValueError, match=match):
        fe.parse(expr)


def test_sixty_four_terms_are_taken():
    assert len(fe.parse('TEXT_MATCH(text, "' + " ".join(f"w{i}" for i in range(64)) + '")').terms()) == 64
    assert len(fe.parse('PHRASE_MATCH(text, "' + "a " * 64 + '")').terms()) == 64


# ---- the definition: posting arrays against strings -----------------------------------------------------
def rows_of(bitmap_row, n):
    return np.unpackbits(bitmap_row.view(np.uint8), bitorder="little")[:n].astype(bool)


def check_definition(texts, postings, positions, exprs):
    n = len(texts)
    for expr in exprs:
        node = fe.parse(expr)
        prog = fe.compile_expr(node, {}, {}, postings.term_id)
        want = np.array([node.eval({"text": t}) for t in texts], dtype=bool)
        if prog.text_leaves:
            ref = lexical.text_match_reference(postings, positions, prog.text_leaves, n)
            assert ref.shape == (1, (n + 31) // 32) and ref.dtype == np.uint32
            got = rows_of(ref[0], n)
            assert not np.unpackbits(ref[0].view(np.uint8), bitorder="little")[n:].any(), expr
        else:
            assert [o[0] for o in prog.ops] == [_lib.RF_FOP_FALSE], expr
            got = np.zeros(n, dtype=bool)
        assert np.array_equal(got, want), (expr, np.flatnonzero(got != want)[:8])
        yield expr, want


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(GOLD, "chunks_golden.json")) as f:
        texts = [c["text"] for c in json.load(f)]
    postings = lexical.build_postings(texts)
    return texts, postings, lexical.build_positions(postings, texts)


def test_definition_on_the_golden_chunks():
    texts, postings, positions = golden()
    docs = lexical.analyze(texts)
    df = {}
    for d in docs:
        for t in set(d):
            df[t] = df.get(t, 0) + 1
    rare = sorted(t for t, c in df.items() if c == 1 and t.isalnum())[0]
    # a verbatim four-word phrase that not every row holds, and its words in another order
    words = next(d[j:j + 4] for d in docs for j in range(len(d) - 4)
                 if all(w.isalpha() for w in d[j:j + 4]) and len(set(d[j:j + 4])) == 4
                 and sum(" ".join(d[j:j + 4]) in " ".join(e) for e in docs) < len(docs))
    phrase = " ".join(words)
    swapped = " ".join([words[1], words[0]] + words[2:])
    exprs = [
        'TEXT_MATCH(text, "icici")',                                    # in every row
        f'TEXT_MATCH(text, "{rare}")',
        'TEXT_MATCH(text, "zzzunknown")',
        'TEXT_MATCH(text, "zzzunknown treasury")',
        'PHRASE_MATCH(text, "Q1_FY2024")',
        'PHRASE_MATCH(text, "Q1_FY2025")',
        f'PHRASE_MATCH(text, "{phrase}")',
        f'PHRASE_MATCH(text, "{swapped}")',
        f'TEXT_MATCH(text, "{swapped}", minimum_should_match=4)',       # the words, in any order
        'PHRASE_MATCH(text, ") (")',
        'PHRASE_MATCH(text, "crore crore")',                            # a repeated term
        'PHRASE_MATCH(text, "% of total assets ) • investments : ₹")',   # punctuation and a rupee sign inside
        'PHRASE_MATCH(text, "zzzunknown bank")',
        'PHRASE_MATCH(text, "")',
        'TEXT_MATCH(text, "")',
        'TEXT_MATCH(text, "retail treasury wholesale", minimum_should_match=3)',   # N = |Q|
        'TEXT_MATCH(text, "retail treasury wholesale", minimum_should_match=4)',   # N = |Q| + 1
        'TEXT_MATCH(text, "retail treasury wholesale", minimum_should_match=2)',
    ]
    got = dict(check_definition(texts, postings, positions, exprs))
    assert got[exprs[0]].all() and got[exprs[1]].sum() == 1 and not got[exprs[2]].any()
    assert got[exprs[4]].sum() == sum("Q1_FY2024" in t for t in texts) > 0
    assert got[exprs[6]].any() and not got[exprs[6]].all()
    # the swapped phrase must not match rows that only hold the words
    assert got[exprs[8]].sum() >= got[exprs[6]].sum() and got[exprs[7]].sum() < got[exprs[8]].sum()
    assert not got[exprs[16]].any() and got[exprs[15]].sum() <= got[exprs[17]].sum()


@functools.lru_cache(maxsize=None)
def synthetic():
    rng = np.random.default_rng(77)
    vocab = [f"w{i}" for i in range(300)]
    p = 1.0 / np.arange(1, len(vocab) + 1)
    p /= p.sum()
    lens = rng.integers(0, 30, 20000)
    draws = rng.choice(len(vocab), size=int(lens.sum()), p=p)
    texts, at = [], 0
    for ln in lens.tolist():
        texts.append(" ".join(vocab[i] for i in draws[at:at + ln]))
        at += ln
    postings = lexical.build_postings(texts)
    return texts, postings, lexical.build_positions(postings, texts)


def test_definition_on_synthetic_rows():
    texts, postings, positions = synthetic()
    exprs = ['TEXT_MATCH(text, "w0")', 'TEXT_MATCH(text, "w299 w250")', 'TEXT_MATCH(text, "w1 w2 w3", minimum_should_match=3)',
             'TEXT_MATCH(text, "w1 w2 w3 nope", minimum_should_match=3)', 'TEXT_MATCH(text, "w1 w2 w3", minimum_should_match=4)',
             'PHRASE_MATCH(text, "w0 w1")', 'PHRASE_MATCH(text, "w1 w0")', 'PHRASE_MATCH(text, "w0 w0")',
             'PHRASE_MATCH(text, "w0 w1 w0")', 'PHRASE_MATCH(text, "w2 w0 w1 w0")', 'PHRASE_MATCH(text, "w0")',
             'PHRASE_MATCH(text, "w0 nope")', 'TEXT_MATCH(text, "' + " ".join(f"w{i}" for i in range(64)) + '", 20)']
    got = dict(check_definition(texts, postings, positions, exprs))
    assert got[exprs[5]].any() and got[exprs[7]].any() and got[exprs[8]].any() and got[exprs[12]].any()
    assert not np.array_equal(got[exprs[5]], got[exprs[6]])


def test_positions_against_a_per_row_enumeration():
    for texts, postings, (pos_off, pos) in (golden(), synthetic()):
        docs = lexical.analyze(texts)
        assert pos_off.dtype == np.int64 and pos.dtype == np.uint32
        assert pos_off.shape == (postings.nnz + 1,) and pos.size == sum(len(d) for d in docs) == pos_off[-1]
        step = max(1, postings.nnz // 3000)
        for t in range(0, postings.n_terms, max(1, postings.n_terms // 50)):
            for q in range(int(postings.post_off[t]), int(postings.post_off[t + 1]), step):
                d = docs[int(postings.post_row[q])]
                want = [j for j, w in enumerate(d) if w == postings.vocab[t]]
                assert pos[pos_off[q]:pos_off[q + 1]].tolist() == want and want
    with pytest.raises(ValueError):
        lexical.build_positions(golden()[1], golden()[0][:-1])


# ---- compilation ---------------------------------------------------------------------------------------
def test_compiled_program():
    tid = {"a": 0, "b": 1, "c": 2}
    F, B = _lib.RF_FOP_FALSE, _lib.RF_FOP_BITMAP
    p = fe.compile_expr('TEXT_MATCH(text, "c a zz a", 2)', {}, {}, tid)
    assert p.text_leaves == [(_lib.RF_TEXT_MATCH, [0, 2], 2)] and [o[0] for o in p.ops] == [B]
    assert [o[0] for o in fe.compile_expr('TEXT_MATCH(text, "a zz", 2)', {}, {}, tid).ops] == [F]
    assert [o[0] for o in fe.compile_expr('TEXT_MATCH(text, "zz")', {}, {}, tid).ops] == [F]
    assert [o[0] for o in fe.compile_expr('TEXT_MATCH(text, "a", 2)', {}, {}, tid).ops] == [F]
    assert [o[0] for o in fe.compile_expr('PHRASE_MATCH(text, "a zz b")', {}, {}, tid).ops] == [F]
    assert [o[0] for o in fe.compile_expr('PHRASE_MATCH(text, "")', {}, {}, tid).ops] == [F]
    assert [o[0] for o in fe.compile_expr('TEXT_MATCH(text, "a")', {}, {}, {}).ops] == [F]   # declared, no postings
    p = fe.compile_expr('PHRASE_MATCH(text, "b a b") and not TEXT_MATCH(text, "zz") or TEXT_MATCH(text, "c")', {}, {}, tid)
    assert p.text_leaves == [(_lib.RF_TEXT_PHRASE, [1, 0, 1], 1), (_lib.RF_TEXT_MATCH, [2], 1)]
    assert [o[0] for o in p.ops] == [B, F, _lib.RF_FOP_NOT, _lib.RF_FOP_AND, B, _lib.RF_FOP_OR] and p.max_depth() == 2
    ops = p.ops_ctypes(words_per_leaf=12)
    assert (ops[0].off, ops[0].len, ops[4].off, ops[4].len) == (0, 12, 12, 12)
    arr, terms = fe.text_leaf_arrays(p)
    assert [(x.kind, x.term_off, x.n_terms, x.min_match) for x in arr] == [(2, 0, 3, 1), (1, 3, 1, 1)]
    assert terms.tolist() == [1, 0, 1, 2] and terms.dtype == np.int32
    many = " or ".join(f'TEXT_MATCH(text, "{w}")' for w in ["a"] * (_lib.RF_TEXT_MAX_LEAVES + 1))
    with pytest.raises(ValueError, match="more than 16"):
        fe.compile_expr(many, {}, {}, tid)


def test_compiling_without_a_lexical_index_names_the_call():
    for expr in ('TEXT_MATCH(text, "a")', 'period == "x" and not PHRASE_MATCH(text, "a b")'):
        with pytest.raises(ValueError, match=r"create_index\('sparse'"):
            fe.compile_expr(expr, {"period": ["x"]}, {})


def test_store_without_the_index_raises_before_any_device_work():
    from rag_fin_amd.store import CorpusStore

    class Index:
        size, capacity, device = 0, 4, None

    st = CorpusStore("c", dim=16, capacity=4, index=Index())
    with pytest.raises(ValueError, match=r"create_index\('sparse'"):
        st.build_filter('TEXT_MATCH(text, "a")')
    with pytest.raises(ValueError, match=r"create_index\('sparse'"):
        st.delete('PHRASE_MATCH(text, "a b")')
    st.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
    assert st.delete('PHRASE_MATCH(text, "a b")').delete_count == 0   # an empty collection: nothing to match


# ---- C ABI: host-side argument checks (no GPU needed) ------------------------------------------------------
def test_text_match_abi_argument_checks():
    lib = _lib.load_library()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every case below fails its checks first
    odd = ctypes.c_void_p(4100)
    sp = ctypes.c_void_p()
    assert lib.rf_sparse_create(ctypes.byref(sp), 100, 10, 50, fake, fake, fake, 0) == 0
    try:
        def leaves(*ls):
            arr = (_lib.TextLeaf * max(len(ls), 1))()
            for i, l in enumerate(ls):
                arr[i].kind, arr[i].term_off, arr[i].n_terms, arr[i].min_match = l
            return arr

        M, P = _lib.RF_TEXT_MATCH, _lib.RF_TEXT_PHRASE
        ok = leaves((M, 0, 2, 1))
        big = 1 << 20

        def call(lv=ok, n=1, terms=fake, total=2, out=fake, words=4, ws=fake, ws_bytes=big, handle=sp):
            return lib.rf_text_match(handle, lv, n, terms, total, out, words, ws, ws_bytes, None)

        assert lib.rf_text_match_workspace_bytes(sp, 1) > 0
        assert lib.rf_text_match_workspace_bytes(sp, 0) == 0 and lib.rf_text_match_workspace_bytes(sp, 17) == 0
        assert lib.rf_text_match_workspace_bytes(None, 1) == 0
        assert call(handle=None) == -1 and call(lv=None) == -1
        assert call(n=0) == -1 and call(lv=leaves(*[(M, 0, 2, 1)] * 17), n=17) == -1
        assert call(lv=leaves((M, 0, 0, 1))) == -1                     # n_terms out of 1..64
        assert call(lv=leaves((M, 0, 65, 1)), total=65) == -1
        assert call(lv=leaves((M, 1, 2, 1))) == -1                     # terms past the end of terms_dev
        assert call(lv=leaves((M, -1, 2, 1))) == -1
        assert call(lv=leaves((M, 0, 2, 0))) == -1                     # min_match < 1
        assert b"min_match" in lib.rf_last_error()
        assert call(lv=leaves((7, 0, 2, 1))) == -1                     # unknown kind
        assert call(lv=leaves((P, 0, 2, 1))) == -1                     # a phrase, no positions attached
        assert b"positions" in lib.rf_last_error()
        assert call(ws_bytes=lib.rf_text_match_workspace_bytes(sp, 1) - 1) == -1
        assert b"workspace" in lib.rf_last_error()
        assert call(words=3) == -1                                     # 100 rows need 4 words
        assert call(terms=None) == -1 and call(out=None) == -1 and call(ws=None) == -1
        assert call(out=odd) == -1 and call(ws=odd) == -1 and call(terms=ctypes.c_void_p(4098)) == -1
        # positions: null, misaligned, fewer than the postings
        assert lib.rf_sparse_attach_positions(None, fake, fake, 60) == -1
        assert lib.rf_sparse_attach_positions(sp, None, fake, 60) == -1
        assert lib.rf_sparse_attach_positions(sp, fake, odd, 60) == -1
        assert lib.rf_sparse_attach_positions(sp, fake, fake, 49) == -1
        assert lib.rf_sparse_attach_positions(sp, fake, fake, 60) == 0
        assert call(lv=leaves((P, 0, 2, 1)), ws_bytes=0) == -1         # now only the workspace is wrong
        assert b"workspace" in lib.rf_last_error()
        # a bitmap leaf needs bitmaps: rf_filter_eval has none, rf_filter_eval_bitmaps may be given none
        cols = (ctypes.c_void_p * 4)(4096, 4096, 4096, 8192)
        prog = (_lib.FilterOp * 1)()
        prog[0].op, prog[0].off, prog[0].len = _lib.RF_FOP_BITMAP, 0, 4
        assert lib.rf_filter_eval(prog, 1, None, None, cols, 100, fake, None) == -1
        assert b"bitmap" in lib.rf_last_error()
        assert lib.rf_filter_eval_bitmaps(prog, 1, None, None, None, cols, 100, fake, None) == -1
        prog[0].off = -1
        assert lib.rf_filter_eval_bitmaps(prog, 1, None, None, fake, cols, 100, fake, None) == -1
    finally:
        lib.rf_sparse_destroy(sp)
