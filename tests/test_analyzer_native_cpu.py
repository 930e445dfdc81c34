"""The native analyzer of the lexical index (csrc/analyzer.cpp through lexical.analyze_native) against
its definition, lexical.analyze; the numpy restatement of the device build (lexical.counts_from_tokens)
against lexical.count_terms; and the host-side argument checks of the new rf_* calls.  No GPU."""
import ctypes
import json
import os
from ctypes import c_void_p

import numpy as np
import pytest

from rag_fin_amd import _lib, lexical
from oracle.synth_text import retemplated_texts
from test_tokenizer import EDGE, _texts

HERE = os.path.dirname(os.path.abspath(__file__))

# beyond tests/test_tokenizer.py's EDGE: separators str.split() knows and the native rules do not, astral
# code points beside BMP ones, lone surrogates, combining marks, controls inside and between words
MORE_EDGE = ["line sep para sep", "nel\x85here fs\x1cgs\x1drs\x1eus\x1fend", "a\ud800b \udfff", "\ud83d alone",
             "\U0001f600中\U00020000x￿", "ȩ́ ǻ", "각 가",
             "\x00\x01\x02", "a\x00b c\x7fd", "ǅ ǆ ß ẞ ΑΣ ΑΣ. Σ",
             "x​y­z﻿", "«a»—b…c¿d", "　  ", "\t\n\r ",
             "İ i̇ I ı", "ﬁ ligature ＡＢＣ fullwidth", "٣ ३ ௩",
             "\U000e0001tag \U0010ffff", "; greek question mark", "་ tibetan   ogham space",
             # what basic_tokens drops sits between characters whose neighbourhood NFC and lower() look at
             "A\x1b\u03a3 a\x00\u03a3\x7f. \u0391\u03a3\x01b", "e\x1b\u0301 E\ufffd\u0301 a\u00ad\u03a3",
             "A\u03a3\u2028\u03a3A \u03a3"]


def _check(texts, n_threads=0):
    vocab, tok, dl = lexical.analyze_native(texts, n_threads)
    want = lexical.analyze(texts)
    got = lexical.tokens_from_native(vocab, tok, dl)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, texts[i][:60])
    assert len(got) == len(want)
    assert vocab == sorted({t for d in want for t in d})
    assert dl.dtype == np.int64 and dl.tolist() == [len(d) for d in want]
    assert tok.dtype == np.int32 and tok.size == int(dl.sum())
    return vocab, tok, dl


@pytest.fixture(scope="module")
def corpus():
    _, fuzz = _texts()
    return fuzz + MORE_EDGE


def test_fuzz_corpus_and_edges_match_analyze(corpus):
    _check(corpus)


def test_golden_chunks_and_retemplated_texts_match_analyze():
    chunks = json.load(open(os.path.join(HERE, "golden", "chunks_golden.json")))
    _check([c["text"] for c in chunks])            # an all-ASCII or simple batch: one joined blob
    _check(retemplated_texts(1500, 7))


def test_every_text_alone_matches_analyze():
    """One text per call: the joined-blob route and the per-text route each see every edge text."""
    for t in EDGE + MORE_EDGE:
        _check([t])


def test_empty_batch_and_batch_without_tokens():
    vocab, tok, dl = lexical.analyze_native([])
    assert vocab == [] and tok.size == 0 and dl.size == 0
    vocab, tok, dl = _check(["", "  ", "\x01"])
    assert vocab == [] and tok.size == 0 and dl.tolist() == [0, 0, 0]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_result_does_not_depend_on_threads_or_on_the_slicing(corpus, n):
    texts = corpus[100:100 + n]
    ref = _check(texts, 1)
    for nt in (4, 64):
        got = lexical.analyze_native(texts, nt)
        assert got[0] == ref[0] and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])


def test_threads_agree_on_the_whole_corpus(corpus):
    a = lexical.analyze_native(corpus, 1)
    b = lexical.analyze_native(corpus, 4)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_any_unicode_text_matches_analyze():
    """Property (hypothesis): over all of Unicode -- U+2028, CJK, combining marks, astral code points
    beside BMP ones, controls, lone surrogates, empty and whitespace-only texts -- and for any mix in
    one batch, analyze_native is analyze."""
    from hypothesis import given, settings, strategies as st
    anything = st.text(max_size=40)                                            # every code point, surrogates included
    spiced = st.text(alphabet="ab Z.,  \x85\x1c中\U00020000̧́\U0001f600\x00\x7f\t\n"
                              "é₹«—İΣσßǅ\ud800　 가￿",
                     max_size=40)
    # cased letters, Final_Sigma and combining marks around what cleaning drops, pads or splits on
    context = st.text(alphabet="aA\u03a3\u03c3\u03c2\u0391\u0130I\u0131.'\u0301\u0327\u0345\u00ad\u200b\x1b\x00\x7f\x0b\x1c "
                               "\u2028\x85\u4e2d\uac00\u00e9\u01c5:\u00b7\ufffd\ud800", max_size=8)
    batch = st.lists(st.one_of(anything, spiced, context, st.just(""), st.just(" \t ")), min_size=0, max_size=10)

    @settings(max_examples=400, deadline=None)
    @given(batch)
    def check(texts):
        _check(texts)
    check()


def test_counts_from_tokens_is_count_terms(corpus):
    for texts in (corpus, retemplated_texts(400, 3), ["", "a b a", "", "", "b", ""], ["x"]):
        vocab, tok, dl = lexical.analyze_native(texts)
        got = lexical.counts_from_tokens(tok, dl, len(vocab), vocab)
        want = lexical.count_terms(texts)
        assert got.vocab == want.vocab
        for name in ("post_off", "post_row", "post_tf", "dl", "pos_off", "pos"):
            a, b = getattr(got, name), getattr(want, name)
            assert a.dtype == b.dtype and np.array_equal(a, b), name


def test_counts_from_tokens_keeps_terms_without_a_posting():
    got = lexical.counts_from_tokens(np.asarray([5, 1, 5, 5], dtype=np.int32), np.asarray([0, 3, 0, 1]), 8)
    assert got.post_off.tolist() == [0, 0, 1, 1, 1, 1, 3, 3, 3]
    assert got.post_row.tolist() == [1, 1, 3] and got.post_tf.tolist() == [1, 2, 1]
    assert got.pos_off.tolist() == [0, 1, 3, 4] and got.pos.tolist() == [1, 0, 2, 0]


def test_dictionary_is_in_code_point_order_not_utf16_order():
    """U+FFFF sorts before U+10000 by code point (and by UTF-8 bytes), after it in UTF-16 code units."""
    vocab, _, _ = _check(["\U00010400x ～x zz ￦ \U0001f600"])
    assert vocab == sorted(vocab) and len(vocab) >= 3


# ---- host-side argument checks: RF_ERR_INVALID before any device call ----------------------------------
def test_analyzer_argument_checks():
    lib = _lib.load_library()
    h = c_void_p()
    off = np.zeros(3, dtype=np.int64)
    assert lib.rf_analyze(b"", c_void_p(off.ctypes.data), 2, None, 0, 1, None) == -1
    assert lib.rf_analyze(b"", None, 2, None, 0, 1, ctypes.byref(h)) == -1 and not h.value
    assert lib.rf_analyze(b"", c_void_p(off.ctypes.data), -1, None, 0, 1, ctypes.byref(h)) == -1
    assert lib.rf_analyze(b"", c_void_p(off.ctypes.data), 2, None, 2, 1, ctypes.byref(h)) == -1
    down = np.asarray([0, 2, 1], dtype=np.int64)
    assert lib.rf_analyze(b"abc", c_void_p(down.ctypes.data), 2, None, 0, 1, ctypes.byref(h)) == -1 and not h.value
    assert lib.rf_analysis_sizes(None, c_void_p(off.ctypes.data)) == -1
    assert lib.rf_analysis_read(None, None, None, None, None) == -1
    assert lib.rf_analysis_destroy(None) == 0


def test_count_argument_checks_need_no_gpu():
    lib = _lib.load_library()
    ws_bytes = lib.rf_sparse_count_workspace_bytes
    assert ws_bytes(0, 5) == 0 and ws_bytes(5, 0) == 0 and ws_bytes(-1, 5) == 0
    assert ws_bytes(1 << 31, 5) == 0 and ws_bytes(5, 1 << 31) == 0
    need = ws_bytes(1000, 70000)
    assert need > 1000 * 36 and need % 16 == 0
    assert ws_bytes(_lib.RF_LEX_SORT_TILE + 1, 3) > ws_bytes(_lib.RF_LEX_SORT_TILE, 3)
    A = 0x10000   # an aligned, never dereferenced address: every check below fails before a device call
    plan, apply_ = lib.rf_sparse_count_plan, lib.rf_sparse_count_apply
    good = dict(tok=A, rs=A, n=1000, rows=10, terms=70000, off=A, tot=A, ws=A, wsb=need)

    def call_plan(**kw):
        a = dict(good, **kw)
        return plan(a["tok"], a["rs"], a["n"], a["rows"], a["terms"], a["off"], a["tot"], a["ws"], a["wsb"], None)
    for bad in (dict(tok=None), dict(rs=None), dict(off=None), dict(tot=None), dict(ws=None), dict(tok=A + 4),
                dict(rs=A + 8), dict(off=A + 8), dict(tot=A + 4), dict(ws=A + 4), dict(n=0), dict(n=-5), dict(n=1 << 31),
                dict(rows=0), dict(rows=1 << 31), dict(terms=0), dict(terms=1 << 31), dict(wsb=need - 1), dict(wsb=0)):
        assert call_plan(**bad) == -1, bad
        assert lib.rf_last_error()
    out = _lib.Postings(10, 70000, 500, 1000)
    out.post_row, out.post_tf, out.pos_off, out.pos = A, A, A, A

    def call_apply(desc, want_pos=1, **kw):
        a = dict(good, **kw)
        return apply_(a["rs"], a["n"], a["rows"], a["terms"], a["ws"], a["wsb"], desc, want_pos, None)
    assert call_apply(None) == -1
    for bad in (dict(rs=None), dict(ws=None), dict(rs=A + 8), dict(n=0), dict(rows=1 << 31), dict(terms=-1),
                dict(wsb=need - 1)):
        assert call_apply(ctypes.byref(out), **bad) == -1, bad
    for field, value in (("post_row", None), ("post_tf", None), ("pos_off", None), ("pos", None), ("post_row", A + 4),
                         ("pos_off", A + 8), ("nnz", 0), ("nnz", 1001), ("n_pos", 0), ("n_pos", -1)):
        d = _lib.Postings(10, 70000, 500, 1000)
        d.post_row, d.post_tf, d.pos_off, d.pos = A, A, A, A
        setattr(d, field, value)
        assert call_apply(ctypes.byref(d)) == -1, field
