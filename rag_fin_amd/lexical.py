"""Lexical retrieval: the host side of BM25 search and of reciprocal-rank fusion.

The analyzer, the posting lists and the query encoding that rf_sparse_search (include/ragfin.h,
"lexical search") consumes are built here with numpy, in fp64, and rounded to fp32 once; the
scoring itself runs on the GPU (csrc/sparse.hip).  `bm25_reference` and `rrf_reference` are the
definitions in numpy: what the kernels must reproduce bit for bit.  They are for tests and tools;
no product path calls them.

Definition
  terms     basic tokenisation (lower-case, accent strip, whitespace and punctuation split; no
            WordPiece step, no vocabulary file).  The dictionary is the sorted list of the distinct
            terms of the corpus; a term's id is its position in it.
  postings  dl[r] = terms of row r, avgdl = sum(dl) / N, df[t] = rows holding t, tf[t, r]
            idf[t]    = log(1 + (N - df + 0.5) / (df + 0.5))
            imp[t, r] = float32(idf[t] * ((tf * (k1 + 1)) / (tf + k1 * (1 - b + b * (dl[r] / avgdl)))))
            every operation in fp64 in this order; every impact is a positive normal fp32 value.
  query     its distinct known terms t_1 < .. < t_m (unknown terms are dropped), weights
            w_i = float32(count of t_i in the query); m <= 64.
  score     acc = 0.0f; for i = 1..m, if t_i in r: acc = acc + (w_i * imp[t_i, r]), the product and
            the sum each rounded to fp32.  A row is a hit iff it holds a query term (and passes the
            filter); ranking (score desc, row asc).
  keyword   (TEXT_MATCH / PHRASE_MATCH filters) positions[q] = the ascending token
            positions of posting q's term in its row (build_positions).  A MATCH leaf passes the rows
            that hold at least min_match of its distinct terms; a PHRASE leaf p_0 .. p_{m-1} passes row
            r iff some j has p_i at position j + i of r for every i (text_match_reference).
  fusion    fused(d) = sum over the arms a, in arm order, that hold d of weight_a / (rrf_k + rank_a(d)),
            rank 1-based, in fp64; the best k distinct ids by (fused desc, id asc).
  upkeep     the index after a write equals a build of the surviving texts, bit for bit.
            With tf kept beside the postings every impact is re-derivable from N, avgdl, df and dl.
            counts   count_terms(texts): the postings of a text list on its own (its own sorted
                     dictionary, rows from 0, tf, dl and positions; no impacts).
            append   rows N_old.. are new.  The dictionary is the sorted union (merge_vocab); per merged
                     term the list is the old segment, then the delta segment with rows + N_old;
                     positions follow their postings (append_reference).
            compact  keep bool [N]: a posting survives iff its row does, rows are renumbered by their
                     rank among the kept rows, a term whose df became 0 leaves the dictionary and the
                     later ids move down; positions follow their postings (compact_reference).
            Then idf from the new N and df (term_idf, on the host) and imp by the formula above.
  build      build_postings / build_positions below are the definition and the route of a
            store with a custom analyzer.  Otherwise the product builds through analyze_native (the
            analyzer in C++: dictionary, a term id per token, tokens per row) and SparseIndex.from_tokens
            (the postings from that stream, on the device); counts_from_tokens restates the device part.
"""
from __future__ import annotations

import re
import unicodedata
from typing import Callable, Sequence

import numpy as np

from .tokenizer import _is_cjk, _is_control, _is_punctuation, _is_whitespace

MAX_QUERY_TERMS = 64   # RF_SPARSE_MAX_TERMS (include/ragfin.h)
DEFAULT_K1 = 1.2
DEFAULT_B = 0.75

# the ASCII fast path of basic_tokens: control characters (removed, not split on) force the slow path
_ASCII_CONTROL = re.compile(r"[\x00-\x08\x0b\x0c\x0e-\x1f\x7f]")
_ASCII_TOKEN = re.compile(r"[^\s!-/:-@\[-`{-~]+|[!-/:-@\[-`{-~]")

Analyzer = Callable[[Sequence[str]], "list[list[str]]"]


def basic_tokens(text: str) -> list[str]:
    """The basic tokenisation of a BERT uncased tokenizer (WordPieceTokenizer.basic_tokens without
    the special tokens and without the WordPiece step): clean, NFC, split on whitespace, lower-case,
    strip accents, split every punctuation character off."""
    if text.isascii() and not _ASCII_CONTROL.search(text):
        # ASCII without control characters: cleaning, NFC, NFD and the accent strip are identities
        return _ASCII_TOKEN.findall(text.lower())
    cleaned = []
    for ch in text:
        cp = ord(ch)
        if cp == 0 or cp == 0xFFFD or _is_control(ch):
            continue
        if _is_cjk(cp):
            cleaned.append(" " + ch + " ")
        elif _is_whitespace(ch):
            cleaned.append(" ")
        else:
            cleaned.append(ch)
    out = []
    for word in unicodedata.normalize("NFC", "".join(cleaned)).strip().split():
        word = "".join(c for c in unicodedata.normalize("NFD", word.lower()) if unicodedata.category(c) != "Mn")
        cur = []
        for ch in word:
            if _is_punctuation(ch):
                if cur:
                    out.append("".join(cur))
                    cur = []
                out.append(ch)
            else:
                cur.append(ch)
        if cur:
            out.append("".join(cur))
    return out


def analyze(texts: Sequence[str]) -> list[list[str]]:
    """The default analyzer: basic_tokens of every text."""
    return [basic_tokens(t) for t in texts]


# ---- the native analyzer (csrc/analyzer.cpp) -------------------------------------------
_NATIVE = None
# whitespace of str.split() that the native rules do not split on (they know " \t\n\r" only)
_ODD_SPACE = re.compile(r"[^\S \t\n\r]")


def _native_tables():
    """(regex of the characters that need the Python pre-pass, the 'simple' non-ASCII punctuation as
    int32, and the two str.translate tables of the pre-pass), built once."""
    global _NATIVE
    if _NATIVE is None:
        from .tokenizer import _LazyTable, _clean_map, _simple_tables
        complex_re, punct = _simple_tables()
        # precomposed Hangul has no entry in unicodedata.decomposition() (it decomposes by rule), yet NFD takes it
        # apart and nothing puts it together again: a term keeps the jamo, so such text needs the pre-pass too
        complex_re = re.compile("(?:" + complex_re.pattern + ")|[\uac00-\ud7a3]")

        def mn_punct(cp):
            cat = unicodedata.category(chr(cp))
            if cat == "Mn":
                return None
            return " " + chr(cp) + " " if cp >= 128 and cat.startswith("P") else cp

        def clean(cp):
            # ASCII controls go HERE, not on the native side: what basic_tokens drops before NFC and lower() must
            # be gone before them too (a control between a cased letter and a capital sigma decides Final_Sigma)
            if cp < 128:
                return None if (cp < 32 and cp not in (9, 10, 13)) or cp == 127 else cp
            return _clean_map(cp)

        _NATIVE = (complex_re, np.asarray(punct, dtype=np.int32), _LazyTable(clean), _LazyTable(mn_punct))
    return _NATIVE


def _prenormalise(text: str, clean_tab, mn_punct_tab) -> str:
    """Non-ASCII text -> a string on which the native rules give basic_tokens(text): clean, NFC, lower,
    NFD, Mn stripped and non-ASCII punctuation padded with spaces, with C-speed string primitives.  What
    the tables cannot express (a character str.split() splits on is still there) comes back as the
    tokens of basic_tokens joined by spaces: each of them re-tokenises to itself."""
    s = text.translate(clean_tab)
    if not unicodedata.is_normalized("NFC", s):
        s = unicodedata.normalize("NFC", s)
    s = s.lower()
    if not unicodedata.is_normalized("NFD", s):
        s = unicodedata.normalize("NFD", s)
    s = s.translate(mn_punct_tab)
    if _ODD_SPACE.search(s) is not None:
        return " ".join(basic_tokens(text))
    return s


def native_input(texts: list) -> tuple:
    """What analyze_native hands to rf_analyze: (the texts' UTF-8 bytes back to back, pre-normalised
    where they need it, and their byte offsets int64 [n + 1])."""
    from ctypes import c_void_p
    from . import _lib
    from .tokenizer import only_simple_non_ascii
    lib = _lib.load_library()
    n = len(texts)
    complex_re, _, clean_tab, mn_punct_tab = _native_tables()
    offsets = np.zeros(n + 1, dtype=np.int64)
    joined = "".join(texts)
    blob = None
    if joined.isascii() or only_simple_non_ascii(joined, complex_re):
        try:
            blob = joined.encode("utf-8")
        except UnicodeEncodeError:               # a lone surrogate somewhere: the per-text path sorts it out
            blob = None
    if blob is not None:
        np.cumsum(np.fromiter(map(len, texts), dtype=np.int64, count=n), out=offsets[1:])
        if len(blob) != int(offsets[n]):         # non-ASCII present: characters -> bytes
            chars = offsets.copy()
            if lib.rf_utf8_offsets(blob, len(blob), c_void_p(chars.ctypes.data), n, c_void_p(offsets.ctypes.data)) != 0:
                raise RuntimeError("rf_utf8_offsets: the character counts do not match the blob")
    else:
        enc = []
        for t in texts:
            if not t.isascii() and complex_re.search(t) is not None:
                t = _prenormalise(t, clean_tab, mn_punct_tab)
            try:
                enc.append(t.encode("utf-8"))
            except UnicodeEncodeError:           # lone surrogates: basic_tokens drops them
                enc.append(" ".join(basic_tokens(t)).encode("utf-8"))
        np.cumsum([len(b) for b in enc], out=offsets[1:])
        blob = b"".join(enc)
    return blob, offsets


def analyze_native(texts: Sequence[str], n_threads: int = 0, timing: dict | None = None):
    """`analyze` through rf_analyze (csrc/analyzer.cpp) -> (vocab list[str], tok int32 [n_tokens], dl
    int64 [n]): the sorted distinct terms, the term id of every token in text order (texts back to
    back) and the tokens per text; [vocab[i] for i in tok] cut by dl is analyze(texts), for every str.
    Division of labour as in WordPieceTokenizer.batch_native: an ASCII batch, or one whose non-ASCII
    characters are all "simple", goes over as one joined blob; other non-ASCII texts are pre-normalised
    one by one (_prenormalise).  timing: a dict the seconds of the stages are added into (for tools)."""
    import time
    from ctypes import byref, c_void_p
    from . import _lib
    texts = list(texts)
    n = len(texts)
    if n == 0:
        return [], np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64)
    if n_threads <= 0 and n < 64:
        n_threads = 1        # a query-sized batch: no pool
    if n_threads <= 0:       # the CPUs the process may burn, not the ones it may run on: hostcpu.py
        from .hostcpu import cpu_budget
        n_threads = min(cpu_budget(), 64)
    t_start = time.perf_counter()
    lib = _lib.load_library()
    blob, offsets = native_input(texts)
    punct = _native_tables()[1]
    t_native = time.perf_counter()
    handle = c_void_p()
    _lib.check(lib.rf_analyze(blob, c_void_p(offsets.ctypes.data), n, c_void_p(punct.ctypes.data), int(punct.size),
                              int(n_threads), byref(handle)))
    try:
        sizes = np.zeros(4, dtype=np.int64)
        _lib.check(lib.rf_analysis_sizes(handle, c_void_p(sizes.ctypes.data)))
        vocab_blob = np.empty(max(int(sizes[3]), 1), dtype=np.uint8)
        tok = np.empty(int(sizes[1]), dtype=np.int32)
        dl = np.empty(n, dtype=np.int64)
        _lib.check(lib.rf_analysis_read(handle, c_void_p(vocab_blob.ctypes.data), None,
                                        c_void_p(tok.ctypes.data) if tok.size else None, c_void_p(dl.ctypes.data)))
    finally:
        lib.rf_analysis_destroy(handle)
    t_read = time.perf_counter()
    # every term is followed by '\n' and holds none: one decode and one split give the list
    vocab = vocab_blob[:int(sizes[3])].tobytes().decode("utf-8").split("\n")[:-1]
    if len(vocab) != int(sizes[2]):
        raise RuntimeError("analyze_native: the dictionary does not split into its terms")
    t_done = time.perf_counter()
    if timing is not None:
        for k, v in (("prepass_s", t_native - t_start), ("native_s", t_read - t_native), ("vocab_s", t_done - t_read)):
            timing[k] = timing.get(k, 0.0) + v
    return vocab, tok, dl


def tokens_from_native(vocab, tok, dl) -> list[list[str]]:
    """The term lists that (vocab, tok, dl) of analyze_native stand for (tests and tools)."""
    terms = [vocab[i] for i in np.asarray(tok).tolist()]
    ends = np.cumsum(dl).tolist()
    return [terms[e - int(d):e] for e, d in zip(ends, np.asarray(dl).tolist())]


def counts_from_tokens(tok, dl, n_terms: int, vocab=None) -> "TermCounts":
    """count_terms from term ids instead of strings: the definition, in numpy, of what
    rf_sparse_count_plan / _apply compute (csrc/lexical_build.hip).  tok int32 [n_tokens]: the term id
    of every token in (row, position) order, dl int64 [n]: the tokens per row.  A stable sort by term
    id alone gives (term, row, position) order; a token whose (term, row) differs from its
    predecessor's heads a posting.  For tests and tools only."""
    tok = np.clip(np.asarray(tok, dtype=np.int64), 0, max(int(n_terms) - 1, 0))
    dl = np.asarray(dl, dtype=np.int64)
    total = int(tok.size)
    row_start = np.zeros(dl.size + 1, dtype=np.int64)
    np.cumsum(dl, out=row_start[1:])
    order = np.argsort(tok, kind="stable")
    term = tok[order]
    row = np.searchsorted(row_start, order, side="right") - 1   # the last row that starts at or before the token
    head = np.ones(total, dtype=bool)
    head[1:] = (term[1:] != term[:-1]) | (row[1:] != row[:-1])
    scan = np.zeros(total + 1, dtype=np.int64)
    np.cumsum(head, out=scan[1:])
    post_off = scan[np.searchsorted(term, np.arange(int(n_terms) + 1), side="left")]
    first = np.flatnonzero(head)
    pos_off = np.concatenate([first, [total]]).astype(np.int64)
    return TermCounts(vocab, post_off, row[first].astype(np.uint32), np.diff(pos_off).astype(np.uint32), dl, pos_off,
                      (order - row_start[row]).astype(np.uint32))


class Postings:
    """What build_postings returns: the dictionary and the three posting arrays, host numpy."""

    def __init__(self, vocab, post_off, post_row, post_imp, dl, k1, b, post_tf=None):
        self.vocab = vocab                        # sorted distinct terms; id = position
        self.term_id = {t: i for i, t in enumerate(vocab)}
        self.post_off = post_off                  # int64 [V + 1]
        self.post_row = post_row                  # uint32 [nnz], ascending within a term
        self.post_imp = post_imp                  # fp32 [nnz]
        self.post_tf = post_tf                    # uint32 [nnz]: the term frequencies (index maintenance)
        self.dl = dl                              # int64 [N]
        self.k1 = float(k1)
        self.b = float(b)

    @property
    def n_rows(self) -> int:
        return int(self.dl.size)

    @property
    def n_terms(self) -> int:
        return len(self.vocab)

    @property
    def nnz(self) -> int:
        return int(self.post_row.size)

    @property
    def avgdl(self) -> float:
        return float(self.dl.sum()) / self.n_rows if self.n_rows else 0.0


class LivePostings(Postings):
    """The Postings of an index that is kept up to date on the device: the dictionary,
    the term offsets and the row lengths are maintained on the host; post_row, post_imp and post_tf are
    fetched through `fetch(name)` on first access and kept."""

    def __init__(self, vocab, term_id, post_off, dl, k1, b, fetch):
        self.vocab = vocab
        self.term_id = term_id if term_id is not None else {t: i for i, t in enumerate(vocab)}
        self.post_off = post_off
        self.dl = dl
        self.k1 = float(k1)
        self.b = float(b)
        self._fetch = fetch
        self._fetched: dict = {}

    def _array(self, name):
        if name not in self._fetched:
            self._fetched[name] = self._fetch(name)
        return self._fetched[name]

    post_row = property(lambda self: self._array("post_row"))
    post_imp = property(lambda self: self._array("post_imp"))
    post_tf = property(lambda self: self._array("post_tf"))

    @property
    def nnz(self) -> int:
        return int(self.post_off[-1])


def check_bm25_params(k1, b) -> tuple[float, float]:
    import math
    import numbers
    for name, v in (("bm25_k1", k1), ("bm25_b", b)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(float(v)):
            raise ValueError(f"{name} must be a finite real number, got {v!r}")
    if not float(k1) >= 0.0:
        raise ValueError(f"bm25_k1 must be >= 0, got {k1!r}")
    if not 0.0 <= float(b) <= 1.0:
        raise ValueError(f"bm25_b must be in [0, 1], got {b!r}")
    return float(k1), float(b)


def build_postings(texts: Sequence[str], k1: float = DEFAULT_K1, b: float = DEFAULT_B,
                   analyzer: Analyzer | None = None) -> Postings:
    """The BM25 posting lists of a corpus, one row per text (module docstring, "postings")."""
    k1, b = check_bm25_params(k1, b)
    docs = (analyzer or analyze)(list(texts))
    n = len(docs)
    if len(docs) != len(texts):
        raise ValueError("the analyzer must return one term list per text")
    vocab = sorted({t for d in docs for t in d})
    term_id = {t: i for i, t in enumerate(vocab)}
    dl = np.asarray([len(d) for d in docs], dtype=np.int64)
    # one (term, row) key per token; np.unique sorts them by term, then row, and counts the tf
    flat = np.fromiter((term_id[t] for d in docs for t in d), dtype=np.int64, count=int(dl.sum()))
    keys, tfs = np.unique(flat * max(n, 1) + np.repeat(np.arange(n, dtype=np.int64), dl), return_counts=True)
    tids, rows = keys // max(n, 1), keys % max(n, 1)
    post_tf = tfs.astype(np.uint32)
    tfs = tfs.astype(np.float64)
    df = np.bincount(tids, minlength=len(vocab)).astype(np.float64)
    post_off = np.zeros(len(vocab) + 1, dtype=np.int64)
    np.cumsum(df.astype(np.int64), out=post_off[1:])
    imp = impacts(tfs, dl[rows].astype(np.float64), df[tids], n, float(dl.sum()) / n if n else 0.0, k1, b)
    if imp.size and not bool((imp >= np.finfo(np.float32).tiny).all() and np.isfinite(imp).all()):
        raise ValueError("BM25 impacts must be positive normal fp32 values (check bm25_k1 / bm25_b)")
    return Postings(vocab, post_off, rows.astype(np.uint32), imp, dl, k1, b, post_tf)


def term_idf(n: int, df) -> np.ndarray:
    """idf[t] = log(1 + (n - df + 0.5) / (df + 0.5)) in fp64 (numpy's log: the host's, never the device's)."""
    df = np.asarray(df, dtype=np.float64)
    return np.log(1.0 + (n - df + 0.5) / (df + 0.5))


def impacts(tf, dl, df, n: int, avgdl: float, k1: float, b: float) -> np.ndarray:
    """float32(idf * ((tf * (k1 + 1)) / (tf + k1 * (1 - b + b * (dl / avgdl))))) elementwise over fp64
    arrays, idf = log(1 + (n - df + 0.5) / (df + 0.5)); every operation in fp64, in this order."""
    tf = np.asarray(tf, dtype=np.float64)
    dl = np.asarray(dl, dtype=np.float64)
    df = np.asarray(df, dtype=np.float64)
    idf = term_idf(n, df)
    norm = (1.0 - b) + b * (dl / avgdl)
    return (idf * ((tf * (k1 + 1.0)) / (tf + k1 * norm))).astype(np.float32)


def encode_queries(postings: Postings, texts: Sequence[str], analyzer: Analyzer | None = None):
    """Query texts -> the CSR batch (q_off int32 [B + 1], q_term int32, q_weight fp32): per query
    its distinct KNOWN terms in ascending id order, weight = float32(count).  More than 64 distinct
    known terms in one query raises ValueError (nothing is truncated)."""
    docs = (analyzer or analyze)(list(texts))
    if len(docs) != len(texts):
        raise ValueError("the analyzer must return one term list per text")
    off, terms, weights = [0], [], []
    for qi, d in enumerate(docs):
        counts: dict[int, int] = {}
        for t in d:
            i = postings.term_id.get(t)
            if i is not None:
                counts[i] = counts.get(i, 0) + 1
        if len(counts) > MAX_QUERY_TERMS:
            raise ValueError(f"query {qi} has {len(counts)} distinct known terms; BM25 search takes at most "
                             f"{MAX_QUERY_TERMS} per query")
        for i in sorted(counts):
            terms.append(i)
            weights.append(counts[i])
        off.append(len(terms))
    return (np.asarray(off, dtype=np.int32), np.asarray(terms, dtype=np.int32),
            np.asarray(weights, dtype=np.float32))


def build_positions(postings: Postings, texts: Sequence[str], analyzer: Analyzer | None = None):
    """Token positions of every posting -> (pos_off int64 [nnz + 1], pos uint32 [n_tokens]): posting q,
    that is (term, row) in post_row order, owns pos[pos_off[q] : pos_off[q + 1]], the ascending
    positions of the term in the row's term sequence.  texts / analyzer: what build_postings was given.
    Only PHRASE_MATCH reads positions, so they are built apart from the postings, when first needed."""
    docs = (analyzer or analyze)(list(texts))
    n = len(docs)
    if n != postings.n_rows:
        raise ValueError(f"build_positions: {n} texts for postings over {postings.n_rows} rows")
    dl = np.asarray([len(d) for d in docs], dtype=np.int64)
    total = int(dl.sum())
    flat = np.fromiter((postings.term_id[t] for d in docs for t in d), dtype=np.int64, count=total)
    rows = np.repeat(np.arange(n, dtype=np.int64), dl)
    starts = np.zeros(n, dtype=np.int64)
    np.cumsum(dl[:-1], out=starts[1:])
    position = np.arange(total, dtype=np.int64) - np.repeat(starts, dl)
    keys = flat * max(n, 1) + rows
    order = np.argsort(keys, kind="stable")   # (term, row), and within one the tokens stay in text order
    _, counts = np.unique(keys, return_counts=True)
    if counts.size != postings.nnz:
        raise ValueError("build_positions: the texts do not give the postings' (term, row) pairs")
    pos_off = np.zeros(postings.nnz + 1, dtype=np.int64)
    np.cumsum(counts, out=pos_off[1:])
    return pos_off, position[order].astype(np.uint32)


# ---- index maintenance (module docstring, "upkeep") -------------------------------------
class TermCounts:
    """What count_terms returns: the postings of a text list on its own, without impacts."""

    def __init__(self, vocab, post_off, post_row, post_tf, dl, pos_off, pos):
        self.vocab = vocab            # sorted distinct terms of these texts
        self.post_off = post_off      # int64 [V + 1]
        self.post_row = post_row      # uint32 [nnz], relative to the first text
        self.post_tf = post_tf        # uint32 [nnz]
        self.dl = dl                  # int64 [n]
        self.pos_off = pos_off        # int64 [nnz + 1]
        self.pos = pos                # uint32 [sum(dl)]

    @property
    def nnz(self) -> int:
        return int(self.post_row.size)


def count_terms(texts: Sequence[str], analyzer: Analyzer | None = None) -> TermCounts:
    """The (term, row) counts and token positions of a text list: the analyzer runs once over it."""
    docs = (analyzer or analyze)(list(texts))
    n = len(docs)
    if n != len(texts):
        raise ValueError("the analyzer must return one term list per text")
    vocab = sorted({t for d in docs for t in d})
    term_id = {t: i for i, t in enumerate(vocab)}
    dl = np.asarray([len(d) for d in docs], dtype=np.int64)
    total = int(dl.sum())
    flat = np.fromiter((term_id[t] for d in docs for t in d), dtype=np.int64, count=total)
    rows = np.repeat(np.arange(n, dtype=np.int64), dl)
    starts = np.zeros(n, dtype=np.int64)
    np.cumsum(dl[:-1], out=starts[1:])
    position = np.arange(total, dtype=np.int64) - np.repeat(starts, dl)
    keys = flat * max(n, 1) + rows
    order = np.argsort(keys, kind="stable")   # (term, row); the tokens of one stay in text order
    ukeys, tfs = np.unique(keys, return_counts=True)
    post_off = np.zeros(len(vocab) + 1, dtype=np.int64)
    np.cumsum(np.bincount(ukeys // max(n, 1), minlength=len(vocab)), out=post_off[1:])
    pos_off = np.zeros(ukeys.size + 1, dtype=np.int64)
    np.cumsum(tfs, out=pos_off[1:])
    return TermCounts(vocab, post_off, (ukeys % max(n, 1)).astype(np.uint32), tfs.astype(np.uint32), dl, pos_off,
                      position[order].astype(np.uint32))


def merge_vocab(vocab: list, term_id: dict, delta_vocab: list):
    """The sorted union of two sorted dictionaries -> (merged list, map_old int64 [V_old], map_delta
    int64 [V_delta]): the merged id of every old and of every delta term.  O(V_old + V_delta log V_old);
    with no new term the old list itself comes back."""
    import bisect
    fresh = [t for t in delta_vocab if t not in term_id]
    at = np.asarray([bisect.bisect_left(vocab, t) for t in fresh], dtype=np.int64)   # ascending: fresh is sorted
    map_old = np.arange(len(vocab), dtype=np.int64)
    merged = vocab
    if fresh:
        map_old += np.searchsorted(at, map_old, side="right")
        merged, last = [], 0
        for t, i in zip(fresh, at.tolist()):
            merged.extend(vocab[last:i])
            merged.append(t)
            last = i
        merged.extend(vocab[last:])
    fresh_id = dict(zip(fresh, (at + np.arange(at.size)).tolist()))
    map_delta = np.asarray([fresh_id[t] if t in fresh_id else int(map_old[term_id[t]]) for t in delta_vocab],
                           dtype=np.int64)
    return merged, map_old, map_delta


def merged_offsets(n_terms: int, post_off, map_old, delta_post_off, map_delta) -> np.ndarray:
    """post_off int64 [n_terms + 1] of an append: a merged term's df is its old df plus its delta df."""
    df = np.zeros(n_terms, dtype=np.int64)
    df[map_old] += np.diff(post_off)
    df[map_delta] += np.diff(delta_post_off)
    out = np.zeros(n_terms + 1, dtype=np.int64)
    np.cumsum(df, out=out[1:])
    return out


def rescored(vocab, post_off, post_row, post_tf, dl, k1: float, b: float) -> Postings:
    """Postings over the given counts: idf and the impacts by the definition."""
    n = int(dl.size)
    df = np.diff(post_off)
    imp = impacts(post_tf, dl[post_row.astype(np.int64)], np.repeat(df, df), n,
                  float(dl.sum()) / n if n else 0.0, k1, b)
    return Postings(vocab, post_off, post_row, imp, dl, k1, b, post_tf)


def _segments(lo, hi):
    """The indices of the ranges [lo[i], hi[i]) one after the other (two int64 arrays)."""
    n = hi - lo
    total = int(n.sum())
    starts = np.zeros(n.size, dtype=np.int64)
    np.cumsum(n[:-1], out=starts[1:])
    return np.repeat(lo - starts, n) + np.arange(total, dtype=np.int64)


def append_reference(postings: Postings, positions, delta: TermCounts):
    """The definition of an append in numpy -> (Postings, (pos_off, pos) | None).  positions: the pair
    of build_positions for `postings`, or None to leave positions out.  For tests and tools only."""
    vocab, map_old, map_delta = merge_vocab(postings.vocab, postings.term_id, delta.vocab)
    n_old = postings.n_rows
    post_off = merged_offsets(len(vocab), postings.post_off, map_old, delta.post_off, map_delta)
    nnz = int(post_off[-1])
    row = np.zeros(nnz, dtype=np.uint32)
    tf = np.zeros(nnz, dtype=np.uint32)
    cnt = np.zeros(nnz, dtype=np.int64)
    # where every old and every delta posting goes: the old segment first, the delta segment at the end
    t_old = np.repeat(np.arange(len(postings.vocab)), np.diff(postings.post_off))
    dst_old = post_off[map_old[t_old]] + (np.arange(postings.nnz) - postings.post_off[t_old])
    t_d = np.repeat(np.arange(len(delta.vocab)), np.diff(delta.post_off))
    dst_d = post_off[map_delta[t_d] + 1] - delta.post_off[t_d + 1] + np.arange(delta.nnz)
    row[dst_old], tf[dst_old] = postings.post_row, postings.post_tf
    row[dst_d], tf[dst_d] = delta.post_row + np.uint32(n_old), delta.post_tf
    out_pos = None
    if positions is not None:
        pos_off_old, pos_old = positions
        cnt[dst_old] = np.diff(pos_off_old)
        cnt[dst_d] = np.diff(delta.pos_off)
        pos_off = np.zeros(nnz + 1, dtype=np.int64)
        np.cumsum(cnt, out=pos_off[1:])
        pos = np.zeros(int(pos_off[-1]), dtype=np.uint32)
        pos[_segments(pos_off[dst_old], pos_off[dst_old + 1])] = pos_old
        pos[_segments(pos_off[dst_d], pos_off[dst_d + 1])] = delta.pos
        out_pos = (pos_off, pos)
    dl = np.concatenate([postings.dl, delta.dl])
    return rescored(vocab, post_off, row, tf, dl, postings.k1, postings.b), out_pos


def compact_reference(postings: Postings, positions, keep):
    """The definition of a compaction by a keep mask (bool [N]) in numpy -> (Postings, (pos_off, pos)
    | None).  For tests and tools only."""
    keep = np.asarray(keep, dtype=bool)
    row_map = np.where(keep, np.cumsum(keep) - 1, -1)
    kept = keep[postings.post_row.astype(np.int64)]
    term = np.repeat(np.arange(postings.n_terms), np.diff(postings.post_off))
    df = np.bincount(term[kept], minlength=postings.n_terms)
    alive = df > 0
    vocab = [t for t, a in zip(postings.vocab, alive.tolist()) if a]
    post_off = np.zeros(len(vocab) + 1, dtype=np.int64)
    np.cumsum(df[alive], out=post_off[1:])
    row = row_map[postings.post_row[kept].astype(np.int64)].astype(np.uint32)
    out_pos = None
    if positions is not None:
        pos_off_old, pos_old = positions
        cnt = np.diff(pos_off_old)[kept]
        pos_off = np.zeros(cnt.size + 1, dtype=np.int64)
        np.cumsum(cnt, out=pos_off[1:])
        q = np.flatnonzero(kept)
        out_pos = (pos_off, pos_old[_segments(pos_off_old[q], pos_off_old[q + 1])])
    return rescored(vocab, post_off, row, postings.post_tf[kept], postings.dl[keep], postings.k1, postings.b), out_pos


def _term_slice(postings: Postings, t: int) -> tuple[int, int]:
    if not 0 <= t < postings.n_terms:
        return 0, 0
    return int(postings.post_off[t]), int(postings.post_off[t + 1])


def text_match_reference(postings: Postings, positions, leaves, n_rows: int) -> np.ndarray:
    """The definition of rf_text_match in numpy -> uint32 [L, ceil(n_rows / 32)], bit r & 31 of word
    r >> 5 = row r passes; bits past n_rows are zero.  leaves: (kind, term ids, min_match) as in
    filter_expr.Program.text_leaves, kind 1 = MATCH (distinct ids), 2 = PHRASE (ids in phrase order);
    an id outside the dictionary has no postings.  positions: build_positions' pair (None when no
    leaf is a phrase).  For tests and tools only."""
    words = (n_rows + 31) // 32
    out = np.zeros((len(leaves), words), dtype=np.uint32)
    for li, (kind, ids, min_match) in enumerate(leaves):
        ids = [int(t) for t in ids]
        count = np.zeros(n_rows, dtype=np.int64)
        for t in sorted(set(ids)):
            lo, hi = _term_slice(postings, t)
            count[postings.post_row[lo:hi].astype(np.int64)] += 1
        if kind == 1:
            passing = count >= int(min_match)
        else:
            pos_off, pos = positions
            starts = None   # (row << 32 | start position) of the occurrences of p_0 .. p_i found so far
            for i, t in enumerate(ids):
                lo, hi = _term_slice(postings, t)
                rows = np.repeat(postings.post_row[lo:hi].astype(np.int64), np.diff(pos_off[lo:hi + 1]))
                at = pos[int(pos_off[lo]):int(pos_off[hi])].astype(np.int64) if hi > lo else np.zeros(0, dtype=np.int64)
                keep = at >= i
                key = (rows[keep] << 32) | (at[keep] - i)
                starts = key if starts is None else np.intersect1d(starts, key)
            passing = np.zeros(n_rows, dtype=bool)
            if starts is not None:
                passing[np.unique(starts >> 32)] = True
        bits = np.zeros(words * 32, dtype=np.uint8)
        bits[:n_rows] = passing
        out[li] = np.packbits(bits, bitorder="little").view(np.uint32)
    return out


def bm25_scores(postings: Postings, terms, weights, reverse: bool = False) -> np.ndarray:
    """The fp32 score of every row for one query (0 = holds no query term).  reverse: the terms taken
    in descending id order instead -- NOT the definition; tests use it to show that the order matters."""
    acc = np.zeros(postings.n_rows, dtype=np.float32)
    pairs = list(zip(np.asarray(terms).tolist(), np.asarray(weights, dtype=np.float32)))
    for t, w in (reversed(pairs) if reverse else pairs):
        sl = slice(int(postings.post_off[t]), int(postings.post_off[t + 1]))
        rows = postings.post_row[sl].astype(np.int64)
        acc[rows] = acc[rows] + (np.float32(w) * postings.post_imp[sl])   # two fp32 roundings, no fma
    return acc


def bm25_reference(postings: Postings, q_off, q_term, q_weight, k: int, mask=None, id_base: int = 0):
    """The definition of rf_sparse_search in numpy -> (scores fp32 [B, k], ids int64 [B, k], exact
    fp64 [B, k]), padded with -inf / -1.  mask: bool [N], the rows a filter passes."""
    B = len(q_off) - 1
    scores = np.full((B, k), -np.inf, dtype=np.float32)
    ids = np.full((B, k), -1, dtype=np.int64)
    for bi in range(B):
        sl = slice(int(q_off[bi]), int(q_off[bi + 1]))
        acc = bm25_scores(postings, q_term[sl], q_weight[sl])
        hit = acc > 0
        if mask is not None:
            hit &= np.asarray(mask, dtype=bool)
        rows = np.flatnonzero(hit)
        order = rows[np.lexsort((rows, -acc[rows].astype(np.float64)))][:k]
        scores[bi, :order.size] = acc[order]
        ids[bi, :order.size] = order + id_base
    return scores, ids, scores.astype(np.float64)


def rrf_reference(arms, k: int, rrf_k: float = 60.0, weights=None):
    """The definition of rf_fuse_rrf in Python floats (fp64).  arms: int64 [A, B, F], -1 = padding ->
    (scores fp32 [B, k], ids int64 [B, k], fused fp64 [B, k]), padded with -inf / -1."""
    arms = np.asarray(arms, dtype=np.int64)
    A, B, F = arms.shape
    w = [1.0] * A if weights is None else [float(x) for x in weights]
    if len(w) != A:
        raise ValueError(f"{A} arms but {len(w)} weights")
    fused = np.full((B, k), -np.inf, dtype=np.float64)
    ids = np.full((B, k), -1, dtype=np.int64)
    for bi in range(B):
        total: dict[int, float] = {}
        for a in range(A):
            seen = set()
            for j, d in enumerate(arms[a, bi].tolist()):
                if d < 0 or d in seen:
                    continue
                seen.add(d)
                total[d] = total.get(d, 0.0) + w[a] / (float(rrf_k) + float(j + 1))
        best = sorted(total.items(), key=lambda kv: (-kv[1], kv[0]))[:k]
        for j, (d, s) in enumerate(best):
            ids[bi, j] = d
            fused[bi, j] = s
    return fused.astype(np.float32), ids, fused
