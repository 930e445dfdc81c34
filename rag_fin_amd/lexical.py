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


class Postings:
    """What build_postings returns: the dictionary and the three posting arrays, host numpy."""

    def __init__(self, vocab, post_off, post_row, post_imp, dl, k1, b):
        self.vocab = vocab                        # sorted distinct terms; id = position
        self.term_id = {t: i for i, t in enumerate(vocab)}
        self.post_off = post_off                  # int64 [V + 1]
        self.post_row = post_row                  # uint32 [nnz], ascending within a term
        self.post_imp = post_imp                  # fp32 [nnz]
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
    tfs = tfs.astype(np.float64)
    df = np.bincount(tids, minlength=len(vocab)).astype(np.float64)
    post_off = np.zeros(len(vocab) + 1, dtype=np.int64)
    np.cumsum(df.astype(np.int64), out=post_off[1:])
    imp = impacts(tfs, dl[rows].astype(np.float64), df[tids], n, float(dl.sum()) / n if n else 0.0, k1, b)
    if imp.size and not bool((imp >= np.finfo(np.float32).tiny).all() and np.isfinite(imp).all()):
        raise ValueError("BM25 impacts must be positive normal fp32 values (check bm25_k1 / bm25_b)")
    return Postings(vocab, post_off, rows.astype(np.uint32), imp, dl, k1, b)


def impacts(tf, dl, df, n: int, avgdl: float, k1: float, b: float) -> np.ndarray:
    """float32(idf * ((tf * (k1 + 1)) / (tf + k1 * (1 - b + b * (dl / avgdl))))) elementwise over fp64
    arrays, idf = log(1 + (n - df + 0.5) / (df + 0.5)); every operation in fp64, in this order."""
    tf = np.asarray(tf, dtype=np.float64)
    dl = np.asarray(dl, dtype=np.float64)
    df = np.asarray(df, dtype=np.float64)
    idf = np.log(1.0 + (n - df + 0.5) / (df + 0.5))
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
