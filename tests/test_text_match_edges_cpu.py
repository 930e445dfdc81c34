"""The corpora and leaves of tests/test_text_match_edges_gpu.py, and the proof (CPU only) that
lexical.text_match_reference agrees on every one of them with the definition on token lists.

The definition is written here on lexical.basic_tokens(text) and shares nothing with the postings:
  PHRASE  the row's token list holds the terms contiguously and in order
  MATCH   at least min_match of the leaf's DISTINCT terms occur in the row
A leaf is (kind, [term strings], min_match); `leaf_ids` turns the strings into dictionary ids."""
import functools

import numpy as np
import pytest

from rag_fin_amd import _lib, lexical

M, P = _lib.RF_TEXT_MATCH, _lib.RF_TEXT_PHRASE
TILE = _lib.RF_SPARSE_TILE_ROWS


# ---- the definition ------------------------------------------------------------------------------------
def row_passes(tokens, leaf):
    kind, terms, min_match = leaf
    if kind == P:
        m = len(terms)
        return m > 0 and any(tokens[j:j + m] == terms for j in range(len(tokens) - m + 1))
    return len(set(terms) & set(tokens)) >= min_match


def defined_rows(texts, leaf):
    leaf = (leaf[0], list(leaf[1]), leaf[2])
    return np.array([row_passes(lexical.basic_tokens(t), leaf) for t in texts], dtype=bool)


def pack(mask):
    bits = np.zeros((mask.size + 31) // 32 * 32, dtype=np.uint8)
    bits[:mask.size] = mask
    return np.packbits(bits, bitorder="little").view(np.uint32)


def leaf_ids(postings, leaves):
    """Term strings -> dictionary ids; a term no row holds gets an id past the dictionary (no postings)."""
    return [(kind, [postings.term_id.get(t, postings.n_terms + 7) for t in terms], mm) for kind, terms, mm in leaves]


class Corpus:
    def __init__(self, texts, leaves):
        self.texts, self.leaves = texts, leaves
        self.n = len(texts)
        self.words = (self.n + 31) // 32
        self.n_tiles = (self.n + TILE - 1) // TILE

    @functools.cached_property
    def postings(self):
        return lexical.build_postings(self.texts)

    @functools.cached_property
    def positions(self):
        return lexical.build_positions(self.postings, self.texts)

    @functools.cached_property
    def want(self):
        """uint32 [L, words]: the definition's bitmap of every leaf."""
        return np.stack([pack(defined_rows(self.texts, leaf)) for leaf in self.leaves])

    def rows(self, l):
        return np.flatnonzero(np.unpackbits(self.want[l].view(np.uint8), bitorder="little")[:self.n]).tolist()


# ---- long rows: more than 64 positions of a phrase's first term -----------------------------------------
# (k, hit): k repetitions of "aa bb xx", repetition number `hit` (1-based) replaced by "aa bb cc"; 0 = none.
# text_phrase_row takes the positions of "aa" 64 at a time: hit 64 is bit 63 of a FULL chunk (the ~0 mask),
# 65 the first bit of the second trip, 130 the third trip, (129, 128) bit 63 of the second full chunk.
LONG_KINDS = [(64, 64), (65, 65), (130, 130), (130, 0), (64, 1), (129, 128), "short", "none"]
LONG_N = TILE + 40


def long_row(kind):
    if kind == "short":
        return "aa bb cc"
    if kind == "none":
        return "f1 f2 f3"
    k, hit = kind
    reps = ["aa bb xx"] * k
    if hit:
        reps[hit - 1] = "aa bb cc"
    return " ".join(reps)


@functools.lru_cache(maxsize=None)
def long_rows():
    """Every kind once around each of row 0, both sides of the tile edge and the last row, rotated so that
    the four anchor rows themselves hold (65, 65), (130, 130), (64, 64) and (129, 128); filler elsewhere."""
    rng = np.random.default_rng(8)
    filler = ["f%d" % i for i in range(20)] + ["aa", "cc", "xx"]
    texts = [" ".join(rng.choice(filler, int(rng.integers(1, 8)))) for _ in range(LONG_N)]
    place = {}
    for first, anchor, kind in ((0, 0, (65, 65)), (TILE - 8, TILE - 1, (130, 130)), (TILE, TILE, (64, 64)),
                                (LONG_N - 8, LONG_N - 1, (129, 128))):
        shift = LONG_KINDS.index(kind) - (anchor - first)
        for j in range(8):
            place[first + j] = LONG_KINDS[(j + shift) % 8]
        assert place[anchor] == kind
    for r, kind in place.items():
        texts[r] = long_row(kind)
    leaves = [(P, ["aa", "bb", "cc"], 1), (P, ["cc", "aa"], 1), (P, ["aa"], 1), (M, ["aa", "cc"], 2)]
    c = Corpus(texts, leaves)
    c.place = place
    return c


# ---- corpus sizes ------------------------------------------------------------------------------------------
SIZES = [1, 31, 32, 33, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE]


@functools.lru_cache(maxsize=None)
def sized(n):
    rng = np.random.default_rng(1000 + n)
    vocab = ["s%d" % i for i in range(20)]
    lens = rng.integers(1, 7, n)
    draws = rng.integers(0, len(vocab), int(lens.sum()))
    texts, at = [], 0
    for ln in lens.tolist():
        texts.append(" ".join(vocab[i] for i in draws[at:at + ln]))
        at += ln
    texts[-1] = "s0 s1 s2"                # the last row passes both leaves: the last bit of the last word is live
    texts[0] = texts[0] + " s0 s1"
    return Corpus(texts, [(M, ["s0", "s2", "s5"], 2), (P, ["s0", "s1"], 1)])


# ---- a tile in which every row is a phrase candidate --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def candidates():
    n = TILE + 5
    texts = [("g%d pp qq h%d" if r % 2 == 0 else "g%d qq pp h%d") % (r % 7, r % 5) for r in range(n)]
    return Corpus(texts, [(P, ["pp", "qq"], 1), (P, ["qq", "pp"], 1), (M, ["pp", "qq"], 2)])


# ---- leaf shapes -------------------------------------------------------------------------------------------
SHAPES_N = TILE + 37
PHRASE64_FULL, PHRASE64_BROKEN = TILE, 100     # the row that holds the 64-term phrase, and the one off by its last term


@functools.lru_cache(maxsize=None)
def shapes():
    rng = np.random.default_rng(77)
    vocab = ["w%d" % i for i in range(120)]
    p = 1.0 / np.arange(1, len(vocab) + 1)
    p /= p.sum()
    lens = rng.integers(1, 24, SHAPES_N)
    draws = rng.choice(len(vocab), size=int(lens.sum()), p=p)
    texts, at = [], 0
    for ln in lens.tolist():
        texts.append(" ".join(vocab[i] for i in draws[at:at + ln]))
        at += ln
    phrase = [vocab[i] for i in rng.integers(0, 40, 64)]       # 64 terms, several of them more than once
    assert len(set(phrase)) < 64
    broken = phrase[:-1] + ["w119" if phrase[-1] != "w119" else "w118"]
    texts[PHRASE64_FULL] = "w3 " + " ".join(phrase) + " w4"
    texts[PHRASE64_BROKEN] = "w3 " + " ".join(broken) + " w4"
    texts[200] = "w7 w0 w0 w1 w7"
    texts[201] = "w0 w1 w0 w7"
    first64 = vocab[:64]
    leaves = [(P, phrase, 1), (P, broken, 1),
              (M, ["w0", "w0", "w9"], 2), (M, ["w0", "w0", "w9"], 3), (M, ["w0", "w9"], 2),
              (M, first64, 65), (M, first64, 12), (P, ["w0", "w0", "w1"], 1)]
    return Corpus(texts, leaves)


ALL = [("long", long_rows), ("candidates", candidates), ("shapes", shapes)] + [("sized-%d" % n, functools.partial(sized, n))
                                                                               for n in SIZES]


@pytest.mark.parametrize("name,make", ALL, ids=[a for a, _ in ALL])
def test_the_numpy_reference_equals_the_definition_on_token_lists(name, make):
    c = make()
    got = lexical.text_match_reference(c.postings, c.positions, leaf_ids(c.postings, c.leaves), c.n)
    assert got.shape == c.want.shape == (len(c.leaves), c.words)
    for l, leaf in enumerate(c.leaves):
        assert np.array_equal(got[l], c.want[l]), (leaf[0], leaf[1][:4], np.flatnonzero(got[l] != c.want[l])[:8])


def test_long_rows_pass_exactly_where_the_replaced_repetition_is():
    c = long_rows()
    hit = sorted(r for r, kind in c.place.items() if kind == "short" or (kind not in ("short", "none") and kind[1] > 0))
    assert c.rows(0) == hit and len(hit) == 4 * 6
    # "cc aa": the rare term first; its successor has more than 64 positions in the rows it passes here
    after = sorted(r for r, kind in c.place.items() if kind in ((64, 1), (129, 128)))
    assert set(after) <= set(c.rows(1)) and not set(c.rows(1)) & (set(c.place) - set(after))
    assert set(c.rows(2)) >= {r for r, kind in c.place.items() if kind != "none"}
    assert {0, TILE - 1, TILE, LONG_N - 1} <= set(c.place)
    tokens = lexical.basic_tokens(c.texts[TILE - 1])
    assert tokens.count("aa") == 130 and tokens[-1] == "cc"


def test_the_other_corpora_hold_what_their_names_say():
    c = candidates()
    assert c.rows(0) == list(range(0, c.n, 2)) and c.rows(1) == list(range(1, c.n, 2)) and c.rows(2) == list(range(c.n))
    s = shapes()
    assert s.rows(0) == [PHRASE64_FULL] and s.rows(1) == [PHRASE64_BROKEN] and len(s.leaves[0][1]) == 64
    assert s.rows(2) == s.rows(4) and len(s.rows(2)) > 10 and s.rows(3) == [] and s.rows(5) == []
    assert len(s.rows(6)) > 0 and {200} <= set(s.rows(7)) and 201 not in s.rows(7)
    for n in SIZES:
        z = sized(n)
        assert z.n == n and (n - 1) in z.rows(0) and (n - 1) in z.rows(1) and 0 in z.rows(1)
        assert n < 64 or 0 < len(z.rows(1)) < n
