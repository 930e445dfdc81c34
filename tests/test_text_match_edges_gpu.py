"""rf_text_match at the edges tests/test_text_match_gpu.py does not reach, against the definition on
token lists (tests/test_text_match_edges_cpu.py: the corpora, the leaves, and the expected bitmaps):

  long rows     more than 64 positions of a phrase's first term in one row: the second and third trip of
                text_phrase_row's 64-position loop, a full chunk's all-ones mask and its bit 63
  sizes         N below one ballot, around 32 / 64, and around one and two 8192-row tiles (exact multiples:
                the last tile is full)
  candidates    a tile in which all 8192 rows are phrase candidates
  leaf shapes   a 64-term phrase, a MATCH leaf that repeats an id, min_match above the term count, a
                phrase that starts with a repeated id
  words_per_leaf  given explicitly: above n_tiles * 256 (the tail-zeroing loop) and the minimum

Every call goes straight to the C ABI with the output prefilled with 0xFF bytes and four guard words
behind it: every word up to words_per_leaf must have been written, nothing past L * words_per_leaf."""
from ctypes import c_void_p

import numpy as np
import pytest

from rag_fin_amd import _lib, filter_expr as fe
from test_text_match_edges_cpu import (LONG_N, PHRASE64_BROKEN, PHRASE64_FULL, SIZES, TILE, candidates, leaf_ids, long_rows,
                                       shapes, sized)

pytestmark = pytest.mark.gpu

TILE_WORDS = TILE // 32
GUARD = 4
_INDEX = {}


def sparse_index(c, device):
    from rag_fin_amd.store import SparseIndex
    if id(c) not in _INDEX:
        sp = SparseIndex(c.postings, device)
        sp.attach_positions(*c.positions)
        _INDEX[id(c)] = (c, sp)
    return _INDEX[id(c)][1]


def run(c, device, leaves=None, words_per_leaf=None):
    """rf_text_match of the corpus' leaves -> uint32 [L, words_per_leaf] (default: the row words rounded
    up to four, what SparseIndex.text_match passes)."""
    import torch
    lib = _lib.load_library()
    sp = sparse_index(c, device)
    leaves = leaf_ids(c.postings, c.leaves if leaves is None else leaves)
    arr, terms = fe.text_leaf_arrays(fe.Program(text_leaves=leaves))
    L = len(arr)
    wpl = (c.words + 3) // 4 * 4 if words_per_leaf is None else words_per_leaf
    with torch.cuda.device(device):
        terms_d = torch.from_numpy(np.concatenate([terms, np.zeros(1, dtype=np.int32)])).to(device)
        out = torch.full((L * wpl + GUARD,), -1, dtype=torch.int32, device=device)
        ws = torch.empty(lib.rf_text_match_workspace_bytes(sp.handle, L), dtype=torch.uint8, device=device)
        _lib.check(lib.rf_text_match(sp.handle, arr, L, c_void_p(terms_d.data_ptr()), int(terms.size),
                                     c_void_p(out.data_ptr()), wpl, c_void_p(ws.data_ptr()), ws.numel(),
                                     _lib.current_stream_ptr()))
        torch.cuda.synchronize(device)
    got = out.cpu().numpy().view(np.uint32)
    assert (got[L * wpl:] == 0xFFFFFFFF).all(), "written past the last leaf's words"
    return got[:L * wpl].reshape(L, wpl).copy()


def check(c, got, want=None):
    want = c.want if want is None else want
    assert got.shape[0] == want.shape[0] and got.shape[1] >= c.words
    for l in range(want.shape[0]):
        assert np.array_equal(got[l, :c.words], want[l]), (l, np.flatnonzero(got[l, :c.words] != want[l])[:8])
    assert not got[:, c.words:].any()   # the pad words are written, and zero


def rows_of(words, n):
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n]).tolist()


def test_long_rows_beyond_sixty_four_positions(gpu_device):
    c = long_rows()
    got = run(c, gpu_device)
    # PHRASE "aa bb cc", row by row: (k, hit) with hit > 0 and the short row pass, (130, 0) and the rest do not
    passed = set(rows_of(got[0], c.n))
    for r, kind in sorted(c.place.items()):
        want = kind == "short" or (kind not in ("short", "none") and kind[1] > 0)
        assert (r in passed) == want, (r, kind)
    check(c, got)


@pytest.mark.parametrize("n", SIZES)
def test_corpus_sizes_around_a_ballot_and_a_tile(gpu_device, n):
    c = sized(n)
    got = run(c, gpu_device)
    assert got.shape == (2, (c.words + 3) // 4 * 4)
    check(c, got)
    if n % TILE == 0:      # the last tile is full: its last word is the leaf's last word, and its last bit is live
        assert c.n_tiles * TILE_WORDS == c.words and got[0, c.words - 1] >> 31 == 1 and got[1, c.words - 1] >> 31 == 1


def test_a_tile_in_which_every_row_is_a_candidate(gpu_device):
    c = candidates()
    got = run(c, gpu_device)
    assert rows_of(got[0], c.n) == list(range(0, c.n, 2))
    assert rows_of(got[1], c.n) == list(range(1, c.n, 2))
    check(c, got)


def test_leaf_shapes_and_the_same_bytes_twice(gpu_device):
    c = shapes()
    got = run(c, gpu_device)
    check(c, got)
    assert rows_of(got[0], c.n) == [PHRASE64_FULL] and rows_of(got[1], c.n) == [PHRASE64_BROKEN]
    assert np.array_equal(got[2], got[4]) and got[2].any()       # [a, a, b] with min_match 2 is [a, b] with 2
    assert not got[3].any() and not got[5].any()                 # min_match 3 of two distinct ids; 65 of 64
    again = run(c, gpu_device)
    assert got.tobytes() == again.tobytes()
    long = long_rows()
    assert run(long, gpu_device).tobytes() == run(long, gpu_device).tobytes()


@pytest.mark.parametrize("which", ["long", "one-full-tile"])
def test_explicit_words_per_leaf(gpu_device, which):
    c = long_rows() if which == "long" else sized(TILE)
    assert (c.n, c.n_tiles) == ((LONG_N, 2) if which == "long" else (TILE, 1))
    for extra in (c.n_tiles * TILE_WORDS + 8, c.words):     # past the tiles' words; the minimum
        for leaves in (c.leaves[:2], c.leaves[:1]):
            got = run(c, gpu_device, leaves, words_per_leaf=extra)
            assert got.shape == (len(leaves), extra)        # leaf l's words start at l * words_per_leaf
            check(c, got, c.want[:len(leaves)])
