"""The lexical index build on the GPU: rf_sparse_count_plan / _apply through
SparseIndex.count_tokens / .from_tokens, bit for bit against the numpy definition
(lexical.counts_from_tokens, itself checked against count_terms on the CPU) on token streams whose
shapes aim at the edges of the radix sort (wave, round, tile, pass count) and of the scans; then a
CorpusStore built by the device route against lexical.build_postings / build_positions of the same
texts, through writes on top, and against the host route's answers."""
import functools

import numpy as np
import pytest

from oracle import synth_text
from rag_fin_amd import _lib, lexical
from test_analyzer_native_cpu import MORE_EDGE
from test_tokenizer import EDGE

pytestmark = pytest.mark.gpu

T = _lib.RF_LEX_SORT_TILE
CHUNK = _lib.RF_LEX_CHUNK
PARAMS = [(1.2, 0.75), (0.0, 0.75), (1.2, 0.0), (1.2, 1.0)]   # tests/test_lexical_update_gpu.py's


def device_counts(device, tok, dl, n_terms, positions):
    from rag_fin_amd.index import SparseIndex
    post_off, row, tf, pos = SparseIndex.count_tokens(n_terms, tok, dl, device, positions)
    out = [post_off, row.cpu().numpy().view(np.uint32), tf.cpu().numpy().view(np.uint32)]
    if positions:
        out += [pos[0].cpu().numpy(), pos[1].cpu().numpy().view(np.uint32)]
    return out


def check(device, tok, dl, n_terms, twice=False):
    tok, dl = np.asarray(tok, dtype=np.int32), np.asarray(dl, dtype=np.int64)
    assert int(dl.sum()) == tok.size
    want = lexical.counts_from_tokens(tok, dl, n_terms)
    ref = [want.post_off, want.post_row, want.post_tf, want.pos_off, want.pos]
    names = ["post_off", "post_row", "post_tf", "pos_off", "pos"]
    for positions in (False, True):
        for _ in range(2 if twice else 1):
            got = device_counts(device, tok, dl, n_terms, positions)
            for name, g, w in zip(names, got, ref):
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), \
                    (name, positions, int((g != w).sum()) if g.shape == w.shape else (g.shape, w.shape))
    return want


def split_rows(rng, n_tokens, n_rows):
    """dl of n_rows rows that hold n_tokens tokens, cut at random places (empty rows included)."""
    cuts = np.sort(rng.integers(0, n_tokens + 1, n_rows - 1))
    return np.diff(np.concatenate([[0], cuts, [n_tokens]]))


SIZES = [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1]


@pytest.mark.parametrize("n_tokens", SIZES)
def test_one_term_at_the_wave_round_and_tile_edges(gpu_device, n_tokens):
    rng = np.random.default_rng(n_tokens)
    check(gpu_device, np.zeros(n_tokens), split_rows(rng, n_tokens, min(n_tokens, 7)), 1)


@pytest.mark.parametrize("n_tokens", SIZES)
def test_random_terms_at_the_wave_round_and_tile_edges(gpu_device, n_tokens):
    rng = np.random.default_rng(100 + n_tokens)
    check(gpu_device, rng.integers(0, 300, n_tokens), split_rows(rng, n_tokens, max(1, n_tokens // 9)), 300)


@pytest.mark.parametrize("n_terms", [1, 2, 255, 256, 257, 65535, 65536, 65537, 200000])
def test_the_pass_count_and_terms_without_a_posting(gpu_device, n_terms):
    """1 -> 2 -> 3 passes at 256 / 257 and 65 536 / 65 537 terms; the largest id is always there, most
    terms of the large dictionaries hold no posting (200 000 terms: fewer tokens than terms)."""
    rng = np.random.default_rng(n_terms)
    n_tokens = 2 * T + 37
    tok = rng.integers(0, n_terms, n_tokens)
    tok[rng.integers(0, n_tokens, 5)] = 0
    tok[rng.integers(0, n_tokens, 5)] = n_terms - 1
    check(gpu_device, tok, split_rows(rng, n_tokens, 500), n_terms)


def test_a_wave_on_one_digit_and_the_end_digits_only(gpu_device):
    rng = np.random.default_rng(5)
    n_tokens = T + 300
    one_digit_per_wave = np.repeat(rng.integers(0, 256, (n_tokens + 63) // 64), 64)[:n_tokens]
    check(gpu_device, one_digit_per_wave, split_rows(rng, n_tokens, 40), 256)
    ends = rng.choice([0, 255], n_tokens)
    check(gpu_device, ends, split_rows(rng, n_tokens, 40), 256)
    # the same in the second digit: ids 0 and 255 << 8, and in both at once
    check(gpu_device, ends * 256, split_rows(rng, n_tokens, 40), 65536)
    check(gpu_device, ends * 257, split_rows(rng, n_tokens, 40), 65536)


def test_one_term_fills_several_tiles_between_others(gpu_device):
    """Stability across waves, rounds and tiles: a term of 3 T + 1 tokens spread over every row keeps
    (row, position) order, with smaller and larger ids around and inside it."""
    rng = np.random.default_rng(6)
    big = np.full(3 * T + 1, 7)
    tok = np.concatenate([rng.integers(0, 7, 500), big, rng.integers(8, 1000, 500)])
    tok[rng.integers(0, tok.size, 200)] = rng.integers(0, 1000, 200)
    check(gpu_device, tok, split_rows(rng, tok.size, 300), 1000)
    check(gpu_device, rng.permutation(tok), split_rows(rng, tok.size, 300), 1000)


def test_one_row_whose_single_term_repeats_across_tiles(gpu_device):
    n = 3 * T + 1
    want = check(gpu_device, np.full(n, 3), [n], 5)
    assert want.post_tf.tolist() == [n] and want.post_row.tolist() == [0]
    assert np.array_equal(want.pos, np.arange(n, dtype=np.uint32))
    # the same row between two others, the term also in them
    want = check(gpu_device, np.full(n + 5, 3), [2, n, 3], 5)
    assert want.post_tf.tolist() == [2, n, 3]


def test_empty_rows_first_last_and_in_runs_and_a_row_across_a_tile_edge(gpu_device):
    rng = np.random.default_rng(8)
    dl = np.asarray([0, 0, 5, 0, T - 3, 0, 0, 0, 9, 1, 0, 2 * T, 0, 0])     # row 4 holds tokens 5 .. T + 1: across the tile edge
    tok = rng.integers(0, 40, int(dl.sum()))
    check(gpu_device, tok, dl, 40)
    check(gpu_device, np.full(int(dl.sum()), 2), dl, 40)                     # tf = dl: every row's run crosses what it crosses
    check(gpu_device, rng.integers(0, 40, T + 10), [T + 10], 40)             # n_rows = 1
    check(gpu_device, [4], [0, 0, 1, 0], 9)


@pytest.mark.parametrize("seed", range(20))
def test_seeded_random_streams_twice_with_identical_bits(gpu_device, seed):
    rng = np.random.default_rng(1000 + seed)
    n_tokens = int(rng.integers(1, 50001))
    n_terms = int(rng.choice([3, 200, 256, 5000, 70000]))
    tok = np.minimum(rng.zipf(1.3, n_tokens) - 1, n_terms - 1)
    if seed % 3 == 0:
        tok = rng.permutation(n_terms)[tok]                                 # the frequent terms anywhere in the id range
    n_rows = int(rng.integers(1, max(2, n_tokens // 4)))
    check(gpu_device, tok, split_rows(rng, n_tokens, n_rows), n_terms, twice=True)


@pytest.mark.parametrize("nnz", [CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1])
def test_nnz_and_the_head_scan_cross_the_chunk_edge(gpu_device, nnz):
    """Every token a posting of its own (nnz = n_tokens: the head scan holds nnz + 1 entries), then
    the same postings with repeats, so that n_tokens is well past the edge and nnz at it."""
    rng = np.random.default_rng(nnz)
    tok = rng.permutation(nnz)
    check(gpu_device, tok, np.ones(nnz, dtype=np.int64), nnz)
    dl = rng.integers(1, 4, nnz)
    check(gpu_device, np.repeat(tok, dl), dl, nnz)


def test_ids_out_of_range_are_clamped(gpu_device):
    tok = np.asarray([5, -1, 99, 2, -2147483648, 2147483647, 3], dtype=np.int32)
    got = device_counts(gpu_device, tok, np.asarray([3, 4]), 6, True)
    want = lexical.counts_from_tokens(np.clip(tok, 0, 5), [3, 4], 6)
    for g, w in zip(got, [want.post_off, want.post_row, want.post_tf, want.pos_off, want.pos]):
        assert np.array_equal(g, w)


# ---- the store ---------------------------------------------------------------------------------------------
N0, DIM = 3000, 64
COS = {"metric_type": "COSINE"}
BM25 = {"metric_type": "BM25"}
QTEXTS = ["total deposits of the bank", "net profit after tax, net profit", "provision coverage ratio 7"]
FILTERS = ['TEXT_MATCH(text, "deposits")', 'PHRASE_MATCH(text, "net profit")',
           'TEXT_MATCH(text, "profit tax capital", minimum_should_match=2) and not PHRASE_MATCH(text, "of the")']


@functools.lru_cache(maxsize=None)
def corpus():
    texts = synth_text.retemplated_texts(N0 + 64, 23) + EDGE + MORE_EDGE
    rng = np.random.default_rng(24)
    x = rng.standard_normal((len(texts), DIM))
    v16 = np.ascontiguousarray((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16))
    return texts, v16


def build_store(device, idx, k1=1.2, b=0.75, analyzer=None):
    import torch
    from rag_fin_amd.store import CorpusStore
    texts, v16 = corpus()
    st = CorpusStore("b", dim=DIM, capacity=len(texts) + 64, device=device)
    st.analyzer = analyzer
    st.add([f"k{i}" for i in idx], [texts[i] for i in idx], torch.from_numpy(v16[idx]).to(device), [f"P{i % 5}" for i in idx],
           ["t"] * len(idx), ["s"] * len(idx), [float(i) for i in idx])
    st.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25",
                               "params": {"bm25_k1": k1, "bm25_b": b}})
    return st


@functools.lru_cache(maxsize=None)
def host_reference(idx, k1, b):
    """lexical.build_postings / build_positions of the rows `idx` (a tuple), computed once per session."""
    texts, _ = corpus()
    rows = [texts[i] for i in idx]
    p = lexical.build_postings(rows, k1, b)
    return p, lexical.build_positions(p, rows)


def assert_store_equals_host_build(st, idx, k1, b, positions=True):
    want, (pos_off, pos) = host_reference(tuple(idx), k1, b)
    postings, sp = st._lexical.built
    assert postings.vocab == want.vocab and postings.term_id == want.term_id
    assert np.array_equal(postings.post_off, want.post_off) and postings.post_off.dtype == np.int64
    assert np.array_equal(postings.dl, want.dl)
    assert np.array_equal(postings.post_row, want.post_row) and np.array_equal(postings.post_tf, want.post_tf)
    assert np.array_equal(postings.post_imp.view(np.uint32), want.post_imp.view(np.uint32))
    assert np.array_equal(sp.post_off.cpu().numpy(), want.post_off)
    assert np.array_equal(sp.dl.cpu().numpy(), want.dl) and sp.supports_update
    if positions:
        assert sp.positions is not None
        assert np.array_equal(sp.positions[0].cpu().numpy(), pos_off)
        assert np.array_equal(sp.positions[1].cpu().numpy().view(np.uint32), pos)


def answers(st, device):
    import torch
    from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
    _, v16 = corpus()
    q = torch.from_numpy(np.array(v16[:3])).to(device)
    hits = lambda res: [[(h.id, h.row, np.float32(h.score).view(np.uint32).item()) for h in r] for r in res]   # noqa: E731
    out = [hits(st.search(QTEXTS, "sparse", BM25, limit=20))]
    out += [st.filter_rows(f).tolist() for f in FILTERS]
    out.append(hits(st.search(QTEXTS, "sparse", BM25, limit=10, expr=FILTERS[1])))
    out.append(hits(st.hybrid_search([AnnSearchRequest(q, "embedding", COS, limit=20),
                                      AnnSearchRequest(QTEXTS, "sparse", BM25, limit=20)], RRFRanker(), limit=10)))
    return out


@pytest.mark.parametrize("k1,b", PARAMS)
def test_a_store_built_on_the_device_equals_the_host_build(gpu_device, monkeypatch, k1, b):
    monkeypatch.setenv("RAGFIN_LEXICAL_BUILD", "device")
    texts, _ = corpus()
    idx = [i for i in range(len(texts)) if not N0 <= i < N0 + 64]          # the retemplated texts and every edge text
    st = build_store(gpu_device, idx, k1, b)
    monkeypatch.setattr(lexical, "build_postings", None)                     # the host build is not what runs
    monkeypatch.setattr(lexical, "build_positions", None)
    assert st.search(QTEXTS, "sparse", BM25, limit=5)[0]
    assert st._lexical.route == "device" and st._lexical.built[1].positions is None
    assert st.filter_rows(FILTERS[1]).size > 0                               # the first phrase: positions, on the device
    monkeypatch.undo()
    assert_store_equals_host_build(st, idx, k1, b)


def test_writes_on_top_of_a_device_built_index_equal_a_fresh_host_build(gpu_device, monkeypatch):
    import torch
    monkeypatch.setenv("RAGFIN_LEXICAL_BUILD", "device")
    texts, v16 = corpus()
    idx = list(range(N0))
    st = build_store(gpu_device, idx)
    assert st.filter_rows(FILTERS[1]).size > 0 and st._lexical.route == "device"
    first = st._lexical.built[1]

    def batch(keys, rows):
        return [keys, [texts[i] for i in rows], torch.from_numpy(v16[rows]).to(gpu_device), [f"P{i % 5}" for i in rows],
                ["t"] * len(rows), ["s"] * len(rows), [float(i) for i in rows]]
    new = list(range(N0, N0 + 16))
    st.insert(batch([f"k{i}" for i in new], new))                            # an add
    idx = idx + new
    assert st.search(QTEXTS, "sparse", BM25, limit=5)[0]
    assert_store_equals_host_build(st, idx, 1.2, 0.75)
    up = list(range(N0 + 16, N0 + 32))
    keys = [f"k{i}" for i in idx[10:18]] + [f"k{i}" for i in up[8:]]         # eight restated rows and eight new ones
    assert st.upsert(batch(keys, up)).upsert_count == 16
    idx = idx[:10] + idx[18:] + up
    assert st.search(QTEXTS, "sparse", BM25, limit=5)[0]
    assert_store_equals_host_build(st, idx, 1.2, 0.75)
    assert st.delete('period == "P3"').delete_count > 0                      # a delete
    idx = [i for i in idx if i % 5 != 3]
    assert st.search(QTEXTS, "sparse", BM25, limit=5)[0]
    assert_store_equals_host_build(st, idx, 1.2, 0.75)
    assert st._lexical.built[1] is not first and st._lexical.route == "device"


def test_answers_equal_the_host_routes_and_a_custom_analyzer_stays_on_the_host(gpu_device, monkeypatch):
    idx = list(range(0, N0, 2))
    monkeypatch.setenv("RAGFIN_LEXICAL_BUILD", "host")
    host = build_store(gpu_device, idx)
    want = answers(host, gpu_device)
    assert host._lexical.route == "host"
    monkeypatch.setenv("RAGFIN_LEXICAL_BUILD", "auto")
    dev = build_store(gpu_device, idx)
    assert answers(dev, gpu_device) == want
    assert dev._lexical.route == "device"                                    # auto: every non-empty corpus
    monkeypatch.setenv("RAGFIN_LEXICAL_BUILD", "device")
    dev = build_store(gpu_device, idx)
    assert answers(dev, gpu_device) == want and dev._lexical.route == "device"
    assert dev.lexical_fallback_reason is None

    def broken(texts, *args, **kw):
        raise OSError("no analyzer today")
    monkeypatch.setattr(lexical, "analyze_native", broken)                   # the device route raises: seen, not silent
    fell = build_store(gpu_device, idx)
    with pytest.warns(RuntimeWarning, match="the device route failed for the first build: OSError: no analyzer today"):
        got = answers(fell, gpu_device)
    assert got == want and fell._lexical.route == "host" and "no analyzer today" in fell.lexical_fallback_reason
    monkeypatch.undo()
    monkeypatch.setenv("RAGFIN_LEXICAL_BUILD", "device")
    custom = build_store(gpu_device, idx, analyzer=lexical.analyze)
    assert answers(custom, gpu_device) == want and custom._lexical.route == "host"
    monkeypatch.setenv("RAGFIN_LEXICAL_BUILD", "gpu")
    with pytest.raises(ValueError, match="RAGFIN_LEXICAL_BUILD"):
        build_store(gpu_device, idx).search(QTEXTS, "sparse", BM25, limit=5)
