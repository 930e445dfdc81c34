"""BM25 search on the GPU (rf_sparse_search through SparseIndex) against the definition,
restated here from a DENSE tf matrix so that it shares nothing with lexical.build_postings /
bm25_reference: impacts in fp64 rounded to fp32 once, acc = acc + (w * imp) in fp32 in ascending
term order, hits = rows holding a query term (and passing the filter), ranking (score desc, row asc).
Bar: ids, order and fp64 scores bit-identical, fp32 scores equal.

Corpus: seeded Zipf term draws (p ~ 1 / rank over 2 000 terms), 5..60 terms per row, N = 2 tiles + 37
rows (a partial last tile, hits on both sides of both tile boundaries); one row with three terms of
its own copied 40 times across the first tile boundary, so that exact ties fill more than k slots."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K1, B_ = 1.2, 0.75
V = 2000
N_COPIES = 40


def tile_rows():
    from rag_fin_amd import _lib
    return _lib.RF_SPARSE_TILE_ROWS


# ---- corpus and the dense restatement ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus():
    """The rows as term lists (read-only)."""
    T = tile_rows()
    n = 2 * T + 37
    rng = np.random.default_rng(2024)
    p = 1.0 / np.arange(1, V + 1)
    p /= p.sum()
    lens = rng.integers(5, 61, n)
    draws = rng.choice(V, size=int(lens.sum()), p=p)
    names = [f"w{i:04d}" for i in range(V)]
    docs, at = [], 0
    for ln in lens.tolist():
        docs.append([names[i] for i in draws[at:at + ln]])
        at += ln
    copied = ["zqa", "zqb", "zqb", "zqc"] + docs[100][:8]
    for r in range(T - N_COPIES // 2, T + N_COPIES // 2):
        docs[r] = list(copied)
    for r in (5, T + 100, 2 * T + 5, 2 * T + 30):   # a rare term: one hit in the first two tiles, two in the last
        docs[r] = docs[r] + ["rareterm"]
    return tuple(tuple(d) for d in docs)


def copy_rows():
    T = tile_rows()
    return np.arange(T - N_COPIES // 2, T + N_COPIES // 2)


@functools.lru_cache(maxsize=None)
def dense():
    """(vocab, term id map, tf int16 [N, V'], dl fp64 [N], idf fp64 [V']) of corpus()."""
    docs = corpus()
    vocab = sorted({t for d in docs for t in d})
    tid = {t: i for i, t in enumerate(vocab)}
    tf = np.zeros((len(docs), len(vocab)), dtype=np.int16)
    for r, d in enumerate(docs):
        for t in d:
            tf[r, tid[t]] += 1
    dl = np.asarray([len(d) for d in docs], dtype=np.float64)
    df = (tf > 0).sum(axis=0).astype(np.float64)
    idf = np.log(1.0 + (len(docs) - df + 0.5) / (df + 0.5))
    tf.setflags(write=False)
    return vocab, tid, tf, dl, idf


@functools.lru_cache(maxsize=None)
def scores_of(query: tuple):
    """fp32 score of every row for one query (a tuple of terms), 0 = no query term in the row."""
    _, tid, tf, dl, idf = dense()
    counts = {}
    for t in query:
        if t in tid:
            counts[tid[t]] = counts.get(tid[t], 0) + 1
    avgdl = dl.sum() / dl.size
    acc = np.zeros(dl.size, dtype=np.float32)
    for t in sorted(counts):
        tfc = tf[:, t].astype(np.float64)
        imp = (idf[t] * ((tfc * (K1 + 1.0)) / (tfc + K1 * (1.0 - B_ + B_ * (dl / avgdl))))).astype(np.float32)
        prod = np.float32(counts[t]) * imp
        has = tfc > 0
        acc[has] = acc[has] + prod[has]
    acc.setflags(write=False)
    return acc


def reference(queries, k, mask=None, id_base=0):
    scores = np.full((len(queries), k), -np.inf, dtype=np.float32)
    ids = np.full((len(queries), k), -1, dtype=np.int64)
    for b, q in enumerate(queries):
        acc = scores_of(tuple(q))
        hit = acc > 0
        if mask is not None:
            hit = hit & mask
        rows = np.flatnonzero(hit)
        order = rows[np.lexsort((rows, -acc[rows].astype(np.float64)))][:k]
        scores[b, :order.size] = acc[order]
        ids[b, :order.size] = order + id_base
    return scores, ids


@functools.lru_cache(maxsize=None)
def queries():
    """64 queries: the special ones first, then prefixes of rows spread over the three tiles."""
    docs = corpus()
    vocab, tid, tf, _, _ = dense()
    df = (tf > 0).sum(axis=0)
    common = [vocab[i] for i in np.argsort(-df, kind="stable")[:80] if not vocab[i].startswith("zq")]
    special = [
        docs[copy_rows()[0]],                       # 0: the copied row's own text
        ("w0003", "w0017", "w0003", "w0003"),       # 1: a repeated term
        ("rareterm",),                              # 2: one rare term, fewer than k hits
        ("nosuchterm", "neitherthis"),              # 3: no known term
        tuple(common[:64]),                         # 4: 64 distinct terms
    ]
    rng = np.random.default_rng(7)
    rest = []
    for r in rng.integers(0, len(docs), 64 - len(special)).tolist():
        rest.append(docs[r][:int(rng.integers(2, 10))])
    return tuple(tuple(q) for q in special + rest)


# ---- device side ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse(gpu_device):
    from rag_fin_amd import lexical
    from rag_fin_amd.index import SparseIndex
    postings = lexical.build_postings([" ".join(d) for d in corpus()], K1, B_)
    assert postings.vocab == dense()[0]
    return postings, SparseIndex(postings, gpu_device)


def run(sparse, qs, k, filt=None, id_base=0):
    from rag_fin_amd import lexical
    postings, sp = sparse
    enc = lexical.encode_queries(postings, [" ".join(q) for q in qs])
    return tuple(t.cpu().numpy() for t in sp.search(*enc, k, id_base=id_base, filt=filt))


def filter_of(mask, n_rows, device):
    """A filter buffer (rf_filter_from_mask) of a host bool mask, built for n_rows rows."""
    import torch
    from rag_fin_amd import _lib
    from rag_fin_amd.index import _ptr, mask_words
    lib = _lib.load_library()
    bits = torch.zeros(n_rows, dtype=torch.bool, device=device)
    bits[:min(n_rows, mask.size)] = torch.from_numpy(mask[:n_rows]).to(device)
    words = mask_words(bits)
    buf = torch.empty(lib.rf_filter_bytes(n_rows), dtype=torch.uint8, device=device)
    _lib.check(lib.rf_filter_from_mask(_ptr(words), n_rows, _ptr(buf), _lib.current_stream_ptr()))
    return buf


def assert_equal(got, want, what=""):
    scores, ids, exact = got
    ws, wi = want
    assert np.array_equal(ids, wi), f"{what}: ids differ at {np.argwhere(ids != wi)[:5].tolist()}"
    assert np.array_equal(scores, ws), f"{what}: fp32 scores differ"
    assert np.array_equal(exact, ws.astype(np.float64)), f"{what}: fp64 scores differ"


# ---- premises (CPU) -----------------------------------------------------------------------------------
def test_premises_of_the_corpus():
    T = tile_rows()
    qs = queries()
    assert len(corpus()) == 2 * T + 37 and len(qs) == 64
    # the copies tie exactly, straddle the tile boundary and are the best hits of their own text
    _, wi = reference(qs[:1], 64)
    assert np.array_equal(wi[0, :N_COPIES], copy_rows())
    assert copy_rows()[0] < T <= copy_rows()[-1]
    assert np.unique(scores_of(qs[0])[copy_rows()]).size == 1
    # the rare term has fewer than k hits, the unknown terms none, the long query 64 distinct known terms
    assert int((scores_of(qs[2]) > 0).sum()) == 4
    assert int((scores_of(qs[3]) > 0).sum()) == 0
    tid = dense()[1]
    assert len({tid[t] for t in qs[4]}) == 64
    # hits on both sides of both tile boundaries for the ordinary queries
    hit_tiles = {int(r) // T for q in qs[5:] for r in reference([q], 64)[1][0] if r >= 0}
    assert hit_tiles == {0, 1, 2}


# ---- parity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_matches_the_definition(sparse, B, k):
    qs = queries()[:B]
    assert_equal(run(sparse, qs, k), reference(qs, k), f"B={B} k={k}")


def test_special_queries_each_alone(sparse):
    for i in range(5):
        q = queries()[i:i + 1]
        got = run(sparse, q, 10, id_base=1000)
        assert_equal(got, reference(q, 10, id_base=1000), f"query {i}")
    assert (run(sparse, queries()[3:4], 10)[1] == -1).all()                 # no known term: empty
    ids = run(sparse, queries()[2:3], 10)[1]
    assert int((ids >= 0).sum()) == 4 and (ids[0, 4:] == -1).all()          # fewer than k hits: padded
    assert np.array_equal(run(sparse, queries()[:1], 10)[1][0], copy_rows()[:10])   # ties: lowest rows first


def test_filters(sparse, gpu_device):
    n = len(corpus())
    qs = queries()
    third = np.arange(n) % 3 == 0
    assert_equal(run(sparse, qs, 10, filt=filter_of(third, n, gpu_device)), reference(qs, 10, mask=third), "every third")
    none = np.zeros(n, dtype=bool)
    got = run(sparse, qs, 10, filt=filter_of(none, n, gpu_device))
    assert (got[1] == -1).all() and np.isneginf(got[0]).all() and np.isneginf(got[2]).all()
    # a header built for another row count passes no row
    other = filter_of(np.ones(n - 1, dtype=bool), n - 1, gpu_device)
    assert (run(sparse, qs[:3], 10, filt=other)[1] == -1).all()


def test_same_bits_on_every_run_and_for_every_batch_size(sparse):
    qs = queries()
    a = run(sparse, qs, 64)
    b = run(sparse, qs, 64)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for i in (0, 4, 17, 63):
        alone = run(sparse, qs[i:i + 1], 64)
        for x, y in zip(alone, a):
            assert x[0].tobytes() == y[i].tobytes(), f"query {i} alone differs from its row in the batch of 64"


def test_tiny_index(gpu_device):
    from rag_fin_amd import lexical
    from rag_fin_amd.index import SparseIndex
    texts = ["basic eps 15.22", "diluted eps 14.9", "net profit rose", "eps eps eps", "total income"]
    postings = lexical.build_postings(texts)
    sp = SparseIndex(postings, gpu_device)
    enc = lexical.encode_queries(postings, ["eps", "income of the bank", "eps profit"])
    scores, ids, exact = (t.cpu().numpy() for t in sp.search(*enc, 10))
    ws, wi, we = lexical.bm25_reference(postings, *enc, 10)
    assert np.array_equal(ids, wi) and np.array_equal(scores, ws) and np.array_equal(exact, we)
    assert sorted(ids[0][ids[0] >= 0].tolist()) == [0, 1, 3] and (ids[0, 3:] == -1).all()
    assert ids[1].tolist() == [4] + [-1] * 9


def test_more_tiles_than_the_merge_has_threads(gpu_device):
    """Above 256 tiles a thread of the merge kernel owns several tile lists and finds its next head by
    another path (the largest key below the one just taken) than with one list and a cursor.  259
    tiles; the hits sit in tiles 0, 1, 2 and 256, 257, 258 -- lists of the SAME three threads -- and in
    two tiles between, 12 per tile with 12 row lengths, so scores tie across tiles and k = 64 of the 96
    hits interleave the lists.  Every other row holds one term the queries do not use.  The expected
    answer is restated from the rows that hold a query term."""
    from rag_fin_amd import lexical
    from rag_fin_amd.index import SparseIndex
    T = tile_rows()
    n = 258 * T + 100
    texts = ["o"] * n
    special = {}
    for tile in (0, 1, 2, 100, 255, 256, 257, 258):
        for j in range(12):
            row = tile * T + (7 * j + 3 * tile) % min(T, n - tile * T)
            special[row] = j
            texts[row] = "hit" + " f" * j
    assert len(special) == 96 and max(special) < n and (n + T - 1) // T == 259
    postings = lexical.build_postings(texts)
    sp = SparseIndex(postings, gpu_device)
    enc = lexical.encode_queries(postings, ["hit", "f hit f"])
    rows = np.array(sorted(special))
    tf_f = np.array([special[r] for r in rows], dtype=np.float64)
    dl = 1.0 + tf_f
    avgdl = (n + tf_f.sum()) / n
    norm = 1.0 - B_ + B_ * (dl / avgdl)

    def imp(tf, df):
        idf = np.log(1.0 + (n - df + 0.5) / (df + 0.5))
        with np.errstate(invalid="ignore"):
            return (idf * ((tf * (K1 + 1.0)) / (tf + K1 * norm))).astype(np.float32)

    imp_hit, imp_f = imp(np.ones(96), 96.0), imp(tf_f, float((tf_f > 0).sum()))
    acc1 = np.zeros(96, dtype=np.float32) + np.float32(1.0) * imp_hit
    acc2 = np.zeros(96, dtype=np.float32)
    acc2[tf_f > 0] = acc2[tf_f > 0] + (np.float32(2.0) * imp_f)[tf_f > 0]       # "f" sorts before "hit"
    acc2 = acc2 + np.float32(1.0) * imp_hit
    assert postings.term_id["f"] < postings.term_id["hit"]
    for k in (10, 64):
        scores, ids, exact = (t.cpu().numpy() for t in sp.search(*enc, k, id_base=5))
        for b, acc in enumerate((acc1, acc2)):
            order = np.lexsort((rows, -acc.astype(np.float64)))[:k]
            assert np.array_equal(ids[b], rows[order] + 5), (k, b)
            assert np.array_equal(scores[b], acc[order]) and np.array_equal(exact[b], acc[order].astype(np.float64))
            if k == 64:
                tiles = (ids[b] - 5) // T
                assert {0, 256} <= set(tiles.tolist()) and (np.diff(tiles) < 0).any()   # the lists interleave
