"""Hybrid search on the GPU: rf_fuse_rrf against lexical.rrf_reference, and CorpusStore.hybrid_search
end to end against the three definitions composed on the host -- the dense oracle (oracle/search.py)
for the "embedding" arm, a BM25 restatement (below, from per-row term counts; it shares nothing with
lexical.build_postings) for the "sparse" arm, and the RRF definition restated below.  Bar: rows and
order identical, fused scores bit-identical.

Store: 3 000 rows, dim 64.  Texts come from a template (line item, period label, a figure, a segment),
vectors are clustered independently of the texts, so the two arms disagree and the fused list differs
from the dense one (asserted)."""
import functools
import math

import numpy as np
import pytest

from oracle import encoder as oenc
from oracle import search as osearch
from rag_fin_amd import lexical

pytestmark = pytest.mark.gpu

N, DIM, NQ = 3000, 64, 12
ITEMS = ["basic eps", "diluted eps", "net profit", "net interest income", "total deposits", "gross npa", "net npa",
         "capital adequacy ratio", "operating expenses", "fee income", "treasury income", "provision coverage",
         "return on assets", "cost to income", "casa ratio", "retail advances"]
PERIODS = ["Q1_FY2023", "Q2_FY2023", "Q3_FY2023", "Q4_FY2023", "Q1_FY2024"]
SEGMENTS = ["retail banking", "wholesale banking", "treasury", "insurance", "other banking"]
COS = {"metric_type": "COSINE"}
BM25 = {"metric_type": "BM25"}
SPARSE = {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"}


# ---- data -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def data():
    rng = np.random.default_rng(321)
    item = rng.integers(0, len(ITEMS), N)
    period = rng.integers(0, len(PERIODS), N)
    seg = rng.integers(0, len(SEGMENTS), N)
    value = rng.integers(100, 4000, N)
    texts = [f"{ITEMS[i]} for {PERIODS[p]} was {v / 100:.2f} in the {SEGMENTS[s]} segment"
             for i, p, v, s in zip(item.tolist(), period.tolist(), value.tolist(), seg.tolist())]
    centres = rng.standard_normal((30, DIM))
    x = centres[rng.integers(0, 30, N)] + 0.4 * rng.standard_normal((N, DIM))
    c16 = np.ascontiguousarray((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16))
    xq = centres[rng.integers(0, 30, NQ)] + 0.4 * rng.standard_normal((NQ, DIM))
    q16 = np.ascontiguousarray((xq / np.linalg.norm(xq, axis=1, keepdims=True)).astype(np.float16))
    qtexts = [f"{ITEMS[rng.integers(0, len(ITEMS))]} {PERIODS[rng.integers(0, len(PERIODS))]} "
              f"{value[rng.integers(0, N)] / 100:.2f}" for _ in range(NQ)]
    qtexts[3] = "basic EPS, Q1_FY2024: basic eps?"        # repeated terms, punctuation, case
    qtexts[5] = "dividend payout"                         # no known term: the dense arm alone
    c16.setflags(write=False)
    q16.setflags(write=False)
    return texts, [PERIODS[p] for p in period.tolist()], c16, q16, qtexts


def make_store(device, rows=None):
    import torch
    from rag_fin_amd.store import CorpusStore
    texts, periods, c16, _, _ = data()
    rows = list(range(N)) if rows is None else rows
    st = CorpusStore("h", dim=DIM, capacity=N, device=device)
    st.add([f"k{i}" for i in rows], [texts[i] for i in rows], torch.from_numpy(c16[rows]).to(device),
           [periods[i] for i in rows], ["t"] * len(rows), ["s"] * len(rows), [float(i) for i in rows])
    st.create_index("sparse", SPARSE)
    return st


# ---- the definitions, restated ------------------------------------------------------------------------
def bm25_restated(texts, qtexts, k, mask=None, k1=1.2, b=0.75):
    """Top-k row lists per query, from per-row term counts."""
    docs = [lexical.basic_tokens(t) for t in texts]
    n = len(docs)
    vocab = sorted({w for d in docs for w in d})
    dl = np.array([len(d) for d in docs], dtype=np.float64)
    avgdl = dl.sum() / n
    counts = [{w: d.count(w) for w in set(d)} for d in docs]
    out = []
    for q in qtexts:
        qc = {}
        for w in lexical.basic_tokens(q):
            if w in vocab:
                qc[w] = qc.get(w, 0) + 1
        acc = np.zeros(n, dtype=np.float32)
        for w in sorted(qc):                                  # sorted terms = ascending term ids
            tf = np.array([c.get(w, 0) for c in counts], dtype=np.float64)
            df = float((tf > 0).sum())
            idf = np.log(1.0 + (n - df + 0.5) / (df + 0.5))
            imp = (idf * ((tf * (k1 + 1.0)) / (tf + k1 * (1.0 - b + b * (dl / avgdl))))).astype(np.float32)
            has = tf > 0
            acc[has] = acc[has] + (np.float32(qc[w]) * imp)[has]
        hit = acc > 0 if mask is None else (acc > 0) & mask
        rows = np.flatnonzero(hit)
        out.append(rows[np.lexsort((rows, -acc[rows].astype(np.float64)))][:k].tolist())
    return out


def dense_oracle(q16, c16, k, mask=None):
    s = osearch.exact_scores(q16, c16)
    if mask is not None:
        s = np.where(mask[None, :], s, -np.inf)
    ws, wi = osearch.topk_from_scores(s, k)
    return [[i for i, v in zip(r.tolist(), sc.tolist()) if i >= 0 and v > -math.inf] for r, sc in zip(wi, ws)]


def rrf_restated(lists, k, rrf_k=60.0, weights=None):
    """lists: per arm one ranked id list -> [(id, fused)] best first."""
    w = weights or [1.0] * len(lists)
    fused = {}
    for a, ids in enumerate(lists):
        for j, d in enumerate(ids):
            fused[d] = fused.get(d, 0.0) + w[a] / (rrf_k + (j + 1))
    return sorted(fused.items(), key=lambda kv: (-kv[1], kv[0]))[:k]


# ---- rf_fuse_rrf --------------------------------------------------------------------------------------
def _arms(A, F, B, kind, seed):
    rng = np.random.default_rng(seed)
    arms = np.full((A, B, F), -1, dtype=np.int64)
    for a in range(A):
        for b in range(B):
            if kind == "identical":
                ids = np.random.default_rng(seed + b).permutation(5 * F)[:F] + 2 ** 33
            elif kind == "disjoint":
                ids = rng.permutation(5 * F)[:F] + a * 10 ** 6
            else:   # overlapping draws from a small pool, with a padded tail of random length
                ids = rng.permutation(2 * F)[:F]
                ids[F - int(rng.integers(0, F + 1) if kind == "padded" else 0):] = -1
            arms[a, b] = ids
    return arms


@pytest.mark.parametrize("kind", ["overlap", "padded", "disjoint", "identical"])
@pytest.mark.parametrize("F", [1, 10, 64])
@pytest.mark.parametrize("A", [1, 2, 4])
def test_fuse_rrf_matches_the_definition(gpu_device, A, F, kind):
    import torch
    from rag_fin_amd.index import fuse_rrf
    B = 5
    arms = _arms(A, F, B, kind, 100 * A + F)
    if kind == "padded":
        arms[0, 0] = -1                                                  # one arm empty for one query
        if A > 1:
            arms[:, 1] = -1                                              # ... and one query without a candidate
    for k, rrf_k, weights in ((1, 60.0, None), (10, 60.0, None), (64, 7.5, [0.5, 2.0, 1.0, 0.0][:A])):
        scores, ids, fused = (t.cpu().numpy() for t in fuse_rrf(torch.from_numpy(arms).to(gpu_device), k, weights, rrf_k))
        ws, wi, wf = lexical.rrf_reference(arms, k, rrf_k, weights)
        assert np.array_equal(ids, wi), (k, np.argwhere(ids != wi)[:4].tolist())
        assert fused.tobytes() == wf.tobytes() and scores.tobytes() == ws.tobytes()
    # premises of the two special shapes, on the unweighted definition
    _, wi, wf = lexical.rrf_reference(arms, 64)
    if kind == "identical":
        assert np.array_equal(wi[:, :F], arms[0]) and (wi[:, F:] == -1).all()      # A times the same list: its order
    if kind == "disjoint":
        assert (wi[:, :A * F] >= 0).all() and (wi[:, A * F:] == -1).all()          # every id once
        if A > 1:
            assert wf[0, 0] == wf[0, 1] and wi[0, 0] < wi[0, 1]                  # rank 1 of two arms: a tie, by id


# ---- hybrid_search end to end ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store(gpu_device):
    return make_store(gpu_device)


def check_hybrid(hits, want):
    assert len(hits) == len(want)
    for b, (got, w) in enumerate(zip(hits, want)):
        assert [h.row for h in got] == [d for d, _ in w], f"query {b}"
        assert [h.score for h in got] == [f for _, f in w], f"query {b}: fused scores differ"


def test_hybrid_search_equals_the_composed_definitions(store, gpu_device):
    import torch
    from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
    texts, periods, c16, q16, qtexts = data()
    q = torch.from_numpy(np.array(q16)).to(gpu_device)
    dense = dense_oracle(q16, c16, 64)
    sparse = bm25_restated(texts, qtexts, 64)
    assert sparse[5] == [] and all(len(s) > 0 for i, s in enumerate(sparse) if i != 5)
    # BM25 alone, through the store
    got = store.search(qtexts, "sparse", BM25, limit=64)
    assert [[h.row for h in r] for r in got] == sparse
    for fk, limit, rrf_k, weights in ((64, 10, 60.0, None), (20, 20, 60.0, None), (33, 7, 12.0, [0.3, 1.7])):
        reqs = [AnnSearchRequest(q, "embedding", COS, limit=fk), AnnSearchRequest(qtexts, "sparse", BM25, limit=fk)]
        hits = store.hybrid_search(reqs, RRFRanker(k=rrf_k, weights=weights), limit=limit, output_fields=["text"])
        want = [rrf_restated([dense[b][:fk], sparse[b][:fk]], limit, rrf_k, weights) for b in range(NQ)]
        check_hybrid(hits, want)
        assert all(h.entity.text == texts[h.row] and h.id == f"k{h.row}" for r in hits for h in r)
    # the lexical arm changes the answer: some query's fused list is not its dense list
    want = [rrf_restated([dense[b], sparse[b]], 10) for b in range(NQ)]
    assert any([d for d, _ in w] != dense[b][:10] for b, w in enumerate(want))
    assert [d for d, _ in want[5]] == dense[5][:10]                     # no known term: the dense order
    # arms with different limits, and the sparse arm first
    reqs = [AnnSearchRequest(qtexts, "sparse", BM25, limit=5), AnnSearchRequest(q, "embedding", COS, limit=40)]
    check_hybrid(store.hybrid_search(reqs, RRFRanker(), limit=12),
                 [rrf_restated([sparse[b][:5], dense[b][:40]], 12) for b in range(NQ)])


def test_hybrid_search_with_expr_on_one_arm_only(store, gpu_device):
    import torch
    from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
    texts, periods, c16, q16, qtexts = data()
    q = torch.from_numpy(np.array(q16)).to(gpu_device)
    mask = np.array([p == "Q1_FY2024" for p in periods])
    expr = 'period == "Q1_FY2024"'
    dense, sparse = dense_oracle(q16, c16, 30), bm25_restated(texts, qtexts, 30)
    dense_f, sparse_f = dense_oracle(q16, c16, 30, mask), bm25_restated(texts, qtexts, 30, mask)
    assert dense_f != dense and sparse_f != sparse
    for e_dense, e_sparse, lists in ((None, expr, (dense, sparse_f)), (expr, None, (dense_f, sparse)),
                                     (expr, expr, (dense_f, sparse_f))):
        reqs = [AnnSearchRequest(q, "embedding", COS, limit=30, expr=e_dense),
                AnnSearchRequest(qtexts, "sparse", BM25, limit=30, expr=e_sparse)]
        hits = store.hybrid_search(reqs, RRFRanker(), limit=15)
        check_hybrid(hits, [rrf_restated([lists[0][b], lists[1][b]], 15) for b in range(NQ)])
    got = store.search(qtexts, "sparse", BM25, limit=30, expr=expr)
    assert [[h.row for h in r] for r in got] == sparse_f
    assert all(periods[h.row] == "Q1_FY2024" for r in got for h in r)


def test_the_sparse_index_is_rebuilt_after_a_delete(gpu_device):
    import torch
    from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
    texts, periods, c16, q16, qtexts = data()
    q = torch.from_numpy(np.array(q16)).to(gpu_device)
    st = make_store(gpu_device)
    before = st.search(qtexts, "sparse", BM25, limit=20)
    built = st._lexical.built[1]
    assert st.delete('period == "Q2_FY2023"').delete_count == periods.count("Q2_FY2023") > 0
    assert st._lexical.built is None
    keep = [i for i in range(N) if periods[i] != "Q2_FY2023"]
    fresh = make_store(gpu_device, keep)

    def reqs():
        return [AnnSearchRequest(q, "embedding", COS, limit=20), AnnSearchRequest(qtexts, "sparse", BM25, limit=20)]

    for a, b in ((st.search(qtexts, "sparse", BM25, limit=20), fresh.search(qtexts, "sparse", BM25, limit=20)),
                 (st.hybrid_search(reqs(), RRFRanker(), limit=10), fresh.hybrid_search(reqs(), RRFRanker(), limit=10))):
        assert [[(h.id, h.row, h.score) for h in r] for r in a] == [[(h.id, h.row, h.score) for h in r] for r in b]
    assert st._lexical.built[1] is not built and st._lexical.built[1].n_rows == len(keep)
    after = st.search(qtexts, "sparse", BM25, limit=20)
    want = bm25_restated([texts[i] for i in keep], qtexts, 20)
    assert [[h.row for h in r] for r in after] == want
    assert [[h.id for h in r] for r in after] != [[h.id for h in r] for r in before]   # df, avgdl and the rows changed
    assert all(periods[int(h.id[1:])] != "Q2_FY2023" for r in after for h in r)


# ---- VectorRAG ----------------------------------------------------------------------------------------
def test_vector_rag_hybrid_end_to_end(gpu_device):
    """Text -> embedder -> both arms at fetch_k -> RRF: the contexts are the fusion of the plain dense
    answer and the store's BM25 answer, `score` the fused score."""
    from rag_fin_amd.embedder import Embedder
    from rag_fin_amd.rag import VectorRAG
    from rag_fin_amd.service import ingest
    from rag_fin_amd.store import CorpusStore
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(200)] + list("abcdefghij")
    tok = WordPieceTokenizer(vocab)
    cfg = dict(oenc.MINILM_L6, layers=2, vocab_size=len(vocab), max_position=64)
    emb = Embedder(oenc.random_weights(cfg, 2), cfg, tokenizer=tok, device=gpu_device)
    rng = np.random.default_rng(1)
    texts = [" ".join(f"w{rng.integers(0, 200)}" for _ in range(rng.integers(1, 40))) for _ in range(37)]
    chunks = [dict(id=f"c{i}", text=t, period=f"Q{i % 2 + 1}_FY2024", chunk_type="t", statement_type="s",
                   primary_value=float(i)) for i, t in enumerate(texts)]
    store = CorpusStore("t", dim=384, capacity=64, device=gpu_device)
    assert ingest(store, emb, chunks) == 37
    rag = VectorRAG("k", "t", embedder=emb, store=store)
    query = "w3 w77 w150 w9 w21"
    with pytest.raises(ValueError, match="no sparse index"):
        rag.search(query, 3, hybrid=True)
    store.create_index("sparse", SPARSE)
    dense = [h.row for h in store.search(rag._embed([query]), "embedding", COS, limit=20)[0]]
    assert [texts[r] for r in dense] == [c["text"] for c in rag.search(query, 20)]
    sparse = [h.row for h in store.search([query], "sparse", BM25, limit=20)[0]]
    assert sparse == bm25_restated(texts, [query], 20)[0] and 0 < len(sparse) < 20
    want = rrf_restated([dense, sparse], 5)
    assert [r for r, _ in want] != dense[:5]
    got = rag.search(query, top_k=5, hybrid=True)                      # fetch_k defaults to 20
    assert [(c["rank"], c["text"], c["score"]) for c in got] == [(j + 1, texts[r], f) for j, (r, f) in enumerate(want)]
    assert rag.search_batch([query, "w5 w6"], top_k=5, hybrid=True)[0] == got
    only = rag.search(query, top_k=5, hybrid=True, expr='period == "Q1_FY2024"')
    assert only and all(c["period"] == "Q1_FY2024" for c in only)
