"""Diversified search (rf_mmr_select, GpuIndex.search(mmr=...), CorpusStore.search(mmr_lambda=...))
against a numpy oracle of the definition, which lives here because oracle/ holds none:
exact_scores -> topk_from_scores(fetch_k) -> exact_scores(rows, rows) for the similarities -> the
selection loop in float64, one operation per statement.  Bar: ids, order and fp64 scores
bit-identical, fp32 scores == float32(oracle).

Data: clustered unit rows (centres from default_rng(seed), rows = centre + 0.15 noise, queries =
centre + 0.6 noise, normalised, fp16), so that the best fetch_k hits hold near-copies and the MMR
list differs from the plain one: every parity case with lambda < 1 and k > 1 asserts that for at
least half of its queries.

The ladder case builds its own flagged queries: 60 clustered rows and ~20 000 copies of one filler
row, so the 64th candidate ties with thousands of rows and the rescoring set overflows (the recipe
of test_search_gpu.py's all-rows-identical case, with distinct best hits on top)."""
import functools

import numpy as np
import pytest

from oracle import search as osearch

pytestmark = pytest.mark.gpu

P = {"metric_type": "COSINE"}


# ---- data and oracle ------------------------------------------------------------------------------
def _unit16(x):
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x.astype(np.float16))


@functools.lru_cache(maxsize=None)
def clustered(n, dim, n_queries, seed=11):
    """(corpus fp16 [n, dim], queries fp16 [n_queries, dim]); read-only, shared between tests."""
    rng = np.random.default_rng(seed)
    n_centres = max(2, n // 50)
    centres = rng.standard_normal((n_centres, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    noise = rng.standard_normal((n, dim)) / np.sqrt(dim)
    c = _unit16(centres[rng.integers(0, n_centres, n)] + 0.15 * noise)
    qn = rng.standard_normal((n_queries, dim)) / np.sqrt(dim)
    q = _unit16(centres[rng.integers(0, n_centres, n_queries)] + 0.6 * qn)
    c.setflags(write=False)
    q.setflags(write=False)
    return c, q


@functools.lru_cache(maxsize=None)
def scores_of(n, dim, n_queries, seed=11):
    c, q = clustered(n, dim, n_queries, seed)
    s = osearch.exact_scores(q, c)
    s.setflags(write=False)
    return s


def mmr_select_oracle(s, g, k, lam):
    """The loop of the definition over F candidates: s fp64 [F] in candidate order, g fp64 [F, F]
    -> the picked candidate indices, in MMR order."""
    F = s.shape[0]
    lam = np.float64(lam)
    mu = np.float64(1.0) - lam
    m = np.full(F, -np.inf, dtype=np.float64)
    selected = np.zeros(F, dtype=bool)
    picks = []
    for t in range(min(k, F)):
        rel = lam * s
        if t == 0:
            pen = np.zeros(F, dtype=np.float64)
        else:
            pen = mu * m
        v = rel - pen
        best = -1
        for i in range(F):
            if not selected[i] and (best < 0 or v[i] > v[best]):
                best = i
        picks.append(best)
        selected[best] = True
        m = np.maximum(m, g[:, best])
    return picks


def mmr_oracle(scores, c16, fetch_k, k, lam, id_base=0):
    """scores: fp64 [B, N] contract scores with -inf where a row is not eligible (filter, band)
    -> (relevance fp64 [B, k], ids i64 [B, k]) in MMR order, -inf / -1 padded."""
    B = scores.shape[0]
    cs, ci = osearch.topk_from_scores(scores, fetch_k)
    out_s = np.full((B, k), -np.inf, dtype=np.float64)
    out_i = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        real = (ci[b] >= 0) & np.isfinite(cs[b])
        rows, s = ci[b][real], cs[b][real]
        g = osearch.exact_scores(c16[rows], c16[rows]) if rows.size else np.zeros((0, 0))
        assert np.array_equal(g, g.T)
        picks = mmr_select_oracle(s, g, k, lam)
        out_s[b, :len(picks)] = s[picks]
        out_i[b, :len(picks)] = rows[picks] + id_base
    return out_s, out_i


def make_index(c16, device):
    import torch
    from rag_fin_amd.store import GpuIndex
    ix = GpuIndex(c16.shape[1], c16.shape[0], device)
    ix.add(torch.from_numpy(np.array(c16)).to(device))
    return ix


def assert_equal(got, want, what=""):
    scores, ids, exact = (t.cpu().numpy() for t in got)
    ws, wi = want
    assert np.array_equal(ids, wi), f"{what}: ids differ at {np.argwhere(ids != wi)[:5].tolist()}"
    assert np.array_equal(exact, ws), f"{what}: fp64 scores differ"
    assert np.array_equal(scores, ws.astype(np.float32)), f"{what}: fp32 scores differ"


def n_differing(wi, scores, k):
    plain = osearch.topk_from_scores(scores, k)[1]
    return int((wi != plain).any(axis=1).sum())


# ---- parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n,B,fetch_k,k,lam,id_base", [
    (64, 2000, 3, 64, 10, 0.5, 0),          # KS = 4
    (384, 2000, 65, 64, 10, 0.3, 1000),     # the product's dim; B beyond one 64-query sweep
    (1024, 2000, 3, 64, 64, 0.5, 0),        # the LDS budget; every candidate is picked
    (384, 20000, 3, 64, 10, 0.0, 0),        # above 8192 rows: candidates from the sampled path
    (1024, 20000, 1, 64, 10, 0.3, 1000),
    (64, 20000, 65, 64, 64, 0.0, 0),
    (384, 2000, 1, 17, 5, 0.3, 0),
    (384, 33, 3, 17, 5, 0.5, 1000),         # one row beyond a 32-row block
    (64, 33, 3, 64, 10, 0.3, 0),            # fewer rows than fetch_k
    (384, 2000, 3, 64, 10, 1.0, 0),         # lambda = 1: the plain top-k
    (384, 33, 3, 1, 1, 0.5, 0),
    (1024, 33, 1, 1, 1, 0.0, 1000),
])
def test_parity_with_oracle(gpu_device, dim, n, B, fetch_k, k, lam, id_base):
    import torch
    c, q = clustered(n, dim, B)
    sc = scores_of(n, dim, B)
    want = mmr_oracle(sc, c, fetch_k, k, lam, id_base)
    differ = n_differing(want[1] - np.where(want[1] >= 0, id_base, 0), sc, k)
    print(f"queries whose MMR list differs from the plain list: {differ} of {B}")
    if lam == 1.0:
        plain = osearch.topk_from_scores(sc, k, id_base)
        assert np.array_equal(want[1], plain[1]) and np.array_equal(want[0], plain[0])
    elif k > 1:
        assert 2 * differ >= B, "the case is vacuous: MMR picked the plain list"
    assert np.array_equal(want[1][:, 0], osearch.topk_from_scores(sc, 1, id_base)[1][:, 0])
    ix = make_index(c, gpu_device)
    qd = torch.from_numpy(np.array(q)).to(gpu_device)
    scores, ids, exact, flags = ix.search_raw(qd, k, id_base, want_exact=True, mmr=(fetch_k, lam))
    torch.cuda.synchronize()
    assert int(flags.abs().sum()) == 0
    assert_equal((scores, ids, exact), want, "search_raw")
    assert_equal(ix.search(qd, k, id_base, want_exact=True, mmr=(fetch_k, lam)), want, "search")
    if id_base == 0:
        hs, hi = ix.search_host(qd, k, mmr=(fetch_k, lam))
        assert np.array_equal(hi, want[1]) and np.array_equal(hs, want[0].astype(np.float32))


def test_fewer_candidates_than_fetch_k_pads_the_tail(gpu_device):
    """A corpus of 20 rows with fetch_k 64: k = 10 fills, k = 30 leaves slots 20.. at -inf / -1."""
    import torch
    c, q = clustered(2000, 64, 3)
    c = c[:20]
    sc = osearch.exact_scores(q, c)
    ix = make_index(c, gpu_device)
    qd = torch.from_numpy(np.array(q)).to(gpu_device)
    for k in (10, 30):
        want = mmr_oracle(sc, c, 64, k, 0.5)
        assert (want[1][:, :min(k, 20)] >= 0).all() and (want[1][:, 20:] == -1).all()
        assert_equal(ix.search(qd, k, want_exact=True, mmr=(64, 0.5)), want, f"k = {k}")


def test_rf_mmr_select_skips_bad_rows_and_writes_without_exact(gpu_device):
    """The C entry point on hand-made candidates: a padded tail, an id whose row is past the index
    and an id below id_base are absent (never gathered); exact_dev may be NULL."""
    import torch
    from rag_fin_amd import _lib
    from rag_fin_amd.index import _ptr
    c, _ = clustered(2000, 64, 3)
    c = c[:40]
    ix = make_index(c, gpu_device)
    base = 100
    rows = np.array([7, 3, 4000, 12, -101, 30, 1, 39], dtype=np.int64)       # 4000: past the index; -101 -> id -1
    s = np.array([0.9, 0.8, 0.75, 0.7, 0.6, 0.5, 0.4, 0.3], dtype=np.float64)
    cand_ids = np.full((1, 12), -1, dtype=np.int64)
    cand_ids[0, :8] = rows + base
    cand_ids[0, 8] = base - 1                                                # a row of -1
    cand_s = np.full((1, 12), -np.inf)
    cand_s[0, :8] = s
    cand_s[0, 8] = 0.2
    ok = np.array([0, 1, 3, 5, 6, 7])
    g = osearch.exact_scores(c[rows[ok]], c[rows[ok]])
    picks = mmr_select_oracle(s[ok], g, 8, 0.5)
    want_i = np.full(8, -1, dtype=np.int64)
    want_i[:6] = rows[ok][picks] + base
    want_s = np.full(8, -np.inf)
    want_s[:6] = s[ok][picks]
    ci = torch.from_numpy(cand_ids).to(gpu_device)
    cs = torch.from_numpy(cand_s).to(gpu_device)
    scores = torch.zeros((1, 8), dtype=torch.float32, device=gpu_device)
    ids = torch.zeros((1, 8), dtype=torch.int64, device=gpu_device)
    _lib.check(ix.lib.rf_mmr_select(ix.handle, 1, 12, 8, 0.5, base, _ptr(cs), _ptr(ci), _ptr(scores), _ptr(ids), None,
                                    _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(ids.cpu().numpy()[0], want_i)
    assert np.array_equal(scores.cpu().numpy()[0], want_s.astype(np.float32))


def test_exact_duplicates_tie_break_by_row(gpu_device):
    """One vector stored four times among others: the copies tie in score and in similarity, the
    lower row wins, and once one copy is picked the others carry the full penalty (g = |c|^2)."""
    import torch
    c, q = clustered(2000, 384, 3)
    c = np.array(c)
    best = osearch.topk_from_scores(scores_of(2000, 384, 3), 1)[1][:, 0]
    dup = c[best[0]].copy()
    copies = [5, 700, 1311, 1999]
    copies = [r for r in copies if r != best[0]][:3]
    c[copies] = dup                                  # with the original: four copies
    sc = osearch.exact_scores(q, c)
    want = mmr_oracle(sc, c, 64, 10, 0.5)
    group = sorted(copies + [int(best[0])])
    assert want[1][0, 0] == group[0]                 # the first pick: the lowest row of the tie
    where = [int(np.flatnonzero(want[1][0] == r)[0]) if (want[1][0] == r).any() else None for r in group]
    assert where[0] == 0 and all(w is None or w > 1 for w in where[1:])   # no second copy right behind it
    ix = make_index(c, gpu_device)
    qd = torch.from_numpy(np.array(q)).to(gpu_device)
    assert_equal(ix.search(qd, 10, want_exact=True, mmr=(64, 0.5)), want)


# ---- composition, through the store ---------------------------------------------------------------------
def make_store(c16, device, kinds=("a", "b", "c")):
    import torch
    from rag_fin_amd.store import CorpusStore
    n, dim = c16.shape
    st = CorpusStore("c", dim=dim, capacity=n, device=device)
    st.add(list(range(n)), [f"t{i}" for i in range(n)], torch.from_numpy(np.array(c16)).to(device),
           [f"Q{i % 4}" for i in range(n)], [kinds[i % len(kinds)] for i in range(n)], ["s"] * n,
           [float(i) for i in range(n)])
    return st


def hits_of(res, k):
    ids = np.full((len(res), k), -1, dtype=np.int64)
    sc = np.full((len(res), k), -np.inf, dtype=np.float32)
    for b, hits in enumerate(res):
        ids[b, :len(hits)] = [h.id for h in hits]
        sc[b, :len(hits)] = [h.score for h in hits]
    return sc, ids


def test_store_surface_and_composition_with_expr_and_band(gpu_device):
    import torch
    n, dim, B = 2000, 64, 3
    c, q = clustered(n, dim, B)
    sc = scores_of(n, dim, B)
    st = make_store(c, gpu_device)
    qd = torch.from_numpy(np.array(q)).to(gpu_device)
    # plain: CorpusStore.search(mmr_lambda=0.5), the default fetch_k = max(20, 4 * 10) = 40
    want = mmr_oracle(sc, c, 40, 10, 0.5)
    got = hits_of(st.search(qd, "embedding", P, limit=10, mmr_lambda=0.5), 10)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0].astype(np.float32))
    assert n_differing(want[1], sc, 10) * 2 >= B
    # expr: candidates among the passing rows
    allowed = np.arange(n) % 3 == 0
    sc_f = np.where(allowed[None, :], sc, -np.inf)
    want = mmr_oracle(sc_f, c, 64, 10, 0.3)
    got = hits_of(st.search(qd, "embedding", P, limit=10, expr='chunk_type == "a"', mmr_lambda=0.3, mmr_fetch_k=64), 10)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0].astype(np.float32))
    assert allowed[want[1]].all()
    # a filter passing 5 rows: F = 5 < k, the tail is padded (index level: the store drops the padding)
    sc_5 = np.where((np.arange(n) < 5)[None, :], sc, -np.inf)
    want = mmr_oracle(sc_5, c, 64, 10, 0.5)
    assert (want[1][:, :5] >= 0).all() and (want[1][:, 5:] == -1).all()
    filt = st.build_filter("primary_value < 5")
    assert_equal(st.index.search(qd, 10, want_exact=True, filt=filt, mmr=(64, 0.5)), want, "5 passing rows")
    got = st.search(qd, "embedding", P, limit=10, expr="primary_value < 5", mmr_lambda=0.5, mmr_fetch_k=64)
    assert [[h.id for h in hits] for hits in got] == [want[1][b, :5].tolist() for b in range(B)]
    # a band: candidates with radius < score <= range_filter (at least the 7 best hits of every query are cut off)
    hi = float(np.sort(sc, axis=1)[:, -8].min())
    lo = 0.0
    sc_b = np.where((sc > lo) & (sc <= hi), sc, -np.inf)
    want = mmr_oracle(sc_b, c, 64, 10, 0.5)
    param = {"metric_type": "COSINE", "params": {"radius": lo, "range_filter": hi}}
    got = hits_of(st.search(qd, "embedding", param, limit=10, mmr_lambda=0.5, mmr_fetch_k=64), 10)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0].astype(np.float32))
    assert (want[1] >= 0).all() and (want[0] <= hi).all() and (want[0] > lo).all()


def test_sq8_collection(gpu_device):
    """An SQ8 collection above 8192 rows: the candidates come from the int8 sweep, the similarities
    from the fp16 rows."""
    import torch
    n, dim, B = 20000, 64, 65
    c, q = clustered(n, dim, B)
    sc = scores_of(n, dim, B)
    st = make_store(c, gpu_device)
    st.create_index("embedding", {"index_type": "SQ8", "metric_type": "COSINE"})
    want = mmr_oracle(sc[:64], c, 64, 10, 0.5)
    qd = torch.from_numpy(np.array(q[:64])).to(gpu_device)
    assert st._use_sq8(64, 10)
    got = hits_of(st.search(qd, "embedding", P, limit=10, mmr_lambda=0.5, mmr_fetch_k=64), 10)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0].astype(np.float32))
    assert_equal(st.index.search(qd, 10, want_exact=True, sq8=True, mmr=(64, 0.5)), want, "index, sq8")


def test_vector_rag_search(gpu_device):
    from rag_fin_amd.rag import VectorRAG
    n, dim = 2000, 64
    c, q = clustered(n, dim, 3)
    st = make_store(c, gpu_device)

    class Emb:
        def encode(self, texts):
            return np.array(q[:len(texts)]).astype(np.float32)

    # (the store normalises what an embedder returns as fp32: the oracle takes the same fp16 queries)
    q16 = st.index.to_fp16(Emb().encode(["x"]), normalize=True).cpu().numpy()
    sc = osearch.exact_scores(q16, c)
    want = mmr_oracle(sc, c, 40, 10, 0.5)
    got = VectorRAG("k", embedder=Emb(), store=st).search("net interest income trend", 10, mmr_lambda=0.5)
    assert [x["text"] for x in got] == [f"t{i}" for i in want[1][0]]
    assert [x["score"] for x in got] == [float(np.float32(s)) for s in want[0][0]]
    assert [x["rank"] for x in got] == list(range(1, 11))
    want = mmr_oracle(sc, c, 17, 5, 0.3)
    got = VectorRAG("k", embedder=Emb(), store=st).search("net interest income trend", 5, mmr_lambda=0.3, fetch_k=17)
    assert [x["text"] for x in got] == [f"t{i}" for i in want[1][0]]


# ---- the ladder ---------------------------------------------------------------------------------------------
def test_flagged_queries_are_selected_again_from_the_ladders_candidates(gpu_device):
    import torch
    dim, n = 384, 20000
    rng = np.random.default_rng(5)
    u = rng.standard_normal(dim)
    u /= np.linalg.norm(u)
    centres = u[None, :] + 0.5 * rng.standard_normal((4, dim)) / np.sqrt(dim)
    near = _unit16(np.repeat(centres, 15, axis=0) + 0.1 * rng.standard_normal((60, dim)) / np.sqrt(dim))
    filler = _unit16((u + 1.0 * rng.standard_normal(dim) / np.sqrt(dim))[None, :])
    c = np.repeat(filler, n, axis=0)
    at = np.sort(rng.choice(n, 60, replace=False))
    c[at] = near
    q = _unit16(u[None, :] + 0.2 * rng.standard_normal((3, dim)) / np.sqrt(dim))
    sc = osearch.exact_scores(q, c)
    want = mmr_oracle(sc, c, 64, 10, 0.5)
    assert n_differing(want[1], sc, 10) * 2 >= 3
    assert np.isin(osearch.topk_from_scores(sc, 64)[1][:, :60], at).all()     # the near rows lead, 4 filler rows follow
    ix = make_index(c, gpu_device)
    qd = torch.from_numpy(q).to(gpu_device)
    _, _, _, flags = ix.search_raw(qd, 10, mmr=(64, 0.5))
    assert (flags.cpu().numpy() != 0).all()
    assert_equal(ix.search(qd, 10, want_exact=True, mmr=(64, 0.5)), want, "search")
    hs, hi = ix.search_host(qd, 10, mmr=(64, 0.5))
    assert np.array_equal(hi, want[1]) and np.array_equal(hs, want[0].astype(np.float32))
