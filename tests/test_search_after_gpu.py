"""Paged search on the GPU: rf_search_after (the search-after sweep), GpuIndex.search_after /
search_large above it, and CorpusStore.search(offset=) / search_iterator above those.

Bar, as in tests/test_search_gpu.py: ids and ranks equal to the oracle's on the whole window, fp64
scores bit-equal, fp32 scores == float32(oracle); no tolerance anywhere.  The truth of a page is a
slice of c_oracle.search at a larger k; with a filter or a band it is osearch.topk_from_scores over
the oracle's score matrix with every ineligible entry removed (as tests/test_range_search_gpu.py).

Corpora: 3 000 rows (the small-corpus path: no sample pass) and 20 011 rows (sample pass, ragged
last block) at dim 384, and 20 011 rows at dims 64, 768 and 1 024 (one kernel instantiation per dim).
Each corpus, its queries and its oracle ranking are computed once and shared, read-only."""
import functools

import numpy as np
import pytest

from oracle import c_oracle, search as osearch

pytestmark = pytest.mark.gpu

SMALL, LARGE = 3_000, 20_011
INF = float("inf")
KTOT = 1_024          # depth of the shared oracle rankings
NOWHERE = 2 ** 62     # the id of the bound nothing can follow


@functools.lru_cache(maxsize=8)
def ranked(n, dim, B=70, cseed=1234, qseed=5678):
    """(corpus, queries, oracle scores f64 [B, KTOT], oracle ids [B, KTOT]); read-only."""
    c16 = osearch.synth_unit_rows(n, dim, cseed)
    q16 = osearch.synth_unit_rows(B, dim, qseed)
    os_, oi = c_oracle.search(q16, c16, KTOT)
    for a in (c16, q16, os_, oi):
        a.setflags(write=False)
    return c16, q16, os_, oi


@functools.lru_cache(maxsize=2)
def scored(n, dim, B):
    """(corpus, queries, oracle score matrix f64 [B, n]) of the first B queries of ranked(n, dim)."""
    c16, q16, _, _ = ranked(n, dim)
    S = osearch.exact_scores(np.array(q16[:B]), np.array(c16))
    S.setflags(write=False)
    return c16, q16[:B], S


def make_index(c16, device):
    import torch
    from rag_fin_amd.store import GpuIndex
    ix = GpuIndex(c16.shape[1], c16.shape[0], device)
    ix.add(torch.from_numpy(np.array(c16)).to(device))
    return ix


def dev(a, device, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.array(a), dtype=dtype)).to(device)


def bound_at(os_, oi, ranks):
    """The bound of each query b: its hit of rank ranks[b] (1-based; 0 = the +inf bound before the first hit)."""
    ranks = np.asarray(ranks)
    b = np.arange(len(ranks))
    bs = np.where(ranks > 0, os_[b, np.maximum(ranks, 1) - 1], INF)
    bi = np.where(ranks > 0, oi[b, np.maximum(ranks, 1) - 1], -1)
    return bs.astype(np.float64), bi.astype(np.int64)


def slice_after(os_, oi, ranks, k):
    """The oracle's page of k hits after rank ranks[b] of each query, padded where the ranking ends."""
    B = len(ranks)
    es = np.full((B, k), -np.inf)
    ei = np.full((B, k), -1, dtype=np.int64)
    for b, r in enumerate(ranks):
        m = max(0, min(k, os_.shape[1] - r))
        es[b, :m], ei[b, :m] = os_[b, r:r + m], oi[b, r:r + m]
    ei[es == -np.inf] = -1
    return es, ei


def eligible_truth(S, k, bs, bi, mask=None, band=None, id_base=0):
    """topk_from_scores with the ineligible entries removed: filter, band, and the (score, id) bound."""
    ids = np.arange(S.shape[1], dtype=np.int64)[None, :] + id_base
    keep = (S < bs[:, None]) | ((S == bs[:, None]) & (ids > bi[:, None]))
    if mask is not None:
        keep &= mask[None, :]
    if band is not None:
        keep &= (S > band[0]) & (S <= band[1])
    es, ei = osearch.topk_from_scores(np.where(keep, S, -np.inf), k, id_base)
    ei[es == -np.inf] = -1
    return es, ei


def raw_page(ix, q, bs, bi, k, device, flags_zero=True, **kw):
    """One rf_search_after call alone -> (scores, ids, exact, flags) as numpy."""
    import torch
    out = ix.search_after_raw(q, k, (dev(bs, device, np.float64), dev(bi, device, np.int64)), want_exact=True, **kw)
    torch.cuda.synchronize()
    scores, ids, exact, flags = (t.cpu().numpy() for t in out)
    if flags_zero:
        assert not flags.any(), f"flags set: {np.flatnonzero(flags)[:8]} = {flags[flags != 0][:8]}"
    return scores, ids, exact, flags


def assert_page(got, es, ei, what=""):
    scores, ids, exact = got[:3]
    assert np.array_equal(ids, ei), f"{what}: ids differ at {np.argwhere(ids != ei)[:5].tolist()}"
    assert np.array_equal(exact, es), f"{what}: fp64 scores differ"
    assert np.array_equal(scores, es.astype(np.float32)), f"{what}: fp32 scores differ"


# ---- 1. the walk ------------------------------------------------------------------------------------
WALKS = [(SMALL, 384, 3), (SMALL, 384, 64), (LARGE, 384, 3), (LARGE, 384, 64),
         (LARGE, 64, 33), (LARGE, 768, 33), (LARGE, 1024, 33)]


@pytest.mark.parametrize("n,dim,B", WALKS)
def test_walk_from_the_top(gpu_device, n, dim, B):
    """From a +inf bound, 5 pages of 64 then 5 of 10, each bound taken from the page before on the
    device; the raw entry point alone, flags 0; page 1 is rf_search."""
    import torch
    c16, q16, os_, oi = ranked(n, dim)
    os_, oi = os_[:B], oi[:B]
    ix = make_index(c16, gpu_device)
    q = dev(q16[:B], gpu_device)
    bs = torch.full((B,), INF, dtype=torch.float64, device=gpu_device)
    bi = torch.full((B,), -1, dtype=torch.int64, device=gpu_device)
    at = 0
    for page, k in enumerate([64] * 5 + [10] * 5):
        scores, ids, exact, flags = ix.search_after_raw(q, k, (bs, bi), want_exact=True)
        torch.cuda.synchronize()
        assert int(flags.abs().sum()) == 0, f"page {page}: flags {flags.cpu().numpy()}"
        assert_page([t.cpu().numpy() for t in (scores, ids, exact)], os_[:, at:at + k], oi[:, at:at + k], f"page {page}")
        if page == 0:
            first = ix.search_raw(q, k, want_exact=True)
            torch.cuda.synchronize()
            for a, b in zip(first, (scores, ids, exact, flags)):
                assert torch.equal(a, b)
        bs, bi = exact[:, -1].contiguous(), ids[:, -1].contiguous()
        at += k


# ---- 2. ties on the bound ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_bound_on_each_of_eleven_equal_rows(gpu_device, n):
    """Row 5 copied to rows 60..69 and asked for by itself: the bound on each of the 11 equal rows
    in turn (one query of the batch each); the page starts at the next copy by row order."""
    c16 = np.array(ranked(n, 384)[0])
    c16[60:70] = c16[5]
    q16 = np.repeat(c16[5:6], 11, axis=0)
    os_, oi = c_oracle.search(q16, c16, 11 + 20)
    assert oi[0, :11].tolist() == [5] + list(range(60, 70)) and np.unique(os_[0, :11]).size == 1
    ranks = np.arange(1, 12)
    bs, bi = bound_at(os_, oi, ranks)
    got = raw_page(make_index(c16, gpu_device), dev(q16, gpu_device), bs, bi, 20, gpu_device)
    assert_page(got, *slice_after(os_, oi, ranks, 20))
    assert got[1][0, :3].tolist() == [60, 61, 62] and got[1][9, 0] == 69 and got[1][10, 0] not in range(60, 70)


# ---- 3. crowded ties --------------------------------------------------------------------------------
def test_three_hundred_rows_on_the_bound_flag_and_the_ladder_answers(gpu_device):
    """300 copies of one row at ranks 1..300 of query 0, the bound on the 150th: more rows tied at the
    bound than the rescoring set holds, so the raw call flags the query (and never answers wrongly);
    search_after and search_large give the oracle's pages through the ladder."""
    from rag_fin_amd import _lib
    n, k = LARGE, 10
    c16 = np.array(ranked(n, 384)[0])
    copies = np.sort(np.random.default_rng(7).choice(n, 300, replace=False))
    c16[copies] = c16[copies[0]]
    q16 = np.concatenate([c16[copies[:1]], np.array(ranked(n, 384)[1][:2])])
    os_, oi = c_oracle.search(q16, c16, 400)
    assert np.array_equal(oi[0, :300], copies)
    ranks = np.array([150, 10, 0])
    bs, bi = bound_at(os_, oi, ranks)
    es, ei = slice_after(os_, oi, ranks, k)
    assert np.array_equal(ei[0], copies[150:160])
    ix = make_index(c16, gpu_device)
    q = dev(q16, gpu_device)
    scores, ids, exact, flags = raw_page(ix, q, bs, bi, k, gpu_device, flags_zero=False)
    assert flags[0] & _lib.RF_FLAG_TIE_OVERFLOW and not flags[1:].any(), flags
    assert_page((scores[1:], ids[1:], exact[1:]), es[1:], ei[1:], "unflagged queries")
    got = ix.search_after(q, k, (dev(bs, gpu_device), dev(bi, gpu_device)), want_exact=True)
    assert_page([t.cpu().numpy() for t in got], es, ei, "search_after")
    # search_large walks through the tie block: its pages 2..5 are flagged for query 0 and walked again
    # through the ladder, the others' pages stay the sweep's
    got = ix.search_large(q, 400, want_exact=True)
    assert_page([t.cpu().numpy() for t in got], os_, oi, "search_large")


# ---- 4. near-tie clusters ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
@pytest.mark.parametrize("rank", [3, 48, 96])
def test_bound_on_a_cluster_row(gpu_device, n, rank):
    """Ranks 1..97 of every query are its near-tie cluster (scores a fraction of a float32 spacing
    apart): which of them lie after the bound only the fp64 (score, id) rule can tell."""
    from test_near_ties_gpu import case
    c16, q16, pos, _, _ = case(n, 384, 3, 97)
    c16, q16 = np.array(c16), np.array(q16)
    os_, oi = c_oracle.search(q16, c16, 96 + 64)
    assert all(np.isin(oi[b, :97], pos[b]).all() for b in range(3))
    ranks = np.full(3, rank)
    bs, bi = bound_at(os_, oi, ranks)
    got = raw_page(make_index(c16, gpu_device), dev(q16, gpu_device), bs, bi, 64, gpu_device)
    assert_page(got, *slice_after(os_, oi, ranks, 64))


# ---- 5. chunked bounds ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_seventy_queries_each_at_its_own_depth(gpu_device, n):
    """B = 70 = a sweep of 64 and one of 6: queries 64..69 use their own bounds."""
    c16, q16, os_, oi = ranked(n, 384)
    depth = (10, 64, 500)
    ranks = np.array([0 if b % 3 == 0 else depth[(b // 3) % 3] for b in range(70)])
    assert len(set(ranks[64:].tolist())) > 1 and ranks[64:].tolist() != ranks[:6].tolist()
    bs, bi = bound_at(os_, oi, ranks)
    got = raw_page(make_index(c16, gpu_device), dev(q16, gpu_device), bs, bi, 10, gpu_device)
    assert_page(got, *slice_after(os_, oi, ranks, 10))


# ---- 6. id base --------------------------------------------------------------------------------------
def test_id_base_rides_on_bounds_and_outputs(gpu_device):
    base = 1_000_000
    c16, q16, os_, oi = ranked(LARGE, 384)
    ranks = np.array([64, 7, 0])
    bs, bi = bound_at(os_[:3], oi[:3], ranks)
    bi = np.where(ranks > 0, bi + base, bi)
    es, ei = slice_after(os_[:3], oi[:3], ranks, 64)
    got = raw_page(make_index(c16, gpu_device), dev(q16[:3], gpu_device), bs, bi, 64, gpu_device, id_base=base)
    assert_page(got, es, ei + base)


# ---- 7. filter and band -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
@pytest.mark.parametrize("use_filter,use_band", [(True, False), (False, True), (True, True)])
def test_filter_and_band(gpu_device, n, use_filter, use_band):
    """A filter passing about half the rows, a band between query 0's scores of ranks 200 and 900.
    The bound inside the eligible rows (rank 50 of them), above them (then rf_search_range /
    rf_search_filtered) and below the floor (empty, flags 0)."""
    import torch
    from test_filtered_search_gpu import filter_from_mask
    B, k = 3, 64
    c16, q16, S = scored(n, 384, B)
    _, _, os_, _ = ranked(n, 384)
    mask = np.random.default_rng(5).random(n) < 0.5 if use_filter else None
    band = (float(os_[0, 899]), float(os_[0, 199])) if use_band else None
    kw = {}
    if use_filter:
        kw["filt"] = filter_from_mask(mask, gpu_device)
    if use_band:
        kw["band"] = band
    ix = make_index(c16, gpu_device)
    q = dev(q16, gpu_device)
    top = np.full(B, INF), np.full(B, -1, dtype=np.int64)
    es0, ei0 = eligible_truth(S, 128, *top, mask=mask, band=band)
    assert (ei0[:, 127] >= 0).all()
    # above every eligible row: the first page, and the bits of the search without a bound
    first = raw_page(ix, q, *top, k, gpu_device, **kw)
    assert_page(first, es0[:, :k], ei0[:, :k], "bound above")
    plain = ix.search_raw(q, k, want_exact=True, **kw)
    torch.cuda.synchronize()
    for a, b in zip(plain, first):
        assert np.array_equal(a.cpu().numpy(), b)
    if use_band:   # a finite bound above the ceiling of the band
        bs, bi = np.full(B, band[1] + 0.01), np.zeros(B, dtype=np.int64)
        assert_page(raw_page(ix, q, bs, bi, k, gpu_device, **kw), es0[:, :k], ei0[:, :k], "bound above the band")
    # inside: after the 50th eligible row of each query
    bs, bi = es0[:, 49].copy(), ei0[:, 49].copy()
    es, ei = eligible_truth(S, k, bs, bi, mask=mask, band=band)
    assert np.array_equal(ei, ei0[:, 50:50 + k])
    assert_page(raw_page(ix, q, bs, bi, k, gpu_device, **kw), es, ei, "bound inside")
    # below: under the floor of the band, or under every score
    bs = np.full(B, band[0] - 0.01 if use_band else -INF)
    bi = np.zeros(B, dtype=np.int64)
    got = raw_page(ix, q, bs, bi, k, gpu_device, **kw)
    assert (got[1] == -1).all() and (got[2] == -np.inf).all() and (got[0] == -np.inf).all()


# ---- 8. ends ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_ends_of_the_ranking(gpu_device, n):
    B, k = 3, 10
    c16, q16, S = scored(n, 384, B)
    es_all, ei_all = osearch.topk_from_scores(np.array(S), n)
    ix = make_index(c16, gpu_device)
    q = dev(q16, gpu_device)
    # the bound nothing can follow: all padding, flags 0
    got = raw_page(ix, q, np.full(B, -INF), np.full(B, NOWHERE, dtype=np.int64), k, gpu_device)
    assert (got[1] == -1).all() and (got[0] == -np.inf).all() and (got[2] == -np.inf).all()
    # on the last-ranked row: an empty page; five rows before the end: five hits and padding
    for left in (0, 5):
        ranks = np.full(B, n - left)
        bs, bi = bound_at(es_all, ei_all, ranks)
        es, ei = slice_after(es_all, ei_all, ranks, k)
        assert ((ei >= 0).sum(axis=1) == left).all()
        assert_page(raw_page(ix, q, bs, bi, k, gpu_device), es, ei, f"{left} rows left")


# ---- 9. search_large pages through the sweep, not through the exhaustive kernel -----------------------
def test_search_large_never_calls_the_exhaustive_kernel(gpu_device):
    c16, q16, os_, oi = ranked(LARGE, 384)
    ix = make_index(c16, gpu_device)
    calls = []
    inner = ix._exhaustive

    def counting(*a, **kw):
        calls.append(kw.get("after") is not None)
        return inner(*a, **kw)

    ix._exhaustive = counting
    scores, ids, exact = ix.search_large(dev(q16[:3], gpu_device), 1000, want_exact=True)
    assert_page([t.cpu().numpy() for t in (scores, ids, exact)], os_[:3, :1000], oi[:3, :1000])
    assert calls == []


# ---- 10. the store -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _store_case():
    c16, q16, _, _ = ranked(LARGE, 384)
    return np.array(c16), np.array(q16[:2])


def make_store(device, index_type=None):
    import torch
    from rag_fin_amd.store import CorpusStore
    c16, _ = _store_case()
    n = c16.shape[0]
    st = CorpusStore("paged", dim=384, capacity=n, device=device, metric_type="IP")
    st.add(list(range(n)), [""] * n, torch.from_numpy(c16).to(device), ["Q1" if i % 3 else "Q2" for i in range(n)],
           ["t"] * n, ["s"] * n, [float(i % 7) - 3.0 for i in range(n)])
    if index_type:
        st.create_index("embedding", {"index_type": index_type, "metric_type": "IP"})
    return st


def hit_list(hits):
    return [(h.id, h.score) for h in hits]


@pytest.mark.parametrize("index_type", [None, "SQ8"])
def test_store_offset_equals_the_slice(gpu_device, index_type):
    st = make_store(gpu_device, index_type)
    _, q16 = _store_case()
    q = dev(q16, gpu_device)
    _, _, os_, oi = ranked(LARGE, 384)
    full = st.search(q, "embedding", {"metric_type": "IP"}, limit=1020)
    for b in range(2):   # the long list itself is the oracle's
        assert [h.id for h in full[b]] == oi[b, :1020].tolist()
        assert [h.score for h in full[b]] == os_[b, :1020].astype(np.float32).tolist()
    radius = float(os_[0, 700])
    for kw in ({}, {"expr": "primary_value > 0"}, {"expr": 'period == "Q1"', "param": {"params": {"radius": radius}}},
               {"param": {"params": {"radius": radius}}}):
        param = dict({"metric_type": "IP"}, **kw.get("param", {}))
        expr = kw.get("expr")
        for o, l in ((0, 5), (7, 10), (60, 10), (64, 64), (990, 30)):
            whole = st.search(q, "embedding", param, limit=o + l, expr=expr)
            part = st.search(q, "embedding", param, limit=l, expr=expr, offset=o)
            for b in range(2):
                assert hit_list(part[b]) == hit_list(whole[b][o:]), (kw, o, l, b)
        part = st.search(q, "embedding", dict(param, offset=7), limit=10, expr=expr)     # pymilvus' spelling
        assert [hit_list(p) for p in part] == [hit_list(w[7:17]) for w in st.search(q, "embedding", param, limit=17, expr=expr)]


@pytest.mark.parametrize("batch", [10, 100])
def test_iterator_pages_concatenate_to_the_search(gpu_device, batch):
    st = make_store(gpu_device)
    _, q16 = _store_case()
    q = dev(q16[:1], gpu_device)
    for expr in (None, "primary_value > 0"):
        want = st.search(q, "embedding", {"metric_type": "IP"}, limit=250, expr=expr)[0]
        it = st.search_iterator(q, "embedding", {"metric_type": "IP"}, batch_size=batch, limit=250, expr=expr)
        got, pages = [], 0
        while True:
            page = it.next()
            if not page:
                break
            assert len(page) == min(batch, 250 - len(got))
            got += page
            pages += 1
        assert pages == -(-250 // batch) and hit_list(got) == hit_list(want)
        assert it.next() == [] and it.next() == []
        it.close()


def test_iterator_runs_a_band_dry_and_refuses_after_a_delete(gpu_device):
    st = make_store(gpu_device)
    _, q16 = _store_case()
    q = dev(q16[:1], gpu_device)
    _, _, os_, _ = ranked(LARGE, 384)
    param = {"metric_type": "IP", "params": {"radius": float(os_[0, 150])}}      # 150 hits above the radius
    want = st.search(q, "embedding", param, limit=400)[0]
    assert len(want) == 150
    it = st.search_iterator(q, "embedding", param, batch_size=100)
    a, b, c = it.next(), it.next(), it.next()
    assert (len(a), len(b), c) == (100, 50, []) and hit_list(a + b) == hit_list(want)
    with pytest.raises(ValueError):
        st.search_iterator(dev(q16, gpu_device), "embedding", {"metric_type": "IP"})     # two vectors
    it = st.search_iterator(q, "embedding", {"metric_type": "IP"}, batch_size=10)
    assert len(it.next()) == 10
    st.delete("id in [17]")
    with pytest.raises(RuntimeError):
        it.next()
