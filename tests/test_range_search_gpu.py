"""Range search on the GPU: rf_search_range / rf_search_exhaustive_range and everything above them
against the CPU oracle.  The reference of every comparison: osearch.exact_scores for the full score
matrix, every entry outside the band (radius < score <= range_filter, compared as float64) set to
-inf, osearch.topk_from_scores, ids of -inf slots set to -1.  Bar as for filtered search: ids and
ranks bit-exact, fp64 ranking scores bit-exact, fp32 scores == float32(oracle), flags 0 on the raw
path unless the case is about overflow."""
import os
import threading

import numpy as np
import pytest

from oracle import encoder as oenc, search as osearch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
INF = float("inf")

_CACHE = {}


def scored(n, d, B, cseed=1234, qseed=5678):
    """(corpus fp16, queries fp16, oracle score matrix f64 [B, n]); one large case kept at a time."""
    key = (n, d, B, cseed, qseed)
    if key not in _CACHE:
        _CACHE.clear()
        c16 = osearch.synth_unit_rows(n, d, cseed)
        q16 = osearch.synth_unit_rows(B, d, qseed)
        _CACHE[key] = (c16, q16, osearch.exact_scores(q16, c16))
    return _CACHE[key]


def make_index(c16, device):
    import torch
    from rag_fin_amd.store import GpuIndex
    ix = GpuIndex(c16.shape[1], max(c16.shape[0], 1), device)
    ix.add(torch.from_numpy(c16).to(device))
    return ix


def band_oracle(S, lo, hi, k, mask=None):
    M = S.copy()
    out = ~((S > lo) & (S <= hi))
    if mask is not None:
        out |= ~mask[None, :]
    M[out] = -np.inf
    es, ei = osearch.topk_from_scores(M, k)
    ei[es == -np.inf] = -1
    return es, ei


def band_counts(S, lo, hi):
    return ((S > lo) & (S <= hi)).sum(axis=1)


def kth_best(S, k):
    """The k-th best score of every query (k = 1: the best)."""
    return -np.partition(-S, k - 1, axis=1)[:, k - 1]


def check_equal(scores, ids, exact, es, ei):
    ids = ids.cpu().numpy()
    assert np.array_equal(ids, ei), f"ids differ at {np.argwhere(ids != ei)[:5]}"
    assert np.array_equal(exact.cpu().numpy(), es)
    assert np.array_equal(scores.cpu().numpy(), es.astype(np.float32))


def check_band(ix, q16, S, lo, hi, k, device, raw=True, mask=None, filt=None):
    import torch
    q = torch.from_numpy(q16).to(device)
    es, ei = band_oracle(S, lo, hi, k, mask)
    if raw:
        scores, ids, exact, flags = ix.search_raw(q, k, want_exact=True, filt=filt, band=(lo, hi))
        torch.cuda.synchronize()
        assert int(flags.abs().sum()) == 0, f"flags set: {np.flatnonzero(flags.cpu().numpy())[:8]}"
    else:
        scores, ids, exact = ix.search(q, k, want_exact=True, filt=filt, band=(lo, hi))
    check_equal(scores, ids, exact, es, ei)
    return es, ei


# ---- parity on random unit corpora ------------------------------------------------------------
SHAPES = [(100_000, 384, B, k) for B in (1, 64, 100) for k in (1, 10, 64)] + \
         [(20_000, 768, B, k) for B, k in ((1, 10), (64, 10), (64, 64), (100, 1))] + \
         [(5_000, 384, B, k) for B, k in ((1, 64), (64, 10), (64, 64), (100, 10))]


def quantile_band(S, k):
    """lo = the median over queries of the k-th best score, hi = the median of the best score (for
    k < 4 the 4th best stands in for the k-th, so that the band is not empty by construction)."""
    lo = float(np.median(kth_best(S, max(k, 4))))
    hi = float(np.median(kth_best(S, 1)))
    return lo, hi


def assert_not_vacuous(S, lo, hi, k):
    """The condition of the B >= 64, k >= 10 cases, on the oracle's counts alone."""
    B = S.shape[0]
    cnt = band_counts(S, lo, hi)
    short = int(((cnt >= 1) & (cnt <= k - 1)).sum())
    full = int((cnt >= k).sum())
    clipped = int((S > hi).any(axis=1).sum())
    print(f"band ({lo:.5f}, {hi:.5f}]: {short} queries end by the band, {full} by the limit, {clipped} lose a row "
          f"to the ceiling, at most {int(cnt.max())} band rows")
    assert short * 4 >= B and full * 4 >= B and clipped * 4 >= B, (short, full, clipped, B)


@pytest.mark.parametrize("n,d,B,k", SHAPES)
def test_band_equals_oracle(gpu_device, n, d, B, k):
    c16, q16, S = scored(n, d, B)
    lo, hi = quantile_band(S, k)
    if B >= 64 and k >= 10:
        assert_not_vacuous(S, lo, hi, k)
    else:
        assert band_counts(S, lo, hi).max() >= 1
    check_band(make_index(c16, gpu_device), q16, S, lo, hi, k, gpu_device)


def test_band_equals_oracle_one_million_rows(gpu_device):
    c16, q16, S = scored(1_000_000, 384, 8)
    lo, hi = quantile_band(S, 10)
    assert band_counts(S, lo, hi).max() >= 1 and (S > hi).any()
    check_band(make_index(c16, gpu_device), q16, S, lo, hi, 10, gpu_device)


# ---- edges ------------------------------------------------------------------------------------
def _edge_values(S):
    """Scores of chosen rows of query 0: its 2nd best (a ceiling) and its 12th best (a floor)."""
    s0 = np.sort(S[0])[::-1]
    return float(s0[11]), float(s0[1])


@pytest.mark.parametrize("n", [5_000, 100_000])
@pytest.mark.parametrize("lo_step", [-1, 0, 1])
@pytest.mark.parametrize("hi_step", [-1, 0, 1])
def test_bounds_equal_to_row_scores(gpu_device, n, lo_step, hi_step):
    """radius / range_filter equal to the contract score of a row (excluded / included), and the
    neighbouring doubles either side."""
    c16, q16, S = scored(n, 384, 8)
    lo, hi = _edge_values(S)
    step = lambda v, s: v if s == 0 else float(np.nextafter(v, s * INF))
    lo, hi = step(lo, lo_step), step(hi, hi_step)
    es, ei = check_band(make_index(c16, gpu_device), q16, S, lo, hi, 16, gpu_device)
    # query 0: ranks 2..11 (10 rows) at the exact values; one more at either end when the bound moves outwards
    want = 10 + (1 if lo_step < 0 else 0) - (1 if hi_step < 0 else 0)
    assert int((ei[0] >= 0).sum()) == want


@pytest.mark.parametrize("n", [5_000, 100_000])
def test_band_above_the_best_score_is_empty(gpu_device, n):
    c16, q16, S = scored(n, 384, 8)
    lo = float(S.max())
    es, ei = check_band(make_index(c16, gpu_device), q16, S, lo, INF, 10, gpu_device)
    assert (ei == -1).all()
    check_band(make_index(c16, gpu_device), q16, S, 0.9, 0.95, 10, gpu_device)


@pytest.mark.parametrize("n", [5_000, 100_000])
def test_ceiling_only_and_open_band(gpu_device, n):
    import torch
    c16, q16, S = scored(n, 384, 8)
    ix = make_index(c16, gpu_device)
    hi = float(np.median(kth_best(S, 30)))   # "the 10 best below the 30th best of the median query"
    es, ei = check_band(ix, q16, S, -INF, hi, 10, gpu_device)
    assert (ei >= 0).all()
    # (-inf, +inf] holds every row: the bits of rf_search
    q = torch.from_numpy(q16).to(gpu_device)
    a = ix.search_raw(q, 10, want_exact=True)
    b = ix.search_raw(q, 10, want_exact=True, band=(-INF, INF))
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert int(b[3].abs().sum()) == 0


@pytest.mark.parametrize("n", [5_000, 60_000])
def test_duplicate_rows_straddle_the_limit(gpu_device, n):
    """Twelve copies of one row inside the band, limit 8 cutting through them: tie order by row."""
    c16 = osearch.synth_unit_rows(n, 384, 21).copy()
    q16 = osearch.synth_unit_rows(4, 384, 22)
    S0 = osearch.exact_scores(q16, c16)
    src = int(np.argsort(-S0[0])[4])              # query 0's 5th best row
    dup = np.random.default_rng(3).choice(n, 12, replace=False)
    c16[dup] = c16[src]
    S = osearch.exact_scores(q16, c16)
    s0 = np.sort(S[0])[::-1]
    lo, hi = float(s0[40]), float(s0[2])          # drops the best two, keeps the equal rows
    es, ei = check_band(make_index(c16, gpu_device), q16, S, lo, hi, 8, gpu_device)
    tied = np.unique(np.append(dup, src))
    assert tied.size >= 12 and np.array_equal(ei[0][2:], tied[:6])   # ranks 3, 4, then the first six copies by row


# ---- crowding -----------------------------------------------------------------------------------
def test_upper_fringe_crowding(gpu_device):
    """320 identical rows scoring one ulp above range_filter, the band below them: the fused path
    proves the answer or flags and the ladder answers; either way it is the oracle's."""
    import torch
    n = 50_000
    c16 = osearch.synth_unit_rows(n, 384, 31).copy()
    q16 = osearch.synth_unit_rows(4, 384, 32)
    S0 = osearch.exact_scores(q16, c16)
    src = int(np.argsort(-S0[0])[20])
    c16[np.random.default_rng(4).choice(n, 320, replace=False)] = c16[src]
    S = osearch.exact_scores(q16, c16)
    hi = float(np.nextafter(S[0, src], -INF))
    lo = float(np.sort(S[0])[::-1][400])
    assert int((S[0] == S[0, src]).sum()) >= 300 and band_counts(S, lo, hi)[0] >= 10
    ix = make_index(c16, gpu_device)
    check_band(ix, q16, S, lo, hi, 10, gpu_device, raw=False)
    q = torch.from_numpy(q16).to(gpu_device)
    scores, ids, exact, flags = ix.search_raw(q, 10, want_exact=True, band=(lo, hi))
    es, ei = band_oracle(S, lo, hi, 10)
    ok = (flags == 0).cpu().numpy()
    assert np.array_equal(ids.cpu().numpy()[ok], ei[ok]) and np.array_equal(exact.cpu().numpy()[ok], es[ok])


def test_all_duplicate_corpus_inside_the_band(gpu_device):
    """Every row the same vector, all inside the band: the candidate lists overflow, the ladder
    answers through the exhaustive band kernel with rows 0..k-1."""
    import torch
    n = 40_000
    row = osearch.synth_unit_rows(1, 384, 41)
    c16 = np.repeat(row, n, axis=0)
    q16 = np.concatenate([row, osearch.synth_unit_rows(2, 384, 42)])
    S = osearch.exact_scores(q16, c16)
    ix = make_index(c16, gpu_device)
    lo, hi = float(S[0, 0]) - 0.5, float(S[0, 0])
    es, ei = check_band(ix, q16, S, lo, hi, 10, gpu_device, raw=False)
    assert np.array_equal(ei[0], np.arange(10))
    q = torch.from_numpy(q16).to(gpu_device)
    flags = ix.search_raw(q, 10, band=(lo, hi))[3]
    assert int(flags[0]) != 0


# ---- with expr --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5_001, 100_003])
@pytest.mark.parametrize("kind", ["all", "none", "k-1", "contig8", "rr8", "rand50", "rand0.1"])
def test_band_within_a_filter(gpu_device, n, kind):
    from test_filtered_search_gpu import filter_from_mask, selection
    B, k = (7, 10) if n < 8192 else (64, 10)
    c16, q16, S = scored(n, 384, B)
    mask = selection(kind, n, k, np.random.default_rng(2))
    Sm = np.where(mask[None, :], S, -np.inf)
    if mask.sum() >= 4:
        lo, hi = quantile_band(Sm, min(k, int(mask.sum())))
    else:
        lo, hi = -0.5, 0.5
    filt = filter_from_mask(mask, gpu_device)
    check_band(make_index(c16, gpu_device), q16, S, lo, hi, k, gpu_device, mask=mask, filt=filt)


# ---- limits above RF_MAX_K --------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [200, 1000])
def test_paged_band(gpu_device, limit):
    """Half of the queries scaled down (inner-product scores shrink with them): at one floor the
    full-length queries have more than 1000 band rows, the others a few hundred at most, so the
    paging runs to the limit for some and stops early for others."""
    import torch
    n, d, B = 100_000, 384, 6
    c16 = osearch.synth_unit_rows(n, d, 1234)
    q = osearch.synth_unit_rows(B, d, 77).astype(np.float32)
    q[B // 2:] *= 0.73
    q16 = q.astype(np.float16)
    S = osearch.exact_scores(q16, c16)
    lo = float(np.median(kth_best(S[:B // 2], 1500)))
    cnt = band_counts(S, lo, INF)
    print("band rows per query:", cnt.tolist())
    assert (cnt > 1000).any() and ((cnt >= 50) & (cnt <= 400)).any()
    ix = make_index(c16, gpu_device)
    scores, ids, exact = ix.search_large(torch.from_numpy(q16).to(gpu_device), limit, want_exact=True, band=(lo, INF))
    check_equal(scores, ids, exact, *band_oracle(S, lo, INF, limit))
    hi = float(np.median(kth_best(S[:B // 2], 100)))
    scores, ids, exact = ix.search_large(torch.from_numpy(q16).to(gpu_device), limit, want_exact=True, band=(lo, hi))
    check_equal(scores, ids, exact, *band_oracle(S, lo, hi, limit))


def _store(c16, device, index_type=None):
    import torch
    from rag_fin_amd.store import CorpusStore
    n = c16.shape[0]
    st = CorpusStore("range", dim=c16.shape[1], capacity=n, device=device, metric_type="IP")
    st.add(list(range(n)), [""] * n, torch.from_numpy(c16).to(device), ["Q1"] * n, ["t"] * n, ["s"] * n, [0.0] * n)
    if index_type:
        st.create_index("embedding", {"index_type": index_type, "metric_type": "IP"})
    return st


def test_store_search_with_radius_on_flat_and_sq8(gpu_device):
    """CorpusStore.search with range parameters: hit lists equal the oracle's band ranking (a short
    list where the band ends it), also at limit 200, and an SQ8 collection gives the same answers
    from its fp16 rows while staying an SQ8 collection."""
    import torch
    n, d, B, k = 50_000, 384, 16, 10
    c16 = osearch.synth_unit_rows(n, d, 1234)
    q16 = osearch.synth_unit_rows(B, d, 5678)
    S = osearch.exact_scores(q16, c16)
    lo, hi = quantile_band(S, k)
    cnt = band_counts(S, lo, hi)
    assert (cnt < k).any() and (cnt >= k).any()
    for itype in (None, "SQ8"):
        st = _store(c16, gpu_device, itype)
        for limit, (blo, bhi) in ((k, (lo, hi)), (200, (float(np.median(kth_best(S, 150))), INF))):
            es, ei = band_oracle(S, blo, bhi, limit)
            params = {"radius": blo} if bhi == INF else {"radius": blo, "range_filter": bhi}
            res = st.search(torch.from_numpy(q16).to(gpu_device), "embedding",
                            {"metric_type": "IP", "params": dict(params, nprobe=16)}, limit=limit)
            for b in range(B):
                want = ei[b][ei[b] >= 0]
                assert [h.id for h in res[b]] == want.tolist()
                assert [h.score for h in res[b]] == es[b][:want.size].astype(np.float32).tolist()
        assert st.index_type == ("SQ8" if itype else "FLAT")


# ---- hipGraph, threads --------------------------------------------------------------------------
def test_graph_capture_and_replay(gpu_device):
    """rf_search_range captured into a graph on one stream; two replays give the eager bits."""
    import torch
    c16, q16, S = scored(100_000, 384, 64)
    lo, hi = quantile_band(S, 10)
    ix = make_index(c16, gpu_device)
    q = torch.from_numpy(q16).to(gpu_device)
    eager = ix.search_raw(q, 10, want_exact=True, band=(lo, hi))
    torch.cuda.synchronize()
    out = ix._outputs(64, 10, want_exact=True)
    ws = ix.new_workspace()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ix.search_raw(q, 10, want_exact=True, out=out, workspace=ws, band=(lo, hi))
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    for _ in range(2):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(eager, out):
            assert torch.equal(x, y)
    check_equal(out[0], out[1], out[2], *band_oracle(S, lo, hi, 10))


def test_two_threads_two_bands(gpu_device):
    import torch
    c16, q16, S = scored(100_000, 384, 64)
    ix = make_index(c16, gpu_device)
    q = torch.from_numpy(q16).to(gpu_device)
    bands = [quantile_band(S, 10), (float(np.median(kth_best(S, 40))), float(np.median(kth_best(S, 5))))]
    want = [band_oracle(S, lo, hi, 10) for lo, hi in bands]
    errors = []

    def work(t):
        try:
            with torch.cuda.device(gpu_device), torch.cuda.stream(torch.cuda.Stream(gpu_device)):
                ws = ix.new_workspace()
                torch.cuda.current_stream().synchronize()
                for _ in range(20):
                    scores, ids, exact, flags = ix.search_raw(q, 10, want_exact=True, workspace=ws, band=bands[t])
                    torch.cuda.current_stream().synchronize()
                    assert int(flags.abs().sum()) == 0
                    check_equal(scores, ids, exact, *want[t])
        except BaseException as e:   # noqa: BLE001 - reported by the main thread
            errors.append(e)

    torch.cuda.synchronize()
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ---- C ABI argument checks ------------------------------------------------------------------------
def test_invalid_bands_are_refused(gpu_device):
    import torch
    from rag_fin_amd import _lib
    c16, q16, S = scored(5_000, 384, 8)
    ix = make_index(c16, gpu_device)
    q = torch.from_numpy(q16).to(gpu_device)
    for band in ((0.5, 0.5), (0.6, 0.5), (float("nan"), 0.5), (0.1, float("nan")), (INF, INF)):
        with pytest.raises(_lib.RagfinError):
            ix.search_raw(q, 10, band=band)
        with pytest.raises(_lib.RagfinError):
            ix.search_exhaustive(q, 10, band=band)
    s, i, e = ix.search_exhaustive(q, 10, want_exact=True, band=(-INF, 0.1))
    check_equal(s, i, e, *band_oracle(S, -INF, 0.1, 10))


# ---- end to end on the golden chunks -----------------------------------------------------------------
def test_min_score_on_the_golden_chunks(gpu_device):
    from rag_fin_amd import chunker
    from rag_fin_amd.embedder import Embedder
    from rag_fin_amd.rag import VectorRAG
    from rag_fin_amd.service import ingest
    from rag_fin_amd.store import CorpusStore
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    question = "What was ICICI's Q1 net profit and profitability?"
    chunks = chunker.build_all_chunks(os.path.join(GOLD, "extract_data"))
    probe = WordPieceTokenizer(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"])
    words = sorted({w for t in [c["text"] for c in chunks] + [question] for w in probe.basic_tokens(t)})
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words + \
            [ch for ch in "abcdefghijklmnopqrstuvwxyz0123456789"] + ["##" + ch for ch in "abcdefghijklmnopqrstuvwxyz0123456789"]
    tok = WordPieceTokenizer(list(dict.fromkeys(vocab)))
    cfg = dict(oenc.MINILM_L6, vocab_size=len(tok.vocab))
    emb = Embedder(oenc.random_weights(cfg, 42), cfg, tokenizer=tok, device=gpu_device)
    store = CorpusStore("fin_chunks", dim=384, capacity=16, device=gpu_device)
    assert ingest(store, emb, chunks) == 16
    rag = VectorRAG("no-key", "fin_chunks", embedder=emb, store=store)
    plain = rag.search(question, top_k=5)
    # the fp64 ranking scores of the plain search for this question
    q16 = store._prepare_queries(emb.encode([question]))
    exact = store.index.search(q16, 5, want_exact=True)[2][0].cpu().numpy()
    assert exact[1] > exact[2]
    s = float(exact[2] + (exact[1] - exact[2]) / 2)
    got = rag.search(question, top_k=5, min_score=s)
    assert [c["rank"] for c in got] == [1, 2]
    assert got == plain[:2]
    assert rag.search(question, top_k=5, min_score=float(exact[0]) + 1e-3) == []
    below = rag.search(question, top_k=5, max_score=s)      # the five best below the cut: ranks 3..7 of the plain order
    assert [c["rank"] for c in below] == [1, 2, 3, 4, 5]
    assert [c["text"] for c in below[:3]] == [c["text"] for c in plain[2:]]
    res = rag.search_and_answer(question, top_k=5, min_score=float(exact[0]) + 1e-3)
    assert res["contexts"] == [] and res["context_count"] == 0 and set(res) == {"error", "contexts", "context_count"}
