"""Filtered search on the GPU: rf_filter_eval / rf_filter_from_mask against numpy, and
rf_search_filtered against the CPU oracle run on the passing rows only (ids mapped back).
Bar as for unfiltered search: ids and ranks bit-exact, fp64 ranking scores bit-exact, fp32
scores == float32(oracle), flags 0 on the raw path."""
import os
import threading
from ctypes import c_void_p

import numpy as np
import pytest

from oracle import c_oracle, encoder as oenc, search as osearch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

_CORPORA = {}


def corpus(n, d, seed=11):
    key = (n, d, seed)
    if key not in _CORPORA:
        _CORPORA.clear()   # one large corpus at a time
        _CORPORA[key] = osearch.synth_unit_rows(n, d, seed)
    return _CORPORA[key]


def make_index(c16, device):
    import torch
    from rag_fin_amd.store import GpuIndex
    ix = GpuIndex(c16.shape[1], max(c16.shape[0], 1), device)
    ix.add(torch.from_numpy(c16).to(device))
    return ix


def pack_mask(mask):
    n = mask.size
    words = np.zeros((n + 31) // 32 * 32, dtype=bool)
    words[:n] = mask
    return np.packbits(words.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint32).copy()


def filter_from_mask(mask, device):
    import torch
    from rag_fin_amd import _lib
    lib = _lib.load_library()
    n = mask.size
    buf = torch.empty(lib.rf_filter_bytes(n), dtype=torch.uint8, device=device)
    w = torch.from_numpy(pack_mask(mask).view(np.int32)).to(device)
    with torch.cuda.device(device):
        _lib.check(lib.rf_filter_from_mask(c_void_p(w.data_ptr()) if n else None, n, c_void_p(buf.data_ptr()),
                                           _lib.current_stream_ptr()))
    torch.cuda.synchronize(device)
    return buf


def read_filter(buf, n):
    raw = buf.cpu().numpy().view(np.uint32)
    nblk = (n + 31) // 32
    a = (nblk * 4 + 15) // 16 * 16 // 4
    hdr = raw[:4]
    mask = raw[4:4 + nblk]
    blocks = raw[4 + a:4 + a + int(hdr[2])]
    return hdr, mask, blocks


def expect_filter(mask):
    n = mask.size
    words = pack_mask(mask)
    blocks = np.flatnonzero(words != 0).astype(np.uint32)
    return words, blocks, int(mask.sum())


def oracle_on_subset(q16, c16, S, k):
    B = q16.shape[0]
    es = np.full((B, k), -np.inf)
    ei = np.full((B, k), -1, dtype=np.int64)
    if S.size:
        s, i = c_oracle.search(q16, c16[S], k)
        es[:] = s
        ei[:] = np.where(i >= 0, S[np.maximum(i, 0)], -1)
    return es, ei


def selection(kind, n, k, rng):
    m = np.zeros(n, dtype=bool)
    if kind == "all":
        m[:] = True
    elif kind == "none":
        pass
    elif kind == "one":
        m[rng.integers(n)] = True
    elif kind == "k-1":
        m[rng.choice(n, max(k - 1, 0), replace=False)] = True
    elif kind == "last_block":
        m[n // 32 * 32:] = True
    elif kind == "contig8":
        m[3 * n // 8:4 * n // 8] = True
    elif kind == "contig64":
        m[n // 2:n // 2 + n // 64] = True
    elif kind == "rr8":
        m[3::8] = True
    elif kind == "rand50":
        m[rng.random(n) < 0.5] = True
    elif kind == "rand0.1":
        m[rng.random(n) < 0.001] = True
    else:
        raise ValueError(kind)
    return m


def check_filtered(ix, q16, c16, mask, k, device, raw=True):
    import torch
    filt = filter_from_mask(mask, device)
    q = torch.from_numpy(q16).to(device)
    if raw:
        scores, ids, exact, flags = ix.search_raw(q, k, want_exact=True, filt=filt)
        torch.cuda.synchronize()
        assert int(flags.abs().sum()) == 0, f"flags set: {np.flatnonzero(flags.cpu().numpy())[:8]}"
    else:
        scores, ids, exact = ix.search(q, k, want_exact=True, filt=filt)
    es, ei = oracle_on_subset(q16, c16, np.flatnonzero(mask), k)
    ids = ids.cpu().numpy()
    assert np.array_equal(ids, ei), f"ids differ at {np.argwhere(ids != ei)[:5]}"
    assert np.array_equal(exact.cpu().numpy(), es)
    assert np.array_equal(scores.cpu().numpy(), es.astype(np.float32))
    return filt


# ---- the filter buffer -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 8193, 100_003])
def test_filter_eval_mask_counts_and_blocks_equal_numpy(gpu_device, n):
    from rag_fin_amd import filter_expr
    from rag_fin_amd.store import eval_filter
    import torch
    rng = np.random.default_rng(n)
    dicts = {"period": ["Q1_FY2024", "Q2_FY2024", "Q3_FY2024", "Q4_FY2024", ""],
             "chunk_type": ["balance_sheet", "key_ratios", "segment"], "statement_type": ["consolidated", "standalone"]}
    codes = [rng.integers(len(dicts[f]), size=n).astype(np.int32) for f in ("period", "chunk_type", "statement_type")]
    vals = rng.normal(size=n)
    vals[rng.random(n) < 0.05] = np.nan
    vals[rng.random(n) < 0.05] = -0.0
    pk = {f"k{i}": i for i in range(n)}
    picked = sorted(set(rng.integers(n, size=min(n, 50)).tolist()))
    expr = ('(period in ["Q1_FY2024", "Q3_FY2024"] and primary_value > 0.25) or chunk_type like "%ratio%" and '
            f'statement_type != "standalone" or id in [{", ".join(repr(f"k{i}") for i in picked)}] or primary_value == 0')
    prog = filter_expr.compile_expr(expr, dicts, pk)
    cols = [torch.from_numpy(c).to(gpu_device) for c in codes] + [torch.from_numpy(vals).to(gpu_device)]
    buf = eval_filter(gpu_device, prog, cols, n)
    per = np.array(dicts["period"])[codes[0]]
    ct = np.array(dicts["chunk_type"])[codes[1]]
    st = np.array(dicts["statement_type"])[codes[2]]
    want = ((np.isin(per, ["Q1_FY2024", "Q3_FY2024"]) & (vals > 0.25)) |
            (np.char.find(ct.astype(str), "ratio") >= 0) & (st != "standalone") |
            np.isin(np.arange(n), picked) | (vals == 0))
    hdr, mask, blocks = read_filter(buf, n)
    words, wblocks, npass = expect_filter(want)
    assert list(hdr[:3]) == [n, npass, wblocks.size]
    assert np.array_equal(mask, words)
    assert np.array_equal(blocks, wblocks)


@pytest.mark.parametrize("n", [0, 1, 33, 100_003])
def test_filter_from_mask_clears_bits_past_the_end(gpu_device, n):
    import torch
    from rag_fin_amd import _lib
    lib = _lib.load_library()
    rng = np.random.default_rng(1)
    want = rng.random(n) < 0.3
    words = pack_mask(want)
    if words.size:
        words[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32) if n % 32 else np.uint32(0)   # garbage past n
    buf = torch.empty(lib.rf_filter_bytes(n), dtype=torch.uint8, device=gpu_device)
    w = torch.from_numpy(words.view(np.int32)).to(gpu_device) if words.size else None
    _lib.check(lib.rf_filter_from_mask(c_void_p(w.data_ptr()) if w is not None else None, n,
                                       c_void_p(buf.data_ptr()), _lib.current_stream_ptr()))
    hdr, mask, blocks = read_filter(buf, n)
    ew, eb, npass = expect_filter(want)
    assert list(hdr[:3]) == [n, npass, eb.size]
    assert np.array_equal(mask, ew) and np.array_equal(blocks, eb)


# ---- parity with the oracle on the passing rows --------------------------------------------------
SMALL_KINDS = ["all", "none", "one", "k-1", "last_block", "contig8", "rr8", "rand50", "rand0.1"]


@pytest.mark.parametrize("kind", SMALL_KINDS)
def test_small_corpus_path(gpu_device, kind):
    n, d, B, k = 5001, 384, 7, 10
    c16 = corpus(n, d)
    q16 = osearch.synth_unit_rows(B, d, 5)
    check_filtered(make_index(c16, gpu_device), q16, c16, selection(kind, n, k, np.random.default_rng(2)), k, gpu_device)


@pytest.mark.parametrize("kind", SMALL_KINDS + ["contig64"])
def test_sample_path(gpu_device, kind):
    n, d, B, k = 100_003, 384, 64, 10
    c16 = corpus(n, d)
    q16 = osearch.synth_unit_rows(B, d, 6)
    check_filtered(make_index(c16, gpu_device), q16, c16, selection(kind, n, k, np.random.default_rng(3)), k, gpu_device)


@pytest.mark.parametrize("n,d,B,k,kinds", [
    (100_003, 384, 1, 10, ["contig8", "rand0.1"]),
    (100_003, 384, 7, 1, ["rand50", "rr8"]),
    (100_003, 384, 7, 64, ["contig8", "rr8", "rand0.1", "all"]),
    (100_003, 384, 65, 10, ["rr8"]),
    (100_003, 384, 256, 10, ["contig8", "rand50"]),   # never the wide sweep: four 64-query sweeps
    (50_000, 768, 64, 10, ["contig8", "rand50", "last_block"]),   # 8-wave kernel
    (50_000, 768, 65, 64, ["rr8"]),
])
def test_shapes(gpu_device, n, d, B, k, kinds):
    c16 = corpus(n, d)
    ix = make_index(c16, gpu_device)
    q16 = osearch.synth_unit_rows(B, d, 7)
    rng = np.random.default_rng(4)
    for kind in kinds:
        check_filtered(ix, q16, c16, selection(kind, n, k, rng), k, gpu_device)


def test_one_million_rows(gpu_device):
    n, d, B, k = 1_000_000, 384, 64, 10
    c16 = corpus(n, d)
    ix = make_index(c16, gpu_device)
    q16 = osearch.synth_unit_rows(B, d, 8)
    rng = np.random.default_rng(5)
    for kind in ["contig8", "rr8", "rand0.1", "contig64"]:
        check_filtered(ix, q16, c16, selection(kind, n, k, rng), k, gpu_device)


@pytest.mark.parametrize("n", [5001, 100_003])
def test_all_pass_filter_gives_the_unfiltered_bits(gpu_device, n):
    import torch
    c16 = corpus(n, 384)
    ix = make_index(c16, gpu_device)
    q = torch.from_numpy(osearch.synth_unit_rows(64, 384, 9)).to(gpu_device)
    filt = filter_from_mask(np.ones(n, dtype=bool), gpu_device)
    a = ix.search_raw(q, 10, want_exact=True)
    b = ix.search_raw(q, 10, want_exact=True, filt=filt)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("n", [5001, 100_003])
def test_rejected_rows_that_outscore_every_passing_row_never_appear(gpu_device, n):
    c16 = corpus(n, 384)
    ix = make_index(c16, gpu_device)
    mask = selection("rr8", n, 10, None)
    rejected = np.flatnonzero(~mask)[:: max(1, n // 40)][:40]
    q16 = c16[rejected]       # each query's best row overall is a rejected row (itself)
    check_filtered(ix, q16, c16, mask, 10, gpu_device)


def test_duplicate_passing_rows_flag_and_store_answer_is_exact(gpu_device):
    import torch
    n, d, k = 100_003, 384, 10
    c16 = corpus(n, d).copy()
    c16[:20_000] = c16[0]          # 20 000 identical passing rows: ties overflow the candidate lists
    ix = make_index(c16, gpu_device)
    mask = np.zeros(n, dtype=bool)
    mask[:20_000] = True
    mask[50_000:50_100] = True
    q16 = np.concatenate([c16[:1], osearch.synth_unit_rows(3, d, 10)])
    filt = filter_from_mask(mask, gpu_device)
    _, _, _, flags = ix.search_raw(torch.from_numpy(q16).to(gpu_device), k, filt=filt)
    assert int(flags[0]) != 0
    check_filtered(ix, q16, c16, mask, k, gpu_device, raw=False)


@pytest.mark.parametrize("limit", [100, 1000])
def test_limits_above_64_with_a_filter(gpu_device, limit):
    import torch
    n = 100_003
    c16 = corpus(n, 384)
    ix = make_index(c16, gpu_device)
    q16 = osearch.synth_unit_rows(3, 384, 11)
    mask = selection("contig8", n, limit, np.random.default_rng(6))
    filt = filter_from_mask(mask, gpu_device)
    s, i, e = ix.search_large(torch.from_numpy(q16).to(gpu_device), limit, want_exact=True, filt=filt)
    es, ei = oracle_on_subset(q16, c16, np.flatnonzero(mask), limit)
    assert np.array_equal(i.cpu().numpy(), ei)
    assert np.array_equal(e.cpu().numpy(), es)


def test_same_filtered_search_twice_is_bit_identical(gpu_device):
    import torch
    n = 100_003
    c16 = corpus(n, 384)
    ix = make_index(c16, gpu_device)
    q = torch.from_numpy(osearch.synth_unit_rows(64, 384, 12)).to(gpu_device)
    filt = filter_from_mask(selection("rand50", n, 10, np.random.default_rng(7)), gpu_device)
    a = [t.clone() for t in ix.search_raw(q, 10, want_exact=True, filt=filt)]
    b = ix.search_raw(q, 10, want_exact=True, filt=filt)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_two_threads_with_different_filters(gpu_device):
    import torch
    n = 100_003
    c16 = corpus(n, 384)
    ix = make_index(c16, gpu_device)
    q16 = osearch.synth_unit_rows(16, 384, 13)
    masks = [selection("contig8", n, 10, None), selection("rr8", n, 10, None)]
    want = [oracle_on_subset(q16, c16, np.flatnonzero(m), 10) for m in masks]
    errors = []

    def work(j):
        try:
            torch.cuda.set_device(gpu_device)
            filt = filter_from_mask(masks[j], gpu_device)
            q = torch.from_numpy(q16).to(gpu_device)
            for _ in range(5):
                _, ids, exact = ix.search(q, 10, want_exact=True, filt=filt)
                torch.cuda.synchronize()
                if not (np.array_equal(ids.cpu().numpy(), want[j][1]) and np.array_equal(exact.cpu().numpy(), want[j][0])):
                    errors.append(j)
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))
    ts = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


# ---- through the store ---------------------------------------------------------------------------
def golden_store(device, capacity=8):
    from rag_fin_amd import chunker
    from rag_fin_amd.store import CorpusStore
    chunks = chunker.build_all_chunks(os.path.join(GOLD, "extract_data"))
    st = CorpusStore("fin_chunks", dim=384, capacity=capacity, device=device)
    emb = np.random.default_rng(0).normal(size=(len(chunks), 384)).astype(np.float32)
    st.add([c["id"] for c in chunks], [c["text"] for c in chunks], emb, [c["period"] for c in chunks],
           [c["chunk_type"] for c in chunks], [c["statement_type"] for c in chunks],
           [c["primary_value"] for c in chunks])
    return st, chunks, emb


def store_oracle(st, q32, mask, k):
    import torch
    c16 = st.index.get_rows(np.arange(st.num_entities)).cpu().numpy()
    q16 = st._prepare_queries(q32).cpu().numpy()
    return oracle_on_subset(q16, c16, np.flatnonzero(mask), k)


def test_store_search_with_a_period_filter(gpu_device):
    st, chunks, emb = golden_store(gpu_device)
    per = np.array([c["period"] for c in chunks])
    q = np.random.default_rng(1).normal(size=(3, 384)).astype(np.float32)
    res = st.search(q, "embedding", {"metric_type": "COSINE"}, 3, expr='period == "Q2_FY2024"',
                    output_fields=["period"])
    assert (per == "Q2_FY2024").sum() >= 3
    _, ei = store_oracle(st, q, per == "Q2_FY2024", 3)
    for b, hits in enumerate(res):
        assert [h.row for h in hits] == ei[b].tolist()
        assert all(h.entity.period == "Q2_FY2024" for h in hits)


def test_store_search_mixed_predicate_and_query_rows(gpu_device):
    st, chunks, emb = golden_store(gpu_device)
    per = np.array([c["period"] for c in chunks])
    pv = np.array([c["primary_value"] for c in chunks], dtype=float)
    x = float(np.nanmedian(pv))
    expr = f'period in ["Q1_FY2024", "Q3_FY2024"] and primary_value > {x!r}'
    mask = np.isin(per, ["Q1_FY2024", "Q3_FY2024"]) & (pv > x)
    q = np.random.default_rng(2).normal(size=(2, 384)).astype(np.float32)
    res = st.search(q, limit=5, expr=expr)
    _, ei = store_oracle(st, q, mask, 5)
    for b, hits in enumerate(res):
        assert [h.row for h in hits] == [r for r in ei[b].tolist() if r >= 0]
    got = st.query(expr=expr, output_fields=["id", "period"])
    assert [st._pk_row[r["id"]] for r in got] == np.flatnonzero(mask).tolist()
    assert len(st.query(expr=expr, limit=1)) == min(1, int(mask.sum()))
    # the original forms are unchanged
    assert [r["id"] for r in st.query(expr=f'id in ["{chunks[5]["id"]}", "{chunks[2]["id"]}"]')] == \
        [chunks[5]["id"], chunks[2]["id"]]
    assert len(st.query(expr="", limit=4)) == 4
    assert st.search(q, limit=3, expr="  ")[0][0].row == st.search(q, limit=3)[0][0].row
    with pytest.raises(ValueError):
        st.search(q, limit=3, expr="period > 3")


def test_lazy_column_sync_after_insert_drop_and_reload(gpu_device, tmp_path):
    from rag_fin_amd.store import CorpusStore
    st, chunks, emb = golden_store(gpu_device)
    assert len(st.query(expr='period == "Q9"')) == 0
    st.add(["extra"], ["t"], emb[:1], ["Q9"], ["x"], ["consolidated"], [1.5])
    assert [r["id"] for r in st.query(expr='period == "Q9"')] == ["extra"]
    q = emb[:1] + 0.0
    assert [h.id for h in st.search(q, limit=3, expr='chunk_type == "x"')[0]] == ["extra"]
    st.save(str(tmp_path / "c"))
    again = CorpusStore.load_from(str(tmp_path / "c"), device=gpu_device)
    assert [r["id"] for r in again.query(expr='period == "Q9" or primary_value == 1.5')] == ["extra"]
    st.drop()
    st.add(["a", "b"], ["t", "u"], emb[:2], ["Q9", "Q1"], ["y", "x"], ["s", "s"], [0.0, float("nan")])
    assert [r["id"] for r in st.query(expr='period == "Q9"')] == ["a"]
    assert [r["id"] for r in st.query(expr='chunk_type == "x"')] == ["b"]
    assert [r["id"] for r in st.query(expr="primary_value != 0")] == ["b"]    # NaN != 0 holds
    assert [r["id"] for r in st.query(expr="primary_value < 1 or primary_value >= 1")] == ["a"]


def test_vector_rag_search_with_expr_end_to_end(gpu_device):
    from rag_fin_amd import chunker
    from rag_fin_amd.embedder import Embedder
    from rag_fin_amd.rag import VectorRAG
    from rag_fin_amd.service import ingest
    from rag_fin_amd.store import CorpusStore
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    chunks = chunker.build_all_chunks(os.path.join(GOLD, "extract_data"))
    probe = WordPieceTokenizer(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"])
    words = sorted({w for c in chunks for w in probe.basic_tokens(c["text"])})
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words + list("abcdefghijklmnopqrstuvwxyz0123456789")
    tok = WordPieceTokenizer(list(dict.fromkeys(vocab)))
    cfg = dict(oenc.MINILM_L6, vocab_size=len(tok.vocab))
    emb = Embedder(oenc.random_weights(cfg, 42), cfg, tokenizer=tok, device=gpu_device)
    store = CorpusStore("fin_chunks", dim=384, capacity=16, device=gpu_device)
    ingest(store, emb, chunks)
    rag = VectorRAG("no-key", "fin_chunks", embedder=emb, store=store)
    q = "net profit in Q3 FY2024"
    per = np.array([c["period"] for c in chunks])
    got = rag.search(q, 3, expr='period == "Q3_FY2024"')
    assert len(got) == min(3, int((per == "Q3_FY2024").sum()))
    assert all(c["period"] == "Q3_FY2024" for c in got)
    assert [c["score"] for c in got] == sorted((c["score"] for c in got), reverse=True)
    # the store answer for the same query bits is the oracle's on the Q3 rows
    q16 = emb.encode_to_device([q])
    hits = store.search(q16, limit=3, expr='period == "Q3_FY2024"')[0]
    c16 = store.index.get_rows(np.arange(store.num_entities)).cpu().numpy()
    es, ei = oracle_on_subset(q16.cpu().numpy(), c16, np.flatnonzero(per == "Q3_FY2024"), 3)
    assert [h.row for h in hits] == [r for r in ei[0].tolist() if r >= 0]
    assert [h.score for h in hits] == [float(np.float32(s)) for s in es[0] if s > -np.inf]
    batch = rag.search_batch([q, "deposits"], 2, expr='period == "Q3_FY2024"')
    assert all(c["period"] == "Q3_FY2024" for b in batch for c in b) and [len(b) for b in batch] == [2, 2]
    from rag_fin_amd import mcp_server
    mcp_server.set_rag(rag)
    try:
        r = mcp_server.search_vectors(q, 3, filter='period == "Q3_FY2024"')
        assert r["status"] == "success" and all(c["period"] == "Q3_FY2024" for c in r["results"])
        assert mcp_server.search_vectors(q, 3, filter="period >")["status"] == "error"
    finally:
        mcp_server.set_rag(None)
