"""Per-query filters on the GPU: the multi-filter buffer (rf_multi_filter_build) against numpy, and
rf_search_multi_filtered -- one sweep for a batch whose queries differ in their filter -- against
the CPU oracle run per query on that query's passing rows.  Bar as for filtered search: ids, fp64
ranking scores and fp32 scores bit-equal; where a case says so, flags 0 on the raw path."""
import threading

import numpy as np
import pytest

from oracle import adversarial as adv, search as osearch
from test_filtered_search_gpu import (corpus, expect_filter, filter_from_mask, golden_store, make_index,
                                      oracle_on_subset, pack_mask, read_filter, selection)

pytestmark = pytest.mark.gpu


def multi_filter(masks, qf, device):
    """-> (MultiFilter over one filter buffer per mask, those buffers)."""
    import torch
    from rag_fin_amd.index import MultiFilter
    filters = [filter_from_mask(m, device) for m in masks]
    with torch.cuda.device(device):
        mf = MultiFilter(filters, qf, masks[0].size, device)
    return mf, filters


def expected(q16, c16, masks, qf, k):
    """The oracle per query on its own passing rows (one oracle call per filter)."""
    qf = np.asarray(qf)
    es = np.full((q16.shape[0], k), -np.inf)
    ei = np.full((q16.shape[0], k), -1, dtype=np.int64)
    for g in np.unique(qf):
        at = np.flatnonzero(qf == g)
        es[at], ei[at] = oracle_on_subset(q16[at], c16, np.flatnonzero(masks[g]), k)
    return es, ei


def assert_bits(scores, ids, exact, es, ei):
    ids = ids.cpu().numpy()
    assert np.array_equal(ids, ei), f"ids differ at {np.argwhere(ids != ei)[:5].tolist()}"
    assert np.array_equal(exact.cpu().numpy(), es)
    assert np.array_equal(scores.cpu().numpy(), es.astype(np.float32))


def check_multi(ix, q16, c16, masks, qf, k, device, raw=True, want=None):
    """raw: the raw call must flag no query.  Always: parity through the ladder.  -> (mf, filters, raw flags)."""
    import torch
    mf, filters = multi_filter(masks, qf, device)
    q = torch.from_numpy(q16).to(device)
    es, ei = expected(q16, c16, masks, qf, k) if want is None else want
    scores, ids, exact, flags = ix.search_raw(q, k, want_exact=True, filt=mf)
    torch.cuda.synchronize()
    flags = flags.cpu().numpy()
    if raw:
        assert not flags.any(), f"flags set: {np.flatnonzero(flags)[:8]}"
        assert_bits(scores, ids, exact, es, ei)
    assert_bits(*ix.search(q, k, want_exact=True, filt=mf), es, ei)
    return mf, filters, flags


# ---- 1. the buffer ---------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 33, 8193, 100_003])
def test_buffer_union_and_transposed_words_equal_numpy(gpu_device, n, G):
    import torch
    rng = np.random.default_rng(n + G)
    masks = [rng.random(n) < p for p in rng.choice([0.0, 0.001, 0.3, 1.0], size=G)]
    mf, _ = multi_filter(masks, [0], gpu_device)
    torch.cuda.synchronize()
    nblk = (n + 31) // 32
    union = np.logical_or.reduce(masks)
    hdr, mask, blocks = read_filter(mf.buf, n)
    words, wblocks, npass = expect_filter(union)
    assert list(hdr[:3]) == [n, npass, wblocks.size]
    assert np.array_equal(mask, words) and np.array_equal(blocks, wblocks)
    gp = 1
    while gp < G:
        gp *= 2
    from rag_fin_amd import _lib
    off = (_lib.load_library().rf_filter_bytes(n) + 255) // 256 * 256
    assert mf.buf.numel() == off + nblk * gp * 4
    t = mf.buf[off:].cpu().numpy().view(np.uint32).reshape(nblk, gp)
    for g in range(G):
        assert np.array_equal(t[:, g], pack_mask(masks[g])), g
    assert not t[:, G:].any()
    if n % 32:   # bits past n_rows are clear
        assert not (t[-1] >> np.uint32(n % 32)).any()
    again, _ = multi_filter(masks, [0], gpu_device)
    assert torch.equal(mf.buf, again.buf)


# ---- 2. small-corpus path ----------------------------------------------------------------------------
KINDS = ["all", "none", "one", "k-1", "last_block", "rr8", "rand50"]


@pytest.mark.parametrize("B,kinds", [(7, ["all", "none", "k-1"]), (7, ["one", "last_block", "rr8"]),
                                      (64, [KINDS[g % 7] for g in range(64)])])
def test_small_corpus_path(gpu_device, B, kinds):
    n, d, k = 5001, 384, 10
    c16 = corpus(n, d)
    q16 = osearch.synth_unit_rows(B, d, 5)
    rng = np.random.default_rng(2)
    masks = [selection(kind, n, k, rng) for kind in kinds]
    qf = [b % len(masks) for b in range(B)]
    ix = make_index(c16, gpu_device)
    import torch
    mf, _, flags = check_multi(ix, q16, c16, masks, qf, k, gpu_device)
    # a query whose filter passes no row: an empty padded row, flags 0
    scores, ids, _, _ = ix.search_raw(torch.from_numpy(q16).to(gpu_device), k, filt=mf)
    for b in range(B):
        if kinds[qf[b]] == "none":
            assert (ids[b] == -1).all() and bool(torch.isinf(scores[b]).all()) and flags[b] == 0


# ---- 3. sample path, 5. the same bits as the single-filter path ---------------------------------------
def layout(name, n):
    r = np.arange(n)
    if name == "quarters":
        return [(r * 4 // n) == g for g in range(4)]
    if name == "mod4":
        return [r % 4 == g for g in range(4)]
    if name == "eighths":
        return [(r * 8 // n) == g for g in range(8)]
    if name == "all+half":
        return [np.ones(n, dtype=bool), r % 2 == 1]
    if name == "block_parity":   # every sample stride here is even: a fixed-stride sample reads filter 0 only
        return [(r // 32) % 2 == g for g in range(2)]
    raise ValueError(name)


@pytest.mark.parametrize("name", ["quarters", "mod4", "eighths", "all+half", "block_parity"])
def test_sample_path_flags_nothing_and_equals_the_single_filter_path(gpu_device, name):
    import torch
    n, d, B, k = 100_003, 384, 64, 10
    c16 = corpus(n, d)
    q16 = osearch.synth_unit_rows(B, d, 6)
    masks = layout(name, n)
    qf = [b % len(masks) for b in range(B)]
    ix = make_index(c16, gpu_device)
    mf, filters, _ = check_multi(ix, q16, c16, masks, qf, k, gpu_device)
    q = torch.from_numpy(q16).to(gpu_device)
    multi = ix.search(q, k, want_exact=True, filt=mf)
    for b in range(B):   # every query alone through the single-filter path: bit-identical
        one = ix.search(q[b:b + 1], k, want_exact=True, filt=filters[qf[b]])
        for x, y in zip(multi, one):
            assert torch.equal(x[b:b + 1], y), (name, b)


def test_sample_path_with_a_thin_filter_beside_seven_eighths(gpu_device, capsys):
    """A filter of 0.1 % of the rows beside seven of 1/8 each: parity through the ladder; the raw
    flags of the thin filter's queries are a measurement (printed), not asserted."""
    n, d, B, k = 100_003, 384, 64, 10
    c16 = corpus(n, d)
    q16 = osearch.synth_unit_rows(B, d, 6)
    masks = layout("eighths", n)[:7] + [selection("rand0.1", n, k, np.random.default_rng(3))]
    qf = [b % 8 for b in range(B)]
    _, _, flags = check_multi(make_index(c16, gpu_device), q16, c16, masks, qf, k, gpu_device, raw=False)
    thin = np.array(qf) == 7
    with capsys.disabled():
        print(f"\n[multi-filter] thin filter (0.1 %): {int((flags[thin] != 0).sum())} of {int(thin.sum())} queries "
              f"flagged raw; other filters: {int((flags[~thin] != 0).sum())} of {int((~thin).sum())}")


# ---- 4. shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 64])
@pytest.mark.parametrize("B", [1, 33, 65, 130])
def test_shapes_batch_and_k(gpu_device, B, k):
    n, d = 100_003, 384
    c16 = corpus(n, d)
    q16 = osearch.synth_unit_rows(B, d, 7)
    masks = layout("mod4", n)
    qf = np.random.default_rng(B).integers(4, size=B).tolist()   # the caller's order, not the filters'
    check_multi(make_index(c16, gpu_device), q16, c16, masks, qf, k, gpu_device, raw=False)


def test_shapes_dim_768_and_a_filter_of_the_last_partial_block(gpu_device):
    n, d, B, k = 50_000 + 13, 768, 64, 10   # n is no multiple of 32
    c16 = corpus(n, d)
    q16 = osearch.synth_unit_rows(B, d, 7)
    rng = np.random.default_rng(4)
    masks = [selection("last_block", n, k, rng), selection("rand50", n, k, rng), selection("contig8", n, k, rng)]
    assert masks[0].sum() == n % 32
    qf = [b % 3 for b in range(B)]
    check_multi(make_index(c16, gpu_device), q16, c16, masks, qf, k, gpu_device)


def test_same_multi_filter_search_twice_is_bit_identical(gpu_device):
    import torch
    n = 100_003
    c16 = corpus(n, 384)
    ix = make_index(c16, gpu_device)
    q = torch.from_numpy(osearch.synth_unit_rows(64, 384, 12)).to(gpu_device)
    mf, _ = multi_filter(layout("mod4", n), [b % 4 for b in range(64)], gpu_device)
    a = [t.clone() for t in ix.search_raw(q, 10, want_exact=True, filt=mf)]
    b = ix.search_raw(q, 10, want_exact=True, filt=mf)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_variants_without_a_multi_filter_form_raise(gpu_device):
    import torch
    n = 5001
    ix = make_index(corpus(n, 384), gpu_device)
    q = torch.from_numpy(osearch.synth_unit_rows(2, 384, 1)).to(gpu_device)
    mf, _ = multi_filter(layout("mod4", n), [0, 1], gpu_device)
    for kw in ({"sq8": True}, {"band": (0.1, 0.9)}, {"mmr": (20, 0.5)}):
        with pytest.raises(ValueError, match="per-query filters"):
            ix.search(q, 10, filt=mf, **kw)
    with pytest.raises(ValueError, match="per-query filters"):
        ix.search(q[:1], 10, filt=mf)   # built for two queries


# ---- 6. rejected rows never appear -------------------------------------------------------------------
@pytest.mark.parametrize("n", [5001, 100_003])
def test_rows_of_the_other_filter_that_outscore_every_passing_row_never_appear(gpu_device, n):
    c16 = corpus(n, 384)
    r = np.arange(n)
    masks = [r % 2 == 0, r % 2 == 1]   # complementary
    # each query IS a row of the other filter: its best row overall (itself, score 1) is rejected
    rows = np.arange(40) * max(1, n // 40)
    q16 = c16[rows]
    qf = [1 - int(x % 2) for x in rows]
    assert all(not masks[g][x] for g, x in zip(qf, rows))
    check_multi(make_index(c16, gpu_device), q16, c16, masks, qf, 10, gpu_device)


# ---- 7. overflow ladder -----------------------------------------------------------------------------
def test_duplicate_rows_flag_and_the_ladder_answers_each_query_over_its_own_set(gpu_device):
    import torch
    n, d, k = 100_003, 384, 10
    c16 = corpus(n, d).copy()
    c16[:20_000] = c16[0]          # 20 000 identical rows: ties overflow the candidate lists
    masks = [np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)]
    masks[0][:20_000] = True
    masks[0][50_000:50_100] = True
    masks[1][5_000:25_000] = True
    masks[1][60_000:60_100] = True
    q16 = np.concatenate([c16[:1], c16[:1], osearch.synth_unit_rows(4, d, 10)])
    qf = [0, 1, 0, 1, 0, 1]
    ix = make_index(c16, gpu_device)
    _, _, flags = check_multi(ix, q16, c16, masks, qf, k, gpu_device, raw=False)
    assert flags[0] != 0 and flags[1] != 0
    # the same through the store: the two sets as two scalar columns, one expression per query
    from rag_fin_amd.store import CorpusStore
    st = CorpusStore("dups", dim=d, capacity=n, device=gpu_device)
    st.add([f"k{i}" for i in range(n)], ["t"] * n, torch.from_numpy(c16).to(gpu_device),
           np.where(masks[0], "A", "B").tolist(), np.where(masks[1], "x", "y").tolist(), ["s"] * n, [0.0] * n)
    exprs = ['period == "A"', 'chunk_type == "x"']
    res = st.search(torch.from_numpy(q16).to(gpu_device), limit=k, expr=[exprs[g] for g in qf])
    es, ei = expected(q16, c16, masks, qf, k)
    for b, hits in enumerate(res):
        assert [h.row for h in hits] == ei[b].tolist(), b
        assert [h.score for h in hits] == [float(np.float32(s)) for s in es[b]], b


# ---- 8. near ties ------------------------------------------------------------------------------------
def test_a_near_tie_cluster_split_across_two_interleaved_filters(gpu_device):
    n, d, k, m = 20_011, 384, 10, 97
    qc, rows = adv.near_tie_cluster(d, m, 0)
    c16, pos = adv.embed_clusters(n, d, 1234, [rows], stride=adv.scatter_stride(n, m))
    r = np.arange(n)
    masks = [r % 2 == 0, r % 2 == 1]
    q16 = np.concatenate([np.stack([qc, qc]), osearch.synth_unit_rows(6, d, 1235)])
    qf = [0, 1, 0, 1, 0, 1, 0, 1]
    es, ei = expected(q16, c16, masks, qf, k + 1)
    for b in (0, 1):   # the cut at rank k falls inside the cluster for both filters
        assert ei[b, k - 1] in pos[0] and ei[b, k] in pos[0]
    check_multi(make_index(c16, gpu_device), q16, c16, masks, qf, k, gpu_device, want=(es[:, :k], ei[:, :k]))


# ---- 9. store level ----------------------------------------------------------------------------------
def hit_bits(res):
    return [[(h.row, h.id, h.score) for h in hits] for hits in res]


def test_store_search_with_an_expr_list_equals_one_call_per_query(gpu_device, monkeypatch):
    st, chunks, emb = golden_store(gpu_device)
    st.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
    periods = sorted({c["period"] for c in chunks})
    exprs = [f'period == "{p}"' for p in periods] + [None, 'TEXT_MATCH(text, "profit")', "",
                                                      f'period == "{periods[0]}" and primary_value > 0']
    B = 130   # three sweeps: the queries are ordered by filter inside and come back in the caller's order
    rng = np.random.default_rng(3)
    picks = rng.integers(len(exprs), size=B)
    lst = [exprs[j] for j in picks]
    q = rng.normal(size=(B, 384)).astype(np.float32)
    built = []
    real = st.build_filter
    monkeypatch.setattr(st, "build_filter", lambda e: built.append(e) or real(e))
    res = st.search(q, "embedding", {"metric_type": "COSINE"}, 5, expr=lst, output_fields=["period"])
    assert sorted(built) == sorted({e for e in lst if e}), "every distinct expression is built once"
    assert len(res) == B
    for b in range(B):
        one = st.search(q[b:b + 1], "embedding", {"metric_type": "COSINE"}, 5, expr=lst[b], output_fields=["period"])
        assert hit_bits([res[b]]) == hit_bits(one), (b, lst[b])
        assert [h.entity.period for h in res[b]] == [h.entity.period for h in one[0]]
    assert hit_bits(st.search(q, limit=5, expr=lst)) == hit_bits(res)   # a second run: bit-identical
    # a list of one distinct expression is the string call
    same = st.search(q[:9], limit=5, expr=[exprs[0]] * 9)
    assert hit_bits(same) == hit_bits(st.search(q[:9], limit=5, expr=exprs[0]))
    with pytest.raises(ValueError):
        st.search(q[:2], limit=5, expr=[exprs[0], "period >"])


# ---- 10. threads -------------------------------------------------------------------------------------
def test_two_threads_with_different_filter_lists(gpu_device):
    import torch
    n = 100_003
    c16 = corpus(n, 384)
    ix = make_index(c16, gpu_device)
    q16 = osearch.synth_unit_rows(16, 384, 13)
    cases = [(layout("quarters", n), [b % 4 for b in range(16)]), (layout("mod4", n), [(b * 3) % 4 for b in range(16)])]
    want = [expected(q16, c16, m, qf, 10) for m, qf in cases]
    errors = []

    def work(j):
        try:
            torch.cuda.set_device(gpu_device)
            mf, _ = multi_filter(cases[j][0], cases[j][1], gpu_device)
            q = torch.from_numpy(q16).to(gpu_device)
            for _ in range(5):
                _, ids, exact = ix.search(q, 10, want_exact=True, filt=mf)
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
