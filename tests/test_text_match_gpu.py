"""Keyword filters on the GPU: rf_text_match against lexical.text_match_reference bit for bit, and
TEXT_MATCH / PHRASE_MATCH through CorpusStore against the per-row definition on strings (the AST's
eval) -- as a filter of filter_rows / query, of the dense search (CPU oracle over exactly the passing
rows), of the BM25 search (bm25_reference with the same mask) and of delete.

One corpus of 2 * 8192 + 37 rows (three row tiles of the kernel, the last one partial, and no
multiple of 32), dim 64, texts drawn from 300 words with a Zipf weight, plus planted rows:
  "everywhere"   in every row
  "cornerstone"  in exactly rows 0, 8191, 8192 and N - 1 (both sides of a tile edge, the last row)
  "alpha beta gamma"  at the very start of row 100 and the very end of row 9000; in row 200 after an
                 "alpha" that "beta" does not follow; row 300 holds the three words in another order"""
import functools

import numpy as np
import pytest

from oracle import c_oracle
from rag_fin_amd import _lib, filter_expr as fe, lexical

pytestmark = pytest.mark.gpu

N, DIM = 2 * 8192 + 37, 64
WORDS = (N + 31) // 32
PERIODS = ["Q1_FY2023", "Q2_FY2023", "Q3_FY2023", "Q4_FY2023", "Q1_FY2024"]
SPARSE = {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"}
CORNER = (0, 8191, 8192, N - 1)
M, P = _lib.RF_TEXT_MATCH, _lib.RF_TEXT_PHRASE


@functools.lru_cache(maxsize=None)
def data():
    rng = np.random.default_rng(2024)
    vocab = [f"w{i}" for i in range(300)]
    p = 1.0 / np.arange(1, len(vocab) + 1)
    p /= p.sum()
    lens = rng.integers(1, 24, N)
    draws = rng.choice(len(vocab), size=int(lens.sum()), p=p)
    texts, at = [], 0
    for ln in lens.tolist():
        texts.append("everywhere " + " ".join(vocab[i] for i in draws[at:at + ln]))
        at += ln
    for r in CORNER:
        texts[r] += " cornerstone"
    texts[100] = "alpha beta gamma " + texts[100]
    texts[9000] = texts[9000] + " alpha beta gamma"
    texts[200] = "everywhere alpha w3 beta alpha alpha beta gamma w1"
    texts[300] = "everywhere gamma beta alpha w0 beta gamma"
    x = rng.standard_normal((N, DIM))
    c16 = np.ascontiguousarray((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16))
    xq = rng.standard_normal((4, DIM))
    q16 = np.ascontiguousarray((xq / np.linalg.norm(xq, axis=1, keepdims=True)).astype(np.float16))
    periods = [PERIODS[i % len(PERIODS)] for i in range(N)]
    postings = lexical.build_postings(texts)
    positions = lexical.build_positions(postings, texts)
    c16.setflags(write=False)
    return texts, periods, c16, q16, postings, positions


def make_store(device):
    import torch
    from rag_fin_amd.store import CorpusStore
    texts, periods, c16, _, _, _ = data()
    st = CorpusStore("t", dim=DIM, capacity=N, device=device)
    st.add([f"k{i}" for i in range(N)], texts, torch.from_numpy(c16).to(device), periods, ["t"] * N, ["s"] * N,
           [float(i) for i in range(N)])
    st.create_index("sparse", SPARSE)
    return st


_STORE = {}


def store(device):
    """The shared, unmodified store (the delete test makes its own)."""
    if "st" not in _STORE:
        _STORE["st"] = make_store(device)
    return _STORE["st"]


def expected_mask(expr):
    texts, periods = data()[:2]
    node = fe.parse(expr)
    return np.array([node.eval({"text": t, "period": p, "id": f"k{i}", "primary_value": float(i)})
                     for i, (t, p) in enumerate(zip(texts, periods))], dtype=bool)


def ids(*terms):
    tid = data()[4].term_id
    return [tid[t] for t in terms]


# ---- the kernel against its definition ---------------------------------------------------------------------
def run_text_match(device, leaves):
    import torch
    from rag_fin_amd.store import SparseIndex
    postings, positions = data()[4:]
    if "sp" not in _STORE:
        sp = SparseIndex(postings, device)
        sp.attach_positions(*positions)
        _STORE["sp"] = sp
    out = _STORE["sp"].text_match(leaves)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert got.shape == (len(leaves), (WORDS + 3) // 4 * 4)
    return got


def check_leaves(device, leaves):
    postings, positions = data()[4:]
    got = run_text_match(device, leaves)
    want = lexical.text_match_reference(postings, positions, leaves, N)
    assert want.shape == (len(leaves), WORDS)
    for l, leaf in enumerate(leaves):
        assert np.array_equal(got[l, :WORDS], want[l]), (leaf, np.flatnonzero(got[l, :WORDS] != want[l])[:8])
    assert not got[:, WORDS:].any()   # the pad words are written, and zero
    return want


def rows_of(words):
    return np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")[:N])


def test_match_leaves_equal_the_definition(gpu_device):
    three = sorted(ids("w0", "w5", "w40"))
    leaves = [(M, ids("everywhere"), 1), (M, ids("cornerstone"), 1), (M, ids("w299"), 1),
              (M, three, 1), (M, three, 2), (M, three, 3), (M, three, 4),
              (M, sorted(ids(*[f"w{i}" for i in range(64)])), 10),
              (M, [len(data()[4].vocab) + 5], 1)]   # an id outside the dictionary: no postings
    want = check_leaves(gpu_device, leaves)
    assert rows_of(want[0]).size == N and rows_of(want[1]).tolist() == list(CORNER)
    assert 0 < rows_of(want[5]).size < rows_of(want[4]).size < rows_of(want[3]).size < N
    assert rows_of(want[6]).size == 0 and rows_of(want[8]).size == 0 and rows_of(want[7]).size > 0


def test_phrase_leaves_equal_the_definition(gpu_device):
    leaves = [(P, ids("alpha", "beta", "gamma"), 1), (P, ids("gamma", "beta", "alpha"), 1), (P, ids("beta", "alpha"), 1),
              (P, ids("alpha", "alpha", "beta"), 1), (P, ids("w0", "w1"), 1), (P, ids("w1", "w0"), 1),
              (P, ids("w0", "w0"), 1), (P, ids("w0", "w1", "w0"), 1), (P, ids("everywhere", "w0"), 1),
              (P, ids("cornerstone"), 1), (P, ids("w0", "cornerstone"), 1),
              (P, ids("everywhere") + [-3], 1)]
    want = check_leaves(gpu_device, leaves)
    assert rows_of(want[0]).tolist() == [100, 200, 9000]      # the start of a row, a false start first, the end of a row
    assert rows_of(want[1]).tolist() == [300] and rows_of(want[2]).tolist() == [200, 300]
    assert rows_of(want[3]).tolist() == [200]
    assert rows_of(want[4]).size > 100 and not np.array_equal(want[4], want[5]) and rows_of(want[6]).size > 100
    assert rows_of(want[9]).tolist() == list(CORNER) and rows_of(want[11]).size == 0


def test_sixteen_leaves_in_one_call_and_the_same_bytes_twice(gpu_device):
    three = sorted(ids("w1", "w2", "w3"))
    leaves = [(M, three, 1), (P, ids("w1", "w2"), 1), (M, three, 3), (P, ids("alpha", "beta", "gamma"), 1),
              (M, ids("cornerstone"), 1), (P, ids("w2", "w1", "w3"), 1), (M, three, 4), (M, ids("everywhere"), 1)] * 2
    assert len(leaves) == _lib.RF_TEXT_MAX_LEAVES
    want = check_leaves(gpu_device, leaves)
    assert np.array_equal(want[:8], want[8:])
    a = run_text_match(gpu_device, leaves)
    b = run_text_match(gpu_device, leaves)
    assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError):
        _STORE["sp"].text_match(leaves + leaves[:1])


# ---- through the store -------------------------------------------------------------------------------------
EXPRS = [
    'TEXT_MATCH(text, "cornerstone")',
    'PHRASE_MATCH(text, "alpha beta gamma")',
    'not TEXT_MATCH(text, "w0 w1 w2", minimum_should_match=2)',
    'TEXT_MATCH(text, "w7") and period == "Q1_FY2024"',
    'PHRASE_MATCH(text, "w0 w1") or TEXT_MATCH(text, "cornerstone nosuchword")',
    'not (PHRASE_MATCH(text, "w0 w0") or period in ["Q2_FY2023", "Q3_FY2023"]) and TEXT_MATCH(text, "W1, w2!")',
    'id in ["k100", "k200", "k300", "k301"] and not PHRASE_MATCH(text, "gamma beta")',
    'TEXT_MATCH(text, "nosuchword") or primary_value < 40 and TEXT_MATCH(text, "w0")',
    'PHRASE_MATCH(text, "beta nosuchword") or PHRASE_MATCH(text, "everywhere alpha")',
]


def defined_parts(buf):
    """(header, row mask, the n_pass_blocks valid entries of the block list) of a filter buffer; what
    lies behind the valid entries is scratch (include/ragfin.h, "filtered search")."""
    raw = buf.cpu().numpy().view(np.uint32)
    a = (WORDS * 4 + 15) // 16 * 16 // 4
    return raw[:3].tolist(), raw[4:4 + WORDS].tobytes(), raw[4 + a:4 + a + int(raw[2])].tobytes()


@pytest.mark.parametrize("expr", EXPRS)
def test_filter_rows_equal_the_per_row_definition(gpu_device, expr):
    st = store(gpu_device)
    want = expected_mask(expr)
    got = st.filter_rows(expr)
    assert got.tolist() == np.flatnonzero(want).tolist()
    # a second identical call: the same bytes in every defined part of the filter buffer
    a, b = defined_parts(st.build_filter(expr)), defined_parts(st.build_filter(expr))
    assert a == b and a[0][1] == int(want.sum())


def test_query_returns_the_passing_rows(gpu_device):
    st = store(gpu_device)
    got = st.query(expr='PHRASE_MATCH(text, "alpha beta gamma")', output_fields=["id"])
    assert [r["id"] for r in got] == ["k100", "k200", "k9000"]


def test_dense_search_among_the_passing_rows(gpu_device):
    import torch
    st = store(gpu_device)
    _, _, c16, q16, _, _ = data()
    for expr, k in (('TEXT_MATCH(text, "w7 w9", minimum_should_match=2)', 10), ('PHRASE_MATCH(text, "w0 w1")', 10),
                    ('TEXT_MATCH(text, "cornerstone")', 10), ('PHRASE_MATCH(text, "alpha beta gamma") and period == "Q1_FY2023"', 5)):
        S = np.flatnonzero(expected_mask(expr))
        assert S.size > 0
        es, ei = c_oracle.search(q16, c16[S], min(k, S.size))
        res = st.search(torch.from_numpy(q16), "embedding", {"metric_type": "COSINE"}, k, expr=expr)
        for b, hits in enumerate(res):
            assert [h.row for h in hits] == S[ei[b]].tolist(), expr
            assert [np.float32(h.score) for h in hits] == es[b].astype(np.float32).tolist(), expr


def test_bm25_search_among_the_passing_rows(gpu_device):
    st = store(gpu_device)
    postings = data()[4]
    queries = ["w3 w8 cornerstone", "alpha gamma", "w0"]
    for expr in ('PHRASE_MATCH(text, "w0 w1")', 'not TEXT_MATCH(text, "w3") and period == "Q4_FY2023"'):
        mask = expected_mask(expr)
        q_off, q_term, q_weight = lexical.encode_queries(postings, queries)
        ws, wi, _ = lexical.bm25_reference(postings, q_off, q_term, q_weight, 10, mask=mask)
        res = st.search(queries, "sparse", {"metric_type": "BM25"}, 10, expr=expr)
        for b, hits in enumerate(res):
            assert [h.row for h in hits] == [r for r in wi[b].tolist() if r >= 0], expr
            assert [np.float32(h.score) for h in hits] == [s for s, r in zip(ws[b].tolist(), wi[b].tolist()) if r >= 0]


def test_delete_by_phrase_and_the_rebuilt_index(gpu_device):
    st = make_store(gpu_device)
    texts = data()[0]
    assert st.filter_rows('PHRASE_MATCH(text, "alpha beta gamma")').tolist() == [100, 200, 9000]
    res = st.delete('PHRASE_MATCH(text, "alpha beta gamma")')
    assert res.delete_count == 3 and sorted(res.primary_keys) == ["k100", "k200", "k9000"]
    assert st.num_entities == N - 3
    assert st.filter_rows('PHRASE_MATCH(text, "alpha beta gamma")').size == 0
    kept = [t for i, t in enumerate(texts) if i not in (100, 200, 9000)]
    for expr in ('TEXT_MATCH(text, "alpha gamma")', 'PHRASE_MATCH(text, "gamma beta alpha")', 'TEXT_MATCH(text, "cornerstone")',
                 'PHRASE_MATCH(text, "w0 w1")'):
        node = fe.parse(expr)
        want = [i for i, t in enumerate(kept) if node.eval({"text": t})]
        assert st.filter_rows(expr).tolist() == want, expr
    assert st.filter_rows('TEXT_MATCH(text, "cornerstone")').tolist() == [0, 8189, 8190, N - 4]   # two rows went before them


def test_a_declared_index_without_postings_passes_no_row(gpu_device):
    import torch
    from rag_fin_amd.store import CorpusStore
    st = CorpusStore("e", dim=DIM, capacity=8, device=gpu_device)
    st.add(["a", "b"], ["", "  "], torch.from_numpy(np.array(data()[2][:2])).to(gpu_device), ["p", "p"], ["t"] * 2, ["s"] * 2,
           [0.0, 1.0])
    with pytest.raises(ValueError, match=r"create_index\('sparse'"):
        st.filter_rows('TEXT_MATCH(text, "w0")')
    st.create_index("sparse", SPARSE)
    assert st.filter_rows('TEXT_MATCH(text, "w0") or PHRASE_MATCH(text, "w0 w1")').size == 0
    assert st.filter_rows('not TEXT_MATCH(text, "w0")').tolist() == [0, 1]
