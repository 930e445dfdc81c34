"""Lexical index maintenance on the GPU: rf_sparse_append, rf_sparse_compact_plan /
_apply and rf_sparse_impacts through SparseIndex.appended / .compacted, bit for bit against the numpy
definitions (lexical.append_reference / compact_reference) on synthetic posting arrays whose shapes
aim at the chunk edges of the kernels; then a live CorpusStore through a sequence of adds, upserts and
deletes against a store built fresh from the surviving rows after every step."""
import functools

import numpy as np
import pytest

from oracle import synth_text
from rag_fin_amd import _lib, lexical

pytestmark = pytest.mark.gpu

CHUNK = _lib.RF_LEX_CHUNK
PARAMS = [(1.2, 0.75), (0.0, 0.75), (1.2, 0.0), (1.2, 1.0)]


# ---- synthetic postings: exact shapes, no text -------------------------------------------------------------
def synth_counts(seed, n_rows, dfs, max_tf=1, name="t{:07d}".format):
    """TermCounts over n_rows rows: term i has dfs[i] postings (random distinct rows; all rows when df =
    n_rows), tf in 1..max_tf, and tf ascending positions per posting."""
    rng = np.random.default_rng(seed)
    dfs = np.asarray(dfs, dtype=np.int64)
    post_off = np.zeros(dfs.size + 1, dtype=np.int64)
    np.cumsum(dfs, out=post_off[1:])
    rows = np.empty(int(post_off[-1]), dtype=np.int64)
    one = np.flatnonzero(dfs == 1)
    rows[post_off[one]] = rng.integers(0, max(n_rows, 1), one.size)
    for t in np.flatnonzero(dfs > 1).tolist():
        d = int(dfs[t])
        rows[post_off[t]:post_off[t + 1]] = np.arange(n_rows) if d == n_rows else np.sort(rng.choice(n_rows, d, replace=False))
    tf = rng.integers(1, max_tf + 1, rows.size).astype(np.uint32)
    dl = np.bincount(rows, weights=tf, minlength=n_rows).astype(np.int64)
    pos_off = np.zeros(rows.size + 1, dtype=np.int64)
    np.cumsum(tf, out=pos_off[1:])
    step = rng.integers(1, 4, int(pos_off[-1]))
    run = np.cumsum(step)
    first = pos_off[:-1]
    pos = (run - np.repeat(run[first] - step[first], tf)).astype(np.uint32) if rows.size else np.zeros(0, dtype=np.uint32)
    return lexical.TermCounts([name(i) for i in range(dfs.size)], post_off, rows.astype(np.uint32), tf, dl, pos_off, pos)


def as_postings(c, k1=1.2, b=0.75):
    return lexical.rescored(c.vocab, c.post_off, c.post_row, c.post_tf, c.dl, k1, b), (c.pos_off, c.pos)


def on_device(device, p, positions, with_positions):
    from rag_fin_amd.index import SparseIndex
    sp = SparseIndex(p, device)
    assert sp.supports_update
    if with_positions:
        sp.attach_positions(*positions)
    return sp


def assert_device_equals(sp, want, want_pos):
    assert (sp.n_rows, sp.n_terms, sp.nnz) == (want.n_rows, want.n_terms, want.nnz)
    assert np.array_equal(sp.post_off.cpu().numpy(), want.post_off)
    assert np.array_equal(sp.host_array("post_row"), want.post_row)
    assert np.array_equal(sp.host_array("post_tf"), want.post_tf)
    assert np.array_equal(sp.dl.cpu().numpy(), want.dl)
    got, ref = sp.host_array("post_imp").view(np.uint32), want.post_imp.view(np.uint32)
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {ref.size} impacts differ"
    if want_pos is None:
        assert sp.positions is None
    else:
        assert np.array_equal(sp.positions[0].cpu().numpy(), want_pos[0])
        assert np.array_equal(sp.positions[1].cpu().numpy().view(np.uint32), want_pos[1])


def check_append(sp, p, positions, delta):
    want, want_pos = lexical.append_reference(p, positions if sp.positions is not None else None, delta)
    vocab, map_old, map_delta = lexical.merge_vocab(p.vocab, p.term_id, delta.vocab)
    post_off = lexical.merged_offsets(len(vocab), p.post_off, map_old, delta.post_off, map_delta)
    new = sp.appended(delta, map_old, map_delta, post_off, np.concatenate([p.dl, delta.dl]), p.k1, p.b)
    assert new is not sp and vocab == want.vocab
    assert_device_equals(new, want, want_pos)
    return new, want, want_pos


def check_compact(sp, p, positions, keep):
    want, want_pos = lexical.compact_reference(p, positions if sp.positions is not None else None, keep)
    row_map = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    new, alive, post_off = sp.compacted(row_map, p.dl[keep], p.k1, p.b)
    assert [t for t, a in zip(p.vocab, alive.tolist()) if a] == want.vocab
    assert np.array_equal(post_off, want.post_off)
    assert new is not sp
    assert_device_equals(new, want, want_pos)
    return new, want, want_pos


# ---- chunk edges -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nnz", [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1])
def test_a_single_term_at_the_chunk_edges(gpu_device, nnz):
    c = synth_counts(nnz, nnz, [nnz], max_tf=3)
    p, positions = as_postings(c)
    for with_positions in (False, True):
        sp = on_device(gpu_device, p, positions, with_positions)
        rng = np.random.default_rng(nnz)
        for keep in (rng.random(nnz) > 0.3, np.arange(nnz) != 0, np.arange(nnz) != nnz - 1, np.ones(nnz, dtype=bool),
                     np.arange(nnz) == nnz // 2):
            check_compact(sp, p, positions, keep)
        # the same term again, and a term on either side of it
        for names, dfs in (([c.vocab[0]], [5]), (["a", c.vocab[0], "z"], [2, 3, 1]), (["a"], [CHUNK + 3])):
            delta = synth_counts(nnz + 1, CHUNK + 3, dfs, max_tf=2, name=lambda i, names=names: names[i])
            check_append(sp, p, positions, delta)


def test_one_long_term_beside_tens_of_thousands_of_single_postings(gpu_device):
    n = 12 * CHUNK + 17
    long_t = 14000
    dfs = [1] * long_t + [9 * CHUNK + 5] + [1] * 16001 + [n // 3, 1, 1]
    c = synth_counts(5, n, dfs, max_tf=4)
    p, positions = as_postings(c)
    sp = on_device(gpu_device, p, positions, True)
    keep = np.random.default_rng(6).random(n) > 0.5
    new, want, want_pos = check_compact(sp, p, positions, keep)
    assert want.n_terms < p.n_terms                                   # single postings died: the ids moved
    # new terms before, between and after the old ones, old terms again; and rows without a posting
    names = sorted(["a0", "a1", p.vocab[7], p.vocab[long_t], p.vocab[-1], "t0007000x", "t0014000x", "z0", "z1"])
    delta = synth_counts(7, 300, [3, 1, 200, 1, 40, 250, 1, 2, 299], max_tf=3, name=lambda i: names[i])
    for state in ((sp, p, positions), (new, want, want_pos)):
        check_append(*state, delta)
    # every row of the longest term goes: it vanishes, everything after it moves down
    gone = np.zeros(n, dtype=bool)
    gone[p.post_row[p.post_off[long_t]:p.post_off[long_t + 1]]] = True
    assert 0 < (~gone).sum() < n
    _, want, _ = check_compact(sp, p, positions, ~gone)
    assert p.vocab[long_t] not in want.term_id and want.term_id[p.vocab[-3]] < p.term_id[p.vocab[-3]] - 1
    only = np.zeros(n, dtype=bool)
    only[p.post_row[p.post_off[long_t]]] = True
    check_compact(sp, p, positions, only)                             # all rows but one go


def test_the_second_scan_level_crosses_its_own_chunk_edge(gpu_device):
    """More than RF_LEX_CHUNK chunks: the workgroup that scans the chunk sums takes a second tile."""
    n = 350 * CHUNK + 5
    c = synth_counts(11, n, [n, n // 2, n, 3, n // 2 + 9], max_tf=2)
    assert c.nnz > CHUNK * CHUNK + CHUNK
    p, positions = as_postings(c)
    sp = on_device(gpu_device, p, positions, True)
    keep = np.random.default_rng(12).random(n) > 0.4
    keep[:3 * CHUNK] = False                                          # whole chunks without a kept posting
    new, want, want_pos = check_compact(sp, p, positions, keep)
    delta = synth_counts(13, 2 * CHUNK, [2 * CHUNK, 1, CHUNK, 7], max_tf=2,
                         name=lambda i: ["a", p.vocab[1], p.vocab[3], "z"][i])
    check_append(new, want, want_pos, delta)


def test_deltas_without_new_terms_and_without_tokens(gpu_device):
    c = synth_counts(21, 500, [500, 1, 40, 250, 1, 1, 77], max_tf=5)
    p, positions = as_postings(c)
    for with_positions in (False, True):
        sp = on_device(gpu_device, p, positions, with_positions)
        same_terms = synth_counts(22, 64, [64, 3, 9], max_tf=5, name=lambda i: [p.vocab[0], p.vocab[2], p.vocab[6]][i])
        new, want, want_pos = check_append(sp, p, positions, same_terms)
        assert want.vocab == p.vocab
        no_tokens = lexical.count_terms(["", "  ", ""])
        assert no_tokens.nnz == 0 and no_tokens.vocab == []
        new, want, want_pos = check_append(new, want, want_pos, no_tokens)
        assert want.n_rows == 500 + 64 + 3 and want.dl[-3:].tolist() == [0, 0, 0]
        keep = np.ones(want.n_rows, dtype=bool)
        keep[0] = keep[-1] = False
        check_compact(new, want, want_pos, keep)


@pytest.mark.parametrize("k1,b", PARAMS)
def test_impacts_bits_at_the_parameter_edges(gpu_device, k1, b):
    c = synth_counts(31, 3 * CHUNK + 11, [3 * CHUNK + 11, 1, 2 * CHUNK, 1, 1, 5, CHUNK + 1], max_tf=40)
    p, positions = as_postings(c, k1, b)
    sp = on_device(gpu_device, p, positions, False)
    keep = np.random.default_rng(32).random(p.n_rows) > 0.2
    new, want, _ = check_compact(sp, p, positions, keep)
    df = np.diff(want.post_off)
    ref = lexical.impacts(want.post_tf, want.dl[want.post_row.astype(np.int64)], np.repeat(df, df), want.n_rows, want.avgdl, k1, b)
    assert np.array_equal(new.host_array("post_imp").view(np.uint32), ref.view(np.uint32))
    delta = synth_counts(33, 100, [100, 31, 2], max_tf=40, name=lambda i: ["a", want.vocab[0], "z"][i])
    check_append(new, want, None, delta)


# ---- the store ---------------------------------------------------------------------------------------------
N0, DIM = 2000, 64
COS = {"metric_type": "COSINE"}
BM25 = {"metric_type": "BM25"}
SPARSE = {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"}
QTEXTS = ["total deposits of the bank", "net profit after tax, net profit", "provision coverage ratio 7"]
FILTERS = ['TEXT_MATCH(text, "deposits")', 'PHRASE_MATCH(text, "net profit")',
           'TEXT_MATCH(text, "profit tax capital", minimum_should_match=2) and not PHRASE_MATCH(text, "of the")']


@functools.lru_cache(maxsize=None)
def corpus():
    texts = synth_text.retemplated_texts(N0 + 400, 17)
    rng = np.random.default_rng(18)
    x = rng.standard_normal((len(texts), DIM))
    v16 = np.ascontiguousarray((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16))
    v16.setflags(write=False)
    return texts, v16


@functools.lru_cache(maxsize=None)
def tokens(text):
    return tuple(lexical.basic_tokens(text))


def analyze_once(texts):
    """lexical.analyze, each distinct text tokenised once per session: the fresh stores of every step
    analyse the same strings again and again."""
    return [list(tokens(t)) for t in texts]


class Recording:
    def __init__(self):
        self.calls = []

    def __call__(self, texts):
        self.calls.append(len(texts))
        return analyze_once(texts)


def build_store(device, rows, analyzer=None):
    """A store over `rows`: (key, text number) pairs in row order."""
    import torch
    from rag_fin_amd.store import CorpusStore
    texts, v16 = corpus()
    st = CorpusStore("u", dim=DIM, capacity=N0 + 400, device=device)
    st.analyzer = analyzer or analyze_once
    idx = [i for _, i in rows]
    st.add([k for k, _ in rows], [texts[i] for i in idx], torch.from_numpy(v16[idx]).to(device), [f"P{i % 5}" for i in idx],
           ["t"] * len(idx), ["s"] * len(idx), [float(i) for i in idx])
    st.create_index("sparse", SPARSE)
    return st


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


def assert_same_index(live, fresh):
    (lp, ls), (fp, fs) = live._lexical.built, fresh._lexical.built
    assert lp.vocab == fp.vocab and lp.term_id == fp.term_id
    assert np.array_equal(lp.post_off, fp.post_off) and np.array_equal(lp.dl, fp.dl)
    for name in ("post_off", "post_row", "post_imp"):
        a, b = getattr(ls, name).cpu().numpy(), getattr(fs, name).cpu().numpy()
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    assert np.array_equal(lp.post_row, fp.post_row) and np.array_equal(lp.post_imp.view(np.uint32), fp.post_imp.view(np.uint32))
    assert ls.positions is not None and fs.positions is not None
    for a, b in zip(ls.positions, fs.positions):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_a_live_store_equals_a_fresh_one_after_every_step(gpu_device):
    import torch
    texts, v16 = corpus()
    rec = Recording()
    rows = [(f"k{i}", i) for i in range(N0)]
    live = build_store(gpu_device, rows, rec)
    fresh = build_store(gpu_device, rows)
    assert answers(live, gpu_device) == answers(fresh, gpu_device)      # (the phrase filters attached the positions)
    first = live._lexical.built[1]
    assert first.positions is not None and first.supports_update
    rng = np.random.default_rng(19)
    spare = list(range(N0, N0 + 400))

    def batch(keys, idx):
        return [keys, [texts[i] for i in idx], torch.from_numpy(v16[idx]).to(gpu_device), [f"P{i % 5}" for i in idx],
                ["t"] * len(idx), ["s"] * len(idx), [float(i) for i in idx]]

    for step in range(10):
        rec.calls.clear()
        kind = ["add", "upsert", "delete", "word", "upsert", "add", "delete", "upsert", "add", "delete"][step]
        n_new = 0
        if kind == "add":
            idx = [spare.pop() for _ in range(16)]
            keys = [f"n{i}" for i in idx]
            live.insert(batch(keys, idx))
            rows = rows + list(zip(keys, idx))
            n_new = 16
        elif kind == "upsert":                                          # eight restated rows and eight new ones
            idx = [spare.pop() for _ in range(16)]
            old = [rows[i][0] for i in rng.choice(len(rows), 8, replace=False).tolist()]
            keys = old + [f"n{i}" for i in idx[8:]]
            assert live.upsert(batch(keys, idx)).upsert_count == 16
            rows = [r for r in rows if r[0] not in set(old)] + list(zip(keys, idx))
            n_new = 16
        elif kind == "delete":
            period = f"P{step % 5}"
            want = [k for k, i in rows if i % 5 == step % 5]
            assert live.delete(f'period == "{period}"').delete_count == len(want) > 0
            rows = [r for r in rows if r[1] % 5 != step % 5]
        else:                                                           # every row holding a word: the term leaves the dictionary
            expr = 'TEXT_MATCH(text, "deposits")'
            assert "deposits" in live._lexical.built[0].term_id
            a, b = live.delete(expr), fresh.delete(expr)
            assert a.delete_count == b.delete_count > 0 and list(a.primary_keys) == list(b.primary_keys)
            gone = set(a.primary_keys)
            rows = [r for r in rows if r[0] not in gone]
            rec.calls.clear()                                           # (the expression's own terms were analysed)
        assert live._lexical.built is None
        fresh = build_store(gpu_device, rows)
        assert answers(live, gpu_device) == answers(fresh, gpu_device)
        assert live.columns["id"] == [k for k, _ in rows]
        assert_same_index(live, fresh)
        assert live._lexical.built[1] is not first and live._lexical.built[1].n_rows == len(rows)
        if kind == "word":
            assert "deposits" not in live._lexical.built[0].term_id
        # the analyzer saw the new rows once, then queries and filter strings: never the surviving rows
        assert rec.calls[0] == (n_new or rec.calls[0]) and max(rec.calls[1:] + [0]) <= len(QTEXTS)
        assert sum(rec.calls) < len(rows) // 4
