"""GPU tests of late interaction: rf_encode_tokens, rf_maxsim and rf_maxsim_topk through
rag_fin_amd.late_interaction, the store's "token_embeddings" field and VectorRAG's rerank_with="late".

Token vectors are judged by tolerance against the fp64 numpy mirror tokens_reference (pinned to transformers in
tests/test_late_interaction_cpu.py), evaluated on the SAME fp16-rounded weights; seeded random weights.
TOL = 3 x the largest |component - mirror| measured on the MI355X over the parity shapes below
(profiles/late_interaction_measurements.jsonl), the margin rule of tests/test_sparse_encoder_gpu.py; and,
independently of that measurement, every similarity formed from GPU vectors lies within 1e-3 of the mirror's.

MaxSim is judged against maxsim_reference on the SAME fp16 inputs by a bound that needs no measurement:
q_len (2 D + q_len) 2^-24 x 1.01 -- D fp32 accumulation roundings per similarity (operands of norm <= 1 + 2^-10),
doubled for the MFMA's internal order, plus the q_len-term sum.  Selection and search are judged exactly."""
import functools

import numpy as np
import pytest

from test_late_interaction_cpu import l2_model

pytestmark = pytest.mark.gpu
TOL = 1.37e-3         # 3 x the 4.57e-4 measured (64 x 128, D = 32; the other shapes and widths: 1.6e-4 .. 2.9e-4)
SIM_TOL = 1e-3        # the project's bound on a cosine score
DIMS = [32, 96, 128]


def _fused_lens():
    lens = np.random.default_rng(64).integers(40, 129, 64)
    lens[0] = 128
    return lens


# name -> (T, lens)
SHAPES = {
    "one_16": (16, [16]),                                # a single short row: the one-launch QKV + attention path
    "ragged_7x40": (40, [40, 17, 1, 33, 0, 29, 5]),      # lengths 1 and 0; packed blocks shared by rows
    "fused_64x128": (128, _fused_lens()),                # >= 8192 token slots: the fused layer path
}
SKIP_EVERY = 7        # the test's skiplist: every id that is a multiple of 7


@functools.lru_cache(maxsize=None)
def case(name):
    T, lens = SHAPES[name]
    cfg = l2_model()[0]
    rng = np.random.default_rng(T)
    # (padding slots carry random ids too: what they hold must not matter)
    return rng.integers(1, cfg["vocab_size"], (len(lens), T)).astype(np.int32), np.asarray(lens, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def skip_bits():
    V = l2_model()[0]["vocab_size"]
    bits = np.zeros((V + 31) // 32, dtype=np.uint32)
    for i in range(0, V, SKIP_EVERY):
        bits[i >> 5] |= np.uint32(1 << (i & 31))
    return bits


@functools.lru_cache(maxsize=None)
def hidden(name):
    """The mirror's last hidden state of a parity case, computed once and shared by the three projections."""
    from rag_fin_amd.sparse_encoder import hidden_reference
    cfg, _, w16 = l2_model()
    ids, lens = case(name)
    h = hidden_reference(w16, cfg, ids, lens)
    h.setflags(write=False)
    return h


def projection(dim):
    from rag_fin_amd.late_interaction import random_projection
    cfg = l2_model()[0]
    p = random_projection(cfg, 5, dim)
    return p, p.astype(np.float16).astype(np.float32)


@pytest.fixture(scope="module")
def encoders(gpu_device):
    import torch
    from rag_fin_amd.late_interaction import ColBERT
    made = {}

    def get(dim):
        if dim not in made:
            cfg, w, _ = l2_model()
            col = ColBERT(w, projection(dim)[0], cfg, device=gpu_device)
            col._skip = torch.from_numpy(skip_bits().view(np.int32)).to(gpu_device)   # documents drop the test's skiplist
            made[dim] = col
        return made[dim]
    return get


def rows_of(off, vec):
    off = off.cpu().numpy()
    vec = vec.cpu().numpy()
    return off, [vec[off[b]:off[b + 1]] for b in range(off.size - 1)]


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_token_vectors_match_the_mirror(encoders, name, dim):
    from conftest import record_measurement
    from rag_fin_amd.late_interaction import tokens_reference
    cfg, _, w16 = l2_model()
    ids, lens = case(name)
    off, got = rows_of(*encoders(dim).encode_ids(ids, lens, is_query=False))
    want = tokens_reference(w16, projection(dim)[1], cfg, ids, lens, skip=skip_bits(), hidden=hidden(name))
    # the offsets are the numpy count, exactly; dropped ids are absent; a row with lens < 1 is empty
    keep = (np.arange(ids.shape[1])[None, :] < lens[:, None]) & (ids % SKIP_EVERY != 0)
    assert off.dtype == np.int32 and np.array_equal(off, np.concatenate([[0], np.cumsum(keep.sum(axis=1))]))
    assert (~keep & (np.arange(ids.shape[1])[None, :] < lens[:, None])).any()            # the skiplist is exercised
    for b in np.flatnonzero(lens < 1):
        assert got[b].shape[0] == 0
    g = np.concatenate(got).astype(np.float64)
    m = np.concatenate(want)
    assert g.shape == m.shape and got[0].dtype == np.float16 and np.isfinite(g).all()
    err = float(np.abs(g - m).max())
    norm_err = float(np.abs(np.linalg.norm(g, axis=1) - 1.0).max())
    q = g[:32]                                          # similarities of the first tokens with every token
    sim_err = float(np.abs(q @ g.T - m[:32] @ m.T).max())
    record_measurement(f"late_interaction_{name}_d{dim}", max_abs_component=err, max_abs_similarity=sim_err,
                       max_norm_error=norm_err)
    print(f"late_interaction_{name}_d{dim}: max |component - mirror| = {err:.3e}, max |similarity - mirror| = "
          f"{sim_err:.3e}, max | |v| - 1 | = {norm_err:.3e}")
    assert norm_err <= 2.0 ** -10, norm_err
    assert sim_err <= SIM_TOL, sim_err
    assert err < TOL, err


def test_queries_keep_every_token(encoders):
    ids, lens = case("ragged_7x40")
    off, _ = rows_of(*encoders(96).encode_ids(ids, lens, is_query=True))
    assert np.array_equal(np.diff(off), np.clip(lens, 0, None))


def test_same_row_same_bits_anywhere_in_the_batch_and_across_calls(encoders):
    col = encoders(96)
    ids, lens = case("ragged_7x40")
    _, a = rows_of(*col.encode_ids(ids, lens))
    _, b = rows_of(*col.encode_ids(ids, lens))
    assert all(np.array_equal(x.view(np.uint16), y.view(np.uint16)) for x, y in zip(a, b))
    for seed in (0, 1):
        perm = np.random.default_rng(seed).permutation(7)
        _, p = rows_of(*col.encode_ids(ids[perm], lens[perm]))
        for j, src in enumerate(perm):
            assert np.array_equal(p[j].view(np.uint16), a[src].view(np.uint16)), (seed, j)
    assert len({r.tobytes() for r in a}) == 7 and a[0].any()


# ---- rf_maxsim ------------------------------------------------------------------------------------------------------
COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 200]
Q_LENS = [32, 7, 0, 1, 31]
N_ROWS = 300


def unit_rows(rng, n, dim):
    v = rng.standard_normal((n, dim))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float16)


@functools.lru_cache(maxsize=None)
def maxsim_case(dim):
    """docs: a list of N_ROWS float16 [n_tok, dim] arrays; queries: 64 float16 [q_len, dim] arrays.
    Query 0 has 32 tokens with sixteen entries of +-1/4 each -- exactly unit vectors in fp16; query 1 has 7 tokens
    close to one direction.  Rows 1..4 are crafted around them."""
    rng = np.random.default_rng(dim)
    q_lens = [Q_LENS[b % len(Q_LENS)] for b in range(64)]
    queries = [unit_rows(rng, n, dim) for n in q_lens]
    q0 = np.zeros((32, dim), dtype=np.float16)
    for i in range(32):
        q0[i, rng.choice(dim, 16, replace=False)] = rng.choice([-0.25, 0.25], 16)
    queries[0] = q0
    u = rng.standard_normal(dim)
    q1 = u[None, :] + 0.1 * rng.standard_normal((7, dim))
    queries[1] = (q1 / np.linalg.norm(q1, axis=1, keepdims=True)).astype(np.float16)
    counts = [COUNTS[(r * 4 + r // 9) % len(COUNTS)] for r in range(N_ROWS)]
    counts[:5] = [33, 7, 65, 65, 32]
    docs = [unit_rows(rng, n, dim) for n in counts]
    docs[1] = -queries[1]                               # every similarity with query 1 is negative
    docs[2][0] = q0[0]                                  # the best token of query 0's first token comes first ...
    docs[3][64] = q0[0]                                 # ... or last, alone in the row's third tile
    docs[4] = q0.copy()                                 # the query itself
    return docs, queries


def bound(q_len, dim):
    return max(q_len, 1) * (2 * dim + max(q_len, 1)) * 2.0 ** -24 * 1.01


def device_field(docs, dim, device):
    from rag_fin_amd.late_interaction import TokenField
    return TokenField.from_rows(docs, dim, device)


def packed(queries, dim, fill):
    from rag_fin_amd.late_interaction import pack_queries
    q_vec, q_len = pack_queries(queries, dim)
    for b, n in enumerate(q_len):
        q_vec[b, n:] = fill
    return q_vec, q_len


def bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("dim", DIMS)
def test_maxsim_equals_the_definition_in_every_mode(gpu_device, dim):
    from rag_fin_amd.index import filter_from_mask
    from rag_fin_amd.late_interaction import maxsim, maxsim_reference
    import torch
    docs, queries = maxsim_case(dim)
    field = device_field(docs, dim, gpu_device)
    starts = field.off_host[:-1]
    assert (starts % 32 != 0).sum() > N_ROWS // 2 and set(np.diff(field.off_host).tolist()) == set(COUNTS + [7])
    want = maxsim_reference(docs, queries)
    # the crafted rows are what they claim to be
    assert ((queries[1].astype(np.float64) @ docs[1].astype(np.float64).T) < 0).all() and want[1, 1] < 0
    sims = queries[0][:1].astype(np.float64) @ docs[2].astype(np.float64).T
    assert sims.argmax() == 0 and (queries[0][:1].astype(np.float64) @ docs[3].astype(np.float64).T).argmax() == 64
    assert want[0, 4] == 32.0
    tol = np.array([bound(q.shape[0], dim) for q in queries])[:, None]
    full = None
    for B in (64, 3, 1):
        got = maxsim(field, packed(queries[:B], dim, np.nan))               # slots >= q_len hold NaN ...
        zero = maxsim(field, packed(queries[:B], dim, 0.0))                 # ... and change no bit
        assert got.shape == (B, N_ROWS) and np.array_equal(bits(got), bits(zero))
        g = got.cpu().numpy().astype(np.float64)
        w = want[:B]
        assert np.array_equal(np.isneginf(g), np.isneginf(w)) and not np.isnan(g).any()
        hit = ~np.isneginf(w)
        assert (np.abs(np.where(hit, g - np.where(hit, w, 0.0), 0.0)) <= tol[:B]).all()
        if full is None:
            full = got
        else:
            assert np.array_equal(bits(got), bits(full[:B]))                # the same bits at any batch size
    g = full.cpu().numpy()
    assert np.isneginf(g[2]).all() and np.isneginf(g[:, np.diff(field.off_host) == 0]).all()
    assert g[1, 1] < 0 and abs(float(g[0, 4]) - 32.0) <= bound(32, dim)
    # candidate mode: ragged lists, a repeated row, an empty list, rows outside the collection
    rng = np.random.default_rng(1)
    cands = [rng.integers(0, N_ROWS, int(n)).tolist() for n in rng.integers(1, 40, 64)]
    cands[0] = [4, 2, 3, 4, 1, 4]
    cands[5] = []
    cands[6] = [7, N_ROWS, 8, -1, 2 ** 40]
    flat = maxsim(field, packed(queries, dim, np.nan), cands)
    assert flat.shape == (sum(len(c) for c in cands),)
    flat_bits, at = bits(flat), 0
    full_bits = bits(full)
    for b, c in enumerate(cands):
        for r in c:
            if 0 <= r < N_ROWS:
                assert flat_bits[at] == full_bits[b, r], (b, r)
            else:
                assert flat_bits[at] == np.float32(-np.inf).view(np.uint32), (b, r)
            at += 1
    # alone in a call
    for b, r in ((0, 4), (1, 1), (4, 8), (63, 299)):
        alone = maxsim(field, packed(queries[b:b + 1], dim, np.nan), [[r]])
        assert bits(alone)[0] == full_bits[b, r]
        alone = maxsim(device_field(docs[r:r + 1], dim, gpu_device), packed(queries[b:b + 1], dim, 0.0))
        assert bits(alone)[0, 0] == full_bits[b, r]
    # a filter that passes about half the rows
    mask = np.random.default_rng(2).random(N_ROWS) < 0.5
    words = np.packbits(np.concatenate([mask, np.zeros(-N_ROWS % 32, bool)]), bitorder="little").view(np.int32)
    filt = filter_from_mask(torch.from_numpy(words.copy()).to(gpu_device), N_ROWS)
    f = bits(maxsim(field, packed(queries, dim, np.nan), filter=filt))
    ninf = np.float32(-np.inf).view(np.uint32)
    assert np.array_equal(f[:, mask], full_bits[:, mask]) and (f[:, ~mask] == ninf).all()
    fc = bits(maxsim(field, packed(queries[:1], dim, 0.0), [list(range(N_ROWS))], filter=filt))
    assert np.array_equal(fc, f[0])


# ---- rf_maxsim_topk -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 64])
def test_topk_equals_the_definition_exactly(gpu_device, k):
    import torch
    from rag_fin_amd.late_interaction import maxsim_topk, topk_reference
    rng = np.random.default_rng(k)
    sizes = [0, 1, 63, 64, 65, 100_000, 1000, 300]
    segs = []
    for n in sizes:
        s = (rng.integers(-40, 40, n) / 8.0).astype(np.float32)             # few distinct values: ties at every cut
        s[rng.random(n) < 0.2] = -np.inf
        segs.append(s)
    segs[6][:] = -np.inf                                                    # more -inf entries than hits: padding
    segs[6][[3, 500, 999, 17, 18]] = [1.5, 1.5, -2.0, 0.0, 1.5]
    segs[7] = rng.standard_normal(300).astype(np.float32)                   # distinct values, both signs
    segs[7][[10, 20]] = segs[7].max() + 1.0                                 # duplicates at the top: the lower row first
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    scores = torch.from_numpy(np.concatenate(segs)).to(gpu_device)
    rows = np.concatenate([rng.permutation(n) + 1000 for n in sizes]).astype(np.int64)
    for given, id_base in ((None, 0), (None, 5000), (rows, 0)):
        got_s, got_i, exact = maxsim_topk(scores, off, k, rows=given, id_base=id_base, want_exact=True)
        got_s, got_i, exact = got_s.cpu().numpy(), got_i.cpu().numpy(), exact.cpu().numpy()
        for b, s in enumerate(segs):
            r = None if given is None else [given[off[b]:off[b + 1]]]
            want_s, want_i = topk_reference(s, k, rows=r, id_base=id_base)
            assert np.array_equal(got_i[b], want_i[0]), (b, id_base)
            assert np.array_equal(got_s[b].view(np.uint32), want_s[0].view(np.uint32)), b
            assert np.array_equal(exact[b], want_s[0].astype(np.float64))
    want_i = topk_reference(segs[6], k)[1][0]
    assert want_i[:min(k, 3)].tolist() == [3, 18, 500][:min(k, 3)] and (k < 10 or want_i[5] == -1)
    assert topk_reference(segs[7], 2)[1][0].tolist() == [10, 20]


# ---- the store's token field ----------------------------------------------------------------------------------------
FIELD = "token_embeddings"
SPEC = {"index_type": "EMB_LIST_FLAT", "metric_type": "MAX_SIM_IP"}
MS = {"metric_type": "MAX_SIM_IP"}
PERIODS = ["Q1_FY2024", "Q2_FY2024", "Q3_FY2024", "Q4_FY2024"]
N0, N_ADD = 300, 7


@pytest.fixture(scope="module")
def corpus(gpu_device):
    from oracle import synth_text
    from rag_fin_amd.late_interaction import ColBERT
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    cfg, w, _ = l2_model()
    tok = WordPieceTokenizer(synth_text.vocab_for(size=cfg["vocab_size"]))
    col = ColBERT(w, projection(96)[0], cfg, tokenizer=tok, device=gpu_device, settings={"document_length": 64})
    texts = synth_text.retemplated_texts(N0 + N_ADD, 41)
    rng = np.random.default_rng(7)
    vec = rng.standard_normal((N0 + N_ADD, 384)).astype(np.float32)
    return dict(enc=col, texts=texts, vec=vec, queries=synth_text.retemplated_texts(5, 42),
                periods=[PERIODS[i % 4] for i in range(N0 + N_ADD)], device=gpu_device)


def make_store(c, rows):
    from rag_fin_amd.store import CorpusStore
    st = CorpusStore("t", dim=384, capacity=512, device=c["device"])
    rows = list(rows)
    st.add([f"c{i}" for i in rows], [c["texts"][i] for i in rows], c["vec"][rows], [c["periods"][i] for i in rows],
           ["t"] * len(rows), ["s"] * len(rows), [float(i) for i in rows])
    st.create_index(FIELD, SPEC, encoder=c["enc"])
    return st


def check_against_the_definition(st, c, limit, expr=None, mask=None):
    from rag_fin_amd import late_interaction as late
    hits = st.search(c["queries"], FIELD, MS, limit, expr=expr, output_fields=["period"])
    q = c["enc"].encode(c["queries"], is_query=True)
    assert all(v.shape == (32, 96) for v in q)                              # expanded to 32 tokens
    n = st.num_entities
    field = st._text_fields[FIELD].index()
    filt = None if expr is None else st.build_filter(expr)
    scores = late.maxsim(field, q, filter=filt).cpu().numpy()
    want_s, want_i = late.topk_reference(scores, limit)
    ref = late.maxsim_reference(st.token_vectors(range(n)), q, mask=mask)
    for b in range(5):
        m = int((want_i[b] >= 0).sum())
        assert m == min(limit, n if mask is None else int(mask.sum()))
        assert [h.row for h in hits[b]] == want_i[b, :m].tolist()
        got = np.array([h.score for h in hits[b]], dtype=np.float32)
        assert np.array_equal(got.view(np.uint32), want_s[b, :m].view(np.uint32))
        assert (np.abs(got.astype(np.float64) - ref[b, want_i[b, :m]]) <= bound(32, 96)).all()
    return hits


def test_store_search_equals_the_definition_with_and_without_a_filter(corpus):
    st = make_store(corpus, range(N0))
    hits = check_against_the_definition(st, corpus, 10)
    vecs = st.token_vectors(range(N0))
    assert len(vecs) == N0 and all(v.dtype == np.float16 and v.shape[1] == 96 and 3 <= v.shape[0] <= 64 for v in vecs)
    mask = np.array([p == "Q2_FY2024" for p in corpus["periods"][:N0]])
    filtered = check_against_the_definition(st, corpus, 10, expr='period == "Q2_FY2024"', mask=mask)
    assert all(h.entity.period == "Q2_FY2024" for q in filtered for h in q) and all(len(q) == 10 for q in filtered)
    assert [h.row for h in hits[0]] != [h.row for h in filtered[0]]
    # supplied token vectors: the first query's own
    q0 = corpus["enc"].encode(corpus["queries"][:1], is_query=True)
    by_vec = st.search(q0, FIELD, MS, 10)
    assert [h.row for h in by_vec[0]] == [h.row for h in st.search(corpus["queries"][:1], FIELD, MS, 10)[0]]


def test_store_after_add_and_delete_answers_as_a_fresh_store(corpus):
    c = corpus
    st = make_store(c, range(N0))
    st.search(c["queries"], FIELD, MS, 10)
    new = list(range(N0, N0 + N_ADD))
    st.add([f"c{i}" for i in new], [c["texts"][i] for i in new], c["vec"][new], [c["periods"][i] for i in new],
           ["t"] * N_ADD, ["s"] * N_ADD, [float(i) for i in new])
    st.search(c["queries"], FIELD, MS, 10)                            # encodes the 7 new rows alone
    assert st.delete('period == "Q3_FY2024"').delete_count > 0
    survivors = [i for i in range(N0 + N_ADD) if c["periods"][i] != "Q3_FY2024"]
    fresh = make_store(c, survivors)
    got = check_against_the_definition(st, c, 10)
    want = check_against_the_definition(fresh, c, 10)
    assert [[(h.id, h.score) for h in q] for q in got] == [[(h.id, h.score) for h in q] for q in want]
    a, b = st._text_fields[FIELD].index(), fresh._text_fields[FIELD].index()
    assert np.array_equal(a.off_host, b.off_host) and a.n_rows == len(survivors)
    assert np.array_equal(a.off[:a.n_rows + 1].cpu().numpy(), a.off_host)
    assert np.array_equal(a.vec[:a.n_tok].cpu().numpy().view(np.uint16), b.vec[:b.n_tok].cpu().numpy().view(np.uint16))


def test_hybrid_of_a_dense_and_a_token_arm_is_the_rrf_of_the_two_lists(corpus):
    from rag_fin_amd import lexical
    from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
    c = corpus
    st = make_store(c, range(N0))
    qv = c["vec"][[3, 50, 99, 200, 299]] + 0.5 * c["vec"][[4, 51, 100, 201, 0]]
    dense = st.search(qv, "embedding", {"metric_type": "COSINE"}, 12)
    late = st.search(c["queries"], FIELD, MS, 9)
    got = st.hybrid_search([AnnSearchRequest(qv, "embedding", {"metric_type": "COSINE"}, 12),
                            AnnSearchRequest(c["queries"], FIELD, MS, 9)], RRFRanker(), 10)
    pad = lambda hits: [h.row for h in hits] + [-1] * (12 - len(hits))   # noqa: E731
    arms = np.array([[pad(q) for q in dense], [pad(q) for q in late]])
    _, want, fused = lexical.rrf_reference(arms, 10)
    for b in range(5):
        n = int((want[b] >= 0).sum())
        assert [h.row for h in got[b]] == want[b, :n].tolist()
        assert [h.score for h in got[b]] == fused[b, :n].tolist()


def test_a_four_arm_hybrid_search_equals_a_fresh_store_after_a_delete_and_an_append(corpus):
    """The dense field and the three fields derived from the text column on ONE store of 70 rows (a filter mask of
    three 32-bit words, the last one partial): 2 queries, 8 hits per arm, one arm with an expr, the best 5 fused.
    As built, after a delete of 7 rows (row 0, the last row, both sides of a mask word) and after an append of 5
    the hits -- rows, primary keys, fused scores -- are bit for bit those of a fresh store of the surviving rows."""
    from oracle import synth_text
    from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
    from rag_fin_amd.sparse_encoder import SparseEncoder
    from rag_fin_amd.store import CorpusStore
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    from test_sparse_encoder_cpu import model
    c = corpus
    cfg, _, w, head, _, _ = model("l2")
    splade = SparseEncoder(w, head, cfg, tokenizer=WordPieceTokenizer(synth_text.vocab_for(size=cfg["vocab_size"])),
                           device=c["device"], max_seq_length=64, max_terms=48, query_max_terms=24)

    def add(st, rows):
        st.add([f"c{i}" for i in rows], [c["texts"][i] for i in rows], c["vec"][rows], [c["periods"][i] for i in rows],
               ["t"] * len(rows), ["s"] * len(rows), [float(i) for i in rows])

    def store_of(rows):
        st = CorpusStore("t", dim=384, capacity=128, device=c["device"])
        add(st, rows)
        st.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
        st.create_index("sparse_embedding", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "IP"}, encoder=splade)
        st.create_index(FIELD, SPEC, encoder=c["enc"])
        return st

    words = [" ".join(q.split()[:8]) for q in c["queries"][:2]]              # (a BM25 query holds at most 64 terms)
    qv = c["vec"][[3, 50]] + 0.5 * c["vec"][[4, 51]]

    def ask(st):
        reqs = [AnnSearchRequest(qv, "embedding", {"metric_type": "COSINE"}, 8),
                AnnSearchRequest(words, "sparse", {"metric_type": "BM25"}, 8),
                AnnSearchRequest(words, "sparse_embedding", {"metric_type": "IP"}, 8, expr='period != "Q3_FY2024"'),
                AnnSearchRequest(words, FIELD, MS, 8)]
        hits = st.hybrid_search(reqs, RRFRanker(), 5)
        assert [len(q) for q in hits] == [5, 5]
        return [[(h.row, h.id, np.float64(h.score).tobytes()) for h in q] for q in hits]

    rows = list(range(70))
    st = store_of(rows)
    assert ask(st) == ask(store_of(rows))                                      # as built
    gone = [0, 13, 31, 32, 63, 64, 69]
    assert st.delete("id in [" + ", ".join(f'"c{i}"' for i in gone) + "]").delete_count == 7
    rows = [i for i in rows if i not in gone]
    assert st.num_entities == 63 and ask(st) == ask(store_of(rows))
    new = list(range(70, 75))
    add(st, new)
    rows += new
    assert st.num_entities == 68 and ask(st) == ask(store_of(rows))


class RowEmbedder:
    """Stands in for the sentence embedder: a text's vector is the corpus vector of its row (queries: of a row
    close to it)."""
    dim = 384

    def __init__(self, c):
        self.c = c

    def encode(self, texts):
        return np.stack([self.c["vec"][(7 * self.c["queries"].index(t)) % N0] + 0.5 * self.c["vec"][3] for t in texts])


def test_vector_rag_reranks_by_maxsim_of_the_stored_token_vectors(corpus):
    from rag_fin_amd import late_interaction as late
    from rag_fin_amd.rag import VectorRAG
    c = corpus
    st = make_store(c, range(N0))
    st.drop_index(field_name=FIELD)
    rag = VectorRAG("k", embedder=RowEmbedder(c), store=st, late_encoder=c["enc"])
    assert st.has_index(field_name=FIELD)
    per_query = [rag.search(q, 5, rerank=True, rerank_with="late", fetch_k=24) for q in c["queries"]]
    batch = rag.search_batch(c["queries"], 5, rerank=True, rerank_with="late", fetch_k=24)
    assert batch == per_query
    field = st._text_fields[FIELD].index()
    for b, query in enumerate(c["queries"]):
        fetched = st.search(RowEmbedder(c).encode([query]), "embedding", {"metric_type": "COSINE"}, 24,
                            output_fields=["text"])[0]
        rows = [h.row for h in fetched]
        s = late.maxsim(field, c["enc"].encode([query], is_query=True), [rows]).cpu().numpy()
        order = sorted(range(24), key=lambda i: (-float(s[i]), i))[:5]
        assert [x["text"] for x in per_query[b]] == [fetched[i].entity.text for i in order]
        assert [np.float32(x["rerank_score"]).view(np.uint32) for x in per_query[b]] == [s[i].view(np.uint32) for i in order]
        assert [x["score"] for x in per_query[b]] == [float(fetched[i].score) for i in order]
        assert [x["rank"] for x in per_query[b]] == [1, 2, 3, 4, 5]
    with pytest.raises(ValueError, match="late encoder"):
        VectorRAG("k", embedder=RowEmbedder(c), store=make_store(c, range(8))).search("q", 3, rerank=True, rerank_with="late")


def test_rank_orders_documents_by_maxsim(corpus):
    c = corpus
    docs = c["texts"][:70]
    ranked = c["enc"].rank(c["queries"][0], docs, top_k=5)
    everything = c["enc"].rank(c["queries"][0], docs)
    assert len(everything) == 70 and ranked == everything[:5]
    assert [r["score"] for r in everything] == sorted((r["score"] for r in everything), reverse=True)
    assert sorted(r["corpus_id"] for r in everything) == list(range(70))


# ---- refusals at the C boundary -------------------------------------------------------------------------------------
def test_unsupported_and_invalid_calls_are_refused(gpu_device):
    import ctypes
    import torch
    from oracle import encoder as oenc
    from rag_fin_amd import _lib
    from rag_fin_amd.late_interaction import ColBERT, TokenField, maxsim, random_projection
    cfg = dict(oenc.MINILM_L6, layers=1, vocab_size=100, max_position=32)
    col = ColBERT(oenc.random_weights(cfg, 1), random_projection(cfg, 1, 32), cfg, device=gpu_device)
    with pytest.raises(_lib.RagfinError) as e:                        # T > max_position
        col.encode_ids(np.ones((1, 33), np.int32), np.array([8], np.int32))
    assert e.value.code == -2 and "max_position" in str(e.value)
    lib, h = col.lib, col.encoder.handle
    ids = torch.ones((1, 8), dtype=torch.int32, device=gpu_device)
    lens = torch.full((1,), 8, dtype=torch.int32, device=gpu_device)
    off = torch.empty(2, dtype=torch.int32, device=gpu_device)
    vec = torch.empty((8, 32), dtype=torch.float16, device=gpu_device)
    need = lib.rf_encode_tokens_workspace_bytes(h, 1, 8)
    assert need == lib.rf_encode_workspace_bytes(h, 1, 8) and lib.rf_encode_tokens_workspace_bytes(h, 0, 8) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def call(head, nbytes=need, B=1, T=8):
        return lib.rf_encode_tokens(h, p(ids), p(lens), B, T, ctypes.byref(head), p(off), p(vec), p(ws), nbytes,
                                    _lib.current_stream_ptr())
    head = lambda **kw: _lib.TokenHead(**dict(dict(proj_w=col._proj.data_ptr(), dim=32, skip=None, vocab=100), **kw))   # noqa: E731
    assert call(head()) == 0
    for bad, code, word in ((head(dim=24), -2, "dim"), (head(dim=144), -2, "dim"), (head(dim=0), -2, "dim"),
                            (head(vocab=99), -2, "vocab"), (head(proj_w=col._proj.data_ptr() + 2), -1, "misaligned"),
                            (head(proj_w=None), -1, "null")):
        assert call(bad) == code
        assert word in lib.rf_last_error().decode()
    assert call(head(), B=0) == -1 and call(head(), T=0) == -1
    assert call(head(), nbytes=need - 1) == -3 and "workspace" in lib.rf_last_error().decode()
    # rf_maxsim / rf_maxsim_topk
    field = TokenField.from_rows([np.ones((3, 32), np.float16)], 32, gpu_device)
    q = torch.zeros((1, 32, 32), dtype=torch.float16, device=gpu_device)
    ql = torch.ones(1, dtype=torch.int32, device=gpu_device)
    out = torch.empty(4, dtype=torch.float32, device=gpu_device)

    def score(f, B=1, qv=q):
        return lib.rf_maxsim(ctypes.byref(f), p(qv) if qv is not None else None, p(ql), B, None, None, None, p(out),
                             _lib.current_stream_ptr())
    assert score(field.struct()) == 0
    f = field.struct()
    f.dim = 24
    assert score(f) == -2 and "dim" in lib.rf_last_error().decode()
    f.dim = 144
    assert score(f) == -2
    assert score(field.struct(), B=0) == -1 and score(field.struct(), qv=None) == -1
    f = field.struct()
    f.vec += 2
    assert score(f) == -1 and "misaligned" in lib.rf_last_error().decode()
    with pytest.raises(ValueError):
        maxsim(field, [np.ones((33, 32), np.float16)])                # more than 32 query tokens
    with pytest.raises(ValueError):
        maxsim(field, [np.ones((3, 16), np.float16)])                 # another width
    seg = torch.tensor([0, 4], dtype=torch.int64, device=gpu_device)
    so = torch.empty(64, dtype=torch.float32, device=gpu_device)
    io = torch.empty(64, dtype=torch.int64, device=gpu_device)
    for B, k in ((0, 4), (1, 0), (1, 65)):
        assert lib.rf_maxsim_topk(p(out), p(seg), None, B, k, 0, p(so), p(io), None, _lib.current_stream_ptr()) == -1
    assert lib.rf_maxsim_topk(None, p(seg), None, 1, 4, 0, p(so), p(io), None, _lib.current_stream_ptr()) == -1


def test_store_refuses_what_the_token_field_has_no_form_for_on_the_device(corpus):
    from rag_fin_amd.ranker import BoostRanker
    st = make_store(corpus, range(40))
    q = corpus["queries"][:1]
    for kw in (dict(param={"metric_type": "IP"}), dict(limit=65), dict(param=dict(MS, params={"radius": 0.1})),
               dict(offset=1), dict(group_by_field="period"), dict(mmr_lambda=0.5), dict(expr=['period == "Q1_FY2024"']),
               dict(ranker=BoostRanker('period == "Q1_FY2024"', 2.0)),
               dict(data=np.ones((1, 384), np.float32)), dict(data=[np.ones((33, 96), np.float16)]),
               dict(data=[np.ones((4, 32), np.float16)])):
        args = dict(data=q, anns_field=FIELD, param=MS, limit=3)
        args.update(kw)
        with pytest.raises(ValueError, match="token_embeddings"):
            st.search(**args)
    with pytest.raises(ValueError, match="token_embeddings"):
        st.search_iterator(np.ones((1, 384), np.float32), FIELD, MS)
    st.drop_index(field_name=FIELD)
    with pytest.raises(ValueError, match="token_embeddings"):
        st.search(q, FIELD, MS, 3)
