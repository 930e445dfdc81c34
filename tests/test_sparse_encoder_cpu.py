"""Learned sparse search, the parts that need no GPU:
  * terms_reference (the fp64 numpy definition of rf_encode_terms) pinned to the in-container
    transformers.BertForMaskedLM + log1p(relu) + masked max, through the state-dict mapping the product loads
    checkpoints with (tied and untied decoder);
  * the parity cases tests/test_sparse_encoder_gpu.py runs, and the condition their bias is chosen for;
  * sparsify_reference and sparse_ip_reference on hand-made cases;
  * the store's surface with a fake encoder, the lexical= forwarding of VectorRAG, the tool and the REST body;
  * the ABI."""
import functools

import numpy as np
import pytest

from oracle import encoder as oenc
from rag_fin_amd import mcp_server
from rag_fin_amd.sparse_encoder import (TermPostings, check_query_rows, hidden_reference, random_mlm_head,
                                        sparse_ip_reference, sparsify_reference, stack_hf_mlm_head, terms_reference)

# ---- the parity cases (shared with the GPU tests) ------------------------------------------------------------------
CFG2 = dict(oenc.MINILM_L6, layers=2, vocab_size=2005)
CFG6 = dict(oenc.MINILM_L6)          # six layers, the full vocabulary of 30 522
BIAS = -1.0                          # decoder bias N(-1, 1): see test_between_10_and_90_percent_of_the_mirror_is_zero
SEED2, SEED6 = 5, 6


@functools.lru_cache(maxsize=None)
def model(which: str):
    """(cfg, seed, fp32 weights, fp32 head, fp16-rounded weights, fp16-rounded head): both sides from the seed."""
    cfg, seed = (CFG2, SEED2) if which == "l2" else (CFG6, SEED6)
    w = oenc.random_weights(cfg, seed)
    head = random_mlm_head(cfg, seed, bias=BIAS)
    return cfg, seed, w, head, oenc.round_weights_fp16(w), oenc.round_weights_fp16(head)


def _rows(seed, lens, T, vocab):
    rng = np.random.default_rng(seed)
    # (padding slots carry random ids too: what they hold must not matter)
    return rng.integers(1, vocab, (len(lens), T)).astype(np.int32), np.asarray(lens, dtype=np.int32)


def _fused_lens():
    lens = np.random.default_rng(64).integers(40, 129, 64)
    lens[0] = 128
    return lens


# name -> (model, T, lens)
SHAPES = {
    "one_24": ("l2", 24, [24]),                          # a single short row: the one-launch QKV + attention path
    "ragged_5x96": ("l2", 96, [96, 70, 64, 33, 1]),      # a packed 32-token block holds the end of a row and the start of the next
    "long_2x300": ("l2", 300, [300, 257]),               # T > 256: the vector-ALU attention
    "fused_64x128": ("l2", 128, _fused_lens()),          # >= 8192 token slots: k_linear_dma + k_post_block
    "vocab_30522": ("l6", 40, [40, 17, 33]),             # the tail tile (30 522 = 119 x 256 + 58) and term ids past 2^15
    "empty_row_3x20": ("l2", 20, [20, 0, 13]),           # a row with lens 0
}


def case(name):
    """-> (model key, ids int32 [B, T], lens int32 [B])"""
    which, T, lens = SHAPES[name]
    ids, lens = _rows(T, lens, T, model(which)[0]["vocab_size"])
    return which, ids, lens


@functools.lru_cache(maxsize=None)
def mirror(name) -> np.ndarray:
    """terms_reference of a parity case on the fp16-rounded weights, fp64 [B, V]; computed once, read-only."""
    which, ids, lens = case(name)
    cfg, _, _, _, w16, head16 = model(which)
    out = terms_reference(w16, head16, cfg, ids, lens)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_between_10_and_90_percent_of_the_mirror_is_zero(name):
    """The bias is chosen so that the parity shapes test both branches of relu: neither nearly all weights zero
    nor nearly none (logits of standard deviation ~1, maxima over 1 .. 300 tokens of ~0 .. 3)."""
    want = mirror(name)
    zero = float((want == 0).mean())
    print(f"{name}: {zero:.3f} of the mirror's weights are zero, max {want.max():.3f}")
    assert 0.10 <= zero <= 0.90, zero
    assert np.isfinite(want).all() and want.min() >= 0
    _, _, lens = case(name)
    for b in np.flatnonzero(lens < 1):
        assert not want[b].any()


def test_hidden_reference_is_the_encoder_oracle():
    cfg = dict(oenc.MINILM_L6, layers=2, vocab_size=300, max_position=40)
    w = oenc.random_weights(cfg, 4)
    ids = np.random.default_rng(0).integers(1, 300, (3, 17))
    lens = np.array([17, 5, 1])
    assert np.array_equal(hidden_reference(w, cfg, ids, lens), oenc.encode(w, cfg, ids, lens, return_hidden=True))


# ---- the definition against transformers ----------------------------------------------------------------------------
@pytest.mark.parametrize("tied", [True, False])
def test_terms_reference_and_state_dict_mapping_match_transformers(tied):
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    from rag_fin_amd.embedder import stack_hf_state_dict
    cfg = dict(oenc.MINILM_L6, layers=2, vocab_size=211, max_position=48)
    torch.manual_seed(11)
    hc = transformers.BertConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"],
                                 num_attention_heads=cfg["heads"], intermediate_size=cfg["intermediate"],
                                 max_position_embeddings=cfg["max_position"], type_vocab_size=2, hidden_act="gelu",
                                 hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                 layer_norm_eps=cfg["ln_eps"], tie_word_embeddings=tied)
    m = transformers.BertForMaskedLM(hc)
    with torch.no_grad():   # the default init leaves biases at 0 and LayerNorm at (1, 0): move them
        for name, p in m.named_parameters():
            if name.endswith("bias") or "LayerNorm" in name:
                p.add_(0.1 * torch.randn_like(p))
            if name.startswith("cls.predictions.decoder.weight") or "word_embeddings" in name:
                p.mul_(4.0)   # logits of standard deviation ~1: both branches of relu
    m = m.double().eval()
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    if tied:   # what a checkpoint saved with tied embeddings holds: no decoder matrix (and no alias of the bias)
        assert np.array_equal(sd["cls.predictions.decoder.weight"], sd["bert.embeddings.word_embeddings.weight"])
        sd.pop("cls.predictions.decoder.weight")
        sd.pop("cls.predictions.decoder.bias", None)
    else:
        assert not np.array_equal(sd["cls.predictions.decoder.weight"], sd["bert.embeddings.word_embeddings.weight"])
        sd.pop("cls.predictions.bias", None)   # the bias under its other name
    w, head = stack_hf_state_dict(sd, cfg), stack_hf_mlm_head(sd)
    assert head["dec_w"].shape == (211, 384) and head["dec_b"].shape == (211,) and head["tr_w"].shape == (384, 384)
    assert np.array_equal(head["dec_w"], w["word_emb"]) == tied
    rng = np.random.default_rng(1)
    B, T = 5, 33
    lens = np.array([33, 20, 9, 1, 12])
    ids = rng.integers(1, cfg["vocab_size"], (B, T))
    att = (np.arange(T)[None, :] < lens[:, None]).astype(np.int64)
    with torch.no_grad():
        logits = m(input_ids=torch.as_tensor(ids), attention_mask=torch.as_tensor(att)).logits
        want = torch.max(torch.log1p(torch.relu(logits)) * torch.as_tensor(att)[:, :, None], dim=1).values.numpy()
    got = terms_reference(w, head, cfg, ids, lens)
    assert got.shape == want.shape == (B, 211)
    assert 0.1 < (want == 0).mean() < 0.9
    assert np.abs(got - want).max() < 1e-9, np.abs(got - want).max()


def test_mlm_head_mapping_refuses_a_plain_bert_model():
    sd = {"embeddings.word_embeddings.weight": np.zeros((5, 384), np.float32),
          "pooler.dense.weight": np.zeros((384, 384), np.float32)}
    with pytest.raises(KeyError, match="cls.predictions.transform.dense.weight"):
        stack_hf_mlm_head(sd)
    full = {"cls.predictions.transform.dense.weight": 0, "cls.predictions.transform.dense.bias": 0,
            "cls.predictions.transform.LayerNorm.weight": 0, "cls.predictions.transform.LayerNorm.bias": 0,
            "bert.embeddings.word_embeddings.weight": 0}
    with pytest.raises(KeyError, match="cls.predictions.bias"):
        stack_hf_mlm_head(full)


# ---- selection and scoring definitions ------------------------------------------------------------------------------
def test_sparsify_reference_by_hand():
    w = np.zeros((4, 8), dtype=np.float32)
    w[0, [1, 4, 6]] = [0.5, 2.0, 1.0]
    w[1] = 1.0                                    # all equal: the lowest ids win
    w[2, [0, 3, 5, 7]] = [1.0, 3.0, 1.0, 2.0]     # a tie at the cut: term 0 beats term 5
    off, term, val = sparsify_reference(w, 3)
    assert off.tolist() == [0, 3, 6, 9, 9] and off.dtype == np.int32
    assert term.tolist() == [1, 4, 6, 0, 1, 2, 0, 3, 7] and term.dtype == np.int32
    assert val.tolist() == [0.5, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 3.0, 2.0] and val.dtype == np.float32
    off, term, val = sparsify_reference(w, 1)
    assert off.tolist() == [0, 1, 2, 3, 3] and term.tolist() == [4, 0, 3]
    w[3, 2] = -1.0                                # negative and -0.0 are not entries
    w[3, 5] = -0.0
    assert sparsify_reference(w, 8)[0].tolist() == [0, 3, 11, 15, 15]


def test_sparse_ip_reference_by_hand():
    from scipy.sparse import csr_array
    docs = csr_array(np.array([[0, 1.0, 0, 2.0], [0.5, 0, 0, 0], [0, 1.0, 0, 2.0], [0, 0, 3.0, 0]], dtype=np.float32))
    q = csr_array(np.array([[0, 2.0, 0, 1.0], [1.0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.float32))
    scores, ids = sparse_ip_reference(docs, q, 3)
    assert ids.tolist() == [[0, 2, -1], [1, -1, -1], [-1, -1, -1]]          # equal scores: the lower row first
    assert scores[0, :2].tolist() == [4.0, 4.0] and scores[1, 0] == 0.5 and np.isneginf(scores[0, 2])
    scores, ids = sparse_ip_reference(docs, q, 3, mask=np.array([False, True, True, True]))
    assert ids[0].tolist() == [2, -1, -1]
    # the sum runs over the query's terms in ascending id, two fp32 roundings per term and no fma
    d = csr_array(np.array([[1.0, 2.0 ** -24, 2.0 ** -24]], dtype=np.float32))
    qq = csr_array(np.array([[1.0, 1.0, 1.0]], dtype=np.float32))
    s, _ = sparse_ip_reference(d, qq, 1)
    assert s[0, 0] == np.float32(1.0)            # (1 + 2^-24) + 2^-24 in fp32; any other order gives 1 + 2^-23
    p = TermPostings.from_csr(docs)
    assert p.post_off.tolist() == [0, 1, 3, 4, 6] and p.post_row.tolist() == [1, 0, 2, 3, 0, 2] and p.n_rows == 4


def test_supplied_query_vectors_are_checked():
    from scipy.sparse import csr_array
    off, term, val = check_query_rows([{5: 1.5, 2: 0.25}, {}], 10)
    assert off.tolist() == [0, 2, 2] and term.tolist() == [2, 5] and val.tolist() == [0.25, 1.5]
    m = csr_array(np.array([[0, 0, 1.0], [2.0, 0, 3.0]], dtype=np.float32))
    off, term, val = check_query_rows(m, 3)
    assert off.tolist() == [0, 1, 3] and term.tolist() == [2, 0, 2] and val.tolist() == [1.0, 2.0, 3.0]
    for bad in ([{10: 1.0}], [{-1: 1.0}], [{1: 0.0}], [{1: -2.0}], [{1: float("nan")}], [{1: float("inf")}],
                [{i: 1.0 for i in range(65)}], [[1.0, 2.0]], [{1: 1e-60}]):
        with pytest.raises(ValueError):
            check_query_rows(bad, 100 if len(bad[0]) > 10 else 10)


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_terms_abi_is_declared_and_bound():
    from rag_fin_amd import _lib, build
    assert "splade.hip" in build.SOURCES
    lib = _lib.load_library()
    for name in ("rf_encode_terms", "rf_encode_terms_workspace_bytes", "rf_sparsify_terms"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.RF_TERMS_MAX == 256
    # pointer and range checks come before anything touches a device
    assert lib.rf_encode_terms(None, None, None, 1, 8, None, None, None, 0, None) == -1
    assert lib.rf_sparsify_terms(None, 1, 8, 4, None, None, None, None) == -1
    assert lib.rf_encode_terms_workspace_bytes(None, 1, 8) == 0
    buf = (np.zeros(64, np.float32), np.zeros(8, np.int32), np.zeros(64, np.int32), np.zeros(64, np.float32))
    p = [b.ctypes.data for b in buf]
    for B, V, mt in ((0, 8, 4), (1, 0, 4), (1, 8, 0), (1, 8, 257)):
        assert lib.rf_sparsify_terms(p[0], B, V, mt, p[1], p[2], p[3], None) == -1


# ---- the store's surface, with a fake encoder -----------------------------------------------------------------------
from rag_fin_amd import store as store_mod  # noqa: E402
from rag_fin_amd import text_fields  # noqa: E402
from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker  # noqa: E402
from rag_fin_amd.rag import VectorRAG  # noqa: E402
from test_hybrid_surface_cpu import TEXTS, FakeIndex, FakeSparse, HostStore, fake_fuse  # noqa: E402

FIELD = "sparse_embedding"
SPEC = {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "IP"}
IP = {"metric_type": "IP"}
WORDS = sorted({w for t in TEXTS for w in t.split()} | {"new", "row", "words"})


class FakeSparseEncoder:
    """Bag of words over a closed word list: weight = 1 + count of the word (documents), 1 (queries)."""
    vocab_size = len(WORDS)

    def __init__(self):
        self.doc_calls, self.query_calls = [], []

    def _rows(self, texts, doc):
        from scipy.sparse import csr_array
        m = np.zeros((len(texts), self.vocab_size), dtype=np.float32)
        for i, t in enumerate(texts):
            for w in t.split():
                if w in WORDS:
                    m[i, WORDS.index(w)] = m[i, WORDS.index(w)] + 1 if doc else 1.0
        return csr_array(m)

    def encode_document(self, texts):
        self.doc_calls.append(list(texts))
        return self._rows(texts, True)

    def encode_query(self, texts):
        self.query_calls.append(list(texts))
        return self._rows(texts, False)


@pytest.fixture
def doubles(monkeypatch):
    monkeypatch.setattr(text_fields, "SparseIndex", FakeSparse)
    monkeypatch.setattr(store_mod, "fuse_rrf", fake_fuse)
    FakeSparse.built.clear()


def make_store(texts=TEXTS, declare=True):
    n = len(texts)
    st = HostStore("c", dim=8, capacity=64, index=FakeIndex(capacity=64))
    st.add([f"k{i}" for i in range(n)], list(texts), np.ones((n, 8), dtype=np.float32), [f"Q{i % 2}" for i in range(n)],
           ["a"] * n, ["s"] * n, [float(i) for i in range(n)])
    enc = FakeSparseEncoder()
    if declare:
        st.create_index(FIELD, SPEC, encoder=enc)
    return st, enc


def posting_arrays(st):
    tp = st._text_fields[FIELD].postings()[0]
    return tp.post_off.tolist(), tp.post_row.tolist(), tp.post_imp.tolist()


def test_store_declares_searches_and_drops_the_learned_field(doubles):
    st, enc = make_store()
    assert st.has_index(field_name=FIELD) and not st.has_index(field_name="sparse") and not st.has_index()
    assert enc.doc_calls == []                                           # lazily, at the first search
    hits = st.search(["eps q1", "deposits"], FIELD, IP, 3, output_fields=["text"])
    assert enc.doc_calls == [TEXTS] and enc.query_calls == [["eps q1", "deposits"]]
    docs = enc._rows(TEXTS, True)
    want_s, want_i = sparse_ip_reference(docs, enc._rows(["eps q1", "deposits"], False), 3)
    assert [[h.row for h in q] for q in hits] == [[r for r in row if r >= 0] for row in want_i.tolist()]
    assert [h.score for h in hits[0]] == [float(s) for s in want_s[0] if np.isfinite(s)]
    assert hits[0][0].entity.text == TEXTS[want_i[0, 0]] and hits[0][0].id == f"k{want_i[0, 0]}"
    # supplied vectors: the pymilvus forms
    e, q1 = WORDS.index("eps"), WORDS.index("q1")
    by_dict = st.search([{e: 1.0, q1: 1.0}], FIELD, IP, 3)
    assert [h.row for h in by_dict[0]] == [h.row for h in hits[0]] and [h.score for h in by_dict[0]] == [h.score for h in hits[0]]
    by_csr = st.search(enc._rows(["eps q1"], False), FIELD, IP, 3)
    assert [h.row for h in by_csr[0]] == [h.row for h in hits[0]]
    assert st.search([{}], FIELD, IP, 3) == [[]]
    # a filter travels as the filt of the sparse search
    st.build_filter = lambda expr: np.arange(len(TEXTS)) != hits[0][0].row
    filtered = st.search(["eps q1"], FIELD, IP, 3, expr='period == "Q0"')
    assert hits[0][0].row not in [h.row for h in filtered[0]] and FakeSparse.built[-1].calls[-1][1] is not None
    st.drop_index(field_name=FIELD)
    assert not st.has_index(field_name=FIELD)
    with pytest.raises(ValueError, match="create_index"):
        st.search(["eps"], FIELD, IP, 3)


def test_store_refuses_what_the_learned_field_has_no_form_for(doubles):
    st, enc = make_store()
    for params, kw in ((dict(SPEC, metric_type="BM25"), dict(encoder=enc)), (dict(SPEC, index_type="FLAT"), dict(encoder=enc)),
                       (SPEC, {}), (SPEC, dict(encoder=object())), (dict(SPEC, params=3), dict(encoder=enc))):
        with pytest.raises(ValueError):
            st.create_index(FIELD, params, **kw)
    q = ["eps q1"]
    bad = [dict(param={"metric_type": "BM25"}), dict(param={"metric_type": "COSINE"}), dict(limit=65), dict(limit=0),
           dict(limit=True), dict(param=dict(IP, params={"radius": 0.1})), dict(param=dict(IP, params={"range_filter": 1.0})),
           dict(offset=2), dict(param=dict(IP, offset=2)), dict(group_by_field="period"), dict(mmr_lambda=0.5),
           dict(mmr_fetch_k=20), dict(expr=['period == "Q0"']), dict(ranker={"filter": 'period == "Q0"', "weight": 2.0}),
           dict(data=np.ones((1, 8), np.float32)), dict(data=[[1.0, 2.0]]), dict(data=[{len(WORDS): 1.0}]),
           dict(data=[{-1: 1.0}]), dict(data=[{0: 0.0}]), dict(data=[{0: -1.0}]), dict(data=[{0: float("nan")}]),
           dict(data=[{0: float("inf")}]), dict(data=[{i: 1.0 for i in range(65)}])]
    if len(WORDS) < 65:
        bad.pop()
    for kw in bad:
        args = dict(data=q, anns_field=FIELD, param=IP, limit=3)
        args.update(kw)
        with pytest.raises(ValueError):
            st.search(**args)
    with pytest.raises(ValueError):
        st.search_iterator(np.ones((1, 8), np.float32), FIELD, IP)
    with pytest.raises(ValueError):
        st.search(q, "embedding", {"metric_type": "COSINE"}, 3)          # strings are not vectors
    with pytest.raises(KeyError):
        st.search(q, FIELD, IP, 3, output_fields=["nope"])


def test_store_encodes_only_new_rows_and_a_delete_leaves_the_postings_of_a_fresh_build(doubles):
    st, enc = make_store()
    st.search(["eps"], FIELD, IP, 3)
    assert enc.doc_calls == [TEXTS]
    new = ["new row words eps", "q1 words"]
    st.add(["n0", "n1"], new, np.ones((2, 8), np.float32), ["Q0", "Q1"], ["a"] * 2, ["s"] * 2, [1.0, 2.0])
    st.search(["eps"], FIELD, IP, 3)
    assert enc.doc_calls == [TEXTS, new]                                 # only the appended rows
    st.search(["eps"], FIELD, IP, 3)
    assert len(enc.doc_calls) == 2                                       # nothing to do
    st.delete('period == "Q0"')
    st.search(["eps"], FIELD, IP, 3)
    assert len(enc.doc_calls) == 2                                       # a delete encodes nothing
    survivors = list(st.columns["text"])
    fresh, _ = make_store(survivors)
    assert posting_arrays(st) == posting_arrays(fresh) and st._text_fields[FIELD].postings()[0].n_rows == len(survivors)
    # rows appended and deleted before they were ever encoded
    st.add(["m0", "m1"], ["eps eps", "words"], np.ones((2, 8), np.float32), ["Q0", "Q1"], ["a"] * 2, ["s"] * 2, [1.0, 2.0])
    st.delete('id == "m0"')
    fresh, _ = make_store(list(st.columns["text"]))
    assert posting_arrays(st) == posting_arrays(fresh) and enc.doc_calls[-1] == ["words"]
    # an upsert replaces a row: its vector goes, the new text is encoded
    st.upsert([["k1"], ["deposits deposits"], np.ones((1, 8), np.float32), ["Q1"], ["a"], ["s"], [9.0]])
    fresh, _ = make_store(list(st.columns["text"]))
    assert posting_arrays(st) == posting_arrays(fresh) and enc.doc_calls[-1] == ["deposits deposits"]
    st.drop()
    assert st.search(["eps"], FIELD, IP, 3) == [[]]


def test_hybrid_search_takes_a_learned_arm(doubles):
    st, enc = make_store()
    st.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
    Q = np.ones((1, 8), dtype=np.float32)
    reqs = [AnnSearchRequest(Q, "embedding", {"metric_type": "COSINE"}, 4),
            AnnSearchRequest(["eps q1"], FIELD, IP, 5),
            AnnSearchRequest(["eps q1"], "sparse", {"metric_type": "BM25"}, 3)]
    got = st.hybrid_search(reqs, RRFRanker(), 4)
    dense = [9, 8, 7, 6]
    learned = [h.row for h in st.search(["eps q1"], FIELD, IP, 5)[0]]
    bm25 = [h.row for h in st.search(["eps q1"], "sparse", {"metric_type": "BM25"}, 3)[0]]
    pad = lambda a: a + [-1] * (5 - len(a))   # noqa: E731
    from rag_fin_amd import lexical
    _, want, fused = lexical.rrf_reference(np.array([[pad(dense)], [pad(learned)], [pad(bm25)]]), 4)
    assert [h.row for h in got[0]] == want[0].tolist() and [h.score for h in got[0]] == fused[0].tolist()
    for bad in (AnnSearchRequest(["eps"], FIELD, {"metric_type": "BM25"}, 3), AnnSearchRequest(Q, FIELD, IP, 3),
                AnnSearchRequest(["eps"], FIELD, dict(IP, params={"radius": 1.0}), 3),
                AnnSearchRequest(["eps", "q1"], FIELD, IP, 3)):
        with pytest.raises(ValueError):
            st.hybrid_search([reqs[0], bad], RRFRanker(), 3)


@pytest.fixture
def one_rank_group():
    import os
    import socket
    import torch.distributed as dist
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def test_sharded_store_refuses_the_learned_field(one_rank_group):
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    st = ShardedCorpusStore("c", dim=8, capacity=4, index=FakeIndex(8, 4), backend=object())
    with pytest.raises(NotImplementedError):
        st.create_index(FIELD, SPEC, encoder=FakeSparseEncoder())
    with pytest.raises(NotImplementedError):
        st.search(["eps"], FIELD, IP, 3)
    with pytest.raises(NotImplementedError):
        st.has_index(field_name=FIELD)
    with pytest.raises(NotImplementedError):
        st.drop_index(field_name=FIELD)
    with pytest.raises(NotImplementedError):
        st.hybrid_search([AnnSearchRequest(["eps"], FIELD, IP, 3)], RRFRanker(), 3)


# ---- serving: lexical= ----------------------------------------------------------------------------------------------
class RecordingStore:
    """Records create_index and the arms of hybrid_search."""
    num_entities = 3

    def __init__(self):
        self.created, self.arms = [], []

    def load(self):
        pass

    def create_index(self, field, params, **kw):
        self.created.append((field, params, kw))

    def hybrid_search(self, reqs, rerank, limit, output_fields=None):
        self.arms.append([(r.anns_field, r.param, r.limit, r.expr, type(r.data).__name__) for r in reqs])
        return [[] for _ in range(len(reqs[1].data))]


class FakeEmbedder:
    dim = 4

    def encode(self, texts):
        return np.ones((len(texts), 4), dtype=np.float32)


def test_vector_rag_declares_the_field_and_forwards_lexical():
    enc, store = FakeSparseEncoder(), RecordingStore()
    rag = VectorRAG("k", embedder=FakeEmbedder(), store=store, sparse_encoder=enc)
    assert store.created == [(FIELD, SPEC, {"encoder": enc})]
    rag.search("net profit", 3, hybrid=True)                             # today's call: dense + BM25
    assert [a[0] for a in store.arms[-1]] == ["embedding", "sparse"]
    assert store.arms[-1][1] == ("sparse", {"metric_type": "BM25"}, 20, None, "list")
    rag.search("net profit", 3, hybrid=True, lexical="bm25")
    assert store.arms[-1] == store.arms[-2]
    rag.search("net profit", 3, hybrid=True, lexical="learned", expr='period == "Q1"', fetch_k=8)
    assert store.arms[-1][1:] == [(FIELD, IP, 8, 'period == "Q1"', "list")] and len(store.arms[-1]) == 2
    rag.search_batch(["a b c d e", "f g h i j"], 2, hybrid=True, lexical="both")
    assert [a[0] for a in store.arms[-1]] == ["embedding", "sparse", FIELD]
    for kw in (dict(lexical="learned"), dict(hybrid=True, lexical="splade"), dict(lexical="both")):
        with pytest.raises(ValueError):
            rag.search("q", 3, **kw)
        with pytest.raises(ValueError):
            rag.search_batch(["q"], 3, **kw)
    plain_store = RecordingStore()
    plain = VectorRAG("k", embedder=FakeEmbedder(), store=plain_store)
    assert plain_store.created == []
    plain.search("q", 3, hybrid=True)
    for lex in ("learned", "both"):
        with pytest.raises(ValueError, match="sparse encoder"):
            plain.search("q", 3, hybrid=True, lexical=lex)


class FakeRag:
    def __init__(self):
        self.calls = []

    def search(self, query, top_k=3, expr=None, **kw):
        self.calls.append((query, top_k, expr, kw))
        return []


def test_mcp_tool_and_rest_body_forward_lexical_only_when_given(monkeypatch):
    from rag_fin_amd import service
    from rag_fin_amd.adapter import SearchRequest, search_args
    rag = FakeRag()
    mcp_server.set_rag(rag)
    try:
        mcp_server.search_vectors("net interest income", 4, hybrid=True, lexical="learned")
        assert rag.calls[-1] == ("net interest income", 4, None, {"hybrid": True, "lexical": "learned"})
        mcp_server.search_vectors("q", 4, filter="id == 1", hybrid=True, lexical="both", fetch_k=32)
        assert rag.calls[-1] == ("q", 4, "id == 1", {"fetch_k": 32, "hybrid": True, "lexical": "both"})
        mcp_server.search_vectors("q", 2, hybrid=True)                   # the calls of before
        assert rag.calls[-1] == ("q", 2, None, {"hybrid": True})
        mcp_server.search_vectors("q", 2, filter="id == 1")
        assert rag.calls[-1] == ("q", 2, "id == 1", {})
        mcp_server.set_rag(VectorRAG("k", embedder=FakeEmbedder(), store=RecordingStore()))
        r = mcp_server.search_vectors("q", 3, hybrid=True, lexical="learned")
        assert r["status"] == "error" and "sparse encoder" in r["message"]
    finally:
        mcp_server.set_rag(None)
    assert search_args(SearchRequest(query="hello", top_k=4)) == {"query": "hello", "top_k": 4}
    assert search_args(SearchRequest(query="hello", hybrid=True)) == {"query": "hello", "top_k": 3, "hybrid": True}
    assert search_args(SearchRequest(query="hello", hybrid=True, lexical="both")) == \
        {"query": "hello", "top_k": 3, "lexical": "both", "hybrid": True}
    # SPARSE_MODEL_DIR reaches build_rag, and only when it is set
    seen = []
    monkeypatch.setattr(service, "build_rag", lambda *a, **kw: seen.append(kw))
    monkeypatch.setenv("RAGFIN_MODEL_DIR", "/models/minilm")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("SPARSE_MODEL_DIR", raising=False)
    service.build_rag_from_env()
    assert "sparse_dir" not in seen[-1]
    monkeypatch.setenv("SPARSE_MODEL_DIR", "/models/splade")
    service.build_rag_from_env()
    assert seen[-1]["sparse_dir"] == "/models/splade"
