"""Late interaction, the parts that need no GPU:
  * tokens_reference (the fp64 numpy definition of rf_encode_tokens) and both checkpoint layouts pinned to the
    in-container transformers.BertModel + Linear(bias=False) + normalize, through a synthetic checkpoint directory;
  * the row layout by hand: markers, skiplist, truncation to 32, expansion, and the refusal of unattended expansion;
  * maxsim_reference and topk_reference on hand-made cases;
  * the library's host-side refusals;
  * the store's "token_embeddings" field with doubles for the encoder and the scorer, the rerank_with= forwarding
    of VectorRAG, the tool and the REST body."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import encoder as oenc
from rag_fin_amd import late_interaction as late
from rag_fin_amd import mcp_server
from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
from rag_fin_amd.rag import VectorRAG
from test_hybrid_surface_cpu import TEXTS, FakeIndex, HostStore, fake_fuse

CFG2 = dict(oenc.MINILM_L6, layers=2, vocab_size=2005)


@functools.lru_cache(maxsize=None)
def l2_model():
    """(cfg, fp32 weights, fp16-rounded weights) of the 2-layer parity model: both sides from the seed."""
    w = oenc.random_weights(CFG2, 5)
    return CFG2, w, oenc.round_weights_fp16(w)


# ---- the definition against transformers, through both checkpoint layouts --------------------------------------------
def write_checkpoint(path, layout, cfg, dim, extra=None):
    """A synthetic ColBERT directory in the Stanford or the PyLate layout -> (the torch BertModel, the Linear)."""
    transformers = pytest.importorskip("transformers")
    from safetensors.numpy import save_file
    torch.manual_seed(13)
    hc = transformers.BertConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"],
                                 num_attention_heads=cfg["heads"], intermediate_size=cfg["intermediate"],
                                 max_position_embeddings=cfg["max_position"], type_vocab_size=2, hidden_act="gelu",
                                 hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, layer_norm_eps=cfg["ln_eps"])
    bert = transformers.BertModel(hc, add_pooling_layer=False)
    linear = torch.nn.Linear(cfg["hidden"], dim, bias=False)
    with torch.no_grad():   # the default init leaves biases at 0 and LayerNorm at (1, 0): move them
        for name, p in bert.named_parameters():
            if name.endswith("bias") or "LayerNorm" in name:
                p.add_(0.1 * torch.randn_like(p))
    bert, linear = bert.double().eval(), linear.double().eval()
    sd = {k: v.detach().numpy().astype(np.float32) for k, v in bert.state_dict().items()}
    proj = linear.weight.detach().numpy().astype(np.float32)
    os.makedirs(path, exist_ok=True)
    if layout == "stanford":
        save_file(dict({"bert." + k: v for k, v in sd.items()}, **{"linear.weight": proj}),
                  os.path.join(path, "model.safetensors"))
        if extra is not None:
            with open(os.path.join(path, "artifact.metadata"), "w") as f:
                json.dump(extra, f)
    else:
        save_file(sd, os.path.join(path, "model.safetensors"))
        os.makedirs(os.path.join(path, "1_Dense"))
        save_file({"linear.weight": proj}, os.path.join(path, "1_Dense", "model.safetensors"))
        if extra is not None:
            with open(os.path.join(path, "config_sentence_transformers.json"), "w") as f:
                json.dump(extra, f)
    # (the checkpoint holds float32: the torch side is reloaded from what was written)
    bert.load_state_dict({k: torch.as_tensor(v).double() for k, v in sd.items()})
    linear.weight.data = torch.as_tensor(proj).double()
    return bert, linear


@pytest.mark.parametrize("layout", ["stanford", "pylate"])
def test_tokens_reference_and_checkpoint_mappings_match_transformers(tmp_path, layout):
    from rag_fin_amd.embedder import stack_hf_state_dict
    cfg = dict(oenc.MINILM_L6, layers=2, vocab_size=211, max_position=48)
    bert, linear = write_checkpoint(str(tmp_path / layout), layout, cfg, 48)
    sd, proj = late.load_checkpoint(str(tmp_path / layout))
    assert proj.shape == (48, 384) and proj.dtype == np.float32
    w = stack_hf_state_dict(sd, cfg)
    rng = np.random.default_rng(1)
    B, T = 5, 33
    lens = np.array([33, 20, 9, 1, 0])
    ids = rng.integers(1, cfg["vocab_size"], (B, T))
    att = (np.arange(T)[None, :] < np.maximum(lens, 1)[:, None]).astype(np.int64)   # (torch needs one key per row)
    with torch.no_grad():
        x = bert(input_ids=torch.as_tensor(ids), attention_mask=torch.as_tensor(att)).last_hidden_state
        want = torch.nn.functional.normalize(linear(x), p=2, dim=-1).numpy()
    skip = np.zeros((cfg["vocab_size"] + 31) // 32, dtype=np.uint32)
    dropped = sorted(set(ids[0, :5].tolist()))
    for i in dropped:
        skip[i >> 5] |= np.uint32(1 << (i & 31))
    got = late.tokens_reference(w, proj, cfg, ids, lens)
    assert [g.shape for g in got] == [(33, 48), (20, 48), (9, 48), (1, 48), (0, 48)]
    for b in range(4):
        assert np.abs(got[b] - want[b, :lens[b]]).max() < 1e-9
    cut = late.tokens_reference(w, proj, cfg, ids, lens, skip=skip)
    for b in range(4):
        keep = ~np.isin(ids[b, :lens[b]], dropped)
        assert cut[b].shape[0] == keep.sum() and np.abs(cut[b] - want[b, :lens[b]][keep]).max() < 1e-9
    assert cut[0].shape[0] <= 28


def test_a_directory_without_a_projection_is_refused(tmp_path):
    from safetensors.numpy import save_file
    save_file({"embeddings.word_embeddings.weight": np.zeros((5, 384), np.float32)}, str(tmp_path / "model.safetensors"))
    with pytest.raises(KeyError, match="linear.weight"):
        late.load_checkpoint(str(tmp_path))


def test_settings_are_read_for_the_keys_that_are_present(tmp_path):
    assert late.read_settings(str(tmp_path)) == late.DEFAULTS
    with open(tmp_path / "config_sentence_transformers.json", "w") as f:
        json.dump({"query_length": 24, "document_prefix": "[D] ", "attend_to_expansion_tokens": False,
                   "skiplist_words": [".", ","]}, f)
    s = late.read_settings(str(tmp_path))
    assert s == dict(late.DEFAULTS, query_length=24, document_marker="[D]", attend_to_expansion_tokens=False,
                     skiplist_words=[".", ","])
    os.remove(tmp_path / "config_sentence_transformers.json")
    with open(tmp_path / "artifact.metadata", "w") as f:
        json.dump({"query_maxlen": 32, "doc_maxlen": 300, "query_token_id": "[unused0]", "attend_to_mask_tokens": True,
                   "mask_punctuation": False}, f)
    s = late.read_settings(str(tmp_path))
    assert s == dict(late.DEFAULTS, document_length=300, attend_to_expansion_tokens=True, skiplist_words=[])


# ---- the row layout, by hand ---------------------------------------------------------------------------------------
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "[unused0]", "[unused1]", ".", ",", "!", "net", "profit", "rose",
         "in", "q", "##1", "eps", "[Q]"]


def tokenizer():
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    return WordPieceTokenizer(VOCAB)


def test_row_layout_markers_truncation_and_expansion():
    tok = tokenizer()
    v = tok.vocab
    ids, lens = late.build_rows(tok, ["net profit rose.", "eps"], False, document_length=8)
    assert ids.tolist() == [[v["[CLS]"], v["[unused1]"], v["net"], v["profit"], v["rose"], v["."], v["[SEP]"]],
                            [v["[CLS]"], v["[unused1]"], v["eps"], v["[SEP]"], 0, 0, 0]]
    assert lens.tolist() == [7, 4] and ids.dtype == np.int32 and lens.dtype == np.int32
    ids, lens = late.build_rows(tok, ["net profit rose in q1, net profit!"], False, document_length=8)
    assert lens.tolist() == [8] and ids[0, 1] == v["[unused1]"] and ids[0, -1] == v["[SEP]"]   # cut to 8, [SEP] kept
    # queries: marker, cut to 32 whatever query_length says, filled with [MASK] tokens that count
    ids, lens = late.build_rows(tok, ["net profit", " ".join(["eps"] * 50)], True, query_length=64)
    assert ids.shape == (2, 32) and lens.tolist() == [32, 32]
    assert ids[0].tolist() == [v["[CLS]"], v["[unused0]"], v["net"], v["profit"], v["[SEP]"]] + [v["[MASK]"]] * 27
    assert ids[1, 1] == v["[unused0]"] and ids[1, 31] == v["[SEP]"] and (ids[1, 2:31] == v["eps"]).all()
    ids, lens = late.build_rows(tok, ["net profit", "eps"], True, query_expansion=False)
    assert lens.tolist() == [5, 4] and ids.shape == (2, 5) and ids[1, 4] == v["[PAD]"]
    ids, _ = late.build_rows(tok, ["eps"], True, query_length=6, query_marker="[Q] ")
    assert ids.tolist() == [[v["[CLS]"], v["[Q]"], v["eps"], v["[SEP]"], v["[MASK]"], v["[MASK]"]]]
    ids, _ = late.build_rows(tok, ["eps"], False, document_marker="[D]")      # a marker the vocabulary lacks
    assert ids[0, 1] == v["[unused1]"]
    assert late.build_rows(tok, ["eps"], False, document_marker=9)[0][0, 1] == 9
    with pytest.raises(ValueError):
        late.build_rows(tok, ["eps"], True, query_length=2)


def test_skiplist_bitmap_and_packed_queries():
    tok = tokenizer()
    bits = late.skip_bitmap(tok.vocab, late.DEFAULT_SKIPLIST, 40)
    assert bits.dtype == np.uint32 and bits.shape == (2,)
    assert [i for i in range(40) if (bits[i >> 5] >> (i & 31)) & 1] == [7, 8, 9]              # . , ! are tokens
    assert not late.skip_bitmap(tok.vocab, [], 40).any()
    q_vec, q_len = late.pack_queries([np.ones((3, 16), np.float32), np.zeros((0, 16))], 16)
    assert q_vec.shape == (2, 32, 16) and q_vec.dtype == np.float16 and q_len.tolist() == [3, 0]
    assert q_vec[0, :3].all() and not q_vec[0, 3:].any()
    for bad in ([np.ones((33, 16))], [np.ones((3, 32))], [np.ones(16)]):
        with pytest.raises(ValueError):
            late.pack_queries(bad, 16)


def test_unattended_expansion_is_off_by_default_and_refused_when_asked():
    assert late.resolve_query_expansion(None, None) is True and late.resolve_query_expansion(True, None) is True
    assert late.resolve_query_expansion(None, False) is False
    assert late.resolve_query_expansion(False, None) is False and late.resolve_query_expansion(False, False) is False
    with pytest.raises(ValueError, match="expansion"):
        late.resolve_query_expansion(False, True)


# ---- scoring and selection definitions, by hand ------------------------------------------------------------------------
def test_maxsim_reference_by_hand():
    e = np.eye(4)
    docs = [np.array([e[0], e[1]]), np.array([-e[0]]), np.zeros((0, 4)), np.array([0.5 * e[0] + 0.5 * e[1]])]
    queries = [np.array([e[0], e[1], e[2]]), np.array([e[0]]), np.zeros((0, 4))]
    s = late.maxsim_reference(docs, queries)
    assert s.shape == (3, 4) and s.dtype == np.float64
    assert s[0].tolist() == [2.0, -1.0, -np.inf, 1.0]            # an all-negative row stays negative, an empty row is no hit
    assert s[1].tolist() == [1.0, -1.0, -np.inf, 0.5]
    assert np.isneginf(s[2]).all()                               # a query without tokens hits nothing
    s = late.maxsim_reference(docs, queries, mask=np.array([False, True, True, True]))
    assert s[0].tolist() == [-np.inf, -1.0, -np.inf, 1.0]


def test_topk_reference_by_hand():
    s = np.array([[1.0, 3.0, -np.inf, 3.0, -2.0, np.nan], [-np.inf] * 6], dtype=np.float32)
    got_s, got_i = late.topk_reference(s, 3)
    assert got_i.tolist() == [[1, 3, 0], [-1, -1, -1]] and got_i.dtype == np.int64       # ties: the lower row first
    assert got_s[0].tolist() == [3.0, 3.0, 1.0] and np.isneginf(got_s[1]).all() and got_s.dtype == np.float32
    got_s, got_i = late.topk_reference(s[0], 6, id_base=100)
    assert got_i[0].tolist() == [101, 103, 100, 104, -1, -1] and np.isneginf(got_s[0, 4:]).all()
    _, got_i = late.topk_reference(s[:1], 2, rows=[[9, 8, 7, 6, 5, 4]])
    assert got_i[0].tolist() == [8, 6]                           # ties in the order of the segment
    _, got_i = late.topk_reference(np.array([-0.0, 0.0, -1.0], np.float32), 3)
    assert got_i[0].tolist() == [1, 0, 2]                        # bit patterns: -0.0 below +0.0


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_late_interaction_abi_is_declared_bound_and_refuses_on_the_host():
    import ctypes
    from rag_fin_amd import _lib, build
    assert "late_interaction.hip" in build.SOURCES
    lib = _lib.load_library()
    for name in ("rf_encode_tokens", "rf_encode_tokens_workspace_bytes", "rf_maxsim", "rf_maxsim_topk"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.RF_MAXSIM_QTOK == 32 and _lib.RF_MAXSIM_DIM == 128
    # pointer and range checks come before anything touches a device
    assert lib.rf_encode_tokens_workspace_bytes(None, 1, 8) == 0
    assert lib.rf_encode_tokens(None, None, None, 1, 8, None, None, None, None, 0, None) == -1
    vec = np.zeros((64, 128), np.float16)
    off = np.array([0, 4], np.int64)
    q = np.zeros((1, 32, 128), np.float16)
    ql = np.ones(1, np.int32)
    out = np.zeros(8, np.float32)

    def field(dim):
        return _lib.TokenField(vec.ctypes.data, off.ctypes.data, 1, dim)

    def call(f, qv=q.ctypes.data, B=1):
        return lib.rf_maxsim(ctypes.byref(f), qv, ql.ctypes.data, B, None, None, None, out.ctypes.data, None)
    assert call(field(32), qv=None) == -1 and "null" in lib.rf_last_error().decode()
    assert lib.rf_maxsim(None, q.ctypes.data, ql.ctypes.data, 1, None, None, None, out.ctypes.data, None) == -1
    for dim in (24, 144, 0, 8):
        assert call(field(dim)) == -2 and "dim" in lib.rf_last_error().decode()
    assert call(field(32), B=0) == -1
    seg = np.array([0, 4], np.int64)
    ids = np.zeros(64, np.int64)
    so = np.zeros(64, np.float32)
    for B, k in ((0, 4), (1, 0), (1, 65)):
        assert lib.rf_maxsim_topk(out.ctypes.data, seg.ctypes.data, None, B, k, 0, so.ctypes.data, ids.ctypes.data,
                                  None, None) == -1
    assert lib.rf_maxsim_topk(None, seg.ctypes.data, None, 1, 4, 0, so.ctypes.data, ids.ctypes.data, None, None) == -1


# ---- the store's surface, with doubles for the encoder and the scorer ----------------------------------------------
from rag_fin_amd import store as store_mod  # noqa: E402

FIELD = "token_embeddings"
SPEC = {"index_type": "EMB_LIST_FLAT", "metric_type": "MAX_SIM_IP"}
MS = {"metric_type": "MAX_SIM_IP"}
WORDS = sorted({w for t in TEXTS for w in t.split()} | {"new", "row", "words"})
DIM = 32


class FakeColBERT:
    """One one-hot vector per known word of a text (documents and queries alike)."""
    dim = DIM

    def __init__(self):
        self.doc_calls, self.query_calls = [], []

    @staticmethod
    def _rows(texts):
        out = []
        for t in texts:
            idx = [WORDS.index(w) % DIM for w in t.split() if w in WORDS][:32]
            out.append(np.eye(DIM, dtype=np.float16)[idx].reshape(len(idx), DIM))
        return out

    def encode(self, texts, is_query=False):
        (self.query_calls if is_query else self.doc_calls).append(list(texts))
        return self._rows(texts)


class FakeTokenField:
    """late_interaction.TokenField without a device: host lists and the numpy definitions."""

    def __init__(self, dim, device=None):
        self.dim, self.rows, self.calls = dim, [], []

    n_rows = property(lambda self: len(self.rows))
    n_tok = property(lambda self: sum(r.shape[0] for r in self.rows))
    off_host = property(lambda self: np.concatenate([[0], np.cumsum([r.shape[0] for r in self.rows])]).astype(np.int64))

    def append(self, rows):
        self.rows.extend(np.asarray(r, dtype=np.float16) for r in rows)

    def keep(self, mask):
        self.rows = [r for r, k in zip(self.rows, mask) if k]

    def vectors(self, rows):
        return [self.rows[r] for r in rows]

    def search(self, queries, k, filt=None):
        self.calls.append((k, filt))
        mask = None if filt is None else np.asarray(filt, dtype=bool)
        s, i = late.topk_reference(late.maxsim_reference(self.rows, queries, mask).astype(np.float32), k)
        return torch.from_numpy(s), torch.from_numpy(i)


def fake_maxsim(field, queries, candidates=None, filter=None):
    s = late.maxsim_reference(field.rows, queries).astype(np.float32)
    if candidates is None:
        return s
    return np.array([s[b, r] if 0 <= r < field.n_rows else -np.inf for b, c in enumerate(candidates) for r in c],
                    dtype=np.float32)


@pytest.fixture
def doubles(monkeypatch):
    monkeypatch.setattr(late, "TokenField", FakeTokenField)
    monkeypatch.setattr(late, "maxsim", fake_maxsim)
    monkeypatch.setattr(store_mod, "fuse_rrf", fake_fuse)


def make_store(texts=TEXTS, declare=True):
    n = len(texts)
    st = HostStore("c", dim=8, capacity=64, index=FakeIndex(capacity=64))
    st.add([f"k{i}" for i in range(n)], list(texts), np.ones((n, 8), dtype=np.float32), [f"Q{i % 2}" for i in range(n)],
           ["a"] * n, ["s"] * n, [float(i) for i in range(n)])
    enc = FakeColBERT()
    if declare:
        st.create_index(FIELD, SPEC, encoder=enc)
    return st, enc


def field_arrays(st):
    f = st._text_fields[FIELD].index()
    return f.off_host.tolist(), [r.tolist() for r in f.rows]


def test_store_declares_searches_and_drops_the_token_field(doubles):
    st, enc = make_store()
    assert st.has_index(field_name=FIELD) and not st.has_index(field_name="sparse") and not st.has_index()
    assert enc.doc_calls == []                                           # lazily, at the first search
    hits = st.search(["eps q1", "deposits"], FIELD, MS, 3, output_fields=["text"])
    assert enc.doc_calls == [TEXTS] and enc.query_calls == [["eps q1", "deposits"]]
    want_s, want_i = late.topk_reference(
        late.maxsim_reference(enc._rows(TEXTS), enc._rows(["eps q1", "deposits"])).astype(np.float32), 3)
    assert [[h.row for h in q] for q in hits] == want_i.tolist()
    assert [h.score for h in hits[0]] == [float(s) for s in want_s[0]]
    assert hits[0][0].row == 0 and hits[0][0].score == 2.0 and hits[0][0].entity.text == TEXTS[0] and hits[0][0].id == "k0"
    # supplied token vectors
    by_vec = st.search(enc._rows(["eps q1"]), FIELD, MS, 3)
    assert [(h.row, h.score) for h in by_vec[0]] == [(h.row, h.score) for h in hits[0]]
    assert st.search([np.zeros((0, DIM), np.float16)], FIELD, MS, 3) == [[]]    # a query without tokens hits nothing
    assert [len(v) for v in st.token_vectors([0, 7])] == [len(TEXTS[0].split()), 3]
    # a filter travels as the filt of the search
    st.build_filter = lambda expr: np.arange(len(TEXTS)) != 0
    filtered = st.search(["eps q1"], FIELD, MS, 3, expr='period == "Q0"')
    assert 0 not in [h.row for h in filtered[0]] and st._text_fields[FIELD].index().calls[-1][1] is not None
    # candidate mode on the stored vectors
    got = st.rerank_tokens(["eps q1", "deposits"], [[7, 0, 99], []])
    assert [g.tolist() for g in got] == [[1.0, 2.0, -np.inf], []]
    st.drop_index(field_name=FIELD)
    assert not st.has_index(field_name=FIELD)
    with pytest.raises(ValueError, match="create_index"):
        st.search(["eps"], FIELD, MS, 3)
    with pytest.raises(ValueError, match="create_index"):
        st.token_vectors([0])


def test_store_refuses_what_the_token_field_has_no_form_for(doubles):
    from rag_fin_amd.ranker import BoostRanker
    st, enc = make_store()
    for params, kw in ((dict(SPEC, metric_type="IP"), dict(encoder=enc)), (dict(SPEC, index_type="FLAT"), dict(encoder=enc)),
                       (SPEC, {}), (SPEC, dict(encoder=object())), (dict(SPEC, params=3), dict(encoder=enc))):
        with pytest.raises(ValueError):
            st.create_index(FIELD, params, **kw)
    q = ["eps q1"]
    bad = [dict(param={"metric_type": "IP"}), dict(param={"metric_type": "COSINE"}), dict(limit=65), dict(limit=0),
           dict(limit=True), dict(param=dict(MS, params={"radius": 0.1})), dict(param=dict(MS, params={"range_filter": 1.0})),
           dict(offset=2), dict(param=dict(MS, offset=2)), dict(group_by_field="period"), dict(mmr_lambda=0.5),
           dict(mmr_fetch_k=20), dict(expr=['period == "Q0"']), dict(ranker=BoostRanker('period == "Q0"', 2.0)),
           dict(data=np.ones((1, 8), np.float32)), dict(data=[[1.0, 2.0]]), dict(data=[{0: 1.0}]),
           dict(data=[np.ones((33, DIM), np.float16)]), dict(data=[np.ones((2, DIM + 16), np.float16)])]
    for kw in bad:
        args = dict(data=q, anns_field=FIELD, param=MS, limit=3)
        args.update(kw)
        with pytest.raises(ValueError, match=FIELD):
            st.search(**args)
    with pytest.raises(ValueError, match=FIELD):
        st.search_iterator(np.ones((1, 8), np.float32), FIELD, MS)
    with pytest.raises(ValueError):
        st.search(q, "embedding", {"metric_type": "COSINE"}, 3)          # strings are not vectors
    with pytest.raises(KeyError):
        st.search(q, FIELD, MS, 3, output_fields=["nope"])
    with pytest.raises(ValueError):
        st.rerank_tokens(["a", "b"], [[0]])


def test_store_encodes_only_new_rows_and_a_delete_leaves_the_field_of_a_fresh_build(doubles):
    st, enc = make_store()
    st.search(["eps"], FIELD, MS, 3)
    assert enc.doc_calls == [TEXTS]
    new = ["new row words eps", "q1 words"]
    st.add(["n0", "n1"], new, np.ones((2, 8), np.float32), ["Q0", "Q1"], ["a"] * 2, ["s"] * 2, [1.0, 2.0])
    st.search(["eps"], FIELD, MS, 3)
    assert enc.doc_calls == [TEXTS, new]                                 # only the appended rows
    st.search(["eps"], FIELD, MS, 3)
    assert len(enc.doc_calls) == 2                                       # nothing to do
    st.delete('period == "Q0"')
    st.search(["eps"], FIELD, MS, 3)
    assert len(enc.doc_calls) == 2                                       # a delete encodes nothing
    survivors = list(st.columns["text"])
    fresh, _ = make_store(survivors)
    assert field_arrays(st) == field_arrays(fresh) and st._text_fields[FIELD].index().n_rows == len(survivors)
    # rows appended and deleted before they were ever encoded
    st.add(["m0", "m1"], ["eps eps", "words"], np.ones((2, 8), np.float32), ["Q0", "Q1"], ["a"] * 2, ["s"] * 2, [1.0, 2.0])
    st.delete('id == "m0"')
    fresh, _ = make_store(list(st.columns["text"]))
    assert field_arrays(st) == field_arrays(fresh) and enc.doc_calls[-1] == ["words"]
    # an upsert replaces a row: its vectors go, the new text is encoded
    st.upsert([["k1"], ["deposits deposits"], np.ones((1, 8), np.float32), ["Q1"], ["a"], ["s"], [9.0]])
    fresh, _ = make_store(list(st.columns["text"]))
    assert field_arrays(st) == field_arrays(fresh) and enc.doc_calls[-1] == ["deposits deposits"]
    st.drop()
    assert st.search(["eps"], FIELD, MS, 3) == [[]]


def test_hybrid_search_takes_a_token_arm(doubles):
    from rag_fin_amd import lexical
    st, enc = make_store()
    Q = np.ones((1, 8), dtype=np.float32)
    reqs = [AnnSearchRequest(Q, "embedding", {"metric_type": "COSINE"}, 4), AnnSearchRequest(["eps q1"], FIELD, MS, 5)]
    got = st.hybrid_search(reqs, RRFRanker(), 4)
    dense = [9, 8, 7, 6]
    tokens = [h.row for h in st.search(["eps q1"], FIELD, MS, 5)[0]]
    pad = lambda a: a + [-1] * (5 - len(a))   # noqa: E731
    _, want, fused = lexical.rrf_reference(np.array([[pad(dense)], [pad(tokens)]]), 4)
    assert [h.row for h in got[0]] == want[0].tolist() and [h.score for h in got[0]] == fused[0].tolist()
    for bad in (AnnSearchRequest(["eps"], FIELD, {"metric_type": "IP"}, 3), AnnSearchRequest(Q, FIELD, MS, 3),
                AnnSearchRequest(["eps"], FIELD, dict(MS, params={"radius": 1.0}), 3),
                AnnSearchRequest(["eps", "q1"], FIELD, MS, 3)):
        with pytest.raises(ValueError):
            st.hybrid_search([reqs[0], bad], RRFRanker(), 3)


def test_save_and_load_do_not_persist_the_field(doubles, tmp_path):
    from test_hybrid_surface_cpu import LoadableStore
    st, _ = make_store()
    st.search(["eps"], FIELD, MS, 3)
    st.save(str(tmp_path / "s"))
    assert sorted(os.listdir(tmp_path / "s")) == ["columns.json", "vectors.f16"]
    loaded = LoadableStore.load_from(str(tmp_path / "s"))
    assert not loaded.has_index(field_name=FIELD)


@pytest.fixture
def one_rank_group():
    import socket
    import torch.distributed as dist
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def test_sharded_store_refuses_the_token_field(one_rank_group):
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    st = ShardedCorpusStore("c", dim=8, capacity=4, index=FakeIndex(8, 4), backend=object())
    with pytest.raises(NotImplementedError):
        st.create_index(FIELD, SPEC, encoder=FakeColBERT())
    with pytest.raises(NotImplementedError):
        st.search(["eps"], FIELD, MS, 3)
    with pytest.raises(NotImplementedError):
        st.has_index(field_name=FIELD)
    with pytest.raises(NotImplementedError):
        st.drop_index(field_name=FIELD)
    with pytest.raises(NotImplementedError):
        st.hybrid_search([AnnSearchRequest(["eps"], FIELD, MS, 3)], RRFRanker(), 3)


# ---- serving: rerank_with= --------------------------------------------------------------------------------------------
class Entity:
    def __init__(self, row):
        self.text, self.period, self.chunk_type, self.statement_type, self.primary_value = f"text {row}", "Q1", "a", "s", 1.0


class RecHit:
    def __init__(self, row, score):
        self.row, self.id, self.score, self.entity = row, f"k{row}", score, Entity(row)


class RecordingStore:
    """Records create_index, the dense searches and the candidate-mode calls."""
    num_entities = 8
    LATE = {0: 1.0, 1: 3.0, 2: 3.0, 3: -np.inf, 4: 2.0, 5: 0.5, 6: 0.0, 7: 0.25}

    def __init__(self):
        self.created, self.searches, self.reranks = [], [], []

    def load(self):
        pass

    def create_index(self, field, params, **kw):
        self.created.append((field, params, kw))

    def search(self, data, anns_field, param, limit, **kw):
        self.searches.append((anns_field, param, limit, kw))
        return [[RecHit(r, 1.0 - 0.1 * r) for r in range(min(limit, 8))] for _ in range(len(data))]

    def rerank_tokens(self, queries, candidates):
        self.reranks.append((list(queries), [list(c) for c in candidates]))
        return [np.array([self.LATE[r] for r in c], dtype=np.float32) for c in candidates]


class FakeEmbedder:
    dim = 4

    def encode(self, texts):
        return np.ones((len(texts), 4), dtype=np.float32)


class FakeCross:
    def predict(self, pairs):
        return [float(len(p[1])) for p in pairs]


def test_vector_rag_declares_the_field_and_forwards_rerank_with():
    enc, store = FakeColBERT(), RecordingStore()
    rag = VectorRAG("k", embedder=FakeEmbedder(), store=store, late_encoder=enc, reranker=FakeCross())
    assert store.created == [(FIELD, SPEC, {"encoder": enc})]
    got = rag.search("net profit", 3, rerank=True, rerank_with="late", fetch_k=8)
    assert store.reranks == [(["net profit"], [[0, 1, 2, 3, 4, 5, 6, 7]])]
    assert [c["text"] for c in got] == ["text 1", "text 2", "text 4"]      # MaxSim descending, then retrieval order
    assert [c["rerank_score"] for c in got] == [3.0, 3.0, 2.0] and [c["rank"] for c in got] == [1, 2, 3]
    assert [c["score"] for c in got] == [0.9, 0.8, 0.6]                   # `score` stays the cosine
    batch = rag.search_batch(["net profit", "eps"], 3, rerank=True, rerank_with="late", fetch_k=8)
    assert store.reranks[-1] == (["net profit", "eps"], [[0, 1, 2, 3, 4, 5, 6, 7]] * 2) and len(store.reranks) == 2
    assert batch == [got, got]
    # the default stays the cross-encoder, and its call is the call of before
    n = len(store.reranks)
    a = rag.search("net profit", 3, rerank=True, fetch_k=8)
    b = rag.search("net profit", 3, rerank=True, fetch_k=8, rerank_with="cross")
    assert a == b and len(store.reranks) == n and store.searches[-1] == store.searches[-2]
    plain_store = RecordingStore()
    plain = VectorRAG("k", embedder=FakeEmbedder(), store=plain_store, reranker=FakeCross())
    assert plain_store.created == [] and plain.search("net profit", 3, rerank=True, fetch_k=8) == a
    for kw in (dict(rerank=True, rerank_with="late"), dict(rerank=True, rerank_with="colbert")):
        with pytest.raises(ValueError):
            plain.search("q", 3, **kw)
        with pytest.raises(ValueError):
            plain.search_batch(["q"], 3, **kw)
    with pytest.raises(ValueError, match="late encoder"):
        plain.search("q", 3, rerank=True, rerank_with="late")
    with pytest.raises(ValueError, match="rerank=True"):
        rag.search("q", 3, rerank_with="late")
    late_only = VectorRAG("k", embedder=FakeEmbedder(), store=RecordingStore(), late_encoder=enc)   # no cross-encoder
    assert [c["text"] for c in late_only.search("q", 2, rerank=True, rerank_with="late", fetch_k=8)] == ["text 1", "text 2"]
    with pytest.raises(ValueError, match="reranker"):
        late_only.search("q", 2, rerank=True)


class FakeRag:
    def __init__(self):
        self.calls = []

    def search(self, query, top_k=3, expr=None, **kw):
        self.calls.append((query, top_k, expr, kw))
        return []


def test_mcp_tool_and_rest_body_forward_rerank_with_only_when_given(monkeypatch):
    from rag_fin_amd import service
    from rag_fin_amd.adapter import SearchRequest, search_args
    rag = FakeRag()
    mcp_server.set_rag(rag)
    try:
        mcp_server.search_vectors("net interest income", 4, rerank=True, rerank_with="late")
        assert rag.calls[-1] == ("net interest income", 4, None, {"rerank": True, "rerank_with": "late"})
        mcp_server.search_vectors("q", 4, filter="id == 1", rerank=True, rerank_with="cross", fetch_k=32)
        assert rag.calls[-1] == ("q", 4, "id == 1", {"fetch_k": 32, "rerank": True, "rerank_with": "cross"})
        mcp_server.search_vectors("q", 2, rerank=True)                   # the calls of before
        assert rag.calls[-1] == ("q", 2, None, {"rerank": True})
        mcp_server.search_vectors("q", 2, filter="id == 1")
        assert rag.calls[-1] == ("q", 2, "id == 1", {})
        mcp_server.set_rag(VectorRAG("k", embedder=FakeEmbedder(), store=RecordingStore()))
        r = mcp_server.search_vectors("q", 3, rerank=True, rerank_with="late")
        assert r["status"] == "error" and "late encoder" in r["message"]
    finally:
        mcp_server.set_rag(None)
    assert search_args(SearchRequest(query="hello", top_k=4)) == {"query": "hello", "top_k": 4}
    assert search_args(SearchRequest(query="hello", rerank=True)) == {"query": "hello", "top_k": 3, "rerank": True}
    assert search_args(SearchRequest(query="hello", rerank=True, rerank_with="late")) == \
        {"query": "hello", "top_k": 3, "rerank_with": "late", "rerank": True}
    # COLBERT_MODEL_DIR reaches build_rag, and only when it is set
    seen = []
    monkeypatch.setattr(service, "build_rag", lambda *a, **kw: seen.append(kw))
    monkeypatch.setenv("RAGFIN_MODEL_DIR", "/models/minilm")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("COLBERT_MODEL_DIR", raising=False)
    service.build_rag_from_env()
    assert "late_dir" not in seen[-1]
    monkeypatch.setenv("COLBERT_MODEL_DIR", "/models/colbert")
    service.build_rag_from_env()
    assert seen[-1]["late_dir"] == "/models/colbert"
