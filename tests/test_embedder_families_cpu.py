"""Sentence-embedder families without a GPU: what a sentence-transformers directory says about its own ends
(sentence_config), the numpy definition of the pooling head (pool_reference) against sentence-transformers' Pooling
and Normalize arithmetic restated with torch ops (the package itself is not installed), the prompt rules, how the
query / document prompt travels through VectorRAG and service.ingest, the store's metric, and the host-side refusals
of rf_encode_sentences."""
import ctypes
import json
import os

import numpy as np
import pytest

from rag_fin_amd import _lib
from rag_fin_amd.embedder import Embedder, check_pooling, pool_reference, sentence_config
from rag_fin_amd.tokenizer import WordPieceTokenizer

ST = "sentence_transformers.models."
FLAGS = {"cls": "pooling_mode_cls_token", "mean": "pooling_mode_mean_tokens", "max": "pooling_mode_max_tokens",
         "mean_sqrt_len": "pooling_mode_mean_sqrt_len_tokens", "weightedmean": "pooling_mode_weightedmean_tokens",
         "lasttoken": "pooling_mode_lasttoken"}


def write_dir(tmp_path, modes=("mean",), normalize=True, extra_modules=(), st_config=None, dim=384, hidden=384,
              include_prompt=None, modules=True, name="m"):
    d = tmp_path / name
    (d / "1_Pooling").mkdir(parents=True)
    (d / "config.json").write_text(json.dumps({"hidden_size": hidden}))
    if modules:
        mods = [{"idx": 0, "name": "0", "path": "", "type": ST + "Transformer"},
                {"idx": 1, "name": "1", "path": "1_Pooling", "type": ST + "Pooling"}]
        mods += [{"idx": len(mods) + i, "name": str(2 + i), "path": f"{2 + i}_X", "type": ST + t}
                 for i, t in enumerate(extra_modules)]
        if normalize:
            mods.append({"idx": len(mods), "name": str(len(mods)), "path": f"{len(mods)}_Normalize", "type": ST + "Normalize"})
        (d / "modules.json").write_text(json.dumps(mods))
    pc = {"word_embedding_dimension": dim, **{flag: mode in modes for mode, flag in FLAGS.items()}}
    if include_prompt is not None:
        pc["include_prompt"] = include_prompt
    (d / "1_Pooling" / "config.json").write_text(json.dumps(pc))
    if st_config is not None:
        (d / "config_sentence_transformers.json").write_text(json.dumps(st_config))
    return str(d)


# ---- the loader ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["cls", "mean", "max", "mean_sqrt_len"])
def test_every_offered_pooling_mode_resolves(tmp_path, mode):
    sc = sentence_config(write_dir(tmp_path, modes=(mode,)))
    assert sc["pooling"] == mode and sc["normalize"] is True and sc["include_prompt"] is True
    assert sc["prompts"] == {} and sc["default_prompt_name"] is None and sc["similarity_fn_name"] is None


def test_plain_directory_missing_normalize_and_the_sentence_transformers_config(tmp_path):
    sc = sentence_config(write_dir(tmp_path, modes=("cls",), modules=False, name="plain"))
    assert (sc["pooling"], sc["normalize"]) == ("mean", True)          # no modules.json: today's behaviour
    sc = sentence_config(write_dir(tmp_path, modes=("mean",), normalize=False, include_prompt=False, name="dot", st_config={
        "prompts": {"query": "q: ", "passage": "p: "}, "default_prompt_name": "query", "similarity_fn_name": "dot"}))
    assert sc == {"pooling": "mean", "normalize": False, "include_prompt": False,
                  "prompts": {"query": "q: ", "passage": "p: "}, "default_prompt_name": "query",
                  "similarity_fn_name": "dot"}


@pytest.mark.parametrize("kw,msg", [
    (dict(modes=("cls", "mean")), "exactly one"),
    (dict(modes=()), "exactly one"),
    (dict(modes=("weightedmean",)), "weightedmean"),
    (dict(modes=("mean", "lasttoken")), "lasttoken"),
    (dict(extra_modules=("Dense",)), "sentence_transformers.models.Dense"),
    (dict(extra_modules=("LayerNorm",)), "LayerNorm"),
    (dict(dim=768), "word_embedding_dimension 768"),
])
def test_loader_refusals(tmp_path, kw, msg):
    with pytest.raises(ValueError, match=msg):
        sentence_config(write_dir(tmp_path, **kw))


def test_module_order_is_checked(tmp_path):
    d = write_dir(tmp_path)
    mods = json.load(open(os.path.join(d, "modules.json")))
    mods[1]["idx"], mods[2]["idx"] = 2, 1                              # Transformer, Normalize, Pooling
    json.dump(mods, open(os.path.join(d, "modules.json"), "w"))
    with pytest.raises(ValueError, match="expected Transformer, Pooling"):
        sentence_config(d)


def bare(pooling=None, normalize=None, prompts=None, default_prompt_name=None, include_prompt=None, tokenizer=None,
         max_seq_length=16):
    """An Embedder without a device: the ends and the prompt rules read attributes only."""
    e = Embedder.__new__(Embedder)
    e._set_ends(pooling, normalize, prompts, default_prompt_name, include_prompt)
    e.tokenizer, e.max_seq_length, e.dim = tokenizer, max_seq_length, 384
    return e


def test_keyword_overrides_win_over_the_directory(tmp_path, monkeypatch):
    import safetensors.numpy
    from rag_fin_amd import embedder as E
    d = write_dir(tmp_path, modes=("cls",), st_config={"prompts": {"query": "q: "}, "default_prompt_name": "query",
                                                       "similarity_fn_name": "cosine"})
    seen = {}
    monkeypatch.setattr(safetensors.numpy, "load_file", lambda p: {})
    monkeypatch.setattr(E, "hf_encoder_config", lambda hc: dict(E.MINILM_L6))
    monkeypatch.setattr(E, "stack_hf_state_dict", lambda sd, cfg: {})
    monkeypatch.setattr(E.WordPieceTokenizer, "from_vocab_file", classmethod(lambda cls, p: None))
    monkeypatch.setattr(Embedder, "__init__", lambda self, w, cfg, tok, dev, msl, **kw: seen.update(kw, msl=msl))
    Embedder.from_local(d)
    assert seen == dict(pooling="cls", normalize=True, prompts={"query": "q: "}, default_prompt_name="query",
                        include_prompt=True, similarity_fn_name="cosine", msl=256)
    Embedder.from_local(d, pooling="max", normalize=False, prompts={"query": "query: ", "document": "passage: "},
                        include_prompt=False, max_seq_length=64)
    assert seen == dict(pooling="max", normalize=False, prompts={"query": "query: ", "document": "passage: "},
                        default_prompt_name="query", include_prompt=False, similarity_fn_name="cosine", msl=64)
    Embedder.from_local(d, prompts={"document": "passage: "})           # the directory's default names a dropped prompt
    assert seen["default_prompt_name"] is None
    Embedder.from_local(d, prompts={"document": "passage: "}, default_prompt_name="document")
    assert seen["default_prompt_name"] == "document"


def test_constructor_defaults_and_checks():
    e = bare()
    assert (e.pooling, e.normalize, e.prompts, e.include_prompt) == ("mean", True, {}, True)
    assert e.query_prompt is None and e.document_prompt is None and e.similarity_fn_name is None
    assert bare(pooling="CLS").pooling == "cls" and check_pooling("mean-sqrt-len") == "mean_sqrt_len"
    for bad in ("weightedmean", "lasttoken", "median"):
        with pytest.raises(ValueError, match=bad):
            bare(pooling=bad)
    with pytest.raises(ValueError, match="default_prompt_name"):
        bare(prompts={"query": "q: "}, default_prompt_name="doc")
    assert bare(prompts={"query": "q: ", "corpus": "c: ", "passage": "p: "}).document_prompt == "p: "
    assert bare(prompts={"document": "d: ", "passage": "p: "}).document_prompt == "d: "


# ---- pool_reference against sentence-transformers' arithmetic ------------------------------------------------------
def st_pooling(hidden, mask, mode, normalize):
    """sentence_transformers.models.Pooling.forward + Normalize.forward on an attention mask that leaves the
    excluded prompt tokens out (what include_prompt = False does to it), restated."""
    import torch
    m = mask.unsqueeze(-1).expand(hidden.size()).to(hidden.dtype)
    if mode == "cls":
        out = hidden[:, 0]
    elif mode == "max":
        h = hidden.clone()
        h[m == 0] = -1e9
        out = torch.max(h, 1)[0]
    else:
        s = torch.sum(hidden * m, 1)
        n = torch.clamp(m.sum(1), min=1e-9)
        out = s / n if mode == "mean" else s / torch.sqrt(n)
    return torch.nn.functional.normalize(out, p=2, dim=1) if normalize else out


@pytest.mark.parametrize("mode", ["mean", "cls", "max", "mean_sqrt_len"])
@pytest.mark.parametrize("normalize", [True, False])
def test_pool_reference_is_sentence_transformers_arithmetic(mode, normalize):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    T, H = 12, 384
    lens = np.repeat(np.arange(1, T + 1), T)                            # every (len, skip) with skip < len
    skip = np.tile(np.arange(T), T)
    keep = skip < lens
    lens, skip = lens[keep], skip[keep]
    hidden = rng.standard_normal((len(lens), T, H)).astype(np.float32)
    pos = np.arange(T)[None, :]
    mask = ((pos >= skip[:, None]) & (pos < lens[:, None])).astype(np.int64)
    want = st_pooling(torch.from_numpy(hidden), torch.from_numpy(mask), mode, normalize).numpy()
    got = pool_reference(hidden, lens, skip, mode, normalize)
    assert got.dtype == np.float64 and got.shape == want.shape
    # fp32 rounding of sums of <= 12 values of order 1 (and of a unit vector's components)
    assert np.abs(got - want).max() < 12 * 4 * 2.0 ** -24 * max(1.0, np.abs(want).max())
    if mode == "cls":
        assert np.array_equal(got, pool_reference(hidden, lens, None, mode, normalize))


def test_pool_reference_empty_sets_are_zero():
    h = np.ones((2, 4, 384))
    for mode in ("mean", "max", "mean_sqrt_len"):
        out = pool_reference(h, [3, 0], [3, 0], mode, True)
        assert out.shape == (2, 384) and not out.any()
    assert pool_reference(h, [3, 0], [3, 0], "cls", False)[0].all() and not pool_reference(h, [3, 0], None, "cls", False)[1].any()


# ---- prompts ------------------------------------------------------------------------------------------------------
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "q", ":", "query", "passage", "hello", "world", "p"]


def test_prompt_precedence_and_unknown_names():
    e = bare(prompts={"query": "q: ", "passage": "p: "}, default_prompt_name="passage")
    assert e._resolve_prompt() == "p: "                                # default_prompt_name
    assert e._resolve_prompt(prompt_name="query") == "q: "             # prompt_name over the default
    assert e._resolve_prompt(prompt_name="query", prompt="x: ") == "x: "   # prompt over both
    with pytest.raises(ValueError, match=r"'nope'.*passage, query"):
        e._resolve_prompt(prompt_name="nope")
    assert bare()._resolve_prompt() is None
    with pytest.raises(ValueError, match="none are set"):
        bare()._resolve_prompt(prompt_name="query")


class Rows:
    def __init__(self, n):
        self.n = n

    def cpu(self):
        return self

    def numpy(self):
        return np.zeros((self.n, 384), np.float32)


def recording(e):
    calls = []

    def encode_to_device(sentences, batch_tokens=65536, out_dtype="float16", **kw):
        calls.append((list(sentences), out_dtype, kw))
        return Rows(len(sentences))
    e.encode_to_device = encode_to_device
    return calls


def test_encode_passes_prompt_and_normalisation_and_the_named_forms_look_their_prompt_up():
    e = bare(prompts={"query": "q: ", "passage": "p: "}, normalize=False)
    calls = recording(e)
    assert e.encode(["a", "b"]).shape == (2, 384) and calls[-1] == (["a", "b"], "float32", {})
    assert e.encode("a").shape == (384,)
    e.encode(["a"], prompt_name="query", normalize_embeddings=True, convert_to_numpy=True, show_progress_bar=False)
    assert calls[-1][2] == {"prompt": "q: ", "normalize": True}
    e.encode(["a"], normalize_embeddings=False)
    assert calls[-1][2] == {}
    e.encode_query(["a"])
    assert calls[-1][2] == {"prompt": "q: "}
    e.encode_document(["a"])
    assert calls[-1][2] == {"prompt": "p: "}
    e.encode_query(["a"], prompt="x: ")
    assert calls[-1][2] == {"prompt": "x: "}
    e.encode_document(["a"], prompt_name="query")
    assert calls[-1][2] == {"prompt": "q: "}
    with pytest.raises(ValueError, match="nope"):
        e.encode(["a"], prompt_name="nope")
    plain = bare()
    calls = recording(plain)
    plain.encode_query(["a"])
    plain.encode_document(["a"])
    assert [c[2] for c in calls] == [{}, {}]


def test_skip_is_the_prompts_tokens_less_its_sep():
    tok = WordPieceTokenizer(VOCAB)
    assert tok.encode("q: ", 64) == [2, 5, 6, 3]
    assert bare(prompts={"query": "q: "}, include_prompt=False, tokenizer=tok)._prompt_skip("q: ") == 3
    assert bare(include_prompt=False, pooling="max", tokenizer=tok)._prompt_skip("query: passage: ") == 5
    assert bare(include_prompt=True, tokenizer=tok)._prompt_skip("q: ") is None        # the prompt is pooled
    assert bare(include_prompt=False, pooling="cls", tokenizer=tok)._prompt_skip("q: ") is None   # CLS reads token 0
    assert bare(include_prompt=False, tokenizer=tok)._prompt_skip("") is None
    assert bare(include_prompt=False, tokenizer=tok)._prompt_skip(None) is None
    # [CLS] q : + one text token + [SEP] = 5: fits 5, not 4 -- whatever include_prompt says
    assert bare(include_prompt=False, tokenizer=tok, max_seq_length=5)._prompt_skip("q: ") == 3
    for inc in (True, False):
        with pytest.raises(ValueError, match="no room"):
            bare(include_prompt=inc, tokenizer=tok, max_seq_length=4)._prompt_skip("q: ")


@pytest.mark.parametrize("include_prompt,pooling,skips", [(False, "mean", True), (True, "mean", False), (False, "cls", False)])
def test_prompt_is_prepended_before_tokenisation_and_skip_reaches_the_forward(include_prompt, pooling, skips):
    torch = pytest.importorskip("torch")
    tok = WordPieceTokenizer(VOCAB)
    e = bare(pooling=pooling, include_prompt=include_prompt, tokenizer=tok, max_seq_length=16)
    e.device = torch.device("cpu")
    calls = []

    def encode_ids(ids, lens, out_dtype="float16", **kw):
        calls.append((np.asarray(ids), np.asarray(lens), kw))
        return torch.zeros((len(lens), 384), dtype=torch.float16)
    e.encode_ids = encode_ids
    out = e.encode_to_device(["hello world", "world"], prompt="q: ", normalize=True)
    assert out.shape == (2, 384)
    ids, lens, kw = calls[-1]
    assert ids[0, :lens[0]].tolist() == tok.encode("q: hello world", 16) == [2, 5, 6, 9, 10, 3]
    assert ids[1, :lens[1]].tolist() == [2, 5, 6, 10, 3]
    assert kw.pop("normalize") is True
    if skips:
        assert kw["skip"].tolist() == [3, 3] and kw["skip"].dtype == np.int32 and (lens > kw["skip"]).all()
    else:
        assert kw == {}
    e.encode_to_device(["hello"])                                       # no prompt: the call of before
    assert calls[-1][2] == {} and calls[-1][0][0, :3].tolist() == [2, 9, 3]
    with pytest.raises(ValueError, match="no room"):
        e.encode_to_device(["hello"], prompt="q: " * 8)


# ---- plumbing -----------------------------------------------------------------------------------------------------
class Hit:
    def __init__(self):
        self.score = 1.0
        self.entity = type("E", (), dict(text="t", period="p", chunk_type="c", statement_type="s", primary_value=1.0))()


class Store:
    schema = ()

    def __init__(self, metric_type=None):
        if metric_type:
            self.metric_type = metric_type
        self.params, self.inserted = [], []

    num_entities = 1

    def load(self):
        pass

    def flush(self):
        pass

    def search(self, data, anns_field, param, limit, **kw):
        self.params.append(param)
        return [[Hit()] for _ in range(len(data))]

    def insert(self, cols):
        self.inserted.append(cols)
        return len(cols[0])


class OldEmbedder:
    """Today's signatures: no prompt keyword anywhere."""
    def __init__(self):
        self.calls = []

    def encode(self, texts):
        self.calls.append(("encode", list(texts)))
        return np.zeros((len(texts), 4), np.float32)


class OldDeviceEmbedder(OldEmbedder):
    def encode_to_device(self, texts):
        self.calls.append(("device", list(texts)))
        return np.zeros((len(texts), 4), np.float32)


class PromptEmbedder:
    def __init__(self, query_prompt=None, document_prompt=None):
        self.query_prompt, self.document_prompt, self.calls = query_prompt, document_prompt, []
        self.pooling, self.normalize, self.prompts = "cls", True, {"query": query_prompt} if query_prompt else {}

    def encode_to_device(self, texts, **kw):
        self.calls.append((list(texts), kw))
        return np.zeros((len(texts), 4), np.float32)


def chunks(n):
    return [dict(id=f"c{i}", text=f"text {i}", period="Q1_FY2024", chunk_type="t", statement_type="s",
                 primary_value=float(i)) for i in range(n)]


def test_queries_and_chunks_carry_their_prompt_only_when_the_embedder_has_one():
    from rag_fin_amd.rag import VectorRAG
    from rag_fin_amd.service import ingest
    e = PromptEmbedder("q: ", "p: ")
    rag = VectorRAG("k", embedder=e, store=Store())
    rag.search("profit", 1)
    assert e.calls[-1] == (["profit"], {"prompt": "q: "})
    rag.search_batch(["a", "b"], 1)
    assert e.calls[-1] == (["a", "b"], {"prompt": "q: "})
    ingest(Store(), e, chunks(2))
    assert e.calls[-1] == (["text 0", "text 1"], {"prompt": "p: "})
    for empty in (PromptEmbedder(), PromptEmbedder("", "")):
        VectorRAG("k", embedder=empty, store=Store()).search("profit", 1)
        ingest(Store(), empty, chunks(1))
        assert [kw for _, kw in empty.calls] == [{}, {}]
    # doubles with today's signatures keep working
    for old, kind in ((OldEmbedder(), "encode"), (OldDeviceEmbedder(), "device")):
        VectorRAG("k", embedder=old, store=Store()).search("profit", 1)
        assert old.calls == [(kind, ["profit"])]
    old = OldDeviceEmbedder()
    assert ingest(Store(), old, chunks(2)) == 2 and old.calls == [("device", ["text 0", "text 1"])]


def test_search_asks_for_the_stores_metric_and_health_check_reports_the_ends():
    from rag_fin_amd.rag import VectorRAG
    rag = VectorRAG("k", embedder=PromptEmbedder("q: "), store=Store("IP"))
    rag.search("profit", 1)
    rag.search("profit", 1, min_score=0.5)
    assert rag.collection.params == [{"metric_type": "IP"}, {"metric_type": "IP", "params": {"radius": 0.5}}]
    h = rag.health_check()
    assert (h["pooling"], h["normalize"], h["prompts"]) == ("cls", True, True)
    plain = VectorRAG("k", embedder=OldEmbedder(), store=Store())
    plain.search("profit", 1)
    assert plain.collection.params == [{"metric_type": "COSINE"}]
    assert list(plain.health_check()) == ["status", "milvus", "gemini", "collection", "total_chunks"]


def test_build_rag_picks_the_metric_from_the_model_and_takes_the_overrides(monkeypatch, tmp_path):
    from rag_fin_amd import chunker, embedder, service
    from rag_fin_amd import store as store_mod
    made = {}

    class S(Store):
        def __init__(self, name, dim, device=None, metric_type="COSINE", **kw):
            Store.__init__(self, metric_type)
            made["metric"] = metric_type

    class E:
        dim = 8
        similarity_fn_name = None

        @classmethod
        def from_local(cls, model_dir, device=None, **kw):
            made["kw"] = kw
            return cls()

    monkeypatch.setattr(embedder, "Embedder", E)
    monkeypatch.setattr(store_mod, "CorpusStore", S)
    monkeypatch.setattr(chunker, "build_all_chunks", lambda data_dir: [])
    d = write_dir(tmp_path, st_config={"prompts": {"query": "q: ", "passage": "p: "}})
    service.build_rag(d, "x")
    assert made == {"metric": "COSINE", "kw": {}}
    for name, want in (("dot", "IP"), ("cosine", "COSINE")):
        E.similarity_fn_name = name
        service.build_rag(d, "x")
        assert made["metric"] == want
    for name in ("euclidean", "manhattan"):
        E.similarity_fn_name = name
        with pytest.raises(ValueError, match="no L2 metric"):
            service.build_rag(d, "x")
    service.build_rag(d, "x", metric="IP")                              # an explicit metric wins over the model's
    assert made["metric"] == "IP"
    E.similarity_fn_name = "dot"
    service.build_rag(d, "x", metric="COSINE", query_prompt="query: ", pooling="cls")
    assert made == {"metric": "COSINE", "kw": {"prompts": {"query": "query: ", "passage": "p: "}, "pooling": "cls"}}
    with pytest.raises(ValueError, match="COSINE or IP"):
        service.build_rag(d, "x", metric="hamming")
    # the environment reaches build_rag, and only what is set
    seen = []
    monkeypatch.setattr(service, "build_rag", lambda *a, **kw: seen.append(kw))
    monkeypatch.setenv("RAGFIN_MODEL_DIR", d)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k in ("RAGFIN_QUERY_PROMPT", "RAGFIN_DOCUMENT_PROMPT", "RAGFIN_POOLING", "RAGFIN_METRIC"):
        monkeypatch.delenv(k, raising=False)
    service.build_rag_from_env()
    assert not {"query_prompt", "document_prompt", "pooling", "metric"} & set(seen[-1])
    monkeypatch.setenv("RAGFIN_QUERY_PROMPT", "query: ")
    monkeypatch.setenv("RAGFIN_DOCUMENT_PROMPT", "passage: ")
    monkeypatch.setenv("RAGFIN_POOLING", "cls")
    monkeypatch.setenv("RAGFIN_METRIC", "IP")
    service.build_rag_from_env()
    assert {k: seen[-1][k] for k in ("query_prompt", "document_prompt", "pooling", "metric")} == \
        {"query_prompt": "query: ", "document_prompt": "passage: ", "pooling": "cls", "metric": "IP"}


# ---- the ABI ------------------------------------------------------------------------------------------------------
def test_abi_declares_binds_and_refuses_on_the_host():
    lib = _lib.load_library()
    assert "rf_encode_sentences" in _lib.SIGNATURES and hasattr(lib, "rf_encode_sentences")
    assert (_lib.RF_POOL_MEAN, _lib.RF_POOL_CLS, _lib.RF_POOL_MAX, _lib.RF_POOL_MEAN_SQRT_LEN) == (0, 1, 2, 3)
    assert ctypes.sizeof(_lib.SentenceHead) == 8
    p = ctypes.c_void_p(4096)                          # never dereferenced: every call below is refused on the host

    def call(enc=p, ids=p, lens=p, skip=None, head=(0, 1), o16=p, o32=p, ws=p):
        h = None if head is None else ctypes.byref(_lib.SentenceHead(*head))
        return lib.rf_encode_sentences(enc, ids, lens, skip, 1, 8, h, o16, o32, ws, 1 << 20, None)
    bad = [dict(enc=None), dict(ids=None), dict(lens=None), dict(head=None), dict(ws=None), dict(o16=None, o32=None),
           dict(head=(-1, 1)), dict(head=(4, 0)), dict(head=(99, 1))]
    for kw in bad:
        assert call(**kw) == -1, kw                    # RF_ERR_INVALID
        assert b"rf_encode_sentences" in lib.rf_last_error()
