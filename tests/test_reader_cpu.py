"""The extractive reader, the parts that need no GPU:
  * the fp64 numpy mirror of a reader forward (mirror_hidden of tests/test_rerank_cpu.py, then the span head),
    pinned to the in-container transformers.BertForQuestionAnswering through the state-dict mapping the product
    loads checkpoints with;
  * span_reference, the numpy definition of the device's decode, against a brute-force triple loop;
  * token -> character offsets against transformers.BertTokenizerFast;
  * the surfaces (VectorRAG, MCP tool) with a fake reader.
tests/test_reader_gpu.py compares rf_answer_spans with the same mirror and the same span_reference."""
import numpy as np
import pytest

from oracle import encoder as oenc
from rag_fin_amd import mcp_server
from rag_fin_amd.rag import VectorRAG
from rag_fin_amd.reader import span_reference
from test_rerank_cpu import FakeEmbedder, FakeStore, mirror_hidden


# ---- the mirror ---------------------------------------------------------------------------------------------------
def mirror_qa_logits(w, head, cfg, ids, lens, seg, dtype=np.float64):
    """Start / end logit per position: token types 1 from seg[b] on, the layers, x @ qa_w.T + qa_b.
    -> [B, T, 2] (positions >= len hold the values of padding rows: not part of any contract)."""
    type_ids = (np.arange(ids.shape[1])[None, :] >= np.asarray(seg)[:, None]).astype(np.int64)
    x = mirror_hidden(w, cfg, ids, lens, type_ids, dtype)
    return x @ head["qa_w"].astype(dtype).T + head["qa_b"].astype(dtype)


def test_mirror_and_state_dict_mapping_match_transformers():
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    from rag_fin_amd.embedder import stack_hf_qa_head, stack_hf_state_dict
    cfg = dict(oenc.MINILM_L6, layers=2, vocab_size=211, max_position=48)
    torch.manual_seed(11)
    hc = transformers.BertConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"],
                                 num_attention_heads=cfg["heads"], intermediate_size=cfg["intermediate"],
                                 max_position_embeddings=cfg["max_position"], type_vocab_size=2,
                                 hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                 layer_norm_eps=cfg["ln_eps"])
    model = transformers.BertForQuestionAnswering(hc)
    with torch.no_grad():   # the default init leaves biases at 0 and LayerNorm at (1, 0): move them
        for name, p in model.named_parameters():
            if name.endswith("bias") or "LayerNorm" in name:
                p.add_(0.1 * torch.randn_like(p))
    model = model.double().eval()
    sd = {k: v.detach().numpy() for k, v in model.state_dict().items()}
    w, head = stack_hf_state_dict(sd, cfg), stack_hf_qa_head(sd)
    assert head["qa_w"].shape == (2, 384) and head["qa_b"].shape == (2,) and head["qa_w"].dtype == np.float32
    rng = np.random.default_rng(1)
    B, T = 6, 33
    lens = np.array([33, 20, 9, 3, 12, 33])
    seg = np.array([10, 5, 4, 2, 12, 32])
    ids = rng.integers(1, cfg["vocab_size"], (B, T))
    pos = np.arange(T)[None, :]
    with torch.no_grad():
        out = model(input_ids=torch.as_tensor(ids), attention_mask=torch.as_tensor((pos < lens[:, None]).astype(np.int64)),
                    token_type_ids=torch.as_tensor((pos >= seg[:, None]).astype(np.int64)))
    got = mirror_qa_logits(w, head, cfg, ids, lens, seg)
    assert got.shape == (B, T, 2)
    live = pos < lens[:, None]
    assert np.abs(got[..., 0] - out.start_logits.numpy())[live].max() < 1e-9
    assert np.abs(got[..., 1] - out.end_logits.numpy())[live].max() < 1e-9
    # row 0 is the start logit's and row 1 the end logit's: swapped, the two differ by far more than that
    assert np.abs(got[..., 1] - out.start_logits.numpy())[live].max() > 1e-3
    with pytest.raises(KeyError, match="qa_outputs.bias"):
        stack_hf_qa_head({k: v for k, v in sd.items() if k != "qa_outputs.bias"})
    with pytest.raises(KeyError, match="qa_outputs.weight"):
        stack_hf_qa_head({})


def test_random_qa_head_is_seeded_and_shaped():
    from rag_fin_amd.reader import random_qa_head
    a, b = random_qa_head(384, 5, head_scale=0.1), random_qa_head(384, 5, head_scale=0.1)
    assert a["qa_w"].shape == (2, 384) and a["qa_b"].shape == (2,)
    assert all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
    assert not np.array_equal(a["qa_w"], random_qa_head(384, 6, head_scale=0.1)["qa_w"])


# ---- the decode ---------------------------------------------------------------------------------------------------
def brute_force(s, e, seg, length, max_answer_len, n_best):
    cands = []
    for i in range(max(seg, 0), length - 1):
        for j in range(i, length - 1):
            if j - i + 1 <= max_answer_len:
                cands.append((i, j, np.float32(s[i]) + np.float32(e[j])))
    picked = []
    for _ in range(n_best):       # selection, not a sort: the best remaining by (z desc, i asc, j asc)
        best = None
        for c in cands:
            if c in picked:
                continue
            if best is None or c[2] > best[2] or (c[2] == best[2] and (c[0], c[1]) < (best[0], best[1])):
                best = c
        picked.append(best if best is not None else (-1, -1, np.float32(-np.inf)))
    members = sorted({0} | set(range(max(seg, 0), length - 1)))
    lse = [float(np.log(np.sum(np.exp(np.asarray(v, dtype=np.float64)[members])))) for v in (s, e)]
    return picked, np.float32(s[0]) + np.float32(e[0]), lse[0], lse[1]


def same_decode(got, want):
    assert len(got[0]) == len(want[0])
    for a, b in zip(got[0], want[0]):
        assert (a[0], a[1]) == (b[0], b[1]), (got[0], want[0])
        assert np.float32(a[2]).view(np.uint32) == np.float32(b[2]).view(np.uint32)
        assert isinstance(a[2], np.float32)
    assert np.float32(got[1]).view(np.uint32) == np.float32(want[1]).view(np.uint32)
    assert abs(got[2] - want[2]) < 1e-12 and abs(got[3] - want[3]) < 1e-12


@pytest.mark.parametrize("case", [
    dict(T=14, seg=4, length=14, L=4, n=5),
    dict(T=14, seg=4, length=11, L=30, n=16),
    dict(T=9, seg=1, length=9, L=1, n=3),          # max_answer_len = 1: i == j
    dict(T=8, seg=5, length=8, L=3, n=16),         # 2 context tokens, 3 candidates < n_best
    dict(T=8, seg=6, length=8, L=3, n=4),          # a context of one token
    dict(T=8, seg=7, length=8, L=3, n=4),          # seg == length - 1: empty context
    dict(T=8, seg=8, length=8, L=3, n=2),          # seg == length: no second segment
    dict(T=5, seg=1, length=2, L=3, n=2),          # fewer than three tokens
    dict(T=12, seg=0, length=12, L=5, n=6),        # seg = 0: [CLS] is part of the context, counted once
])
def test_span_reference_equals_the_brute_force(case):
    rng = np.random.default_rng(case["T"] * 100 + case["seg"])
    s = rng.standard_normal(case["T"]).astype(np.float32) * 3
    e = rng.standard_normal(case["T"]).astype(np.float32) * 3
    args = (s, e, case["seg"], case["length"], case["L"], case["n"])
    same_decode(span_reference(*args), brute_force(*args))


def test_span_reference_orders_exact_ties_by_start_then_end():
    z = np.zeros(10, dtype=np.float32)
    spans, z_null, ls, le = span_reference(z, z, 3, 10, 3, 7)
    assert [(i, j) for i, j, _ in spans] == [(3, 3), (3, 4), (3, 5), (4, 4), (4, 5), (4, 6), (5, 5)]
    assert all(v == 0 and isinstance(v, np.float32) for _, _, v in spans) and z_null == 0
    assert abs(ls - np.log(7)) < 1e-15 and abs(le - np.log(7)) < 1e-15      # [CLS] + 6 context tokens
    same_decode(span_reference(z, z, 3, 10, 3, 7), brute_force(z, z, 3, 10, 3, 7))
    # ties between a few values only: quantised logits
    rng = np.random.default_rng(0)
    s, e = (rng.integers(0, 3, 20).astype(np.float32) for _ in range(2))
    same_decode(span_reference(s, e, 5, 20, 6, 16), brute_force(s, e, 5, 20, 6, 16))


def test_span_reference_empty_cases():
    s = np.arange(6, dtype=np.float32)
    spans, z_null, ls, le = span_reference(s, -s, 5, 6, 4, 3)
    assert spans == [(-1, -1, np.float32(-np.inf))] * 3 and z_null == 0
    assert ls == float(s[0]) and le == float(-s[0])                          # the set is {0}
    spans, z_null, ls, le = span_reference(s, s, 2, 0, 4, 2)                 # no tokens: no [CLS] slot
    assert spans == [(-1, -1, np.float32(-np.inf))] * 2 and z_null == -np.inf and ls == -np.inf and le == -np.inf


# ---- offsets ------------------------------------------------------------------------------------------------------
OFFSET_VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "net", "profit", "cafe", "resume", "uber", "q", "##1",
                "fy", "##20", "##24", "un", "##aff", "##able", "the", "was", "rs", "11", "##05", "##9", "crore", ".",
                ",", "!", "?", "(", ")", "-", "%", "$", "'", "\u2014", "\u4e2d", "\u6587", "\u9280", "in", "up", "##s",
                "naive", "a", "b", "##b", "ab", "##cd", "abcd", "x"]
OFFSET_TEXTS = [
    "Net profit was Rs. 11059 crore in Q1 FY2024!",
    "  leading and   trailing \t\n whitespace  ",
    "Caf\xe9 R\xe9sum\xe9 \xdcBER na\xefve",                      # precomposed accents, mixed case
    "cafe\u0301 re\u0301sume\u0301 Cafe\u0301x",                           # combining marks: they vanish
    "\u4e2d\u6587net\u9280profit \u4e2d \u6587",                           # CJK: every ideograph a word
    "(net)--profit?!,$%'x'",                                                     # punctuation clusters
    "profit\u2014net \u2014 up",                                           # non-ASCII punctuation
    "ab\x00cd a\x07b \x7fnet\u200b profit\ufffdx",                         # control / format characters vanish
    "net profit\xa0was\u3000the",                                        # non-ASCII whitespace
    "unaffable zzzz unaffzzz profits ups qqqq1",                                 # continuation pieces, unknown words
    "",
    "   ",
    "\u0301\u0301 net",                                                    # a word of marks alone: no token
    "NET PROFIT WAS " * 12,                                                      # truncates at max_length 16
]


@pytest.fixture(scope="module")
def offset_rig(tmp_path_factory):
    transformers = pytest.importorskip("transformers")
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    path = tmp_path_factory.mktemp("offsets") / "vocab.txt"
    path.write_text("\n".join(OFFSET_VOCAB) + "\n", encoding="utf-8")
    try:
        ref = transformers.BertTokenizerFast(str(path), do_lower_case=True)
    except Exception as e:   # an API change in the installed version is not a parity failure
        pytest.skip(f"transformers.BertTokenizerFast not constructible from a vocab file here: {e}")
    return ref, WordPieceTokenizer.from_vocab_file(str(path))


@pytest.mark.parametrize("max_length", [16, 64])
def test_encode_with_offsets_matches_bert_tokenizer_fast(offset_rig, max_length):
    ref, tok = offset_rig
    seen_unk = seen_cont = seen_cut = False
    for text in OFFSET_TEXTS:
        want = ref(text, truncation=True, max_length=max_length, return_offsets_mapping=True)
        ids, offs = tok.encode_with_offsets(text, max_length)
        assert ids == tok.encode(text, max_length), text
        assert ids == list(want["input_ids"]), (text, ids, want["input_ids"])
        assert [tuple(o) for o in offs] == [tuple(o) for o in want["offset_mapping"]], (text, offs, want["offset_mapping"])
        assert len(ids) <= max_length and offs[0] == (0, 0) and offs[-1] == (0, 0)
        seen_unk |= tok.unk_id in ids
        seen_cont |= any(OFFSET_VOCAB[i].startswith("##") for i in ids)
        seen_cut |= len(ids) == max_length
    assert seen_unk and seen_cont and (seen_cut or max_length == 64)


def test_offsets_index_the_callers_string(offset_rig):
    _, tok = offset_rig
    text = "  Caf\xe9:  Net\x00Profit was 11059 CRORE"
    ids, offs = tok.encode_with_offsets(text, 64)
    pieces = [text[a:b] for a, b in offs[1:-1]]
    assert pieces == ["Caf\u00e9", ":", "Net\x00Profit", "was", "11", "05", "9", "CRORE"]
    assert ids[3] == tok.unk_id and ids[1] == tok.vocab["cafe"]      # "netprofit" is no word of the vocabulary


# ---- surfaces -----------------------------------------------------------------------------------------------------
class FakeReader:
    """Answers with the first word of the context whose row number the table likes best."""
    def __init__(self, pick=None, fail=False):
        self.pick, self.fail, self.calls = pick, fail, []

    def predict(self, question, contexts, top_k=1, **kw):
        self.calls.append((question, list(contexts), top_k, kw))
        if self.fail:
            raise RuntimeError("reader exploded")
        if self.pick is None:
            return []
        text = contexts[self.pick]
        return [{"answer": text[5:], "score": 0.75, "start": 5, "end": len(text), "context_index": self.pick}][:top_k]


def make_rag(reader=None, generator=None, n=30):
    return VectorRAG("k", embedder=FakeEmbedder(), store=FakeStore(n), reader=reader, generator=generator, llm_delay_s=0)


def test_search_and_answer_returns_the_span_payload():
    rd = FakeReader(pick=2)
    rag = make_rag(rd)
    got = rag.search_and_answer("what was the net profit", 4)
    contexts = rag.search("what was the net profit", 4)
    assert got == {"answer": "2", "answer_span": {"context_index": 2, "start": 5, "end": 6, "score": 0.75},
                   "answer_source": "reader", "contexts": contexts, "context_count": 4}
    assert list(got) == ["answer", "answer_span", "answer_source", "contexts", "context_count"]
    span = got["answer_span"]
    assert got["answer"] == got["contexts"][span["context_index"]]["text"][span["start"]:span["end"]]
    assert rd.calls == [("what was the net profit", ["text 0", "text 1", "text 2", "text 3"], 1, {})]


def test_generator_takes_precedence_over_the_reader():
    rd = FakeReader(pick=0)
    rag = make_rag(rd, generator=lambda prompt: " generated ")
    got = rag.search_and_answer("what was the net profit", 2)
    assert got == {"answer": "generated", "contexts": rag.search("what was the net profit", 2), "context_count": 2}
    assert rd.calls == []


def test_zero_contexts_and_no_candidate_give_an_empty_answer():
    rd = FakeReader(pick=0)
    got = make_rag(rd, n=0).search_and_answer("what was the net profit", 3)
    assert got == {"answer": "", "answer_span": None, "answer_source": "reader", "contexts": [], "context_count": 0}
    assert rd.calls == []                                        # nothing to read: the reader is not called
    got = make_rag(FakeReader(pick=None)).search_and_answer("what was the net profit", 2)
    assert got["answer"] == "" and got["answer_span"] is None and got["context_count"] == 2


def test_reader_failure_takes_the_blanket_handler():
    rag = make_rag(FakeReader(fail=True))
    got = rag.search_and_answer("what was the net profit", 2)
    assert got == {"error": "reader exploded", "contexts": rag.search("what was the net profit", 2), "context_count": 2}


def test_without_reader_the_payload_is_todays():
    got = make_rag().search_and_answer("what was the net profit", 2)
    want = {"error": "no LLM generator configured (generation is outside this build)",
            "contexts": make_rag().search("what was the net profit", 2), "context_count": 2}
    assert got == want and list(got) == list(want)
    assert make_rag().reader is None
    # and the pinned payloads carry no new key
    assert list(make_rag(FakeReader(pick=0)).health_check()) == ["status", "milvus", "gemini", "collection", "total_chunks"]


def test_answer_question_tool_carries_the_span_keys():
    rag = make_rag(FakeReader(pick=1))
    mcp_server.set_rag(rag)
    try:
        r = mcp_server.answer_question("what was the net profit", 3)
        assert r["status"] == "success" and r["question"] == "what was the net profit"
        assert r["answer"] == "1" and r["answer_source"] == "reader" and r["context_count"] == 3
        assert r["answer_span"] == {"context_index": 1, "start": 5, "end": 6, "score": 0.75}
        assert r["contexts"][1]["text"][5:6] == "1"
        r = mcp_server.answer_question("what was the net profit", 3, min_score=0.5)
        assert r["answer_source"] == "reader"
    finally:
        mcp_server.set_rag(None)


def test_service_wires_the_reader_directory(monkeypatch):
    from rag_fin_amd import service
    seen = []
    monkeypatch.setattr(service, "build_rag", lambda *a, **kw: seen.append(kw))
    monkeypatch.setenv("RAGFIN_MODEL_DIR", "m")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("READER_MODEL_DIR", raising=False)
    service.build_rag_from_env()
    assert seen[-1]["reader_dir"] is None
    monkeypatch.setenv("READER_MODEL_DIR", "/models/minilm-squad2")
    service.build_rag_from_env()
    assert seen[-1]["reader_dir"] == "/models/minilm-squad2"
    assert service._load_reader(None, None) is None


def test_answer_spans_abi_is_declared_and_bound():
    from rag_fin_amd import _lib, build
    assert "reader.hip" in build.SOURCES
    lib = _lib.load_library()
    assert hasattr(lib, "rf_answer_spans") and "rf_answer_spans" in _lib.SIGNATURES
    # pointer checks come before anything touches a device
    assert lib.rf_answer_spans(None, None, None, None, 1, 8, None, 30, 16, None, None, None, None, 0, None) == -1
    text = open(_lib.__file__.replace("rag_fin_amd/_lib.py", "include/ragfin.h")).read()
    assert f"#define RF_READER_MAX_BEST {_lib.RF_READER_MAX_BEST}" in text
    assert f"#define RF_READER_MAX_SPAN {_lib.RF_READER_MAX_SPAN}" in text
