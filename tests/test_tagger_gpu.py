"""GPU tests of entity tagging: rf_tag_logits and rf_group_entities through rag_fin_amd.tagger.
  * the logits against the fp64 numpy mirror of tests/test_tagger_cpu.py (itself pinned to
    transformers.BertForTokenClassification), evaluated on the SAME fp16-rounded weights;
  * the decode (groups, counts, per-token labels and scores) against rag_fin_amd.tagger.entities_reference on
    synthetic logits -- no forward in front of it, so every pattern is reachable -- and, end to end, on the
    device's own logits;
  * placement stability, isolation from the embedder's hipGraph replay, argument checks, ingest + filtered search.
Seeded random weights; the classifier is scaled so that the logits are O(1) (HEAD_SCALE).

TOL = 3 x the largest |logit - mirror| measured on the MI355X over the parity shapes below
(profiles/tagger_measurements.jsonl), the margin rule of tests/test_reader_gpu.py."""
import ctypes

import numpy as np
import pytest

from oracle import encoder as oenc
from rag_fin_amd import _lib
from rag_fin_amd.tagger import entities_reference, label_tables
from test_rerank_cpu import mirror_hidden
from test_tagger_cpu import LABELS9

pytestmark = pytest.mark.gpu
# Measured (the largest over L in {1, 2, 9, 37, 64}, reached at L = 64 each time): 1x8 4.09e-3, 3x64 4.08e-3, 64x128 4.59e-3,
# 2x512 4.61e-3 -- the level tests/test_reader_gpu.py records for the span head's logits over the same hidden states
# (3.66e-3 as a maximum over 16 k logits; here over up to 343 k); the root-mean-square error is 1.0e-3 at every shape.
TOL = 1.4e-2          # 3 x the 4.61e-3 measured (2 x 512, 64 labels)
HEAD_SCALE = 0.1      # classifier rows N(0, 0.1^2): logits of standard deviation ~1
CFG2 = dict(oenc.MINILM_L6, layers=2, vocab_size=2000)
SCORE_TOL = 2.0 ** -23   # two fp32 roundings of one fp64 value in (0, 1] whose exp evaluations differ by a few fp64 ulp
WIDTHS = (1, 2, 9, 37, 64)


def labels_of(L):
    """L label names: "O", then B- / I- pairs, the last one unprefixed when L is even."""
    names = ["O"] + [f"{p}-T{k}" for k in range(32) for p in ("B", "I")]
    return LABELS9 if L == 9 else (names[:L - 1] + ["PLAIN"] if L % 2 == 0 else names[:L])


@pytest.fixture(scope="module")
def models(gpu_device):
    """{L: (TokenClassifier, fp16-rounded head)} over ONE set of encoder weights, and those weights fp16-rounded."""
    from rag_fin_amd.tagger import TokenClassifier, random_tag_head
    w = oenc.random_weights(CFG2, 5)
    out = {}
    for L in WIDTHS:
        head = random_tag_head(384, L, 5, head_scale=HEAD_SCALE)
        out[L] = (TokenClassifier(w, head, labels_of(L), CFG2, device=gpu_device), oenc.round_weights_fp16(head))
    return out, oenc.round_weights_fp16(w)


# ---- logits against the mirror ------------------------------------------------------------------------------------
SHAPES = {
    "1x8": (8, [8]),                                   # the one-launch QKV + attention path
    "3x64": (64, [64, 33, 5]),
    "64x128": (128, None),                             # 8192 token slots: the fused layer path
    "2x512": (512, [512, 300]),                        # T > 256: the vector-ALU attention; two blocks of k_tag_logits rows
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_logits_match_the_mirror(models, name):
    from conftest import record_measurement
    by_width, w16 = models
    T, lens = SHAPES[name]
    rng = np.random.default_rng(T)
    if lens is None:
        lens = rng.integers(40, 129, 64)
        lens[0] = 128
    lens = np.asarray(lens, dtype=np.int32)
    ids = rng.integers(1, 2000, (len(lens), T)).astype(np.int32)
    x = mirror_hidden(w16, CFG2, ids, lens, np.zeros(ids.shape, dtype=np.int64), np.float64)   # once per shape
    live = np.arange(T)[None, :] < lens[:, None]
    worst = 0.0
    for L in WIDTHS:
        tc, head16 = by_width[L]
        got = tc.tag_ids(ids, lens).cpu().numpy()
        want = x @ head16["cls_w"].astype(np.float64).T + head16["cls_b"].astype(np.float64)
        assert got.dtype == np.float32 and got.shape == (len(lens), T, L) and np.isfinite(got[live]).all()
        assert not got[~live].any()                          # positions >= len are not written
        err = float(np.abs(got - want)[live].max())
        rms = float(np.sqrt(np.mean((got - want)[live] ** 2)))
        record_measurement(f"tagger_{name}_L{L}", max_abs_logit=err, rms_logit=rms, logits=int(L * live.sum()),
                           logit_std=float(want[live].std()), logit_abs_max=float(np.abs(want[live]).max()))
        print(f"tagger_{name}_L{L}: max |logit - mirror| = {err:.3e}, rms {rms:.3e} over {L * live.sum()} logits "
              f"(logits std {want[live].std():.2f}, max {np.abs(want[live]).max():.2f})")
        worst = max(worst, err)
    assert worst < TOL, worst


def test_same_row_same_bits_in_a_batch_of_1_and_any_slot_of_a_batch_of_64(models):
    """64 x 16 = 1024 token slots, the widest batch of 64 whose layers run the kernels a single row's do (see
    tests/test_reader_gpu.py: above 1024 slots the layers switch GEMM kernels and the hidden rows differ in their
    last fp16 bits between batch widths).  The classifier itself never depends on the batch, and a tag forward
    sends a lone row of <= 32 tokens through the launches of a batch, not through the embedder's one-launch
    QKV + attention, whose rounding differs on most inputs."""
    tc = models[0][9][0]
    rng = np.random.default_rng(5)
    lens = rng.integers(5, 17, 64).astype(np.int32)
    ids = rng.integers(1, 2000, (64, 16)).astype(np.int32)
    for slot in (0, 17, 63):
        ids[slot], lens[slot] = ids[0], 16
    many = tc.tag_ids(ids, lens).cpu().numpy().view(np.uint32)
    one = tc.tag_ids(ids[:1], lens[:1]).cpu().numpy().view(np.uint32)
    again = tc.tag_ids(ids, lens).cpu().numpy().view(np.uint32)
    assert one.any() and np.array_equal(many, again)
    for slot in (0, 17, 63):
        assert np.array_equal(one[0], many[slot]), slot
    assert not np.array_equal(many[0], many[1])              # (another row)


# ---- the decode on synthetic logits -------------------------------------------------------------------------------
def synthetic_rows(T, L, rng):
    """Rows (logits [T, L], len, word_start [T]) for every pattern x every length."""
    _, lt, lb = label_tables(labels_of(L))
    inner = next((c for c in range(L) if c and not lb[c]), 0)          # an I- label (label 0 when there is none)
    begin = next((c for c in range(L) if lb[c]), 0)                    # a B- label
    rows = []
    for n in sorted({0, 1, 2, 3, T}):
        def peak(c):
            z = rng.standard_normal((T, L)).astype(np.float32)
            z[:, c] += 20.0
            return z
        ws = (rng.random(T) < 0.6).astype(np.uint8)
        one_word = np.zeros(T, dtype=np.uint8)
        one_word[:2] = 1
        rows += [((rng.standard_normal((T, L)) * 3).astype(np.float32), n, ws),           # random
                 (peak(inner), n, ws),                                                     # all one tag: one group
                 (peak(begin), n, np.ones(T, dtype=np.uint8)),                             # every unit B-X
                 (np.full((T, L), 0.25, dtype=np.float32), n, ws),                         # all equal: label 0
                 ((rng.standard_normal((T, L)) * 3).astype(np.float32), n, one_word),      # one word
                 (np.round(rng.standard_normal((T, L)) * 2).astype(np.float32), n, ws)]    # quantised: argmax ties
    return rows, lt, lb, inner, begin


@pytest.mark.parametrize("L", [1, 9, 64])
@pytest.mark.parametrize("T", [3, 64, 65, 512])
def test_grouping_equals_entities_reference_on_synthetic_logits(gpu_device, T, L):
    import torch
    from rag_fin_amd.tagger import group_logits
    rows, lt, lb, inner, begin = synthetic_rows(T, L, np.random.default_rng(1000 * T + L))
    logits = np.stack([r[0] for r in rows])
    lens = np.array([r[1] for r in rows], dtype=np.int32)
    ws = np.stack([r[2] for r in rows])
    dev = torch.as_tensor(logits).to(gpu_device)
    worst = 0.0
    for strategy in (0, 1):
        for ignore in (-1, 0):
            me = 128 if strategy == 0 else 37                # (another capacity: the fill of the unused slots)
            want, wcount, wlab, wsc = entities_reference(logits, lens, ws, lt, lb, strategy, ignore, me)
            host = group_logits(dev, lens, ws, lt, lb, strategy, ignore, me, want_tokens=True).cpu()
            ent, score, count = host.ent.numpy(), host.score.numpy(), host.count.numpy()
            assert np.array_equal(count, wcount), (strategy, ignore, count, wcount)
            assert np.array_equal(host.tok_label.numpy(), wlab)
            assert np.abs(host.tok_score.numpy() - wsc).max() <= SCORE_TOL
            for b in range(len(rows)):
                assert [tuple(e) for e in ent[b]] == [e[:3] for e in want[b]], (strategy, ignore, b, lens[b])
                ws_b = np.array([e[3] for e in want[b]], dtype=np.float32)
                none = np.isinf(ws_b)
                assert np.array_equal(np.isinf(score[b]), none) and (score[b][none] == -np.inf).all()
                if (~none).any():
                    worst = max(worst, float(np.abs(score[b][~none] - ws_b[~none]).max()))
            # the patterns did what they are there for (rows of the full length: the last six)
            full = len(rows) - 6
            if T >= 3:
                assert wcount[full + 1] == (0 if ignore == lt[inner] else 1)                 # all one tag: one group
                if not (ignore == lt[inner] == 0):
                    assert want[full + 1][0][:2] == (1, T - 2)
                assert wcount[full + 2] == (T - 2 if lb[begin] else (1 if ignore == -1 else 0))   # every unit a B-
                assert (wlab[full + 3, 1:T - 1] == 0).all()                                  # all equal: label 0
            if T == 512 and L > 1:
                assert wcount[full + 2] == 510 > me and ent[full + 2, me - 1, 0] == me       # the overflow path
            if strategy == 1 and T >= 4 and ignore == -1:
                assert wcount[full + 4] == 1 and want[full + 4][0][:2] == (1, T - 2)         # one word: one group
    assert worst <= SCORE_TOL, worst
    print(f"grouping T={T} L={L}: max |score - reference| = {worst:.3e} (bound {SCORE_TOL:.3e})")


def test_grouping_without_token_outputs_and_without_word_starts(gpu_device):
    """tok_label / tok_score and, under RF_TAG_SIMPLE, word_start are optional: the groups are the same."""
    import torch
    from rag_fin_amd.tagger import group_logits
    _, lt, lb = label_tables(LABELS9)
    logits = (np.random.default_rng(2).standard_normal((5, 40, 9)) * 3).astype(np.float32)
    lens = np.array([40, 17, 3, 0, 29], dtype=np.int32)
    dev = torch.as_tensor(logits).to(gpu_device)
    a = group_logits(dev, lens, None, lt, lb, 0, 0, 16).cpu()
    b = group_logits(dev, lens, np.ones((5, 40), np.uint8), lt, lb, 0, 0, 16, want_tokens=True).cpu()
    assert a.tok_label is None and np.array_equal(a.packed.numpy(), b.packed.numpy()[:a.packed.numel()])
    want = entities_reference(logits, lens, None, lt, lb, 0, 0, 16)
    assert np.array_equal(a.count.numpy(), want[1]) and a.count.numpy()[0] > 0
    with pytest.raises(_lib.RagfinError) as e:                                        # FIRST needs the word starts
        group_logits(dev, lens, None, lt, lb, 1, 0, 16)
    assert e.value.code == -1


# ---- end to end ---------------------------------------------------------------------------------------------------
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(200)] + \
        [f"##{c}" for c in "abcdefghij"] + list("abcdefghij") + [".", ","]


@pytest.fixture(scope="module")
def text_rig(gpu_device):
    from rag_fin_amd.tagger import TokenClassifier
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    tok = WordPieceTokenizer(VOCAB)
    cfg = dict(oenc.MINILM_L6, layers=2, vocab_size=len(VOCAB), max_position=512)
    tc = TokenClassifier.from_random(cfg, LABELS9, 6, tokenizer=tok, device=gpu_device, head_scale=HEAD_SCALE)
    rng = np.random.default_rng(1)

    def word():
        return f"W{rng.integers(0, 200)}" + "".join(rng.choice(list("abcdefghij"), rng.integers(0, 3)))
    texts = ["  " + " ".join(word() + rng.choice(["", ".", ",", "  "]) for _ in range(rng.integers(1, 40))) for _ in range(37)]
    return tc, tok, cfg, texts


@pytest.mark.parametrize("strategy", ["simple", "first", "none"])
def test_predict_equals_entities_reference_on_the_devices_logits(text_rig, strategy):
    tc, tok, _, texts = text_rig
    texts = texts + ["", "w1"]
    got = tc.predict(texts, aggregation_strategy=strategy)
    assert got == tc.predict(texts, aggregation_strategy=strategy)                    # bit-identical across calls
    ids, lens, offsets = tc._rows(texts)
    order = np.argsort(lens, kind="stable")                                           # predict's one bucket
    logits = np.empty((len(texts), ids.shape[1], 9), dtype=np.float32)
    logits[order] = tc.tag_ids(ids[order], lens[order]).cpu().numpy()
    ws = tc.word_starts(ids)
    assert (ws == 0).any() and ws[:, 0].all()
    want, count, lab, sc = entities_reference(logits, lens, ws, tc.label_tag, tc.label_begin,
                                              {"simple": 0, "first": 1, "none": 0}[strategy], 0, 128)
    assert len(got) == len(texts) and got[-2] == [] and count.max() <= 128
    n = 0
    for ti, text in enumerate(texts):
        off = offsets[ti]
        if strategy == "none":
            exp = [dict(entity=LABELS9[lab[ti, t]], score=float(sc[ti, t]), index=t, word=text[off[t][0]:off[t][1]],
                        start=off[t][0], end=off[t][1]) for t in range(1, lens[ti] - 1) if lab[ti, t] != 0]
        else:
            exp = [dict(entity_group=tc.tag_names[t], score=float(s), word=text[off[a][0]:off[b][1]], start=off[a][0],
                        end=off[b][1]) for a, b, t, s in want[ti][:count[ti]]]
        assert [{k: v for k, v in d.items() if k != "score"} for d in got[ti]] == \
               [{k: v for k, v in d.items() if k != "score"} for d in exp], (ti, text)
        assert all(abs(g["score"] - e["score"]) <= SCORE_TOL for g, e in zip(got[ti], exp))
        assert all(d["word"] == text[d["start"]:d["end"]] and d["word"] == d["word"].strip() and d["word"] for d in got[ti])
        n += len(exp)
    assert n > 100
    # several length buckets (other batch shapes: the logits may differ in their last bits): the same layout
    split = tc.predict(texts, aggregation_strategy=strategy, batch_tokens=600)
    assert len(split) == len(texts) and split[-2] == [] and sum(len(r) for r in split) > 100
    assert all(d["word"] == text[d["start"]:d["end"]] for text, row in zip(texts, split) for d in row)


def test_predict_warns_past_the_entity_capacity_and_cuts_long_texts(text_rig):
    tc, _, _, _ = text_rig
    text = " ".join(f"w{i % 200}" for i in range(700))                                # 700 tokens: cut at 510
    with pytest.warns(RuntimeWarning, match="entity groups"):
        got = tc.predict([text], ignore_labels=())
    assert len(got[0]) == 128 and got[0][-1]["end"] <= len(" ".join(f"w{i % 200}" for i in range(510)))
    per_token = tc.predict([text], aggregation_strategy="none", ignore_labels=())
    assert [d["index"] for d in per_token[0]] == list(range(1, 511))


def test_ingest_fills_the_array_field_and_match_entities_filters_on_it(gpu_device, text_rig):
    from rag_fin_amd.embedder import Embedder
    from rag_fin_amd.rag import VectorRAG
    from rag_fin_amd.schema import DataType, FieldSchema
    from rag_fin_amd.service import ingest
    from rag_fin_amd.store import CorpusStore
    from rag_fin_amd.tagger import entity_expr
    tc, tok, cfg, texts = text_rig
    emb = Embedder(oenc.random_weights(cfg, 2), cfg, tokenizer=tok, device=gpu_device)
    chunks = [dict(id=f"c{i}", text=t, period="Q1_FY2024", chunk_type="t", statement_type="s", primary_value=float(i))
              for i, t in enumerate(texts)]
    store = CorpusStore("t", dim=384, capacity=64, device=gpu_device,
                        fields=[FieldSchema("entities", DataType.ARRAY, element_type=DataType.VARCHAR, max_capacity=16)])
    assert ingest(store, emb, chunks, tagger=tc, entity_field="entities") == 37
    rag = VectorRAG("k", "t", embedder=emb, store=store, tagger=tc, entity_field="entities",
                    extra_output_fields=["entities"])
    stored = tc.tags(texts, max_per_row=16)
    assert any(len(row) > 16 for row in tc.tags(texts))                               # the capacity cut something
    question = texts[5]
    found = tc.tags([question])[0]
    assert len(found) >= 2
    for how, test in (("any", lambda row: bool(set(row) & set(found))), ("all", lambda row: set(found) <= set(row))):
        got = rag.search(question, 37, match_entities=how)
        by_hand = rag.search(question, 37, expr=entity_expr("entities", found, how))
        assert got == by_hand
        assert sorted(c["text"] for c in got) == sorted(t for t, row in zip(texts, stored) if test(row)), how
        assert all(c["entities"] == stored[texts.index(c["text"])] for c in got)
    assert 0 < len(rag.search(question, 37, match_entities="any")) < 37
    both = rag.search(question, 37, expr="primary_value < 20", match_entities="any")
    assert both == rag.search(question, 37, expr=f'(primary_value < 20) and {entity_expr("entities", found)}')
    assert both and all(c["primary_value"] < 20 for c in both)
    assert tc.tags([""]) == [[]] and rag.search("", 5, match_entities="any") == rag.search("", 5)   # no entities: unfiltered


# ---- isolation, argument checks -----------------------------------------------------------------------------------
def test_embedder_graph_replay_is_untouched_by_interleaved_tagging(models):
    """rf_encode replays a cached hipGraph for query-sized calls; tag calls at the same (B, T) on the same handle
    in between take plain launches and leave it, and themselves, bit-identical."""
    tc = models[0][9][0]
    emb = tc.encoder
    rng = np.random.default_rng(8)
    lens = np.array([24, 9, 16, 24], dtype=np.int32)
    ids = rng.integers(1, 2000, (4, 24)).astype(np.int32)
    e = [emb.encode_ids(ids, lens).cpu().numpy().view(np.uint16) for _ in range(3)]   # plain, capture, replay
    t = [tc.tag_ids(ids, lens).cpu().numpy().view(np.uint32)]
    e.append(emb.encode_ids(ids, lens).cpu().numpy().view(np.uint16))
    t.append(tc.tag_ids(ids, lens).cpu().numpy().view(np.uint32))
    e.append(emb.encode_ids(ids, lens).cpu().numpy().view(np.uint16))
    assert all(np.array_equal(e[0], x) for x in e[1:])
    assert np.array_equal(t[0], t[1]) and e[0].any() and t[0].any()


def test_bad_arguments_are_refused_before_anything_is_launched(gpu_device, models):
    import torch
    from rag_fin_amd.tagger import TokenClassifier
    tc = models[0][9][0]
    cfg = dict(CFG2, layers=1, vocab_size=100, max_position=32, type_vocab=1)          # one token-type row is enough
    small = TokenClassifier.from_random(cfg, LABELS9, 1, device=gpu_device)
    assert small.tag_ids(np.ones((1, 8), np.int32), np.array([8], np.int32)).cpu().numpy().any()
    with pytest.raises(_lib.RagfinError) as e:                                        # T > max_position
        small.tag_ids(np.ones((1, 33), np.int32), np.array([8], np.int32))
    assert e.value.code == -2 and "max_position" in str(e.value)
    with pytest.raises(ValueError, match="labels"):
        TokenClassifier.from_random(cfg, [f"L{i}" for i in range(65)], 1, device=gpu_device)
    # nothing was launched: a refused call leaves its output buffer as it was
    ids = torch.ones((1, 8), dtype=torch.int32, device=gpu_device)
    lens = torch.full((1,), 8, dtype=torch.int32, device=gpu_device)
    out = torch.full((8 * 9,), 12345.0, dtype=torch.float32, device=gpu_device)
    ws = torch.empty(tc.lib.rf_encode_workspace_bytes(tc.encoder.handle, 1, 8), dtype=torch.uint8, device=gpu_device)
    p = ctypes.c_void_p
    head = _lib.TagHead(tc._head["cls_w"].data_ptr(), tc._head["cls_b"].data_ptr(), 65)
    rc = tc.lib.rf_tag_logits(tc.encoder.handle, p(ids.data_ptr()), p(lens.data_ptr()), 1, 8, ctypes.byref(head),
                              p(out.data_ptr()), p(ws.data_ptr()), ws.numel(), _lib.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc == -2 and (out.cpu().numpy() == 12345.0).all()
    rc = tc.lib.rf_tag_logits(tc.encoder.handle, p(ids.data_ptr()), p(lens.data_ptr()), 1, 8, ctypes.byref(tc._head_c),
                              p(out.data_ptr()), p(ws.data_ptr()), 16, _lib.current_stream_ptr())   # workspace too small
    torch.cuda.synchronize()
    assert rc == -3 and (out.cpu().numpy() == 12345.0).all()
