"""GPU tests of cross-encoder reranking: rf_score_pairs through rag_fin_amd.reranker.CrossEncoder against the
fp64 numpy mirror of tests/test_rerank_cpu.py (itself pinned to transformers.BertForSequenceClassification),
evaluated on the SAME fp16-rounded weights.  Seeded random weights; the classifier row is scaled so that the
logits are O(1) (HEAD_SCALE).

TOL = 3 x the largest |logit - mirror| measured on the MI355X over the parity shapes below
(profiles/rerank_measurements.jsonl), the margin rule of tests/test_encoder_gpu.py."""
import numpy as np
import pytest

from oracle import encoder as oenc
from test_rerank_cpu import mirror_logits

pytestmark = pytest.mark.gpu
TOL = 4.8e-3          # 3 x the 1.61e-3 measured (64 x 128, the fused layer path; the other shapes: 2.5e-4 .. 1.0e-3)
HEAD_SCALE = 0.1      # classifier row N(0, 0.1^2): logits of standard deviation ~1
CFG2 = dict(oenc.MINILM_L6, layers=2, vocab_size=2000)


def build(cfg, seed, device, tokenizer=None, num_labels=1):
    """(CrossEncoder, fp16-rounded weights, fp16-rounded head): both sides from the seed."""
    from rag_fin_amd.reranker import CrossEncoder, random_pair_head
    w = oenc.random_weights(cfg, seed)
    head = random_pair_head(cfg["hidden"], seed, head_scale=HEAD_SCALE)
    if num_labels != 1:
        head["cls_w"] = np.repeat(head["cls_w"], num_labels, axis=0)
        head["cls_b"] = np.repeat(head["cls_b"], num_labels, axis=0)
    ce = CrossEncoder(w, head, cfg, tokenizer=tokenizer, device=device, num_labels=num_labels)
    return ce, oenc.round_weights_fp16(w), oenc.round_weights_fp16(head)


@pytest.fixture(scope="module")
def model2(gpu_device):
    return build(CFG2, 5, gpu_device)


def pairs(rng, lens, seg, T, vocab=2000):
    lens, seg = np.asarray(lens, dtype=np.int32), np.asarray(seg, dtype=np.int32)
    return rng.integers(1, vocab, (len(lens), T)).astype(np.int32), lens, seg


def parity(ce, w16, head16, cfg, ids, lens, seg, name):
    from conftest import record_measurement
    got = ce.score_ids(ids, lens, seg).cpu().numpy()
    want = mirror_logits(w16, head16, cfg, ids, lens, seg)[:, 0]
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    err = float(np.abs(got - want).max())
    record_measurement(f"rerank_{name}", max_abs_logit=err, logit_std=float(want.std()), logit_abs_max=float(np.abs(want).max()))
    print(f"rerank_{name}: max |logit - mirror| = {err:.3e} (logits std {want.std():.2f}, max {np.abs(want).max():.2f})")
    assert err < TOL, err


SHAPES = {
    # a single short pair: the one-launch QKV + attention path (k_qkv_attn_one)
    "one_pair_24": (24, [24], [9]),
    # ragged, second segment starting at the edges of the embedding kernel's 32-position chunks; seg == len: none
    "ragged_5x96": (96, [96, 70, 64, 90, 40], [1, 31, 32, 33, 40]),
    # T > 256: the vector-ALU attention
    "long_2x300": (300, [300, 257], [20, 130]),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_logits_match_the_mirror(model2, name):
    ce, w16, head16 = model2
    T, lens, seg = SHAPES[name]
    ids, lens, seg = pairs(np.random.default_rng(T), lens, seg, T)
    parity(ce, w16, head16, CFG2, ids, lens, seg, name)


def test_logits_match_the_mirror_on_the_fused_layer_path(model2):
    """64 x 128 = 8192 token slots: k_linear_dma + k_post_block."""
    ce, w16, head16 = model2
    rng = np.random.default_rng(64)
    lens = rng.integers(40, 129, 64)
    lens[0] = 128
    seg = rng.integers(2, 30, 64)
    ids, lens, seg = pairs(rng, lens, seg, 128)
    parity(ce, w16, head16, CFG2, ids, lens, seg, "fused_64x128")


def test_logits_match_the_mirror_at_twelve_layers(gpu_device):
    cfg = dict(oenc.MINILM_L6, layers=12, vocab_size=2000)
    ce, w16, head16 = build(cfg, 9, gpu_device)
    rng = np.random.default_rng(12)
    ids, lens, seg = pairs(rng, [64, 33, 50, 12], [10, 20, 7, 5], 64)
    parity(ce, w16, head16, cfg, ids, lens, seg, "l12_4x64")


ORDER_SEED = 2   # chosen on the CPU: the mirror's smallest adjacent gap is 0.039 there, all 15 pairs decided


def order_case():
    rng = np.random.default_rng(ORDER_SEED)
    lens = rng.integers(20, 49, 16)
    return pairs(rng, lens, np.full(16, 8), 48)


def test_ranking_of_16_candidates_equals_the_mirrors(model2):
    ce, w16, head16 = model2
    ids, lens, seg = order_case()
    want = mirror_logits(w16, head16, CFG2, ids, lens, seg)[:, 0]
    order = np.argsort(-want, kind="stable")
    gaps = want[order][:-1] - want[order][1:]
    decided = gaps > 2 * TOL
    assert (~decided).sum() <= 2, gaps                 # the mirror's own condition (seed chosen for it)
    got = ce.score_ids(ids, lens, seg).cpu().numpy()
    for i in np.flatnonzero(decided):
        assert got[order[i]] > got[order[i + 1]], (i, gaps[i], got[order[i]], got[order[i + 1]])
    if decided.all():
        assert np.array_equal(np.argsort(-got, kind="stable"), order)


def test_same_pair_same_bits_anywhere_in_the_batch_and_across_calls(model2):
    ce = model2[0]
    rng = np.random.default_rng(3)
    ids, lens, seg = pairs(rng, [40, 17, 33, 40, 5, 29, 40], [7, 3, 9, 7, 2, 11, 7], 40)
    ids[3] = ids[0]
    ids[6] = ids[0]
    a = ce.score_ids(ids, lens, seg).cpu().numpy().view(np.uint32)
    b = ce.score_ids(ids, lens, seg).cpu().numpy().view(np.uint32)
    assert a[0] == a[3] == a[6]
    assert np.array_equal(a, b)
    assert len(set(a.tolist())) == 5                   # (the other rows are other pairs)


def test_embedder_graph_replay_is_untouched_by_interleaved_scoring(model2):
    """rf_encode replays a cached hipGraph for query-sized calls; a rerank call at the same (B, T) on the same
    handle takes plain launches and must leave the replay, and its own result, bit-identical."""
    ce = model2[0]
    emb = ce.encoder
    rng = np.random.default_rng(8)
    ids, lens, seg = pairs(rng, [24, 9, 16, 24], [5, 3, 8, 10], 24)
    e = [emb.encode_ids(ids, lens).cpu().numpy().view(np.uint16) for _ in range(3)]   # plain, capture, replay
    s1 = ce.score_ids(ids, lens, seg).cpu().numpy().view(np.uint32)
    e.append(emb.encode_ids(ids, lens).cpu().numpy().view(np.uint16))
    s2 = ce.score_ids(ids, lens, seg).cpu().numpy().view(np.uint32)
    e.append(emb.encode_ids(ids, lens).cpu().numpy().view(np.uint16))
    assert all(np.array_equal(e[0], x) for x in e[1:])
    assert np.array_equal(s1, s2)
    # and the two forwards are different functions of the same ids: the scores are not a replayed embedding
    assert np.isfinite(s1.view(np.float32)).all() and e[0].any()


def test_empty_row_scores_minus_infinity_and_leaves_its_neighbours_alone(model2):
    ce, w16, head16 = model2
    rng = np.random.default_rng(4)
    ids, lens, seg = pairs(rng, [20, 6, 13], [4, 2, 5], 20)
    full = ce.score_ids(ids, lens, seg).cpu().numpy()
    lens0 = lens.copy()
    lens0[1] = 0
    got = ce.score_ids(ids, lens0, seg).cpu().numpy()
    assert got[1] == -np.inf
    assert np.array_equal(got[[0, 2]].view(np.uint32), full[[0, 2]].view(np.uint32))
    want = mirror_logits(w16, head16, CFG2, ids[[0, 2]], lens[[0, 2]], seg[[0, 2]])[:, 0]
    assert np.abs(got[[0, 2]] - want).max() < TOL
    first = ce.score_ids(ids, np.array([0, 6, 13], np.int32), seg).cpu().numpy()       # the batch's first row
    assert first[0] == -np.inf and np.array_equal(first[1:].view(np.uint32), full[1:].view(np.uint32))
    one = ce.score_ids(ids[:1], np.array([0], np.int32), seg[:1]).cpu().numpy()        # a lone empty pair
    assert one.shape == (1,) and one[0] == -np.inf


def test_two_labels_and_overlong_rows_are_refused(gpu_device, model2):
    from rag_fin_amd import _lib
    cfg = dict(CFG2, layers=1, vocab_size=100, max_position=32)
    ce2, _, _ = build(cfg, 1, gpu_device, num_labels=2)
    with pytest.raises(_lib.RagfinError) as e:
        ce2.score_ids(np.ones((1, 8), np.int32), np.array([8], np.int32), np.array([3], np.int32))
    assert e.value.code == -2 and "num_labels" in str(e.value)
    ce1, _, _ = build(cfg, 1, gpu_device)
    with pytest.raises(_lib.RagfinError) as e:                                        # T > max_position
        ce1.score_ids(np.ones((1, 33), np.int32), np.array([8], np.int32), np.array([3], np.int32))
    assert e.value.code == -2
    cfg1 = dict(cfg, type_vocab=1)
    ce0, _, _ = build(cfg1, 1, gpu_device)
    with pytest.raises(_lib.RagfinError) as e:                                        # no second token-type row
        ce0.score_ids(np.ones((1, 8), np.int32), np.array([8], np.int32), np.array([3], np.int32))
    assert e.value.code == -2


def test_search_with_rerank_end_to_end_with_synthetic_vocab(gpu_device):
    """Text -> bi-encoder search for fetch_k = 8 -> pair tokenisation -> rf_score_pairs -> the best 3: exactly
    the mirror's best 3 of the store's 8 candidates, cosine scores untouched."""
    from rag_fin_amd.embedder import Embedder
    from rag_fin_amd.rag import VectorRAG
    from rag_fin_amd.service import ingest
    from rag_fin_amd.store import CorpusStore
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(200)] + list("abcdefghij")
    tok = WordPieceTokenizer(vocab)
    cfg = dict(oenc.MINILM_L6, layers=2, vocab_size=len(vocab), max_position=64)
    emb = Embedder(oenc.random_weights(cfg, 2), cfg, tokenizer=tok, device=gpu_device)
    ce, w16, head16 = build(cfg, 6, gpu_device, tokenizer=tok)
    rng = np.random.default_rng(1)
    texts = [" ".join(f"w{rng.integers(0, 200)}" for _ in range(rng.integers(1, 40))) for _ in range(37)]
    chunks = [dict(id=f"c{i}", text=t, period="Q1_FY2024", chunk_type="t", statement_type="s", primary_value=float(i))
              for i, t in enumerate(texts)]
    store = CorpusStore("t", dim=384, capacity=64, device=gpu_device)
    assert ingest(store, emb, chunks) == 37
    rag = VectorRAG("k", "t", embedder=emb, store=store, reranker=ce)
    query = "w3 w77 w150 w9 w21"
    plain = rag.search(query, 8)
    got = rag.search(query, top_k=3, rerank=True, fetch_k=8)
    cand = [c["text"] for c in plain]
    ids, lens, seg = tok.batch_pairs([query] * 8, cand, cfg["max_position"])
    want = mirror_logits(w16, head16, cfg, ids, lens, seg)[:, 0]
    order = np.argsort(-want, kind="stable")
    assert want[order][2] - want[order][3] > 2 * TOL and np.diff(-want[order][:4]).min() > 2 * TOL   # a decided case
    assert [c["text"] for c in got] == [cand[i] for i in order[:3]]
    assert [c["rank"] for c in got] == [1, 2, 3]
    assert [c["score"] for c in got] == [plain[i]["score"] for i in order[:3]]
    sig = 1 / (1 + np.exp(-want[order[:3]]))             # predict()'s default activation: sigmoid
    assert np.abs(np.array([c["rerank_score"] for c in got]) - sig).max() < TOL
    ranked = ce.rank(query, cand, top_k=3)
    assert [i for i, _ in ranked] == list(order[:3])
