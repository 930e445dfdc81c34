"""Sentence-embedder families on the GPU: rf_encode_sentences (csrc/sentence_head.hip) through Embedder.

Exact part, no tolerance: MEAN + normalise without skip is rf_encode bit for bit on every route of the forward,
and the modes agree with each other where their definitions coincide.

Oracle part: pool_reference (fp64) over oracle.encoder.encode(..., return_hidden=True) on the SAME fp16-rounded
weights.  The project's bound on the SCORE (cosine scores within 1e-3, north_star) applies as it stands.  The
per-component constants below are 3 x the maxima measured on the first GPU run of this file
(profiles/embedder_families_measurements.jsonl), the rule tests/test_encoder_gpu.py words for its own TOL."""
import json
import os

import numpy as np
import pytest

from conftest import record_measurement
from oracle import encoder as oenc

pytestmark = pytest.mark.gpu

CFG = dict(oenc.MINILM_L6, layers=2, max_position=512)
SEED = 11
MODES = ("mean", "cls", "max", "mean_sqrt_len")
RAGGED = (1, 2, 31, 32, 33, 255, 256, 257)   # the 32-token fragment, the 256-token trip, rows that start mid-fragment
NORTH_STAR_TOL = 1e-3                        # cosine scores, GPU-encoded vs oracle-encoded rows
GOLDEN_TOL = 9e-4                            # vs fp32-weight transformers outputs (tests/test_encoder_gpu.py)
TRAINED_TOL = 1.9e-3                         # the loosest bound the encoder tests carry: a ceiling for TOL_NORM
# max-abs error per component of a NORMALISED output (fp32), per mode: 3 x the measured maximum over the ragged
# batch and every skip (measured: mean 1.057e-4, cls 1.094e-4, max 1.057e-4, mean_sqrt_len 1.057e-4 -- the set
# modes share their worst row, a set of one token, where nothing averages the rounding away; all far below
# TRAINED_TOL)
TOL_NORM = {"mean": 3.17e-4, "cls": 3.28e-4, "max": 3.17e-4, "mean_sqrt_len": 3.17e-4}
# ||got - want||_2 / ||want||_2 per row of an UN-NORMALISED output, per mode: 3 x the measured maximum
# (measured: mean 5.93e-4, cls 5.93e-4, max 6.29e-4, mean_sqrt_len 5.93e-4)
TOL_REL = {"mean": 1.78e-3, "cls": 1.78e-3, "max": 1.89e-3, "mean_sqrt_len": 1.78e-3}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def batch(lens, T=None, seed=0, vocab=30522):
    lens = np.asarray(lens, dtype=np.int32)
    T = int(T or lens.max())
    ids = np.random.default_rng(seed).integers(1, vocab, (len(lens), T)).astype(np.int32)
    return ids, lens


def make_rig(gpu_device):
    """One set of weights, one embedder per (mode, normalize) over it, the ragged batch and its oracle hidden states
    (computed once, shared, never modified)."""
    from rag_fin_amd.embedder import Embedder
    w = oenc.random_weights(CFG, SEED)
    embs = {}

    def emb(mode="mean", normalize=True):
        if (mode, normalize) not in embs:
            embs[(mode, normalize)] = Embedder(w, CFG, device=gpu_device, pooling=mode, normalize=normalize)
        return embs[(mode, normalize)]
    ids, lens = batch(RAGGED, seed=1)
    hidden = oenc.encode(oenc.round_weights_fp16(w), CFG, ids, lens, return_hidden=True)
    hidden.setflags(write=False)
    return dict(emb=emb, ids=ids, lens=lens, hidden=hidden, device=gpu_device)


@pytest.fixture(scope="module")
def rig(gpu_device):
    return make_rig(gpu_device)


def both(e, ids, lens, **kw):
    return (e.encode_ids(ids, lens, out_dtype="float32", **kw).cpu().numpy(),
            e.encode_ids(ids, lens, out_dtype="float16", **kw).cpu().numpy())


# ---- exact --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["ragged", "one_query", "small", "fused_6_layers"])
def test_mean_without_skip_is_rf_encode_bit_for_bit(rig, shape):
    """The sentences entry is reached with a skip of zeros; the plain entry with none."""
    from rag_fin_amd.embedder import Embedder
    e = rig["emb"]()
    if shape == "ragged":                     # B * T > 1024: the bucketed route; T = 257: the attention beyond 256
        ids, lens = rig["ids"], rig["lens"]
    elif shape == "one_query":                # B = 1, T = 16: the single-query launch
        ids, lens = batch([16], seed=2)
    elif shape == "small":                    # 3 x 40: the small-batch GEMMs
        ids, lens = batch([40, 7, 33], seed=3)
    else:                                     # 64 x 128 at 6 layers: 8192 token slots, the fused post-block route,
        cfg = dict(CFG, layers=6)             # where the final activations sit in the other buffer
        e = Embedder(oenc.random_weights(cfg, SEED), cfg, device=rig["device"])
        ids, lens = batch(np.random.default_rng(4).integers(1, 129, 64), T=128, seed=4)
        lens[0] = 128
    want32, want16 = both(e, ids, lens)
    got32, got16 = both(e, ids, lens, skip=np.zeros(len(lens), np.int32))
    assert np.isfinite(want32).all() and np.abs(np.linalg.norm(want32, axis=1) - 1).max() < 1e-6
    assert np.array_equal(bits(got32), bits(want32))
    assert np.array_equal(bits(got16), bits(want16))


def test_rows_of_one_token_agree_across_modes_and_an_empty_set_is_zero(rig):
    ids, lens = batch([1, 1, 5, 1], seed=5)
    one = lens == 1
    outs = {m: both(rig["emb"](m, False), ids, lens) for m in MODES}
    for m in MODES:
        for k in (0, 1):
            assert np.array_equal(bits(outs[m][k][one]), bits(outs["cls"][k][one])), m
    assert np.abs(outs["cls"][0][one]).max() > 0.1
    skip = np.ones(4, np.int32)
    for m in MODES:
        got32, got16 = both(rig["emb"](m, False), ids, lens, skip=skip)
        if m == "cls":
            assert np.array_equal(bits(got32), bits(outs["cls"][0])) and np.array_equal(bits(got16), bits(outs["cls"][1]))
        else:
            assert not got32[one].any() and not got16[one].any() and np.abs(got32[~one]).max() > 0.1, m
            n32, _ = both(rig["emb"](m, True), ids, lens, skip=skip)       # and stays zero through the normalisation
            assert not n32[one].any() and np.abs(np.linalg.norm(n32[~one], axis=1) - 1).max() < 1e-6


def test_a_set_of_one_token_has_mean_equal_to_max(rig):
    ids, lens = batch([2, 2, 2], T=9, seed=6)
    skip = np.ones(3, np.int32)
    mean = both(rig["emb"]("mean", False), ids, lens, skip=skip)
    mx = both(rig["emb"]("max", False), ids, lens, skip=skip)
    root = both(rig["emb"]("mean_sqrt_len", False), ids, lens, skip=skip)
    for k in (0, 1):
        assert np.array_equal(bits(mean[k]), bits(mx[k])) and np.array_equal(bits(root[k]), bits(mx[k]))
    assert np.abs(mx[0]).max() > 0.1


def test_order_relations_on_the_ragged_batch(rig):
    ids, lens = rig["ids"], rig["lens"]
    cls32, _ = both(rig["emb"]("cls", False), ids, lens)
    max32, max16 = both(rig["emb"]("max", False), ids, lens)
    assert (max32 >= cls32).all()                                          # token 0 is in the set
    for s in (1, 31, 32, 33):
        skip = np.minimum(s, lens - 1).astype(np.int32)
        sub32, _ = both(rig["emb"]("max", False), ids, lens, skip=skip)
        assert (sub32 <= max32).all() and (sub32 < max32).any(), s         # a subset's maximum
    for m in MODES:
        for normalize in (True, False):
            o32, o16 = both(rig["emb"](m, normalize), ids, lens, skip=np.minimum(33, lens - 1).astype(np.int32))
            assert np.array_equal(bits(o16), bits(o32.astype(np.float16))), (m, normalize)
    # max is an exact maximum of fp16 values: representable, so the fp16 output loses nothing
    assert np.array_equal(max16.astype(np.float32), max32)


def test_cls_ignores_skip(rig):
    ids, lens = rig["ids"], rig["lens"]
    for normalize in (True, False):
        e = rig["emb"]("cls", normalize)
        a = both(e, ids, lens)
        for skip in (np.minimum(33, lens - 1), lens, np.full(len(lens), 1000)):    # also beyond the row
            b = both(e, ids, lens, skip=skip.astype(np.int32))
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


# ---- against the oracle ---------------------------------------------------------------------------------------------
def unit(a):
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-30)


def oracle_errors(rig, mode):
    """The maxima over every skip, with and without normalisation: the error per component of the normalised
    outputs, the error of the un-normalised rows relative to their L2 norm, the error of the cosine scores."""
    from rag_fin_amd.embedder import pool_reference
    ids, lens, hidden = rig["ids"], rig["lens"], rig["hidden"]
    worst = {"norm_max_abs": 0.0, "rel_l2": 0.0, "cos_score": 0.0}
    for s in (0, 1, 31, 32, 33, "len-1"):
        skip = (lens - 1 if s == "len-1" else np.minimum(s, lens - 1)).astype(np.int32)
        for normalize in (True, False):
            got = rig["emb"](mode, normalize).encode_ids(ids, lens, out_dtype="float32", skip=skip).cpu().numpy()
            want = pool_reference(hidden, lens, skip, mode, normalize)
            assert np.isfinite(got).all()
            if normalize:
                err = np.abs(got - want).max()
                worst["norm_max_abs"] = max(worst["norm_max_abs"], err)
                assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-6
            else:
                err = (np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)).max()
                worst["rel_l2"] = max(worst["rel_l2"], err)
            # north star: every cosine score between two GPU-encoded rows against the oracle's
            g, o = unit(got.astype(np.float64)), unit(want)
            worst["cos_score"] = max(worst["cos_score"], np.abs(g @ g.T - o @ o.T).max())
    return worst


@pytest.mark.parametrize("mode", MODES)
def test_every_mode_matches_the_oracle(rig, mode):
    worst = oracle_errors(rig, mode)
    print(f"embedder_families_oracle_{mode}", worst)
    record_measurement(f"embedder_families_oracle_{mode}", **worst)
    assert worst["cos_score"] < NORTH_STAR_TOL, worst
    assert TOL_NORM[mode] <= TRAINED_TOL
    assert worst["norm_max_abs"] < TOL_NORM[mode], worst
    assert worst["rel_l2"] < TOL_REL[mode], worst


# ---- end to end: directories --------------------------------------------------------------------------------------
WORDS = ["q", ":", "net", "profit", "rose", "in", "the", "first", "quarter", "retail", "banking", "deposits", "grew",
         "capital", "adequacy", "ratio", "gross", "npa", "fell", "total", "income", "was", "higher", "what", "?", "."]
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + WORDS + ["##" + w for w in WORDS if w.isalpha()]
TEXTS = ["what was the net profit in the first quarter?", "retail banking deposits grew.", "capital adequacy ratio",
         "gross npa fell", "total income was higher in the first quarter. net profit rose."]
ST = "sentence_transformers.models."


def make_dir(tmp_path, name, pooling, normalize, st_config=None, include_prompt=True, layers=2):
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    cfg = transformers.BertConfig(vocab_size=len(VOCAB), hidden_size=384, num_hidden_layers=layers,
                                  num_attention_heads=12, intermediate_size=1536, max_position_embeddings=512,
                                  type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu",
                                  hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(7)
    model = transformers.BertModel(cfg, add_pooling_layer=False).eval()
    with torch.no_grad():   # the default init (std 0.02) makes a nearly linear net: widen it
        for n_, p_ in model.named_parameters():
            if "LayerNorm" not in n_:
                p_.mul_(2.5)
    d = str(tmp_path / name)
    model.save_pretrained(d, safe_serialization=True)
    with open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(VOCAB) + "\n")
    mods = [{"idx": 0, "name": "0", "path": "", "type": ST + "Transformer"},
            {"idx": 1, "name": "1", "path": "1_Pooling", "type": ST + "Pooling"}]
    if normalize:
        mods.append({"idx": 2, "name": "2", "path": "2_Normalize", "type": ST + "Normalize"})
    json.dump(mods, open(os.path.join(d, "modules.json"), "w"))
    os.makedirs(os.path.join(d, "1_Pooling"))
    flags = {"cls": "pooling_mode_cls_token", "mean": "pooling_mode_mean_tokens", "max": "pooling_mode_max_tokens",
             "mean_sqrt_len": "pooling_mode_mean_sqrt_len_tokens"}
    json.dump({"word_embedding_dimension": 384, "include_prompt": include_prompt,
               **{f: m == pooling for m, f in flags.items()}}, open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    if st_config is not None:
        json.dump(st_config, open(os.path.join(d, "config_sentence_transformers.json"), "w"))
    return d, model


def st_encode(d, model, texts, mode, normalize, skip=0):
    """transformers' BertTokenizer + BertModel on the host in fp32, then sentence-transformers' Pooling / Normalize
    arithmetic restated; `skip` leading tokens are taken out of the attention mask the pooling sees (what
    include_prompt = False does), not out of the model's."""
    import torch
    import transformers
    tok = transformers.BertTokenizer(os.path.join(d, "vocab.txt"), do_lower_case=True)
    enc = tok(texts, padding=True, truncation=True, max_length=256, return_tensors="pt")
    with torch.no_grad():
        hid = model(input_ids=enc["input_ids"], attention_mask=enc["attention_mask"]).last_hidden_state
    mask = enc["attention_mask"].clone()
    mask[:, :skip] = 0
    m = mask.unsqueeze(-1).expand(hid.size()).float()
    if mode == "cls":
        out = hid[:, 0]
    elif mode == "max":
        h = hid.clone()
        h[m == 0] = -1e9
        out = torch.max(h, 1)[0]
    else:
        s, n = torch.sum(hid * m, 1), torch.clamp(m.sum(1), min=1e-9)
        out = s / n if mode == "mean" else s / torch.sqrt(n)
    return (torch.nn.functional.normalize(out, p=2, dim=1) if normalize else out).numpy(), enc


def test_cls_directory_with_a_query_prompt_matches_transformers(tmp_path, gpu_device):
    from rag_fin_amd.embedder import Embedder
    d, model = make_dir(tmp_path, "bge", "cls", True, {"prompts": {"query": "q: "}, "similarity_fn_name": "cosine"})
    emb = Embedder.from_local(d, device=gpu_device)
    assert (emb.pooling, emb.normalize, emb.query_prompt, emb.document_prompt) == ("cls", True, "q: ", None)
    got = emb.encode_query(TEXTS)
    want, enc = st_encode(d, model, ["q: " + t for t in TEXTS], "cls", True)
    ids, lens = emb.tokenizer.batch_native(["q: " + t for t in TEXTS], 256)
    for i in range(len(TEXTS)):
        assert ids[i, :lens[i]].tolist() == enc["input_ids"][i][:int(enc["attention_mask"][i].sum())].tolist()
    err = np.abs(got - want).max()
    record_measurement("embedder_families_cls_dir_vs_transformers", max_abs=err)
    assert got.shape == (len(TEXTS), 384) and got.dtype == np.float32
    assert err < GOLDEN_TOL, err
    # without the prompt the vectors are others; a document has no prompt in this directory
    plain = emb.encode(TEXTS)
    assert np.abs(plain - got).max() > 10 * GOLDEN_TOL
    assert np.array_equal(bits(emb.encode_document(TEXTS)), bits(plain))
    assert np.array_equal(bits(emb.encode(TEXTS, prompt="q: ")), bits(got))
    one = emb.encode_query(TEXTS[0])                                       # the one-query route
    assert one.shape == (384,) and np.abs(one - want[0]).max() < GOLDEN_TOL


def test_mean_directory_that_excludes_its_prompt_matches_transformers(tmp_path, gpu_device):
    from rag_fin_amd.embedder import Embedder
    d, model = make_dir(tmp_path, "e5", "mean", True, {"prompts": {"query": "q: "}}, include_prompt=False)
    emb = Embedder.from_local(d, device=gpu_device)
    assert (emb.pooling, emb.include_prompt) == ("mean", False)
    got = emb.encode_query(TEXTS)
    want, _ = st_encode(d, model, ["q: " + t for t in TEXTS], "mean", True, skip=3)      # [CLS] q :
    err = np.abs(got - want).max()
    record_measurement("embedder_families_mean_skip_dir_vs_transformers", max_abs=err)
    assert err < GOLDEN_TOL, err
    pooled, _ = st_encode(d, model, ["q: " + t for t in TEXTS], "mean", True)            # the prompt pooled: another vector
    assert np.abs(pooled - want).max() > 10 * GOLDEN_TOL
    # the bucketed route carries a row's skip through its sort and gather: the same rows in a large batch
    many = (TEXTS * 60)[:257]
    big = emb.encode(many, prompt_name="query")
    assert big.shape == (257, 384) and np.abs(big - np.concatenate([want] * 52)[:257]).max() < GOLDEN_TOL


def test_dot_product_directory_gives_an_ip_store_with_the_oracles_scores(tmp_path, gpu_device):
    from safetensors.numpy import load_file
    from rag_fin_amd.embedder import hf_encoder_config, pool_reference, stack_hf_state_dict
    from rag_fin_amd.rag import VectorRAG
    from rag_fin_amd.service import ingest, load_embedder, store_metric
    from rag_fin_amd.store import CorpusStore
    d, _ = make_dir(tmp_path, "dot", "mean", False, {"similarity_fn_name": "dot"})
    emb = load_embedder(d, gpu_device)
    assert (emb.pooling, emb.normalize, emb.similarity_fn_name) == ("mean", False, "dot")
    metric = store_metric(emb)
    assert metric == "IP"
    store = CorpusStore("dot_chunks", dim=emb.dim, device=gpu_device, metric_type=metric)
    chunks = [dict(id=f"c{i}", text=t, period="Q1_FY2024", chunk_type="t", statement_type="s", primary_value=float(i))
              for i, t in enumerate(TEXTS)]
    assert ingest(store, emb, chunks) == len(TEXTS)
    rag = VectorRAG(None, "dot_chunks", embedder=emb, store=store)
    # the oracle: fp64 forward on the fp16-rounded weights, un-normalised mean
    cfg = hf_encoder_config(json.load(open(os.path.join(d, "config.json"))))
    w = oenc.round_weights_fp16(stack_hf_state_dict(load_file(os.path.join(d, "model.safetensors")), cfg))
    queries = ["net profit", "what was the capital adequacy ratio?"]

    def oracle(texts):
        ids, lens = emb.tokenizer.batch(texts, 256)
        return pool_reference(oenc.encode(w, cfg, ids, lens, return_hidden=True), lens, None, "mean", False)
    docs, qs = oracle(TEXTS), oracle(queries)
    assert np.linalg.norm(docs, axis=1).min() > 2                          # not unit rows: IP and COSINE differ
    worst = 0.0
    for qi, q in enumerate(queries):
        ctx = rag.search(q, len(TEXTS))
        assert len(ctx) == len(TEXTS)
        for c in ctx:
            di = TEXTS.index(c["text"])
            # each side within TOL_REL of its oracle row (relative to the row's norm), both rounded to fp16 for the
            # store's sweep (2^-11 each): |<q, d> - <q', d'>| <= (2 TOL_REL + 2^-10) |q| |d| to first order
            scale = np.linalg.norm(qs[qi]) * np.linalg.norm(docs[di])
            rel = abs(c["score"] - float(qs[qi] @ docs[di])) / scale
            worst = max(worst, rel)
            assert rel < 2 * TOL_REL["mean"] + 2.0 ** -10, (q, c["text"], rel)
    record_measurement("embedder_families_dot_scores_vs_oracle", rel_to_norms=worst)
    assert rag.health_check()["normalize"] is False


def test_minilm_style_directory_is_todays_embedder_bit_for_bit(tmp_path, gpu_device):
    from safetensors.numpy import load_file
    from rag_fin_amd.embedder import Embedder, hf_encoder_config, stack_hf_state_dict
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    d, _ = make_dir(tmp_path, "minilm", "mean", True)
    new = Embedder.from_local(d, device=gpu_device)
    assert (new.pooling, new.normalize, new.prompts, new.query_prompt) == ("mean", True, {}, None)
    cfg = hf_encoder_config(json.load(open(os.path.join(d, "config.json"))))
    old = Embedder(stack_hf_state_dict(load_file(os.path.join(d, "model.safetensors")), cfg), cfg,
                   WordPieceTokenizer.from_vocab_file(os.path.join(d, "vocab.txt")), gpu_device, 256)
    calls = []
    real = new.lib.rf_encode_sentences
    new.lib.rf_encode_sentences = lambda *a: calls.append(a) or real(*a)
    try:
        for texts in (TEXTS, TEXTS[:1], (TEXTS * 60)[:257]):               # small, one query, bucketed
            assert np.array_equal(bits(new.encode(texts)), bits(old.encode(texts)))
            assert np.array_equal(bits(new.encode_query(texts, normalize_embeddings=False)), bits(old.encode(texts)))
    finally:
        new.lib.rf_encode_sentences = real
    assert not calls                                                       # today's path: rf_encode alone
