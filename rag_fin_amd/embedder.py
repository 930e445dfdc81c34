"""Sentence embedder on the GPU: the in-process replacement for
`SentenceTransformer('all-MiniLM-L6-v2')` on the vector-RAG path.

Reference call sites mirrored:
  ctor            vector_rag_mcp/main.py:41, retrieve.py:14, "chunking_storing (1).py":8
  .encode([q])    vector_rag_mcp/main.py:50, retrieve.py:27  -> np.float32 [1, 384]
  .encode(texts)  "chunking_storing (1).py":379-380          -> np.float32 [n, 384]

The reference loads the model by NAME (a network fetch); here the checkpoint comes
from a LOCAL directory in the Hugging Face layout (config.json, vocab.txt,
model.safetensors), read with safetensors only.  The forward pass runs in
libragfin_hip.so (rf_encode); there is no CPU path.

Other sentence-transformers models of the same BERT-H384 family (CLS pooling, prompts, no
Normalize module) are read with their own modules.json / Pooling config / prompts
(sentence_config) and end in rf_encode_sentences; mean + normalise stays on rf_encode.
"""
from __future__ import annotations

import ctypes
import json
import os
import threading
from ctypes import c_void_p

import numpy as np

from . import _lib
from .store import require_gpu
from .tokenizer import WordPieceTokenizer

MINILM_L6 = dict(vocab_size=30522, hidden=384, layers=6, heads=12, intermediate=1536,
                 max_position=512, type_vocab=2, ln_eps=1e-12)


def _torch():
    import torch
    return torch


# ---- sentence-embedder families: what a sentence-transformers directory says about its own ends ---------------------
POOLING_MODES = {"mean": _lib.RF_POOL_MEAN, "cls": _lib.RF_POOL_CLS, "max": _lib.RF_POOL_MAX,
                 "mean_sqrt_len": _lib.RF_POOL_MEAN_SQRT_LEN}
_POOLING_FLAGS = {"pooling_mode_cls_token": "cls", "pooling_mode_mean_tokens": "mean", "pooling_mode_max_tokens": "max",
                  "pooling_mode_mean_sqrt_len_tokens": "mean_sqrt_len"}
_UNOFFERED_FLAGS = {"pooling_mode_weightedmean_tokens": "weightedmean", "pooling_mode_lasttoken": "lasttoken"}
_ST = "sentence_transformers.models."


def check_pooling(pooling) -> str:
    """The name of a pooling mode the kernels offer ("mean", "cls", "max", "mean_sqrt_len"); ValueError otherwise."""
    name = str(pooling).lower().replace("-", "_")
    if name in ("weightedmean", "lasttoken"):
        raise ValueError(f"pooling {name!r} is not offered (mean, cls, max and mean_sqrt_len are)")
    if name not in POOLING_MODES:
        raise ValueError(f"pooling must be one of {', '.join(POOLING_MODES)}, not {pooling!r}")
    return name


def pool_reference(hidden, lens, skip=None, pooling="mean", normalize=True) -> np.ndarray:
    """The numpy definition of rf_encode_sentences' last launch, in float64: hidden [B, T, H] last hidden states,
    lens [B], skip [B] or None (= 0) -> [B, H].  The pooled set of row b is the tokens skip[b] <= t < lens[b]:
    mean = sum / max(count, 1e-9), mean_sqrt_len = sum / sqrt(count), max = the per-feature maximum, cls = token 0
    whatever skip says; an empty set gives the zero vector (sentence-transformers' Pooling gives -1e9 for max
    there; Embedder never produces one).  normalize divides by max(||x||_2, 1e-12), as its Normalize module does."""
    pooling = check_pooling(pooling)
    hidden = np.asarray(hidden, dtype=np.float64)
    B, T, H = hidden.shape
    lens = np.clip(np.asarray(lens, dtype=np.int64), 0, T)
    skip = np.zeros(B, dtype=np.int64) if skip is None else np.clip(np.asarray(skip, dtype=np.int64), 0, lens)
    out = np.zeros((B, H), dtype=np.float64)
    for b in range(B):
        if pooling == "cls":
            if lens[b] > 0:
                out[b] = hidden[b, 0]
            continue
        rows = hidden[b, skip[b]:lens[b]]
        n = len(rows)
        if n == 0:
            continue
        if pooling == "max":
            out[b] = rows.max(0)
        elif pooling == "mean":
            out[b] = rows.sum(0) / max(float(n), 1e-9)
        else:
            out[b] = rows.sum(0) / np.sqrt(float(n))
    if normalize:
        out = out / np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-12)
    return out


def _read_json(path: str):
    with open(path) as f:
        return json.load(f)


def sentence_config(path: str) -> dict:
    """What a local sentence-transformers directory says about the ends of its forward: {"pooling", "normalize",
    "include_prompt", "prompts", "default_prompt_name", "similarity_fn_name"}.  Reads modules.json (Transformer,
    then Pooling, then optionally Normalize: any other module type raises ValueError naming it), the Pooling
    module's config.json and config_sentence_transformers.json; a directory without modules.json is a plain Hugging
    Face one: mean, normalise, no prompts.  No GPU, no torch."""
    out = {"pooling": "mean", "normalize": True, "include_prompt": True, "prompts": {}, "default_prompt_name": None,
           "similarity_fn_name": None}
    st_cfg = os.path.join(path, "config_sentence_transformers.json")
    if os.path.exists(st_cfg):
        c = _read_json(st_cfg)
        out["prompts"] = {str(k): str(v) for k, v in (c.get("prompts") or {}).items()}
        out["default_prompt_name"] = c.get("default_prompt_name")
        out["similarity_fn_name"] = c.get("similarity_fn_name")
    mod_path = os.path.join(path, "modules.json")
    if not os.path.exists(mod_path):
        return out
    mods = sorted(_read_json(mod_path), key=lambda m: m.get("idx", 0))
    types = [str(m.get("type", "")) for m in mods]
    for t in types:
        if t not in (_ST + "Transformer", _ST + "Pooling", _ST + "Normalize"):
            raise ValueError(f"modules.json: module type {t!r} is not supported (Transformer, Pooling and Normalize are)")
    if types[:2] != [_ST + "Transformer", _ST + "Pooling"] or types[2:] not in ([], [_ST + "Normalize"]):
        raise ValueError(f"modules.json: expected Transformer, Pooling and optionally Normalize, found {types}")
    out["normalize"] = len(types) == 3
    pc = _read_json(os.path.join(path, mods[1].get("path", "1_Pooling"), "config.json"))
    for flag, name in _UNOFFERED_FLAGS.items():
        if pc.get(flag):
            raise ValueError(f"Pooling config: {name} pooling ({flag}) is not offered")
    on = [name for flag, name in _POOLING_FLAGS.items() if pc.get(flag)]
    if len(on) != 1:
        raise ValueError("Pooling config: exactly one pooling mode must be true (concatenated outputs are not "
                         f"offered), found {on or 'none'}")
    out["pooling"] = on[0]
    hc_path = os.path.join(path, "config.json")
    hidden = _read_json(hc_path)["hidden_size"] if os.path.exists(hc_path) else MINILM_L6["hidden"]
    if "word_embedding_dimension" in pc and pc["word_embedding_dimension"] != hidden:
        raise ValueError(f"Pooling config: word_embedding_dimension {pc['word_embedding_dimension']} is not the "
                         f"model's hidden size {hidden}")
    out["include_prompt"] = bool(pc.get("include_prompt", True))
    return out


def stack_hf_state_dict(sd: dict, cfg: dict) -> dict:
    """Hugging Face BertModel tensor names -> the stacked layout of rf_encoder_weights."""
    def get(name):
        for prefix in ("", "bert.", "0.auto_model."):
            if prefix + name in sd:
                return np.asarray(sd[prefix + name], dtype=np.float32)
        raise KeyError(f"checkpoint lacks {name}")
    L = cfg["layers"]
    lay = lambda l, n: get(f"encoder.layer.{l}.{n}")
    return {
        "word_emb": get("embeddings.word_embeddings.weight"),
        "pos_emb": get("embeddings.position_embeddings.weight"),
        "type_emb": get("embeddings.token_type_embeddings.weight"),
        "emb_ln_g": get("embeddings.LayerNorm.weight"), "emb_ln_b": get("embeddings.LayerNorm.bias"),
        "qkv_w": np.stack([np.concatenate([lay(l, "attention.self.query.weight"),
                                           lay(l, "attention.self.key.weight"),
                                           lay(l, "attention.self.value.weight")]) for l in range(L)]),
        "qkv_b": np.stack([np.concatenate([lay(l, "attention.self.query.bias"),
                                           lay(l, "attention.self.key.bias"),
                                           lay(l, "attention.self.value.bias")]) for l in range(L)]),
        "ao_w": np.stack([lay(l, "attention.output.dense.weight") for l in range(L)]),
        "ao_b": np.stack([lay(l, "attention.output.dense.bias") for l in range(L)]),
        "ln1_g": np.stack([lay(l, "attention.output.LayerNorm.weight") for l in range(L)]),
        "ln1_b": np.stack([lay(l, "attention.output.LayerNorm.bias") for l in range(L)]),
        "ff1_w": np.stack([lay(l, "intermediate.dense.weight") for l in range(L)]),
        "ff1_b": np.stack([lay(l, "intermediate.dense.bias") for l in range(L)]),
        "ff2_w": np.stack([lay(l, "output.dense.weight") for l in range(L)]),
        "ff2_b": np.stack([lay(l, "output.dense.bias") for l in range(L)]),
        "ln2_g": np.stack([lay(l, "output.LayerNorm.weight") for l in range(L)]),
        "ln2_b": np.stack([lay(l, "output.LayerNorm.bias") for l in range(L)]),
    }


def stack_hf_pair_head(sd: dict) -> dict:
    """The classification head of a Hugging Face BertForSequenceClassification state dict -> the tensors of
    rf_pair_head: the pooler (dense + tanh on the [CLS] row) and the classifier on top of it."""
    def get(name):
        if name not in sd:
            raise KeyError(f"checkpoint lacks {name} (not a BertForSequenceClassification?)")
        return np.asarray(sd[name], dtype=np.float32)
    return {"pool_w": get("bert.pooler.dense.weight"), "pool_b": get("bert.pooler.dense.bias"),
            "cls_w": get("classifier.weight"), "cls_b": get("classifier.bias")}


def stack_hf_qa_head(sd: dict) -> dict:
    """The span head of a Hugging Face BertForQuestionAnswering state dict -> the tensors of rf_qa_head:
    qa_outputs, row 0 the start logit's, row 1 the end logit's."""
    def get(name):
        if name not in sd:
            raise KeyError(f"checkpoint lacks {name} (not a BertForQuestionAnswering?)")
        return np.asarray(sd[name], dtype=np.float32)
    return {"qa_w": get("qa_outputs.weight"), "qa_b": get("qa_outputs.bias")}


def stack_hf_tag_head(sd: dict) -> dict:
    """The token classifier of a Hugging Face BertForTokenClassification state dict -> the tensors of rf_tag_head:
    classifier.weight [num_labels, H], row c the logit of label c, and classifier.bias [num_labels]."""
    def get(name):
        if name not in sd:
            raise KeyError(f"checkpoint lacks {name} (not a BertForTokenClassification?)")
        return np.asarray(sd[name], dtype=np.float32)
    return {"cls_w": get("classifier.weight"), "cls_b": get("classifier.bias")}


def hf_encoder_config(hc: dict) -> dict:
    """config.json of a BERT checkpoint -> the fields of rf_encoder_config."""
    if hc.get("hidden_act", "gelu") != "gelu":
        raise _lib.RagfinError(-2, f"activation {hc.get('hidden_act')} is not supported (gelu only)")
    return dict(vocab_size=hc["vocab_size"], hidden=hc["hidden_size"], layers=hc["num_hidden_layers"],
                heads=hc["num_attention_heads"], intermediate=hc["intermediate_size"],
                max_position=hc["max_position_embeddings"], type_vocab=hc.get("type_vocab_size", 2),
                ln_eps=hc.get("layer_norm_eps", 1e-12))


def random_weights(cfg: dict, seed: int = 0, scale: float = 0.05) -> dict:
    """Seeded random weights of the named architecture (no checkpoint exists offline): same generator as the
    test oracle so both sides can be rebuilt from the seed alone."""
    rng = np.random.default_rng(seed)
    H, L, I = cfg["hidden"], cfg["layers"], cfg["intermediate"]

    def mat(*shape, s=scale):
        return (rng.standard_normal(shape, dtype=np.float32) * s).astype(np.float32)
    return {"word_emb": mat(cfg["vocab_size"], H), "pos_emb": mat(cfg["max_position"], H),
            "type_emb": mat(cfg["type_vocab"], H), "emb_ln_g": 1 + mat(H, s=0.1), "emb_ln_b": mat(H, s=0.1),
            "qkv_w": mat(L, 3 * H, H), "qkv_b": mat(L, 3 * H, s=0.02), "ao_w": mat(L, H, H),
            "ao_b": mat(L, H, s=0.02), "ln1_g": 1 + mat(L, H, s=0.1), "ln1_b": mat(L, H, s=0.1),
            "ff1_w": mat(L, I, H), "ff1_b": mat(L, I, s=0.02), "ff2_w": mat(L, H, I),
            "ff2_b": mat(L, H, s=0.02), "ln2_g": 1 + mat(L, H, s=0.1), "ln2_b": mat(L, H, s=0.1)}


class Embedder:
    """`encode(list[str]) -> np.float32 [n, 384]`: unit-norm mean-pooled rows by default, or what the model's own
    Pooling / Normalize modules and prompts say (pooling=, normalize=, prompts=: from_local reads them)."""

    def __init__(self, weights: dict, cfg: dict | None = None, tokenizer: WordPieceTokenizer | None = None,
                 device=None, max_seq_length: int = 256, pooling: str | None = None, normalize: bool | None = None,
                 prompts: dict | None = None, default_prompt_name: str | None = None, include_prompt: bool | None = None,
                 similarity_fn_name: str | None = None):
        torch = _torch()
        self._set_ends(pooling, normalize, prompts, default_prompt_name, include_prompt, similarity_fn_name)
        self.cfg = dict(cfg or MINILM_L6)
        self.device = require_gpu(device)
        self.lib = _lib.load_library()
        self.tokenizer = tokenizer
        self.max_seq_length = min(max_seq_length, self.cfg["max_position"])
        self.dim = self.cfg["hidden"]
        c = self.cfg
        self._cfg_c = _lib.EncoderConfig(c["vocab_size"], c["hidden"], c["layers"], c["heads"],
                                         c["intermediate"], c["max_position"], c["type_vocab"],
                                         c["ln_eps"])
        nbytes = self.lib.rf_encoder_storage_bytes(ctypes.byref(self._cfg_c))
        if nbytes == 0:
            raise _lib.RagfinError(-2, f"encoder config not supported by the HIP kernels: {c}")
        # fp16 device copies of every tensor (kept alive: the library keeps pointers)
        self._w = {}
        wc = _lib.EncoderWeights()
        for name in _lib.ENCODER_WEIGHT_FIELDS:
            t = torch.as_tensor(np.ascontiguousarray(weights[name])).to(torch.float16)
            t = t.to(self.device).contiguous()
            self._w[name] = t
            setattr(wc, name, t.data_ptr())
        with torch.cuda.device(self.device):
            self._storage = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            h = c_void_p()
            _lib.check(self.lib.rf_encoder_create(ctypes.byref(h), ctypes.byref(self._cfg_c),
                                                  ctypes.byref(wc), c_void_p(self._storage.data_ptr()),
                                                  nbytes, self.device.index, _lib.current_stream_ptr()))
        self.handle = h
        # Threading: the handle holds no per-call state, so concurrent encodes only
        # have to keep their BUFFERS apart.  Large batches take a workspace of their own per call
        # (torch's caching allocator: stream-ordered reuse, no hipMalloc in steady state).
        # Query-sized batches share fixed staging buffers (rf_encode replays a hipGraph keyed by
        # their addresses) and serialise on _small_lock; _small_done orders a caller on another
        # stream behind the previous use.  The chunked text ingest (pinned staging, copy stream)
        # runs one at a time under _ingest_lock.
        self._small_ws = None
        self._small_lock = threading.Lock()
        self._small_done = None
        self._ingest_lock = threading.Lock()
        self._copy_stream = None
        self._pin = None

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.lib.rf_encoder_destroy(h)
            self.handle = None

    # -- construction -----------------------------------------------------------------
    def _set_ends(self, pooling=None, normalize=None, prompts=None, default_prompt_name=None, include_prompt=None,
                  similarity_fn_name=None):
        """The ends of the forward and the prompts (None: mean, normalise, no prompts -- all-MiniLM's)."""
        self.pooling = check_pooling("mean" if pooling is None else pooling)
        self.normalize = True if normalize is None else bool(normalize)
        self.prompts = {str(k): str(v) for k, v in (prompts or {}).items()}
        self.default_prompt_name = default_prompt_name
        if default_prompt_name is not None and default_prompt_name not in self.prompts:
            raise ValueError(f"default_prompt_name {default_prompt_name!r} is not one of the prompts "
                             f"({', '.join(sorted(self.prompts)) or 'none are set'})")
        self.include_prompt = True if include_prompt is None else bool(include_prompt)
        self.similarity_fn_name = similarity_fn_name

    @property
    def query_prompt(self):
        """The prompt queries are embedded with (prompts["query"]), or None."""
        return self.prompts.get("query")

    @property
    def document_prompt(self):
        """The prompt chunks are embedded with: the first of prompts' "document", "passage", "corpus", or None."""
        return next((self.prompts[k] for k in ("document", "passage", "corpus") if k in self.prompts), None)

    def _resolve_prompt(self, prompt_name=None, prompt=None):
        """sentence-transformers' rule: prompt wins over prompt_name, which wins over default_prompt_name."""
        if prompt is not None:
            return prompt
        name = prompt_name if prompt_name is not None else self.default_prompt_name
        if name is None:
            return None
        if name not in self.prompts:
            raise ValueError(f"prompt name {name!r} is not one of the prompts "
                             f"({', '.join(sorted(self.prompts)) or 'none are set'})")
        return self.prompts[name]

    def _prompt_skip(self, prompt):
        """How many leading tokens of a row "prompt + text" the pooled set leaves out: the token count of the prompt
        tokenised alone minus its [SEP] ([CLS] is therefore left out too, as sentence-transformers does) when
        include_prompt is false and the pooling is over a set; None otherwise.  A prompt that leaves no room for a
        text token and the closing [SEP] within max_seq_length raises ValueError."""
        if not prompt:
            return None
        k = len(self.tokenizer.encode(prompt, 1 << 30)) - 1
        if k + 2 > self.max_seq_length:
            raise ValueError(f"the prompt takes {k} tokens with [CLS]: no room for a text token within "
                             f"max_seq_length {self.max_seq_length}")
        return k if (not self.include_prompt and self.pooling != "cls") else None

    @classmethod
    def from_local(cls, path: str, device=None, max_seq_length: int | None = None, pooling: str | None = None,
                   normalize: bool | None = None, prompts: dict | None = None, default_prompt_name: str | None = None,
                   include_prompt: bool | None = None) -> "Embedder":
        """Load config.json + vocab.txt + model.safetensors from a local directory
        (e.g. a copy of sentence-transformers/all-MiniLM-L6-v2).  Nothing is downloaded.
        The pooling mode, the Normalize module, the prompts and the similarity function are the directory's own
        (sentence_config); a keyword argument overrides what it says -- E5 ships no prompts in its files:
        prompts={"query": "query: ", "document": "passage: "}."""
        from safetensors.numpy import load_file
        sc = sentence_config(path)
        ends = dict(pooling=sc["pooling"] if pooling is None else pooling,
                    normalize=sc["normalize"] if normalize is None else normalize,
                    prompts=sc["prompts"] if prompts is None else prompts,
                    default_prompt_name=sc["default_prompt_name"] if default_prompt_name is None else default_prompt_name,
                    include_prompt=sc["include_prompt"] if include_prompt is None else include_prompt,
                    similarity_fn_name=sc["similarity_fn_name"])
        if prompts is not None and default_prompt_name is None and ends["default_prompt_name"] not in ends["prompts"]:
            ends["default_prompt_name"] = None      # the directory's default names a prompt the override dropped
        with open(os.path.join(path, "config.json")) as f:
            hc = json.load(f)
        cfg = hf_encoder_config(hc)
        sd = load_file(os.path.join(path, "model.safetensors"))
        tok = WordPieceTokenizer.from_vocab_file(os.path.join(path, "vocab.txt"))
        msl = max_seq_length
        sbert_cfg = os.path.join(path, "sentence_bert_config.json")
        if msl is None and os.path.exists(sbert_cfg):
            with open(sbert_cfg) as f:
                msl = json.load(f).get("max_seq_length")
        return cls(stack_hf_state_dict(sd, cfg), cfg, tok, device, msl or 256, **ends)

    @classmethod
    def from_random(cls, cfg: dict | None = None, seed: int = 0, tokenizer=None, device=None,
                    scale: float = 0.05, pooling: str | None = None, normalize: bool | None = None) -> "Embedder":
        """Seeded random weights of the named architecture (no checkpoint exists
        offline): same generator as the test oracle so both sides can be rebuilt
        from the seed alone."""
        cfg = dict(cfg or MINILM_L6)
        w = random_weights(cfg, seed, scale)
        return cls(w, cfg, tokenizer, device, pooling=pooling, normalize=normalize)

    # -- forward ------------------------------------------------------------------------
    def encode_ids(self, ids, lens, out_dtype="float16", skip=None, normalize=None):
        """ids int32 [B, T], lens int32 [B] (tensors or arrays) -> [B, 384] tensor on
        the device (fp16 by default: exactly what CorpusStore stores).
        skip int32 [B] or None: leading tokens of each row left out of the pooled set (a prompt's).  normalize=True
        normalises the output of a model without a Normalize module; False changes nothing on a model with one.
        Mean + normalise without skip is rf_encode (small-batch staging, graph replay); anything else is
        rf_encode_sentences on the same two routes."""
        torch = _torch()
        ids = torch.as_tensor(ids, dtype=torch.int32)
        lens = torch.as_tensor(lens, dtype=torch.int32)
        if ids.dim() != 2 or lens.shape != (ids.shape[0],):
            raise ValueError("encode_ids expects ids [B, T] and lens [B]")
        norm = self.normalize or bool(normalize)
        head = None
        if skip is not None or self.pooling != "mean" or not norm:
            head = _lib.SentenceHead(POOLING_MODES[self.pooling], int(norm))
        if skip is not None:
            skip = torch.as_tensor(skip, dtype=torch.int32)
            if skip.shape != lens.shape:
                raise ValueError("encode_ids expects skip [B]")
        B, T = ids.shape
        if T > self.cfg["max_position"]:
            raise ValueError(f"T={T} exceeds max_position {self.cfg['max_position']}")
        want32 = out_dtype in ("float32", np.float32)
        small = B * T <= self.SMALL_SLOTS
        if small:
            with self._small_lock:   # the staging buffers are shared: enqueue copy + forward + clone as one unit
                return self._encode_small(ids, lens, B, T, want32, head, skip)
        return self._encode_large(ids, lens, B, T, want32, head, skip)

    def _launch(self, ids, lens, B, T, out16, out32, ws=None, head=None, skip=None):
        torch = _torch()
        with torch.cuda.device(self.device):
            if ws is None:   # per call: concurrent encodes (any thread, any stream) never share scratch
                ws = torch.empty(self.lib.rf_encode_workspace_bytes(self.handle, B, T), dtype=torch.uint8,
                                 device=self.device)
            if head is not None:   # the model's own pooling head: always plain launches
                _lib.check(self.lib.rf_encode_sentences(
                    self.handle, c_void_p(ids.data_ptr()), c_void_p(lens.data_ptr()),
                    c_void_p(skip.data_ptr()) if skip is not None else None, B, T, ctypes.byref(head),
                    c_void_p(out16.data_ptr()) if out16 is not None else None,
                    c_void_p(out32.data_ptr()) if out32 is not None else None,
                    c_void_p(ws.data_ptr()), ws.numel(), _lib.current_stream_ptr()))
                return
            _lib.check(self.lib.rf_encode(self.handle, c_void_p(ids.data_ptr()), c_void_p(lens.data_ptr()),
                                          B, T, c_void_p(out16.data_ptr()) if out16 is not None else None,
                                          c_void_p(out32.data_ptr()) if out32 is not None else None,
                                          c_void_p(ws.data_ptr()), ws.numel(),
                                          _lib.current_stream_ptr()))

    def _encode_large(self, ids, lens, B, T, want32, head=None, skip=None):
        torch = _torch()
        ids = ids.to(self.device).contiguous()
        lens = lens.to(self.device).contiguous()
        if skip is not None:
            skip = skip.to(self.device).contiguous()
        out16 = None if want32 else torch.empty((B, self.dim), dtype=torch.float16, device=self.device)
        out32 = torch.empty((B, self.dim), dtype=torch.float32, device=self.device) if want32 else None
        self._launch(ids, lens, B, T, out16, out32, head=head, skip=skip)
        return out32 if want32 else out16

    def _encode_small(self, ids, lens, B, T, want32, head=None, skip=None):
        # a query-sized batch: fixed staging buffers, so that rf_encode sees the same pointers call
        # after call and replays its cached hipGraph instead of ~45 launches (the result is cloned)
        torch = _torch()
        sb = self._small_buffers()
        cur = torch.cuda.current_stream(self.device)
        if self._small_done is not None:
            cur.wait_event(self._small_done)     # a previous caller on ANOTHER stream may still be using the buffers
        # rf_encode keys its cached hipGraphs on (B, T, buffers) and the tokenizer returns T = the longest row, so every
        # query length would be a key of its own: round the width up (padding changes no bit:
        # tests/test_encoder_gpu.py::test_padding_content_and_width_are_ignored) -- to a multiple of 8 up to 32 tokens
        # (a lone query is 5-20 tokens: its forward should not grow to 32 rows), of 32 beyond: at most 11 widths per
        # batch size.  Host ids are padded on the host (one upload, no extra launch); device ids with two small kernels.
        Tr = (T + 7) // 8 * 8 if T <= 32 else (T + 31) // 32 * 32
        Tr = min(Tr, self.cfg["max_position"])
        if B * Tr > self.SMALL_SLOTS:
            Tr = T
        if ids.device.type == "cpu" and lens.device.type == "cpu":
            # Host inputs go through PINNED staging buffers owned by the embedder: an asynchronous copy from pageable
            # memory reads its source when the copy RUNS, and the caller's arrays (or a padded temporary made here) can
            # be freed and reused before that -- seen as a rare wrong hit when two ranks share one card
            # (tests/test_sharded_gpu.py::test_world2_sharded_store_behind_vector_rag).  The buffers are rewritten only
            # after the previous use's copy has run (host wait on its event: already complete in a serving loop).
            if self._small_done is not None:
                self._small_done.synchronize()
            hid = sb["ids_host"][:B * Tr].view(B, Tr)
            hid[:, :T] = ids
            if Tr != T:
                hid[:, T:] = 0
            sb["lens_host"][:B] = lens
            sb["ids"][:B * Tr].copy_(sb["ids_host"][:B * Tr], non_blocking=True)
            sb["lens"][:B].copy_(sb["lens_host"][:B], non_blocking=True)
            if skip is not None:
                if skip.device.type == "cpu":
                    sb["skip_host"][:B] = skip
                    sb["skip"][:B].copy_(sb["skip_host"][:B], non_blocking=True)
                else:
                    sb["skip"][:B].copy_(skip)
        else:
            ids = ids.to(self.device, non_blocking=False)
            lens = lens.to(self.device, non_blocking=False)
            wide = sb["ids"][:B * Tr].view(B, Tr)
            wide[:, :T].copy_(ids)
            if Tr != T:
                wide[:, T:].zero_()
            sb["lens"][:B].copy_(lens)
            if skip is not None:
                sb["skip"][:B].copy_(skip.to(self.device, non_blocking=False))
        T = Tr
        ids, lens = sb["ids"], sb["lens"]
        if skip is not None:
            skip = sb["skip"]
        out16 = None if want32 else sb["o16"]
        out32 = sb["o32"] if want32 else None
        self._launch(ids, lens, B, T, out16, out32, ws=self._small_ws, head=head, skip=skip)
        res = (out32 if want32 else out16)[:B].clone()
        if self._small_done is None:
            self._small_done = torch.cuda.Event()
        self._small_done.record(cur)
        return res

    SMALL_SLOTS = 1024   # = SM_MAX_TOK of csrc/encoder.hip: the small-batch GEMM path / hipGraph replay

    def _small_buffers(self):
        torch = _torch()
        if getattr(self, "_sb", None) is None:
            n = self.SMALL_SLOTS
            self._sb = {"ids": torch.zeros(n, dtype=torch.int32, device=self.device),
                        "lens": torch.zeros(n, dtype=torch.int32, device=self.device),
                        "ids_host": torch.zeros(n, dtype=torch.int32).pin_memory(),
                        "lens_host": torch.zeros(n, dtype=torch.int32).pin_memory(),
                        "skip": torch.zeros(n, dtype=torch.int32, device=self.device),
                        "skip_host": torch.zeros(n, dtype=torch.int32).pin_memory(),
                        "o16": torch.zeros((n, self.dim), dtype=torch.float16, device=self.device),
                        "o32": torch.zeros((n, self.dim), dtype=torch.float32, device=self.device)}
            # workspace large enough for every small shape: its pointer must not move either
            nbytes = max(self.lib.rf_encode_workspace_bytes(self.handle, n, 1),
                         self.lib.rf_encode_workspace_bytes(self.handle, max(1, n // 256), 256))
            self._small_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._sb

    def encode_to_device(self, sentences, batch_tokens: int = 65536, out_dtype="float16", prompt=None, normalize=None):
        """Tokenise, bucket by length, encode; returns fp16 (default: what CorpusStore keeps) or
        fp32 [n, 384] on the device in the input order.
        prompt: a string prepended to every text before tokenisation (the model's "query: " / "passage: "; with
        include_prompt false its tokens are left out of the pooled set).  normalize: as for encode_ids."""
        held = [False]    # the chunked path takes _ingest_lock on first use (queries never do)
        try:
            return self._encode_to_device(sentences, batch_tokens, out_dtype, held, prompt, normalize)
        finally:
            if held[0]:
                self._ingest_lock.release()

    def _encode_to_device(self, sentences, batch_tokens, out_dtype, held, prompt=None, normalize=None):
        torch = _torch()
        want32 = out_dtype in ("float32", np.float32)
        odt = torch.float32 if want32 else torch.float16
        if self.tokenizer is None:
            raise RuntimeError("Embedder has no tokenizer: construct it with from_local(path) or pass "
                               "tokenizer=WordPieceTokenizer(vocab)")
        if isinstance(sentences, str):
            sentences = [sentences]
        # text -> ids through the native tokenizer (csrc/tokenizer.cpp, one thread per host core);
        # a tokenizer object without batch_native (a test double) takes the per-sentence path.
        # Large inputs go in chunks of `chunk_texts`: rf_encode only ENQUEUES, so while the GPU works
        # through one chunk's buckets the host is already tokenising the next chunk.
        import time
        sentences = list(sentences)
        n = len(sentences)
        skip_n = self._prompt_skip(prompt)       # (refuses a prompt that leaves no room for text)
        if prompt:
            sentences = [prompt + s for s in sentences]
        ends = {} if normalize is None else {"normalize": normalize}
        out = torch.empty((n, self.dim), dtype=odt, device=self.device)
        if n == 0:
            return out
        # host seconds per stage of the last call (bench.py reports them beside from_text): the GPU work is only
        # ENQUEUED below, so whatever the host spends here in series is time the card may sit idle
        stats = self.ingest_stats = {"prepass_s": 0.0, "native_tokenize_s": 0.0, "sort_s": 0.0, "pinned_wait_s": 0.0, "pinned_stage_s": 0.0,
                                     "upload_enqueue_s": 0.0, "bucket_and_launch_s": 0.0, "chunks": 0, "buckets": 0}

        def lap(key, t0):
            t1 = time.perf_counter()
            stats[key] += t1 - t0
            return t1
        chunk_texts = int(os.environ.get("RAGFIN_INGEST_CHUNK_TEXTS", "4096"))   # (tools/ingest_probe.py sweeps it)
        # the first chunk is a quarter of the others: nothing overlaps ITS tokenisation, so the
        # GPU should get its first buckets early
        starts = [0] + list(range(min(n, chunk_texts // 4), n, chunk_texts))
        for ci, c0 in enumerate(starts):
            part = sentences[c0:(starts[ci + 1] if ci + 1 < len(starts) else n)]
            stats["chunks"] += 1
            tm = time.perf_counter()
            if hasattr(self.tokenizer, "batch_native"):
                all_ids, all_lens = self.tokenizer.batch_native(part, self.max_seq_length)
                lt = getattr(self.tokenizer, "last_timing", None)
                if lt:
                    stats["prepass_s"] += lt["prepass_s"]
                    stats["native_tokenize_s"] += lt["native_s"]
            else:
                rows = [self.tokenizer.encode(s, self.max_seq_length) for s in part]
                all_lens = np.array([len(r) for r in rows], dtype=np.int32)
                all_ids = np.full((len(rows), max(int(all_lens.max()), 1) if len(rows) else 1),
                                  self.tokenizer.pad_id, dtype=np.int32)
                for r, row in enumerate(rows):
                    all_ids[r, :len(row)] = row
            m = len(part)
            if m * int(all_ids.shape[1]) <= self.SMALL_SLOTS:
                # a query or a handful: straight to the small-batch path (no sorting, no side stream)
                if skip_n is not None:
                    ends["skip"] = np.full(m, skip_n, dtype=np.int32)
                out[c0:c0 + m] = self.encode_ids(all_ids, all_lens, out_dtype=out_dtype, **ends)
                continue
            if not held[0]:      # pinned staging buffers + copy stream below are one-at-a-time
                self._ingest_lock.acquire()
                held[0] = True
            tm = time.perf_counter()
            order = np.argsort(all_lens, kind="stable")
            sorted_lens = all_lens[order].astype(np.int64)
            tm = lap("sort_s", tm)
            # ONE upload per chunk, from pinned memory on a side stream: a pageable host-to-device copy
            # on the compute stream would make the host wait for every kernel already queued there, and
            # the chunk-to-chunk overlap would be gone.  Buckets are then gathered ON the device.
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(device=self.device)
            # two sets of pinned staging buffers used alternately, so that chunk k+1 can be staged
            # while chunk k's copy is still in flight (allocating pinned memory per chunk would
            # synchronise the device each time)
            Tc = int(all_ids.shape[1])
            if self._pin is None:
                cap = chunk_texts * self.max_seq_length
                self._pin = [dict(ids=torch.empty(cap, dtype=torch.int32).pin_memory(),
                                  lens=torch.empty(chunk_texts, dtype=torch.int32).pin_memory(),
                                  order=torch.empty(chunk_texts, dtype=torch.int64).pin_memory(),
                                  done=None) for _ in range(2)]
            pb = self._pin[ci & 1]
            if pb["done"] is not None:
                pb["done"].synchronize()      # its previous upload has left the buffers
            tm = lap("pinned_wait_s", tm)
            # numpy views of the pinned buffers: a plain memcpy on this thread (torch's CPU copy_ fans a 4 MB copy
            # out over every OpenMP thread of the host, which a container's CPU quota punishes: hostcpu.py)
            pb["ids"].numpy()[:m * Tc].reshape(m, Tc)[...] = all_ids
            pb["lens"].numpy()[:m] = all_lens
            pb["order"].numpy()[:m] = order
            tm = lap("pinned_stage_s", tm)
            with torch.cuda.stream(self._copy_stream):
                ids_dev = pb["ids"][:m * Tc].view(m, Tc).to(self.device, non_blocking=True)
                lens_dev = pb["lens"][:m].to(self.device, non_blocking=True)
                order_dev = pb["order"][:m].to(self.device, non_blocking=True)
                ready = torch.cuda.Event()
                ready.record()
            pb["done"] = ready
            torch.cuda.current_stream(self.device).wait_event(ready)
            for t in (ids_dev, lens_dev, order_dev):
                t.record_stream(torch.cuda.current_stream(self.device))
            # a row's skip travels with it through the gather below
            skip_dev = None if skip_n is None else torch.full((m,), skip_n, dtype=torch.int32, device=self.device)
            tm = lap("upload_enqueue_s", tm)
            i = 0
            while i < m:
                stats["buckets"] += 1
                # rows are sorted ascending, so the last row of a bucket sets its width and
                # (rows in bucket) x (that width) is non-decreasing in the bucket's end: binary search
                cost = (np.arange(1, m - i + 1, dtype=np.int64)) * sorted_lens[i:]
                j = i + max(1, int(np.searchsorted(cost, batch_tokens, side="right")))
                T = int(sorted_lens[j - 1])
                sel = order_dev[i:j]
                ids = ids_dev.index_select(0, sel)[:, :T].contiguous()
                lens = lens_dev.index_select(0, sel)
                if skip_dev is not None:
                    ends["skip"] = skip_dev.index_select(0, sel)
                out.index_copy_(0, sel + c0, self.encode_ids(ids, lens, out_dtype=out_dtype, **ends))
                i = j
            lap("bucket_and_launch_s", tm)
        return out

    def encode(self, sentences, batch_size: int = 32, prompt_name: str | None = None, prompt: str | None = None,
               normalize_embeddings: bool | None = None, **_ignored) -> np.ndarray:
        """sentence-transformers' signature: numpy float32 [n, 384] (or [384] for a str) --
        rf_encode's fp32 output (the reference returns fp32, vector_rag_mcp/main.py:50), not the
        fp16 rows the store keeps.
        prompt wins over prompt_name, which wins over default_prompt_name; an unknown name raises ValueError.
        normalize_embeddings=True normalises (on the GPU) the output of a model without a Normalize module; False
        on a model with one changes nothing, as in sentence-transformers."""
        single = isinstance(sentences, str)
        p = self._resolve_prompt(prompt_name, prompt)
        emb = self.encode_to_device([sentences] if single else list(sentences), out_dtype="float32",
                                    **({"prompt": p} if p else {}),
                                    **({"normalize": True} if normalize_embeddings else {}))
        arr = emb.cpu().numpy()
        return arr[0] if single else arr

    def _encode_as(self, names, sentences, kw):
        if kw.get("prompt") is None and kw.get("prompt_name") is None:
            name = next((k for k in names if k in self.prompts), None)
            if name is not None:
                kw = dict(kw, prompt_name=name)
        return self.encode(sentences, **kw)

    def encode_query(self, sentences, **kw) -> np.ndarray:
        """encode() with the "query" prompt, when the model has one and the call names no other."""
        return self._encode_as(("query",), sentences, kw)

    def encode_document(self, sentences, **kw) -> np.ndarray:
        """encode() with the first of the "document", "passage", "corpus" prompts, when the model has one and the
        call names no other."""
        return self._encode_as(("document", "passage", "corpus"), sentences, kw)

