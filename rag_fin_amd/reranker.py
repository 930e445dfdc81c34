"""Cross-encoder reranker on the GPU: the "retrieve fetch_k, rerank, keep top_k" stage behind the
bi-encoder search, with the interface of sentence-transformers' `CrossEncoder`
(`CrossEncoder('cross-encoder/ms-marco-MiniLM-L-6-v2').predict([(query, passage), ...])`).

The checkpoint is a LOCAL BertForSequenceClassification directory in the Hugging Face layout
(config.json, vocab.txt, model.safetensors) of the MiniLM-L{6,12}-H384 family; nothing is fetched.
The forward runs in libragfin_hip.so (rf_score_pairs): the sentence embedder's layers between a
pair embedding kernel (segment ids) and a classification head kernel; there is no CPU path.
"""
from __future__ import annotations

import ctypes
import json
import os
from ctypes import c_void_p

import numpy as np

from . import _lib
from .embedder import (MINILM_L6, Embedder, hf_encoder_config, random_weights, stack_hf_pair_head,
                       stack_hf_state_dict)
from .tokenizer import WordPieceTokenizer

HEAD_FIELDS = ["pool_w", "pool_b", "cls_w", "cls_b"]


def random_pair_head(hidden: int, seed: int = 0, scale: float = 0.05, head_scale: float = 0.05) -> dict:
    """Seeded pooler + one-label classifier (float32), a stream of its own beside random_weights(cfg, seed)."""
    rng = np.random.default_rng([seed, 1])

    def mat(*shape, s):
        return (rng.standard_normal(shape, dtype=np.float32) * s).astype(np.float32)
    return {"pool_w": mat(hidden, hidden, s=scale), "pool_b": mat(hidden, s=0.02),
            "cls_w": mat(1, hidden, s=head_scale), "cls_b": mat(1, s=0.02)}


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x.astype(np.float64)))


def _identity(x):
    return x


def resolve_activation(spec):
    """None -> None; a callable as it is; a name -- "sigmoid", "identity", or the dotted torch class path
    config.json's sbert_ce_default_activation_function holds -- to the host function."""
    if spec is None or callable(spec):
        return spec
    name = str(spec).rsplit(".", 1)[-1].lower()
    if name == "sigmoid":
        return _sigmoid
    if name == "identity":
        return _identity
    raise ValueError(f"activation {spec!r} is not supported (sigmoid, identity or a callable)")


class CrossEncoder:
    """`predict([(query, passage), ...]) -> np.float32 [n]`, `rank(query, documents)`."""

    def __init__(self, weights: dict, head: dict, cfg: dict | None = None, tokenizer: WordPieceTokenizer | None = None,
                 device=None, max_length: int | None = None, num_labels: int = 1, default_activation=None):
        import torch
        cfg = dict(cfg or MINILM_L6)
        # the BertModel part: the embedder's weight upload and encoder handle
        self.encoder = Embedder(weights, cfg, tokenizer, device)
        self.cfg, self.device, self.lib, self.tokenizer = cfg, self.encoder.device, self.encoder.lib, tokenizer
        self.max_length = min(max_length or cfg["max_position"], cfg["max_position"])
        self.num_labels = int(num_labels)
        # sentence-transformers 2.7: the configured default, else sigmoid for one label
        self.default_activation = resolve_activation(default_activation) or (_sigmoid if self.num_labels == 1 else _identity)
        H = cfg["hidden"]
        shapes = {"pool_w": (H, H), "pool_b": (H,), "cls_w": (self.num_labels, H), "cls_b": (self.num_labels,)}
        self._head = {}
        self._head_c = _lib.PairHead(num_labels=self.num_labels)
        for name in HEAD_FIELDS:
            a = np.ascontiguousarray(head[name], dtype=np.float32)
            if a.shape != shapes[name]:
                raise ValueError(f"head tensor {name} has shape {a.shape}, expected {shapes[name]}")
            t = torch.as_tensor(a).to(torch.float16).to(self.device).contiguous()
            self._head[name] = t   # kept alive: the library reads them in every call
            setattr(self._head_c, name, t.data_ptr())

    # -- construction -----------------------------------------------------------------
    @classmethod
    def from_local(cls, path: str, device=None, max_length: int | None = None) -> "CrossEncoder":
        """Load config.json + vocab.txt + model.safetensors of a BertForSequenceClassification checkpoint
        (e.g. a copy of cross-encoder/ms-marco-MiniLM-L-6-v2) from a local directory."""
        from safetensors.numpy import load_file
        with open(os.path.join(path, "config.json")) as f:
            hc = json.load(f)
        cfg = hf_encoder_config(hc)
        sd = load_file(os.path.join(path, "model.safetensors"))
        tok = WordPieceTokenizer.from_vocab_file(os.path.join(path, "vocab.txt"))
        head = stack_hf_pair_head(sd)
        return cls(stack_hf_state_dict(sd, cfg), head, cfg, tok, device, max_length,
                   num_labels=head["cls_w"].shape[0],
                   default_activation=hc.get("sbert_ce_default_activation_function"))

    @classmethod
    def from_random(cls, cfg: dict | None = None, seed: int = 0, tokenizer=None, device=None, scale: float = 0.05,
                    head_scale: float = 0.05, max_length: int | None = None) -> "CrossEncoder":
        """Seeded random weights (random_weights(cfg, seed) + random_pair_head(hidden, seed)): both sides of a
        test can be rebuilt from the seed alone."""
        cfg = dict(cfg or MINILM_L6)
        return cls(random_weights(cfg, seed, scale), random_pair_head(cfg["hidden"], seed, scale, head_scale), cfg,
                   tokenizer, device, max_length)

    # -- forward ------------------------------------------------------------------------
    def score_ids(self, ids, lens, seg):
        """ids int32 [B, T] ([CLS] q [SEP] d [SEP], padded), lens int32 [B], seg int32 [B] (index of the first
        document token) -> raw logits, float32 [B] on the device."""
        import torch
        ids = torch.as_tensor(ids, dtype=torch.int32)
        lens = torch.as_tensor(lens, dtype=torch.int32)
        seg = torch.as_tensor(seg, dtype=torch.int32)
        if ids.dim() != 2 or lens.shape != (ids.shape[0],) or seg.shape != lens.shape:
            raise ValueError("score_ids expects ids [B, T], lens [B] and seg [B]")
        B, T = ids.shape
        ids, lens, seg = (t.to(self.device).contiguous() for t in (ids, lens, seg))
        h = self.encoder.handle
        with torch.cuda.device(self.device):
            out = torch.empty(B, dtype=torch.float32, device=self.device)
            # per call: concurrent calls (any thread, any stream) never share scratch
            ws = torch.empty(self.lib.rf_encode_workspace_bytes(h, B, T), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.rf_score_pairs(h, c_void_p(ids.data_ptr()), c_void_p(lens.data_ptr()),
                                               c_void_p(seg.data_ptr()), B, T, ctypes.byref(self._head_c),
                                               c_void_p(out.data_ptr()), c_void_p(ws.data_ptr()), ws.numel(),
                                               _lib.current_stream_ptr()))
        return out

    def predict(self, pairs, activation=None, batch_tokens: int = 65536) -> np.ndarray:
        """Scores of (query, passage) pairs, np.float32 [n] in the input order.  activation: a callable on the
        logits array, "sigmoid" or "identity"; when not given, config.json's
        sbert_ce_default_activation_function, else sigmoid.  It is applied on the host."""
        import torch
        if self.tokenizer is None:
            raise RuntimeError("CrossEncoder has no tokenizer: construct it with from_local(path) or pass "
                               "tokenizer=WordPieceTokenizer(vocab)")
        pairs = list(pairs)
        act = resolve_activation(activation) or self.default_activation
        if not pairs:
            return np.zeros((0,), dtype=np.float32)
        ids, lens, seg = self.tokenizer.batch_pairs([p[0] for p in pairs], [p[1] for p in pairs], self.max_length)
        # length-sorted buckets of about batch_tokens token slots, like the text ingest: rows are sorted
        # ascending, so a bucket's last row sets its width
        order = np.argsort(lens, kind="stable")
        sorted_lens = lens[order].astype(np.int64)
        n = len(pairs)
        logits = torch.empty(n, dtype=torch.float32, device=self.device)
        i = 0
        while i < n:
            cost = np.arange(1, n - i + 1, dtype=np.int64) * sorted_lens[i:]
            j = i + max(1, int(np.searchsorted(cost, batch_tokens, side="right")))
            sel = order[i:j]
            T = int(sorted_lens[j - 1])
            logits[torch.as_tensor(sel, device=self.device)] = self.score_ids(
                np.ascontiguousarray(ids[sel, :T]), lens[sel], seg[sel])
            i = j
        return np.asarray(act(logits.cpu().numpy()), dtype=np.float32)

    def rank(self, query: str, documents, top_k: int | None = None, activation=None) -> list[tuple[int, float]]:
        """(index into documents, score) by score descending; equal scores keep the input order."""
        documents = list(documents)
        scores = self.predict([(query, d) for d in documents], activation=activation)
        order = sorted(range(len(documents)), key=lambda i: (-float(scores[i]), i))
        return [(i, float(scores[i])) for i in (order if top_k is None else order[:top_k])]
