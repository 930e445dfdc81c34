"""Extractive reader on the GPU: the answer step behind the retrieval -- the span of a retrieved chunk that
answers the question, with its score and character offsets -- in the shape of the `transformers`
question-answering pipeline / Haystack's `ExtractiveReader`
(`ExtractiveReader.from_local(dir).predict(question, [chunk, ...], top_k=3)`).

The checkpoint is a LOCAL BertForQuestionAnswering directory in the Hugging Face layout (config.json,
vocab.txt, model.safetensors) of the MiniLM-L{6,12}-H384 family, e.g. a copy of deepset/minilm-uncased-squad2;
nothing is fetched.  The forward runs in libragfin_hip.so (rf_answer_spans): the sentence embedder's layers
between the cross-encoder's pair embedding kernel and a span kernel (QA head, log-sum-exps, best n_best
spans); there is no CPU path.  `span_reference` is the numpy definition of what that kernel decodes.

A context longer than the model's window is cut at its end (`only_second` truncation): sliding windows over
long contexts are out of scope -- the chunks of this corpus fit.
"""
from __future__ import annotations

import ctypes
import json
import os
from ctypes import c_void_p

import numpy as np

from . import _lib
from .embedder import MINILM_L6, Embedder, hf_encoder_config, random_weights, stack_hf_qa_head, stack_hf_state_dict
from .tokenizer import WordPieceTokenizer

MAX_QUESTION_TOKENS = 64   # the question-answering pipeline's max_question_len


def random_qa_head(hidden: int, seed: int = 0, head_scale: float = 0.05) -> dict:
    """Seeded span head (float32), a stream of its own beside random_weights(cfg, seed)."""
    rng = np.random.default_rng([seed, 2])
    return {"qa_w": (rng.standard_normal((2, hidden), dtype=np.float32) * head_scale).astype(np.float32),
            "qa_b": (rng.standard_normal(2, dtype=np.float32) * 0.02).astype(np.float32)}


def span_reference(s, e, seg: int, length: int, max_answer_len: int, n_best: int):
    """The decode rf_answer_spans performs on one pair's logits, in numpy.
    s, e: start / end logits per position (fp32; at least `length` of them); seg: index of the context's first
    token; length: tokens of the pair, the closing [SEP] last.
      context     positions lo = seg .. hi = length - 2
      candidates  (i, j), lo <= i <= j <= hi, j - i + 1 <= max_answer_len, z = fp32(s[i] + e[j])
      spans       the best n_best by (z descending, i ascending, j ascending); missing ones are (-1, -1, -inf)
      z_null      fp32(s[0] + e[0]), the [CLS] slot
      lse_start   log sum exp(s[t]) over t in {0} u [lo, hi] in fp64; lse_end the same over e
    -> (spans: list of n_best (i, j, np.float32 z), z_null: np.float32, lse_start: float, lse_end: float).
    A pair without tokens has no [CLS] slot: z_null and both log-sum-exps are -inf."""
    s, e = np.asarray(s, dtype=np.float32), np.asarray(e, dtype=np.float32)
    seg, length = int(seg), int(length)
    none = (-1, -1, np.float32(-np.inf))
    if length < 1:
        return [none] * n_best, np.float32(-np.inf), -np.inf, -np.inf
    lo, hi = max(seg, 0), length - 2
    i, w = np.meshgrid(np.arange(lo, max(hi, lo - 1) + 1), np.arange(max_answer_len), indexing="ij")
    i, j = i.ravel(), (i + w).ravel()
    keep = j <= hi
    i, j = i[keep], j[keep]
    z = (s[i] + e[j]).astype(np.float32)                 # fp32 + fp32 -> one fp32 add
    order = np.lexsort((j, i, -z.astype(np.float64)))[:n_best]
    spans = [(int(i[k]), int(j[k]), z[k]) for k in order]
    spans += [none] * (n_best - len(spans))
    members = np.array(sorted({0} | set(range(lo, hi + 1))), dtype=np.int64)

    def lse(v):
        v = v[members].astype(np.float64)
        m = v.max()
        return float(m + np.log(np.exp(v - m).sum()))
    return spans, np.float32(s[0] + e[0]), lse(s), lse(e)


class SpanBatch:
    """What span_ids returns: device tensors, all views of ONE buffer (`packed`, int32), so that a caller who
    wants the numbers on the host downloads once.
      spans   int32 [B, n_best, 2]   (start, end) token positions in the pair; (-1, -1) = none
      z       float32 [B, n_best]    s[start] + e[end]; -inf = none
      norm    float32 [B, 3]         z_null, lse_start, lse_end
      logits  float32 [B, T, 2] or None   (start, end) per position; positions >= len are 0"""
    def __init__(self, packed, B, T, n_best, want_logits):
        import torch
        self.packed, self.B, self.T, self.n_best = packed, B, T, n_best
        n_span = B * n_best * 3
        rows = packed[:n_span].view(B, n_best, 3)
        self.spans = rows[:, :, :2]
        self.z = rows[:, :, 2].view(torch.float32)
        self.norm = packed[n_span:n_span + 3 * B].view(torch.float32).view(B, 3)
        self.logits = packed[n_span + 3 * B:].view(torch.float32).view(B, T, 2) if want_logits else None

    def cpu(self) -> "SpanBatch":
        """The same views over one host copy of the buffer."""
        return SpanBatch(self.packed.cpu(), self.B, self.T, self.n_best, self.logits is not None)


class ExtractiveReader:
    """`predict(question, contexts, top_k=1) -> [{"answer", "score", "start", "end", "context_index"}, ...]`."""

    def __init__(self, weights: dict, head: dict, cfg: dict | None = None, tokenizer: WordPieceTokenizer | None = None,
                 device=None, max_length: int | None = None, max_answer_len: int = 30):
        import torch
        cfg = dict(cfg or MINILM_L6)
        # the BertModel part: the embedder's weight upload and encoder handle
        self.encoder = Embedder(weights, cfg, tokenizer, device)
        self.cfg, self.device, self.lib, self.tokenizer = cfg, self.encoder.device, self.encoder.lib, tokenizer
        self.max_length = min(max_length or cfg["max_position"], cfg["max_position"], _lib.RF_READER_MAX_T)
        if not 1 <= int(max_answer_len) <= _lib.RF_READER_MAX_SPAN:
            raise ValueError(f"max_answer_len {max_answer_len} is outside 1..{_lib.RF_READER_MAX_SPAN}")
        self.max_answer_len = int(max_answer_len)
        H = cfg["hidden"]
        shapes = {"qa_w": (2, H), "qa_b": (2,)}
        self._head = {}
        self._head_c = _lib.QaHead()
        for name, shape in shapes.items():
            a = np.ascontiguousarray(head[name], dtype=np.float32)
            if a.shape != shape:
                raise ValueError(f"head tensor {name} has shape {a.shape}, expected {shape}")
            t = torch.as_tensor(a).to(torch.float16).to(self.device).contiguous()
            self._head[name] = t   # kept alive: the library reads them in every call
            setattr(self._head_c, name, t.data_ptr())

    # -- construction -----------------------------------------------------------------
    @classmethod
    def from_local(cls, path: str, device=None, max_length: int | None = None,
                   max_answer_len: int = 30) -> "ExtractiveReader":
        """Load config.json + vocab.txt + model.safetensors of a BertForQuestionAnswering checkpoint (e.g. a copy
        of deepset/minilm-uncased-squad2) from a local directory."""
        from safetensors.numpy import load_file
        with open(os.path.join(path, "config.json")) as f:
            cfg = hf_encoder_config(json.load(f))
        sd = load_file(os.path.join(path, "model.safetensors"))
        tok = WordPieceTokenizer.from_vocab_file(os.path.join(path, "vocab.txt"))
        return cls(stack_hf_state_dict(sd, cfg), stack_hf_qa_head(sd), cfg, tok, device, max_length, max_answer_len)

    @classmethod
    def from_random(cls, cfg: dict | None = None, seed: int = 0, tokenizer=None, device=None, scale: float = 0.05,
                    head_scale: float = 0.05, max_length: int | None = None,
                    max_answer_len: int = 30) -> "ExtractiveReader":
        """Seeded random weights (random_weights(cfg, seed) + random_qa_head(hidden, seed)): both sides of a test
        can be rebuilt from the seed alone."""
        cfg = dict(cfg or MINILM_L6)
        return cls(random_weights(cfg, seed, scale), random_qa_head(cfg["hidden"], seed, head_scale), cfg, tokenizer,
                   device, max_length, max_answer_len)

    # -- forward ------------------------------------------------------------------------
    def span_ids(self, ids, lens, seg, max_answer_len: int | None = None, n_best: int = 1,
                 want_logits: bool = False) -> SpanBatch:
        """ids int32 [B, T] ([CLS] question [SEP] context [SEP], padded), lens int32 [B], seg int32 [B] (index of
        the first context token) -> SpanBatch of device tensors: the best n_best spans per pair by
        span_reference's rule, the normalisers and, with want_logits, the logits they were decoded from."""
        import torch
        ids = torch.as_tensor(ids, dtype=torch.int32)
        lens = torch.as_tensor(lens, dtype=torch.int32)
        seg = torch.as_tensor(seg, dtype=torch.int32)
        if ids.dim() != 2 or lens.shape != (ids.shape[0],) or seg.shape != lens.shape:
            raise ValueError("span_ids expects ids [B, T], lens [B] and seg [B]")
        B, T = ids.shape
        max_answer_len = self.max_answer_len if max_answer_len is None else int(max_answer_len)
        n_best = int(n_best)
        ids, lens, seg = (t.to(self.device).contiguous() for t in (ids, lens, seg))
        h = self.encoder.handle
        with torch.cuda.device(self.device):
            n_span, n_norm = B * max(n_best, 0) * 3, 3 * B
            # the library writes every span slot and normaliser, but of the logits only the positions < len
            packed = (torch.zeros if want_logits else torch.empty)(
                n_span + n_norm + (2 * B * T if want_logits else 0), dtype=torch.int32, device=self.device)
            base = packed.data_ptr()
            # per call: concurrent calls (any thread, any stream) never share scratch
            ws = torch.empty(self.lib.rf_encode_workspace_bytes(h, B, T), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.rf_answer_spans(
                h, c_void_p(ids.data_ptr()), c_void_p(lens.data_ptr()), c_void_p(seg.data_ptr()), B, T,
                ctypes.byref(self._head_c), max_answer_len, n_best, c_void_p(base), c_void_p(base + 4 * n_span),
                c_void_p(base + 4 * (n_span + n_norm)) if want_logits else None, c_void_p(ws.data_ptr()), ws.numel(),
                _lib.current_stream_ptr()))
        return SpanBatch(packed, B, T, n_best, want_logits)

    def _pairs(self, question: str, contexts: list[str]):
        """[CLS] question [SEP] context [SEP] rows: the question cut to MAX_QUESTION_TOKENS, the context to what
        is left of max_length (`only_second`).  -> (ids, lens, seg, per-context token offsets into its text)."""
        tok = self.tokenizer
        q = tok.encode(question, MAX_QUESTION_TOKENS + 2)[1:-1]
        room = self.max_length - len(q) - 3
        if room < 1:
            raise ValueError(f"max_length {self.max_length} leaves no room for a context behind {len(q)} question tokens")
        rows, offsets = [], []
        for c in contexts:
            cid, off = tok.encode_with_offsets(c, room + 2)
            rows.append([tok.cls_id] + q + [tok.sep_id] + cid[1:-1] + [tok.sep_id])
            offsets.append(off[1:-1])
        lens = np.array([len(r) for r in rows], dtype=np.int32)
        ids = np.full((len(rows), int(lens.max())), tok.pad_id, dtype=np.int32)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = r
        return ids, lens, np.full(len(rows), len(q) + 2, dtype=np.int32), offsets

    def predict(self, question: str, contexts, top_k: int = 1, max_answer_len: int | None = None,
                handle_impossible_answer: bool = False, batch_tokens: int = 65536) -> list[dict]:
        """The best top_k answer spans over all `contexts`: dicts {"answer", "score", "start", "end",
        "context_index"} with answer == contexts[context_index][start:end] (character offsets), sorted by
        (score descending, context_index, start, end ascending).
        score = exp(z - lse_start - lse_end), computed here in fp64 from the device's fp32 values: the product of
        the start and the end softmax probability over the context's tokens + [CLS], as the `transformers`
        question-answering pipeline defined it.  A context contributes its best 16 spans at most (one when
        top_k == 1); spans over the same character range of one context appear once.
        handle_impossible_answer: every context also contributes its null candidate (answer "", start = end = 0,
        score = exp(z_null - lse_start - lse_end)).
        A pair longer than max_length is cut at the end of the context; there are no sliding windows."""
        if self.tokenizer is None:
            raise RuntimeError("ExtractiveReader has no tokenizer: construct it with from_local(path) or pass "
                               "tokenizer=WordPieceTokenizer(vocab)")
        contexts = list(contexts)
        top_k = int(top_k)
        if top_k < 1:
            raise ValueError("top_k must be at least 1")
        if not contexts:
            return []
        n_best = 1 if top_k == 1 else _lib.RF_READER_MAX_BEST
        ids, lens, seg, offsets = self._pairs(question, contexts)
        # length-sorted buckets of about batch_tokens token slots, like CrossEncoder.predict
        order = np.argsort(lens, kind="stable")
        sorted_lens = lens[order].astype(np.int64)
        n, i, pending = len(contexts), 0, []
        while i < n:
            cost = np.arange(1, n - i + 1, dtype=np.int64) * sorted_lens[i:]
            j = i + max(1, int(np.searchsorted(cost, batch_tokens, side="right")))
            sel = order[i:j]
            T = int(sorted_lens[j - 1])
            pending.append((sel, self.span_ids(np.ascontiguousarray(ids[sel, :T]), lens[sel], seg[sel],
                                               max_answer_len, n_best)))
            i = j
        out = []
        for sel, batch in pending:
            host = batch.cpu()
            spans, z, norm = host.spans.numpy(), host.z.numpy(), host.norm.numpy().astype(np.float64)
            for r, ci in enumerate(sel):
                ci, seen, off = int(ci), set(), offsets[int(ci)]
                for (a, b), zz in zip(spans[r], z[r]):
                    if a < 0:
                        break
                    c0, c1 = off[a - seg[ci]][0], off[b - seg[ci]][1]
                    if (c0, c1) in seen:
                        continue
                    seen.add((c0, c1))
                    out.append({"answer": contexts[ci][c0:c1], "score": float(np.exp(np.float64(zz) - norm[r, 1] - norm[r, 2])),
                                "start": int(c0), "end": int(c1), "context_index": ci})
                if handle_impossible_answer:
                    out.append({"answer": "", "score": float(np.exp(norm[r, 0] - norm[r, 1] - norm[r, 2])),
                                "start": 0, "end": 0, "context_index": ci})
        out.sort(key=lambda d: (-d["score"], d["context_index"], d["start"], d["end"]))
        return out[:top_k]
