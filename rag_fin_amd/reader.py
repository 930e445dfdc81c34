"""Extractive reader on the GPU: the answer step behind the retrieval -- the span of a retrieved chunk that
answers the question, with its score and character offsets -- in the shape of the `transformers`
question-answering pipeline / Haystack's `ExtractiveReader`
(`ExtractiveReader.from_local(dir).predict(question, [chunk, ...], top_k=3)`).

The checkpoint is a LOCAL BertForQuestionAnswering directory in the Hugging Face layout (config.json,
vocab.txt, model.safetensors) of the MiniLM-L{6,12}-H384 family, e.g. a copy of deepset/minilm-uncased-squad2;
nothing is fetched.  The forward runs in libragfin_hip.so (rf_answer_spans): the sentence embedder's layers
between the cross-encoder's pair embedding kernel and a span kernel (QA head, log-sum-exps, best n_best
spans); there is no CPU path.  `span_reference` is the numpy definition of what that kernel decodes.

A context longer than the model's window is read in one of two modes:
  cut      (doc_stride=None, the default) the context is cut at the end of the window (`only_second`
           truncation); its tail is not seen.  The chunks of this corpus fit.
  windows  (doc_stride=<overlap in tokens>) the context is read in overlapping windows (`plan_windows`, the
           `stride=` layout of the `transformers` pipeline), all windows go through the same forward, and
           rf_stitch_spans decodes ONE ranking and ONE pair of normalisers per context from the windows' logits
           on the GPU: every token takes its logits from the window in which it has the most context.  Scores of
           spans anywhere in the context are comparable and no span appears twice -- unlike a softmax per
           window.  `stitch_reference` is the numpy definition of that decode.
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


def plan_windows(L: int, room: int, doc_stride: int) -> list[tuple[int, int]]:
    """The windows (first, count) over a context of L tokens when a pair row has room for `room` of them and
    consecutive windows share doc_stride tokens: window k is (k * step, min(room, L - k * step)) with step =
    room - doc_stride, up to the first window that reaches L (the `stride=` layout of BertTokenizerFast that the
    `transformers` question-answering pipeline uses).  L <= room -> [(0, L)]."""
    L, room, doc_stride = int(L), int(room), int(doc_stride)
    if L < 0 or room < 1 or not 0 <= doc_stride < room:
        raise ValueError(f"plan_windows needs L >= 0 and 0 <= doc_stride < room, got L={L}, room={room}, doc_stride={doc_stride}")
    step, out, first = room - doc_stride, [], 0
    while True:
        out.append((first, min(room, L - first)))
        if first + room >= L:
            return out
        first += step


def window_owners(windows) -> np.ndarray:
    """int64 [L]: the window that owns each context token, L = max(first + count).  The owner of token t is the
    window w holding t with the largest min(t - first_w, first_w + count_w - 1 - t) -- BERT's "max context" --
    and among equals the smallest w; -1 where no window holds t.  windows: rows (first, count, ...)."""
    win = [(int(r[0]), int(r[1])) for r in windows]
    L = max((f + n for f, n in win), default=0)
    owner, best = np.full(L, -1, dtype=np.int64), np.full(L, -1, dtype=np.int64)
    for w, (f, n) in enumerate(win):
        t = np.arange(f, f + n)
        margin = np.minimum(t - f, f + n - 1 - t)
        better = margin > best[f:f + n]                      # strictly: an earlier window keeps a tie
        owner[f:f + n][better] = w
        best[f:f + n][better] = margin[better]
    return owner


def stitch_reference(logits, windows, max_answer_len: int, n_best: int):
    """The decode rf_stitch_spans performs on ONE context's windows, in numpy.
    logits: fp32 [W, T, 2] (start, end per position of each window's pair row); windows: W rows (first, count,
    seg) in ascending first -- context tokens first .. first + count - 1 sit at positions seg .. of the row.
      L           max(first + count)
      S[t], E[t]  the logits of token t in its owner (window_owners), copied
      null slot   the window with the smallest fp32(s_w[0] + e_w[0]), the first of equals; z_null is that sum
      candidates  (i, j), 0 <= i <= j < L, j - i + 1 <= max_answer_len, z = fp32(S[i] + E[j])
      spans       the best n_best by (z descending, i ascending, j ascending), context-token indices; missing
                  ones are (-1, -1, -inf)
      lse_start   log sum exp over the null slot's s[0] and S[0 .. L) in fp64; lse_end the same over e and E
    -> (spans: list of n_best (i, j, np.float32 z), z_null: np.float32, lse_start: float, lse_end: float).
    No windows: no null slot either, z_null and both log-sum-exps are -inf."""
    logits = np.asarray(logits, dtype=np.float32)
    win = [(int(r[0]), int(r[1]), int(r[2])) for r in windows]
    none = (-1, -1, np.float32(-np.inf))
    if not win:
        return [none] * n_best, np.float32(-np.inf), -np.inf, -np.inf
    owner = window_owners(win)
    L = len(owner)
    if (owner < 0).any():
        raise ValueError("the windows do not cover the context")
    first, seg = (np.array([w[k] for w in win], dtype=np.int64) for k in (0, 2))
    pos = seg[owner] + np.arange(L) - first[owner]
    S, E = logits[owner, pos, 0], logits[owner, pos, 1]
    z0 = (logits[:len(win), 0, 0] + logits[:len(win), 0, 1]).astype(np.float32)
    null = int(np.argmin(z0))                                # (the first of equal minima)
    i, w = np.meshgrid(np.arange(L), np.arange(max_answer_len), indexing="ij")
    i, j = i.ravel(), (i + w).ravel()
    keep = j < L
    i, j = i[keep], j[keep]
    z = (S[i] + E[j]).astype(np.float32)                     # fp32 + fp32 -> one fp32 add
    if len(z) > n_best:                                      # (nothing below the n_best-th largest z can be returned)
        keep = z >= np.partition(z, len(z) - n_best)[len(z) - n_best]
        i, j, z = i[keep], j[keep], z[keep]
    order = np.lexsort((j, i, -z.astype(np.float64)))[:n_best]
    spans = [(int(i[k]), int(j[k]), z[k]) for k in order]
    spans += [none] * (n_best - len(spans))

    def lse(v0, v):
        v = np.concatenate([[v0], v]).astype(np.float64)
        m = v.max()
        return float(m + np.log(np.exp(v - m).sum()))
    return spans, z0[null], lse(logits[null, 0, 0], S), lse(logits[null, 0, 1], E)


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


class StitchBatch:
    """What stitch_ids / stitch_logits return: device tensors over ONE buffer (`packed`, int32) whose head -- the
    spans and the normalisers -- is what cpu() downloads.
      spans   int32 [C, n_best, 2]   (start, end) CONTEXT-token indices; (-1, -1) = none
      z       float32 [C, n_best]    S[start] + E[end]; -inf = none
      norm    float32 [C, 3]         z_null, lse_start, lse_end
      logits  float32 [W, T, 2]      the windows' logits the decode read (stitch_ids: the tail of `packed`)"""
    def __init__(self, packed, C, n_best, logits=None):
        import torch
        self.packed, self.C, self.n_best, self.logits = packed, C, n_best, logits
        n_span = C * n_best * 3
        rows = packed[:n_span].view(C, n_best, 3)
        self.spans = rows[:, :, :2]
        self.z = rows[:, :, 2].view(torch.float32)
        self.norm = packed[n_span:n_span + 3 * C].view(torch.float32).view(C, 3)

    def cpu(self) -> "StitchBatch":
        """The same views over one host copy of the spans and normalisers (the logits stay on the device)."""
        return StitchBatch(self.packed[:self.C * (self.n_best + 1) * 3].cpu(), self.C, self.n_best)


_INSTANCE = object()   # predict(doc_stride=...): "the instance's"


class ExtractiveReader:
    """`predict(question, contexts, top_k=1) -> [{"answer", "score", "start", "end", "context_index"}, ...]`.
    doc_stride: None cuts a context that does not fit the window; an int reads it in windows that overlap by
    that many tokens and decodes them as one context (the module docstring's two modes)."""

    def __init__(self, weights: dict, head: dict, cfg: dict | None = None, tokenizer: WordPieceTokenizer | None = None,
                 device=None, max_length: int | None = None, max_answer_len: int = 30, doc_stride: int | None = None):
        import torch
        cfg = dict(cfg or MINILM_L6)
        # the BertModel part: the embedder's weight upload and encoder handle
        self.encoder = Embedder(weights, cfg, tokenizer, device)
        self.cfg, self.device, self.lib, self.tokenizer = cfg, self.encoder.device, self.encoder.lib, tokenizer
        self.max_length = min(max_length or cfg["max_position"], cfg["max_position"], _lib.RF_READER_MAX_T)
        if not 1 <= int(max_answer_len) <= _lib.RF_READER_MAX_SPAN:
            raise ValueError(f"max_answer_len {max_answer_len} is outside 1..{_lib.RF_READER_MAX_SPAN}")
        self.max_answer_len = int(max_answer_len)
        if doc_stride is not None and int(doc_stride) < 0:
            raise ValueError(f"doc_stride {doc_stride} is negative")
        self.doc_stride = None if doc_stride is None else int(doc_stride)
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
                   max_answer_len: int = 30, doc_stride: int | None = None) -> "ExtractiveReader":
        """Load config.json + vocab.txt + model.safetensors of a BertForQuestionAnswering checkpoint (e.g. a copy
        of deepset/minilm-uncased-squad2) from a local directory."""
        from safetensors.numpy import load_file
        with open(os.path.join(path, "config.json")) as f:
            cfg = hf_encoder_config(json.load(f))
        sd = load_file(os.path.join(path, "model.safetensors"))
        tok = WordPieceTokenizer.from_vocab_file(os.path.join(path, "vocab.txt"))
        return cls(stack_hf_state_dict(sd, cfg), stack_hf_qa_head(sd), cfg, tok, device, max_length, max_answer_len,
                   doc_stride)

    @classmethod
    def from_random(cls, cfg: dict | None = None, seed: int = 0, tokenizer=None, device=None, scale: float = 0.05,
                    head_scale: float = 0.05, max_length: int | None = None,
                    max_answer_len: int = 30, doc_stride: int | None = None) -> "ExtractiveReader":
        """Seeded random weights (random_weights(cfg, seed) + random_qa_head(hidden, seed)): both sides of a test
        can be rebuilt from the seed alone."""
        cfg = dict(cfg or MINILM_L6)
        return cls(random_weights(cfg, seed, scale), random_qa_head(cfg["hidden"], seed, head_scale), cfg, tokenizer,
                   device, max_length, max_answer_len, doc_stride)

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

    def stitch_logits(self, logits, windows, ctx_win, max_answer_len: int | None = None, n_best: int = 1,
                      _packed=None) -> StitchBatch:
        """rf_stitch_spans on windows' logits that are already there: logits float32 [W, T, 2] as span_ids(...,
        want_logits=True) writes them, windows int32 [W, 3] (first, count, seg) and ctx_win int32 [C + 1], the rows
        ctx_win[c] .. ctx_win[c + 1] being context c's windows in ascending first -> StitchBatch: per context what
        stitch_reference defines."""
        import torch
        logits = torch.as_tensor(logits, dtype=torch.float32)
        windows = np.ascontiguousarray(windows, dtype=np.int32)
        windows = windows.reshape(len(windows), -1) if windows.size else np.zeros((0, 3), dtype=np.int32)
        ctx_win = torch.as_tensor(ctx_win, dtype=torch.int32)
        if (logits.dim() != 3 or logits.shape[2] != 2 or windows.shape[0] != logits.shape[0] or windows.shape[1] < 3
                or ctx_win.dim() != 1):
            raise ValueError("stitch_logits expects logits [W, T, 2], windows [W, 3] and ctx_win [C + 1]")
        W, T, C = logits.shape[0], logits.shape[1], ctx_win.shape[0] - 1
        max_answer_len = self.max_answer_len if max_answer_len is None else int(max_answer_len)
        n_best = int(n_best)
        longest = int((windows[:, 0].astype(np.int64) + windows[:, 1]).max()) if W else 0
        if longest > _lib.RF_READER_MAX_CONTEXT:
            raise ValueError(f"a context of {longest} tokens exceeds RF_READER_MAX_CONTEXT = {_lib.RF_READER_MAX_CONTEXT}")
        win = np.zeros((W, 4), dtype=np.int32)                # rf_window rows: first, count, seg, pad
        win[:, :3] = windows[:, :3]
        logits, win, ctx_win = (t.to(self.device).contiguous() for t in (logits, torch.from_numpy(win), ctx_win))
        with torch.cuda.device(self.device):
            n_head = max(C, 0) * (max(n_best, 0) + 1) * 3
            packed = torch.empty(n_head, dtype=torch.int32, device=self.device) if _packed is None else _packed
            base = packed.data_ptr()
            # per call, like span_ids' workspace
            ws = torch.empty(max(self.lib.rf_stitch_workspace_bytes(W, max(C, 1), max(longest, 0)), 256),
                             dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.rf_stitch_spans(
                c_void_p(logits.data_ptr()), W, T, c_void_p(win.data_ptr()), c_void_p(ctx_win.data_ptr()), C,
                max_answer_len, n_best, c_void_p(base), c_void_p(base + 4 * max(C, 0) * max(n_best, 0) * 3),
                c_void_p(ws.data_ptr()), ws.numel(), _lib.current_stream_ptr()))
        return StitchBatch(packed, C, n_best, logits)

    def window_logits(self, ids, lens, seg, batch_tokens: int = 65536, out=None):
        """The forward of W pair rows (ids int32 [W, T], on the host or the device; lens, seg int32 [W], host) in
        length-sorted buckets of about batch_tokens token slots, like predict's.  -> float32 [W, T, 2] on the
        device (`out`, when given: a zeroed buffer of that shape), row w the logits of row w whatever its bucket;
        positions >= lens stay 0.  No host round trip."""
        import torch
        ids = torch.as_tensor(ids, dtype=torch.int32)
        lens, seg = np.ascontiguousarray(lens, dtype=np.int32), np.ascontiguousarray(seg, dtype=np.int32)
        if ids.dim() != 2 or lens.shape != (ids.shape[0],) or seg.shape != lens.shape:
            raise ValueError("window_logits expects ids [W, T], lens [W] and seg [W]")
        W, T = ids.shape
        # (the library writes only the positions < len of a row)
        logits = torch.zeros((W, T, 2), dtype=torch.float32, device=self.device) if out is None else out
        order = np.argsort(lens, kind="stable")
        sorted_lens = lens[order].astype(np.int64)
        i = 0
        while i < W:
            cost = np.arange(1, W - i + 1, dtype=np.int64) * sorted_lens[i:]
            j = i + max(1, int(np.searchsorted(cost, batch_tokens, side="right")))
            sel = order[i:j]
            Tb = max(int(sorted_lens[j - 1]), 1)
            rows = torch.as_tensor(sel, dtype=torch.int64)
            # the forward alone is wanted: the bucket's own decode is asked for as little as it can give
            part = self.span_ids(ids[rows.to(ids.device), :Tb], lens[sel], seg[sel], 1, 1, want_logits=True)
            logits[:, :Tb].index_copy_(0, rows.to(self.device), part.logits)
            i = j
        return logits

    def stitch_ids(self, ids, lens, windows, ctx_win, max_answer_len: int | None = None, n_best: int = 1,
                   batch_tokens: int = 65536) -> StitchBatch:
        """ids int32 [W, T] and lens int32 [W]: the windows' pair rows ([CLS] question [SEP] window [SEP], padded);
        windows int32 [W, 3] (first, count, seg) and ctx_win int32 [C + 1] as stitch_logits takes them.  The rows
        go through window_logits, their logits into one device buffer [W, T, 2] (the tail of the returned
        `packed`), and one rf_stitch_spans call decodes them -> StitchBatch of device tensors."""
        import torch
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        windows = np.ascontiguousarray(windows, dtype=np.int32).reshape(len(lens), -1 if len(lens) else 3)
        ctx_win = np.ascontiguousarray(ctx_win, dtype=np.int32)
        if len(ids.shape) != 2 or windows.shape[1] < 3 or ctx_win.ndim != 1:
            raise ValueError("stitch_ids expects ids [W, T], lens [W], windows [W, 3] and ctx_win [C + 1]")
        (W, T), C, n_best = ids.shape, len(ctx_win) - 1, int(n_best)
        n_head = max(C, 0) * (max(n_best, 0) + 1) * 3
        packed = torch.zeros(n_head + 2 * W * T, dtype=torch.int32, device=self.device)
        logits = self.window_logits(ids, lens, windows[:, 2], batch_tokens,
                                    out=packed[n_head:].view(torch.float32).view(W, T, 2))
        return self.stitch_logits(logits, windows, ctx_win, max_answer_len, n_best, _packed=packed)

    def _question(self, question: str):
        """-> (the question's tokens, cut to MAX_QUESTION_TOKENS; the context tokens a pair row has room for)."""
        q = self.tokenizer.encode(question, MAX_QUESTION_TOKENS + 2)[1:-1]
        room = self.max_length - len(q) - 3
        if room < 1:
            raise ValueError(f"max_length {self.max_length} leaves no room for a context behind {len(q)} question tokens")
        return q, room

    def _windows(self, question: str, contexts: list[str], doc_stride: int):
        """Every context tokenised once with offsets and cut by plan_windows into [CLS] question [SEP] window [SEP]
        rows.  -> (ids, lens, windows [W, 3], ctx_win [C + 1], per-context token offsets into its text)."""
        tok = self.tokenizer
        q, room = self._question(question)
        limit = _lib.RF_READER_MAX_CONTEXT
        rows, windows, ctx_win, offsets = [], [], [0], []
        for c in contexts:
            cid, off = tok.encode_with_offsets(c, limit + 3)      # (one token beyond the limit shows that it is passed)
            cid, off = cid[1:-1], off[1:-1]
            if len(cid) > limit:
                raise ValueError(f"a context has more than {limit} tokens (RF_READER_MAX_CONTEXT), the most one "
                                 "stitched context holds")
            for first, count in plan_windows(len(cid), room, doc_stride):
                rows.append([tok.cls_id] + q + [tok.sep_id] + cid[first:first + count] + [tok.sep_id])
                windows.append((first, count, len(q) + 2))
            ctx_win.append(len(rows))
            offsets.append(off)
        lens = np.array([len(r) for r in rows], dtype=np.int32)
        ids = np.full((len(rows), int(lens.max())), tok.pad_id, dtype=np.int32)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = r
        return ids, lens, np.array(windows, dtype=np.int32), np.array(ctx_win, dtype=np.int32), offsets

    def _pairs(self, question: str, contexts: list[str]):
        """[CLS] question [SEP] context [SEP] rows: the question cut to MAX_QUESTION_TOKENS, the context to what
        is left of max_length (`only_second`).  -> (ids, lens, seg, per-context token offsets into its text)."""
        tok = self.tokenizer
        q, room = self._question(question)
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
                handle_impossible_answer: bool = False, batch_tokens: int = 65536, doc_stride=_INSTANCE) -> list[dict]:
        """The best top_k answer spans over all `contexts`: dicts {"answer", "score", "start", "end",
        "context_index"} with answer == contexts[context_index][start:end] (character offsets), sorted by
        (score descending, context_index, start, end ascending).
        score = exp(z - lse_start - lse_end), computed here in fp64 from the device's fp32 values: the product of
        the start and the end softmax probability over the context's tokens + [CLS], as the `transformers`
        question-answering pipeline defined it.  A context contributes its best 16 spans at most (one when
        top_k == 1); spans over the same character range of one context appear once.
        handle_impossible_answer: every context also contributes its null candidate (answer "", start = end = 0,
        score = exp(z_null - lse_start - lse_end)).
        doc_stride (default: the instance's): None -- a pair longer than max_length is cut at the end of the
        context, whose tail is not seen; an int -- every context (up to RF_READER_MAX_CONTEXT tokens, a longer one
        raises ValueError) is read in windows that overlap by doc_stride tokens (plan_windows) and decoded as ONE
        context by rf_stitch_spans: one ranking, one null candidate and one pair of normalisers per context, so
        that the scores of spans anywhere in it, seams included, are comparable (stitch_reference)."""
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
        doc_stride = self.doc_stride if doc_stride is _INSTANCE else doc_stride
        if doc_stride is not None:
            ids, lens, windows, ctx_win, offsets = self._windows(question, contexts, int(doc_stride))
            batch = self.stitch_ids(ids, lens, windows, ctx_win, max_answer_len, n_best, batch_tokens)
            # spans are context-token indices: no shift
            return self._hits(contexts, offsets, np.zeros(len(contexts), dtype=np.int32),
                              [(np.arange(len(contexts)), batch)], handle_impossible_answer, top_k)
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
        return self._hits(contexts, offsets, seg, pending, handle_impossible_answer, top_k)

    @staticmethod
    def _hits(contexts, offsets, seg, pending, handle_impossible_answer: bool, top_k: int) -> list[dict]:
        """One download per batch of `pending` [(context indices, SpanBatch / StitchBatch)] -> predict's list.
        seg[ci]: the position of context ci's first token in what its spans index."""
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
