"""Late interaction (ColBERT) on the GPU, with the surface of PyLate's `models.ColBERT`
(`ColBERT(dir).encode([...], is_query=True | False)` -> one [n_tok, D] matrix of unit vectors per text): a query and
a document are bags of token vectors, and the score of a pair is MaxSim,
    score(q, d) = sum over the query's tokens i of max over the document's tokens j of (q_i . d_j)
-- a Milvus embedding list with metric MAX_SIM_IP, a Vespa / Qdrant multivector.

The checkpoint is a LOCAL directory of the MiniLM / BERT H384 family (config.json, vocab.txt, model.safetensors;
nothing is fetched) in one of two layouts: Stanford / HF_ColBERT (`bert.*` plus `linear.weight` in
model.safetensors) or PyLate (a BertModel in model.safetensors plus `1_Dense/model.safetensors` holding
`linear.weight`).  The forward runs in libragfin_hip.so (rf_encode_tokens: the sentence embedder's layers, then
the projection, the norm and the skiplist), scoring and selection too (rf_maxsim, rf_maxsim_topk); there is no CPU
path.

The numpy definitions the tests compare against live here too: tokens_reference, maxsim_reference,
topk_reference.
"""
from __future__ import annotations

import ctypes
import json
import os
import string
from ctypes import c_void_p

import numpy as np

from . import _lib

QTOK = _lib.RF_MAXSIM_QTOK
DEFAULT_SKIPLIST = list(string.punctuation)      # PyLate's default skiplist_words
SCORES_BYTES_MAX = 256 << 20                     # one [B, n_rows] scores buffer of an all-rows search, at most
DEFAULTS = {"query_length": 32, "document_length": 180, "query_marker": "[unused0]", "document_marker": "[unused1]",
            "skiplist_words": DEFAULT_SKIPLIST, "attend_to_expansion_tokens": None}


# ---- checkpoints ------------------------------------------------------------------------------------------------------
def read_settings(path: str) -> dict:
    """The settings a checkpoint directory states, over DEFAULTS, for the keys that are present:
    config_sentence_transformers.json (PyLate: query_length, document_length, query_prefix, document_prefix,
    skiplist_words, attend_to_expansion_tokens) or artifact.metadata (Stanford: query_maxlen, doc_maxlen,
    query_token_id, doc_token_id, mask_punctuation, attend_to_mask_tokens).  attend_to_expansion_tokens stays
    None when the checkpoint does not say."""
    s = dict(DEFAULTS)
    p = os.path.join(path, "config_sentence_transformers.json")
    if os.path.exists(p):
        with open(p) as f:
            m = json.load(f)
        for src, dst in (("query_length", "query_length"), ("document_length", "document_length"),
                         ("skiplist_words", "skiplist_words"), ("attend_to_expansion_tokens", "attend_to_expansion_tokens")):
            if m.get(src) is not None:
                s[dst] = m[src]
        for src, dst in (("query_prefix", "query_marker"), ("document_prefix", "document_marker")):
            if m.get(src):
                s[dst] = str(m[src]).strip()
    p = os.path.join(path, "artifact.metadata")
    if os.path.exists(p):
        with open(p) as f:
            m = json.load(f)
        for src, dst in (("query_maxlen", "query_length"), ("doc_maxlen", "document_length"),
                         ("query_token_id", "query_marker"), ("doc_token_id", "document_marker"),
                         ("attend_to_mask_tokens", "attend_to_expansion_tokens")):
            if m.get(src) is not None:
                s[dst] = m[src]
        if m.get("mask_punctuation") is False:
            s["skiplist_words"] = []
    return s


def load_checkpoint(path: str):
    """-> (state dict of the BertModel part, projection [D, H] float32) of either layout."""
    from safetensors.numpy import load_file
    sd = load_file(os.path.join(path, "model.safetensors"))
    dense = os.path.join(path, "1_Dense", "model.safetensors")
    if "linear.weight" in sd:                                  # Stanford / HF_ColBERT
        proj = sd["linear.weight"]
    elif os.path.exists(dense):                                # PyLate
        proj = load_file(dense)["linear.weight"]
    else:
        raise KeyError("checkpoint lacks linear.weight (model.safetensors) and 1_Dense/model.safetensors: "
                       "not a ColBERT checkpoint")
    return sd, np.asarray(proj, dtype=np.float32)


def random_projection(cfg: dict, seed: int = 0, dim: int = 96) -> np.ndarray:
    """Seeded projection [dim, H] float32, a stream of its own beside random_weights(cfg, seed)."""
    rng = np.random.default_rng([seed, 3])
    return (rng.standard_normal((dim, cfg["hidden"]), dtype=np.float32) * 0.05).astype(np.float32)


# ---- row layout -------------------------------------------------------------------------------------------------------
def marker_id(vocab: dict, marker, fallback: str) -> int:
    """A marker given as a token ("[unused0]", "[Q]") or an id -> its id; a token the vocabulary lacks falls back
    to `fallback`."""
    if isinstance(marker, (int, np.integer)) and not isinstance(marker, bool):
        return int(marker)
    tok = str(marker).strip()
    if tok in vocab:
        return int(vocab[tok])
    if fallback in vocab:
        return int(vocab[fallback])
    raise ValueError(f"the vocabulary has neither the marker {tok!r} nor {fallback!r}")


def skip_bitmap(vocab: dict, words, vocab_size: int) -> np.ndarray:
    """The skiplist as rf_token_head.skip: uint32 [ceil(vocab_size / 32)], bit id set for every word of `words`
    that is a token of the vocabulary."""
    bits = np.zeros((vocab_size + 31) // 32, dtype=np.uint32)
    for w in words:
        i = vocab.get(w)
        if i is not None and 0 <= i < vocab_size:
            bits[i >> 5] |= np.uint32(1 << (i & 31))
    return bits


def build_rows(tokenizer, texts, is_query: bool, *, query_length: int = 32, document_length: int = 180,
               query_marker="[unused0]", document_marker="[unused1]", query_expansion: bool = True):
    """-> (ids int32 [n, T], lens int32 [n]).  Queries: [CLS] [Q] query [SEP], cut to min(query_length, 32)
    tokens; with query_expansion filled to that length with [MASK] tokens that count as tokens of the row.
    Documents: [CLS] [D] text [SEP], cut to document_length."""
    vocab = tokenizer.vocab
    if is_query:
        width = min(int(query_length), QTOK)
        mark = marker_id(vocab, query_marker, "[unused0]")
    else:
        width = int(document_length)
        mark = marker_id(vocab, document_marker, "[unused1]")
    if width < 3:
        raise ValueError(f"a row needs at least [CLS], its marker and [SEP]: length {width}")
    rows = []
    for t in texts:
        r = tokenizer.encode(t, width - 1)                     # [CLS] .. [SEP], at most width - 1 ids
        rows.append([r[0], mark] + r[1:])
    fill = tokenizer.pad_id
    if is_query and query_expansion:
        if "[MASK]" not in vocab:
            raise ValueError("query expansion needs a [MASK] token in the vocabulary")
        fill = int(vocab["[MASK]"])
    T = width if (is_query and query_expansion) else max((len(r) for r in rows), default=1)
    ids = np.full((len(rows), T), fill, dtype=np.int32)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
    lens = np.full(len(rows), T, dtype=np.int32) if (is_query and query_expansion) else \
        np.asarray([len(r) for r in rows], dtype=np.int32)
    return ids, lens


# ---- the definitions (numpy, host) -----------------------------------------------------------------------------------
def tokens_reference(w16: dict, proj16, cfg: dict, ids, lens, skip=None, dtype=np.float64, hidden=None) -> list:
    """The definition of rf_encode_tokens in fp64 -> one [n_kept, D] array per row: normalize(proj x_t) of the
    tokens t < lens[b] whose id is not in `skip` (a uint32 bitmap as skip_bitmap gives, or None), in token
    order.  hidden: the last hidden state, when the caller has it already."""
    from .sparse_encoder import hidden_reference
    ids, lens = np.asarray(ids), np.asarray(lens)
    x = hidden_reference(w16, cfg, ids, lens, dtype) if hidden is None else np.asarray(hidden, dtype=dtype)
    proj = np.asarray(proj16).astype(dtype)
    out = []
    for b in range(ids.shape[0]):
        n = int(min(max(lens[b], 0), ids.shape[1]))
        keep = np.ones(n, dtype=bool)
        if skip is not None:
            t = np.clip(ids[b, :n], 0, cfg["vocab_size"] - 1)
            keep = ((np.asarray(skip)[t >> 5] >> (t & 31).astype(np.uint32)) & 1) == 0
        v = x[b, :n][keep] @ proj.T
        out.append(v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-12))
    return out


def maxsim_reference(docs, queries, mask=None) -> np.ndarray:
    """The definition of rf_maxsim in fp64 -> [B, n_rows]: docs and queries are lists of [n_tok, D] arrays (a
    query's rows are its q_len tokens).  A row or a query without tokens, and a row with mask[r] false, score
    -inf."""
    out = np.full((len(queries), len(docs)), -np.inf, dtype=np.float64)
    for b, q in enumerate(queries):
        q = np.asarray(q, dtype=np.float64)
        if q.shape[0] == 0:
            continue
        for r, d in enumerate(docs):
            d = np.asarray(d, dtype=np.float64)
            if d.shape[0] == 0 or (mask is not None and not mask[r]):
                continue
            out[b, r] = (q @ d.T).max(axis=1).sum()
    return out


def _order_keys(scores) -> np.ndarray:
    """float32 bit patterns folded so that they order as the floats do (-0.0 below +0.0), as the kernel's keys."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def topk_reference(scores, k: int, rows=None, id_base: int = 0):
    """The definition of rf_maxsim_topk for one batch of equal-length segments: scores [B, n] (or [n]) ->
    (scores fp32 [B, k], ids int64 [B, k]) padded with -inf / -1: the best k by (score descending, position
    ascending); -inf and NaN are no hits; the id is rows[b][position] or id_base + position."""
    s = np.atleast_2d(np.asarray(scores, dtype=np.float32))
    B = s.shape[0]
    out_s = np.full((B, k), -np.inf, dtype=np.float32)
    out_i = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        hit = np.flatnonzero(s[b] > -np.inf)
        order = hit[np.lexsort((hit, -_order_keys(s[b][hit])))][:k]
        out_s[b, :order.size] = s[b][order]
        out_i[b, :order.size] = (np.asarray(rows[b])[order] if rows is not None else id_base + order)
    return out_s, out_i


def pack_queries(queries, dim: int):
    """A list of [n_tok <= 32, dim] arrays -> (q_vec float16 [B, 32, dim], q_len int32 [B]); slots past a
    query's tokens are zero and never read."""
    q_vec = np.zeros((len(queries), QTOK, dim), dtype=np.float16)
    q_len = np.zeros(len(queries), dtype=np.int32)
    for b, q in enumerate(queries):
        q = np.asarray(q)
        if q.ndim != 2 or q.shape[1] != dim:
            raise ValueError(f"query {b}: token vectors have shape {q.shape}, expected [n_tok, {dim}]")
        if q.shape[0] > QTOK:
            raise ValueError(f"query {b} has {q.shape[0]} token vectors, more than {QTOK}")
        q_vec[b, :q.shape[0]] = q.astype(np.float16)
        q_len[b] = q.shape[0]
    return q_vec, q_len


# ---- thin wrappers over the library --------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else c_void_p(t.data_ptr())


class TokenField:
    """The token vectors of the rows of a collection on the device: vec float16 [capacity, dim], off int64
    [row capacity + 1] (CSR over the rows); both grown by doubling.  `off_host` mirrors the offsets."""

    def __init__(self, dim: int, device):
        import torch
        if dim % 16 or not 16 <= dim <= _lib.RF_MAXSIM_DIM:
            raise ValueError(f"token vectors of {dim} features: need a multiple of 16 in 16..{_lib.RF_MAXSIM_DIM}")
        self.dim, self.device = int(dim), torch.device(device)
        self.lib = _lib.load_library()
        self.off_host = np.zeros(1, dtype=np.int64)
        self.vec = torch.empty((1024, self.dim), dtype=torch.float16, device=self.device)
        self.off = torch.zeros(257, dtype=torch.int64, device=self.device)

    @classmethod
    def from_rows(cls, rows, dim: int, device) -> "TokenField":
        f = cls(dim, device)
        f.append(rows)
        return f

    @property
    def n_rows(self) -> int:
        return int(self.off_host.size - 1)

    @property
    def n_tok(self) -> int:
        return int(self.off_host[-1])

    def append(self, rows) -> None:
        """rows: a list of [n_tok, dim] float16 arrays (host), one per new row."""
        import torch
        rows = [np.ascontiguousarray(r, dtype=np.float16).reshape(-1, self.dim) for r in rows]
        if not rows:
            return
        counts = np.asarray([r.shape[0] for r in rows], dtype=np.int64)
        new_off = self.off_host[-1] + np.cumsum(counts)
        n_tok, n_rows = int(new_off[-1]), self.n_rows + len(rows)
        if n_tok > self.vec.shape[0]:
            cap = self.vec.shape[0]
            while cap < n_tok:
                cap *= 2
            grown = torch.empty((cap, self.dim), dtype=torch.float16, device=self.device)
            grown[:self.n_tok] = self.vec[:self.n_tok]
            self.vec = grown
        if n_rows + 1 > self.off.numel():
            cap = self.off.numel() - 1
            while cap < n_rows:
                cap *= 2
            grown = torch.zeros(cap + 1, dtype=torch.int64, device=self.device)
            grown[:self.n_rows + 1] = self.off[:self.n_rows + 1]
            self.off = grown
        if n_tok > self.n_tok:
            self.vec[self.n_tok:n_tok] = torch.from_numpy(np.concatenate(rows)).to(self.device)
        self.off[self.n_rows + 1:n_rows + 1] = torch.from_numpy(new_off).to(self.device)
        self.off_host = np.concatenate([self.off_host, new_off])

    def keep(self, mask) -> None:
        """Drop the rows whose mask entry is false (a mask longer than the field covers rows not encoded yet)."""
        import torch
        keep = np.asarray(mask[:self.n_rows], dtype=bool)
        counts = np.diff(self.off_host)
        tok_keep = np.repeat(keep, counts)
        kept = self.vec[:self.n_tok][torch.from_numpy(tok_keep).to(self.device)]
        new_off = np.zeros(int(keep.sum()) + 1, dtype=np.int64)
        np.cumsum(counts[keep], out=new_off[1:])
        self.vec[:kept.shape[0]] = kept
        self.off[:new_off.size] = torch.from_numpy(new_off).to(self.device)
        self.off_host = new_off

    def vectors(self, rows) -> list:
        """The stored float16 vectors of the given rows, one [n_tok, dim] host array each."""
        out = []
        for r in rows:
            r = int(r)
            if not 0 <= r < self.n_rows:
                raise IndexError(f"row {r} outside [0, {self.n_rows})")
            out.append(self.vec[int(self.off_host[r]):int(self.off_host[r + 1])].cpu().numpy())
        return out

    def struct(self) -> "_lib.TokenField":
        return _lib.TokenField(self.vec.data_ptr(), self.off.data_ptr(), self.n_rows, self.dim)

    # -- search -----------------------------------------------------------------------------------
    def search(self, queries, k: int, filt=None):
        """All-rows MaxSim + the exact top-k -> (scores f32 [B, k], rows i64 [B, k]) device tensors padded with
        -inf / -1.  The queries of a call go in chunks whose [chunk, n_rows] scores stay under 256 MB."""
        import torch
        q_vec, q_len = _device_queries(queries, self.dim, self.device)
        B, n = q_vec.shape[0], self.n_rows
        out_s = torch.full((B, k), float("-inf"), dtype=torch.float32, device=self.device)
        out_i = torch.full((B, k), -1, dtype=torch.int64, device=self.device)
        if B == 0 or n == 0:
            return out_s, out_i
        chunk = max(1, min(B, SCORES_BYTES_MAX // (4 * n)))
        for b0 in range(0, B, chunk):
            nb = min(chunk, B - b0)
            scores = maxsim(self, (q_vec[b0:b0 + nb], q_len[b0:b0 + nb]), filter=filt)
            seg = torch.arange(nb + 1, dtype=torch.int64, device=self.device) * n
            s, i = maxsim_topk(scores, seg, k)
            out_s[b0:b0 + nb], out_i[b0:b0 + nb] = s, i
        return out_s, out_i


def _device_queries(queries, dim: int, device):
    """Queries as a list of [n_tok, dim] arrays, or already packed (q_vec [B, 32, dim], q_len [B]) -> device
    tensors (float16, int32)."""
    import torch
    if isinstance(queries, tuple) and len(queries) == 2 and hasattr(queries[0], "shape") and len(queries[0].shape) == 3:
        q_vec, q_len = queries
    else:
        q_vec, q_len = pack_queries(list(queries), dim)
    q_vec = torch.as_tensor(q_vec).to(device=device, dtype=torch.float16).contiguous()
    q_len = torch.as_tensor(q_len).to(device=device, dtype=torch.int32).contiguous()
    if q_vec.dim() != 3 or q_vec.shape[1:] != (QTOK, dim) or q_len.shape != (q_vec.shape[0],):
        raise ValueError(f"packed queries: need q_vec [B, {QTOK}, {dim}] and q_len [B]")
    return q_vec, q_len


def maxsim(field: TokenField, queries, candidates=None, filter=None):
    """rf_maxsim on the current stream; no host sync.  queries: a list of [n_tok <= 32, D] arrays or packed
    (q_vec, q_len).  candidates None: every query against every row -> scores f32 [B, n_rows] on the device.
    candidates a list of row lists (one per query) or (cand_off int64 [B + 1], cand_row int64) -> scores f32
    parallel to cand_row.  filter: a filter buffer built for the field's rows.  -inf = not a hit."""
    import torch
    q_vec, q_len = _device_queries(queries, field.dim, field.device)
    B = q_vec.shape[0]
    cand_off = cand_row = None
    if candidates is not None:
        if isinstance(candidates, tuple) and len(candidates) == 2 and hasattr(candidates[0], "shape"):
            cand_off, cand_row = candidates
        else:
            if len(candidates) != B:
                raise ValueError(f"{len(candidates)} candidate lists for {B} queries")
            cand_off = np.zeros(B + 1, dtype=np.int64)
            np.cumsum([len(c) for c in candidates], out=cand_off[1:])
            cand_row = np.concatenate([np.asarray(c, dtype=np.int64).reshape(-1) for c in candidates]) \
                if B else np.zeros(0, np.int64)
        cand_off = torch.as_tensor(cand_off).to(device=field.device, dtype=torch.int64).contiguous()
        # (an empty list of rows still needs a pointer: one spare entry)
        cand_row = torch.cat([torch.as_tensor(cand_row).to(device=field.device, dtype=torch.int64),
                              torch.zeros(1, dtype=torch.int64, device=field.device)])
        n_out = cand_row.numel() - 1
        scores = torch.empty(n_out + 1, dtype=torch.float32, device=field.device)
    else:
        scores = torch.empty((B, field.n_rows), dtype=torch.float32, device=field.device)
    if B == 0:
        return scores if candidates is None else scores[:0]
    with torch.cuda.device(field.device):
        f = field.struct()
        _lib.check(field.lib.rf_maxsim(ctypes.byref(f), _ptr(q_vec), _ptr(q_len), B, _ptr(cand_off), _ptr(cand_row),
                                       _ptr(filter), _ptr(scores), _lib.current_stream_ptr()))
    return scores if candidates is None else scores[:n_out]


def maxsim_topk(scores, seg_off, k: int, rows=None, id_base: int = 0, want_exact: bool = False):
    """rf_maxsim_topk on the current stream: scores f32 (device), seg_off int64 [B + 1] -> (scores f32 [B, k],
    ids i64 [B, k]) padded with -inf / -1 (and the scores as f64 with want_exact)."""
    import torch
    dev = scores.device
    scores = scores.contiguous().view(-1)
    if scores.numel() == 0:
        scores = torch.zeros(1, dtype=torch.float32, device=dev)
    seg_off = torch.as_tensor(seg_off).to(device=dev, dtype=torch.int64).contiguous()
    rows = None if rows is None else torch.as_tensor(rows).to(device=dev, dtype=torch.int64).contiguous()
    B = seg_off.numel() - 1
    out_s = torch.empty((B, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((B, k), dtype=torch.int64, device=dev)
    exact = torch.empty((B, k), dtype=torch.float64, device=dev) if want_exact else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load_library().rf_maxsim_topk(_ptr(scores), _ptr(seg_off), _ptr(rows), B, int(k), int(id_base),
                                                      _ptr(out_s), _ptr(out_i), _ptr(exact), _lib.current_stream_ptr()))
    return (out_s, out_i, exact) if want_exact else (out_s, out_i)


# ---- the encoder ------------------------------------------------------------------------------------------------------
class ColBERT:
    """`encode(list[str], is_query=False)` -> a list of float16 [n_tok, D] arrays of unit vectors."""

    DOC_BATCH = 64     # rows of one document forward
    QUERY_BATCH = 32   # rows of one query forward

    def __init__(self, weights: dict, proj_w, cfg: dict | None = None, tokenizer=None, device=None,
                 settings: dict | None = None, query_expansion: bool | None = None):
        import torch
        from .embedder import MINILM_L6, Embedder
        cfg = dict(cfg or MINILM_L6)
        self.settings = dict(DEFAULTS, **(settings or {}))
        self.query_expansion = resolve_query_expansion(self.settings["attend_to_expansion_tokens"], query_expansion)
        proj = np.ascontiguousarray(proj_w, dtype=np.float32)
        if proj.ndim != 2 or proj.shape[1] != cfg["hidden"]:
            raise ValueError(f"the projection has shape {proj.shape}, expected [D, {cfg['hidden']}]")
        self.dim = D = int(proj.shape[0])
        if D % 16 or not 16 <= D <= _lib.RF_MAXSIM_DIM:
            raise ValueError(f"a projection to {D} features is not supported: a multiple of 16 in 16..{_lib.RF_MAXSIM_DIM}")
        self.query_length = min(int(self.settings["query_length"]), QTOK)
        # the BertModel part: the embedder's weight upload and encoder handle
        self.encoder = Embedder(weights, cfg, tokenizer, device, max(int(self.settings["document_length"]), QTOK))
        self.document_length = min(int(self.settings["document_length"]), self.encoder.max_seq_length)
        self.cfg, self.device, self.lib, self.tokenizer = cfg, self.encoder.device, self.encoder.lib, tokenizer
        self._proj = torch.as_tensor(proj).to(torch.float16).to(self.device).contiguous()   # kept alive
        self._skip = None
        if tokenizer is not None and self.settings["skiplist_words"]:
            self._skip = torch.from_numpy(skip_bitmap(tokenizer.vocab, self.settings["skiplist_words"], cfg["vocab_size"])
                                          .view(np.int32)).to(self.device)

    # -- construction -----------------------------------------------------------------
    @classmethod
    def from_local(cls, path: str, device=None, query_expansion: bool | None = None, **kw) -> "ColBERT":
        """Load config.json + vocab.txt + the weights of a ColBERT checkpoint (either layout) from a local
        directory, with the settings the directory states."""
        from .embedder import hf_encoder_config, stack_hf_state_dict
        from .tokenizer import WordPieceTokenizer
        with open(os.path.join(path, "config.json")) as f:
            cfg = hf_encoder_config(json.load(f))
        sd, proj = load_checkpoint(path)
        tok = WordPieceTokenizer.from_vocab_file(os.path.join(path, "vocab.txt"))
        return cls(stack_hf_state_dict(sd, cfg), proj, cfg, tok, device, dict(read_settings(path), **kw),
                   query_expansion)

    @classmethod
    def from_random(cls, cfg: dict | None = None, seed: int = 0, dim: int = 96, tokenizer=None, device=None,
                    **kw) -> "ColBERT":
        """Seeded random weights (random_weights(cfg, seed) + random_projection(cfg, seed, dim))."""
        from .embedder import MINILM_L6, random_weights
        cfg = dict(cfg or MINILM_L6)
        return cls(random_weights(cfg, seed), random_projection(cfg, seed, dim), cfg, tokenizer, device, **kw)

    # -- forward ------------------------------------------------------------------------
    def encode_ids(self, ids, lens, is_query: bool = False):
        """ids int32 [B, T] (padded), lens int32 [B] -> (off int32 [B + 1], vec float16 [B * T, D]) on the device;
        row b's vectors are vec[off[b] : off[b + 1]].  Documents drop the skiplist's tokens."""
        import torch
        ids = torch.as_tensor(ids, dtype=torch.int32)
        lens = torch.as_tensor(lens, dtype=torch.int32)
        if ids.dim() != 2 or lens.shape != (ids.shape[0],):
            raise ValueError("encode_ids expects ids [B, T] and lens [B]")
        B, T = ids.shape
        ids, lens = ids.to(self.device).contiguous(), lens.to(self.device).contiguous()
        skip = None if is_query else self._skip
        head = _lib.TokenHead(self._proj.data_ptr(), self.dim, None if skip is None else skip.data_ptr(),
                              int(self.cfg["vocab_size"]))
        h = self.encoder.handle
        with torch.cuda.device(self.device):
            off = torch.empty(B + 1, dtype=torch.int32, device=self.device)
            vec = torch.empty((B * T, self.dim), dtype=torch.float16, device=self.device)
            # per call: concurrent calls (any thread, any stream) never share scratch
            ws = torch.empty(self.lib.rf_encode_tokens_workspace_bytes(h, B, T), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.rf_encode_tokens(h, _ptr(ids), _ptr(lens), B, T, ctypes.byref(head), _ptr(off),
                                                 _ptr(vec), _ptr(ws), ws.numel(), _lib.current_stream_ptr()))
        return off, vec

    def rows(self, texts, is_query: bool):
        if self.tokenizer is None:
            raise RuntimeError("ColBERT has no tokenizer: construct it with from_local(path) or pass "
                               "tokenizer=WordPieceTokenizer(vocab)")
        return build_rows(self.tokenizer, texts, is_query, query_length=self.query_length,
                          document_length=self.document_length, query_marker=self.settings["query_marker"],
                          document_marker=self.settings["document_marker"], query_expansion=self.query_expansion)

    def encode(self, texts, is_query: bool = False, **_ignored) -> list:
        """Token vectors of documents (is_query=False: the skiplist's tokens dropped) or queries (at most 32
        tokens, filled with [MASK] under query expansion).  Every forward has a fixed shape -- documents
        (DOC_BATCH, document_length), queries (QUERY_BATCH, query_length), short batches filled up with rows of
        no tokens (packed away: they cost nothing) -- so a text's vectors do not depend on what it is encoded
        together with: a query alone and the same query in a batch give the same bits."""
        texts = list(texts)
        n = len(texts)
        if n == 0:
            return []
        ids, lens = self.rows(texts, is_query)
        if is_query:
            B, T = self.QUERY_BATCH, self.query_length
        else:
            B, T = self.DOC_BATCH, self.document_length
        out: list = []
        for i in range(0, n, B):
            m = min(B, n - i)
            bi = np.full((B, T), self.tokenizer.pad_id, dtype=np.int32)
            bi[:m, :ids.shape[1]] = ids[i:i + m]
            bl = np.zeros(B, dtype=np.int32)
            bl[:m] = lens[i:i + m]
            off, vec = self.encode_ids(bi, bl, is_query)
            off = off.cpu().numpy()
            vec = vec[:off[-1]].cpu().numpy()
            out.extend(vec[off[r]:off[r + 1]] for r in range(m))
        return out

    def encode_query(self, texts):
        return self.encode(texts, is_query=True)

    def encode_document(self, texts):
        return self.encode(texts, is_query=False)

    # -- scoring --------------------------------------------------------------------------
    def maxsim(self, field, queries, candidates=None, filter=None):
        return maxsim(field, queries, candidates, filter)

    def rank(self, query: str, documents, top_k: int | None = None) -> list:
        """PyLate's rank.rerank for one query: [{"corpus_id", "score"}], best first, ties in document order."""
        documents = list(documents)
        if not documents:
            return []
        field = TokenField.from_rows(self.encode(documents), self.dim, self.device)
        k = len(documents) if top_k is None else min(int(top_k), len(documents))
        if k < 1:
            raise ValueError(f"top_k must be >= 1, got {top_k}")
        q = self.encode([query], is_query=True)
        if k <= _lib.RF_MAX_K:
            s, i = field.search(q, k)
            s, i = s.cpu().numpy(), i.cpu().numpy()
        else:   # more than the selection kernel returns: the whole ranking, on the host, by the same order
            s, i = topk_reference(maxsim(field, q).cpu().numpy(), k)
        return [{"corpus_id": int(r), "score": float(v)} for v, r in zip(s[0], i[0]) if r >= 0]


def resolve_query_expansion(attended, asked: bool | None) -> bool:
    """Whether queries are filled with [MASK] tokens.  attended: what the checkpoint says about attending to
    them (None: nothing).  The encoder's attention has one length per row, so expansion tokens are ordinary
    attended tokens or absent: a checkpoint trained NOT to attend to them gets no expansion by default, and
    asking for it is refused."""
    if attended is False:
        if asked:
            raise ValueError("query_expansion=True: this checkpoint does not attend to its expansion tokens "
                             "(attend_to_expansion_tokens / attend_to_mask_tokens is false); that form needs a key "
                             "length per row in the attention kernels and is not supported")
        return False
    return True if asked is None else bool(asked)
