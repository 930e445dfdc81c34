"""Learned sparse vectors (SPLADE) on the GPU, with the surface of sentence-transformers' `SparseEncoder`
(`SparseEncoder('naver/splade-...').encode_query([...]) / .encode_document([...])`): every text becomes a sparse
vector over the WordPiece vocabulary -- the terms it holds and the terms it implies -- and a Milvus
SPARSE_FLOAT_VECTOR field with metric IP ranks rows by the inner product with the query's vector.

The checkpoint is a LOCAL BertForMaskedLM directory in the Hugging Face layout (config.json, vocab.txt,
model.safetensors) of the MiniLM-L{6,12}-H384 family; nothing is fetched.  The forward runs in libragfin_hip.so
(rf_encode_terms: the sentence embedder's layers, then the MLM head max-pooled over the row's tokens, the
[tokens, V] logits never stored; rf_sparsify_terms: the exact cut to the heaviest terms); there is no CPU path.

The numpy definitions the tests compare against live here too: terms_reference, sparsify_reference,
sparse_ip_reference.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from ctypes import c_void_p

import numpy as np

from . import _lib, lexical
from .embedder import MINILM_L6, Embedder, hf_encoder_config, random_weights, stack_hf_state_dict
from .tokenizer import WordPieceTokenizer

HEAD_FIELDS = ["tr_w", "tr_b", "tr_ln_g", "tr_ln_b", "dec_w", "dec_b"]


def stack_hf_mlm_head(sd: dict) -> dict:
    """cls.predictions of a Hugging Face BertForMaskedLM state dict -> the tensors of rf_mlm_head.  A checkpoint
    saved with tied embeddings has no cls.predictions.decoder.weight: the decoder is the word embeddings."""
    def get(*names):
        for name in names:
            if name in sd:
                return np.asarray(sd[name], dtype=np.float32)
        raise KeyError(f"checkpoint lacks {names[0]} (not a BertForMaskedLM?)")
    return {"tr_w": get("cls.predictions.transform.dense.weight"),
            "tr_b": get("cls.predictions.transform.dense.bias"),
            "tr_ln_g": get("cls.predictions.transform.LayerNorm.weight"),
            "tr_ln_b": get("cls.predictions.transform.LayerNorm.bias"),
            "dec_w": get("cls.predictions.decoder.weight", "bert.embeddings.word_embeddings.weight"),
            "dec_b": get("cls.predictions.bias", "cls.predictions.decoder.bias")}


def random_mlm_head(cfg: dict, seed: int = 0, bias: float = -1.0, scale: float = 0.05, bias_std: float = 1.0) -> dict:
    """Seeded transform + decoder bias (float32), a stream of its own beside random_weights(cfg, seed).  There is
    no "dec_w": the decoder is tied to the word embeddings of the weights the head is used with.  With rows of
    N(0, 0.05^2) the logits have a standard deviation of about 1; the bias N(bias, bias_std^2) decides how many
    of the pooled weights are zero."""
    rng = np.random.default_rng([seed, 2])
    H, V = cfg["hidden"], cfg["vocab_size"]

    def mat(*shape, s):
        return (rng.standard_normal(shape, dtype=np.float32) * s).astype(np.float32)
    return {"tr_w": mat(H, H, s=scale), "tr_b": mat(H, s=0.02), "tr_ln_g": 1 + mat(H, s=0.1),
            "tr_ln_b": mat(H, s=0.1), "dec_b": (np.float32(bias) + mat(V, s=bias_std)).astype(np.float32)}


# ---- the definitions (numpy, host) -----------------------------------------------------------------------------------
try:
    from scipy.special import erf as _erf
except Exception:  # pragma: no cover
    _erf = np.vectorize(math.erf)


def _layer_norm(x, g, b, eps):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def _gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def hidden_reference(w: dict, cfg: dict, ids, lens, dtype=np.float64) -> np.ndarray:
    """The last hidden state [B, T, H] of a BertModel with token types 0 and the key mask of `lens`."""
    H, L, NH = cfg["hidden"], cfg["layers"], cfg["heads"]
    dh = H // NH
    eps = cfg["ln_eps"]
    W = {k: np.asarray(v).astype(dtype) for k, v in w.items()}
    ids = np.asarray(ids)
    B, T = ids.shape
    mask = np.arange(T)[None, :] < np.asarray(lens)[:, None]
    x = W["word_emb"][ids] + W["pos_emb"][None, :T] + W["type_emb"][0][None, None]
    x = _layer_norm(x, W["emb_ln_g"], W["emb_ln_b"], eps)
    neg = np.where(mask, 0.0, -np.inf)[:, None, None, :]
    neg = np.where(mask.any(axis=1)[:, None, None, None], neg, 0.0)   # a row without tokens: no NaN, never read
    for l in range(L):
        q, k, v = np.split(x @ W["qkv_w"][l].T + W["qkv_b"][l], 3, axis=-1)

        def heads(t):
            return t.reshape(B, T, NH, dh).transpose(0, 2, 1, 3)
        s = heads(q) @ heads(k).transpose(0, 1, 3, 2) / math.sqrt(dh) + neg
        p = np.exp(s - s.max(axis=-1, keepdims=True))
        p = p / p.sum(axis=-1, keepdims=True)
        ctx = (p @ heads(v)).transpose(0, 2, 1, 3).reshape(B, T, H)
        x = _layer_norm(x + ctx @ W["ao_w"][l].T + W["ao_b"][l], W["ln1_g"][l], W["ln1_b"][l], eps)
        h = _gelu(x @ W["ff1_w"][l].T + W["ff1_b"][l])
        x = _layer_norm(x + h @ W["ff2_w"][l].T + W["ff2_b"][l], W["ln2_g"][l], W["ln2_b"][l], eps)
    return x


def terms_reference(w16: dict, head16: dict, cfg: dict, ids, lens, dtype=np.float64, hidden=None) -> np.ndarray:
    """The definition of rf_encode_terms in fp64 -> [B, V]: log1p(relu(.)) of the MLM logits, max-pooled over
    the tokens t < lens[b] ([CLS] and [SEP] included); a row without tokens is all zeros.  A head without
    "dec_w" is tied to w16["word_emb"].  hidden: the last hidden state, when the caller has it already."""
    lens = np.asarray(lens)
    x = hidden_reference(w16, cfg, ids, lens, dtype) if hidden is None else np.asarray(hidden, dtype=dtype)
    hd = {k: np.asarray(v).astype(dtype) for k, v in head16.items()}
    dec_w = hd["dec_w"] if "dec_w" in hd else np.asarray(w16["word_emb"]).astype(dtype)
    g = _layer_norm(_gelu(x @ hd["tr_w"].T + hd["tr_b"]), hd["tr_ln_g"], hd["tr_ln_b"], cfg["ln_eps"])
    out = np.zeros((x.shape[0], dec_w.shape[0]), dtype=dtype)
    for b in range(x.shape[0]):   # (row by row: the [T, V] logits of one row at a time)
        n = int(min(max(lens[b], 0), x.shape[1]))
        if n:
            out[b] = np.log1p(np.maximum((g[b, :n] @ dec_w.T + hd["dec_b"]).max(axis=0), 0.0))
    return out


def sparsify_reference(weights, max_terms: int):
    """The definition of rf_sparsify_terms -> (off int32 [B + 1], term int32 [nnz], val fp32 [nnz]): per row the
    entries > 0, of more than max_terms the best by (value descending, term id ascending), emitted in ascending
    term id."""
    weights = np.asarray(weights, dtype=np.float32)
    off, terms, vals = [0], [], []
    for row in weights:
        pos = np.flatnonzero(row > 0)
        if pos.size > max_terms:
            pos = np.sort(pos[np.lexsort((pos, -row[pos].astype(np.float64)))][:max_terms])
        terms.append(pos.astype(np.int32))
        vals.append(row[pos])
        off.append(off[-1] + pos.size)
    cat = lambda a, dt: np.concatenate(a).astype(dt) if a else np.zeros(0, dt)   # noqa: E731
    return np.asarray(off, dtype=np.int32), cat(terms, np.int32), cat(vals, np.float32)


class TermPostings:
    """Rows of term weights transposed to what SparseIndex takes: n_rows, n_terms, post_off int64 [V + 1],
    post_row uint32 and post_imp fp32 [nnz] -- a stable sort by term, so rows ascend within a term."""

    def __init__(self, indptr, indices, data, n_terms: int):
        indptr = np.asarray(indptr, dtype=np.int64)
        indices = np.asarray(indices, dtype=np.int64)
        self.n_rows, self.n_terms = int(indptr.size - 1), int(n_terms)
        rows = np.repeat(np.arange(self.n_rows, dtype=np.int64), np.diff(indptr))
        order = np.argsort(indices, kind="stable")
        self.post_row = rows[order].astype(np.uint32)
        self.post_imp = np.asarray(data, dtype=np.float32)[order]
        self.post_off = np.zeros(self.n_terms + 1, dtype=np.int64)
        np.cumsum(np.bincount(indices, minlength=self.n_terms), out=self.post_off[1:])

    @property
    def nnz(self) -> int:
        return int(self.post_row.size)

    @classmethod
    def from_csr(cls, csr) -> "TermPostings":
        return cls(csr.indptr, csr.indices, csr.data, csr.shape[1])


def sparse_ip_reference(doc_csr, q_csr, k: int, mask=None):
    """The definition of a learned-sparse search in numpy -> (scores fp32 [B, k], ids int64 [B, k]) padded with
    -inf / -1: rf_sparse_search over the transposed rows, i.e. per row acc = 0.0f, then for the query's terms in
    ascending id acc = acc + (q_weight * doc_weight) with two fp32 roundings and no fma; a hit has acc > 0; the
    best k by (score descending, row ascending).  Both operands CSR with sorted indices."""
    q = q_csr.tocsr() if hasattr(q_csr, "tocsr") else q_csr
    scores, ids, _ = lexical.bm25_reference(TermPostings.from_csr(doc_csr), q.indptr, q.indices,
                                            np.asarray(q.data, dtype=np.float32), k, mask)
    return scores, ids


def check_query_rows(rows, n_terms: int, max_terms: int = _lib.RF_SPARSE_MAX_TERMS):
    """Caller-supplied sparse query vectors -- a scipy sparse matrix or a list of {term_id: weight} dicts, the
    pymilvus forms -- -> the CSR batch (q_off int32, q_term int32 ascending, q_weight fp32).  ValueError: more
    than max_terms non-zeros, a weight that is not finite and > 0, a term id outside [0, n_terms)."""
    if hasattr(rows, "tocsr"):
        m = rows.tocsr()
        m.sort_indices()
        rows = [dict(zip(m.indices[m.indptr[i]:m.indptr[i + 1]].tolist(), m.data[m.indptr[i]:m.indptr[i + 1]].tolist()))
                for i in range(m.shape[0])]
    off, terms, vals = [0], [], []
    for i, row in enumerate(rows):
        if not isinstance(row, dict):
            raise ValueError("a sparse query vector is a {term_id: weight} dict or a row of a scipy sparse matrix")
        if len(row) > max_terms:
            raise ValueError(f"sparse query {i} has {len(row)} non-zeros, more than {max_terms}")
        for t in sorted(row):
            wv = float(row[t])
            if int(t) != t or not 0 <= int(t) < n_terms:
                raise ValueError(f"sparse query {i}: term id {t!r} outside [0, {n_terms})")
            if not (math.isfinite(wv) and wv > 0 and np.float32(wv) > 0 and np.isfinite(np.float32(wv))):
                raise ValueError(f"sparse query {i}: weight {row[t]!r} of term {t} is not finite and > 0")
            terms.append(int(t))
            vals.append(wv)
        off.append(len(terms))
    return np.asarray(off, np.int32), np.asarray(terms, np.int32), np.asarray(vals, np.float32)


# ---- the encoder ------------------------------------------------------------------------------------------------------
class SparseEncoder:
    """`encode_document(list[str])`, `encode_query(list[str])` -> scipy.sparse.csr_array [n, V] fp32."""

    def __init__(self, weights: dict, head: dict, cfg: dict | None = None, tokenizer: WordPieceTokenizer | None = None,
                 device=None, max_seq_length: int = 256, max_terms: int = 128, query_max_terms: int = 64):
        import torch
        cfg = dict(cfg or MINILM_L6)
        if not 1 <= int(max_terms) <= _lib.RF_TERMS_MAX:
            raise ValueError(f"max_terms = {max_terms} outside 1..{_lib.RF_TERMS_MAX}")
        if not 1 <= int(query_max_terms) <= _lib.RF_SPARSE_MAX_TERMS:
            raise ValueError(f"query_max_terms = {query_max_terms} outside 1..{_lib.RF_SPARSE_MAX_TERMS} "
                             "(the terms one query of rf_sparse_search holds)")
        # the BertModel part: the embedder's weight upload and encoder handle
        self.encoder = Embedder(weights, cfg, tokenizer, device, max_seq_length)
        self.cfg, self.device, self.lib, self.tokenizer = cfg, self.encoder.device, self.encoder.lib, tokenizer
        self.max_seq_length = self.encoder.max_seq_length
        self.max_terms, self.query_max_terms = int(max_terms), int(query_max_terms)
        self.vocab_size = V = int(cfg["vocab_size"])
        H = cfg["hidden"]
        shapes = {"tr_w": (H, H), "tr_b": (H,), "tr_ln_g": (H,), "tr_ln_b": (H,), "dec_w": (V, H), "dec_b": (V,)}
        self._head = {}
        self._head_c = _lib.MlmHead(vocab=V)
        for name in HEAD_FIELDS:
            if name == "dec_w" and head.get("dec_w") is None:
                t = self.encoder._w["word_emb"]   # tied: the embedder's own device copy
            else:
                a = np.ascontiguousarray(head[name], dtype=np.float32)
                if a.shape != shapes[name]:
                    raise ValueError(f"head tensor {name} has shape {a.shape}, expected {shapes[name]}")
                t = torch.as_tensor(a).to(torch.float16).to(self.device).contiguous()
            self._head[name] = t   # kept alive: the library reads them in every call
            setattr(self._head_c, name, t.data_ptr())
        self._id_to_token = None

    # -- construction -----------------------------------------------------------------
    @classmethod
    def from_local(cls, path: str, device=None, max_seq_length: int | None = None, **kw) -> "SparseEncoder":
        """Load config.json + vocab.txt + model.safetensors of a BertForMaskedLM checkpoint (a SPLADE model of
        the MiniLM-H384 family) from a local directory."""
        from safetensors.numpy import load_file
        with open(os.path.join(path, "config.json")) as f:
            cfg = hf_encoder_config(json.load(f))
        sd = load_file(os.path.join(path, "model.safetensors"))
        tok = WordPieceTokenizer.from_vocab_file(os.path.join(path, "vocab.txt"))
        return cls(stack_hf_state_dict(sd, cfg), stack_hf_mlm_head(sd), cfg, tok, device, max_seq_length or 256, **kw)

    @classmethod
    def from_random(cls, cfg: dict | None = None, seed: int = 0, tokenizer=None, device=None, bias: float = -1.0,
                    **kw) -> "SparseEncoder":
        """Seeded random weights (random_weights(cfg, seed) + random_mlm_head(cfg, seed, bias), tied decoder)."""
        cfg = dict(cfg or MINILM_L6)
        return cls(random_weights(cfg, seed), random_mlm_head(cfg, seed, bias), cfg, tokenizer, device, **kw)

    # -- forward ------------------------------------------------------------------------
    def encode_ids(self, ids, lens):
        """ids int32 [B, T] (padded), lens int32 [B] -> the dense term weights, float32 [B, V] on the device."""
        import torch
        ids = torch.as_tensor(ids, dtype=torch.int32)
        lens = torch.as_tensor(lens, dtype=torch.int32)
        if ids.dim() != 2 or lens.shape != (ids.shape[0],):
            raise ValueError("encode_ids expects ids [B, T] and lens [B]")
        B, T = ids.shape
        ids, lens = ids.to(self.device).contiguous(), lens.to(self.device).contiguous()
        h = self.encoder.handle
        with torch.cuda.device(self.device):
            out = torch.empty((B, self.vocab_size), dtype=torch.float32, device=self.device)
            # per call: concurrent calls (any thread, any stream) never share scratch
            ws = torch.empty(self.lib.rf_encode_terms_workspace_bytes(h, B, T), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.rf_encode_terms(h, c_void_p(ids.data_ptr()), c_void_p(lens.data_ptr()), B, T,
                                                ctypes.byref(self._head_c), c_void_p(out.data_ptr()),
                                                c_void_p(ws.data_ptr()), ws.numel(), _lib.current_stream_ptr()))
        return out

    def sparsify(self, weights, max_terms: int):
        """rf_sparsify_terms over dense float32 [B, V] weights on the device -> (off int32 [B + 1], term int32,
        val float32) device tensors; the entries are term[: off[B]]."""
        import torch
        weights = torch.as_tensor(weights, dtype=torch.float32).to(self.device).contiguous()
        B, V = weights.shape
        with torch.cuda.device(self.device):
            off = torch.empty(B + 1, dtype=torch.int32, device=self.device)
            term = torch.empty(B * max_terms, dtype=torch.int32, device=self.device)
            val = torch.empty(B * max_terms, dtype=torch.float32, device=self.device)
            _lib.check(self.lib.rf_sparsify_terms(c_void_p(weights.data_ptr()), B, V, int(max_terms),
                                                  c_void_p(off.data_ptr()), c_void_p(term.data_ptr()),
                                                  c_void_p(val.data_ptr()), _lib.current_stream_ptr()))
        return off, term, val

    DOC_BATCH = 64   # rows of one document forward

    def _encode(self, texts, max_terms: int, fixed_shape: bool, batch_tokens: int = 16384):
        from scipy.sparse import csr_array
        if self.tokenizer is None:
            raise RuntimeError("SparseEncoder has no tokenizer: construct it with from_local(path) or pass "
                               "tokenizer=WordPieceTokenizer(vocab)")
        texts = list(texts)
        n, V = len(texts), self.vocab_size
        if n == 0:
            return csr_array((0, V), dtype=np.float32)
        ids, lens = self.tokenizer.batch(texts, self.max_seq_length)
        batches = []   # (rows of the input, ids [B, T], lens [B])
        if fixed_shape:
            # every forward has the shape (DOC_BATCH, max_seq_length), short batches filled up with rows of no
            # tokens (packed away: they cost nothing): rf_encode_terms gives a row the same bits at any place of
            # any batch of one shape, so a document's vector is a function of its text alone -- rows encoded alone
            # after an insert are what a build of the whole collection would hold
            B, T = self.DOC_BATCH, self.max_seq_length
            for i in range(0, n, B):
                sel = np.arange(i, min(i + B, n))
                bi = np.full((B, T), self.tokenizer.pad_id, dtype=np.int32)
                bi[:sel.size, :ids.shape[1]] = ids[sel]
                bl = np.zeros(B, dtype=np.int32)
                bl[:sel.size] = lens[sel]
                batches.append((sel, bi, bl))
        else:
            # length-sorted buckets of about batch_tokens token slots, like the text ingest: rows are sorted
            # ascending, so a bucket's last row sets its width (the dense weights of a bucket: B * V * 4 bytes)
            order = np.argsort(lens, kind="stable")
            sorted_lens = lens[order].astype(np.int64)
            i = 0
            while i < n:
                cost = np.arange(1, n - i + 1, dtype=np.int64) * sorted_lens[i:]
                j = i + max(1, int(np.searchsorted(cost, batch_tokens, side="right")))
                sel = order[i:j]
                T = max(1, int(sorted_lens[j - 1]))
                batches.append((sel, np.ascontiguousarray(ids[sel, :T]), lens[sel]))
                i = j
        rows: list = [None] * n
        for sel, bi, bl in batches:
            off, term, val = self.sparsify(self.encode_ids(bi, bl), max_terms)
            off = off.cpu().numpy()
            term, val = term[:off[-1]].cpu().numpy(), val[:off[-1]].cpu().numpy()
            for r, s in enumerate(sel):
                rows[s] = (term[off[r]:off[r + 1]], val[off[r]:off[r + 1]])
        indptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([r[0].size for r in rows], out=indptr[1:])
        return csr_array((np.concatenate([r[1] for r in rows]).astype(np.float32),
                          np.concatenate([r[0] for r in rows]).astype(np.int32), indptr), shape=(n, V))

    def encode_document(self, texts, **_ignored):
        """Sparse vectors of documents, cut to max_terms.  Every forward has one shape, so a document's vector
        does not depend on what it is encoded together with."""
        return self._encode(texts, self.max_terms, True)

    encode = encode_document

    def encode_query(self, texts, **_ignored):
        """Sparse vectors of queries, cut to query_max_terms (<= the terms one query of the search holds)."""
        return self._encode(texts, self.query_max_terms, False)

    def decode(self, row, top_k: int | None = None) -> list[tuple[str, float]]:
        """A sparse (one row of a csr_array) or dense vector -> [(token, weight)], heaviest first; equal weights
        in ascending term id."""
        if hasattr(row, "tocsr"):
            m = row.tocsr()
            if m.shape[0] != 1:
                raise ValueError("decode takes one row")
            idx, val = m.indices, m.data
        else:
            dense = np.asarray(row, dtype=np.float32).reshape(-1)
            idx = np.flatnonzero(dense > 0)
            val = dense[idx]
        order = np.lexsort((idx, -np.asarray(val, dtype=np.float64)))
        if top_k is not None:
            order = order[:top_k]
        if self._id_to_token is None and self.tokenizer is not None:
            self._id_to_token = {i: t for t, i in self.tokenizer.vocab.items()}
        name = (self._id_to_token or {}).get
        return [(name(int(idx[i]), str(int(idx[i]))), float(val[i])) for i in order]
