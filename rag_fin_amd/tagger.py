"""Entity tagging on the GPU: the named entities of texts -- the metrics a chunk mentions, the organisations, the
periods -- from a token-classification (NER) model, in the shape of the `transformers` token-classification
pipeline (`TokenClassifier.from_local(dir).predict(texts, aggregation_strategy="simple")`).  Its output is what
an ARRAY VARCHAR field and ARRAY_CONTAINS_ANY / _ALL filter on: `tags(texts)` gives the distinct entity strings of
each text, service.ingest(..., tagger=, entity_field=) stores them, VectorRAG.search(..., match_entities=) filters
on the entities of the query.

The checkpoint is a LOCAL BertForTokenClassification directory in the Hugging Face layout (config.json with
id2label, vocab.txt, model.safetensors) of the MiniLM-L{6,12}-H384 family; nothing is fetched.  The forward runs
in libragfin_hip.so (rf_tag_logits: the sentence embedder's layers, then the classifier on every token) and so
does the decode (rf_group_entities: label and score per token, BIO grouping); there is no CPU path.
`entities_reference` is the numpy definition of what rf_group_entities decodes.

Against the pipeline:
  * aggregation_strategy is "simple", "first" or "none".  "max" and "average" label a word by comparing softmax
    values across its tokens, which is no function of the order of the logits alone: they raise ValueError.
  * `word` is text[start:end], the caller's own characters -- not the pipeline's detokenised string (lower-cased,
    "##" pieces glued, spaces between tokens).
  * a text longer than the window is cut at the end of the window; its tail is not tagged.
"""
from __future__ import annotations

import ctypes
import json
import os
import warnings
from ctypes import c_void_p

import numpy as np

from . import _lib
from .embedder import MINILM_L6, Embedder, hf_encoder_config, random_weights, stack_hf_state_dict, stack_hf_tag_head
from .tokenizer import WordPieceTokenizer

STRATEGIES = {"simple": _lib.RF_TAG_SIMPLE, "first": _lib.RF_TAG_FIRST}


def random_tag_head(hidden: int, num_labels: int, seed: int = 0, head_scale: float = 0.05) -> dict:
    """Seeded token classifier (float32), a stream of its own beside random_weights(cfg, seed)."""
    rng = np.random.default_rng([seed, 5])
    return {"cls_w": (rng.standard_normal((num_labels, hidden), dtype=np.float32) * head_scale).astype(np.float32),
            "cls_b": (rng.standard_normal(num_labels, dtype=np.float32) * 0.02).astype(np.float32)}


def label_tables(labels):
    """The label names of a model (id order) -> (tag names, label_tag int32 [L], label_begin uint8 [L]):
    "B-X" -> (tag X, begin), "I-X" -> (tag X), anything else -> (tag = the label itself) -- get_tag of the
    pipeline.  Tags are numbered in the order of their first appearance."""
    tags, label_tag, label_begin = [], [], []
    for name in labels:
        name = str(name)
        begin = name.startswith("B-")
        tag = name[2:] if begin or name.startswith("I-") else name
        if tag not in tags:
            tags.append(tag)
        label_tag.append(tags.index(tag))
        label_begin.append(1 if begin else 0)
    return tags, np.array(label_tag, dtype=np.int32), np.array(label_begin, dtype=np.uint8)


def entities_reference(logits, lens, word_start, label_tag, label_begin, strategy: int, ignore_tag: int = -1,
                       max_entities: int = _lib.RF_TAGGER_MAX_ENTITIES):
    """The decode rf_group_entities performs, in numpy.
    logits: fp32 [B, T, L]; lens: [B] (clamped to 0..T); word_start: [B, T] (1 = the token starts a word; read
    under strategy 1 only, may be None under 0); label_tag int [L], label_begin [L]; strategy: 0 = RF_TAG_SIMPLE,
    1 = RF_TAG_FIRST.
      context   positions 1 .. len - 2; len < 3: none
      label     of a token: argmax over c, the smallest c among equals
      score     of a token: fp32(1 / sum_c exp(l_c - l_max)), the sum in fp64 with c ascending
      unit      SIMPLE: every context token.  FIRST: a context token with word_start = 1 (or the first context
                token) and the tokens with word_start = 0 behind it; its label and score are its first token's
      groups    a unit joins the running group iff label_tag[its label] == label_tag[the previous unit's label]
                and label_begin[its label] == 0; else it starts one
      entity    (first token of the first unit, last token of the last unit, tag of the first unit,
                fp32((the units' fp32 scores summed as fp64 in position order) / their number))
      output    groups whose tag == ignore_tag are dropped (-1: none); count = how many survive; the first
                max_entities of them in position order, the list padded with (-1, -1, -1, -inf)
    -> (entities: per row a list of max_entities (first, last, tag, np.float32 score), count int32 [B],
        tok_label int32 [B, T] (-1 outside the context), tok_score float32 [B, T] (0 outside the context))."""
    logits = np.asarray(logits, dtype=np.float32)
    B, T, L = logits.shape
    label_tag, label_begin = np.asarray(label_tag, dtype=np.int64), np.asarray(label_begin, dtype=np.int64)
    none = (-1, -1, -1, np.float32(-np.inf))
    tok_label = np.full((B, T), -1, dtype=np.int32)
    tok_score = np.zeros((B, T), dtype=np.float32)
    count = np.zeros(B, dtype=np.int32)
    out = []
    for b in range(B):
        n = min(max(int(lens[b]), 0), T)
        ents = []
        if n >= 3:
            row = logits[b, 1:n - 1]
            lab = np.argmax(row, axis=1)                                            # (the first of equal maxima)
            e = np.exp(row.astype(np.float64) - row.max(axis=1, keepdims=True).astype(np.float64))
            sc = (1.0 / np.cumsum(e, axis=1)[:, -1]).astype(np.float32)            # cumsum: c ascending, one by one
            tok_label[b, 1:n - 1], tok_score[b, 1:n - 1] = lab, sc
            starts = [k for k in range(n - 2) if strategy == 0 or k == 0 or word_start[b][k + 1]]
            groups = []                                                            # [first unit, ..., last unit]
            for u, k in enumerate(starts):
                joins = u > 0 and label_tag[lab[k]] == label_tag[lab[starts[u - 1]]] and not label_begin[lab[k]]
                if joins:
                    groups[-1].append(u)
                else:
                    groups.append([u])
            for g in groups:
                tag = int(label_tag[lab[starts[g[0]]]])
                if ignore_tag != -1 and tag == ignore_tag:
                    continue
                last = (starts[g[-1] + 1] if g[-1] + 1 < len(starts) else n - 2) - 1   # the token before the next unit
                s = np.cumsum(sc[[starts[u] for u in g]].astype(np.float64))[-1]
                ents.append((starts[g[0]] + 1, last + 1, tag, np.float32(s / len(g))))
        count[b] = len(ents)
        ents = ents[:max_entities]
        out.append(ents + [none] * (max_entities - len(ents)))
    return out, count, tok_label, tok_score


class EntityBatch:
    """What group_logits returns: device tensors, all views of ONE buffer (`packed`, int32), so that a caller
    who wants the numbers on the host downloads once.
      ent        int32 [B, max_entities, 3]   (first, last, tag); (-1, -1, -1) = none
      score      float32 [B, max_entities]    -inf = none
      count      int32 [B]                    surviving groups, also beyond max_entities
      tok_label  int32 [B, T] or None         per-token label, -1 outside the context
      tok_score  float32 [B, T] or None       per-token score, 0 outside the context"""
    def __init__(self, packed, B, T, max_entities, want_tokens):
        import torch
        self.packed, self.B, self.T, self.max_entities = packed, B, T, max_entities
        n_ent = B * max_entities * 4
        rows = packed[:n_ent].view(B, max_entities, 4)
        self.ent = rows[:, :, :3]
        self.score = rows[:, :, 3].view(torch.float32)
        self.count = packed[n_ent:n_ent + B]
        self.tok_label = self.tok_score = None
        if want_tokens:
            self.tok_label = packed[n_ent + B:n_ent + B + B * T].view(B, T)
            self.tok_score = packed[n_ent + B + B * T:].view(torch.float32).view(B, T)

    def cpu(self) -> "EntityBatch":
        """The same views over one host copy of the buffer."""
        return EntityBatch(self.packed.cpu(), self.B, self.T, self.max_entities, self.tok_label is not None)


def group_logits(logits, lens, word_start, label_tag, label_begin, strategy: int, ignore_tag: int = -1,
                 max_entities: int = _lib.RF_TAGGER_MAX_ENTITIES, want_tokens: bool = False) -> EntityBatch:
    """rf_group_entities on logits that are already on a device: logits float32 [B, T, L] (a cuda tensor), lens
    int32 [B], word_start uint8 [B, T] or None (RF_TAG_SIMPLE only), label_tag int32 [L], label_begin uint8 [L]
    -> EntityBatch of device tensors: per row what entities_reference defines."""
    import torch
    if logits.dim() != 3 or not logits.is_cuda or logits.dtype != torch.float32:
        raise ValueError("group_logits expects a float32 cuda tensor [B, T, L]")
    dev = logits.device
    B, T, L = logits.shape
    logits = logits.contiguous()
    lens = torch.as_tensor(lens, dtype=torch.int32).to(dev).contiguous()
    label_tag = torch.as_tensor(label_tag, dtype=torch.int32).to(dev).contiguous()
    label_begin = torch.as_tensor(label_begin, dtype=torch.uint8).to(dev).contiguous()
    if word_start is not None:
        word_start = torch.as_tensor(word_start, dtype=torch.uint8).to(dev).contiguous()
        if word_start.shape != (B, T):
            raise ValueError("group_logits expects word_start [B, T]")
    if lens.shape != (B,) or label_tag.shape != (L,) or label_begin.shape != (L,):
        raise ValueError("group_logits expects lens [B], label_tag [L] and label_begin [L]")
    lib = _lib.load_library()
    me = int(max_entities)
    n_ent = B * max(me, 0) * 4
    with torch.cuda.device(dev):
        packed = torch.empty(n_ent + B + (2 * B * T if want_tokens else 0), dtype=torch.int32, device=dev)
        if want_tokens:   # the library writes the context positions only
            packed[n_ent + B:n_ent + B + B * T] = -1
            packed[n_ent + B + B * T:] = 0
        base = packed.data_ptr()
        _lib.check(lib.rf_group_entities(
            c_void_p(logits.data_ptr()), c_void_p(lens.data_ptr()),
            c_void_p(word_start.data_ptr()) if word_start is not None else None, B, T, L,
            c_void_p(label_tag.data_ptr()), c_void_p(label_begin.data_ptr()), int(strategy), int(ignore_tag), me,
            c_void_p(base + 4 * (n_ent + B)) if want_tokens else None,
            c_void_p(base + 4 * (n_ent + B + B * T)) if want_tokens else None,
            c_void_p(base), c_void_p(base + 4 * n_ent), _lib.current_stream_ptr()))
    return EntityBatch(packed, B, T, me, want_tokens)


class TokenClassifier:
    """`predict(texts, aggregation_strategy="simple") -> [[{"entity_group", "score", "word", "start", "end"}, ...],
    ...]`, one list per text."""

    def __init__(self, weights: dict, head: dict, labels, cfg: dict | None = None,
                 tokenizer: WordPieceTokenizer | None = None, device=None, max_length: int | None = None):
        import torch
        cfg = dict(cfg or MINILM_L6)
        # the BertModel part: the embedder's weight upload and encoder handle
        self.encoder = Embedder(weights, cfg, tokenizer, device)
        self.cfg, self.device, self.lib, self.tokenizer = cfg, self.encoder.device, self.encoder.lib, tokenizer
        self.max_length = min(max_length or cfg["max_position"], cfg["max_position"], _lib.RF_TAGGER_MAX_T)
        self.labels = [str(name) for name in labels]
        L = len(self.labels)
        if not 1 <= L <= _lib.RF_TAGGER_MAX_LABELS:
            raise ValueError(f"{L} labels: a tagger holds 1..{_lib.RF_TAGGER_MAX_LABELS}")
        self.tag_names, self.label_tag, self.label_begin = label_tables(self.labels)
        self._tables = (torch.as_tensor(self.label_tag).to(self.device), torch.as_tensor(self.label_begin).to(self.device))
        shapes = {"cls_w": (L, cfg["hidden"]), "cls_b": (L,)}
        self._head = {}
        self._head_c = _lib.TagHead()
        for name, shape in shapes.items():
            a = np.ascontiguousarray(head[name], dtype=np.float32)
            if a.shape != shape:
                raise ValueError(f"head tensor {name} has shape {a.shape}, expected {shape}")
            t = torch.as_tensor(a).to(torch.float16).to(self.device).contiguous()
            self._head[name] = t   # kept alive: the library reads them in every call
            setattr(self._head_c, name, t.data_ptr())
        self._head_c.num_labels = L
        self._is_sub = None

    # -- construction -----------------------------------------------------------------
    @classmethod
    def from_local(cls, path: str, device=None, max_length: int | None = None) -> "TokenClassifier":
        """Load config.json (with id2label) + vocab.txt + model.safetensors of a BertForTokenClassification
        checkpoint from a local directory."""
        from safetensors.numpy import load_file
        with open(os.path.join(path, "config.json")) as f:
            hc = json.load(f)
        cfg = hf_encoder_config(hc)
        id2label = hc.get("id2label")
        if not id2label:
            raise ValueError(f"{path}/config.json has no id2label: not a token-classification checkpoint")
        labels = [id2label[k] for k in sorted(id2label, key=int)]
        if sorted(int(k) for k in id2label) != list(range(len(labels))):
            raise ValueError(f"{path}/config.json: id2label does not number its labels 0..{len(labels) - 1}")
        sd = load_file(os.path.join(path, "model.safetensors"))
        tok = WordPieceTokenizer.from_vocab_file(os.path.join(path, "vocab.txt"),
                                                 do_lower_case=bool(hc.get("do_lower_case", True)))
        return cls(stack_hf_state_dict(sd, cfg), stack_hf_tag_head(sd), labels, cfg, tok, device, max_length)

    @classmethod
    def from_random(cls, cfg: dict | None = None, labels=("O", "B-X", "I-X"), seed: int = 0, tokenizer=None,
                    device=None, scale: float = 0.05, head_scale: float = 0.05,
                    max_length: int | None = None) -> "TokenClassifier":
        """Seeded random weights (random_weights(cfg, seed) + random_tag_head(hidden, len(labels), seed)): both
        sides of a test can be rebuilt from the seed alone."""
        cfg = dict(cfg or MINILM_L6)
        labels = list(labels)
        return cls(random_weights(cfg, seed, scale), random_tag_head(cfg["hidden"], len(labels), seed, head_scale),
                   labels, cfg, tokenizer, device, max_length)

    # -- forward ------------------------------------------------------------------------
    def tag_ids(self, ids, lens):
        """ids int32 [B, T] ([CLS] text [SEP], padded), lens int32 [B] -> float32 [B, T, L] on the device: the
        logit of every label at every position < len (rf_tag_logits); positions >= len are 0."""
        import torch
        ids = torch.as_tensor(ids, dtype=torch.int32)
        lens = torch.as_tensor(lens, dtype=torch.int32)
        if ids.dim() != 2 or lens.shape != (ids.shape[0],):
            raise ValueError("tag_ids expects ids [B, T] and lens [B]")
        B, T = ids.shape
        ids, lens = (t.to(self.device).contiguous() for t in (ids, lens))
        h = self.encoder.handle
        with torch.cuda.device(self.device):
            # the library writes only the positions < len of a row
            logits = torch.zeros((B, T, len(self.labels)), dtype=torch.float32, device=self.device)
            # per call: concurrent calls (any thread, any stream) never share scratch
            ws = torch.empty(self.lib.rf_encode_workspace_bytes(h, B, T), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.rf_tag_logits(
                h, c_void_p(ids.data_ptr()), c_void_p(lens.data_ptr()), B, T, ctypes.byref(self._head_c),
                c_void_p(logits.data_ptr()), c_void_p(ws.data_ptr()), ws.numel(), _lib.current_stream_ptr()))
        return logits

    def group(self, logits, lens, word_start=None, strategy: int = _lib.RF_TAG_SIMPLE, ignore_tag: int = -1,
              max_entities: int = _lib.RF_TAGGER_MAX_ENTITIES, want_tokens: bool = False) -> EntityBatch:
        """group_logits with this model's label tables."""
        return group_logits(logits, lens, word_start, self._tables[0], self._tables[1], strategy, ignore_tag,
                            max_entities, want_tokens)

    def word_starts(self, ids) -> np.ndarray:
        """uint8, the shape of ids: 0 where the token's vocabulary piece starts with "##", else 1 ([UNK] and the
        special tokens start a word)."""
        if self._is_sub is None:
            table = np.zeros(self.cfg["vocab_size"], dtype=bool)
            for piece, i in self.tokenizer.vocab.items():
                if 0 <= i < len(table) and piece.startswith("##"):
                    table[i] = True
            self._is_sub = table
        ids = np.clip(np.asarray(ids, dtype=np.int64), 0, len(self._is_sub) - 1)
        return (~self._is_sub[ids]).astype(np.uint8)

    def _rows(self, texts):
        """[CLS] text [SEP] rows cut to max_length -> (ids, lens, per-text token offsets into its text)."""
        tok = self.tokenizer
        rows, offsets = [], []
        for t in texts:
            ids, off = tok.encode_with_offsets(t, self.max_length)
            rows.append(ids)
            offsets.append(off)
        lens = np.array([len(r) for r in rows], dtype=np.int32)
        ids = np.full((len(rows), int(lens.max())), tok.pad_id, dtype=np.int32)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = r
        return ids, lens, offsets

    def predict(self, texts, aggregation_strategy: str = "simple", ignore_labels=("O",),
                batch_tokens: int = 65536) -> list[list[dict]]:
        """One list of dicts per text, in position order.
        aggregation_strategy "simple" (a unit is a token) or "first" (a unit is a word, labelled by its first
        token): {"entity_group", "score", "word", "start", "end"} per group of entities_reference, entity_group
        the tag without its B- / I- prefix, score the mean of the units' softmax probabilities.
        "none": {"entity", "score", "index", "word", "start", "end"} per token, entity the label as the model
        names it, index the token's position in its row ([CLS] = 0).
        start / end are character offsets into the text and word == text[start:end].
        ignore_labels: groups of these tags (tokens of these labels under "none") are left out; () keeps all.
        A text of more than max_length - 2 tokens is cut there.  A text with more than RF_TAGGER_MAX_ENTITIES groups
        gives its first RF_TAGGER_MAX_ENTITIES and a RuntimeWarning."""
        if self.tokenizer is None:
            raise RuntimeError("TokenClassifier has no tokenizer: construct it with from_local(path) or pass "
                               "tokenizer=WordPieceTokenizer(vocab)")
        if aggregation_strategy in ("max", "average"):
            raise ValueError(f"aggregation_strategy {aggregation_strategy!r} is not offered: it labels a word by comparing "
                             "softmax values across tokens; use 'simple', 'first' or 'none'")
        if aggregation_strategy not in ("simple", "first", "none"):
            raise ValueError(f"aggregation_strategy must be 'simple', 'first' or 'none', got {aggregation_strategy!r}")
        if isinstance(texts, str):
            raise TypeError("predict takes a list of texts")
        texts = list(texts)
        if not texts:
            return []
        ignore = {str(name) for name in (ignore_labels or ())}
        per_token = aggregation_strategy == "none"
        strategy = STRATEGIES.get(aggregation_strategy, _lib.RF_TAG_SIMPLE)
        # one ignored tag is dropped on the device; with several the device keeps all and the rest is done here
        ignored_tags = [i for i, name in enumerate(self.tag_names) if name in ignore]
        ignore_tag = ignored_tags[0] if len(ignored_tags) == 1 and not per_token else -1
        ids, lens, offsets = self._rows(texts)
        word_start = self.word_starts(ids) if strategy == _lib.RF_TAG_FIRST else None
        # length-sorted buckets of about batch_tokens token slots, like ExtractiveReader.predict
        order = np.argsort(lens, kind="stable")
        sorted_lens = lens[order].astype(np.int64)
        n, i, pending = len(texts), 0, []
        while i < n:
            cost = np.arange(1, n - i + 1, dtype=np.int64) * sorted_lens[i:]
            j = i + max(1, int(np.searchsorted(cost, batch_tokens, side="right")))
            sel = order[i:j]
            T = int(sorted_lens[j - 1])
            logits = self.tag_ids(np.ascontiguousarray(ids[sel, :T]), lens[sel])
            ws = None if word_start is None else np.ascontiguousarray(word_start[sel, :T])
            pending.append((sel, self.group(logits, lens[sel], ws, strategy, ignore_tag, want_tokens=per_token)))
            i = j
        out = [None] * n
        for sel, batch in pending:
            host = batch.cpu()
            for r, ti in enumerate(sel):
                ti = int(ti)
                text, off = texts[ti], offsets[ti]
                if per_token:
                    lab, sc = host.tok_label.numpy()[r], host.tok_score.numpy()[r]
                    out[ti] = [{"entity": self.labels[lab[t]], "score": float(sc[t]), "index": t,
                                "word": text[off[t][0]:off[t][1]], "start": int(off[t][0]), "end": int(off[t][1])}
                               for t in range(1, int(lens[ti]) - 1) if self.labels[lab[t]] not in ignore]
                    continue
                count = int(host.count.numpy()[r])
                if count > host.max_entities:
                    warnings.warn(f"text {ti} has {count} entity groups; the first {host.max_entities} are returned",
                                  RuntimeWarning, stacklevel=2)
                ents = []
                for (first, last, tag), score in zip(host.ent.numpy()[r], host.score.numpy()[r]):
                    if first < 0:
                        break
                    if self.tag_names[tag] in ignore:
                        continue
                    c0, c1 = off[first][0], off[last][1]
                    ents.append({"entity_group": self.tag_names[tag], "score": float(score), "word": text[c0:c1],
                                 "start": int(c0), "end": int(c1)})
                out[ti] = ents
        return out

    def tags(self, texts, what: str = "word", lower: bool = True, max_per_row: int | None = None,
             aggregation_strategy: str = "first", ignore_labels=("O",)) -> list[list[str]]:
        """The distinct entity strings (what="word": text[start:end], inner whitespace collapsed) or tag names
        (what="group") of each text, in the order of their first appearance, lower-cased with `lower`, at most
        max_per_row of them: a column for an ARRAY VARCHAR field."""
        if what not in ("word", "group"):
            raise ValueError(f"what must be 'word' or 'group', got {what!r}")
        if max_per_row is not None and int(max_per_row) < 0:
            raise ValueError(f"max_per_row {max_per_row} is negative")
        out = []
        for ents in self.predict(texts, aggregation_strategy, ignore_labels):
            seen = {}
            for e in ents:
                s = " ".join(e["word"].split()) if what == "word" else e["entity_group"]
                s = s.lower() if lower else s
                if s:
                    seen.setdefault(s, None)
            out.append(list(seen)[:None if max_per_row is None else int(max_per_row)])
        return out


def entity_expr(field: str, values, how: str = "any") -> str | None:
    """ARRAY_CONTAINS_ANY / ARRAY_CONTAINS_ALL(field, [...]) over the given strings (how = "any" | "all"), or None
    for no values -- the filter VectorRAG.search(..., match_entities=) adds."""
    if how not in ("any", "all"):
        raise ValueError(f"match_entities must be 'any' or 'all', got {how!r}")
    values = list(dict.fromkeys(values))
    if not values:
        return None
    quoted = ", ".join('"' + v.replace("\\", "\\\\").replace('"', '\\"') + '"' for v in values)
    return f"ARRAY_CONTAINS_{how.upper()}({field}, [{quoted}])"
