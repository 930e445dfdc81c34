"""Wiring: build a VectorRAG from local files / environment, and the ingest step.

Environment (dotenv-style names):
  RAGFIN_MODEL_DIR     local all-MiniLM-L6-v2 directory (config.json, vocab.txt,
                       model.safetensors).  Required: nothing is fetched by name.  A sentence-transformers
                       directory of the same BERT-H384 family (bge-small-en-v1.5, e5-small-v2, gte-small,
                       multi-qa-MiniLM-L6-dot-v1, snowflake-arctic-embed-s) is read with its own modules.json,
                       Pooling config and prompts (rag_fin_amd.embedder.sentence_config)
  RAGFIN_QUERY_PROMPT  the prompt queries are embedded behind ("query: " for E5, which ships none in its files);
                       overrides the directory's "query" prompt
  RAGFIN_DOCUMENT_PROMPT  the prompt chunks are embedded behind ("passage: "); overrides the directory's
                       "document" prompt
  RAGFIN_POOLING       mean | cls | max | mean_sqrt_len: overrides the directory's Pooling config
  RAGFIN_METRIC        COSINE | IP (or cosine | dot): the store's metric.  Unset: IP when the model says
                       similarity_fn_name "dot", COSINE otherwise; euclidean / manhattan are refused
  RERANKER_MODEL_DIR   optional local cross-encoder directory (e.g. ms-marco-MiniLM-L-6-v2, same three
                       files): enables search(..., rerank=True)
  READER_MODEL_DIR     optional local extractive-reader directory (a BertForQuestionAnswering such as
                       minilm-uncased-squad2, same three files): search_and_answer answers with a span of a
                       retrieved chunk when no generator is plugged in
  READER_DOC_STRIDE    optional overlap in tokens: the reader reads a context that does not fit its window in
                       sliding windows decoded as one context (ExtractiveReader(doc_stride=...)); unset: it is cut
  SPARSE_MODEL_DIR     optional local SPLADE directory (a BertForMaskedLM of the MiniLM-H384 family, same three
                       files): declares the learned sparse field, enables search(..., hybrid=True,
                       lexical="learned" | "both")
  COLBERT_MODEL_DIR    optional local ColBERT directory (a BertModel of the same family plus a projection, Stanford
                       or PyLate layout): declares the late-interaction field, enables search(..., rerank=True,
                       rerank_with="late")
  TAGGER_MODEL_DIR     optional local token-classification (NER) directory (a BertForTokenClassification of the
                       same family, same three files, id2label in config.json): the entities of every chunk are
                       stored at ingest and search(..., match_entities="any" | "all") filters on the query's
  TAGGER_FIELD         the field the entities go to (default "entities"): a declared ARRAY VARCHAR field, or a
                       dynamic key of a store with enable_dynamic_field
  LEXICAL_INDEX        1: declare the lexical (BM25) index at ingest: enables search(..., hybrid=True)
  RAGFIN_DATA_DIR      folder with icici_q{1..4}_2023/*.json (default: extract_data)
  RAGFIN_DEVICE        torch device string (default cuda:0)
  WORLD_SIZE / RANK / LOCAL_RANK (torch.distributed.run): with WORLD_SIZE > 1 the corpus is
                       row-sharded over the ranks' GPUs (build_sharded_rag); rank 0 serves, the
                       other ranks follow it
  MILVUS_COLLECTION    collection name reported by the tools (default fin_chunks)
"""
from __future__ import annotations

import os

from . import chunker


def extra_columns(fields, chunks, values=None, dynamic: bool = False) -> dict:
    """The columns of a store's own fields for a list of chunks.  values: {field name: a constant, or a
    function of the chunk dict}; a field without an entry is read from the chunk dicts when every chunk holds
    its name, and is otherwise left to its default.  E.g. {"bank": "ICICI", "fiscal_year": lambda c:
    2000 + int(c["period"][-2:])}.
    dynamic: the store has enable_dynamic_field: a name of `values` that is no declared field is a dynamic key
    (its column follows the declared ones in the result); a function may return None: that chunk lacks the key."""
    values = dict(values or {})
    names = [f.name for f in fields]
    for name in values:
        if name not in names and not dynamic:
            raise ValueError(f"field_values: {name!r} is not a declared field" + (f" ({', '.join(names)})" if names else ""))
    out = {}
    for name in names:
        if name in values:
            v = values[name]
            out[name] = [v(c) for c in chunks] if callable(v) else [v] * len(chunks)
        elif chunks and all(name in c for c in chunks):
            out[name] = [c[name] for c in chunks]
    for name, v in values.items():
        if name not in names:
            out[name] = [v(c) for c in chunks] if callable(v) else [v] * len(chunks)
    return out


def store_metric(embedder, metric: str | None = None) -> str:
    """The metric_type of the store behind `embedder`: `metric` when given (COSINE | IP, or sentence-transformers'
    cosine | dot), else IP for a model whose similarity_fn_name is "dot" and COSINE otherwise.  euclidean and
    manhattan raise ValueError: the store has no L2 metric."""
    name = metric if metric else (getattr(embedder, "similarity_fn_name", None) or "cosine")
    key = str(name).strip().lower()
    if key in ("cosine", "cos_sim"):
        return "COSINE"
    if key in ("ip", "dot", "dot_product"):
        return "IP"
    if key in ("euclidean", "manhattan", "l2", "l1"):
        raise ValueError(f"similarity {name!r} is not offered: the store searches by COSINE or IP (there is no L2 metric)")
    raise ValueError(f"metric must be COSINE or IP, not {name!r}")


def load_embedder(model_dir: str, device=None, query_prompt: str | None = None, document_prompt: str | None = None,
                  pooling: str | None = None):
    """Embedder.from_local with the overrides build_rag takes: a query / document prompt given here replaces the
    directory's prompt of that name, the others stay."""
    from .embedder import Embedder, sentence_config
    kw = {}
    if query_prompt or document_prompt:
        prompts = dict(sentence_config(model_dir)["prompts"])
        if query_prompt:
            prompts["query"] = query_prompt
        if document_prompt:
            prompts["document"] = document_prompt
        kw["prompts"] = prompts
    if pooling:
        kw["pooling"] = pooling
    return Embedder.from_local(model_dir, device=device, **kw)


def document_prompt_args(embedder) -> dict:
    """{"prompt": the embedder's document prompt} when it has a non-empty one, else nothing: an embedder with the
    signature of before is called as before."""
    p = getattr(embedder, "document_prompt", None)
    return {"prompt": p} if isinstance(p, str) and p else {}


ENTITY_CAPACITY = 16   # max_capacity of the entity field build_rag declares when the caller declared none


def entity_column(store, tagger, entity_field: str, texts, batch: int = 256):
    """The entities of `texts` as the column of `entity_field`: tagger.tags(texts) in batches of `batch` texts (one
    forward per length bucket of a batch, not one per text).  A declared ARRAY VARCHAR field takes each row's
    distinct entity strings, cut to its max_capacity -> (column, False).  On a store with enable_dynamic_field a
    name that is no declared field is a dynamic key; dynamic keys hold no lists, so it takes the row's first
    entity string, or None (the row lacks the key) -> (column, True).  Anything else: ValueError."""
    from .schema import DataType
    if not isinstance(entity_field, str) or not entity_field:
        raise ValueError("entity_field must name the field the entities go to")
    field = next((f for f in getattr(store, "schema", ()) if f.name == entity_field), None)
    dynamic = field is None and bool(getattr(store, "enable_dynamic_field", False))
    if field is None and not dynamic:
        raise ValueError(f"entity_field: {entity_field!r} is not a field the store declares (declare it as ARRAY of "
                         "VARCHAR, or create the store with enable_dynamic_field)")
    if field is not None and not (field.is_array and field.element_type == DataType.VARCHAR):
        raise ValueError(f"entity_field: {entity_field!r} is {field.dtype.name}, the entities need an ARRAY of VARCHAR")
    cap = 1 if dynamic else field.max_capacity
    rows = []
    for i in range(0, len(texts), batch):
        rows.extend(tagger.tags(texts[i:i + batch], max_per_row=cap))
    if dynamic:
        return [r[0] if r else None for r in rows], True
    return rows, False


def ingest(store, embedder, chunks, upsert: bool = False, field_values: dict | None = None, tagger=None,
           entity_field: str | None = None) -> int:
    """The reference's encode + insert + flush + load
    ("chunking_storing (1).py":377-397) on the GPU: texts are embedded by rf_encode
    and the fp16 rows go straight into the HBM corpus (no host round trip).
    upsert=True: chunks whose id is already stored replace the stored rows (a restated
    quarter is re-ingested in place of dropping the collection); otherwise an existing id
    raises ValueError.
    field_values: the values of the store's own fields (CorpusStore(fields=...)), as extra_columns takes them;
    on a store with enable_dynamic_field a name that is no declared field becomes a dynamic key.
    tagger / entity_field (both or neither): the entities a rag_fin_amd.tagger.TokenClassifier finds in every
    chunk's text fill the field entity_field, as entity_column lays them out."""
    if (tagger is None) != (entity_field is None):
        raise ValueError("tagger and entity_field go together")
    if not chunks:
        return 0
    tagged = None
    if tagger is not None:
        if field_values and entity_field in field_values:
            raise ValueError(f"field_values already names {entity_field!r}, the field the tagger fills")
        tagged = entity_column(store, tagger, entity_field, [c["text"] for c in chunks])[0]
    emb = embedder.encode_to_device([c["text"] for c in chunks], **document_prompt_args(embedder))
    cols = chunker.insert_columns(chunks, emb)
    fields = getattr(store, "schema", ())
    dynamic = bool(getattr(store, "enable_dynamic_field", False))
    if fields or field_values or tagged is not None:
        own = extra_columns(fields, chunks, field_values, dynamic)
        if tagged is not None:
            own[entity_field] = tagged
        missing = [f.name for f in fields if f.name not in own and f.default is None]
        if missing:
            raise ValueError(f"ingest: no value for the field(s) {', '.join(missing)} (field_values, a key of the chunk "
                             "dicts, or a default)")
        cols = cols + [own.get(f.name) if f.name in own else [f.default] * len(chunks) for f in fields]
        keys = [k for k in own if k not in {f.name for f in fields}]
        if keys:   # the rows' $meta: the trailing column of insert / upsert
            cols = cols + [[{k: own[k][j] for k in keys if own[k][j] is not None} for j in range(len(chunks))]]
    n = store.upsert(cols).upsert_count if upsert else store.insert(cols)
    store.flush()
    store.load()
    return n


def _load_reranker(reranker_dir, device):
    if not reranker_dir:
        return None
    from .reranker import CrossEncoder
    return CrossEncoder.from_local(reranker_dir, device=device)


def _load_reader(reader_dir, device, doc_stride=None):
    if not reader_dir:
        return None
    from .reader import ExtractiveReader
    return ExtractiveReader.from_local(reader_dir, device=device, doc_stride=doc_stride)


def _load_sparse_encoder(sparse_dir, device):
    if not sparse_dir:
        return None
    from .sparse_encoder import SparseEncoder
    return SparseEncoder.from_local(sparse_dir, device=device)


def _load_tagger(tagger_dir, device):
    if not tagger_dir:
        return None
    from .tagger import TokenClassifier
    return TokenClassifier.from_local(tagger_dir, device=device)


def _load_late_encoder(late_dir, device):
    if not late_dir:
        return None
    from .late_interaction import ColBERT
    return ColBERT.from_local(late_dir, device=device)


def build_rag(model_dir: str, data_dir: str = "extract_data", device=None,
              collection_name: str = "fin_chunks", generator=None, reranker_dir: str | None = None,
              hybrid: bool = False, reader_dir: str | None = None, reader_doc_stride: int | None = None,
              sparse_dir: str | None = None, late_dir: str | None = None, fields=None, field_values: dict | None = None,
              extra_output_fields=None, enable_dynamic_field: bool = False, tagger_dir: str | None = None,
              entity_field: str | None = None, query_prompt: str | None = None, document_prompt: str | None = None,
              pooling: str | None = None, metric: str | None = None):
    """query_prompt / document_prompt / pooling: overrides of what the model directory says (load_embedder).
    metric: the store's metric_type (store_metric): unset, IP for a model that says similarity_fn_name "dot".
    hybrid: declare the lexical (BM25) index over the chunk texts, so that search(..., hybrid=True)
    can run; its posting lists are built by the first such search.
    sparse_dir: a local SPLADE checkpoint: the learned sparse field is declared on the store (VectorRAG does
    it), its vectors are encoded by the first search(..., hybrid=True, lexical="learned" | "both").
    late_dir: a local ColBERT checkpoint: the late-interaction field is declared on the store (VectorRAG does it),
    its token vectors are encoded by the first search(..., rerank=True, rerank_with="late").
    fields: FieldSchema objects of the collection's own scalar fields (rag_fin_amd.schema); field_values: their
    values per chunk, as extra_columns takes them; extra_output_fields: those of them the context dicts carry.
    enable_dynamic_field: the store takes keys no field declares (a name of field_values that is no declared field
    becomes one; extra_output_fields may name them).
    tagger_dir: a local token-classification checkpoint; entity_field (default "entities" with a tagger): the
    declared ARRAY VARCHAR field, or dynamic key, its entities fill at ingest and search(..., match_entities=)
    filters on.  Where `fields` does not declare it and the store is not dynamic, it is declared here as an ARRAY
    of VARCHAR with max_capacity ENTITY_CAPACITY."""
    from .rag import VectorRAG
    from .store import CorpusStore
    embedder = load_embedder(model_dir, device, query_prompt, document_prompt, pooling)
    metric_type = store_metric(embedder, metric)
    tagger = _load_tagger(tagger_dir, device)
    if tagger is None and entity_field is not None:
        raise ValueError("entity_field needs a tagger (tagger_dir)")
    tagging = {} if tagger is None else {"tagger": tagger, "entity_field": entity_field or "entities"}
    if tagger is not None and not enable_dynamic_field and tagging["entity_field"] not in [f.name for f in fields or ()]:
        # the field the entities go to, declared here when the caller did not
        from .schema import DataType, FieldSchema
        fields = list(fields or ()) + [FieldSchema(tagging["entity_field"], DataType.ARRAY, element_type=DataType.VARCHAR,
                                                   max_capacity=ENTITY_CAPACITY)]
    store = CorpusStore(collection_name, dim=embedder.dim, device=device, **({"fields": fields} if fields else {}),
                        **({"metric_type": metric_type} if metric_type != "COSINE" else {}),
                        **({"enable_dynamic_field": True} if enable_dynamic_field else {}))
    ingest(store, embedder, chunker.build_all_chunks(data_dir), **({"field_values": field_values} if field_values else {}),
           **tagging)
    if hybrid:
        store.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
    sparse = _load_sparse_encoder(sparse_dir, device)
    late = _load_late_encoder(late_dir, device)
    return VectorRAG(None, collection_name, embedder=embedder, store=store, generator=generator,
                     reranker=_load_reranker(reranker_dir, device), reader=_load_reader(reader_dir, device, reader_doc_stride),
                     **({} if sparse is None else {"sparse_encoder": sparse}),
                     **({} if late is None else {"late_encoder": late}),
                     **({"extra_output_fields": extra_output_fields} if extra_output_fields else {}), **tagging)


def ingest_sharded(store, embedder, chunks, upsert: bool = False) -> int:
    """COLLECTIVE form of ingest(): every rank holds the whole chunk list (text work is cheap),
    embeds only ITS slice (encoder replicas) and keeps those rows in its HBM.
    upsert: as for ingest()."""
    from .sharded import ShardedSearcher
    if not chunks:
        return 0
    lo, hi = ShardedSearcher.shard_bounds(len(chunks), store.world, store.rank)
    emb = embedder.encode_to_device([c["text"] for c in chunks[lo:hi]], **document_prompt_args(embedder))
    cols = chunker.insert_columns(chunks, None)
    if upsert:
        cols[2] = emb
        n = store.upsert(cols, local=True).upsert_count
    else:
        n = store.add(cols[0], cols[1], emb, cols[3], cols[4], cols[5], cols[6], local=True)
    store.flush()
    store.load()
    return n


def build_sharded_rag(model_dir: str, data_dir: str = "extract_data", local_rank: int = 0,
                      collection_name: str = "fin_chunks", generator=None, backend: str = "nccl",
                      reranker_dir: str | None = None, reader_dir: str | None = None,
                      reader_doc_stride: int | None = None, query_prompt: str | None = None,
                      document_prompt: str | None = None, pooling: str | None = None, metric: str | None = None):
    """One process per GPU (launched by torch.distributed.run): every rank builds an embedder
    replica and its shard of the store.  Returns the VectorRAG on EVERY rank; a serving
    deployment then calls `rag.collection.start_workers()` on all ranks -- rank 0 comes back and
    serves the MCP / REST surface, the others stay inside answering its searches."""
    import torch
    import torch.distributed as dist
    from .rag import VectorRAG
    from .sharded_store import ShardedCorpusStore
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if not dist.is_initialized():
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group(backend, device_id=dev if backend == "nccl" else None)
    embedder = load_embedder(model_dir, dev, query_prompt, document_prompt, pooling)
    metric_type = store_metric(embedder, metric)
    store = ShardedCorpusStore(collection_name, dim=embedder.dim, device=dev,
                               **({"metric_type": metric_type} if metric_type != "COSINE" else {}))
    ingest_sharded(store, embedder, chunker.build_all_chunks(data_dir))
    # (the serving rank reranks; the others only hold a replica like the embedder's)
    return VectorRAG(None, collection_name, embedder=embedder, store=store, generator=generator,
                     reranker=_load_reranker(reranker_dir, dev), reader=_load_reader(reader_dir, dev, reader_doc_stride))


def build_rag_from_env():
    model_dir = os.getenv("RAGFIN_MODEL_DIR")
    if not model_dir:
        raise RuntimeError("RAGFIN_MODEL_DIR is not set: point it at a local all-MiniLM-L6-v2 "
                           "directory (the reference fetches the model by name; this build never "
                           "touches the network)")
    reranker_dir = os.getenv("RERANKER_MODEL_DIR") or None
    reader_dir = os.getenv("READER_MODEL_DIR") or None
    reader_doc_stride = int(os.environ["READER_DOC_STRIDE"]) if os.getenv("READER_DOC_STRIDE") else None
    sparse_dir = os.getenv("SPARSE_MODEL_DIR") or None
    late_dir = os.getenv("COLBERT_MODEL_DIR") or None
    tagger_dir = os.getenv("TAGGER_MODEL_DIR") or None
    ends = {k: v for k, v in (("query_prompt", os.getenv("RAGFIN_QUERY_PROMPT")),
                              ("document_prompt", os.getenv("RAGFIN_DOCUMENT_PROMPT")),
                              ("pooling", os.getenv("RAGFIN_POOLING")), ("metric", os.getenv("RAGFIN_METRIC"))) if v}
    if int(os.getenv("WORLD_SIZE", "1")) > 1:
        return build_sharded_rag(model_dir, os.getenv("RAGFIN_DATA_DIR", "extract_data"),
                                 int(os.getenv("LOCAL_RANK", "0")), os.getenv("MILVUS_COLLECTION", "fin_chunks"),
                                 reranker_dir=reranker_dir, reader_dir=reader_dir, reader_doc_stride=reader_doc_stride,
                                 **ends)
    return build_rag(model_dir, os.getenv("RAGFIN_DATA_DIR", "extract_data"),
                     os.getenv("RAGFIN_DEVICE", "cuda:0"), os.getenv("MILVUS_COLLECTION", "fin_chunks"),
                     reranker_dir=reranker_dir, hybrid=os.getenv("LEXICAL_INDEX", "0") == "1", reader_dir=reader_dir,
                     reader_doc_stride=reader_doc_stride, **({"sparse_dir": sparse_dir} if sparse_dir else {}),
                     **({"late_dir": late_dir} if late_dir else {}),
                     **({"tagger_dir": tagger_dir, "entity_field": os.getenv("TAGGER_FIELD") or "entities"}
                        if tagger_dir else {}), **ends)
