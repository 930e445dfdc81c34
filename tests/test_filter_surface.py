"""Filtered search through the public surface, with fakes (CPU only): the MCP tool, the REST
request, the micro-batcher, the sharded store, and the host-side argument checks of the new
C-ABI entry points."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

from rag_fin_amd import _lib, filter_expr, mcp_server


class FakeRag:
    """Records how the tool layer calls it; parses filters like the store does."""

    def __init__(self):
        self.calls = []
        self.batches = 0

    def search(self, query, top_k=3, expr=None):
        self.calls.append((query, top_k, expr))
        if not filter_expr.is_empty(expr):
            filter_expr.parse(expr)
        return [{"rank": 1, "text": "t", "period": "Q1_FY2024", "chunk_type": "c", "statement_type": "s",
                 "primary_value": 1.0, "score": 0.5}][:top_k]

    def search_batch(self, queries, top_k=3, expr=None):
        self.batches += 1
        return [self.search(q, top_k, expr) for q in queries]


@pytest.fixture
def fake_rag():
    rag = FakeRag()
    mcp_server.set_rag(rag)
    yield rag
    mcp_server.set_rag(None)


def test_search_vectors_passes_the_filter_as_expr(fake_rag):
    r = mcp_server.search_vectors("net profit Q1", 2, filter='period == "Q1_FY2024"')
    assert r["status"] == "success" and r["result_count"] == 1
    assert set(r) == {"status", "query", "results", "result_count"}
    assert fake_rag.calls[-1] == ("net profit Q1", 2, 'period == "Q1_FY2024"')
    mcp_server.search_vectors("net profit Q1")          # no filter: the call of today
    assert fake_rag.calls[-1] == ("net profit Q1", 3, None)


def test_a_bad_filter_comes_back_as_the_error_dict(fake_rag):
    r = mcp_server.search_vectors("net profit Q1", 3, filter="period > 3")
    assert r["status"] == "error" and r["query"] == "net profit Q1" and "VARCHAR" in r["message"]
    assert set(r) == {"status", "message", "query"}


def test_filtered_calls_bypass_the_micro_batcher(fake_rag, monkeypatch):
    monkeypatch.setenv("RAGFIN_MICROBATCH_MS", "5")
    monkeypatch.setattr(mcp_server, "_batcher", None)
    try:
        assert mcp_server.search_vectors("qqqqq", 1, filter="primary_value > 0")["status"] == "success"
        assert fake_rag.batches == 0 and mcp_server._batcher is None
        assert mcp_server.search_vectors("qqqqq", 1)["status"] == "success"   # unfiltered: batched
        assert fake_rag.batches == 1
    finally:
        if mcp_server._batcher is not None:
            mcp_server._batcher.close()


def test_search_request_payload_unchanged_without_filter():
    from rag_fin_amd.adapter import SearchRequest, search_args
    assert search_args(SearchRequest(query="hello", top_k=4)) == {"query": "hello", "top_k": 4}
    assert search_args(SearchRequest(query="hello", filter='period == "Q1"')) == \
        {"query": "hello", "top_k": 3, "filter": 'period == "Q1"'}


def test_vector_rag_hands_expr_to_the_store():
    from rag_fin_amd.rag import VectorRAG

    class Store:
        num_entities = 0

        def __init__(self):
            self.exprs = []

        def load(self):
            pass

        def search(self, data, anns_field, param, limit, expr=None, output_fields=None):
            self.exprs.append(expr)
            return [[] for _ in range(np.asarray(data).shape[0])]

    class Emb:
        def encode(self, texts):
            return np.zeros((len(texts), 4), dtype=np.float32)

    rag = VectorRAG("k", embedder=Emb(), store=Store())
    rag.search("q", 3, expr="id == 1")
    rag.search_batch(["a", "b"], 2, expr="id == 2")
    rag.search("q")
    assert rag.collection.exprs == ["id == 1", "id == 2", None]


# ---- the sharded store keeps refusing filters ------------------------------------------------------
@pytest.fixture
def one_rank_group():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


class _Index:
    def __init__(self, dim, capacity, device=None):
        self.dim, self.capacity, self.device = dim, capacity, torch.device("cpu")
        self.size = 0


def test_sharded_store_raises_on_filters(one_rank_group):
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    st = ShardedCorpusStore("c", dim=16, capacity=4, index=_Index(16, 4), backend=object())
    q = np.ones((1, 16), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="sharded"):
        st.search(q, limit=3, expr='period == "Q1_FY2024"')
    with pytest.raises(NotImplementedError):
        st.query(expr='period == "Q1_FY2024"')
    assert st.query(expr="") == [] and st.query(expr='id in ["x"]') == []


# ---- C ABI: host-side argument checks (no GPU needed) ------------------------------------------------
def test_filter_abi_argument_checks():
    lib = _lib.load_library()
    assert lib.rf_filter_bytes(-1) == 0 and lib.rf_filter_bytes(1 << 33) == 0
    assert lib.rf_filter_bytes(0) == 16 + 2 * 4 * 1024
    assert lib.rf_filter_bytes(1_000_000) == 16 + 2 * 125_008 + 2 * 4 * 1024   # two 31 250-word arrays, 16-byte aligned
    # the sizes at which the tile plan changes regime (tests/test_filter_scale_gpu.py): header, two
    # nblk-word arrays padded to 16 bytes, then {blocks, rows} counts of 1024 tiles whatever the plan is
    for n in (1_048_576, 1_048_577, 8_388_641, 33_554_465):
        nblk = (n + 31) // 32
        assert lib.rf_filter_bytes(n) == 16 + 2 * ((4 * nblk + 15) // 16 * 16) + 2 * 4 * 1024
    assert lib.rf_filter_bytes(1_048_577) == 16 + 2 * 131_088 + 8192 and lib.rf_filter_bytes(33_554_465) == 16 + 2 * 4_194_320 + 8192
    fake = ctypes.c_void_p(4096)    # never dereferenced: every case below fails its checks first
    cols = (ctypes.c_void_p * 4)(4096, 4096, 4096, 8192)

    def prog(*ops):
        arr = (_lib.FilterOp * max(len(ops), 1))()
        for i, o in enumerate(ops):
            arr[i].op, arr[i].column, arr[i].len = o   # (opcode, column, len)
        return arr

    T, A, N, C = _lib.RF_FOP_TRUE, _lib.RF_FOP_AND, _lib.RF_FOP_NOT, _lib.RF_FOP_CODESET
    ok1 = prog((T, 0, 0))
    assert lib.rf_filter_eval(None, 1, None, None, cols, 10, fake, None) == -1            # null program
    assert lib.rf_filter_eval(ok1, 1, None, None, None, 10, fake, None) == -1             # null column table
    assert lib.rf_filter_eval(ok1, 1, None, None, cols, 10, None, None) == -1             # null buffer
    assert lib.rf_filter_eval(ok1, 1, None, None, cols, 10, ctypes.c_void_p(4100), None) == -1   # misaligned
    assert lib.rf_filter_eval(ok1, 0, None, None, cols, 10, fake, None) == -1             # no ops
    many = prog(*[(T, 0, 0)] + [(N, 0, 0)] * _lib.RF_FILTER_MAX_OPS)
    assert lib.rf_filter_eval(many, _lib.RF_FILTER_MAX_OPS + 1, None, None, cols, 10, fake, None) == -1
    deep = prog(*[(T, 0, 0)] * (_lib.RF_FILTER_MAX_DEPTH + 1))          # one push too many
    assert lib.rf_filter_eval(deep, _lib.RF_FILTER_MAX_DEPTH + 1, None, None, cols, 10, fake, None) == -1
    assert b"depth" in lib.rf_last_error()
    assert lib.rf_filter_eval(prog((A, 0, 0)), 1, None, None, cols, 10, fake, None) == -1        # underflow
    assert lib.rf_filter_eval(prog((T, 0, 0), (T, 0, 0)), 2, None, None, cols, 10, fake, None) == -1   # leaves 2
    assert lib.rf_filter_eval(prog((99, 0, 0)), 1, None, None, cols, 10, fake, None) == -1       # opcode
    assert lib.rf_filter_eval(prog((C, 5, 1)), 1, fake, None, cols, 10, fake, None) == -1        # column
    assert lib.rf_filter_eval(prog((C, 0, 1)), 1, None, None, cols, 10, fake, None) == -1        # no code sets
    assert lib.rf_filter_eval(prog((_lib.RF_FOP_RANGE, 0, 0)), 1, None, None, cols, 10, fake, None) == -1
    assert lib.rf_filter_eval(prog((_lib.RF_FOP_ROWLIST, 0, 2)), 1, None, None, cols, 10, fake, None) == -1
    assert lib.rf_filter_eval(ok1, 1, None, None, cols, -1, fake, None) == -1             # n_rows
    assert lib.rf_filter_from_mask(None, 10, fake, None) == -1
    assert lib.rf_filter_from_mask(fake, 10, None, None) == -1
    assert lib.rf_search_filtered(None, fake, fake, 1, 10, 0, fake, fake, None, fake, fake, 1 << 30, None) == -1
    assert lib.rf_search_exhaustive_filtered(None, None, fake, 1, 10, 0, None, None, fake, fake, None, fake,
                                             1 << 30, None) == -1
    assert lib.rf_search_exhaustive_filtered(None, fake, fake, 1, 10, 0, fake, None, fake, fake, None, fake,
                                             1 << 30, None) == -1   # one bound array without the other
