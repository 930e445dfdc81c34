"""Grouping search through the public surface, with fakes (CPU only): validation of group_by_field /
group_size in CorpusStore.search, what the index receives, the routing of "id" and of an SQ8
collection, the marshalling of the padded slot block into flat hit lists, the sharded store's
refusal, the two arguments through VectorRAG / the MCP tool / the REST request, and the host-side
argument checks of rf_search_grouped."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

from rag_fin_amd import _lib, mcp_server
from rag_fin_amd.store import CorpusStore

PERIODS = ["Q1", "Q2", "Q3", "Q1", "Q2", "Q3", "Q1", "Q4"]
KINDS = ["a", "a", "a", "a", "b", "b", "b", "b"]


class FakeIndex:
    """A CPU double of GpuIndex: records the calls a search makes and returns the block it was given."""

    def __init__(self, dim=8, capacity=64, device=None):
        self.dim, self.capacity, self.device = dim, capacity, torch.device("cpu")
        self.size = 0
        self.sq8 = False
        self.calls = []
        self.block = None      # rows [B, k] to answer with (scores: 1 - 0.01 * slot)

    def add(self, rows):
        self.size += rows.shape[0]

    def to_fp16(self, x, normalize=True):
        return torch.as_tensor(np.asarray(x, dtype=np.float32)).half()

    def enable_sq8(self):
        self.sq8 = True

    def disable_sq8(self):
        self.sq8 = False

    def search_host(self, q16, k, **kw):
        self.calls.append(("host", k, kw))
        B = q16.shape[0]
        rows = np.full((B, k), -1, dtype=np.int64) if self.block is None else np.asarray(self.block, dtype=np.int64)
        scores = np.where(rows >= 0, 1.0 - 0.01 * np.arange(k)[None, :], -np.inf).astype(np.float32)
        return scores, rows

    def search_large(self, q16, k, **kw):
        self.calls.append(("large", k, kw))
        s, r = self.search_host(q16, k)
        self.calls.pop()
        return torch.from_numpy(s), torch.from_numpy(r)


def make_store():
    ix = FakeIndex()
    st = CorpusStore("c", dim=8, capacity=64, index=ix)
    n = len(PERIODS)
    st.add([f"k{i}" for i in range(n)], [f"t{i}" for i in range(n)], np.ones((n, 8), dtype=np.float32), PERIODS, KINDS,
           ["s"] * n, [float(i) for i in range(n)])
    return st, ix


Q = np.ones((1, 8), dtype=np.float32)
P = {"metric_type": "COSINE"}


# ---- validation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    {"group_by_field": "text"}, {"group_by_field": "embedding"}, {"group_by_field": "primary_value"},
    {"group_by_field": "nope"}, {"group_by_field": ""},
    {"group_by_field": "period", "group_size": 0}, {"group_by_field": "period", "group_size": -1},
    {"group_by_field": "period", "group_size": 1.5}, {"group_by_field": "period", "group_size": True},
    {"group_by_field": "id", "group_size": 0},
    {"group_by_field": "period", "group_size": 13},            # 5 * 13 = 65 > 64
])
def test_bad_grouping_arguments_raise_value_error(kw):
    st, ix = make_store()
    with pytest.raises(ValueError, match="group"):
        st.search(Q, "embedding", P, limit=5, **kw)
    assert ix.calls == []


def test_limit_times_group_size_is_capped_at_64():
    st, ix = make_store()
    st.search(Q, "embedding", P, limit=16, group_by_field="period", group_size=4)
    assert ix.calls[-1][1] == 64
    with pytest.raises(ValueError, match="64"):
        st.search(Q, "embedding", P, limit=65, group_by_field="period")
    with pytest.raises(ValueError, match="64"):
        st.search(Q, "embedding", P, limit=17, group_by_field="period", group_size=4)


@pytest.mark.parametrize("params", [{"radius": 0.4}, {"radius": 0.1, "range_filter": 0.5}])
def test_grouping_with_range_parameters_raises(params):
    st, ix = make_store()
    with pytest.raises(ValueError, match="range"):
        st.search(Q, "embedding", {"metric_type": "COSINE", "params": params}, limit=3, group_by_field="period")
    assert ix.calls == []
    st.search(Q, "embedding", {"metric_type": "COSINE", "params": {"nprobe": 8}}, limit=3, group_by_field="period")
    assert len(ix.calls) == 1


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


def test_sharded_store_raises_on_group_by_field(one_rank_group):
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    st = ShardedCorpusStore("c", dim=8, capacity=4, index=FakeIndex(8, 4), backend=object())
    with pytest.raises(NotImplementedError, match="grouping search"):
        st.search(Q, limit=3, group_by_field="period")


# ---- what the index receives ------------------------------------------------------------------------------
@pytest.mark.parametrize("field,column", [("period", PERIODS), ("chunk_type", KINDS), ("statement_type", ["s"] * 8)])
def test_the_index_receives_codes_dictionary_size_limit_and_group_size(field, column):
    st, ix = make_store()
    st.search(Q, "embedding", P, limit=3, group_by_field=field, group_size=2, strict_group_size=True)
    kind, k, kw = ix.calls[-1]
    assert (kind, k) == ("host", 6) and set(kw) == {"group"}
    codes, n_codes, limit, gsize = kw["group"]
    values = list(dict.fromkeys(column))
    assert codes.dtype == torch.int32 and codes.is_contiguous()
    assert codes.tolist() == [values.index(v) for v in column]
    assert (n_codes, limit, gsize) == (len(values), 3, 2)


def test_without_the_argument_the_call_is_the_call_of_before():
    st, ix = make_store()
    st.search(Q, "embedding", P, limit=5)
    assert ix.calls[-1] == ("host", 5, {})
    st.search(Q, "embedding", P, limit=100)
    assert ix.calls[-1] == ("large", 100, {})
    st.search(Q, "embedding", P, limit=5, group_size=7, strict_group_size=True)   # ignored without a field
    assert ix.calls[-1] == ("host", 5, {})


def test_id_routes_to_the_plain_search():
    st, ix = make_store()
    ix.block = [[3, 1, -1, -1, -1]]
    hits = st.search(Q, "embedding", P, limit=5, group_by_field="id", group_size=3)
    assert ix.calls[-1] == ("host", 5, {})
    assert [h.id for h in hits[0]] == ["k3", "k1"]
    ix.block = None
    st.search(Q, "embedding", P, limit=100, group_by_field="id")
    assert ix.calls[-1] == ("large", 100, {})


def test_filter_travels_with_the_grouping(monkeypatch):
    st, ix = make_store()
    monkeypatch.setattr(st, "build_filter", lambda expr: "FILTER")
    st.search(Q, "embedding", P, limit=2, expr='chunk_type == "a"', group_by_field="period")
    kind, k, kw = ix.calls[-1]
    assert (kind, k) == ("host", 2) and kw["filt"] == "FILTER" and set(kw) == {"filt", "group"}


def test_sq8_collection_routes_a_grouping_search_to_fp16_and_stays_sq8():
    st, ix = make_store()
    st.create_index("embedding", {"index_type": "SQ8", "metric_type": "COSINE"})
    st.search(Q, "embedding", P, limit=3)
    assert ix.calls[-1] == ("host", 3, {"sq8": True})
    st.search(Q, "embedding", P, limit=3, group_by_field="period")
    assert set(ix.calls[-1][2]) == {"group"}
    assert st.index_type == "SQ8" and ix.sq8


# ---- marshalling ---------------------------------------------------------------------------------------------
def test_the_padded_block_becomes_flat_hit_lists_with_the_group_value():
    st, ix = make_store()
    # limit 3, group_size 3: Q1 has three rows, Q4 one (short group), the third group is missing;
    # the second query finds nothing
    ix.block = [[0, 6, 3, 7, -1, -1, -1, -1, -1], [-1] * 9]
    res = st.search(np.ones((2, 8), dtype=np.float32), "embedding", P, limit=3, group_by_field="period", group_size=3)
    assert [h.id for h in res[0]] == ["k0", "k6", "k3", "k7"] and res[1] == []
    assert [h.entity.get("period") for h in res[0]] == ["Q1", "Q1", "Q1", "Q4"]
    assert [h.entity.period for h in res[0]] == ["Q1", "Q1", "Q1", "Q4"]
    assert [h.score for h in res[0]] == [np.float32(1.0 - 0.01 * j) for j in (0, 1, 2, 3)]
    assert res[0][0].entity.get("text") is None                      # only the group field was added
    res = st.search(Q, "embedding", P, limit=3, group_by_field="chunk_type", group_size=3,
                    output_fields=["text", "chunk_type"])
    ix.block = None
    assert res[0][3].entity.to_dict() == {"text": "t7", "chunk_type": "b"}


# ---- VectorRAG, the MCP tool, the REST request ---------------------------------------------------------------
class RecStore:
    num_entities = 0

    def __init__(self):
        self.calls = []

    def load(self):
        pass

    def search(self, data, anns_field, param, limit, **kw):
        self.calls.append((param, limit, kw))
        return [[] for _ in range(np.asarray(data).shape[0])]


class Emb:
    def encode(self, texts):
        return np.zeros((len(texts), 4), dtype=np.float32)


def test_vector_rag_carries_the_two_arguments():
    from rag_fin_amd.rag import OUTPUT_FIELDS, VectorRAG
    rag = VectorRAG("k", embedder=Emb(), store=RecStore())
    plain = {"expr": None, "output_fields": OUTPUT_FIELDS}
    rag.search("q", 3)
    rag.search("q", 4, group_by="period")
    rag.search("q", 4, expr="primary_value > 0", group_by="chunk_type", group_size=2)
    rag.search_batch(["a", "b"], 2, group_by="period", group_size=3)
    rag.search_batch(["a", "b"], 2)
    rag.search("q", 3, group_size=5)                                   # no field: the call of before
    assert rag.collection.calls == [
        (P, 3, plain),
        (P, 4, dict(plain, group_by_field="period", group_size=1)),
        (P, 4, dict(plain, expr="primary_value > 0", group_by_field="chunk_type", group_size=2)),
        (P, 2, dict(plain, group_by_field="period", group_size=3)),
        (P, 2, plain),
        (P, 3, plain)]


def test_contexts_rank_the_flat_list_and_carry_the_group_value():
    from rag_fin_amd.rag import VectorRAG
    st, ix = make_store()
    ix.block = [[0, 6, 7, -1]]
    rag = VectorRAG("k", embedder=Emb(), store=st)
    st._prepare_queries = lambda data: torch.ones((np.asarray(data).shape[0], 8)).half()
    got = rag.search("hello", top_k=2, group_by="period", group_size=2)
    assert [(c["rank"], c["period"], c["text"]) for c in got] == [(1, "Q1", "t0"), (2, "Q1", "t6"), (3, "Q4", "t7")]
    assert set(got[0]) == {"rank", "text", "period", "chunk_type", "statement_type", "primary_value", "score"}


class FakeRag:
    def __init__(self):
        self.calls = []

    def search(self, query, top_k=3, expr=None, **kw):
        self.calls.append(("search", query, top_k, expr, kw))
        return []


@pytest.fixture
def fake_rag():
    rag = FakeRag()
    mcp_server.set_rag(rag)
    yield rag
    mcp_server.set_rag(None)


def test_mcp_tool_passes_the_grouping_and_keeps_the_payload(fake_rag):
    r = mcp_server.search_vectors("net profit over the year", 4, group_by="period")
    assert r == {"status": "success", "query": "net profit over the year", "results": [], "result_count": 0}
    assert fake_rag.calls[-1] == ("search", "net profit over the year", 4, None, {"group_by": "period", "group_size": 1})
    mcp_server.search_vectors("net profit over the year", 4, filter="primary_value > 0", group_by="period", group_size=2)
    assert fake_rag.calls[-1] == ("search", "net profit over the year", 4, "primary_value > 0",
                                  {"group_by": "period", "group_size": 2})
    mcp_server.search_vectors("net profit over the year")              # the call of before
    assert fake_rag.calls[-1] == ("search", "net profit over the year", 3, None, {})
    mcp_server.search_vectors("net profit over the year", 2, group_size=4)   # no field: the call of before
    assert fake_rag.calls[-1] == ("search", "net profit over the year", 2, None, {})


def test_search_request_payload():
    from rag_fin_amd.adapter import SearchRequest, search_args
    assert search_args(SearchRequest(query="hello", top_k=4)) == {"query": "hello", "top_k": 4}
    assert search_args(SearchRequest(query="hello", group_by="period")) == {"query": "hello", "top_k": 3, "group_by": "period"}
    assert search_args(SearchRequest(query="hello", filter="id == 1", group_by="period", group_size=2)) == \
        {"query": "hello", "top_k": 3, "filter": "id == 1", "group_by": "period", "group_size": 2}
    with pytest.raises(Exception):
        SearchRequest(query="hello", group_size=0)


# ---- C ABI: host-side argument checks (no GPU needed) ------------------------------------------------------
def test_grouped_abi_argument_checks():
    lib = _lib.load_library()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every case below fails its checks first
    big = 1 << 30

    def call(ix=None, filt=None, codes=fake, n_codes=4, n=4, s=1):
        return lib.rf_search_grouped(ix, filt, codes, n_codes, fake, 1, n, s, 0, fake, fake, None, fake, fake, big, None)

    assert call(codes=None) == -1 and b"codes" in lib.rf_last_error()
    assert call(s=0) == -1 and call(n=0) == -1 and call(n_codes=0) == -1
    assert call(n=13, s=5) == -1                       # 65 slots
    assert call(n=64, s=1) == -1                       # valid shape, null index
    assert _lib.RF_GROUP_MAX_CODES >= 64 and _lib.RF_MAX_K == 64
    assert lib.rf_search_grouped_workspace_bytes(None) > lib.rf_search_sq8_workspace_bytes(None)
    assert lib.rf_debug_grouped_counters_offset() % 256 == 0


def test_a_dictionary_above_the_cap_is_unsupported():
    lib = _lib.load_library()
    fake = ctypes.c_void_p(4096)
    rc = lib.rf_search_grouped(None, None, fake, _lib.RF_GROUP_MAX_CODES + 1, fake, 1, 4, 1, 0, fake, fake, None, fake,
                               fake, 1 << 30, None)
    assert rc == -2 and b"n_codes" in lib.rf_last_error()
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "ragfin.h")) as f:
        assert f"#define RF_GROUP_MAX_CODES {_lib.RF_GROUP_MAX_CODES}" in f.read()
