"""Diversified search (MMR) through the public surface, with fakes (CPU only): validation of
mmr_lambda / mmr_fetch_k in CorpusStore.search, the default fetch_k, what the index receives, the
SQ8 routing, the sharded store's refusal, the two arguments through VectorRAG / the MCP tool / the
REST request, the flagged-query patch path of GpuIndex with a fake device layer, the host-side
argument checks of rf_mmr_select, and the properties of the definition on numpy data."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

from oracle import search as osearch
from rag_fin_amd import _lib, mcp_server
from rag_fin_amd.store import CorpusStore, check_mmr


class FakeIndex:
    """A CPU double of GpuIndex: records the calls a search makes and answers rows 0 .. k-1."""

    def __init__(self, dim=8, capacity=64, device=None):
        self.dim, self.capacity, self.device = dim, capacity, torch.device("cpu")
        self.size = 0
        self.sq8 = False
        self.calls = []

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
        rows = np.tile(np.arange(k, dtype=np.int64), (q16.shape[0], 1))
        return (1.0 - 0.01 * rows).astype(np.float32), rows

    def search_large(self, q16, k, **kw):
        self.calls.append(("large", k, kw))
        s, r = self.search_host(q16, k)
        self.calls.pop()
        return torch.from_numpy(s), torch.from_numpy(r)


def make_store(n=80):
    ix = FakeIndex(capacity=128)
    st = CorpusStore("c", dim=8, capacity=128, index=ix)
    st.add([f"k{i}" for i in range(n)], [f"t{i}" for i in range(n)], np.ones((n, 8), dtype=np.float32),
           [f"Q{i % 4}" for i in range(n)], ["a"] * n, ["s"] * n, [float(i) for i in range(n)])
    return st, ix


Q = np.ones((1, 8), dtype=np.float32)
P = {"metric_type": "COSINE"}


# ---- validation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    {"mmr_fetch_k": 20},                                       # fetch_k without lambda
    {"mmr_lambda": -0.01}, {"mmr_lambda": 1.01}, {"mmr_lambda": float("nan")}, {"mmr_lambda": float("inf")},
    {"mmr_lambda": "0.5"}, {"mmr_lambda": True}, {"mmr_lambda": False}, {"mmr_lambda": 0.5j},
    {"mmr_lambda": 0.5, "mmr_fetch_k": 4},                     # limit 5 > fetch_k
    {"mmr_lambda": 0.5, "mmr_fetch_k": 65},
    {"mmr_lambda": 0.5, "mmr_fetch_k": 20.0}, {"mmr_lambda": 0.5, "mmr_fetch_k": True},
    {"mmr_lambda": 0.5, "group_by_field": "period"},
    {"mmr_lambda": 0.5, "mmr_fetch_k": 20, "group_by_field": "period", "group_size": 2},
])
def test_bad_mmr_arguments_raise_value_error(kw):
    st, ix = make_store()
    with pytest.raises(ValueError, match="diversified search"):
        st.search(Q, "embedding", P, limit=5, **kw)
    assert ix.calls == []


def test_limit_above_64_cannot_be_diversified():
    st, ix = make_store()
    with pytest.raises(ValueError, match="diversified search"):
        st.search(Q, "embedding", P, limit=65, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="limit"):
        st.search(Q, "embedding", P, limit=0, mmr_lambda=0.5)
    assert ix.calls == []


@pytest.mark.parametrize("limit,fetch_k", [(1, 20), (3, 20), (5, 20), (6, 24), (10, 40), (16, 64), (17, 64), (64, 64)])
def test_default_fetch_k(limit, fetch_k):
    assert check_mmr(0.5, None, limit) == (fetch_k, 0.5)
    st, ix = make_store()
    st.search(Q, "embedding", P, limit=limit, mmr_lambda=0.25)
    assert ix.calls[-1] == ("host", limit, {"mmr": (fetch_k, 0.25)})


def test_check_mmr_returns_plain_python_numbers():
    assert check_mmr(None, None, 5) is None
    got = check_mmr(np.float32(0.5), np.int64(30), 5)
    assert got == (30, 0.5) and type(got[0]) is int and type(got[1]) is float
    assert check_mmr(0, 5, 5) == (5, 0.0) and check_mmr(1, 64, 64) == (64, 1.0)


# ---- what the index receives ------------------------------------------------------------------------------
def test_the_index_receives_limit_and_the_mmr_pair():
    st, ix = make_store()
    hits = st.search(Q, "embedding", P, limit=4, mmr_lambda=0.7, mmr_fetch_k=33)
    assert ix.calls[-1] == ("host", 4, {"mmr": (33, 0.7)})
    assert [h.id for h in hits[0]] == ["k0", "k1", "k2", "k3"]
    assert [h.score for h in hits[0]] == [np.float32(1.0 - 0.01 * j) for j in range(4)]   # the relevance score


def test_without_the_arguments_the_call_is_the_call_of_before():
    st, ix = make_store()
    st.search(Q, "embedding", P, limit=5)
    assert ix.calls[-1] == ("host", 5, {})
    st.search(Q, "embedding", P, limit=100)
    assert ix.calls[-1] == ("large", 100, {})
    st.search(Q, "embedding", P, limit=5, mmr_lambda=None, mmr_fetch_k=None)
    assert ix.calls[-1] == ("host", 5, {})
    st.search_rows(Q, 5)
    assert ix.calls[-1] == ("host", 5, {})


def test_filter_and_band_travel_with_the_mmr_pair(monkeypatch):
    st, ix = make_store()
    monkeypatch.setattr(st, "build_filter", lambda expr: "FILTER")
    st.search(Q, "embedding", P, limit=2, expr='chunk_type == "a"', mmr_lambda=0.5)
    assert ix.calls[-1] == ("host", 2, {"filt": "FILTER", "mmr": (20, 0.5)})
    st.search(Q, "embedding", {"metric_type": "COSINE", "params": {"radius": 0.2, "range_filter": 0.9}}, limit=2,
              mmr_lambda=0.5, mmr_fetch_k=30)
    assert ix.calls[-1] == ("host", 2, {"band": (0.2, 0.9), "mmr": (30, 0.5)})
    st.search_rows(Q, 2, mmr=(30, 0.5))
    assert ix.calls[-1] == ("host", 2, {"mmr": (30, 0.5)})
    with pytest.raises(ValueError, match="diversified search"):
        st.search_rows(Q, 31, mmr=(30, 0.5))


def test_sq8_routing_is_still_applied():
    st, ix = make_store()
    st.create_index("embedding", {"index_type": "SQ8", "metric_type": "COSINE"})
    st.search(Q, "embedding", P, limit=3, mmr_lambda=0.5)
    assert ix.calls[-1] == ("host", 3, {"mmr": (20, 0.5), "sq8": True})
    st.search(np.ones((65, 8), dtype=np.float32), "embedding", P, limit=3, mmr_lambda=0.5)   # beyond one sweep: FLAT
    assert ix.calls[-1] == ("host", 3, {"mmr": (20, 0.5)})


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


def test_sharded_store_raises_on_mmr(one_rank_group):
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    st = ShardedCorpusStore("c", dim=8, capacity=4, index=FakeIndex(8, 4), backend=object())
    with pytest.raises(NotImplementedError, match="diversified search"):
        st.search(Q, limit=3, mmr_lambda=0.5)
    with pytest.raises(NotImplementedError, match="diversified search"):
        st.search(Q, limit=3, mmr_fetch_k=20)


# ---- GpuIndex: argument checks and the flagged-query patch path, without a device ------------------------
def bare_index():
    """A GpuIndex without a device: what its search methods use beyond the C library is faked below."""
    import threading
    from rag_fin_amd.index import GpuIndex
    ix = GpuIndex.__new__(GpuIndex)
    ix.handle = None
    ix.device = torch.device("cpu")
    ix.dim = 8
    ix._lock = threading.Lock()
    return ix


@pytest.mark.parametrize("k,mmr", [(5, (4, 0.5)), (0, (4, 0.5)), (5, (65, 0.5)), (5, (20.0, 0.5)), (5, (True, 0.5)),
                                   (5, (20, -0.1)), (5, (20, 1.5)), (5, (20, float("nan"))), (5, (20, "x")),
                                   (5, (20, True))])
def test_check_variant_refuses_bad_mmr(k, mmr):
    with pytest.raises(ValueError, match="diversified search"):
        bare_index()._check_variant(None, False, None, None, k, mmr)


def test_check_variant_allows_filt_band_sq8_and_refuses_group():
    ix = bare_index()
    ix._check_variant("F", False, (0.1, 0.9), None, 5, (20, 0.5))
    ix._check_variant(None, True, None, None, 5, (20, 0.5))
    ix._check_variant(None, False, None, None, 64, (64, 1))
    with pytest.raises(ValueError, match="grouping"):
        ix._check_variant(None, False, None, ("codes", 4, 5, 1), 5, (20, 0.5))


def test_a_flagged_querys_mmr_row_is_replaced_by_a_selection_over_the_ladders_candidates(monkeypatch):
    """The first pass returns an MMR block and flags queries 1 and 3: they get fetch_k candidates
    from the ladder (here: a fake tier) and the MMR stage again; search() returns the patched block."""
    ix = bare_index()
    B, k, fetch_k = 4, 3, 6
    seen = {}

    def search_raw(q16, kk, id_base=0, want_exact=False, out=None, filt=None, sq8=False, band=None, mmr=None, **kw):
        seen["first"] = (kk, mmr, filt, sq8, band)
        return (torch.zeros((B, kk)), torch.full((B, kk), 7, dtype=torch.int64), torch.zeros((B, kk), dtype=torch.float64),
                torch.tensor([0, 2, 0, 1], dtype=torch.int32))

    def exhaustive(q16, kk, id_base=0, want_exact=False, filt=None, after=None, band=None):
        seen["ladder"] = (tuple(q16.shape), kk, want_exact, filt, band)
        n = q16.shape[0]
        ids = torch.arange(100, 100 + kk, dtype=torch.int64).repeat(n, 1) + 1000 * q16[:, :1].long()
        ex = torch.linspace(0.9, 0.4, kk, dtype=torch.float64).repeat(n, 1)
        return ex.float(), ids, ex

    def mmr_select(cand_exact, cand_ids, kk, mmr, id_base, out, stream_ptr=None):
        seen["select"] = (tuple(cand_ids.shape), kk, mmr)
        out[0][:] = cand_exact[:, [0, 2, 4]].float()      # "picks" 0, 2, 4 of the ladder's candidates
        out[1][:] = cand_ids[:, [0, 2, 4]]
        if out[2] is not None:
            out[2][:] = cand_exact[:, [0, 2, 4]]

    monkeypatch.setattr(ix, "search_raw", search_raw)
    monkeypatch.setattr(ix, "_exhaustive", exhaustive)
    monkeypatch.setattr(ix, "_mmr_select", mmr_select)
    q16 = torch.arange(B, dtype=torch.float16)[:, None].repeat(1, 8)
    scores, ids, exact = ix.search(q16, k, want_exact=True, filt="F", band=(0.1, 0.95), mmr=(fetch_k, 0.5))
    assert seen["first"] == (k, (fetch_k, 0.5), "F", False, (0.1, 0.95))
    assert seen["ladder"] == ((2, 8), fetch_k, True, "F", (0.1, 0.95))      # fetch_k candidates, with fp64 scores
    assert seen["select"] == ((2, fetch_k), k, (fetch_k, 0.5))
    assert ids.tolist() == [[7, 7, 7], [1100, 1102, 1104], [7, 7, 7], [3100, 3102, 3104]]
    assert exact[1].tolist() == pytest.approx([0.9, 0.7, 0.5]) and scores[3].tolist() == pytest.approx([0.9, 0.7, 0.5])
    assert exact[0].tolist() == [0.0, 0.0, 0.0]                           # an unflagged row stays as the first pass wrote it


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
    rag.search("q", 4, mmr_lambda=0.5)
    rag.search("q", 4, expr="primary_value > 0", mmr_lambda=0.3, fetch_k=32)
    rag.search_batch(["a", "b"], 2, mmr_lambda=0.0, fetch_k=10)
    rag.search_batch(["a", "b"], 2)
    rag.search("q", 3, min_score=0.2, mmr_lambda=1)
    assert rag.collection.calls == [
        (P, 3, plain),
        (P, 4, dict(plain, mmr_lambda=0.5)),
        (P, 4, dict(plain, expr="primary_value > 0", mmr_lambda=0.3, mmr_fetch_k=32)),
        (P, 2, dict(plain, mmr_lambda=0.0, mmr_fetch_k=10)),
        (P, 2, plain),
        ({"metric_type": "COSINE", "params": {"radius": 0.2}}, 3, dict(plain, mmr_lambda=1))]


def test_contexts_keep_the_relevance_score_in_mmr_order():
    from rag_fin_amd.rag import VectorRAG
    st, ix = make_store()
    rag = VectorRAG("k", embedder=Emb(), store=st)
    st._prepare_queries = lambda data: torch.ones((np.asarray(data).shape[0], 8)).half()
    got = rag.search("hello", top_k=2, mmr_lambda=0.5, fetch_k=9)
    assert ix.calls[-1] == ("host", 2, {"mmr": (9, 0.5)})
    assert [(c["rank"], c["text"], c["score"]) for c in got] == [(1, "t0", 1.0), (2, "t1", float(np.float32(0.99)))]


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


def test_mcp_tool_passes_the_arguments_and_keeps_the_payload(fake_rag):
    r = mcp_server.search_vectors("net interest income trend", 4, mmr_lambda=0.5)
    assert r == {"status": "success", "query": "net interest income trend", "results": [], "result_count": 0}
    assert fake_rag.calls[-1] == ("search", "net interest income trend", 4, None, {"mmr_lambda": 0.5})
    mcp_server.search_vectors("q", 4, filter="primary_value > 0", mmr_lambda=0.3, fetch_k=32)
    assert fake_rag.calls[-1] == ("search", "q", 4, "primary_value > 0", {"mmr_lambda": 0.3, "fetch_k": 32})
    mcp_server.search_vectors("q", 4, min_score=0.2, mmr_lambda=0.3)
    assert fake_rag.calls[-1] == ("search", "q", 4, None, {"min_score": 0.2, "max_score": None, "mmr_lambda": 0.3})
    mcp_server.search_vectors("q", 4, group_by="period", mmr_lambda=0.3)   # (the store refuses the combination)
    assert fake_rag.calls[-1] == ("search", "q", 4, None, {"group_by": "period", "group_size": 1, "mmr_lambda": 0.3})
    mcp_server.search_vectors("q")                                       # the call of before
    assert fake_rag.calls[-1] == ("search", "q", 3, None, {})
    mcp_server.search_vectors("q", 2, filter="id == 1")
    assert fake_rag.calls[-1] == ("search", "q", 2, "id == 1", {})


def test_mcp_tool_reports_a_refused_combination():
    st, ix = make_store()
    from rag_fin_amd.rag import VectorRAG
    mcp_server.set_rag(VectorRAG("k", embedder=Emb(), store=st))
    try:
        st._prepare_queries = lambda data: torch.ones((np.asarray(data).shape[0], 8)).half()
        r = mcp_server.search_vectors("q", 4, mmr_lambda=1.5)
        assert r["status"] == "error" and "mmr_lambda" in r["message"]
        r = mcp_server.search_vectors("q", 4, fetch_k=20)
        assert r["status"] == "error" and "mmr_fetch_k needs mmr_lambda" in r["message"]
    finally:
        mcp_server.set_rag(None)


def test_search_request_payload():
    from rag_fin_amd.adapter import SearchRequest, search_args
    assert search_args(SearchRequest(query="hello", top_k=4)) == {"query": "hello", "top_k": 4}
    assert search_args(SearchRequest(query="hello", mmr_lambda=0.5)) == {"query": "hello", "top_k": 3, "mmr_lambda": 0.5}
    assert search_args(SearchRequest(query="hello", filter="id == 1", mmr_lambda=0.0, fetch_k=40)) == \
        {"query": "hello", "top_k": 3, "filter": "id == 1", "mmr_lambda": 0.0, "fetch_k": 40}
    for bad in ({"mmr_lambda": 1.5}, {"mmr_lambda": -0.1}, {"fetch_k": 0}, {"fetch_k": 65}):
        with pytest.raises(Exception):
            SearchRequest(query="hello", **bad)


# ---- C ABI: host-side argument checks (no GPU needed) ------------------------------------------------------
def test_mmr_abi_argument_checks():
    lib = _lib.load_library()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every case below fails its checks first

    def call(ix=fake, B=1, fetch_k=20, k=5, lam=0.5, ce=fake, ci=fake, sc=fake, ids=fake):
        return lib.rf_mmr_select(ix, B, fetch_k, k, lam, 0, ce, ci, sc, ids, None, None)

    for null in ("ix", "ce", "ci", "sc", "ids"):
        assert call(**{null: None}) == -1 and b"null" in lib.rf_last_error()
    assert call(B=0) == -1 and call(B=-3) == -1
    assert call(k=0) == -1 and call(k=21) == -1 and call(fetch_k=0, k=0) == -1
    assert call(fetch_k=65, k=5) == -1 and call(fetch_k=65, k=65) == -1
    assert b"fetch_k" in lib.rf_last_error()
    for lam in (-0.001, 1.001, float("nan"), float("inf"), -float("inf")):
        assert call(lam=lam) == -1 and b"lambda" in lib.rf_last_error()
    assert _lib.RF_MAX_K == 64


# ---- the definition, on numpy data ------------------------------------------------------------------------------
def mmr_numpy(q16, c16, fetch_k, k, lam):
    """The definition in numpy float64, one operation per statement (the oracle of the GPU test)."""
    cs, ci = osearch.topk_from_scores(osearch.exact_scores(q16, c16), fetch_k)
    out = []
    for b in range(q16.shape[0]):
        rows, s = ci[b][ci[b] >= 0], cs[b][ci[b] >= 0]
        g = osearch.exact_scores(c16[rows], c16[rows])
        assert np.array_equal(g, g.T)                     # symmetric bit for bit
        mu = np.float64(1.0) - np.float64(lam)
        m = np.full(rows.size, -np.inf)
        left = list(range(rows.size))
        picks = []
        for t in range(min(k, rows.size)):
            rel = np.float64(lam) * s
            pen = np.zeros(rows.size) if t == 0 else mu * m
            v = rel - pen
            best = max(left, key=lambda i: (v[i], -i))
            left.remove(best)
            picks.append(best)
            m = np.maximum(m, g[:, best])
        out.append((rows[picks], s[picks], rows))
    return out


@pytest.fixture(scope="module")
def clustered():
    rng = np.random.default_rng(3)
    centres = rng.standard_normal((8, 64))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    c = centres[rng.integers(0, 8, 400)] + 0.15 * rng.standard_normal((400, 64)) / 8.0
    q = centres[rng.integers(0, 8, 4)] + 0.6 * rng.standard_normal((4, 64)) / 8.0
    unit = lambda x: np.ascontiguousarray((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16))  # noqa: E731
    return unit(c), unit(q)


def test_lambda_one_is_the_plain_top_k(clustered):
    c, q = clustered
    ws, wi = osearch.search(q, c, 10)
    for b, (rows, s, _) in enumerate(mmr_numpy(q, c, 32, 10, 1.0)):
        assert np.array_equal(rows, wi[b]) and np.array_equal(s, ws[b])


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.5, 0.7, 1.0])
def test_first_pick_is_the_best_hit_and_the_output_permutes_a_subset_of_the_candidates(clustered, lam):
    c, q = clustered
    _, wi = osearch.search(q, c, 1)
    differ = 0
    for b, (rows, s, cand) in enumerate(mmr_numpy(q, c, 32, 10, lam)):
        assert rows[0] == wi[b, 0]
        assert len(set(rows.tolist())) == 10 and set(rows.tolist()) <= set(cand.tolist())
        differ += int(not np.array_equal(rows, cand[:10]))
    assert lam == 1.0 or differ >= 2
