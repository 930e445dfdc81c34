"""Lexical and hybrid search through the public surface, with fakes (CPU only): the sparse index's
life cycle in CorpusStore (create / has / drop, lazy build, invalidation by every mutation, save and
load), the validation of every new argument in CorpusStore.search / hybrid_search, VectorRAG, the MCP
tool and the REST request, what the arms and the fusion stage receive, the sharded store's refusals,
and the host-side argument checks of rf_sparse_* and rf_fuse_rrf.

The device layer is replaced by doubles that compute the definitions of rag_fin_amd/lexical.py:
FakeSparse (bm25_reference) for SparseIndex and fake_fuse (rrf_reference) for fuse_rrf."""
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch

from rag_fin_amd import _lib, filter_expr, lexical, mcp_server
from rag_fin_amd import store as store_mod
from rag_fin_amd import text_fields
from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker, WeightedRanker
from rag_fin_amd.store import SCALAR_FIELDS, CorpusStore

GOLD_STORE = os.path.join(os.path.dirname(__file__), "golden", "store_v1")
SPARSE = {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"}
BM25 = {"metric_type": "BM25"}
COS = {"metric_type": "COSINE"}


# ---- doubles ------------------------------------------------------------------------------------------
class FakeIndex:
    """A CPU double of GpuIndex: the dense arm answers rows n-1, n-2, .. (so that it differs from BM25)."""

    def __init__(self, dim=8, capacity=64, device=None):
        self.dim, self.capacity, self.device = dim, capacity, torch.device("cpu")
        self.size = 0
        self.sq8 = False
        self.calls = []

    def add(self, rows):
        self.size += rows.shape[0]

    def reset(self):
        self.size = 0

    def enable_sq8(self):
        self.sq8 = True

    def disable_sq8(self):
        self.sq8 = False

    def compact(self, keep, window_rows=None):
        self.size = len(keep)

    def to_fp16(self, x, normalize=True):
        return torch.as_tensor(np.asarray(x, dtype=np.float32)).half()

    def get_rows(self, ids):
        return torch.zeros((len(ids), self.dim), dtype=torch.float16)

    def search(self, q16, k, **kw):
        self.calls.append(("search", k, kw))
        B = q16.shape[0]
        rows = torch.full((B, k), -1, dtype=torch.int64)
        n = min(k, self.size)
        rows[:, :n] = torch.arange(self.size - 1, self.size - 1 - n, -1)
        return torch.zeros((B, k)), rows, None

    def search_host(self, q16, k, **kw):
        self.calls.append(("host", k, kw))
        _, rows, _ = self.search(q16, k)
        self.calls.pop()
        return np.zeros(rows.shape, dtype=np.float32), rows.numpy()


class FakeSparse:
    """SparseIndex without a device: the numpy definition."""
    built = []

    def __init__(self, postings, device=None):
        self.postings = postings
        self.calls = []
        FakeSparse.built.append(self)

    def search(self, q_off, q_term, q_weight, k, id_base=0, filt=None, want_exact=True):
        self.calls.append((k, filt))
        mask = None if filt is None else np.asarray(filt, dtype=bool)
        s, i, e = lexical.bm25_reference(self.postings, q_off, q_term, q_weight, k, mask=mask, id_base=id_base)
        return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(e) if want_exact else None


FUSE_CALLS = []


def fake_fuse(arm_ids, k, weights=None, rrf_k=60.0):
    FUSE_CALLS.append((tuple(arm_ids.shape), k, weights, rrf_k))
    s, i, f = lexical.rrf_reference(arm_ids.numpy(), k, rrf_k, weights)
    return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(f)


@pytest.fixture(autouse=True)
def doubles(monkeypatch):
    monkeypatch.setattr(text_fields, "SparseIndex", FakeSparse)
    monkeypatch.setattr(store_mod, "fuse_rrf", fake_fuse)
    FakeSparse.built.clear()
    FUSE_CALLS.clear()


TEXTS = ["basic eps was 15.22 in q1", "diluted eps was 14.90", "net profit rose in q1", "net interest income grew",
         "total deposits grew", "advances grew faster", "capital ratio tier one", "eps eps eps", "q2 profit fell",
         "nothing else here"]


class HostStore(CorpusStore):
    """CorpusStore whose delete(expr) evaluates the expression with the parser's host semantics
    (rf_filter_eval is the GPU tests')."""

    def _match_mask(self, expr):
        node = filter_expr.parse(expr)
        return np.array([node.eval({f: self.columns[f][r] for f in SCALAR_FIELDS})
                         for r in range(self.num_entities)], dtype=bool)


def make_store(texts=TEXTS, sparse=True, cls=HostStore):
    n = len(texts)
    st = cls("c", dim=8, capacity=64, index=FakeIndex(capacity=64))
    st.add([f"k{i}" for i in range(n)], list(texts), np.ones((n, 8), dtype=np.float32), [f"Q{i % 2}" for i in range(n)],
           ["a"] * n, ["s"] * n, [float(i) for i in range(n)])
    if sparse:
        st.create_index("sparse", SPARSE)
    return st


Q = np.ones((2, 8), dtype=np.float32)


# ---- the sparse index: declared, built lazily, invalidated -----------------------------------------------
def test_create_has_drop_index_learn_the_sparse_field():
    st = make_store(sparse=False)
    assert not st.has_index() and not st.has_index(field_name="sparse")
    st.create_index("sparse", dict(SPARSE, params={"bm25_k1": 0.9, "bm25_b": 0.4}))
    assert st.has_index(field_name="sparse") and st.has_index(index_name="sparse")
    assert not st.has_index() and st.index_type == "FLAT" and st._index_params is None       # the vector index is untouched
    assert st._lexical.params == {"bm25_k1": 0.9, "bm25_b": 0.4}
    st.create_index("embedding", {"index_type": "FLAT", "metric_type": "COSINE"})
    st.drop_index()                                                                          # as before: the vector index
    assert not st.has_index() and st.has_index(field_name="sparse")
    st.drop_index(field_name="sparse")
    assert not st.has_index(field_name="sparse")
    st.create_index("sparse")                                                                # defaults
    assert st._lexical.params == {"bm25_k1": 1.2, "bm25_b": 0.75}


@pytest.mark.parametrize("params", [
    {"index_type": "FLAT", "metric_type": "BM25"}, {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "COSINE"},
    dict(SPARSE, params=[1.2]), dict(SPARSE, params={"bm25_k1": -1}), dict(SPARSE, params={"bm25_b": 1.5}),
    dict(SPARSE, params={"bm25_k1": "x"}), dict(SPARSE, params={"bm25_b": float("nan")}),
])
def test_bad_sparse_index_parameters_raise(params):
    st = make_store(sparse=False)
    with pytest.raises(ValueError):
        st.create_index("sparse", params)
    assert not st.has_index(field_name="sparse")
    with pytest.raises(ValueError, match="unknown vector field"):
        st.create_index("text", SPARSE)


def test_the_index_is_built_by_the_first_search_and_rebuilt_after_every_mutation():
    st = make_store()
    assert FakeSparse.built == []                                     # declared, not built
    hits = st.search(["eps"], "sparse", BM25, limit=5)
    assert len(FakeSparse.built) == 1 and FakeSparse.built[0].postings.n_rows == 10
    assert sorted(h.id for h in hits[0]) == ["k0", "k1", "k7"]
    st.search(["eps", "profit"], "sparse", BM25, limit=5)
    assert len(FakeSparse.built) == 1                                 # reused while nothing changes
    n_built = 1
    mutations = [
        lambda: st.add(["n1"], ["fresh eps row"], np.ones((1, 8), dtype=np.float32), ["Q0"], ["a"], ["s"], [1.0]),
        lambda: st.insert([["n2"], ["another eps row"], np.ones((1, 8), dtype=np.float32), ["Q0"], ["a"], ["s"], [1.0]]),
        lambda: st.upsert([["k1"], ["restated: no such word"], np.ones((1, 8), dtype=np.float32), ["Q0"], ["a"], ["s"], [1.0]]),
        lambda: st.delete('id in ["k7"]'),
    ]
    want = [["k0", "k1", "k7", "n1"], ["k0", "k1", "k7", "n1", "n2"], ["k0", "k7", "n1", "n2"], ["k0", "n1", "n2"]]
    for mutate, ids in zip(mutations, want):
        mutate()
        assert st._lexical.built is None
        hits = st.search(["eps"], "sparse", BM25, limit=10)
        n_built += 1
        assert len(FakeSparse.built) == n_built
        assert FakeSparse.built[-1].postings.n_rows == st.num_entities
        assert sorted(h.id for h in hits[0]) == ids
    st.delete('id in ["absent"]')                                     # matches nothing: nothing changes
    st.search(["eps"], "sparse", BM25, limit=10)
    assert len(FakeSparse.built) == n_built
    st.create_index("sparse", dict(SPARSE, params={"bm25_b": 0.0}))   # new parameters: rebuilt
    st.search(["eps"], "sparse", BM25, limit=10)
    assert len(FakeSparse.built) == n_built + 1 and FakeSparse.built[-1].postings.b == 0.0
    st.drop()
    assert st._lexical.built is None and st.has_index(field_name="sparse")
    assert st.search(["eps"], "sparse", BM25, limit=10) == [[]]


def test_bm25_search_results(monkeypatch):
    st = make_store()
    hits = st.search(["eps", "zzz unknown", "net profit"], "sparse", BM25, limit=3, output_fields=["text", "period"])
    p = lexical.build_postings(TEXTS)
    ws, wi, _ = lexical.bm25_reference(p, *lexical.encode_queries(p, ["eps", "zzz unknown", "net profit"]), 3)
    assert [[h.row for h in q] for q in hits] == [[i for i in r.tolist() if i >= 0] for r in wi]
    assert hits[1] == [] and len(hits[0]) == 3 and len(hits[2]) == 3
    assert hits[0][0].id == "k7" and hits[0][0].score == float(ws[0, 0]) and hits[0][0].entity.text == "eps eps eps"
    assert hits[0][0].distance == hits[0][0].score and hits[0][0].entity.get("period") == "Q1"
    assert len(st.search("eps", "sparse", BM25, limit=64)[0]) == 3                # one string is one query; a short list
    # expr: the filter buffer travels to the sparse index
    monkeypatch.setattr(st, "build_filter", lambda expr: np.arange(10) != 7)
    hits = st.search(["eps"], "sparse", BM25, limit=3, expr='period == "Q0"')
    assert FakeSparse.built[-1].calls[-1][1] is not None and sorted(h.id for h in hits[0]) == ["k0", "k1"]
    with pytest.raises(KeyError):
        st.search(["eps"], "sparse", BM25, limit=3, output_fields=["nope"])


def test_a_corpus_without_terms_answers_empty_lists():
    st = make_store(texts=["", "   "])
    assert st.search(["eps", "x"], "sparse", BM25, limit=3) == [[], []]
    assert FakeSparse.built == []
    hits = st.hybrid_search([AnnSearchRequest(Q, "embedding", COS, 2), AnnSearchRequest(["a", "b"], "sparse", BM25, 2)],
                            RRFRanker(), limit=2)
    assert [[h.id for h in q] for q in hits] == [["k1", "k0"], ["k1", "k0"]]      # the dense arm alone


@pytest.mark.parametrize("call", [
    lambda st: st.search(Q, "sparse", BM25, limit=3),                                         # vectors for "sparse"
    lambda st: st.search([[0.0] * 8], "sparse", BM25, limit=3),
    lambda st: st.search(["eps"], "embedding", COS, limit=3),                                  # strings for "embedding"
    lambda st: st.search("eps", "embedding", COS, limit=3),
    lambda st: st.search(["eps"], "sparse", COS, limit=3),                                     # metric
    lambda st: st.search(["eps"], "sparse", BM25, limit=65),
    lambda st: st.search(["eps"], "sparse", BM25, limit=0),
    lambda st: st.search(["eps"], "sparse", BM25, limit=True),
    lambda st: st.search(["eps"], "sparse", {"metric_type": "BM25", "params": {"radius": 1.0}}, limit=3),
    lambda st: st.search(["eps"], "sparse", {"metric_type": "BM25", "params": {"range_filter": 1.0}}, limit=3),
    lambda st: st.search(["eps"], "sparse", {"metric_type": "BM25", "params": 3}, limit=3),
    lambda st: st.search(["eps"], "sparse", BM25, limit=3, group_by_field="period"),
    lambda st: st.search(["eps"], "sparse", BM25, limit=3, mmr_lambda=0.5),
    lambda st: st.search(["eps"], "sparse", BM25, limit=3, mmr_fetch_k=20),
    lambda st: st.search(["eps"], "sparse2", BM25, limit=3),
    lambda st: st.search([" ".join(f"t{i}" for i in range(70))], "sparse", BM25, limit=3),    # > 64 distinct known terms
])
def test_bad_sparse_search_arguments_raise_value_error(call):
    st = make_store(texts=TEXTS + [" ".join(f"t{i}" for i in range(70))])
    with pytest.raises(ValueError):
        call(st)
    assert st.index.calls == []


def test_a_missing_sparse_index_raises():
    st = make_store(sparse=False)
    with pytest.raises(ValueError, match="no sparse index"):
        st.search(["eps"], "sparse", BM25, limit=3)
    with pytest.raises(ValueError, match="no sparse index"):
        st.hybrid_search([AnnSearchRequest(["eps"], "sparse", BM25, 3)], RRFRanker(), limit=3)


# ---- hybrid_search ------------------------------------------------------------------------------------
def test_hybrid_search_fuses_the_two_arms(monkeypatch):
    st = make_store()
    reqs = [AnnSearchRequest(Q, "embedding", COS, limit=4), AnnSearchRequest(["eps", "net profit"], "sparse", BM25, limit=6)]
    hits = st.hybrid_search(reqs, RRFRanker(), limit=5, output_fields=["text"])
    assert st.index.calls == [("search", 4, {})]
    assert FakeSparse.built[-1].calls == [(6, None)]
    assert FUSE_CALLS == [((2, 2, 6), 5, [1.0, 1.0], 60.0)]                       # padded to the widest arm
    p = lexical.build_postings(TEXTS)
    _, sparse_ids, _ = lexical.bm25_reference(p, *lexical.encode_queries(p, ["eps", "net profit"]), 6)
    dense_ids = np.array([[9, 8, 7, 6, -1, -1]] * 2)
    _, wi, wf = lexical.rrf_reference(np.stack([dense_ids, sparse_ids]), 5)
    assert [[h.row for h in q] for q in hits] == [[i for i in r.tolist() if i >= 0] for r in wi]
    assert [[h.score for h in q] for q in hits] == [[f for f in r.tolist() if f > 0] for r in wf]
    assert hits[0][0].id == "k7" and hits[0][0].entity.text == "eps eps eps"      # in both arms: first
    assert hits[0][0].score == 1 / 61 + 1 / 63
    # weights and k travel; an expr belongs to its own arm
    monkeypatch.setattr(st, "build_filter", lambda expr: np.arange(10) % 2 == 0)
    reqs[1].expr = 'period == "Q0"'
    st.hybrid_search(reqs, RRFRanker(k=10, weights=[0.25, 2]), limit=3)
    assert FUSE_CALLS[-1] == ((2, 2, 6), 3, [0.25, 2.0], 10.0)
    assert st.index.calls[-1] == ("search", 4, {}) and FakeSparse.built[-1].calls[-1][1] is not None
    reqs[0].expr, reqs[1].expr = "primary_value > 1", None
    st.hybrid_search(reqs, RRFRanker(), limit=3)
    assert "filt" in st.index.calls[-1][2] and FakeSparse.built[-1].calls[-1][1] is None


def test_hybrid_search_routes_the_dense_arm_through_sq8_when_the_index_has_a_shadow():
    st = make_store()
    st.create_index("embedding", {"index_type": "SQ8", "metric_type": "COSINE"})
    st.hybrid_search([AnnSearchRequest(Q, "embedding", COS, limit=4)], RRFRanker(), limit=3)
    assert st.index.calls[-1] == ("search", 4, {"sq8": True})


def _arms(n_dense=2, n_sparse=2):
    return [AnnSearchRequest(np.ones((n_dense, 8), dtype=np.float32), "embedding", COS, limit=4),
            AnnSearchRequest(["eps"] * n_sparse, "sparse", BM25, limit=4)]


@pytest.mark.parametrize("call", [
    lambda st: st.hybrid_search([], RRFRanker(), limit=3),
    lambda st: st.hybrid_search(_arms() * 3, RRFRanker(), limit=3),                            # more than 4 arms
    lambda st: st.hybrid_search([("embedding", Q)], RRFRanker(), limit=3),
    lambda st: st.hybrid_search(_arms(), None, limit=3),
    lambda st: st.hybrid_search(_arms(), "rrf", limit=3),
    lambda st: st.hybrid_search(_arms(), RRFRanker(weights=[1.0]), limit=3),                   # one weight per arm
    lambda st: st.hybrid_search(_arms(), RRFRanker(), limit=0),
    lambda st: st.hybrid_search(_arms(), RRFRanker(), limit=65),
    lambda st: st.hybrid_search(_arms(), RRFRanker(), limit=2.0),
    lambda st: st.hybrid_search(_arms(2, 3), RRFRanker(), limit=3),                            # query counts differ
    lambda st: st.hybrid_search([AnnSearchRequest(Q, "embedding", COS, limit=65)], RRFRanker(), limit=3),
    lambda st: st.hybrid_search([AnnSearchRequest(["a", "b"], "sparse", BM25, limit=65)], RRFRanker(), limit=3),
    lambda st: st.hybrid_search([AnnSearchRequest(["a", "b"], "embedding", COS, limit=3)], RRFRanker(), limit=3),
    lambda st: st.hybrid_search([AnnSearchRequest(Q, "sparse", BM25, limit=3)], RRFRanker(), limit=3),
    lambda st: st.hybrid_search([AnnSearchRequest(Q, "embedding", {"metric_type": "IP"}, limit=3)], RRFRanker(), limit=3),
    lambda st: st.hybrid_search([AnnSearchRequest(Q, "embedding", {"metric_type": "COSINE", "params": {"radius": 0.1}},
                                                  limit=3)], RRFRanker(), limit=3),
    lambda st: st.hybrid_search([AnnSearchRequest(Q, "other", COS, limit=3)], RRFRanker(), limit=3),
])
def test_bad_hybrid_arguments_raise_value_error(call):
    st = make_store()
    with pytest.raises(ValueError):
        call(st)
    assert st.index.calls == [] and FUSE_CALLS == []


def test_request_and_ranker_validate_their_own_arguments():
    for bad in (0, -1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="limit"):
            AnnSearchRequest(Q, "embedding", COS, limit=bad)
    with pytest.raises(ValueError):
        AnnSearchRequest(Q, "embedding", ["COSINE"], limit=3)
    for bad in (0, -60, float("nan"), float("inf"), "60", True):
        with pytest.raises(ValueError, match="k must"):
            RRFRanker(k=bad)
    for bad in ([-1.0, 1.0], [float("nan"), 1.0], ["1", 1], [True, 1.0]):
        with pytest.raises(ValueError, match="weights"):
            RRFRanker(weights=bad)
    r = RRFRanker(weights=(1, 2))
    assert r.k == 60.0 and r.arm_weights(2) == [1.0, 2.0] and RRFRanker().arm_weights(3) == [1.0, 1.0, 1.0]
    with pytest.raises(NotImplementedError, match=r"RRFRanker\(weights=\.\.\.\)"):
        WeightedRanker(0.7, 0.3)
    with pytest.raises(KeyError):
        make_store().hybrid_search(_arms(), RRFRanker(), limit=3, output_fields=["nope"])


# ---- persistence ------------------------------------------------------------------------------------------
class LoadableStore(HostStore):
    """CorpusStore on the double, with the constructor signature load_from calls."""

    def __init__(self, name="c", dim=8, capacity=64, device=None, metric_type="COSINE", index=None):
        CorpusStore.__init__(self, name, dim=dim, capacity=capacity, metric_type=metric_type,
                             index=index or FakeIndex(dim, capacity))


def test_save_records_the_sparse_index_and_load_redeclares_it(tmp_path):
    st = make_store(cls=LoadableStore, sparse=False)
    st.save(str(tmp_path / "plain"))
    meta = json.load(open(tmp_path / "plain" / "columns.json"))
    assert "sparse_index" not in meta                                              # a store without one is written as before
    assert not LoadableStore.load_from(str(tmp_path / "plain")).has_index(field_name="sparse")
    st.create_index("sparse", dict(SPARSE, params={"bm25_k1": 1.5, "bm25_b": 0.5}))
    st.save(str(tmp_path / "lex"))
    meta = json.load(open(tmp_path / "lex" / "columns.json"))
    assert meta["sparse_index"] == {"bm25_k1": 1.5, "bm25_b": 0.5}
    back = LoadableStore.load_from(str(tmp_path / "lex"))
    assert back.has_index(field_name="sparse") and back._lexical.params == {"bm25_k1": 1.5, "bm25_b": 0.5}
    assert back._lexical.built is None                                                    # rebuilt on first use
    assert sorted(h.id for h in back.search(["eps"], "sparse", BM25, limit=5)[0]) == ["k0", "k1", "k7"]
    assert FakeSparse.built[-1].postings.k1 == 1.5


def test_the_recorded_v1_directory_still_loads():
    st = LoadableStore.load_from(GOLD_STORE)
    assert st.num_entities == 5 and st.dim == 32 and st.index_type == "FLAT"
    assert not st.has_index() and not st.has_index(field_name="sparse") and st._lexical.params is None
    with pytest.raises(ValueError, match="no sparse index"):
        st.search(["gold"], "sparse", BM25, limit=3)
    st.create_index("sparse", SPARSE)
    assert len(st.search(["gold"], "sparse", BM25, limit=10)[0]) == 5              # every text is "gold:k<i>"


# ---- the sharded store ------------------------------------------------------------------------------------
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


def test_sharded_store_refuses_lexical_and_hybrid_search(one_rank_group):
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    st = ShardedCorpusStore("c", dim=8, capacity=4, index=FakeIndex(8, 4), backend=object())
    with pytest.raises(NotImplementedError, match="sharded store"):
        st.create_index("sparse", SPARSE)
    with pytest.raises(NotImplementedError, match="BM25 search"):
        st.search(["eps"], "sparse", BM25, limit=3)
    with pytest.raises(NotImplementedError, match="hybrid search"):
        st.hybrid_search(_arms(), RRFRanker(), limit=3)
    with pytest.raises(ValueError, match="unknown vector field"):
        st.create_index("text", SPARSE)                                            # as before


# ---- VectorRAG, the MCP tool, the REST request ---------------------------------------------------------------
class RecStore:
    num_entities = 0

    def __init__(self):
        self.calls = []

    def load(self):
        pass

    def search(self, data, anns_field, param, limit, **kw):
        self.calls.append(("search", param, limit, kw))
        return [[] for _ in range(np.asarray(data).shape[0])]

    def hybrid_search(self, reqs, rerank, limit, output_fields=None):
        self.calls.append(("hybrid", [(r.anns_field, r.param, r.limit, r.expr, np.asarray(r.data).shape[0]) for r in reqs],
                           (rerank.k, rerank.weights), limit, output_fields))
        return [[] for _ in range(len(reqs[1].data))]


class Emb:
    def encode(self, texts):
        return np.zeros((len(texts), 4), dtype=np.float32)


def test_vector_rag_runs_both_arms_at_fetch_k():
    from rag_fin_amd.rag import OUTPUT_FIELDS, VectorRAG
    rag = VectorRAG("k", embedder=Emb(), store=RecStore())
    rag.search("basic eps", 3, hybrid=True)
    rag.search("basic eps", 5, expr='period == "Q1"', hybrid=True, fetch_k=30)
    rag.search_batch(["a", "b"], 10, hybrid=True)
    rag.search("basic eps", 3)
    rag.search("basic eps", 3, hybrid=False)

    def arms(fk, expr, n):
        return [("embedding", COS, fk, expr, n), ("sparse", BM25, fk, expr, n)]

    plain = ("search", COS, 3, {"expr": None, "output_fields": OUTPUT_FIELDS})
    assert rag.collection.calls == [
        ("hybrid", arms(20, None, 1), (60.0, None), 3, OUTPUT_FIELDS),
        ("hybrid", arms(30, 'period == "Q1"', 1), (60.0, None), 5, OUTPUT_FIELDS),
        ("hybrid", arms(40, None, 2), (60.0, None), 10, OUTPUT_FIELDS),
        plain, plain]                                                              # without it: the call of before
    assert rag.search_batch([], 3, hybrid=True) == []


@pytest.mark.parametrize("kw", [{"min_score": 0.2}, {"max_score": 0.9}, {"group_by": "period"}, {"mmr_lambda": 0.5},
                                {"fetch_k": 2}, {"fetch_k": 65}, {"fetch_k": 0}, {"fetch_k": 20.0}, {"fetch_k": True}])
def test_vector_rag_refuses_what_has_no_hybrid_form(kw):
    from rag_fin_amd.rag import VectorRAG
    rag = VectorRAG("k", embedder=Emb(), store=RecStore())
    with pytest.raises(ValueError):
        rag.search("basic eps", 3, hybrid=True, **kw)
    with pytest.raises(ValueError):
        rag.search_batch(["basic eps"], 3, hybrid=True, **kw)
    if "fetch_k" not in kw:
        with pytest.raises(ValueError):
            rag.search("basic eps", 3, hybrid=True, rerank=True, **kw)
    assert rag.collection.calls == []


def test_vector_rag_hybrid_contexts_and_rerank():
    """End to end over the doubles: the score of a context is the fused score; with rerank the
    cross-encoder sees the fused candidates."""
    from rag_fin_amd.rag import VectorRAG

    class Rerank:
        def predict(self, pairs):
            self.pairs = pairs
            return [float(len(t)) for _, t in pairs]                               # the longest text wins

    st = make_store()
    st._prepare_queries = lambda data: torch.ones((np.asarray(data).shape[0], 8)).half()
    rr = Rerank()
    rag = VectorRAG("k", embedder=Emb(), store=st, reranker=rr)
    got = rag.search("eps", top_k=2, hybrid=True, fetch_k=4)
    assert FUSE_CALLS[-1] == ((2, 1, 4), 2, [1.0, 1.0], 60.0)
    # row 7 leads the BM25 list and is third in the dense one (rows 9, 8, 7, 6); row 9 leads the dense list
    assert [(c["rank"], c["text"]) for c in got] == [(1, "eps eps eps"), (2, "nothing else here")]
    assert got[0]["score"] == 1 / 61 + 1 / 63 and "rerank_score" not in got[0]
    got = rag.search("eps", top_k=2, hybrid=True, fetch_k=4, rerank=True)
    assert FUSE_CALLS[-1] == ((2, 1, 4), 4, [1.0, 1.0], 60.0)                       # fetch_k fused candidates
    assert len(rr.pairs) == 4 and all(q == "eps" for q, _ in rr.pairs)
    assert sorted(t for _, t in rr.pairs) == sorted(["eps eps eps", "nothing else here", "diluted eps was 14.90",
                                                     "q2 profit fell"])
    assert [c["text"] for c in got] == ["diluted eps was 14.90", "nothing else here"]
    assert got[0]["rerank_score"] == 21.0 and got[0]["score"] == 1 / 62            # the fused score stays
    st.drop_index(field_name="sparse")
    with pytest.raises(ValueError, match="no sparse index"):
        rag.search("eps", top_k=2, hybrid=True)


class FakeRag:
    def __init__(self):
        self.calls = []

    def search(self, query, top_k=3, expr=None, **kw):
        self.calls.append((query, top_k, expr, kw))
        return []


def test_mcp_tool_carries_hybrid():
    rag = FakeRag()
    mcp_server.set_rag(rag)
    try:
        r = mcp_server.search_vectors("basic eps in q1", 4, hybrid=True)
        assert r == {"status": "success", "query": "basic eps in q1", "results": [], "result_count": 0}
        assert rag.calls[-1] == ("basic eps in q1", 4, None, {"hybrid": True})
        mcp_server.search_vectors("q", 4, filter="primary_value > 0", hybrid=True, fetch_k=32, rerank=True)
        assert rag.calls[-1] == ("q", 4, "primary_value > 0", {"fetch_k": 32, "rerank": True, "hybrid": True})
        mcp_server.search_vectors("q", 4, min_score=0.2, hybrid=True)              # (VectorRAG refuses the combination)
        assert rag.calls[-1] == ("q", 4, None, {"min_score": 0.2, "max_score": None, "hybrid": True})
        mcp_server.search_vectors("q", 2, hybrid=False)                            # the call of before
        assert rag.calls[-1] == ("q", 2, None, {})
        from rag_fin_amd.rag import VectorRAG
        mcp_server.set_rag(VectorRAG("k", embedder=Emb(), store=RecStore()))
        r = mcp_server.search_vectors("q", 4, group_by="period", hybrid=True)
        assert r["status"] == "error" and "group_by" in r["message"]
    finally:
        mcp_server.set_rag(None)


def test_search_request_payload():
    from rag_fin_amd.adapter import SearchRequest, search_args
    assert search_args(SearchRequest(query="hello", top_k=4)) == {"query": "hello", "top_k": 4}
    assert search_args(SearchRequest(query="hello", hybrid=True)) == {"query": "hello", "top_k": 3, "hybrid": True}
    assert search_args(SearchRequest(query="hello", hybrid=False)) == {"query": "hello", "top_k": 3}
    assert search_args(SearchRequest(query="hello", filter="id == 1", hybrid=True, fetch_k=40, rerank=True)) == \
        {"query": "hello", "top_k": 3, "filter": "id == 1", "fetch_k": 40, "rerank": True, "hybrid": True}
    with pytest.raises(Exception):
        SearchRequest(query="hello", hybrid="maybe so")


def test_build_rag_declares_the_lexical_index(monkeypatch):
    from rag_fin_amd import chunker, embedder, service
    made = {}

    class Store(LoadableStore):
        def __init__(self, name, dim, device=None):
            LoadableStore.__init__(self, name, dim=dim)
            made["store"] = self

    class E:
        dim = 8

        @classmethod
        def from_local(cls, model_dir, device=None):
            return cls()

    monkeypatch.setattr(embedder, "Embedder", E)
    monkeypatch.setattr(store_mod, "CorpusStore", Store)
    monkeypatch.setattr(chunker, "build_all_chunks", lambda data_dir: [])
    service.build_rag("m", "d")
    assert not made["store"].has_index(field_name="sparse")
    service.build_rag("m", "d", hybrid=True)
    assert made["store"].has_index(field_name="sparse")
    seen = []
    monkeypatch.setattr(service, "build_rag", lambda *a, **kw: seen.append(kw["hybrid"]))
    monkeypatch.setenv("RAGFIN_MODEL_DIR", "m")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for value, want in (("1", True), ("0", False), (None, False)):
        monkeypatch.delenv("LEXICAL_INDEX", raising=False)
        if value is not None:
            monkeypatch.setenv("LEXICAL_INDEX", value)
        service.build_rag_from_env()
        assert seen[-1] is want


# ---- C ABI: host-side argument checks (no GPU needed) ------------------------------------------------------
def test_sparse_abi_argument_checks():
    lib = _lib.load_library()
    fake = ctypes.c_void_p(4096)     # never dereferenced: every failing case fails its checks first
    odd = ctypes.c_void_p(4100)      # not 16-byte aligned
    out = ctypes.c_void_p()

    def create(o=ctypes.byref(out), n=10, v=5, nnz=20, off=fake, row=fake, imp=fake, dev=0):
        return lib.rf_sparse_create(o, n, v, nnz, off, row, imp, dev)

    for null in ("o", "off", "row", "imp"):
        assert create(**{null: None}) == -1 and b"null" in lib.rf_last_error()
    for bad in ({"n": 0}, {"n": -1}, {"n": 2 ** 31}, {"v": 0}, {"nnz": 0}, {"dev": -1}):
        assert create(**bad) == -1 and not out.value
    for mis in ("off", "row", "imp"):
        assert create(**{mis: odd}) == -1 and b"aligned" in lib.rf_last_error()
    assert create(n=2 * _lib.RF_SPARSE_TILE_ROWS + 37) == 0 and out.value          # a handle is host state only
    sp = ctypes.c_void_p(out.value)
    assert lib.rf_sparse_search_workspace_bytes(sp, 1, 1) == 3 * 8                  # 3 tiles x k x one 8-byte key
    assert lib.rf_sparse_search_workspace_bytes(sp, 64, 64) == 64 * 3 * 64 * 8
    for B, k in ((0, 1), (1, 0), (1, 65), (65536, 1)):
        assert lib.rf_sparse_search_workspace_bytes(sp, B, k) == 0
    assert lib.rf_sparse_search_workspace_bytes(None, 1, 1) == 0

    def search(s=sp, filt=None, qo=fake, qt=fake, qw=fake, B=1, k=10, sc=fake, ids=fake, ws=fake, wsb=1 << 20):
        return lib.rf_sparse_search(s, filt, qo, qt, qw, B, k, 0, sc, ids, None, ws, wsb, None)

    for null in ("s", "qo", "qt", "qw", "sc", "ids", "ws"):
        assert search(**{null: None}) == -1 and b"null" in lib.rf_last_error()
    for bad in ({"B": 0}, {"B": 65536}, {"k": 0}, {"k": 65}, {"ws": odd}, {"filt": odd}):
        assert search(**bad) == -1
    assert search(wsb=239) == -3 and b"workspace" in lib.rf_last_error()            # RF_ERR_CAPACITY: 240 needed
    assert lib.rf_sparse_destroy(sp) == 0 and lib.rf_sparse_destroy(None) == 0
    assert (_lib.RF_SPARSE_MAX_TERMS, _lib.RF_SPARSE_TILE_ROWS, _lib.RF_FUSE_MAX_ARMS) == (64, 8192, 4)
    assert lexical.MAX_QUERY_TERMS == _lib.RF_SPARSE_MAX_TERMS


def test_fuse_abi_argument_checks():
    lib = _lib.load_library()
    fake = ctypes.c_void_p(4096)

    def fuse(A=2, arms=fake, F=10, w=None, rrf_k=60.0, B=1, k=5, sc=fake, ids=fake):
        wh = None if w is None else (ctypes.c_double * len(w))(*w)
        return lib.rf_fuse_rrf(A, arms, F, wh, rrf_k, B, k, sc, ids, None, None)

    for null in ("arms", "sc", "ids"):
        assert fuse(**{null: None}) == -1 and b"null" in lib.rf_last_error()
    for bad in ({"A": 0}, {"A": 5}, {"F": 0}, {"F": 65}, {"B": 0}, {"k": 0}, {"k": 65}):
        assert fuse(**bad) == -1
    for rrf_k in (0.0, -1.0, float("nan"), float("inf")):
        assert fuse(rrf_k=rrf_k) == -1 and b"rrf_k" in lib.rf_last_error()
    for w in ([1.0, -0.5], [float("nan"), 1.0], [1.0, float("inf")]):
        assert fuse(w=w) == -1 and b"weight" in lib.rf_last_error()
