"""Decayed search on the GPU: rf_decay_weights against ranker.decay_weights_reference bit for
bit, the weighted chain (rf_search_weighted behind GpuIndex.search(weights=)) against
oracle.search.exact_scores fed into ranker.decay_reference -- ids, decayed and base fp64 scores and float32
scores all bit-equal --, and CorpusStore.search(ranker=DecayRanker(...)) / VectorRAG.search(decay=...) over a
store that is deleted from and upserted into."""
import functools

import numpy as np
import pytest

from oracle import search as osearch
from rag_fin_amd.ranker import DECAY_FUNCTIONS, DecayRanker, decay_reference, decay_weights_reference
from rag_fin_amd.schema import DataType, FieldSchema
from test_filtered_search_gpu import filter_from_mask

pytestmark = pytest.mark.gpu

COS = {"metric_type": "COSINE"}
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def bits(a):
    """The bit patterns of a float array (so that -0.0 / 0.0 and every rounding count)."""
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


# ---- 1. rf_decay_weights ----------------------------------------------------------------------------------
NW = 4099   # 16 workgroups and 3 rows


def run_weights(column, ranker, device):
    import torch
    from rag_fin_amd.index import decay_weights
    w32, w64 = decay_weights(torch.from_numpy(column).to(device), ranker)
    torch.cuda.synchronize(device)
    return w32.cpu().numpy(), w64.cpu().numpy()


def check_weights(column, ranker, device):
    want = decay_weights_reference(column, ranker)
    w32, w64 = run_weights(column, ranker, device)
    assert w64.dtype == np.float64 and w32.dtype == np.float32 and w64.shape == w32.shape == (column.size,)
    bad = np.flatnonzero(bits(w64) != bits(want))
    assert bad.size == 0, (ranker, column[bad[:5]], w64[bad[:5]], want[bad[:5]])
    assert np.array_equal(bits(w32), bits(want.astype(np.float32))), ranker
    assert w64.min() >= 0.0 and w64.max() <= 1.0
    return want


@pytest.mark.parametrize("function", DECAY_FUNCTIONS)
def test_weights_of_a_double_column_equal_the_reference(gpu_device, function):
    rng = np.random.default_rng(DECAY_FUNCTIONS.index(function))
    origin, scale, offset, decay = 100.0, 7.0, 3.0, 0.3
    L = -np.log2(decay)
    v = origin + rng.uniform(-90, 90, NW)
    # the edges: NaN, +-inf, the origin, exactly at the offset, and distances whose t = L d / scale (exp) runs
    # across 1022 .. 1100: the last normal results, the subnormal tail and the cut-off; the same distances put
    # the float32 weights through their subnormals (t 126 .. 149) on the way
    t = np.concatenate([np.arange(1020.0, 1102.0, 0.5), np.arange(120.0, 152.0, 0.25), [1074.0, 1075.0, 1099.999, 1100.0]])
    edge = np.concatenate([[np.nan, np.inf, -np.inf, origin, origin + offset, origin - offset, np.nextafter(origin + offset, np.inf),
                            -0.0, 0.0, 1e308, -1e308, 5e-324], origin + offset + t * scale / L, origin - offset - np.sqrt(t / L) * scale])
    v[:edge.size] = edge
    r = DecayRanker("primary_value", function, origin, scale, offset, decay)
    want = check_weights(v, r, gpu_device)
    assert want[:3].tolist() == [0.0, 0.0, 0.0] and want[3:6].tolist() == [1.0, 1.0, 1.0]
    if function != "linear":
        assert ((want > 0) & (want < 2.3e-308)).any() and (want[12:edge.size] == 0.0).any()   # the tail was visited
    check_weights(v, DecayRanker("primary_value", function, -1e300, 1e-300, 0.0, 0.999), gpu_device)
    check_weights(v, DecayRanker("primary_value", function, 0.0, 1e300, 1e19, 1e-300), gpu_device)


@pytest.mark.parametrize("function", DECAY_FUNCTIONS)
def test_weights_of_an_int64_column_equal_the_reference(gpu_device, function):
    rng = np.random.default_rng(10 + DECAY_FUNCTIONS.index(function))
    v = rng.integers(2000, 2040, NW).astype(np.int64)
    # +-2^63 ends, integers that are no doubles (rounded to nearest first), the origin, exactly at the offset
    edge = [I64_MIN, I64_MIN + 1, I64_MAX, I64_MAX - 1, (1 << 53) + 1, -(1 << 53) - 1, (1 << 62) + 1, 2024, 2026, 2022, 0, -1]
    v[:len(edge)] = edge
    want = check_weights(v, DecayRanker("fiscal_year", function, 2024, 3, offset=2, decay=0.25), gpu_device)
    assert want[7:10].tolist() == [1.0, 1.0, 1.0]
    for origin in (-9.3e18, 9.3e18, 1e300):
        check_weights(v, DecayRanker("fiscal_year", function, origin, 1e18, decay=0.9), gpu_device)
    check_weights(v[:1], DecayRanker("fiscal_year", function, 2024, 3), gpu_device)           # one row
    w32, w64 = run_weights(v[:0], DecayRanker("fiscal_year", function, 2024, 3), gpu_device)  # none
    assert w32.size == w64.size == 0


# ---- 2. the weighted chain ---------------------------------------------------------------------------------
N, NQ = 12_321, 65          # above RF_SMALL_ROWS, 385 blocks and one row; JB 1, JB 2 and two sweeps
N_SMALL = 1_000             # the no-sample route


@functools.lru_cache(maxsize=None)
def corpus(dim):
    """Rows, queries and their fp64 scores for one dim, computed once and never changed; the weights (a quarter
    exactly 0) and a filter that passes about a third of the rows, in scattered blocks and scattered rows."""
    c16 = osearch.synth_unit_rows(N, dim, 4321 + dim)
    q16 = osearch.synth_unit_rows(NQ, dim, 8765 + dim)
    scores = osearch.exact_scores(q16, c16)
    rng = np.random.default_rng(dim)
    w64 = rng.uniform(0.0, 1.0, N)
    w64[rng.random(N) < 0.25] = 0.0
    w64[rng.random(N) < 0.01] = 1.0
    nblk = (N + 31) // 32
    passing = np.repeat(rng.random(nblk) < 0.5, 32)[:N] & (rng.random(N) < 0.66)
    for a in (scores, w64, passing):
        a.setflags(write=False)
    return c16, q16, scores, w64, passing


_INDEX = {}


def index_of(dim, n, device):
    import torch
    from rag_fin_amd.store import GpuIndex
    if (dim, n) not in _INDEX:
        ix = GpuIndex(dim, n, device, shadow=False)
        ix.add(torch.from_numpy(corpus(dim)[0][:n]).to(device))
        _INDEX[(dim, n)] = ix
    return _INDEX[(dim, n)]


def device_weights(w64, device):
    import torch
    return torch.from_numpy(w64.astype(np.float32)).to(device), torch.from_numpy(np.array(w64, dtype=np.float64)).to(device)


def check_search(ix, q16, scores, w64, passing, k, device, id_base=0):
    """GpuIndex.search(weights=) against the reference: everything bit for bit."""
    import torch
    want = decay_reference(scores, passing, w64, k)
    filt = None if passing is None else filter_from_mask(np.ascontiguousarray(passing), device)
    got = ix.search(torch.from_numpy(q16).to(device), k, id_base=id_base, filt=filt, weights=device_weights(w64, device))
    torch.cuda.synchronize(device)
    sc, ids, dec, base = (t.cpu().numpy() for t in got)
    assert np.array_equal(ids, np.where(want[1] >= 0, want[1] + id_base, -1))
    assert np.array_equal(bits(dec), bits(want[2])) and np.array_equal(bits(base), bits(want[3]))
    assert np.array_equal(bits(sc), bits(want[0]))
    return want


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("B", [1, 33, 65])
@pytest.mark.parametrize("dim", [64, 384])
def test_chain_equals_the_reference(gpu_device, dim, B, k, filtered):
    c16, q16, scores, w64, passing = corpus(dim)
    check_search(index_of(dim, N, gpu_device), q16[:B], scores[:B], w64, passing if filtered else None, k, gpu_device)


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("B", [1, 33, 65])
@pytest.mark.parametrize("dim", [64, 384])
def test_small_route_equals_the_reference(gpu_device, dim, B, k, filtered):
    c16, q16, scores, w64, passing = corpus(dim)
    check_search(index_of(dim, N_SMALL, gpu_device), q16[:B], scores[:B, :N_SMALL], w64[:N_SMALL],
                 passing[:N_SMALL] if filtered else None, k, gpu_device)


def test_an_id_base_and_an_empty_filter(gpu_device):
    c16, q16, scores, w64, passing = corpus(64)
    ix = index_of(64, N, gpu_device)
    check_search(ix, q16[:3], scores[:3], w64, passing, 10, gpu_device, id_base=1 << 40)
    want = check_search(ix, q16[:3], scores[:3], w64, np.zeros(N, dtype=bool), 5, gpu_device)
    assert (want[1] == -1).all()
    few = np.zeros(N, dtype=bool)
    few[[5, 4000, N - 1]] = True                       # fewer passing rows than k, the last row among them
    check_search(ix, q16[:3], scores[:3], w64, few, 10, gpu_device)


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("dim", [64, 384])
def test_all_ones_weights_give_the_filtered_search_of_the_existing_path(gpu_device, dim, filtered):
    import torch
    c16, q16, scores, w64, passing = corpus(dim)
    ix = index_of(dim, N, gpu_device)
    q = torch.from_numpy(q16[:40]).to(gpu_device)
    filt = filter_from_mask(np.ascontiguousarray(passing), gpu_device) if filtered else None
    sc0, ids0, ex0 = ix.search(q, 10, want_exact=True, filt=filt)
    sc, ids, dec, base = ix.search(q, 10, filt=filt, weights=device_weights(np.ones(N), gpu_device))
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(ids, ids0) and torch.equal(dec.view(torch.int64), ex0.view(torch.int64))
    assert torch.equal(base.view(torch.int64), ex0.view(torch.int64)) and torch.equal(sc.view(torch.int32), sc0.view(torch.int32))


def test_all_zero_weights_overflow_the_lists_and_the_ladder_answers(gpu_device):
    """Every weighted score is +-0 and the threshold lies below it, so every row is a candidate: the queries
    come back flagged from the first pass (the ordinary overflow path) and the exhaustive weighted kernel ranks
    them by s, then by row."""
    import torch
    from rag_fin_amd import _lib
    from rag_fin_amd.store import GpuIndex
    n, dim = 20_000, 64
    c16 = osearch.synth_unit_rows(n, dim, 99)
    q16 = osearch.synth_unit_rows(2, dim, 98)
    scores = osearch.exact_scores(q16, c16)
    ix = GpuIndex(dim, n, gpu_device, shadow=False)
    ix.add(torch.from_numpy(c16).to(gpu_device))
    q = torch.from_numpy(q16).to(gpu_device)
    weights = device_weights(np.zeros(n), gpu_device)
    flags = ix.search_weighted_raw(q, 10, weights)[4]
    torch.cuda.synchronize(gpu_device)
    assert (flags.cpu().numpy() & _lib.RF_FLAG_CAND_OVERFLOW).all()
    want = check_search(ix, q16, scores, np.zeros(n), None, 10, gpu_device)
    assert np.array_equal(want[1][0], np.lexsort((np.arange(n), -scores[0]))[:10])
    assert np.array_equal(bits(want[2]), bits(np.where(want[3] < 0, -0.0, 0.0)))


def test_negative_scores_rank_a_larger_weight_lower(gpu_device):
    c16, q16, scores, _, _ = corpus(64)
    ix = index_of(64, N, gpu_device)
    negative = scores[0] < 0
    assert negative.sum() > 1000
    plain = check_search(ix, q16[:1], scores[:1], np.ones(N), negative, 10, gpu_device)
    best = int(plain[1][0, 0])                       # the least negative row
    small = 2.0 ** -6
    w64 = np.full(N, small)
    w64[best] = 1.0                                  # everyone else is pulled towards 0, i.e. up
    want = check_search(ix, q16[:1], scores[:1], w64, negative, 10, gpu_device)
    others = negative.copy()
    others[best] = False
    overtaken = int((small * scores[0][others] > scores[0, best]).sum())   # rows now ahead of the heaviest one
    assert overtaken >= 1 and (want[2] < 0).all() and want[1][0, 0] != best
    assert (best in want[1][0].tolist()) == (overtaken < 10)
    if overtaken < 10:
        assert want[1][0].tolist().index(best) == overtaken


# ---- 3. through the store -----------------------------------------------------------------------------------
NS, DS = 9_000, 64
PERIODS = ["Q1_FY2024", "Q2_FY2024", "Q3_FY2024", "Q4_FY2024"]
_STORE = {}


def store(device):
    """One 9 000-row store for the module with an INT64 fiscal_year field; the tests below mutate it in order."""
    if not _STORE:
        import torch
        from rag_fin_amd.store import CorpusStore
        r = np.arange(NS)
        st = CorpusStore("decay", dim=DS, capacity=NS + 64, device=device,
                         fields=[FieldSchema("fiscal_year", DataType.INT64, default=2024)])
        st.add([f"k{i}" for i in r], [f"text {i}" for i in r], torch.from_numpy(osearch.synth_unit_rows(NS, DS, 777)).to(device),
               np.array(PERIODS)[r % 4].tolist(), ["c"] * NS, ["s"] * NS, ((r * 37) % 1000 / 10.0).tolist(),
               extra={"fiscal_year": (2005 + (r * 7) % 23).tolist()})
        _STORE.update(st=st, q=torch.from_numpy(osearch.synth_unit_rows(3, DS, 778)).to(device))
    return _STORE


RANKERS = [DecayRanker("fiscal_year", "gauss", 2024, 3, offset=1), DecayRanker("fiscal_year", "exp", 2020, 2, decay=0.3),
           DecayRanker("fiscal_year", "linear", 2024, 6), DecayRanker("primary_value", "gauss", 50.0, 12.5, offset=2.5),
           DecayRanker("primary_value", "linear", 0.0, 30.0, decay=0.25)]


def check_store(device, ranker, limit, expr=None):
    """search(ranker=) against the reference over the store's LIVE rows and columns."""
    w = store(device)
    st = w["st"]
    n = st.num_entities
    c16 = st.index.get_rows(np.arange(n)).cpu().numpy()
    scores = osearch.exact_scores(w["q"].cpu().numpy(), c16)
    col = np.asarray(st.columns[ranker.field], dtype=np.int64 if ranker.field == "fiscal_year" else np.float64)
    w64 = decay_weights_reference(col, ranker)
    passing = None if expr is None else np.array([p == "Q4_FY2024" for p in st.columns["period"]])
    want = decay_reference(scores, passing, w64, limit)
    res = st.search(w["q"], "embedding", COS, limit, expr=expr, ranker=ranker, output_fields=["fiscal_year", "primary_value"])
    assert len(res) == 3
    for b, hits in enumerate(res):
        live = want[1][b] >= 0
        rows = want[1][b][live]
        assert [h.row for h in hits] == rows.tolist(), (ranker, b)
        assert [h.score for h in hits] == [float(x) for x in want[0][b][live]], (ranker, b)
        assert [h.entity.fiscal_year for h in hits] == [st.columns["fiscal_year"][r] for r in rows]
        assert [h.entity.primary_value for h in hits] == [st.columns["primary_value"][r] for r in rows]
        assert [h.id for h in hits] == [st.columns["id"][r] for r in rows]
    return want, res


@pytest.mark.parametrize("ranker", RANKERS, ids=lambda r: f"{r.field}-{r.function}")
def test_store_search_equals_the_reference(gpu_device, ranker):
    check_store(gpu_device, ranker, 10)
    check_store(gpu_device, ranker, 64, expr='period == "Q4_FY2024"')
    st = store(gpu_device)["st"]
    assert st.search(store(gpu_device)["q"], "embedding", COS, 5, expr='period == "Q9_FY2031"', ranker=ranker) == [[], [], []]


def test_store_search_after_a_delete_and_an_upsert(gpu_device):
    import torch
    w = store(gpu_device)
    st = w["st"]
    recent = RANKERS[0]
    before, _ = check_store(gpu_device, recent, 10)
    top = [st.columns["id"][r] for r in before[1][0][:3]]
    st.delete('id in ["%s", "%s"]' % (top[0], top[1]))                  # the best two hits of query 0 go
    assert st.num_entities == NS - 2
    after, res = check_store(gpu_device, recent, 10)
    assert [h.id for h in res[0]][0] == top[2]
    # the third moves to a year far from the origin, and two fresh rows arrive at the origin
    vec = st.index.get_rows([st.columns["id"].index(top[2])]).float().cpu().numpy()
    fresh = osearch.synth_unit_rows(2, DS, 779).astype(np.float32)
    st.upsert([[top[2], "n0", "n1"], ["moved", "new 0", "new 1"], np.concatenate([vec, fresh]), ["Q4_FY2024"] * 3, ["c"] * 3,
               ["s"] * 3, [1.0, 2.0, 3.0], [1990, 2024, 2024]])
    assert st.num_entities == NS and st.columns["fiscal_year"][-3:] == [1990, 2024, 2024]
    _, res = check_store(gpu_device, recent, 10)
    assert top[2] not in [h.id for h in res[0]]
    for r in RANKERS[1:]:
        check_store(gpu_device, r, 10, expr='period == "Q4_FY2024"')
    torch.cuda.synchronize(gpu_device)


def test_vector_rag_search_with_a_decay(gpu_device):
    from rag_fin_amd.rag import VectorRAG
    w = store(gpu_device)
    st = w["st"]

    class Emb:
        def encode_to_device(self, texts):
            return w["q"][:len(texts)]

    rag = VectorRAG("no-key", "decay", embedder=Emb(), store=st)
    d = {"field": "fiscal_year", "function": "gauss", "origin": 2024, "scale": 3, "offset": 1}
    want, _ = check_store(gpu_device, RANKERS[0], 5)
    got = rag.search("what is the net interest margin", 5, decay=d)
    assert [c["rank"] for c in got] == [1, 2, 3, 4, 5]
    assert [c["score"] for c in got] == [float(x) for x in want[0][0]]              # the decayed score
    assert [c["primary_value"] for c in got] == [st.columns["primary_value"][r] for r in want[1][0]]
    want, _ = check_store(gpu_device, RANKERS[0], 3, expr='period == "Q4_FY2024"')
    batch = rag.search_batch(["a", "b", "c"], 3, expr='period == "Q4_FY2024"', decay=d)
    assert [[c["score"] for c in ctx] for ctx in batch] == [[float(x) for x in row] for row in want[0]]
