"""Boosted search on the GPU: rf_boost_classes against numpy bit operations,
rf_merge_boosted against ranker.boost_reference on synthetic candidate blocks, and
CorpusStore.search(ranker=...) against oracle.search.exact_scores fed into boost_reference --
ids equal and scores bit-equal."""
import numpy as np
import pytest

from oracle import adversarial as adv, search as osearch
from rag_fin_amd.ranker import BoostRanker, boost_reference, class_weights
from test_filtered_search_gpu import filter_from_mask, pack_mask

pytestmark = pytest.mark.gpu

COS = {"metric_type": "COSINE"}


def bits(a):
    """The bit patterns of a float array (so that -0.0 / 0.0 and every rounding count)."""
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


# ---- 1. rf_boost_classes ----------------------------------------------------------------------------------
def run_classes(filters, n, base, device):
    import torch
    from rag_fin_amd.index import boost_classes
    masks, counts = boost_classes(filters, n, base)
    torch.cuda.synchronize(device)
    return masks.cpu().numpy().view(np.uint32), counts.cpu().numpy()


def expect_classes(words, base_words, n):
    """Class words by numpy bit operations on the filters' mask words, padded to the stride."""
    m = len(words)
    nblk = (n + 31) // 32
    stride = (nblk + 3) // 4 * 4
    keep = pack_mask(np.ones(n, dtype=bool))
    out = np.zeros((1 << m, stride), dtype=np.uint32)
    for c in range(1 << m):
        w = keep.copy() if base_words is None else base_words & keep
        for i in range(m):
            w &= words[i] if (c >> i) & 1 else ~words[i]
        out[c, :nblk] = w
    counts = np.array([int(np.unpackbits(out[c].view(np.uint8)).sum()) for c in range(1 << m)], dtype=np.int64)
    return out, counts


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 8193, 100_003])
def test_class_masks_and_counts_equal_numpy(gpu_device, n, m):
    rng = np.random.default_rng(1000 * m + n)
    for with_base in (False, True):
        dens = rng.choice([0.0, 0.001, 0.3, 1.0], size=m)
        masks = [rng.random(n) < d for d in dens]
        base_mask = rng.random(n) < 0.6 if with_base else None
        filters = [filter_from_mask(x, gpu_device) for x in masks]
        base = filter_from_mask(base_mask, gpu_device) if with_base else None
        want, want_counts = expect_classes([pack_mask(x) for x in masks], pack_mask(base_mask) if with_base else None, n)
        got, got_counts = run_classes(filters, n, base, gpu_device)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (n, m, with_base, dens)          # tail bits and stride padding included
        assert np.array_equal(got_counts, want_counts)
        assert int(got_counts.sum()) == (int(base_mask.sum()) if with_base else n)
        again, again_counts = run_classes(filters, n, base, gpu_device)
        assert again.tobytes() == got.tobytes() and again_counts.tobytes() == got_counts.tobytes()


def test_a_filter_built_for_another_row_count_contributes_no_row(gpu_device):
    n = 1000
    rng = np.random.default_rng(5)
    mask = rng.random(n) < 0.5
    good = filter_from_mask(mask, gpu_device)
    other = filter_from_mask(np.ones(n + 64, dtype=bool), gpu_device)      # larger: its words exist, its header says n + 64
    got, counts = run_classes([good, other], n, None, gpu_device)
    want, want_counts = expect_classes([pack_mask(mask), np.zeros((n + 31) // 32, dtype=np.uint32)], None, n)
    assert np.array_equal(got, want) and np.array_equal(counts, want_counts) and counts[2] == counts[3] == 0
    got, counts = run_classes([good], n, other, gpu_device)                # as the base filter: no row at all
    assert not got.any() and not counts.any()


# ---- 2. rf_merge_boosted ------------------------------------------------------------------------------------
def class_blocks(scores, cls, C, k_in):
    """What the class searches hand to the merge: per (query, class) the plain top k_in of the class's
    rows by (s desc, row asc) -> exact f64 [B, C, k_in], ids i64 [B, C, k_in], padded -inf / -1."""
    B = scores.shape[0]
    exact = np.full((B, C, k_in), -np.inf)
    ids = np.full((B, C, k_in), -1, dtype=np.int64)
    for c in range(C):
        rows = np.flatnonzero(cls == c)
        for b in range(B):
            order = np.lexsort((rows, -scores[b, rows]))[:k_in]
            exact[b, c, :order.size] = scores[b, rows[order]]
            ids[b, c, :order.size] = rows[order]
    return exact, ids


def run_merge(exact, ids, W, k, device):
    import torch
    from rag_fin_amd.index import merge_boosted
    out = merge_boosted(torch.from_numpy(exact).to(device), torch.from_numpy(ids).to(device), W, k)
    torch.cuda.synchronize(device)
    return [t.cpu().numpy() for t in out]


def check_merge(scores, cls, W, k_in, k, device):
    exact, ids = class_blocks(scores, cls, len(W), k_in)
    got = run_merge(exact, ids, W, k, device)
    want = boost_reference(scores, None, cls, W, k)
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(bits(got[2]), bits(want[2])) and np.array_equal(bits(got[3]), bits(want[3]))
    assert np.array_equal(bits(got[0]), bits(want[0]))
    return got


WEIGHTS = [1.0, 2.5, 0.4, 1.7, 0.9, 3.0, 0.05, 1.0]


@pytest.mark.parametrize("B,C,k_in,k", [(1, 1, 1, 1), (3, 2, 10, 10), (65, 8, 64, 64), (2, 4, 64, 7)])
def test_merge_equals_the_reference_on_synthetic_blocks(gpu_device, B, C, k_in, k):
    rng = np.random.default_rng(B * 100 + C)
    N = 700
    scores = rng.uniform(-1.0, 1.0, size=(B, N))                            # negative scores under W > 1 and W < 1
    scores[:, ::9] = np.round(scores[:, ::9], 1)                            # and plenty of exact ties
    cls = rng.integers(C, size=N)
    if C >= 2:
        cls[cls == 1] = 0
        cls[[3, 44, 500]] = 1                                               # a class shorter than k_in: padding
    if C >= 4:
        cls[cls == 2] = 3                                                   # an entirely empty class
    got = check_merge(scores, cls, WEIGHTS[:C], k_in, k, gpu_device)
    assert (got[1] >= 0).all()


def test_merge_pads_the_tail_when_the_candidates_are_fewer_than_k(gpu_device):
    scores = np.array([[0.3, -0.2, 0.9, 0.1, 0.5], [-0.3, -0.2, -0.9, -0.1, -0.5]])
    cls = np.array([0, 1, 1, 2, 0])
    got = check_merge(scores, cls, [1.0, 2.0, 0.5, 4.0], 10, 10, gpu_device)
    assert (got[1][:, 5:] == -1).all() and np.isneginf(got[0][:, 5:]).all()
    assert np.isneginf(got[2][:, 5:]).all() and np.isneginf(got[3][:, 5:]).all()
    assert (got[1][:, :5] >= 0).all()


def test_merge_breaks_a_boosted_tie_across_classes_by_the_base_score_then_the_row(gpu_device):
    # s = 0.25 with W = 2 (row 0) against s = 0.5 with W = 1 (row 1): both 0.5; the base score decides
    got = check_merge(np.array([[0.25, 0.5]]), np.array([1, 0]), [1.0, 2.0], 4, 2, gpu_device)
    assert got[1].tolist() == [[1, 0]] and got[2].tolist() == [[0.5, 0.5]] and got[3].tolist() == [[0.5, 0.25]]
    # two classes of equal weight, equal scores: the row decides (row 3 of class 1 before row 7 of class 0)
    scores = np.full((1, 9), -0.75)
    scores[0, [3, 7]] = 0.125
    cls = np.array([0, 0, 0, 1, 0, 1, 1, 0, 1])
    got = check_merge(scores, cls, [2.0, 2.0], 8, 3, gpu_device)
    assert got[1].tolist() == [[3, 7, 0]]


def test_merge_ranks_a_rounding_tie_by_the_base_score(gpu_device):
    """Two scores one ulp apart whose products round to the same double: the larger base score first,
    although it has the larger row -- in one class and across two classes of equal weight."""
    w = 0.7
    x = next(x for x in (0.6 + 1e-3 * i for i in range(1000)) if w * x == w * np.nextafter(x, 1.0))
    scores = np.array([[x, np.nextafter(x, 1.0), 0.1]])
    got = check_merge(scores, np.array([1, 1, 0]), [1.0, w], 4, 3, gpu_device)
    assert got[1].tolist() == [[1, 0, 2]] and got[2][0, 0] == got[2][0, 1] and got[3][0, 0] > got[3][0, 1]
    got = check_merge(scores, np.array([0, 1, 2]), [w, w, 1.0], 4, 3, gpu_device)
    assert got[1].tolist() == [[1, 0, 2]]


# ---- 3. through the store ---------------------------------------------------------------------------------
N, D, NQ = 20_011, 384, 40
CLUSTER = 97
PERIODS = ["Q1_FY2024", "Q2_FY2024", "Q3_FY2024", "Q4_FY2024"]
_WORLD = {}


def world(device):
    """One store for the module: ~20 000 x 384 synth rows with a near-tie cluster scattered through them,
    scalar columns dealt so that every class of the boosts below has rows, and the fp64 scores of the
    40 queries (query 0 is the cluster's), computed once and never changed."""
    if not _WORLD:
        import torch
        from rag_fin_amd.store import CorpusStore
        qc, rows = adv.near_tie_cluster(D, CLUSTER, 0)
        c16, pos = adv.embed_clusters(N, D, 1234, [rows], stride=adv.scatter_stride(N, CLUSTER))
        q16 = np.concatenate([qc[None, :], osearch.synth_unit_rows(NQ - 1, D, 1235)])
        r = np.arange(N)
        cols = {"period": np.array(PERIODS)[r % 4], "chunk_type": np.array(["a", "b", "c"])[r % 3],
                "statement_type": np.array(["s0", "s1"])[(r // 5) % 2], "primary_value": (r % 1000).astype(np.float64)}
        npa = r % 7 == 0
        texts = ["gross npa ratio rose" if x else "net interest margin was stable" for x in npa]
        st = CorpusStore("boost", dim=D, capacity=N, device=device)
        st.add([f"k{i}" for i in r], texts, torch.from_numpy(c16).to(device), cols["period"].tolist(),
               cols["chunk_type"].tolist(), cols["statement_type"].tolist(), cols["primary_value"].tolist())
        st.create_index("sparse", {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"})
        scores = osearch.exact_scores(q16, c16)
        scores.setflags(write=False)
        _WORLD.update(st=st, q=torch.from_numpy(q16).to(device), scores=scores, cols=cols, npa=npa, pos=pos[0], c16=c16)
    return _WORLD


# filter expression -> the rows it selects, in numpy
def selectors(w):
    c = w["cols"]
    return {
        'period == "Q4_FY2024"': c["period"] == "Q4_FY2024",
        'chunk_type == "a"': c["chunk_type"] == "a",
        "primary_value < 500": c["primary_value"] < 500,
        'period == "Q9_FY2031"': np.zeros(N, dtype=bool),
        "primary_value >= 0": np.ones(N, dtype=bool),
        "primary_value == 3": c["primary_value"] == 3,
        'statement_type == "s1" and primary_value < 700': (c["statement_type"] == "s1") & (c["primary_value"] < 700),
        'TEXT_MATCH(text, "npa")': w["npa"],
    }


def check_store(device, boosts, B, limit, expr=None):
    w = world(device)
    sel = selectors(w)
    cls = np.zeros(N, dtype=np.int64)
    for i, b in enumerate(boosts):
        cls |= sel[b.filter].astype(np.int64) << i
    pass_mask = None if expr is None else sel[expr]
    want = boost_reference(w["scores"][:B], pass_mask, cls, class_weights(boosts), limit)
    res = w["st"].search(w["q"][:B], "embedding", COS, limit, expr=expr, ranker=boosts, output_fields=["period"])
    assert len(res) == B
    for b, hits in enumerate(res):
        live = want[1][b] >= 0
        assert [h.row for h in hits] == want[1][b][live].tolist(), (b, limit)
        assert [h.score for h in hits] == [float(x) for x in want[0][b][live]], (b, limit)
        assert [h.entity.period for h in hits] == w["cols"]["period"][want[1][b][live]].tolist()
    return cls, want, res


LATEST = 'period == "Q4_FY2024"'


@pytest.mark.parametrize("weight", [1.5, 0.5])
@pytest.mark.parametrize("B,limit", [(1, 10), (5, 1), (5, 64), (40, 10)])
def test_one_boost_promotes_or_demotes(gpu_device, B, limit, weight):
    cls, want, _ = check_store(gpu_device, [BoostRanker(LATEST, weight)], B, limit)
    assert set(cls.tolist()) == {0, 1}


def test_the_near_tie_cluster_straddles_two_classes(gpu_device):
    """Query 0 is the cluster's query: its 97 near-tied rows fall into both classes of the boost, and the
    cut at rank 64 falls inside the cluster for the boosted class and for the weight 1 call."""
    w = world(gpu_device)
    in_q4 = selectors(w)[LATEST][w["pos"]]
    assert in_q4.any() and not in_q4.all()
    for weight in (1.0, 1.0 + 2.0 ** -20, 1.5):
        _, want, _ = check_store(gpu_device, [BoostRanker(LATEST, weight)], 1, 64)
        assert np.isin(want[1][0], w["pos"]).all()


@pytest.mark.parametrize("B,limit", [(1, 64), (5, 10), (40, 1)])
def test_three_boosts_populate_all_eight_classes(gpu_device, B, limit):
    boosts = [BoostRanker(LATEST, 1.5), BoostRanker('chunk_type == "a"', 0.8), BoostRanker("primary_value < 500", 1.2)]
    cls, _, _ = check_store(gpu_device, boosts, B, limit)
    assert set(cls.tolist()) == set(range(8))


@pytest.mark.parametrize("limit", [10, 64])
def test_forty_queries_with_two_boosts_take_several_sweeps(gpu_device, limit):
    boosts = (BoostRanker(LATEST, 1.25), BoostRanker('chunk_type == "a"', 0.6))    # 160 virtual queries
    cls, _, _ = check_store(gpu_device, boosts, 40, limit)
    assert set(cls.tolist()) == {0, 1, 2, 3}


def test_a_boost_that_matches_no_row_and_one_that_matches_every_row(gpu_device):
    w = world(gpu_device)
    nothing, everything = BoostRanker('period == "Q9_FY2031"', 3.0), BoostRanker("primary_value >= 0", 0.75)
    _, _, res = check_store(gpu_device, [nothing], 5, 10)                          # one class: the plain search
    plain = w["st"].search(w["q"][:5], "embedding", COS, 10)
    assert [[(h.row, h.score) for h in hits] for hits in res] == [[(h.row, h.score) for h in hits] for hits in plain]
    check_store(gpu_device, [everything], 5, 10)                                   # one class: every score scaled
    cls, _, _ = check_store(gpu_device, [nothing, BoostRanker(LATEST, 2.0), everything], 5, 64)
    assert set(cls.tolist()) == {4, 6}


@pytest.mark.parametrize("limit", [10, 64])
def test_a_narrow_expr_brings_negative_cosines_into_the_top_k(gpu_device, limit):
    boosts = [BoostRanker(LATEST, 2.0), BoostRanker('chunk_type == "a"', 0.5)]
    _, want, res = check_store(gpu_device, boosts, 5, limit, expr="primary_value == 3")
    assert ((want[3] < 0) & (want[1] >= 0)).any(axis=1).all()                      # negative cosines in every list
    assert all(len(hits) == min(limit, 21) for hits in res)                         # rows 3, 1003, ..., 20003
    check_store(gpu_device, [BoostRanker(LATEST, 1.5)], 40, 10, expr='statement_type == "s1" and primary_value < 700')
    # an expr no row passes: empty lists
    st = world(gpu_device)["st"]
    assert st.search(world(gpu_device)["q"][:3], "embedding", COS, 5, expr='period == "Q9_FY2031"',
                     ranker=BoostRanker(LATEST, 2.0)) == [[], [], []]


def test_a_text_match_boost(gpu_device):
    cls, _, _ = check_store(gpu_device, [BoostRanker('TEXT_MATCH(text, "npa")', 2.0)], 5, 10)
    assert cls.sum() == (np.arange(N) % 7 == 0).sum()
    check_store(gpu_device, [BoostRanker('TEXT_MATCH(text, "npa")', 0.5), BoostRanker(LATEST, 1.5)], 5, 10,
                expr="primary_value < 500")


def test_weight_one_returns_the_ids_of_the_plain_search(gpu_device):
    w = world(gpu_device)
    for expr in (None, "primary_value < 500"):
        plain = w["st"].search(w["q"], "embedding", COS, 10, expr=expr)
        boosted = w["st"].search(w["q"], "embedding", COS, 10, expr=expr, ranker=[BoostRanker(LATEST, 1.0)])
        assert [[h.row for h in hits] for hits in boosted] == [[h.row for h in hits] for hits in plain]
        assert [[h.score for h in hits] for hits in boosted] == [[h.score for h in hits] for hits in plain]


def test_the_same_boosted_search_twice_is_bit_identical(gpu_device):
    w = world(gpu_device)
    boosts = [BoostRanker(LATEST, 1.5), BoostRanker('chunk_type == "a"', 0.8)]
    a = w["st"].search(w["q"][:5], "embedding", COS, 10, ranker=boosts)
    b = w["st"].search(w["q"][:5], "embedding", COS, 10, ranker=boosts)
    assert [[(h.row, h.score) for h in hits] for hits in a] == [[(h.row, h.score) for h in hits] for hits in b]


def test_an_sq8_collection_answers_from_its_fp16_rows(gpu_device):
    import torch
    from rag_fin_amd.store import CorpusStore
    n = 9_001
    c16 = osearch.synth_unit_rows(n, D, 77)
    q16 = osearch.synth_unit_rows(3, D, 78)
    r = np.arange(n)
    st = CorpusStore("boost8", dim=D, capacity=n, device=gpu_device)
    st.add([f"k{i}" for i in r], ["t"] * n, torch.from_numpy(c16).to(gpu_device), np.array(PERIODS)[r % 4].tolist(),
           ["a"] * n, ["s"] * n, [0.0] * n)
    st.create_index("embedding", {"index_type": "SQ8", "metric_type": "COSINE"})
    want = boost_reference(osearch.exact_scores(q16, c16), None, (r % 4 == 3).astype(np.int64), [1.0, 1.5], 10)
    res = st.search(torch.from_numpy(q16).to(gpu_device), "embedding", COS, 10, ranker=BoostRanker(LATEST, 1.5))
    for b, hits in enumerate(res):
        assert [h.row for h in hits] == want[1][b].tolist()
        assert [h.score for h in hits] == [float(x) for x in want[0][b]]


def test_vector_rag_search_with_a_boost(gpu_device):
    from rag_fin_amd.rag import VectorRAG
    w = world(gpu_device)

    class Emb:
        def encode_to_device(self, texts):
            return w["q"][1:1 + len(texts)]

    rag = VectorRAG("no-key", "boost", embedder=Emb(), store=w["st"])
    got = rag.search("what is the net interest margin", 5, boost={"filter": LATEST, "weight": 1.5})
    cls = selectors(w)[LATEST].astype(np.int64)
    want = boost_reference(w["scores"][1:2], None, cls, [1.0, 1.5], 5)
    assert [set(c) for c in got] == [{"rank", "text", "period", "chunk_type", "statement_type", "primary_value",
                                      "score"}] * 5
    assert [c["rank"] for c in got] == [1, 2, 3, 4, 5]
    assert [c["score"] for c in got] == [float(x) for x in want[0][0]]              # the boosted score
    assert [c["period"] for c in got] == w["cols"]["period"][want[1][0]].tolist()
    batch = rag.search_batch(["a", "b"], 3, expr="primary_value < 500", boost=[{"filter": LATEST, "weight": 1.5}])
    want = boost_reference(w["scores"][1:3], selectors(w)["primary_value < 500"], cls, [1.0, 1.5], 3)
    assert [[c["score"] for c in ctx] for ctx in batch] == [[float(x) for x in row] for row in want[0]]
